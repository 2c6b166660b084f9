"""The GEMM configuration word (ops/csrc/kernels/gemm_cfg.h) on the CPU: which
kernel instantiation, stage / panel request, unit, split-K plan or refusal a
word means for a call form and shape.

tests/golden/gemm_dispatch.json was recorded from the dispatchers as they were
before gemm_cfg.h existed (each launcher logging its template arguments in
place of launching); tests/gemm_cfg_dump.cpp runs the same sweep through
gemm_cfg.h and has to print the same rows.  The table is the yardstick, so it
is never regenerated from gemm_cfg.h: rows for a new word are written by hand
from the behaviour the word is meant to have.

Sweep: every word of the table as a bf16 and an fp32 call, through gemm_nt, conv_nt,
conv_nt_remap, gemm_tn_acc and conv_tn_acc, with and without the BN-backward
epilogue, the lazy operand (fp32) and the pre-split B operand (families 2 and
3), one tap (C = K), four taps (C = K / 4: 16, 32, 48, 64, 512) and, for the
register-staged kernels, an input past the 2^31 element offsets; N and K as
listed in the table.

What this pins is gemm_cfg.h's pure functions.  The dump program composes them
with its own copy of the few lines around them in gemm.hip (nt_run / tn_run:
no BN epilogue on split-K planes, no lazy operand for bf16, remap from the
entry point, a workspace whenever planes are asked for), so a mistake in that
composition shows only in the GPU GEMM tests (tests/test_gemm*_gpu.py)."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaussiank_sgd_amd.ops import autotune as cv  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
X6 = cv.X6


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "gemm_dispatch.json")) as f:
        return json.load(f)


def test_table_covers_the_tuner_and_the_shipped_choices(golden):
    words = {w[0] for w in golden["words"]}
    want = set(cv._NT_CFGS) | set(cv._NT_CFGS_F32) | set(cv._NT_CFGS_X6) | set(cv._NT_CFGS_X62)
    for lst in (cv._TN_CFGS, cv._TN_CFGS_F32, cv._TN_SMALL_F32, cv._TN_CFGS_X62):
        want |= {c for c, _ in lst}
    base = list(cv._SPLITK_BASE) + [c + X6 for c in cv._SPLITK_BASE]
    want |= {c + 10000 * S for S in (2, 4, 8) for c in base}
    with open(os.path.join(ROOT, "tuning", "gemm_choices.json")) as f:
        want |= {int(v[1]) for _, v in json.load(f) if v[0] == "hip"}
    want |= {0, 8, 9, 10, 30, 1008, 130, 300001, 400001}   # out-of-range digits
    # every word also with its product family stripped and as bf16x6
    want |= {c % X6 for c in want} | {c % X6 + X6 for c in want}
    assert want <= words, sorted(want - words)


@pytest.mark.skipif(CXX is None, reason="no C++ compiler on the path")
def test_dispatch_matches_the_recorded_table(golden, tmp_path):
    exe = str(tmp_path / "gemm_cfg_dump")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Wextra",
                    "-I" + os.path.join(ROOT, "gaussiank_sgd_amd", "ops", "csrc", "kernels"),
                    os.path.join(HERE, "gemm_cfg_dump.cpp"), "-o", exe], check=True)
    words = tmp_path / "words.txt"
    words.write_text(" ".join(str(w[0]) for w in golden["words"]))
    got = subprocess.run([exe, str(words)], check=True, capture_output=True, text=True).stdout.splitlines()
    results = [" ".join(map(str, r)) for r in golden["results"]]
    want = []
    for cfg, sweep, *patterns in golden["words"]:
        calls = golden["sweeps"][sweep]
        assert len(calls) == len(patterns)
        for call, pattern in zip(calls, patterns):
            head = " ".join(map(str, call + [cfg]))
            for n, row in zip(golden["N"], golden["patterns"][pattern]):
                want += ["%s %d %d %s" % (head, n, k, results[r]) for k, r in zip(golden["K"], golden["rows"][row])]
    assert len(got) == len(want)
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, "%d rows differ, first (recorded, now): %s" % (len(bad), bad[:3])
