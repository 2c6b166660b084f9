"""ops/build.py keys every object's cache on its source plus the files the
source's quoted #include lines reach (no compiler, no GPU): the GEMM units see
only their own kernel family's header, and editing a header rebuilds exactly
the sources that include it."""
import shutil

import pytest

from gaussiank_sgd_amd.ops import build

FAMILIES = {"gemm_nt.h", "gemm_tn.h", "gemm_tn_f32.h", "gemm_nt_x62.h", "gemm_tn_x62.h"}
SOURCES = build.HIP_SOURCES + build.CXX_SOURCES


def _reached(src_rel):
    """Paths relative to csrc/ of everything `src_rel` reaches, itself excluded."""
    src = build.CSRC / src_rel
    return {p.relative_to(build.CSRC).as_posix() for p in build._closure(src) if p != src}


def _digests():
    return {s: build._digest(build.CSRC / s.partition("#")[0], ["-O3"]) for s in SOURCES}


@pytest.fixture
def csrc_copy(tmp_path, monkeypatch):
    dst = tmp_path / "csrc"
    shutil.copytree(build.CSRC, dst)
    monkeypatch.setattr(build, "CSRC", dst)
    return dst


@pytest.mark.parametrize("src,family", [
    ("gemm_inst_nt.hip", {"gemm_nt.h"}),
    ("gemm_inst_tn.hip", {"gemm_tn.h", "gemm_tn_f32.h"}),
    ("gemm_inst_nt_x62.hip", {"gemm_nt_x62.h"}),
    ("gemm_inst_tn_x62.hip", {"gemm_tn_x62.h"}),
    ("gemm.hip", set()),
])
def test_gemm_sources_reach_their_own_family_only(src, family):
    names = {r.rpartition("/")[2] for r in _reached("kernels/" + src)}
    assert names & FAMILIES == family
    assert {"gemm_units.h", "gemm_cfg.h"} <= names
    assert ("gemm_common.h" in names) == bool(family)


def test_bindings_closure():
    assert _reached("bindings.cpp") == {"comm/rccl_engine.h", "kernels/gemm_cfg.h", "kernels/gk_kernels.h"}


def test_sources_are_listed_once_and_every_unit_has_a_family():
    assert len(set(SOURCES)) == len(SOURCES)
    units = sorted(int(s.partition("#")[2]) for s in build.HIP_SOURCES if "#" in s)
    assert units == list(range(11))
    assert "kernels/gemm_inst_tn_x62.hip#9" in build.HIP_SOURCES
    for s in build.HIP_SOURCES:
        if "gemm_inst" in s:
            assert build.EXTRA_FLAGS[s.partition("#")[0]] == ["-fno-slp-vectorize"]


def test_every_quoted_include_resolves():
    for p in sorted(build.CSRC.rglob("*")):
        if p.suffix in (".h", ".hip", ".cpp"):
            assert p in build._closure(p)


def test_unresolvable_include_raises(csrc_copy):
    with open(csrc_copy / "kernels" / "gemm_units.h", "a") as f:
        f.write('#include "no_such_header.h"\n')
    with pytest.raises(FileNotFoundError, match="no_such_header.h"):
        build._digest(csrc_copy / "kernels" / "gemm.hip", [])


def test_family_header_edit_changes_one_digest(csrc_copy):
    before = _digests()
    with open(csrc_copy / "kernels" / "gemm_tn_x62.h", "a") as f:
        f.write("\n")
    after = _digests()
    assert {s for s in SOURCES if before[s] != after[s]} == {"kernels/gemm_inst_tn_x62.hip#9"}


def test_shared_header_edit_changes_every_includer(csrc_copy):
    includers = {s for s in SOURCES if "kernels/gk_kernels.h" in _reached(s.partition("#")[0])}
    assert "bindings.cpp" in includers and "comm/rccl_engine.cpp" not in includers
    assert includers >= set(build.HIP_SOURCES)
    before = _digests()
    with open(csrc_copy / "kernels" / "gk_kernels.h", "a") as f:
        f.write("\n")
    after = _digests()
    assert {s for s in SOURCES if before[s] != after[s]} == includers


def test_flags_are_part_of_the_digest():
    src = build.CSRC / "kernels" / "gemm.hip"
    assert build._digest(src, ["-O3"]) != build._digest(src, ["-O2"])
