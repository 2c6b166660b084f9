"""The kernel autotuner every hot layer dispatches through: a table from a
shape key to the chosen ``(impl, cfg, grid/splits)`` tag.

For every distinct key the first call times the caller's candidates -- the
HIP kernel configurations *and* the vendor library (MIOpen / hipBLASLt) --
with HIP events and keeps the fastest (``pick``; ``GKSGD_GEMM_TUNE=0`` skips
the search and takes the first candidate that runs).  The table is seeded
from ``tuning/gemm_choices.json`` (``GKSGD_GEMM_CACHE``).  Also here, because
every GEMM caller shares them: the fp32 matmul mode (``set_f32_matmul``) and
the candidate kernel configurations with the key suffix that goes with them
(``nt_cfgs``, ``tn_cfgs``, ``splitk_cfgs``, ``dkey``).

The table, the search log, ``_TUNE`` and the fp32 mode are this module's
globals and are reached only through it (``autotune.pick``,
``autotune.choice``, ``autotune.f32_matmul()``): no other module binds them,
so patching them here (tests) takes effect for every caller.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, Iterable, List, Optional, Tuple

import torch

_TUNE = os.environ.get("GKSGD_GEMM_TUNE", "1") != "0"
_choices: Dict[tuple, tuple] = {}
# candidates that are this package's own kernels; a vendor-library choice
# (MIOpen / hipBLASLt) has to beat the best of them by more than this fraction
# of its time (GKSGD_GK_MARGIN, default 5%: the fp32 implicit-GEMM kernels
# trail MIOpen's by 1-5% on some 3x3 shapes -- kept, so the fp32 step runs on
# code this package owns; 0 = fastest wins)
_OWN = ("hip", "w3", "mat", "wino", "wx6")
_GK_MARGIN = float(os.environ.get("GKSGD_GK_MARGIN", "0.05"))
_timings: Dict[tuple, list] = {}      # key -> [(tag, ms or error)] of the search
# candidate kernel configurations: the digits of a cfg word are fields, see csrc/kernels/gemm_cfg.h
_NT_CFGS = [1, 2, 3, 4, 11, 13, 21, 22, 23, 24, 111, 113, 121, 122, 123, 124, 25, 26, 27, 125, 126, 127,
            211, 212, 213, 214, 221, 222, 223, 224]   # 2xx: four LDS stages (more bytes in flight)
# grid override: 0 = persistent (about two blocks per CU), else a fixed block count
NT_GRIDS = (0, 512, 1 << 20)
_TN_CFGS = [(c, s) for c in (1, 2, 3, 4, 5, 6, 7, 8, 21, 22, 23, 24, 27, 9, 29, 101, 121, 102, 122) for s in (0, 128)]
# fp32: 64x64 wave tiles (NT tiles 5-7 map onto them) and, cfg + 1000, 32x64 wave tiles
# (twice the waves: the small-M layers of small batches, e.g. the reference's bs32)
_NT_CFGS_F32 = [1, 2, 3, 4, 7, 11, 12, 13, 14, 21, 22, 23, 24, 101, 102, 103, 104, 201, 202, 203, 204,
                1001, 1002, 1003, 1004, 1005, 1006, 1007, 1021, 1022, 1101, 1102, 1103]
_TN_CFGS_F32 = [(c, s) for c in (1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15, 16) for s in (0, 64)]
# grad-weight of small-batch layers (pixel rows <= _TN_SMALL_M, e.g. ResNet-50 bs32): the default split
# count (two rounds of block slots) trades partial-sum atomics against idle CUs; these let the tuner pick
_TN_SMALL_M = 1 << 17
_TN_SMALL_F32 = [(c, s) for c in (4, 5, 11, 14, 15) for s in (16, 32, 128)]


# fp32 matmul algorithm (GKSGD_F32_MATMUL / set_f32_matmul):
#   "native" -- fp32 operands on v_mfma_f32_16x16x4_f32 only;
#   "bf16x6" -- the fp32 GEMM / implicit-GEMM candidates also include the bf16x6
#   kernels (gemm_nt.h / gemm_tn_f32.h X6, cfg digit 100000): every fp32 operand split exactly
#   into three bf16 parts, the six part products of order <= 2 accumulated in
#   fp32 on v_mfma_f32_16x16x32_bf16 -- measured MORE accurate than the fp32
#   MFMA against an fp64 reference on every ResNet-50 / BERT shape
#   (bench/x6_probe.py, profiles/r05_x6_probe.json), so it is an fp32 algorithm,
#   not a reduced precision; the tuner picks the faster kernel per shape.
X6 = 100000
_NT_CFGS_X6 = [c + X6 for c in (1, 2, 3, 4, 5, 6, 7, 12, 13, 101, 102, 103, 104, 105, 106, 107, 202, 203, 1001, 1002, 1003)]
# register-staged bf16x6 row GEMMs (gemm_nt_x62.h gemm_nt_x62_kernel, cfg digit 200000; tiles 1-7):
# plain row GEMMs only -- an implicit-GEMM / lazy / split-K call refuses them and the tuner moves on.
# Digit 300000: the same kernels with B split into bf16 planes once per call by the binding
# (split3_rows), no B split in the kernel: within +-3% of 200000, up to 8% faster on a few shapes (r5c33)
_NT_CFGS_X62 = [2 * X6 + t for t in range(1, 8)] + [3 * X6 + t for t in range(1, 8)]
# default bf16x6: the library, the trainers (dist_trainer --f32-matmul) and
# bench.py all run the same fp32 GEMM family unless told otherwise
_F32MM = os.environ.get("GKSGD_F32_MATMUL", "bf16x6")


def set_f32_matmul(mode: str) -> str:
    """Select the fp32 matmul algorithm ("native" or "bf16x6"); returns the
    previous one.  Autotune keys carry the mode, so each mode is tuned once."""
    global _F32MM
    if mode not in ("native", "bf16x6"):
        raise ValueError("f32 matmul mode must be 'native' or 'bf16x6', got %r" % (mode,))
    prev, _F32MM = _F32MM, mode
    return prev


def f32_matmul() -> str:
    return _F32MM


def _x6() -> bool:
    return _F32MM == "bf16x6"


# register-staged bf16x6 grad-weight (gemm_tn_x62.h gemm_tn_x62_kernel, cfg digit 200000; tiles 1-8):
# plain row form only -- an implicit-GEMM / lazy call refuses them and the tuner moves on
_TN_CFGS_X62 = [(2 * X6 + t, sp) for t in (1, 2, 3, 4, 5, 6, 7, 8) for sp in (0, 64)]


def tn_cfgs(dt: torch.dtype) -> List[Tuple[int, int]]:
    if dt == torch.float32:
        # (_TN_CFGS_X62 measured no faster than the LDS-DMA bf16x6 grad-weight on any ResNet-50 /
        # BERT shape, r5c27: not offered by default, GKSGD_TN_X62=1 adds them)
        extra = _TN_CFGS_X62 if os.environ.get("GKSGD_TN_X62", "0") == "1" else []
        return _TN_CFGS_F32 + ([(c + X6, sp) for c, sp in _TN_CFGS_F32] + extra if _x6() else [])
    return _TN_CFGS


def tn_small_cfgs(dt: torch.dtype, rows: int) -> List[Tuple[int, int]]:
    """Further grad-weight candidates of a small-batch fp32 layer (``rows``:
    its pixel rows), offered after ``tn_cfgs``."""
    if dt != torch.float32 or rows > _TN_SMALL_M:
        return []
    return _TN_SMALL_F32 + ([(c + X6, sp) for c, sp in _TN_SMALL_F32] if _x6() else [])


def nt_cfgs(dt: torch.dtype) -> List[int]:
    if dt == torch.float32:
        return _NT_CFGS_F32 + (_NT_CFGS_X6 + _NT_CFGS_X62 if _x6() else [])
    return _NT_CFGS


# fp32 split-K (cfg + 10000 S: S fp32 partial planes over K slices, then one
# reduce pass with the fused epilogue -- gemm.hip nt_splitk_reduce_kernel) for
# row GEMMs whose output tiles cannot fill 256 CUs over a deep K: the 1x1
# convolutions of stages 3-4 at the reference's batch 32 (M = 1568, N = 512,
# K = 2048 is 52 tiles of 128x128).
_SPLITK_BASE = (4, 1, 1001, 1002, 1003)
_SPLITK_MAX_OUT = 1 << 22
SPLITK_GRIDS = (0, 1 << 20)


def splitk_cfgs(dt: torch.dtype, M: int, N: int, K: int) -> List[int]:
    """Split-K candidate configs of an [M, K] x [N, K]^T fp32 GEMM (empty when
    its output alone fills the chip)."""
    if dt != torch.float32 or M * N > _SPLITK_MAX_OUT:
        return []
    base = list(_SPLITK_BASE) + ([c + X6 for c in _SPLITK_BASE] if _x6() else [])
    return [c + 10000 * S for S in (2, 4, 8) if K % (64 * S) == 0 and K // S >= 128 for c in base]


def nt_x62_cfgs() -> List[int]:
    """The register-staged bf16x6 row-GEMM configurations alone (fp32, bf16x6 mode)."""
    return list(_NT_CFGS_X62)


# (the implicit-GEMM convolutions split the same way over their (tap, channel)
# K slices: conv_nt with cfg + 10000 S)


def dkey(dt: torch.dtype) -> tuple:
    """Autotune key suffix: fp32 keys are tagged, bf16 keys keep their
    round-2 form so the shipped tuning cache stays valid."""
    if dt == torch.float32:
        return ("f32", "x6") if _x6() else ("f32",)
    return ()


def hip_cands(run: Callable[[int, int], object], pairs: Iterable[Tuple[int, int]]) -> list:
    """One ``(("hip", cfg, g), closure)`` candidate per ``(cfg, g)`` pair, in
    the pairs' order (g: the grid override of an NT kernel, the split count of
    a TN one); the closure calls ``run(cfg, g)``."""
    return [(("hip", c, g), (lambda c=c, g=g: run(c, g))) for c, g in pairs]


def _time(fn: Callable[[], None], reps: int = 5) -> float:
    fn()
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def choice(key: tuple) -> Optional[tuple]:
    """The tag already chosen for ``key`` (None: not tuned yet); never searches."""
    return _choices.get(key)


def pick(key: tuple, cands: List[Tuple[tuple, Callable[[], None]]]) -> tuple:
    """Fastest candidate for ``key`` (timed once per process, then cached):
    a 3-repetition screen of every candidate, then the best four re-timed
    with 12 repetitions (one noisy sample must not decide)."""
    got = _choices.get(key)
    if got is not None:
        return got
    if len(cands) == 1:
        _choices[key] = cands[0][0]
        return cands[0][0]
    if not _TUNE:
        # untuned: the first candidate that runs (a lazy-operand tile may refuse its LDS budget)
        for tag, fn in cands:
            try:
                fn()
            except RuntimeError:
                continue
            _choices[key] = tag
            return tag
        raise RuntimeError("no candidate ran for %s" % (key,))
    log = _timings.setdefault(key, [])
    screened = []
    for tag, fn in cands:
        try:
            t = _time(fn, reps=3)
        except RuntimeError as e:
            log.append((tag, "error: %s" % str(e).splitlines()[0][:200]))
            continue
        screened.append((t, tag, fn))
    screened.sort(key=lambda e: e[0])
    best, best_t = cands[-1][0], float("inf")
    timed = []
    for _, tag, fn in screened[:4]:
        t = _time(fn, reps=12)
        log.append((tag, round(t, 4)))
        timed.append((t, tag))
        if t < best_t:
            best, best_t = tag, t
    if best[0] not in _OWN and _GK_MARGIN > 0:
        # keep the hand-written kernel unless the vendor library is clearly faster
        own = [(t, tag) for t, tag in timed if tag[0] in _OWN]
        if own and min(own)[0] <= best_t * (1.0 + _GK_MARGIN):
            best = min(own)[1]
            log.append((best, "kept: within GKSGD_GK_MARGIN of %s" % (best_t,)))
    _choices[key] = best
    return best


def tuning_log() -> Dict[tuple, list]:
    """Per key, every candidate's measured ms (or its error) from the search."""
    return dict(_timings)


def load_choices(path: str) -> int:
    """Seed the autotune cache from a JSON file written by save_choices()."""
    import json
    try:
        with open(path) as f:
            rows = json.load(f)
    except (OSError, ValueError):
        return 0
    for k, v in rows:
        _choices.setdefault(tuple(k), tuple(v))
    return len(rows)


def save_choices(path: str) -> None:
    import json
    with open(path, "w") as f:
        json.dump([[list(k), list(v)] for k, v in sorted(_choices.items(), key=str)], f, indent=0)


_CACHE = os.environ.get("GKSGD_GEMM_CACHE", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__)))), "tuning", "gemm_choices.json"))
if _TUNE and _CACHE and os.path.exists(_CACHE) and os.environ.get("GKSGD_GEMM_RETUNE", "0") == "0":
    load_choices(_CACHE)
    # GKSGD_GEMM_RETUNE_ONLY=dgrad_bn,...: retune only the keys of these directions
    _only = {d for d in os.environ.get("GKSGD_GEMM_RETUNE_ONLY", "").split(",") if d}
    if _only:
        for _k in [k for k in _choices if k and k[0] in _only]:
            del _choices[_k]


def tuned_choices() -> Dict[tuple, tuple]:
    """(direction, geometry...) -> chosen (impl, cfg, grid/splits)."""
    return dict(_choices)
