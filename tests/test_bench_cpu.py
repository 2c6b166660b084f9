"""bench.py's fail-soft phase runner and defaults, on CPU (no GPU needed)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("gk_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_optional_phase_records_error(bench, monkeypatch):
    out = {}

    def boom(holder):
        raise ValueError("bad shape\nsecond line")
    assert bench.optional_phase("dense", out, 1, boom) is True     # ranks can still agree: go on
    assert out["dense_error"] == "ValueError: bad shape"


def test_optional_phase_injection_and_success(bench, monkeypatch):
    out = {}
    ran = []
    monkeypatch.setenv("GKSGD_BENCH_FAIL_PHASE", "bf16")
    assert bench.optional_phase("bf16", out, 1, lambda h: ran.append(1)) is True
    assert "injected failure" in out["bf16_error"] and not ran
    assert bench.optional_phase("ref_bs32", out, 1, lambda h: ran.append(1)) is True
    assert ran == [1] and "ref_bs32_error" not in out


def test_reference_batches_and_bert_buckets(bench):
    # the reference's per-worker batches (/root/reference/exp_configs/*.conf:2)
    assert bench.REF_BATCH["resnet50"] == 32 and bench.REF_BATCH["vgg16"] == 128 and bench.REF_BATCH["lstm"] == 20
    # BERT: bucketed compression (~25 MB fp32 buckets) by default
    assert bench.DEFAULT_THRESHOLD["bert"] * 4 == pytest.approx(26e6, rel=0.1)


def test_plain_run_is_the_default_and_full_is_opt_in(bench, monkeypatch):
    import sys
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_sample_is_whole_below_the_cap_and_a_fixed_sample_above(bench):
    import torch
    t = torch.arange(1000, dtype=torch.float32)
    assert torch.equal(bench.dump_sample(t.view(10, 100), max_elems=1000), t)      # whole, flattened
    s1 = bench.dump_sample(t, max_elems=64)
    s2 = bench.dump_sample(t.clone(), max_elems=64)
    assert s1.numel() == 64 and torch.equal(s1, s2)                                # same positions every time
    assert torch.equal(s1, s1.sort().values) and 0 <= s1.min() and s1.max() < 1000  # values are the positions here
    assert s1.unique().numel() > 32                                                # spread, not one spot
    # all --dump-outputs arrays together stay below 64 MB
    assert 4 * bench.DUMP_MAX_ELEMS * 4 + 8 <= 64 * 10 ** 6


def test_dump_outputs_writes_float_npy(bench, tmp_path):
    import types
    import numpy as np
    import torch
    arena = types.SimpleNamespace(weights=torch.arange(6, dtype=torch.float32), momentum=None,
                                  residuals=torch.ones(6))
    ph = types.SimpleNamespace(opt=types.SimpleNamespace(arena=arena))
    written = bench.dump_outputs(str(tmp_path / "o"), ph, 2.5)
    assert written == {"loss": 1, "weights": 6, "residuals": 6}        # no momentum arena: no file
    assert sorted(p.name for p in (tmp_path / "o").iterdir()) == ["loss.npy", "residuals.npy", "weights.npy"]
    loss, w = np.load(tmp_path / "o" / "loss.npy"), np.load(tmp_path / "o" / "weights.npy")
    assert loss.dtype == np.float64 and loss.tolist() == [2.5]
    assert w.dtype == np.float32 and w.tolist() == [0, 1, 2, 3, 4, 5]


def test_snapshot_and_restore_state_put_the_training_state_back_in_place(bench):
    """The dump step starts from the state before the warm-up: arenas and
    buffers restored in place, an arena born later zeroed, LSTM hidden state dropped."""
    import types
    import torch
    net = torch.nn.BatchNorm1d(3)
    arena = types.SimpleNamespace(weights=torch.arange(4.0), residuals=torch.zeros(4), velocity=torch.zeros(4),
                                  momentum=None)
    refreshed = []
    opt = types.SimpleNamespace(arena=arena, refresh_shadow=lambda: refreshed.append(1))
    ph = types.SimpleNamespace(opt=opt, trainer=types.SimpleNamespace(net=net), state={"hidden": "h"})
    snap = bench.snapshot_state(ph)
    assert sorted(snap["arenas"]) == ["residuals", "velocity", "weights"] and "running_mean" in snap["buffers"]
    w_ptr = arena.weights.data_ptr()
    arena.weights += 1.0
    arena.residuals += 2.0
    arena.velocity += 3.0
    arena.momentum = torch.ones(4)          # created by the first step
    net.running_mean += 5.0
    bench.restore_state(ph, snap)
    assert arena.weights.data_ptr() == w_ptr and arena.weights.tolist() == [0, 1, 2, 3]
    assert not arena.residuals.any() and not arena.velocity.any() and not arena.momentum.any()
    assert not net.running_mean.any() and refreshed == [1] and ph.state["hidden"] is None


def test_miopen_user_db_is_a_working_copy_with_fallbacks(bench, tmp_path, monkeypatch):
    """MIOpen gets a copy of tuning/miopen, not the tracked files; where the
    checkout's own build/ cannot be written the copy goes to the temporary
    directory, and failing that the committed directory is used read-only."""
    from tuning import miopen_db
    committed = sorted(os.listdir(miopen_db.COMMITTED))
    assert committed and os.path.dirname(miopen_db.WORKING) == os.path.join(ROOT, "build")
    w = miopen_db.user_db_path(str(tmp_path / "w"))
    assert w == str(tmp_path / "w") and sorted(os.listdir(w)) == committed
    # what MIOpen wrote since is kept
    first = os.path.join(w, committed[0])
    with open(first, "a") as f:
        f.write("learnt\n")
    miopen_db.user_db_path(w)
    assert open(first).read().endswith("learnt\n")
    # unusable working directory (its parent is a file): per-user copy under the temporary directory
    blocker = tmp_path / "file"
    blocker.write_text("x")
    monkeypatch.setattr(miopen_db.tempfile, "tempdir", str(tmp_path / "tmp"))
    t = miopen_db.user_db_path(str(blocker / "db"))
    assert t.startswith(str(tmp_path / "tmp")) and sorted(os.listdir(t)) == committed
    # neither can be written: the committed directory itself
    monkeypatch.setattr(miopen_db, "_fallback", lambda: str(blocker / "other"))
    assert miopen_db.user_db_path(str(blocker / "db")) == miopen_db.COMMITTED


def test_bert_default_threshold_gives_buckets(bench):
    """The BERT default threshold splits the 110 M gradients into >= 4 buckets
    (reference grouping rule: reverse registration order until >= threshold)."""
    import torch
    from gaussiank_sgd_amd.models.bert import bert_base
    from gaussiank_sgd_amd.parallel.buckets import group_with_threshold
    with torch.device("meta"):
        net = bert_base()
    names = [n for n, p in net.named_parameters()]
    sizes = {n: p.numel() for n, p in net.named_parameters()}
    groups = group_with_threshold(names, sizes, bench.DEFAULT_THRESHOLD["bert"])
    assert len(groups) >= 4


def _asym_worker(rank, port, outdir):
    """Rank 1 fails the phase (GKSGD_BENCH_FAIL_PHASE_RANK) while rank 0 waits
    in the phase's own point-to-point exchange for it: the agreement
    collective cannot pair up, so only the phase deadline ends the run."""
    import time
    import torch
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2",
                      LOCAL_RANK=str(rank), GKSGD_BENCH_FAIL_PHASE="dense", GKSGD_BENCH_FAIL_PHASE_RANK="1",
                      GKSGD_BENCH_PHASE_TIMEOUT_S="3")
    spec = importlib.util.spec_from_file_location("gk_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from gaussiank_sgd_amd.parallel import comm
    comm.init(device="cpu")
    bench._EMIT["json_out"] = os.path.join(outdir, "line.json")
    out = {"metric": "m", "value": 1.0}

    def phase(holder):
        t = torch.zeros(1)
        torch.distributed.recv(t, src=1)     # rank 1 never sends: it failed before
    t0 = time.time()
    bench.optional_phase("dense", out, 2, phase)
    # not reached when the deadline fired (os._exit); reached only if the ranks agreed
    with open(os.path.join(outdir, "returned%d" % rank), "w") as f:
        f.write("%.1f" % (time.time() - t0))


def test_asymmetric_phase_failure_keeps_the_headline_line():
    import json
    import socket
    import tempfile
    import time
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    with tempfile.TemporaryDirectory() as d:
        t0 = time.time()
        mp.spawn(_asym_worker, args=(port, d), nprocs=2, join=True)
        assert time.time() - t0 < 60
        line = json.loads(open(os.path.join(d, "line.json")).read())
        assert line["value"] == 1.0 and "timeout" in line["dense_error"], line
        assert not os.path.exists(os.path.join(d, "returned0"))


def test_per_rank_injection(bench, monkeypatch):
    monkeypatch.setenv("GKSGD_BENCH_FAIL_PHASE", "bf16")
    monkeypatch.setenv("GKSGD_BENCH_FAIL_PHASE_RANK", "1")
    assert not bench._injected("bf16")          # this process is rank 0
    monkeypatch.setenv("GKSGD_BENCH_FAIL_PHASE_RANK", "0")
    assert bench._injected("bf16") and not bench._injected("dense")
