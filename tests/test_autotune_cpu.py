"""The kernel autotuner (ops/autotune.py) on the CPU.

* The decision rule of ``autotune.pick`` against fake candidates and a
  scripted ``_time``: cache hit, single candidate, untuned first-that-runs,
  the 3-repetition screen, the 12-repetition re-timing of the best four, error
  logging, the GKSGD_GK_MARGIN rule, and the save / load round trip.
* The dispatch trace: which keys and which candidate tags, in which order,
  every convolution and linear direction hands to ``pick``, and which op runs
  for the returned tag -- against ``tests/golden/autotune_trace.json``,
  recorded once from the tree before the tuner moved out of ops/conv1x1.py
  (``python tests/test_autotune_cpu.py OUT.json`` writes the trace of the
  tree it runs in).
"""
import json
import os
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaussiank_sgd_amd.ops import autotune, conv1x1, linear, weight_prep  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "autotune_trace.json")


# ---------------------------------------------------------------- decision rule
class Fake:
    """A candidate: counts its calls; ``err`` makes it raise RuntimeError."""

    def __init__(self, screen=None, final=None, err=None):
        self.calls, self.times, self.err = 0, {3: screen, 12: final}, err

    def __call__(self):
        self.calls += 1
        if self.err is not None:
            raise RuntimeError(self.err)


@pytest.fixture
def tuner(monkeypatch):
    """An empty table with tuning on, the default margin, and ``_time``
    replaced by a stub that runs the candidate once, records (candidate,
    reps) and returns the candidate's scripted time for that reps."""
    timed = []

    def fake_time(fn, reps=5):
        timed.append((fn, reps))
        fn()
        return fn.times[reps]
    monkeypatch.setattr(autotune, "_choices", {})
    monkeypatch.setattr(autotune, "_timings", {})
    monkeypatch.setattr(autotune, "_TUNE", True)
    monkeypatch.setattr(autotune, "_GK_MARGIN", 0.05)
    monkeypatch.setattr(autotune, "_time", fake_time)
    return timed


def test_cached_key_calls_nothing(tuner):
    autotune._choices[("k",)] = ("hip", 7, 0)
    a, b = Fake(1.0, 1.0), Fake(2.0, 2.0)
    assert autotune.pick(("k",), [(("hip", 1, 0), a), (("blas", 0, 0), b)]) == ("hip", 7, 0)
    assert a.calls == b.calls == 0 and tuner == []
    assert autotune.choice(("k",)) == ("hip", 7, 0) and autotune.choice(("other",)) is None


def test_single_candidate_is_not_run(tuner):
    a = Fake(err="would fail")
    assert autotune.pick(("k",), [(("hip", 3, 512), a)]) == ("hip", 3, 512)
    assert a.calls == 0 and tuner == []
    assert autotune.tuned_choices() == {("k",): ("hip", 3, 512)}


def test_untuned_takes_the_first_candidate_that_runs(tuner, monkeypatch):
    monkeypatch.setattr(autotune, "_TUNE", False)
    a, b, c = Fake(err="no LDS"), Fake(), Fake()
    cands = [(("hip", 1, 0), a), (("hip", 2, 0), b), (("blas", 0, 0), c)]
    assert autotune.pick(("k",), cands) == ("hip", 2, 0)
    assert (a.calls, b.calls, c.calls) == (1, 1, 0) and tuner == []
    assert autotune.choice(("k",)) == ("hip", 2, 0) and autotune.tuning_log() == {}
    with pytest.raises(RuntimeError, match="no candidate ran"):
        autotune.pick(("k2",), [(("hip", 1, 0), Fake(err="x")), (("hip", 2, 0), Fake(err="y"))])
    assert autotune.choice(("k2",)) is None


def test_screen_all_then_retime_the_best_four(tuner):
    # screen order (fastest first): f2 f5 f0 f3 | f4 f1; the re-timing reverses the best four
    f = [Fake(3.0, 2.5), Fake(9.0, 0.1), Fake(1.0, 4.0), Fake(4.0, 2.0), Fake(5.0, 0.1), Fake(2.0, 3.0)]
    bad = Fake(err="refused: tile\nsecond line")
    cands = [(("hip", i, 0), fn) for i, fn in enumerate(f)]
    cands.insert(2, (("hip", 99, 0), bad))
    assert autotune.pick(("k",), cands) == ("hip", 3, 0)        # fastest of the re-timed four, not of the screen
    assert [(fn, r) for fn, r in tuner if r == 3] == [(fn, 3) for _, fn in cands]   # everyone screened, in order
    assert [(fn, r) for fn, r in tuner if r != 3] == [(f[2], 12), (f[5], 12), (f[0], 12), (f[3], 12)]
    assert f[4].calls == f[1].calls == 1 and bad.calls == 1     # screened only
    assert autotune.tuning_log() == {("k",): [
        (("hip", 99, 0), "error: refused: tile"),
        (("hip", 2, 0), 4.0), (("hip", 5, 0), 3.0), (("hip", 0, 0), 2.5), (("hip", 3, 0), 2.0)]}
    assert autotune.choice(("k",)) == ("hip", 3, 0)


def test_a_candidate_that_raises_is_never_chosen(tuner):
    cands = [(("hip", 1, 0), Fake(err="a")), (("blas", 0, 0), Fake(7.0, 7.0)), (("hip", 2, 0), Fake(err="b" * 300))]
    assert autotune.pick(("k",), cands) == ("blas", 0, 0)
    log = autotune.tuning_log()[("k",)]
    assert log == [(("hip", 1, 0), "error: a"), (("hip", 2, 0), "error: " + "b" * 200), (("blas", 0, 0), 7.0)]
    # nothing ran: the default is the last candidate
    assert autotune.pick(("k2",), [(("hip", 1, 0), Fake(err="a")), (("miopen", 0, 0), Fake(err="b"))]) == ("miopen", 0, 0)


@pytest.mark.parametrize("vendor", ["miopen", "blas", "blas32"])
def test_margin_rule(tuner, monkeypatch, vendor):
    def cands(own_t):
        return [(("hip", 1, 0), Fake(own_t + 1.0, own_t + 1.0)), (("wino", 0, 0), Fake(own_t, own_t)),
                ((vendor, 0, 0), Fake(1.0, 1.0))]
    # within the margin: the best own kernel is kept and the log says so
    assert autotune.pick(("near",), cands(1.04)) == ("wino", 0, 0)
    assert autotune.tuning_log()[("near",)][-1] == (("wino", 0, 0), "kept: within GKSGD_GK_MARGIN of 1.0")
    # beyond it the vendor library wins
    assert autotune.pick(("far",), cands(1.06)) == (vendor, 0, 0)
    assert all(not str(v).startswith("kept") for _, v in autotune.tuning_log()[("far",)])
    # margin 0: the fastest wins
    monkeypatch.setattr(autotune, "_GK_MARGIN", 0.0)
    assert autotune.pick(("zero",), cands(1.04)) == (vendor, 0, 0)
    # an own kernel that is fastest needs no margin
    monkeypatch.setattr(autotune, "_GK_MARGIN", 0.05)
    assert autotune.pick(("own",), cands(0.9)) == ("wino", 0, 0)
    assert len(autotune.tuning_log()[("own",)]) == 3


def test_save_then_load_restores_the_table(tuner, tmp_path):
    table = {("fwd", 2, 64, 8, 8, 128, 1, 1, True, "f32", "x6"): ("hip", 100001, 512),
             ("lin_wgrad", 128, 64, 128): ("blas32", 0, 0), ("lstm_step", "fwd", 20, 1500, "f32"): ("hip", 8, 0)}
    autotune._choices.update(table)
    path = str(tmp_path / "choices.json")
    autotune.save_choices(path)
    autotune._choices.clear()
    assert autotune.load_choices(path) == 3
    assert autotune.tuned_choices() == table
    # a key already present keeps its choice
    autotune._choices[("lin_wgrad", 128, 64, 128)] = ("hip", 4, 0)
    assert autotune.load_choices(path) == 3
    assert autotune.choice(("lin_wgrad", 128, 64, 128)) == ("hip", 4, 0)
    assert autotune.load_choices(str(tmp_path / "missing.json")) == 0


def test_tuner_state_lives_in_autotune_only():
    for name in ("_choices", "_TUNE", "_pick", "_time", "_timings", "_F32MM"):
        for mod in (conv1x1, linear):
            assert not hasattr(mod, name), (mod.__name__, name)
    assert conv1x1.set_f32_matmul is autotune.set_f32_matmul and conv1x1.tuned_choices is autotune.tuned_choices


# --------------------------------------------------------------- dispatch trace
CL = torch.channels_last
GEOMS = [(1, 1, 64, 128), (1, 1, 256, 256), (3, 1, 64, 64), (3, 2, 64, 128), (1, 2, 128, 64)]   # k, stride, C -> K
# name, dtype, fp32 matmul mode, conv1x1 attributes patched for the run
MODES = [("bf16", torch.bfloat16, "bf16x6", {}), ("f32_native", torch.float32, "native", {}),
         ("f32_x6", torch.float32, "bf16x6", {}), ("f32_x6_wx6", torch.float32, "bf16x6", {"_WX6": True}),
         ("f32_native_force_wino", torch.float32, "native", {"_FORCE": "wino"})]


def record_trace():
    """Drive every convolution / linear direction on CPU tensors with the
    extension's ops and ``pick`` replaced by recorders; ``pick`` answers with
    its first candidate.  Returns the JSON-ready trace."""
    events = []

    class Ops:
        def __getattr__(self, name):
            def op(*args, **kw):
                events.append(["op", name, [a for a in args if isinstance(a, (bool, int))]])
                return name in ("bn_supported", "wgrad3_supported") or 0
            return op

    def pick(key, cands):
        events.append(["pick", list(key), [list(t) for t, _ in cands]])
        return cands[0][0]
    ops = Ops()
    saved = [(m, n, getattr(m, n)) for m, n in
             [(conv1x1, "_g"), (linear, "_g"), (weight_prep, "_ops"), (autotune, "pick"), (autotune, "_choices"),
              (conv1x1, "_WX6"), (conv1x1, "_FORCE"), (conv1x1, "_WINO")]]
    prev_mode = autotune.f32_matmul()
    calls = []

    def call(label, fn, *args, **kw):
        del events[:]
        fn(*args, **kw)
        calls.append({"call": label, "events": list(events)})
    try:
        for m, n in [(conv1x1, "_g"), (linear, "_g"), (weight_prep, "_ops")]:
            setattr(m, n, lambda: ops)
        autotune.pick = pick
        autotune._choices = {}
        for mname, dt, f32mm, patch in MODES:
            autotune.set_f32_matmul(f32mm)
            conv1x1._WINO, conv1x1._WX6, conv1x1._FORCE = True, False, ""
            for n, v in patch.items():
                setattr(conv1x1, n, v)

            def t(*shape):
                return torch.empty(*shape, dtype=dt).contiguous(memory_format=CL)
            for k, s, C, K in GEOMS:
                tag = "%s k%d s%d %d->%d" % (mname, k, s, C, K)
                x, w = t(2, C, 8, 8), t(K, C, k, k)
                dy = t(2, K, 8 // s, 8 // s)
                call(tag + " fwd", conv1x1._fwd, x, w, s, [])
                call(tag + " dgrad", conv1x1._dgrad, dy, w, x.shape, s)
                if s == 1:
                    for dy2 in (t(2, C, 8, 8), None):
                        link = SimpleNamespace(h=t(2, C, 8, 8), mask=torch.empty(2 * 8 * 8 * C // 8, dtype=torch.uint8),
                                               dy2=dy2)
                        call(tag + " dgrad_bn dy2=%s" % (dy2 is not None), conv1x1._dgrad_bn, dy, w, x.shape, s, link)
                call(tag + " wgrad", conv1x1._wgrad_into, dy, x, w, s, torch.zeros(K, C, k, k).contiguous(memory_format=CL))
            x, w = t(2, 64, 8, 8), t(64, 64, 3, 3)
            call(mname + " fwd bias (no Winograd)", conv1x1._fwd, x, w, 1, [], torch.zeros(64))
            call(mname + " fwd no stats_box", conv1x1._fwd, t(2, 64, 8, 8), t(128, 64, 1, 1), 1)
            big = t(33, 64, 64, 64)        # 33 * 64 * 64 pixel rows > _TN_SMALL_M: no small-batch TN list
            call(mname + " wgrad big", conv1x1._wgrad_into, big, big, t(64, 64, 1, 1), 1,
                 torch.zeros(64, 64, 1, 1).contiguous(memory_format=CL))
            if "force" in mname:
                continue
            for bias in (torch.zeros(128), None):
                tag = "%s linear bias=%s" % (mname, bias is not None)
                call(tag + " fwd", linear._fwd, torch.empty(128, 64, dtype=dt), torch.empty(128, 64, dtype=dt), bias)
                call(tag + " dgrad", linear._dgrad, torch.empty(128, 128, dtype=dt), torch.empty(128, 64, dtype=dt))
    finally:
        for m, n, v in saved:
            setattr(m, n, v)
        autotune.set_f32_matmul(prev_mode)
    # each distinct tag once, each distinct tag list once (as indices into the tags)
    tags, lists = [], []
    for c in calls:
        for e in c["events"]:
            if e[0] == "pick":
                for tg in e[2]:
                    if tg not in tags:
                        tags.append(tg)
                ids = [tags.index(tg) for tg in e[2]]
                if ids not in lists:
                    lists.append(ids)
                e[2] = lists.index(ids)
    return {"tags": tags, "lists": lists, "calls": calls}


def test_dispatch_trace_matches_the_golden():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(record_trace()))
    assert [c["call"] for c in got["calls"]] == [c["call"] for c in want["calls"]]

    def expand(tr, e):
        return [e[0], e[1], [tr["tags"][i] for i in tr["lists"][e[2]]]] if e[0] == "pick" else e
    for g, w in zip(got["calls"], want["calls"]):
        ge, we = [expand(got, e) for e in g["events"]], [expand(want, e) for e in w["events"]]
        assert ge == we, g["call"]
        assert any(e[0] == "pick" for e in ge) and ge[-1][0] == "op", g["call"]   # a pick, then the chosen op ran
    assert json.dumps(got, sort_keys=True) == json.dumps(want, sort_keys=True)    # true / 1 and the like included


if __name__ == "__main__":
    with open(sys.argv[1], "w") as out:
        json.dump(record_trace(), out, separators=(",", ":"))
        out.write("\n")
