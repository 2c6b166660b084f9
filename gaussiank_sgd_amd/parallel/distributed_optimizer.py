"""Communication-compressed data-parallel optimizer (Horovod-style API).

Parity: reference ``distributed_optimizer.py`` -- ``DistributedOptimizer``
(:550-585) returns an instance of a dynamic subclass of the wrapped
optimizer's class with ``step/synchronize/zero_grad/local/increase_one_epoch/
get_current_density/train_iter/train_epoch`` and the same constructor
arguments; the density warm-up ``[0.015625, 0.004, 0.001]`` by epoch
(:60,146-160); threshold / MG-WFBP / MGS bucket planning (:112-310);
selected-count logging (:136-144); gradient dumps (:409-411,422-424).

MI355X execution model (what is different, and why):
  * ``p.data``/``p.grad`` are views of flat arenas (``buckets.GradArena``):
    no per-hook pack copy (reference :364-383) and no pull copy (:385-401).
  * bucket readiness comes from ``register_post_accumulate_grad_hook``; a
    ready bucket is compressed, exchanged and decompressed on a dedicated
    high-priority HIP stream while backward continues on the compute stream.
  * compression is ONE fused HIP pipeline (``ops.compress_``) per bucket with
    no host sync: the reference's 2 + <=3 ``.item()``-style syncs per call and
    its O(n log n) sorts are gone.
  * the exchange is ONE all-gather of a fixed-size packed record
    ``{sent,total,chosen,thr | idx[k_cap] | val[k_cap]}`` (reference: two
    variable-size Horovod all-gathers, :426-427) over RCCL/xGMI, then ONE
    scatter-add launch that averages over ranks.  Unequal counts and
    duplicate indices across ranks are aggregated correctly (the reference's
    half-chunk index_put is wrong for unequal counts).
  * ``synchronize()`` makes the compute stream wait on the bucket events --
    the host never blocks.
  * ``step()`` runs ONE fused SGD (or LARS) launch over the whole arena (wd,
    momentum, nesterov, per-group hyper-parameters) and zeroes the gradient
    arena in the same pass.  ``torch.optim.Adam`` / ``AdamW`` get the same
    one-launch update (``ops.fused_adam_``); their step count is ONE fp32
    device scalar that every ``state[p]["step"]`` aliases, incremented on the
    device, so a captured HIP graph follows it.  ``optim.LAMB`` shares that
    state and runs ``ops.fused_lamb_`` (per-tensor trust ratios reduced in a
    fixed order; ``trust_ratios()``).
"""
from __future__ import annotations

import contextlib
import inspect
import math
import os
import time
from typing import Dict, List, Optional

import numpy as np
import torch

from .. import ops, settings
from ..ops import streams
from ..settings import logger
from ..utils import stats as perf
from ..utils import trace
from . import comm
from .buckets import GradArena, group_with_threshold
from .comm import (allgather, allgather_async, allreduce, allreduce_, allreduce_async_, barrier,  # noqa: F401
                   broadcast, broadcast_, broadcast_async_, broadcast_object, broadcast_optimizer_state,
                   broadcast_parameters, init, local_rank, local_size, rank, size, synchronize)
from .planner import models_for, plan_mgs, plan_mgwfbp

DEFAULT_DYNAMIC_DENSITIES = [0.015625, 0.004, 0.001]
# compress hand-off mode of the buckets that overlap the backward pass
# (ops.compress_ handoff: 1 = in-grid last block, 0 = separate launches,
# -1 = GKSGD_HANDOFF); GKSGD_OVERLAP_HANDOFF=launch restores launches
_OVERLAP_HANDOFF = {"lastblock": 1, "launch": 0, "env": -1}.get(os.environ.get("GKSGD_OVERLAP_HANDOFF", "lastblock"), 1)


def _env_flag(name: str, default: bool) -> bool:
    v = os.environ.get(name)
    if v is None:
        return default
    return v.strip().lower() in ("1", "true", "yes", "on")


# ONE high-priority communication stream per device, shared by every
# DistributedOptimizer of the process.  torch.cuda.Stream(priority=-1) hands
# out the next stream of the high-priority pool on every call, and HIP maps
# streams onto GPU_MAX_HW_QUEUES (4) hardware queues round-robin: a process
# that builds several optimizers (bench.py's phases, a re-created trainer)
# ends up with a comm stream that shares the compute stream's hardware queue,
# which measured 34-100 % slower steps afterwards (profiles/r04_phase_order.txt).
_COMM_STREAMS: Dict[int, "torch.cuda.Stream"] = {}


def _comm_stream_for(dev: torch.device) -> "torch.cuda.Stream":
    i = dev.index if dev.index is not None else torch.cuda.current_device()
    s = _COMM_STREAMS.get(i)
    if s is None:
        s = _COMM_STREAMS[i] = torch.cuda.Stream(device=i, priority=-1)
    return s


class _DistributedOptimizer(torch.optim.Optimizer):
    def __init__(self, params, named_parameters, compression, is_sparse=False, density=0.001,
                 seq_layernames=None, layerwise_times=None, norm_clip=None, threshold=0, writer=None,
                 gradient_path=None, _gk_opts=None):
        opts = dict(_gk_opts or {})
        defaults = opts.pop("defaults", {}) or {}
        # torch.optim.AdamW sets decoupled_weight_decay itself and does not take it back as an
        # argument, and Optimizer.__setstate__ (every load_state_dict) adds differentiable=False to
        # the defaults of classes that do not take it (LAMB, LARS); any other default its class
        # refuses still raises
        takes = inspect.signature(self.__class__.__mro__[1].__init__).parameters
        for own in ("decoupled_weight_decay", "differentiable"):
            if own in defaults and own not in takes and (own != "differentiable" or not defaults[own]):
                defaults = {k: v for k, v in defaults.items() if k != own}
        super(self.__class__, self).__init__(params, **defaults)
        self._compression = compression
        self._sparse = is_sparse
        self._density = density
        self._profiling = bool(opts.get("profiling", False))
        self._seq_layernames = seq_layernames
        self._layerwise_times = layerwise_times
        self._original_layerwise_times_kv = None
        self._norm_clip = norm_clip
        self._threshold = threshold
        self._writer = writer
        self._gradient_path = gradient_path
        if self._layerwise_times is not None and self._seq_layernames is not None:
            self._original_layerwise_times_kv = dict(zip(self._seq_layernames, self._layerwise_times))
        self._layerwise_compressors: Dict[str, float] = {}
        self._compression_timers: Dict[str, list] = {}
        self._allreduce_timers: Dict[str, list] = {}
        self._update_times: Dict[str, list] = {}
        self.train_epoch = 0
        self.train_iter = 0
        dw = opts.get("density_warmup", True)
        self._dynamic_densities = list(DEFAULT_DYNAMIC_DENSITIES) if dw is True else (list(dw) if dw else None)
        logger.info("_dynamic_densities: %s", self._dynamic_densities)
        # entries SENT per bucket-step this epoch (reference :420,136-144 keep the
        # per-call counts and average them at the epoch boundary); with the
        # fused k_cap record these are min(total, k_cap) -- _epoch_sel keeps the
        # (sent, total-above-threshold) pairs
        self._selected_num_gradients: List[int] = []
        self._epoch_sel: List[tuple] = []
        self._sel_generic: List[tuple] = []

        self._compress_single = bool(opts.get("compress_single_rank", _env_flag("GKSGD_COMPRESS_SINGLE", False)))
        self._deterministic = bool(opts.get("deterministic", settings.DETERMINISTIC))
        self._fused_optim = bool(opts.get("fused_optimizer", _env_flag("GKSGD_FUSED_OPTIM", True)))
        self._zero_grad_in_step = bool(opts.get("zero_grad_in_step", True))
        self._overlap = bool(opts.get("overlap", _env_flag("GKSGD_OVERLAP", True)))
        if comm.backend() == "loopback":
            # autograd runs GPU backward (and so the grad hooks) on one shared
            # device thread, not on the virtual rank's thread: exchange in step()
            self._overlap = False
        # native_rccl: True (native engine when world > 1), False, or "force"
        # (native engine even in a world of one: GPU tests of the shared communicator)
        nr = opts.get("native_rccl", True)
        self._force_native_rccl = nr == "force"
        self._prefer_native_rccl = bool(nr)
        self._planner_preset = opts.get("planner_preset", "mi355x")
        # planner: "threshold" (reference default), "mgs" / "mgwfbp" (use the
        # layer-wise times even without settings.ADAPTIVE_MERGE), "auto"
        # (settings.ADAPTIVE_MERGE decides, reference behaviour); planner_world:
        # world size the cost models are evaluated at (default: this world)
        self._planner = opts.get("planner", "auto")
        self._planner_world = opts.get("planner_world")
        # DGC momentum correction (Lin et al. 2018): momentum is accumulated
        # locally BEFORE sparsification and the global update is plain SGD.
        self._mc = bool(opts.get("momentum_correction", _env_flag("GKSGD_MOMENTUM_CORRECTION", False)))
        # optional device scalar multiplying the lr inside the fused update
        # (set by train/graph.py so a captured step follows the lr schedule)
        self._lr_mult: Optional[torch.Tensor] = None
        # optional int32 device words, one per bucket, holding the compressor
        # seeds (train/graph.py: a captured step reads them at replay time, so
        # random-k / DGC sampling draw new indices every replay)
        self._seed_dev: Optional[torch.Tensor] = None
        self._mc_applied = False
        # Under momentum correction the global update is plain SGD on the
        # aggregate: apply it straight from the gathered records (no dense
        # gradient scatter, no dense optimizer pass) unless something needs the
        # dense aggregate (clip_grad_norm_, aggregated_grads()).
        self._sparse_apply_opt = bool(opts.get("sparse_apply", _env_flag("GKSGD_SPARSE_APPLY", True)))
        self._pending_apply = False
        self._base_cls = opts.get("base_cls", None)
        self._state_dirty = False
        # cross-rank agreement on every bucket's record size and density before
        # the first exchange, and again after every event that can change them
        # (epoch boundary of the density schedule, a resume): a mismatch raises
        # on every rank instead of pairing records of different sizes inside
        # one all-gather (an RCCL hang, or garbage) -- GKSGD_PLAN_CHECK=0 skips
        self._plan_check = _env_flag("GKSGD_PLAN_CHECK", True)
        self._plan_check_due = True
        # GKSGD_CHECK_ORDER=1: also agree on (bucket index, record words) before
        # EVERY exchange (one blocking collective per exchange: a debug mode)
        self._check_order = _env_flag("GKSGD_CHECK_ORDER", False)
        self._next_launch = 0     # buckets launch strictly in index order
        # selection_quality_every = N > 0: every N-th step each fused sparse
        # bucket's record is scored against the exact top-k of its accumulator
        # on device (ops.selection_quality_); rows wait in a device ring until
        # collect_selection_quality().  0 (default): nothing is allocated or
        # launched.  Skipped while a HIP graph captures (a captured step
        # cannot advance the ring).
        self._quality_every = max(0, int(opts.get("selection_quality_every",
                                                  os.environ.get("GKSGD_SELECTION_QUALITY_EVERY", "0")) or 0))
        self._q_dev: Optional[torch.Tensor] = None   # ring of float64[8] blocks, allocated on first use
        self._q_meta: List[tuple] = []               # (iter, bucket, k_cap) of the ring's rows
        self._q_host: List[dict] = []
        self._q_capture_logged = False

        named_parameters = list(named_parameters) if named_parameters is not None else []
        if any(not isinstance(p, tuple) for p in named_parameters):
            raise ValueError("named_parameters should be a sequence of tuples (name, parameter), "
                             "usually produced by model.named_parameters().")
        in_groups = {id(p) for g in self.param_groups for p in g["params"]}
        if named_parameters:
            named_parameters = [(k, v) for k, v in named_parameters if id(v) in in_groups and v.requires_grad]
        else:
            named_parameters = [("allreduce.noname.%s" % i, v) for g in self.param_groups
                                for i, v in enumerate(g["params"]) if v.requires_grad]
        self._named_parameters = {k: v for k, v in named_parameters}
        if self._seq_layernames is not None:
            self._sequential_keys = [k for k in self._seq_layernames if k in self._named_parameters]
        else:
            self._sequential_keys = [k for k, _ in named_parameters]
        self._parameter_names = {v: k for k, v in sorted(named_parameters)}

        self._generate_merged_parameters()

        self._world = size()
        self._rank = rank()
        self._handles: Dict[int, object] = {}
        self._grad_accs = []
        self._requires_update = set()
        self.local = False
        self._hooks_on = self._world > 1 or self._compress_single
        self._grads_zero = True
        self._pending_dumps: List[tuple] = []
        self._sel_dev: Optional[torch.Tensor] = None
        self._graph_sel: List[torch.Tensor] = []   # per-bucket selected-count slots of a captured step
        self._sel_n = 0
        self._setup_exchange()
        self._setup_fused_update()
        if self._mc:
            if not (self._fused_sparse and self._fused_kind == "sgd"):
                raise ValueError("momentum_correction needs a fused sparse compressor and torch.optim.SGD "
                                 "(fused update path)")
            self._arena.velocity = torch.zeros(self._arena.total, dtype=torch.float32, device=self._arena.device)
        if self._hooks_on:
            self._register_hooks()
        self._watchdog = None
        wd_s = float(opts.get("watchdog_s", os.environ.get("GKSGD_WATCHDOG_S", "0")) or 0)
        if wd_s > 0:
            from ..utils.watchdog import Watchdog
            self._watchdog = Watchdog(wd_s, self.describe_state)

    # ------------------------------------------------------------------
    # planning
    # ------------------------------------------------------------------
    def _generate_groups_with_threshold(self, threshold):
        sizes = {k: self._named_parameters[k].numel() for k in self._sequential_keys}
        self._sizes = [sizes[k] for k in self._sequential_keys][::-1]
        groups = group_with_threshold(self._sequential_keys, sizes, threshold)
        key_map = {k: gi for gi, g in enumerate(groups) for k in g}
        return groups, key_map

    def _generate_groups_mgwfbp(self):
        P = int(self._planner_world or size())
        ar, alpha, _, _ = models_for(P, self._density, self._planner_preset)
        sizes = [self._named_parameters[k].numel() for k in self._seq_layernames]
        self._sizes = sizes
        return plan_mgwfbp(self._seq_layernames, self._layerwise_times, sizes, ar, alpha)

    def _generate_groups_mgs(self):
        P = int(self._planner_world or size())
        _, _, ct, ag = models_for(P, self._density, self._planner_preset)
        sizes = [self._named_parameters[k].numel() for k in self._seq_layernames]
        self._sizes = sizes
        return plan_mgs(self._seq_layernames, self._layerwise_times, sizes, ct, ag)

    def _generate_merged_parameters(self):
        adaptive = settings.ADAPTIVE_MERGE if self._planner == "auto" else self._planner in ("mgs", "mgwfbp")
        if adaptive and self._layerwise_times is not None and self._seq_layernames is not None:
            if (self._density < 1 and self._planner != "mgwfbp") or self._planner == "mgs":
                groups, key_map = self._generate_groups_mgs()
            else:
                groups, key_map = self._generate_groups_mgwfbp()
            # keys missing from the profile (no grad) go into the last group
            seen = {k for g in groups for k in g}
            rest = [k for k in self._sequential_keys if k not in seen]
            if rest:
                groups[-1].extend(rest)
        else:
            groups, key_map = self._generate_groups_with_threshold(self._threshold)
        logger.info("# of parameters: %d", int(np.sum(self._sizes)))
        logger.info("Total number of tensors: %s", len(self._sizes))
        logger.info("Merged Number of groups: %s", len(groups))
        sparse_fused = self._sparse and getattr(self._compression, "fused", False) and \
            not getattr(self._compression, "dense", False)
        self._arena = GradArena([(k, self._named_parameters[k]) for k in self._sequential_keys], groups,
                                with_residuals=sparse_fused)
        self._groups = groups
        self._key_groupidx_maps = {k: gi for gi, g in enumerate(groups) for k in g}
        self._merged_parameters = {b.name: b for b in self._arena.buckets}
        self._merged_parameter_names = {b.index: b.name for b in self._arena.buckets}
        for b in self._arena.buckets:
            density = self._density
            if self._density < 1 and settings.ADAPTIVE_SPARSE:
                density = max(perf.predict_density_with_size_and_computation(b.numel, 0.0, size()), self._density)
            self._layerwise_compressors[b.name] = density

    # ------------------------------------------------------------------
    # exchange engine setup
    # ------------------------------------------------------------------
    def _setup_exchange(self):
        dev = self._arena.device
        self._device = dev
        self._is_cuda = dev.type == "cuda"
        self._exchanger = comm.Exchanger(dev, prefer_native=self._prefer_native_rccl,
                                         force_native=self._force_native_rccl) if self._hooks_on else None
        self._comm_stream = None
        # GKSGD_COMM_STREAM=0: compression / exchange inline on the compute stream
        # (no overlap; a single-stream step, e.g. for whole-step graph capture)
        if self._is_cuda and self._hooks_on and os.environ.get("GKSGD_COMM_STREAM", "1") != "0":
            self._comm_stream = _comm_stream_for(dev)
        comp = self._compression
        self._fused_sparse = self._sparse and getattr(comp, "fused", False) and not getattr(comp, "dense", False)
        max_density = max([self._density] + (self._dynamic_densities or []))
        P = max(self._world, 1)
        for b in self._arena.buckets:
            if self._is_cuda:
                b.done_event = torch.cuda.Event()
                b.extra["ready_event"] = torch.cuda.Event()
            if self._fused_sparse:
                kmax = comp.k_of(b.numel, max(self.get_current_density(b.name), max_density))
                kcap_max = comp.k_cap_for(kmax, b.numel)
                b.bufs = ops.CompressBuffers(kcap_max, dev)
                b.gathered = torch.zeros(P * (ops.REC_HDR + 2 * kcap_max), dtype=torch.int32, device=dev)
                if getattr(comp, "mode", None) == ops.MODE_RANDOMK:
                    # random-k must never pick the arena's padding slots
                    layout = [(o, self._named_parameters[k].numel()) for k, o in zip(b.keys, b.offsets)]
                    b.extra["valid"] = ops.valid_bitmask(layout, b.span, dev)
            elif getattr(comp, "name", None) == "bucket":
                b.extra["mask"] = torch.zeros(b.span, dtype=torch.uint8, device=dev)
                b.extra["means"] = torch.zeros(2, dtype=torch.float32, device=dev)
                b.extra["ws"] = ops.sign_bucket_ws(dev)
        self._sel_dev = torch.zeros(8192, 2, dtype=torch.int32, device=dev)   # (sent, total) per bucket-step
        self._sel_host: List[tuple] = []

    # ------------------------------------------------------------------
    # hooks
    # ------------------------------------------------------------------
    def _register_hooks(self):
        for group in self.param_groups:
            for p in group["params"]:
                if p.requires_grad and p in self._parameter_names:
                    self._requires_update.add(p)
                    self._grad_accs.append(p.register_post_accumulate_grad_hook(self._make_hook(p)))

    def _make_hook(self, p):
        key = self._parameter_names[p]
        bi = self._arena.key_to_bucket[key]

        def hook(param):
            self._grads_zero = False
            if self.local:
                return
            self._arena.check_grad(key, param)
            b = self._arena.buckets[bi]
            b.ready += 1
            if b.ready == len(b.params) and not b.launched and self._overlap:
                self._launch_in_order()
        return hook

    def _launch_in_order(self):
        """Launch every complete bucket from the next one due, strictly in
        bucket-index order: a bucket whose gradients complete early waits for
        its predecessors and is launched by the launch of the last of them.
        The collective sequence is then the bucket sequence on every rank,
        whatever order autograd runs the hooks in (Horovod gets the same
        guarantee by negotiating tensor names through its coordinator; the
        reference relies on it, distributed_optimizer.py:426-427,461-463)."""
        bs = self._arena.buckets
        while self._next_launch < len(bs):
            b = bs[self._next_launch]
            if not b.launched:
                if b.ready != len(b.params):
                    return
                self._launch_bucket(b)
            self._next_launch += 1

    # ------------------------------------------------------------------
    # bf16 shadow weights (parallel/shadow.py)
    # ------------------------------------------------------------------
    def _ensure_shadow(self) -> torch.Tensor:
        arena = self._arena
        if getattr(arena, "shadow", None) is None:
            arena.shadow = torch.empty(arena.total, dtype=torch.bfloat16, device=arena.device)
            comm.on_storage_overwritten(arena.weights.untyped_storage().data_ptr(), self.refresh_shadow)
        return arena.shadow

    def refresh_shadow(self) -> None:
        """Re-cast the bf16 shadow from the fp32 master weights."""
        shadow = getattr(self._arena, "shadow", None)
        if shadow is not None:
            with torch.no_grad():
                ops.cast_bf16_(shadow, self._arena.weights)

    def _make_sink(self, key):
        arena = self._arena
        gv = arena.grad_views[key]
        p = self._named_parameters[key]

        def check():
            if p.grad is None or p.grad.data_ptr() != gv.data_ptr():
                arena.check_grad(key, p)

        def sink(grad):
            check()
            ops.accum_grad_(gv, grad)
        # kernels that accumulate into the arena themselves (ops/conv1x1.py)
        # call check() and write grad_view directly
        sink.grad_view = gv
        sink.check = check
        return sink

    # ------------------------------------------------------------------
    # density schedule / logging (reference :136-160)
    # ------------------------------------------------------------------
    def increase_one_epoch(self):
        # the epoch's counts are those of the density in force during it (logged
        # before the schedule moves on)
        self.log_selection_summary()
        self.check_compress_sync()
        self.train_epoch += 1
        self._plan_check_due = True

    def log_selection_summary(self):
        """The reference's per-epoch selected-count lines (:136-144) for the
        bucket-steps since the last summary; the counts are then reset (the
        schedule position is not touched: a run stopped mid-epoch logs its
        partial epoch without advancing the density schedule)."""
        self._drain_selected()
        density = self.get_current_density()
        counts = self._selected_num_gradients
        if rank() == 0:
            sz = int(np.sum(self._sizes))
            k = max(int(sz * density), 1)
            mean = float(np.mean(counts)) if counts else 0.0
            logger.info("Average number of selected gradients: %f, exact k: %d", mean, k)
            logger.info("The number of selected gradients: %s", counts)
            totals = [t for _, t in self._epoch_sel]
            if totals and sum(totals) != sum(counts):
                logger.info("Average number above the threshold (before the k_cap cut): %f", float(np.mean(totals)))
            if counts:
                logger.info("Effective compression ratio: %.1fx", self.wire_compression_ratio(density))
        self._selected_num_gradients = []
        self._epoch_sel = []

    def check_compress_sync(self) -> int:
        """New expired bounded spins of the fused decide / fallback grid
        (compress.hip decide_fb_kernel: a grid that was not co-resident) since
        the last check; one small D2H per compressed bucket.  A bucket that
        had one gets its workspace back to the at-rest state (every arrival
        counter and flag zero -- a timed-out block may have left a grid barrier
        half counted) and compresses with in-grid hand-offs from then on, which
        do not use that grid.  Called at every epoch boundary."""
        if not (self._is_cuda and self._fused_sparse):
            return 0
        new = 0
        for b in self._arena.buckets:
            bufs = getattr(b, "bufs", None)
            if bufs is None or getattr(bufs, "ctrl", None) is None:
                continue
            n = ops.sync_timeouts(bufs)
            seen = b.extra.get("sync_seen", 0)
            if n > seen:
                new += n - seen
                b.extra["sync_seen"] = n
                torch.cuda.synchronize(self._device)
                bufs.ws.zero_()
                b.extra["handoff"] = 1
                logger.warning("bucket %d: %d expired grid-barrier spins in the fused compression decide; "
                               "workspace reset, in-grid hand-offs from now on", b.index, n - seen)
        return new

    def _drain_selected(self) -> List[tuple]:
        """(sent, total) per bucket-step logged since the last drain (one D2H
        copy); also appended to the epoch's lists."""
        n = self._sel_n
        dev = [tuple(int(v) for v in x) for x in self._sel_dev[:n].cpu().tolist()] if n else []
        out = self._sel_generic + self._sel_host + dev
        self._sel_generic = []
        self._sel_host = []
        self._sel_n = 0
        self._epoch_sel.extend(out)
        self._selected_num_gradients.extend(s for s, _ in out)
        return out

    def _collect_selected(self, with_totals: bool = False) -> list:
        """Counts of the bucket-steps since the last call (a display window):
        entries sent, or (sent, total) pairs with ``with_totals``.  The epoch
        summary (increase_one_epoch) still sees every window."""
        pairs = self._drain_selected()
        return pairs if with_totals else [s for s, _ in pairs]

    def enable_device_seeds(self) -> torch.Tensor:
        """Switch the compressors to seeds read from device memory (one int32
        word per bucket); ``refresh_device_seeds`` writes the step's seeds."""
        if self._seed_dev is None:
            self._seed_dev = torch.zeros(len(self._arena.buckets), dtype=torch.int32, device=self._device)
        self.refresh_device_seeds()
        return self._seed_dev

    def refresh_device_seeds(self, step: Optional[int] = None) -> None:
        """Write seed_for(step, bucket, rank) of every bucket into the device
        words (one stream-ordered H2D copy; what a graph replay will read)."""
        if self._seed_dev is None:
            return
        comp = self._compression
        it = self.train_iter if step is None else int(step)
        fn = getattr(comp, "seed_for", None)
        vals = [fn(it, b.index, self._rank) if fn is not None else 0 for b in self._arena.buckets]
        host = torch.tensor([v - (1 << 32) if v >= (1 << 31) else v for v in vals], dtype=torch.int32)
        self._seed_dev.copy_(host, non_blocking=True)

    def wire_bytes_per_step(self, density: Optional[float] = None) -> int:
        """Bytes one rank puts on the wire per step: the fixed-size record of
        every sparse bucket ((4 + 2 k_cap) int32 words), the dense fp32 bucket
        otherwise (the sign-bucket compressor: two fp32 means)."""
        comp = self._compression
        name = getattr(comp, "name", "none")
        total = 0
        for b in self._arena.buckets:
            d = self.get_current_density(b.name) if density is None else density
            if self._sparse and d < 1 and hasattr(comp, "k_of"):
                total += (ops.REC_HDR + 2 * comp.k_cap_for(comp.k_of(b.numel, d), b.numel)) * 4
            elif name == "bucket":
                total += 8
            else:
                total += b.numel * 4
        return total

    def wire_compression_ratio(self, density: Optional[float] = None) -> float:
        """Dense fp32 gradient bytes / bytes actually exchanged per rank and step."""
        sz = int(np.sum(self._sizes))
        wb = self.wire_bytes_per_step(density)
        return (sz * 4.0) / wb if wb else 1.0

    def get_current_density(self, name=None):
        density = self._density
        if self._dynamic_densities is not None:
            if self.train_epoch >= len(self._dynamic_densities):
                density = self._dynamic_densities[-1]
            else:
                density = self._dynamic_densities[self.train_epoch]
        if name is not None and self._layerwise_compressors is not None:
            if name not in self._layerwise_compressors:
                errstr = "compressor density not found at layer: %s" % name
                logger.error(errstr)
                raise Exception(errstr)
            ld = self._layerwise_compressors[name]
            density = max(ld, density)
        return density

    # ------------------------------------------------------------------
    # per-bucket pipeline
    # ------------------------------------------------------------------
    def _plan_signature(self) -> List[int]:
        """What every rank must agree on before exchanging: the world, the
        compressor, and per bucket its element count, density (parts per
        billion) and the int32 words of the record (or dense payload) it puts
        into the collective."""
        comp = self._compression
        sig = [self._world, len(self._arena.buckets), int(getattr(comp, "mode", -1) or 0)]
        for b in self._arena.buckets:
            d = self.get_current_density(b.name)
            sig += [b.numel, int(round(d * 1e9)), self._exchange_words(b, d)]
        return sig

    def _exchange_words(self, b, density: float) -> int:
        comp = self._compression
        if self._fused_sparse and self._sparse and density < 1:
            k = comp.k_of(b.numel, density)
            return ops.REC_HDR + 2 * min(comp.k_cap_for(k, b.numel), b.bufs.k_cap)
        if getattr(comp, "name", None) == "bucket":
            return 2
        return b.numel

    def _ensure_plan_agreed(self):
        if not (self._plan_check_due and self._plan_check and self._world > 1):
            return
        if self._is_cuda and torch.cuda.is_current_stream_capturing():
            return      # a captured step replays what the eager warm-up agreed on
        self._plan_check_due = False
        ok, mins, maxs = comm.agree_ints(self._plan_signature())
        if not ok:
            sig = self._plan_signature()
            raise RuntimeError(
                "DistributedOptimizer: the ranks disagree on the exchange plan (rank %d: epoch %d, iter %d, "
                "signature %s; min over ranks %s, max %s). Every rank must run the same model, bucket plan and "
                "density schedule position (after a resume: the same train_epoch); refusing to enter the "
                "collective." % (self._rank, self.train_epoch, self.train_iter, sig, mins, maxs))

    def _check_exchange_order(self, pairs):
        """GKSGD_CHECK_ORDER=1: agree on the (bucket index, payload words) of
        this exchange on every rank before entering it."""
        sig = [x for p in pairs for x in p]
        ok, mins, maxs = comm.agree_ints(sig)
        if not ok:
            raise RuntimeError("DistributedOptimizer: exchange order mismatch at iter %d on rank %d: this rank "
                               "exchanges (bucket, words) %s; min over ranks %s, max %s" % (
                                   self.train_iter, self._rank, sig, mins, maxs))

    def _launch_bucket(self, b):
        self._ensure_plan_agreed()
        b.launched = True
        # a bucket compressed while the backward still runs (another bucket is
        # not launched yet) hands its single-workgroup steps over inside the
        # producing grids: a separate 1-workgroup launch on the comm stream
        # waits behind the backward GEMM blocks that fill the chip (BERT fp32:
        # decide 104 us per call overlapped vs 12 us alone,
        # profiles/r04_bert_fp32_kernel_stats.csv)
        b.extra["overlapped"] = self._overlap and any(not o.launched for o in self._arena.buckets)
        with trace.range("gk/b%d/launch" % b.index):
            if self._comm_stream is not None:
                cur = torch.cuda.current_stream(self._device)
                ev = b.extra["ready_event"]
                ev.record(cur)
                self._comm_stream.wait_event(ev)
                # grad-weight GEMMs still running on the side stream (ops/streams.py)
                streams.join(self._device, self._comm_stream)
                with torch.cuda.stream(self._comm_stream):
                    self._process_bucket(b)
                    b.done_event.record(self._comm_stream)
            else:
                streams.join(self._device)
                self._process_bucket(b)

    def _timer(self):
        if not self._profiling:
            return None
        if self._is_cuda:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            return e
        return time.time()

    def _elapsed(self, t0, t1) -> float:
        if t0 is None or t1 is None:
            return 0.0
        if self._is_cuda:
            t1.synchronize()
            return t0.elapsed_time(t1) / 1e3
        return t1 - t0

    def _process_bucket(self, b):
        density = self.get_current_density(b.name)
        g = b.slice(self._arena.grads)
        comp = self._compression
        t0 = self._timer()
        if self._sparse and density < 1:
            if self._fused_sparse:
                self._sparse_fused(b, g, density, t0)
            else:
                self._sparse_generic(b, g, density, t0)
        else:
            self._dense(b, g, t0)

    def _sparse_fused(self, b, g, density, t0):
        rec, k_cap = self._compress_bucket(b, g, density)
        t1 = self._timer()
        gathered = self._exchange_records([b], [rec], [k_cap])[0]
        t2 = self._timer()
        self._finish_bucket(b, g, gathered, rec, k_cap)
        t3 = self._timer()
        if self._profiling:
            self._pending_timers = getattr(self, "_pending_timers", [])
            self._pending_timers.append((b.name, t0, t1, t2, t3))

    def _compress_bucket(self, b, g, density):
        """Fused HIP compression of one bucket into its fixed-size send record."""
        comp = self._compression
        k = comp.k_of(b.numel, density)
        k_cap = min(comp.k_cap_for(k, b.numel), b.bufs.k_cap)
        r = b.slice(self._arena.residuals)
        # stateless seed: (iteration, bucket, rank) -- identical across ranks for *same* variants
        seed = comp.seed_for(self.train_iter, b.index, self._rank)
        # device seed words only while a graph captures (every replay reads the
        # words refresh_device_seeds wrote); an eager step -- the warm-up steps of a
        # recapture included -- takes seed_for(train_iter) directly
        seed_dev = None
        if self._seed_dev is not None and self._is_cuda and torch.cuda.is_current_stream_capturing():
            seed_dev = self._seed_dev[b.index:b.index + 1]
        arena = self._arena
        mc = None
        if self._mc:
            # DGC momentum correction fused into the compressor's statistics pass;
            # momentum factor masking happens in its select pass
            begin, count = self._bucket_chunks[b.index]
            mc = {"u": b.slice(arena.velocity), "w": b.slice(arena.weights), "chunks": self._chunks, "begin": begin,
                  "count": count, "base": b.start, "groups": self.param_groups, "chunk_list": self._chunk_list}
            self._mc_applied = True
        with trace.range("gk/b%d/compress" % b.index):
            ops.compress_(g, r, b.bufs, comp.mode, ec=comp.ec, zero_g=True, loops=comp.loops,
                          z=comp.z_for(density), k=k, k_cap=k_cap, seed=seed, sample_p=getattr(comp, "sample_p", 0.01),
                          n_stats=b.numel, valid=b.extra.get("valid"), mc=mc, seed_dev=seed_dev,
                          handoff=_OVERLAP_HANDOFF if b.extra.get("overlapped") else b.extra.get("handoff", -1))
        rec_words = ops.REC_HDR + 2 * k_cap
        return b.bufs.record[:rec_words], k_cap

    def _exchange_records(self, bs, recs, k_caps):
        """All-gather the records of one or more buckets (one grouped RCCL launch)."""
        if self._world <= 1:
            return list(recs)
        outs = [b.gathered[: self._world * (ops.REC_HDR + 2 * kc)] for b, kc in zip(bs, k_caps)]
        if self._check_order:
            self._check_exchange_order([(b.index, ops.REC_HDR + 2 * kc) for b, kc in zip(bs, k_caps)])
        with trace.range("gk/allgather/%s" % ",".join("b%d" % b.index for b in bs)):
            if len(bs) == 1:
                self._exchanger.allgather_(outs[0], recs[0])
            else:
                self._exchanger.allgather_many_(outs, list(recs))
        return outs

    def _finish_bucket(self, b, g, gathered, rec, k_cap):
        b.extra["agg"] = (gathered, max(self._world, 1), k_cap)
        if self._mc and self._sparse_apply_ok():
            # the update is applied from the records in step() (after backward:
            # the weights it writes are still read by the rest of backward)
            self._pending_apply = True
        else:
            # One deterministic launch: every index is summed over ranks in rank
            # order and averaged once (reference loop + division,
            # distributed_optimizer.py:468-482), so all replicas compute
            # bit-identical aggregates for any P.
            with trace.range("gk/b%d/decompress" % b.index):
                ops.scatter_add_records_(g, gathered, max(self._world, 1), k_cap, 1.0 / max(self._world, 1), True)
            b.extra["agg_done"] = True
        self._log_selected(b.bufs.record[0:2])
        if self._quality_every and self._fused_sparse and self.train_iter % self._quality_every == 0:
            self._sample_quality(b, k_cap)
        if settings.LOGGING_GRADIENTS and self._rank == 0 and self._gradient_path and \
                self.train_iter % max(1, settings.DUMP_GRAD_EVERY) == 0:
            self._queue_dump(b, b.slice(self._arena.residuals), rec, k_cap)

    def _launch_group(self, bs):
        """Several due buckets at once (synchronize() without overlap): compress
        each, ONE grouped all-gather of all records, then finish each -- one
        collective launch instead of len(bs)."""
        self._ensure_plan_agreed()
        for b in bs:
            b.launched = True
            b.extra["overlapped"] = False
        cur = torch.cuda.current_stream(self._device) if self._comm_stream is not None else None
        ctx = torch.cuda.stream(self._comm_stream) if self._comm_stream is not None else contextlib.nullcontext()
        if cur is not None:
            ev = bs[0].extra["ready_event"]
            ev.record(cur)
            self._comm_stream.wait_event(ev)
            streams.join(self._device, self._comm_stream)
        else:
            streams.join(self._device)
        with ctx, trace.range("gk/group/%d" % len(bs)):
            parts = []
            for b in bs:
                g = b.slice(self._arena.grads)
                rec, kc = self._compress_bucket(b, g, self.get_current_density(b.name))
                parts.append((b, g, rec, kc))
            outs = self._exchange_records([p[0] for p in parts], [p[2] for p in parts], [p[3] for p in parts])
            for (b, g, rec, kc), out in zip(parts, outs):
                self._finish_bucket(b, g, out, rec, kc)
            if self._comm_stream is not None:
                for b in bs:
                    b.done_event.record(self._comm_stream)

    def _sparse_generic(self, b, g, density, t0):
        """Reference-semantics path for compressors without a fused spec (host syncs)."""
        comp = self._compression
        flat = g
        # residuals are per rank: qualify the group name so the virtual ranks of
        # an in-process world never share (and corrupt) one residual
        tensor, ctx, values = comp.compress(flat, "%s@rank%d" % (b.name, self._rank), ratio=density)
        self._sel_generic.append((int(ctx.numel()), int(ctx.numel())))
        if settings.LOGGING_GRADIENTS and self._rank == 0 and self._gradient_path:
            np.save("%s/r%d_gradients_iter_%d" % (self._gradient_path, self._rank, self.train_iter),
                    tensor.detach().cpu().numpy())
        t1 = self._timer()
        all_vals = allgather(values)
        all_idx = allgather(ctx.int())
        counts = allgather(torch.tensor([int(ctx.numel())], dtype=torch.int64, device=flat.device))
        t2 = self._timer()
        flat.zero_()
        # rank order, then one division (reference :468-482): fp32 atomics from
        # several ranks would let the replicas drift apart
        # (indices are unique inside one rank's chunk: one add per index per launch)
        pos = 0
        for c in counts.view(-1).tolist():
            c = int(c)
            if c:
                flat.index_add_(0, all_idx[pos:pos + c].long(), all_vals[pos:pos + c])
            pos += c
        flat.div_(max(self._world, 1))
        t3 = self._timer()
        if self._profiling:
            self._pending_timers = getattr(self, "_pending_timers", [])
            self._pending_timers.append((b.name, t0, t1, t2, t3))

    def _dense(self, b, g, t0):
        comp = self._compression
        name = getattr(comp, "name", "none")
        if name == "bucket":
            mask, means, ws = b.extra["mask"], b.extra["means"], b.extra["ws"]
            ops.sign_bucket_compress_(g, mask, means, ws)
            t1 = self._timer()
            self._allreduce_avg(means, b)
            t2 = self._timer()
            ops.sign_bucket_decompress_(g, mask, means)
        else:
            t1 = self._timer()
            self._allreduce_avg(g, b)
            t2 = self._timer()
        t3 = self._timer()
        if self._norm_clip is not None:
            clip = math.sqrt(1.0 / max(size(), 1)) * self._norm_clip
            ops.clip_grad_norm_(g, clip)
        if self._profiling:
            self._pending_timers = getattr(self, "_pending_timers", [])
            self._pending_timers.append((b.name, t0, t1, t2, t3))

    def _allreduce_avg(self, t, b=None):
        if self._world <= 1:
            return
        if self._check_order and b is not None:
            self._check_exchange_order([(b.index, t.numel())])
        self._exchanger.allreduce_(t, average=True)

    def _log_selected(self, hdr: torch.Tensor):
        """Queue a record header's (sent, total) words (device copy, no sync)."""
        if self._is_cuda and torch.cuda.is_current_stream_capturing():
            # whole-step graph capture: the replayed copy lands in a slot of its
            # own; train/graph.py logs the slots after every replay
            slot = torch.zeros(2, dtype=torch.int32, device=hdr.device)
            slot.copy_(hdr.view(-1)[:2], non_blocking=True)
            self._graph_sel.append(slot)
            return
        if self._sel_n == self._sel_dev.shape[0]:
            # ring full (long epochs x many buckets): flush to the host -- one
            # sync per 8192 bucket-steps, nothing is overwritten
            self._sel_host.extend(tuple(int(v) for v in x) for x in self._sel_dev.cpu().tolist())
            self._sel_n = 0
        self._sel_dev[self._sel_n].copy_(hdr.view(-1)[:2], non_blocking=True)
        self._sel_n += 1

    _Q_RING = 4096   # selection-quality rows held on the device between drains

    def _sample_quality(self, b, k_cap):
        """Score bucket ``b``'s record against the exact top-k of its
        accumulator (residual + record), on the stream it was compressed on;
        the float64[8] block lands in the next ring row (no sync)."""
        if self._is_cuda and torch.cuda.is_current_stream_capturing():
            if not self._q_capture_logged:
                self._q_capture_logged = True
                logger.warning("selection_quality_every=%d: sampling is skipped while a HIP graph captures "
                               "(captured steps are not sampled)", self._quality_every)
            return
        if self._q_dev is None:
            self._q_dev = torch.zeros(self._Q_RING, len(ops.QUALITY_FIELDS), dtype=torch.float64, device=self._device)
        if len(self._q_meta) == self._q_dev.shape[0]:
            # ring full: flush to the host -- one sync per _Q_RING bucket-steps
            self._q_host.extend(self._decode_quality(self._q_dev.cpu().tolist()))
            self._q_meta = []
        ws = b.extra.get("quality_ws")
        if ws is None and self._is_cuda:
            ws = b.extra["quality_ws"] = ops.quality_workspace(self._device)
        k = self._compression.k_of(b.numel, self.get_current_density(b.name))
        with trace.range("gk/b%d/quality" % b.index):
            ops.selection_quality_(b.slice(self._arena.residuals), b.bufs.record, max(int(k), 1), k_cap,
                                   self._q_dev[len(self._q_meta)], ws)
        self._q_meta.append((self.train_iter, b.index, k_cap))

    def _decode_quality(self, rows) -> List[dict]:
        out = []
        for (it, bi, k_cap), row in zip(self._q_meta, rows):
            d = {"iter": it, "bucket": bi}
            d.update(ops.decode_quality(row, k_cap))
            out.append(d)
        return out

    def collect_selection_quality(self) -> List[dict]:
        """Selection-quality rows sampled since the last call (one D2H copy):
        one dict per sampled (iter, bucket) with the fields of
        ``ops.selection_quality_`` and the derived ``record_occupancy``,
        ``topk_overlap``, ``energy_captured`` and ``energy_fraction``.  Call
        it between steps (after ``step()``), like the selected-count drain."""
        n = len(self._q_meta)
        rows = self._decode_quality(self._q_dev[:n].cpu().tolist()) if n else []
        out = self._q_host + rows
        self._q_host = []
        self._q_meta = []
        return out

    def selection_quality_summary(self, rows: Optional[List[dict]] = None) -> dict:
        """Means of the four metrics over ``rows`` (default: the rows since the
        last collect) and ``compression_ratio_used``: dense fp32 gradient bytes
        over the 8 bytes (index + value) of every entry actually sent per
        step.  Empty when nothing was sampled."""
        rows = self.collect_selection_quality() if rows is None else rows
        if not rows:
            return {}
        out = {m: float(np.mean([r[m] for r in rows]))
               for m in ("record_occupancy", "topk_overlap", "energy_captured", "energy_fraction")}
        sent_per_step = float(np.mean([r["sent"] for r in rows])) * len(self._arena.buckets)
        out["compression_ratio_used"] = int(np.sum(self._sizes)) * 4.0 / (8.0 * sent_per_step) if sent_per_step else 0.0
        return out

    def _queue_dump(self, b, r, rec, k_cap):
        """Sampled gradient dump: acc = r_new + scatter(own record), async D2H."""
        acc = r.clone()
        ops.scatter_add_records_(acc, rec, 1, k_cap, 1.0)
        host = torch.empty(acc.shape, dtype=acc.dtype, pin_memory=self._is_cuda)
        host.copy_(acc, non_blocking=True)
        ev = None
        if self._is_cuda:
            ev = torch.cuda.Event()
            ev.record()
        self._pending_dumps.append((self.train_iter, b, host, ev))

    def _flush_dumps(self):
        if not self._pending_dumps:
            return
        os.makedirs(self._gradient_path, exist_ok=True)
        for it, b, host, ev in self._pending_dumps:
            if ev is not None:
                ev.synchronize()
            arr = self._unpad(b, host).numpy()
            np.save("%s/r%d_gradients_iter_%d" % (self._gradient_path, self._rank, it), arr)
        self._pending_dumps = []

    def _unpad(self, b, flat: torch.Tensor) -> torch.Tensor:
        parts = []
        for k, o in zip(b.keys, b.offsets):
            n = self._named_parameters[k].numel()
            parts.append(flat[o:o + n])
        return torch.cat(parts)

    # ------------------------------------------------------------------
    # synchronize / step
    # ------------------------------------------------------------------
    def synchronize(self):
        with trace.range("gk/synchronize"):
            self._synchronize()

    def _synchronize(self):
        if self._is_cuda:
            streams.join(self._device)   # normally done by the end-of-backward callback already
        if self._hooks_on:
            any_ready = False
            due = [b for b in self._arena.buckets if not b.launched and b.ready > 0]
            if len(due) > 1 and self._fused_sparse and self._sparse and not self._profiling and \
                    all(self.get_current_density(b.name) < 1 for b in due):
                self._launch_group(due)
            else:
                for b in due:
                    self._launch_bucket(b)
            any_ready = any(b.launched for b in self._arena.buckets)
            if self._comm_stream is not None and any_ready:
                cur = torch.cuda.current_stream(self._device)
                for b in self._arena.buckets:
                    if b.launched:
                        cur.wait_event(b.done_event)
            for b in self._arena.buckets:
                if b.launched:
                    b.extra["agg_done"] = False if self._pending_apply else True
                else:
                    # no gradients reached this bucket this step: its gathered
                    # records are from an earlier step and must not be re-applied
                    b.extra["agg"] = None
                    b.extra["agg_done"] = True
                b.ready = 0
                b.launched = False
                b.extra["overlapped"] = False
            self._next_launch = 0
            if any_ready:
                self.train_iter += 1
            self._flush_dumps()
            self._print_profiling()
        else:
            self.train_iter += 1
        self._handles.clear()

    def _print_profiling(self):
        timers = getattr(self, "_pending_timers", None)
        if not self._profiling or not timers:
            return
        for name, t0, t1, t2, t3 in timers:
            perf.force_insert_item(self._compression_timers, name, self._elapsed(t0, t1))
            perf.force_insert_item(self._allreduce_timers, name, self._elapsed(t1, t2))
            perf.force_insert_item(self._update_times, name, self._elapsed(t2, t3))
        self._pending_timers = []
        first = next(iter(self._allreduce_timers), None)
        if rank() == 0 and first is not None and len(self._allreduce_timers[first]) >= 40:
            tcp = sum(float(np.mean(v)) for v in self._compression_timers.values())
            tar = sum(float(np.mean(v)) for v in self._allreduce_timers.values())
            tup = sum(float(np.mean(v)) for v in self._update_times.values())
            logger.info("[%d]: Total compress: %f, allreduce: %f, update: %f, total: %f", rank(), tcp, tar, tup,
                        tcp + tar + tup)
            self._compression_timers.clear()
            self._allreduce_timers.clear()
            self._update_times.clear()

    def clip_grad_norm_(self, max_norm: float) -> torch.Tensor:
        """Global-norm clip over the gradient arena on device (no host sync)."""
        self._materialize()
        return ops.clip_grad_norm_(self._arena.grads, max_norm)

    def aggregated_grads(self) -> torch.Tensor:
        """The averaged gradient arena (``p.grad`` views) after ``synchronize()``.

        Under momentum correction with sparse apply the aggregate normally
        stays in the gathered records; this scatters it into the arena (and
        the following ``step()`` then runs the dense update)."""
        self._materialize()
        return self._arena.grads

    def _sparse_apply_ok(self) -> bool:
        if not (self._sparse_apply_opt and self._fused_kind == "sgd"):
            return False
        lrs = {float(g["lr"]) for g in self.param_groups}
        return len(lrs) == 1

    def _materialize(self) -> None:
        if not self._pending_apply:
            return
        with torch.no_grad():
            for b in self._arena.buckets:
                agg = b.extra.get("agg")
                if agg is not None and not b.extra.get("agg_done", False):
                    gathered, P, k_cap = agg
                    ops.scatter_add_records_(b.slice(self._arena.grads), gathered, P, k_cap, 1.0 / P, True)
                    b.extra["agg_done"] = True
        self._pending_apply = False

    def _setup_fused_update(self):
        self._fused_kind = None
        self._adam_capable = False    # "adam" was chosen here (it may be dropped and restored with the state)
        base = self._base_cls
        if not self._fused_optim or base is None:
            return
        from ..optim.lamb import LAMB
        from ..optim.lars import LARS
        in_arena = all(p in self._parameter_names for g in self.param_groups for p in g["params"]
                       if p.requires_grad)
        if not in_arena or len(self.param_groups) > 8:
            return
        if base is torch.optim.SGD:
            if any(g.get("maximize", False) for g in self.param_groups):
                return
            self._fused_kind = "sgd"
        elif base is LARS:
            self._fused_kind = "lars"
        elif base in (torch.optim.Adam, torch.optim.AdamW):
            # eps <= 0: the all-zero padding slots would become 0 / 0 (torch has no padding)
            if any(g.get("amsgrad", False) or g.get("maximize", False) or g.get("differentiable", False)
                   or not float(g["eps"]) > 0.0 for g in self.param_groups):
                return
            self._fused_kind = "adam"
            self._adam_capable = True
            # the step count of every parameter: one device scalar (torch's capturable convention)
            self._adam_step = torch.zeros((), dtype=torch.float32, device=self._device)
        elif base is LAMB:
            # Adam's state (one device step scalar, both moment arenas) with another update
            self._fused_kind = "lamb"
            self._adam_capable = True
            self._adam_step = torch.zeros((), dtype=torch.float32, device=self._device)
        else:
            return
        self._adam_kind = self._fused_kind    # what load_state_dict / broadcast_state restore
        group_of_key = {}
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                if p in self._parameter_names:
                    group_of_key[self._parameter_names[p]] = gi
        segs = self._arena.segments(group_of_key)
        self._chunks = ops.make_chunk_table(segs, self._device)
        # per-bucket [begin, count) ranges of the chunk table (segments are in bucket order)
        self._bucket_chunks = []
        self._chunk_list = []
        pos = 0
        seg_at = {sg[0]: sg for sg in segs}
        for b in self._arena.buckets:
            begin = pos
            for o in b.offsets:
                start = b.start + o
                seg = seg_at[start]
                off = 0
                while off < seg[1]:
                    ln = min(ops.CHUNK_ELEMS, seg[1] - off)
                    self._chunk_list.append((start + off, ln, seg[2], seg[3]))
                    off += ln
                    pos += 1
            self._bucket_chunks.append((begin, pos - begin))
        self._nseg = sum(len(b.keys) for b in self._arena.buckets)
        self._group_first = [True] * len(self.param_groups)
        if self._fused_kind == "lars":
            self._seg_sumsq = torch.zeros(2 * self._nseg, dtype=torch.float64, device=self._device)
        elif self._fused_kind == "lamb":
            self._lamb_ws = ops.make_lamb_workspace(self._chunks, self._device)
            # segment ids follow arena.segments(): bucket by bucket, key by key
            self._lamb_seg_names = [k for b in self._arena.buckets for k in b.keys]

    def _adopt_state(self):
        """Point optimizer state at arena views (after first step / load_state_dict)."""
        arena = self._arena
        if self._fused_kind == "sgd":
            if not any(g["momentum"] != 0 for g in self.param_groups):
                return
            m = arena.ensure_momentum(0.0)
            for gi, g in enumerate(self.param_groups):
                has_all = True
                for p in g["params"]:
                    if p not in self._parameter_names:
                        continue
                    key = self._parameter_names[p]
                    view = arena.view_of(m, key)
                    st = self.state[p]
                    buf = st.get("momentum_buffer")
                    if buf is None:
                        has_all = False
                    elif buf.data_ptr() != view.data_ptr():
                        view.copy_(buf)
                    st["momentum_buffer"] = view
                if has_all:
                    self._group_first[gi] = False
        elif self._fused_kind == "lars":
            m = arena.momentum
            if m is None:
                m = arena.ensure_momentum(1.0)
            for p in [p for g in self.param_groups for p in g["params"]]:
                if p not in self._parameter_names:
                    continue
                key = self._parameter_names[p]
                view = arena.view_of(m, key)
                st = self.state[p]
                buf = st.get("acceleration")
                if buf is not None and buf.data_ptr() != view.data_ptr():
                    view.copy_(buf)
                st["acceleration"] = view
        elif self._fused_kind in ("adam", "lamb"):
            params = [p for g in self.param_groups for p in g["params"] if p in self._parameter_names]
            shared = self._adam_step
            # step counts handed in (factory / load_state_dict); a parameter without state has taken none
            steps = set()
            for p in params:
                s = self.state[p].get("step")
                if s is None:
                    steps.add(0.0)
                elif not (torch.is_tensor(s) and s.data_ptr() == shared.data_ptr()):
                    steps.add(float(s))
            if len(steps) > 1:
                # one bias correction per launch: parameters at different steps keep torch's own update
                logger.warning("Adam state with different per-parameter step counts %s: unfused torch update",
                               sorted(steps))
                self._fused_kind = None
                self._state_dirty = False
                return
            if steps:
                shared.fill_(steps.pop())
            m = arena.ensure_momentum(0.0)
            v = arena.ensure_second_moment()
            for p in params:
                key = self._parameter_names[p]
                st = self.state[p]
                for name, ar in (("exp_avg", m), ("exp_avg_sq", v)):
                    view = arena.view_of(ar, key)
                    buf = st.get(name)
                    if buf is not None and buf.data_ptr() != view.data_ptr():
                        view.copy_(buf)
                    st[name] = view
                st["step"] = shared
        self._state_dirty = False

    def _adam_decoupled(self, g) -> bool:
        return self._base_cls is torch.optim.AdamW or bool(g.get("decoupled_weight_decay", False))

    def _fused_step(self):
        arena = self._arena
        if not self._mc_applied and (self._state_dirty or arena.momentum is None):
            self._adopt_state()
        arena.reattach()
        if self._fused_kind == "sgd" and self._mc_applied and self._pending_apply:
            # momentum + weight decay were applied locally before sparsification
            # and the aggregate is still in the records: sparse SGD straight from
            # them (w[idx] -= lr * avg; bf16 shadow refreshed at idx).  The
            # gradient arena was zeroed by the compressor and stays zero.
            lr = float(self.param_groups[0]["lr"])
            shadow = getattr(arena, "shadow", None)
            for b in arena.buckets:
                agg = b.extra.get("agg")
                if agg is None or b.extra.get("agg_done", False):
                    continue
                gathered, P, k_cap = agg
                ops.apply_records_sgd_(b.slice(arena.weights), b.slice(shadow) if shadow is not None else None,
                                       gathered, P, k_cap, 1.0 / P, lr, self._lr_mult)
                b.extra["agg_done"] = True
            self._pending_apply = False
            self._mc_applied = False
        elif self._fused_kind == "sgd" and self._mc_applied:
            # momentum + weight decay were applied locally before sparsification
            groups = [{"lr": g["lr"], "momentum": 0.0, "dampening": 0.0, "weight_decay": 0.0, "nesterov": False,
                       "first_step": False} for g in self.param_groups]
            ops.fused_sgd_(arena.weights, None, arena.grads, self._chunks, groups, zero_grad=self._zero_grad_in_step,
                           w_bf16=getattr(arena, "shadow", None), lr_mult=self._lr_mult)
            self._mc_applied = False
        elif self._fused_kind == "sgd":
            groups = []
            for gi, g in enumerate(self.param_groups):
                groups.append({"lr": g["lr"], "momentum": g["momentum"], "dampening": g.get("dampening", 0.0),
                               "weight_decay": g.get("weight_decay", 0.0), "nesterov": g.get("nesterov", False),
                               "first_step": self._group_first[gi] and g["momentum"] != 0})
            ops.fused_sgd_(arena.weights, arena.momentum, arena.grads, self._chunks, groups,
                           zero_grad=self._zero_grad_in_step, w_bf16=getattr(arena, "shadow", None),
                           lr_mult=self._lr_mult)
            if any(self._group_first):
                self._group_first = [False] * len(self._group_first)
                self._adopt_state()
        elif self._fused_kind == "lamb":
            # the step tick, the moments with per-chunk norm partials, one wave per tensor for the
            # trust ratio, the update: launch boundaries only, so a captured graph replays it as it is
            groups = [{"lr": g["lr"], "betas": g["betas"], "eps": g["eps"], "weight_decay": g.get("weight_decay", 0.0),
                       "adapt": g.get("adapt", True), "trust_clip": g.get("trust_clip")} for g in self.param_groups]
            ops.fused_lamb_(arena.weights, arena.momentum, arena.second_moment, arena.grads, self._chunks, groups,
                            self._adam_step, self._lamb_ws, zero_grad=self._zero_grad_in_step,
                            w_bf16=getattr(arena, "shadow", None), lr_mult=self._lr_mult)
        elif self._fused_kind == "adam":
            # one tick of the device step count + one update launch; the bias
            # corrections are derived on the device, so this is also what a
            # captured graph replays
            groups = [{"lr": g["lr"], "betas": g["betas"], "eps": g["eps"], "weight_decay": g.get("weight_decay", 0.0),
                       "decoupled": self._adam_decoupled(g)} for g in self.param_groups]
            ops.fused_adam_(arena.weights, arena.momentum, arena.second_moment, arena.grads, self._chunks, groups,
                            self._adam_step, zero_grad=self._zero_grad_in_step,
                            w_bf16=getattr(arena, "shadow", None), lr_mult=self._lr_mult)
        else:
            self._seg_sumsq.zero_()
            ops.segmented_sumsq_(arena.weights, arena.grads, self._chunks, self._seg_sumsq)
            groups = [{"lr": g["lr"], "momentum": g["momentum"], "weight_decay": g["weight_decay"],
                       "eeta": g["eeta"], "epsilon": g["epsilon"]} for g in self.param_groups]
            ops.fused_lars_(arena.weights, arena.momentum, arena.grads, self._chunks, self._seg_sumsq, groups)
            if self._zero_grad_in_step:
                ops.fill_zero_(arena.grads)
            self.refresh_shadow()
        self._grads_zero = self._zero_grad_in_step

    def describe_state(self) -> str:
        """Bucket readiness / launch state (for the hang watchdog)."""
        lines = ["rank %d/%d iter %d epoch %d local=%s" % (self._rank, self._world, self.train_iter,
                                                          self.train_epoch, self.local)]
        for b in self._arena.buckets:
            lines.append("  bucket %d: %d/%d params ready, launched=%s, numel=%d" % (
                b.index, b.ready, len(b.params), b.launched, b.numel))
        return "\n".join(lines)

    def step(self, closure=None):
        if self._watchdog is not None:
            self._watchdog.kick()
        if self._exchanger is not None:
            self._exchanger.check()   # native engine: raise if its watchdog aborted a hung collective
        if not self.local:
            self.synchronize()
        if self._fused_kind in ("adam", "lamb") and (self._state_dirty or self._arena.second_moment is None):
            with torch.no_grad():
                self._adopt_state()    # may fall back to the unfused update (differing step counts)
        if self._fused_kind is not None:
            loss = None
            if closure is not None:
                with torch.enable_grad():
                    loss = closure()
            with torch.no_grad(), trace.range("gk/update"):
                self._fused_step()
            return loss
        self._grads_zero = False
        loss = super(self.__class__, self).step(closure)
        self.refresh_shadow()
        return loss

    def zero_grad(self, set_to_none: bool = True):
        """Gradients are views of the arena: zero it (never set to None).

        With readiness hooks installed the arena is known to be clean after a
        fused step (which zeroes it) until a hook fires, so the fill is skipped."""
        if self._grads_zero and self._hooks_on:
            return
        with torch.no_grad():
            ops.fill_zero_(self._arena.grads)
        self._grads_zero = True

    def state_dict(self):
        sd = super(self.__class__, self).state_dict()
        if self._fused_kind in ("adam", "lamb"):
            # every state[p]["step"] is the one device scalar: hand out one counter
            # per parameter, as a plain torch.optim.Adam(W) that loads this expects
            sd["state"] = {k: ({**st, "step": st["step"].clone()} if torch.is_tensor(st.get("step")) else st)
                           for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super(self.__class__, self).load_state_dict(state_dict)
        self._state_dirty = True
        if self._adam_capable:
            self._fused_kind = self._adam_kind    # the new state decides again (differing step counts drop it)
        if self._fused_kind is not None:
            with torch.no_grad():
                self._adopt_state()

    # ------------------------------------------------------------------
    # checkpoint helpers (residuals are per rank)
    # ------------------------------------------------------------------
    def compression_state(self) -> dict:
        st = {"train_epoch": self.train_epoch, "train_iter": self.train_iter}
        if self._arena.residuals is not None:
            st["residuals"] = {b.name: self._unpad(b, b.slice(self._arena.residuals)).detach().cpu()
                               for b in self._arena.buckets}
        if getattr(self._arena, "velocity", None) is not None:
            st["velocity"] = {b.name: self._unpad(b, b.slice(self._arena.velocity)).detach().cpu()
                              for b in self._arena.buckets}
        return st

    def load_compression_state(self, st: dict) -> None:
        self.train_epoch = int(st.get("train_epoch", self.train_epoch))
        self.train_iter = int(st.get("train_iter", self.train_iter))
        self._plan_check_due = True
        for key, arena_t in (("residuals", self._arena.residuals),
                             ("velocity", getattr(self._arena, "velocity", None))):
            res = st.get(key)
            if not res or arena_t is None:
                continue
            with torch.no_grad():
                for b in self._arena.buckets:
                    if b.name not in res:
                        continue
                    flat = res[b.name].to(self._device)
                    dst = b.slice(arena_t)
                    pos = 0
                    for k, o in zip(b.keys, b.offsets):
                        n = self._named_parameters[k].numel()
                        dst[o:o + n].copy_(flat[pos:pos + n])
                        pos += n

    def broadcast_state(self, root_rank: int = 0) -> None:
        """Make the REPLICATED optimizer state identical on every rank after a
        resume: the density-schedule / iteration position (``train_epoch``,
        ``train_iter``) and the global momentum (or LARS acceleration, or Adam
        moment) buffers and Adam's step count are taken from ``root_rank``.
        Per-rank state -- error-feedback residuals and DGC local velocities --
        is NOT touched: every rank loads its own (``load_compression_state``).

        The reference restores only rank 0's weights and epoch / iteration
        (dist_trainer.py:26-33,57; dl_trainer.py:285-290), so its resume is
        lossy but consistent; restoring momentum on rank 0 alone would make the
        replicas diverge, and a density epoch that differs between ranks gives
        records of different sizes inside one all-gather."""
        dev = self._device
        pos = torch.tensor([self.train_epoch, self.train_iter], dtype=torch.int64,
                           device=dev if comm.backend() == "nccl" else "cpu")
        pos = broadcast(pos, root_rank)
        self.train_epoch, self.train_iter = int(pos[0]), int(pos[1])
        self._plan_check_due = True
        if self._world <= 1 and comm.backend() != "loopback":
            return
        if self._adam_capable:
            # before the local kind is looked at: a rank that dropped to the unfused
            # update on its own state must still enter the root's collectives
            self._broadcast_adam_state(root_rank)
            return
        kind = self._fused_kind
        if kind is None:
            broadcast_optimizer_state(self, root_rank)
            return
        key = "momentum_buffer" if kind == "sgd" else "acceleration"
        # per param group: does the root hold the buffer of every parameter?
        have = [all(key in self.state.get(p, {}) for p in g["params"] if p in self._parameter_names)
                and (kind != "sgd" or g["momentum"] != 0) for g in self.param_groups]
        have = broadcast_object(have, root_rank)
        if not any(have):
            return
        with torch.no_grad():
            if self._state_dirty or self._arena.momentum is None:
                self._adopt_state()    # root: buffers -> arena views; others: a zero arena
            m = self._arena.momentum
            if m is None:
                m = self._arena.ensure_momentum(0.0 if kind == "sgd" else 1.0)
            broadcast_(m, root_rank)   # the whole momentum arena: one collective
            for gi, g in enumerate(self.param_groups):
                if not have[gi]:
                    continue
                for p in g["params"]:
                    if p in self._parameter_names:
                        self.state[p][key] = self._arena.view_of(m, self._parameter_names[p])
                self._group_first[gi] = False
        self._state_dirty = False

    def _broadcast_adam_state(self, root_rank: int) -> None:
        """Both moment arenas and the device step count from the root (two
        arena collectives and one scalar); every rank's state entries are views
        of those arenas (``_adopt_state``), so they follow."""
        params = [p for g in self.param_groups for p in g["params"] if p in self._parameter_names]
        have = all("exp_avg" in self.state.get(p, {}) for p in params)
        have = broadcast_object(have, root_rank)
        if not have:
            return
        with torch.no_grad():
            if self._rank != root_rank:
                for p in params:           # the root's state replaces whatever this rank held,
                    self.state.pop(p, None)
                self._fused_kind = self._adam_kind  # and with it this rank's own reason to run unfused
                self._state_dirty = True
            if self._fused_kind == self._adam_kind and (self._state_dirty or self._arena.second_moment is None):
                self._adopt_state()    # root: buffers -> arena views; others: zero arenas
            # the root's kind decides for every rank: one sequence of collectives
            if not broadcast_object(self._fused_kind == self._adam_kind, root_rank):
                # the root's parameters are at different steps: every rank keeps torch's update
                if self._fused_kind == self._adam_kind:
                    self._fused_kind = None
                    for p in params:
                        self.state[p]["step"] = self.state[p]["step"].clone()
                broadcast_optimizer_state(self, root_rank)
                return
            broadcast_(self._arena.momentum, root_rank)
            broadcast_(self._arena.second_moment, root_rank)
            broadcast_(self._adam_step.view(1), root_rank)
        self._state_dirty = False

    def trust_ratios(self) -> Dict[str, torch.Tensor]:
        """LAMB's trust ratio of every parameter at the last fused step: name ->
        0-d fp32 view of the device buffer (no host sync until a value is read;
        all ones before the first step)."""
        if self._fused_kind != "lamb":
            raise RuntimeError("trust_ratios() needs the fused LAMB update (optim.LAMB in DistributedOptimizer)")
        return {name: self._lamb_ws.trust[i] for i, name in enumerate(self._lamb_seg_names)}

    @property
    def arena(self) -> GradArena:
        return self._arena


def DistributedOptimizer(optimizer, named_parameters=None, compression=None, is_sparse=False, density=0.001,
                         seq_layernames=None, layerwise_times=None, norm_clip=None, threshold=0, writer=None,
                         gradient_path=None, **gk_options):
    """Wrap ``optimizer`` for compressed data-parallel training.

    Same positional/keyword API as the reference (distributed_optimizer.py:550).
    Extra keyword options (MI355X build): ``compress_single_rank``,
    ``deterministic``, ``fused_optimizer``, ``zero_grad_in_step``, ``overlap``,
    ``density_warmup`` (True | False | list), ``native_rccl``, ``profiling``,
    ``planner_preset`` ('mi355x' | 'reference'), ``selection_quality_every``
    (N > 0: every N-th step each fused sparse bucket's record is scored
    against the exact top-k of its accumulator on device, rows from
    ``collect_selection_quality()``; default ``GKSGD_SELECTION_QUALITY_EVERY``
    or 0 = off; steps captured into a HIP graph are not sampled).
    """
    from ..compression import compressors
    if compression is None or isinstance(compression, str):
        compression = compressors[compression]
    cls = type(optimizer.__class__.__name__, (optimizer.__class__,), dict(_DistributedOptimizer.__dict__))
    gk_options = dict(gk_options)
    gk_options["defaults"] = dict(optimizer.defaults)
    gk_options["base_cls"] = optimizer.__class__
    inst = cls(optimizer.param_groups, named_parameters, compression, is_sparse, density,
               seq_layernames=seq_layernames, layerwise_times=layerwise_times, norm_clip=norm_clip,
               threshold=threshold, writer=writer, gradient_path=gradient_path, _gk_opts=gk_options)
    for p, st in optimizer.state.items():
        if st:
            inst.state[p] = st
            inst._state_dirty = True
    return inst
