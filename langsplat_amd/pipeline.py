"""Software pipeline of LangSplat's language step across views (train.py:76-138 with include_feature).

In the language step every geometry parameter is frozen (scene/gaussian_model.py:203-217): the next
view's preprocess, depth order and binning (~200 us at C3) read nothing the current step's
backward, gradient all-reduce or Adam writes.  Only the language feature changes, and the rasterizer
can take it late (include/lsr.h lsr_forward_args.language_ready: the geometry stages run at once,
the compositing waits for an event).  So the views of consecutive steps run on two alternating HIP
streams:

    stream A:  geometry(k) -> [wait update(k-1)] -> render(k) + loss -> backward(k) -> [all-reduce] -> Adam(k)
    stream B:                                                 geometry(k+1) -> [wait update(k)] -> render(k+1) ...

and view k+1's geometry stages fill the CUs that view k's render backward leaves idle in its tail
(its longest tiles run alone at the end) and that the all-reduce and Adam leave idle.  Every step
computes exactly what the serial loop computes, in the same order per parameter: view k+1 composites
with the feature Adam(k) wrote.  Autograd runs a node's backward on its forward's stream, so the
backward of view k stays on stream A without further plumbing.

    pipe = ViewPipeline(optimizer)                  # optimizer: langsplat_amd.optim.Adam (or torch's)
    for cam in views:
        with pipe.step():
            loss = render(cam, gaussians, pipe_params, bg, opt, language_target=(gt, mask))["language_l1"]
            loss.backward()
            pipe.update()                           # [all-reduce,] Adam, zero_grad(set_to_none=True)
    pipe.synchronize()                              # before reading the parameters on another stream

A step's tensors (the loss, the images) live on that step's stream: `.item()` is safe anywhere;
using them in device work on another stream needs `pipe.synchronize()` first.  Do not keep a step's
loss (its autograd graph) alive into the next step: the parameters' AccumulateGrad nodes would then
stay bound to the previous step's stream.
"""
from __future__ import annotations

import contextlib
import os

import torch

from . import _native
from .distributed import collective_capturable
from .graph import (_as_view, _fused_tail_enabled, _nullctx, capture_key, current_params, graph_capture,
                    release_stale_accumulators, resolve_bucket)


# LSR_PG_NATIVE_LAUNCH=0: every replay through torch's stream context and CUDAGraph.replay() (A/B)
_NATIVE_LAUNCH = os.environ.get("LSR_PG_NATIVE_LAUNCH", "1") != "0"

class ViewPipeline:
    def __init__(self, optimizer, bucket=None, device=None):
        """optimizer: steps the trainable parameters; bucket: a langsplat_amd.distributed.GradBucket
        whose all-reduce precedes the optimizer at N > 1 (None at N = 1)."""
        self.optimizer = optimizer
        self.bucket = bucket
        self.streams = (torch.cuda.Stream(device), torch.cuda.Stream(device))
        self.k = 0
        self.ready = None       # event after the last update (the next forward waits for it)
        self._in_step = False

    @contextlib.contextmanager
    def step(self):
        """One view's step on this step's stream; its rasterizer forward defers the language feature
        until the previous step's update has landed."""
        if self._in_step:
            raise RuntimeError("ViewPipeline.step() blocks do not nest")
        s = self.streams[self.k & 1]
        # whatever the caller enqueued on its own stream before this step (parameter surgery,
        # learning-rate changes done on the device, ...) happens first
        s.wait_stream(torch.cuda.current_stream())
        self._in_step = True
        try:
            with torch.cuda.stream(s), _native.language_ready(self.ready):
                yield s
        finally:
            self._in_step = False
            self.k += 1

    def update(self, average: bool = True):
        """Inside step(), after loss.backward(): the gradient all-reduce (N > 1), the optimizer step and
        zero_grad, on this step's stream; the next step's compositing waits for them."""
        if not self._in_step:
            raise RuntimeError("ViewPipeline.update() belongs inside a step() block")
        if self.bucket is not None:
            self.bucket.all_reduce(average=average)
        self.optimizer.step()
        if self.bucket is not None and not self.bucket.direct:
            self.bucket.zero()
        else:
            self.optimizer.zero_grad(set_to_none=True)
        ev = torch.cuda.Event()
        ev.record()
        self.ready = ev

    def synchronize(self):
        """The caller's current stream waits for every step enqueued so far."""
        cur = torch.cuda.current_stream()
        for s in self.streams:
            cur.wait_stream(s)


class ViewCache:
    """The bookkeeping of PipelinedGraphStep's view cache: which views have a pack (include/lsr.h
    lsr_view_save), which buffer sets hold a geometry result that could still be saved, the byte
    budget and the parameter stamp the packs were made under.  It enqueues nothing itself: `native`
    does (PipelinedGraphStep's _ViewNative, or a stand-in in tests), with

        native.pack_bytes(num_rendered) -> int         bytes of a pack of that many tile instances
        native.alloc(nbytes) -> pack                   device memory for one pack
        native.save(r, num_rendered, pack)             set r's geometry into the pack (stream B)
        native.pack_bytes_without_plan(num_rendered)   optional: a smaller pack, tried when pack_bytes'
                                                       (which has room for the view's walk plan) is over budget
        native.restore(r, num_rendered, pack)          the pack into set r (stream B)

    and, for the bound form (include/lsr.h lsr_view_bind: the set reads the pack in place),

        native.can_bind() -> bool                      the library has lsr_view_bind and the step's graphs
                                                       were captured against the sets' tables
        native.bind(r, num_rendered, pack)             set r bound to the pack (stream B)
        native.step_done(r) -> bool                    set r's last enqueued step has finished

    A hit then enqueues a bind in place of the restore; without can_bind (or when it says no) the
    copying restore stays.  A bound set's composite and backward read the pack on stream A long
    after the bind was enqueued, so the cache keeps a reference to the pack a set is bound to
    (`bound`) whatever happens to `packs` -- invalidate() included -- until the set is next visited,
    and from then (`retired`) until the set's step event has completed.  One pack may be bound into
    several sets at once (binds only read it).

    A view's key is any hashable; `ref` is kept with it (the camera object: its id stays unique while
    the cache holds it).  There is no eviction: an epoch is a permutation of the views, so LRU would
    miss every time; once the budget is full the remaining views keep running their geometry graph."""

    RENDERED, OVERFLOW = 1, 7  # counter slots (csrc/lsr_internal.h kCntRendered, kCntOverflow)

    def __init__(self, sets: int, budget_bytes: int, native):
        self.native = native
        can = getattr(native, "can_bind", None)
        self.bind = bool(can()) if can is not None else False
        self.bound = [None] * sets      # per set: the pack its table names
        self.retired = []               # (set, pack): no longer bound, its set's step may still read it
        self.budget = int(budget_bytes)
        self.packs = {}                 # key -> (ref, num_rendered, pack, nbytes)
        self.pending = [None] * sets    # per set: (key, ref, event, host counters) of a geometry graph's result
        self.stamp = None
        self.off = False                # disable(): nothing is saved or hit any more
        self.bytes = self.hits = self.misses = self.drops = 0

    def invalidate(self):
        """Drop every pack, and every set's claim to hold a result worth saving.  (A set bound to a
        dropped pack keeps its reference, and goes on to composite the geometry it was given, as a
        set that holds a restored copy does.)"""
        if self.packs:
            self.drops += 1
        self.packs.clear()
        self.pending = [None] * len(self.pending)
        self.bytes = 0

    def disable(self):
        """No view is cached from here on (a geometry tensor became trainable): every pack is dropped,
        every visit is a miss and nothing is saved.  The cache object stays, because `bound` and
        `retired` must: sets bound ahead still read their packs in steps not yet enqueued."""
        self.invalidate()
        self.off = True

    def check(self, stamp):
        """The geometry tensors' (data_ptr, _version) stamp at this replay: another one than the packs
        were made under drops them (and what the sets hold was computed before the change)."""
        if stamp != self.stamp:
            if self.stamp is not None:
                self.invalidate()
            self.stamp = stamp

    def computed(self, r, key, ref, event, host):
        """Set r's geometry graph was just enqueued for view `key`; `event` follows the copy of its
        counter slots into `host` (pinned).  Nothing is pending for a view that has a pack."""
        self.pending[r] = None if self.off or key in self.packs else (key, ref, event, host)

    def visit(self, r, key) -> bool:
        """Set r is about to receive view `key` (its last reader is done, on stream B's order).  First
        the view it holds is saved, if its counters have arrived (no wait: an event not yet signalled
        skips this visit), it fitted its capacities and the budget allows.  True: `key` has a pack and
        its restore was enqueued in place of the geometry graph."""
        self.save_pending(r)
        return self.restore(r, key)

    def save_pending(self, r) -> bool:
        """visit()'s first half: the view set r holds into a pack, under visit()'s conditions; True if
        it was saved.  Either way the set's claim is spent."""
        pend, self.pending[r] = self.pending[r], None
        if pend is not None and not self.off and pend[0] not in self.packs and pend[2].query():
            pkey, ref, _, host = pend
            if int(host[self.OVERFLOW]) == 0:
                rendered = int(host[self.RENDERED])
                nbytes = self.native.pack_bytes(rendered)
                small = getattr(self.native, "pack_bytes_without_plan", None)
                if self.bytes + nbytes > self.budget and small is not None:
                    # no room for the view's walk plan: a pack that ends after the geometry (a hit on
                    # it is the plain bound form) still saves the geometry phase
                    nbytes = small(rendered)
                if self.bytes + nbytes <= self.budget:
                    pack = self.native.alloc(nbytes)
                    self.native.save(r, rendered, pack)
                    self.packs[pkey] = (ref, rendered, pack, nbytes)
                    self.bytes += nbytes
                    return True
        return False

    def restore(self, r, key) -> bool:
        """visit()'s second half: True if `key` has a pack, whose restore into set r was enqueued in
        place of the geometry graph (counted as a hit, else as a miss)."""
        hit = self.packs.get(key)
        if hit is None:
            self.misses += 1
            self._unbind(r)  # (the geometry graph gives the set its own arrays again)
            return False
        if self.bind:
            if self.bound[r] is not hit[2]:
                self._unbind(r)
            self.native.bind(r, hit[1], hit[2])
            self.bound[r] = hit[2]
        else:
            self.native.restore(r, hit[1], hit[2])
        self.hits += 1
        return True

    def _unbind(self, r):
        """Set r is about to get other geometry: the pack it was bound to is kept until the set's last
        enqueued step (its last reader) has finished; the retired ones whose step has are let go."""
        if self.bound[r] is not None:
            self.retired.append((r, self.bound[r]))
            self.bound[r] = None
        if self.retired:
            self.retired = [(q, pack) for q, pack in self.retired if not self.native.step_done(q)]

    def stats(self):
        return {"hits": self.hits, "misses": self.misses, "packs": len(self.packs), "bytes": self.bytes,
                "drops": self.drops}


class _ViewNative:
    """ViewCache's device side for one PipelinedGraphStep: packs are uint8 tensors, save and restore go
    to stream B with each (set, pack)'s lsr_view_args built once.  It holds the step's buffer sets and
    stream, not the step: no reference cycle, so a step's graphs and packs are freed when its last
    reference goes (not by a later garbage collection, which could run inside a graph capture)."""

    def __init__(self, sets, stream, device, bound=False, readers=(), ev_step=()):
        self.sets, self.stream, self.device = sets, stream, device
        self.bound = bool(bound)   # the step's graphs read the sets' tables (lsr_view_bind)
        self.readers = readers     # the streams whose kernels read a bound pack in place (stream A)
        self.ev_step = ev_step     # the step's per-set events (the list: no reference to the step)
        self.args = {}  # (set, pack address and size, tile instances) -> LsrViewArgs
        call = sets[0].geometry_call
        self.dims = (call["P"], call["W"], call["H"])

    def pack_bytes(self, rendered):
        # bound: with room for the view's walk plan, which a hit then reads in place too
        if self.bound and _native.has_view_plan():
            return _native.view_plan_pack_bytes(*self.dims, rendered)
        return _native.view_pack_bytes(*self.dims, rendered)

    def pack_bytes_without_plan(self, rendered):
        return _native.view_pack_bytes(*self.dims, rendered)

    def alloc(self, nbytes):
        pack = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
        pack.record_stream(self.stream)  # used on stream B, whatever stream allocates it
        for s in self.readers:           # ... and, bound, read in place by the steps on stream A
            pack.record_stream(s)
        return pack

    def _args(self, r, rendered, pack):
        key = (r, pack.data_ptr(), pack.numel(), rendered)
        a = self.args.get(key)
        if a is None:
            a = self.args[key] = _native.view_args(self.sets[r], rendered, pack)
        return a

    def save(self, r, rendered, pack):
        _native.view_save(self._args(r, rendered, pack), self.stream)

    def restore(self, r, rendered, pack):
        _native.view_restore(self._args(r, rendered, pack), self.stream)

    def can_bind(self):
        return self.bound and _native.has_view_bind()

    def bind(self, r, rendered, pack):
        # (the language step reads no clamped bits: lsr_view_bind's LSR_BIND_CLAMPED stays off)
        _native.view_bind(self._args(r, rendered, pack), self.stream)

    def step_done(self, r):
        return self.ev_step[r].query()


class PipelinedGraphStep:
    """ViewPipeline's order as HIP graphs on two streams: the geometry stages of a later view run on
    stream B while view k's compositing, loss, backward and Adam run on stream A, with no host work
    between the kernels (langsplat_amd.graph.GraphedStep is the unpipelined form).

    The rasterizer forward is split in two calls (include/lsr.h lsr_forward_args.phase, capacity
    mode): the geometry half (preprocess, depth order, binning; the language feature deferred) and
    the composite half (the feature into the records, compositing, fused loss).  Per static buffer
    set p (_native.static_buffers: the same addresses at every forward; S sets, default 3) the graphs

        G_geo[p]:  the geometry half of the view, into set p                  (stream B)
        G_comp[p]: the composite half of set p and the loss, then loss.backward() and
                   optimizer.step(skip=overflow[p])                             (stream A)
                   (N > 1: the bucket's all-reduce between the backward and Adam -- inside the
                   graph with RCCL; with gloo launched between G_comp[p] and G_adam[p])

    are captured, and replay k runs (p = k % S; set r = (k + S - 1) % S receives view k + S - 1,
    S - 1 views ahead; its last reader was step k - 1):

        stream A:  wait geo[p] -> G_comp[p] -> record step[p]
        stream B:  G_geo[r] -> record geo[r]

    so a replay is one full language step (the loss it returns is that of the view it composited and
    updated from) and later views' geometry overlaps it.  Two graphs on two streams are separate
    queues: unlike one graph with two branches (which this HIP runtime launches on one queue in
    capture order), they run concurrently.  The geometry reads nothing the step
    writes (the language step freezes the geometry, scene/gaussian_model.py:203-217); the step's
    feature fill reads what the previous step's Adam wrote (stream A order).

    A sequence of views (train.py:85-87): pass slots=[ViewSlot(...) for each set] and a
    forward_fn(slot) that renders from the slot; capture(views=[v0, ..., v_{S-2}]) takes the first
    S - 1 views and replay(next_view=v) the view S - 1 replays ahead (it is copied into that view's
    set on the caller's stream, after that set's last reader finished; each set keeps its own camera
    and target, so a replay never pairs one view's geometry with another's target).  Without slots
    forward_fn() renders one fixed view.

    The rasterizer runs in capacity mode (capacities from eager warm-up views, with headroom).  A
    view over capacity is flagged per set and the captured Adam skips on that flag (no parameter,
    moment or step count changes: the view is left out, include/lsr.h lsr_adam_multi); check()
    counts the skipped steps and re-captures.  N > 1: the flag is all-reduced in the same collective
    as the gradients (GradBucket.all_reduce(flag=)), so when one rank's view overflowed EVERY rank
    skips that step and re-captures: the ranks stay identical and no zero gradient is averaged in.
    The collective runs between the backward and Adam graphs (gloo; RCCL at N > 1 by default), or
    inside the step graph when captured (distributed.collective_capturable); the update then also
    fills the next set's records (lsr_adam_fill_language), as the fused tail does at N = 1.

        g = PipelinedGraphStep(lambda: render(...)["language_l1"], [gaussians._language_feature], optimizer)
        for it in range(iterations):
            loss = g.replay()   # this replay's view's loss (on the caller's stream after the replay)
        g.check(); g.sync()

    forward_fn() runs render() + the loss and returns the loss (no backward).  The graphs own the
    parameters' .grad tensors.  Work the caller enqueues on its stream between replays (a .clone()
    of the returned loss) precedes the device work of the replay S - 1 later, not of the next one;
    after changing the parameters or the optimizer state between replays, call follow_caller().

    Rotation mode (rotation=R > 1, N = 1; LSR_PG_ROT): 2 R buffer sets in two groups; every R-th
    replay launches the next R steps as ONE stream-A graph (fewer graph boundaries: ~20-28 us of idle
    queue each at C3) and the following R views' geometry on stream B; the replays in between launch
    nothing.  Parameters, learning rates and check() apply at rotation boundaries (k % R == 0).

    View cache (view_cache=True, N >= 1, rotation == 1): the language stage freezes every geometry
    parameter, and an epoch visits every view again, so a view's geometry half gives the same result at
    every visit.  When `model` is passed and none of its _xyz, _scaling, _rotation, _opacity,
    _features_dc, _features_rest requires grad, the first visit of a view runs G_geo as before; when its
    set is next about to receive a view, what the later phases read of that result is saved into a
    pack (lsr_view_save; ~74 MB at 1M Gaussians and 1080p), and every later visit enqueues ONE copy
    kernel (lsr_view_restore) on stream B in place of G_geo -- same waits before it, same event after
    it, the captured graphs untouched.  Views are keyed by their camera object (slots; the cache holds
    a reference), or by one constant key for the fixed view without slots, which therefore pays a
    restore per replay like any revisit.  view_cache_bytes bounds the packs (None: half of the device
    memory free at capture); there is no eviction.  Every pack is dropped at a (re-)capture, when any of
    the six tensors' (data_ptr(), _version) changes between replays, and by invalidate_views() -- call
    it after changing a camera object's tensors in place.  Rotation mode keeps its geometry graphs (no
    cache).  view_cache_stats() counts hits, misses, packs and bytes.

    Bound form (the default when the library has lsr_view_bind): the composite, the backward and the
    update's feature fill are captured against each set's table and plane (include/lsr.h "the bound
    form"), a miss's geometry graph writes the identity table itself, and a hit enqueues
    lsr_view_bind -- about 30 MB of traffic at C3 -- in place of the 157 MB restore: the set reads
    the pack's records and point list where they are.  Every form of the step is bound (the fused
    tail, the N > 1 deferred tail, the N > 1 update with lsr_adam_fill_language, the plain composite
    fill); view_cache="copy" forces the copying restore (A/B runs, tests).

    Knobs: the `sets` argument (default 3), LSR_PG_ROT (the `rotation` argument's default),
    LSR_PG_DEFER=0 (N > 1: the gradient epilogue stays in the backward) and LSR_PG_NATIVE_LAUNCH=0
    (every replay through torch's stream context).  Forms measured at C3 and not kept (DESIGN.md
    §5b): the geometry starting only after this view's compositing, stream priorities, the composite
    and the step as two graphs, a host throttle on the replays enqueued ahead."""

    def __init__(self, forward_fn, params, optimizer, headroom: float = 1.125, warmup: int = 2, bucket=None,
                 slots=None, sets: int = None, rotation: int = None, model=None, bucket_factory=None,
                 view_cache: bool = True, view_cache_bytes: int = None):
        self.forward_fn = forward_fn
        self.model = model  # its active_sh_degree is part of the capture key (graph.capture_key)
        self.params = [p for p in params]
        self.optimizer = optimizer
        self.bucket = bucket
        self.bucket_factory = bucket_factory  # rebuilds the bucket at a re-capture over replaced parameters
        self.headroom = float(headroom)
        self.warmup = int(warmup)
        dev = self.params[0].device
        # three sets by default: measured at C3 (one box) 0.435 ms per step against 0.482 with two; a view's geometry then runs two steps ahead, beside the backward and the
        # next compositing, and no compositing waits on a cross-stream event that is not yet signalled
        # rotation R > 1: R consecutive steps per stream-A graph over 2 R buffer sets (N = 1 only)
        R = int(rotation if rotation is not None else os.environ.get("LSR_PG_ROT", "1"))
        if R < 1 or (R > 1 and bucket is not None):
            raise ValueError("PipelinedGraphStep: rotation >= 1, and > 1 only without a bucket (N = 1)")
        self.R = R
        S = int(sets if sets is not None else (len(slots) if slots else (2 * R if R > 1 else 3)))
        if S < 2:
            raise ValueError("PipelinedGraphStep: at least two buffer sets")
        if R > 1 and S != 2 * R:
            raise ValueError("PipelinedGraphStep: a rotation of R steps takes 2 R buffer sets")
        if slots is not None and len(slots) != S:
            raise ValueError("PipelinedGraphStep: one ViewSlot per buffer set")
        self.S = S
        self.slots = list(slots) if slots is not None else None
        self.sets = tuple(_native.static_buffers() for _ in range(S))
        # A: step, B: geometry.  (Stream priorities measured worse: a high-priority geometry stream
        # 0.82 ms per step, a high-priority step stream 0.57, none 0.48.)
        # The later view's geometry starts with the step; starting it after this view's compositing
        # (beside the backward and Adam only) measured C3 with 2 sets 0.54 against 0.49 ms.
        self.streams = (torch.cuda.Stream(dev), torch.cuda.Stream(dev))
        self.overflow = tuple(torch.zeros((), dtype=torch.int32, device=dev) for _ in range(S))
        self._one = torch.ones((), device=dev)
        self._reset_graphs()
        self.captures = 0
        self.rendered = self.entries = 0
        self._skipped_base = 0
        self.fused = self.fill_after = self.defer = False  # the update's record fill (set by capture)
        self._tails = [None] * self.S
        self._loaded = [None] * S  # the view each set's slot holds (slots only)
        self._assigned = [None] * S  # rotation mode: the view each set's next geometry renders
        self.view_cache = bool(view_cache)
        self.view_copy = view_cache == "copy"  # the copying restore even where the sets could be bound
        self.bound = False  # the graphs were captured against the sets' tables and planes (set by capture)
        self.view_cache_bytes = view_cache_bytes
        self._views = None  # the ViewCache while it is active (set by capture)

    def _reset_graphs(self):
        S = self.S
        self.g_geo, self.g_comp, self.g_adam = [None] * S, [None] * S, [None] * S
        self.grads = [None] * S
        self.static_loss = [None] * S
        self.ev_geo = self.ev_step = [None] * S
        self.g_rot = self.g_rot0 = None
        self.k = 0
        self.primed = False

    def _fwd(self, p):
        return self.forward_fn(self.slots[p]) if self.slots is not None else self.forward_fn()

    def _measure(self, min_rendered, min_entries):
        _native.LAST_COUNTS.clear()
        side = torch.cuda.Stream(device=self.params[0].device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for i in range(self.warmup):
                for p in self.params:
                    p.grad = None
                # every set's view when they differ: the capacities cover the views loaded so far
                self._fwd(i % (self.S - 1)).backward()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        for p in self.params:
            p.grad = None
        if not _native.LAST_COUNTS:
            raise RuntimeError("PipelinedGraphStep: forward_fn ran no rasterizer forward")
        r = max(v[0] for v in _native.LAST_COUNTS.values())
        e = max(v[1] for v in _native.LAST_COUNTS.values())
        self.rendered = max(int(r * self.headroom) + 1024, int(min_rendered))
        self.entries = max(int(e * self.headroom) + 1024, int(min_entries))

    def capture(self, min_rendered: int = 0, min_entries: int = 0, views=None):
        """views: the first S - 1 views (camera, gt, mask) when the step renders from ViewSlots (a
        shorter list repeats its last view); the capacities are measured on them."""
        S = self.S
        # every pack goes before anything is measured or captured.  (Safe for bound sets: every step
        # enqueued so far precedes this drop -- the packs are recorded on both streams -- and no later
        # step reads them: after a capture every set gets its geometry again, primed = False.)
        self._views = None
        if self.slots is not None:
            if not views:
                raise ValueError("PipelinedGraphStep.capture: the first views are needed with slots")
            views = list(views)[:S - 1]
            views += [views[-1]] * (S - 1 - len(views))
            for j in range(S - 1):
                self.slots[j].load(*_as_view(views[j]))
                self._loaded[j] = self._assigned[j] = views[j]
        # the optimizer's current tensors (a parameter replaced since the last capture: the capture key
        # changed, replay() re-captures here) and a gradient bucket built over them
        self.params = current_params(self.optimizer, self.params)
        self.bucket = resolve_bucket(self.bucket, self.bucket_factory, self.params)
        # the caller's still-alive autograd graphs keep the parameters' AccumulateGrad nodes bound to
        # their streams: released, so the warm-up and the captures create their own (graph.py)
        self.key = capture_key(self.model, self.optimizer, self.params)
        self.stale_released = release_stale_accumulators(self.params)
        # the bound form wherever the view cache can become active (decided before any set is touched:
        # every capture below and every fill target follows it)
        self.bound = (self.view_cache and not self.view_copy and self.model is not None and self.R == 1
                      and self._geometry_tensors() is not None and _native.has_view_bind())
        for st in self.sets:
            st.view_bind = self.bound
        self._measure(min_rendered, min_entries)
        self._reset_graphs()
        self.optimizer.prepare_capture()
        self._skipped_base = self.optimizer.skipped_steps()
        cur = torch.cuda.current_stream()
        sa, sb = self.streams
        for s in self.streams:
            s.wait_stream(cur)
        caps = [_native.capacity(self.rendered, self.entries, self.overflow[p]) for p in range(S)]
        # eager forwards allocate every set at its capacity sizes (no allocation may happen during a
        # capture); nothing is updated
        for p in range(S):
            with torch.cuda.stream(sa), caps[p], self.sets[p]:
                self._fwd(p)
        sb.wait_stream(sa)
        # N > 1: the all-reduce of the gradients (and, in the same collective, of the set's overflow
        # flag: every rank then skips when one view overflowed) inside the step graph when the collective
        # is captured (distributed.collective_capturable: RCCL with one rank, or LSR_GRAPH_COLLECTIVE=1),
        # else launched between the backward and Adam graphs (gloo, and RCCL at N > 1 by default)
        dev = self.params[0].device
        coll_in_graph = self.bucket is not None and collective_capturable()
        self.coll_in_graph = coll_in_graph
        if coll_in_graph:  # the communicator exists before the capture (its creation is not capturable)
            with torch.cuda.stream(sa):
                self.bucket.all_reduce(average=True, flag=torch.zeros((), dtype=torch.int32, device=dev))
            for q in self.params:
                q.grad = None
        # N = 1 language step: Adam inside the backward's epilogue pass, which also writes the updated
        # feature into the NEXT set's records (the next composite needs no fill; the geometry call never
        # writes those slots, so it may run before, during or after)
        fused = self.bucket is None and len(self.params) == 1 and _fused_tail_enabled()
        self.fused = fused
        # N > 1 language step: the update after the all-reduce writes the feature into the next set's
        # records (lsr_adam_fill_language), so every composite but the first after a capture (refilled
        # from the parameter by replay(), _refill) needs no fill either
        fill_after = self.bucket is not None and len(self.params) == 1 and _fused_tail_enabled()
        self.fill_after = fill_after
        # ... and the gradient epilogue moves behind the collective: the backward leaves the language
        # partials (include/lsr.h LSR_BWD_DEFER_TAIL), the all-reduce averages them, and ONE pass
        # (lsr_language_tail) writes the gradients, steps and fills -- the N = 1 tail with the collective
        # before it (LSR_PG_DEFER=0: the epilogue in the backward, the collective over .grad, then
        # lsr_adam_fill_language)
        defer = fill_after and self.bucket.direct and os.environ.get("LSR_PG_DEFER", "1") != "0"
        self.defer = defer
        self._tails = [None] * S
        comp_phase = (_native.forward_phase.COMPOSITE_FILLED if fused or fill_after
                      else _native.forward_phase.COMPOSITE)
        # fused: the first composite after a capture fills set 0's feature records itself (G_comp0, run
        # by replay k = 0 instead of G_comp[0]; it owns its own gradients, grads0); later sets are
        # filled by the step before
        self.g_comp0 = None
        self.grads0 = None
        # the composite and the step are ONE graph per set: a graph boundary on stream A costs ~16-24 us
        # of idle queue at C3 (rocprofv3 trace, round 4), and nothing needs the point between them

        def update_ctx(p):
            if defer:  # this set's deferred tail (its arguments stay with the context)
                self._tails[p] = _native.fused_update(self.optimizer, self.params[0], skip=self.overflow[p],
                                                      fill=self._record_ptr((p + 1) % S), defer=True,
                                                      fill_plane=self.bound)
                return self._tails[p]
            return _native.fused_update(self.optimizer, self.params[0], skip=self.overflow[p],
                                        fill=self._record_ptr((p + 1) % S),
                                        fill_plane=self.bound) if fused else _nullctx()

        def adam_fill(p):  # (N > 1) the set's update fills the next set's records (bound: its plane)
            return (self._record_ptr((p + 1) % S), _native.RAW_LANGUAGE, self.bound) if fill_after else None

        def step_body(p, loss):
            with update_ctx(p):  # the backward runs on its forward's stream (sa)
                loss.backward(self._one)  # dL/dloss = 1 from a static tensor: no seed-fill kernel
                if coll_in_graph:
                    self._collective(p)
                if defer:
                    if coll_in_graph:
                        self._tails[p].run_tail()
                elif self.bucket is None or coll_in_graph:
                    self.optimizer.step(skip=self.overflow[p], fill=adam_fill(p))

        for p in range(S):
            if self.R > 1:
                continue  # geometry and steps are captured per rotation group below
            g = torch.cuda.CUDAGraph()
            with graph_capture(g, stream=sb), caps[p], self.sets[p], \
                    _native.forward_phase(_native.forward_phase.GEOMETRY):
                self._fwd(p)  # its outputs are written by the composite half
            self.g_geo[p] = g
            for q in self.params:
                q.grad = None  # the captured backward assigns its own .grad (no accumulate)
            if fused and p == 0:
                g = torch.cuda.CUDAGraph()
                with graph_capture(g, stream=sa):
                    with caps[p], self.sets[p], _native.forward_phase(_native.forward_phase.COMPOSITE):
                        loss = self._fwd(p)
                    step_body(p, loss)
                self.grads0 = [q.grad for q in self.params]
                del loss
                for q in self.params:
                    q.grad = None
                self.g_comp0 = g
            g = torch.cuda.CUDAGraph()
            with graph_capture(g, stream=sa):
                with caps[p], self.sets[p], _native.forward_phase(comp_phase):
                    loss = self._fwd(p)
                step_body(p, loss)
            self.g_comp[p] = g
            self.grads[p] = [q.grad for q in self.params]  # this set's graph-owned gradients
            if self.bucket is not None and not coll_in_graph:  # the all-reduce sits between two graphs
                g = torch.cuda.CUDAGraph()
                with graph_capture(g, stream=sa):
                    if defer:
                        self._tails[p].run_tail()
                    else:
                        self.optimizer.step(skip=self.overflow[p], fill=adam_fill(p))
                self.g_adam[p] = g
            self.static_loss[p] = loss.detach()  # the set's static loss tensor
            del loss
        if self.R > 1:
            self._capture_rotations(caps, comp_phase, fused, step_body)
        cur.wait_stream(sa)
        cur.wait_stream(sb)
        self.ev_rot = [torch.cuda.Event() for _ in range(2)]
        self.ev_geo = [torch.cuda.Event() for _ in range(S)]
        self.ev_step = [torch.cuda.Event() for _ in range(S)]
        self.ev_cur = [torch.cuda.Event() for _ in range(S)]
        self._since_capture = 0
        self._fast = False
        self._launchers = {}  # (set, fast) -> _native.GraphLauncher (replay's steady state)
        self._refill = fill_after  # the first composite's records: from the parameter (replay)
        self.captures += 1
        self._views = self._make_view_cache()  # (a re-capture starts empty: the layouts changed)
        return self

    _GEOMETRY_TENSORS = ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest")

    def _geometry_tensors(self):
        """The model's six geometry tensors when every one of them is frozen, else None."""
        ts = [getattr(self.model, n, None) for n in self._GEOMETRY_TENSORS]
        if any(not torch.is_tensor(t) or t.requires_grad for t in ts):
            return None
        return ts

    def _make_view_cache(self):
        if not self.view_cache or self.model is None or self.R != 1 or self._geometry_tensors() is None:
            return None
        call = getattr(self.sets[0], "geometry_call", None)
        if call is None or call["P"] < 1:
            return None
        budget = self.view_cache_bytes
        if budget is None:
            budget = torch.cuda.mem_get_info(self.params[0].device)[0] // 2
        if budget <= 0:
            return None
        # per set: its image buffer (the counter slots) and the pinned words a kernel copies them to
        self._cnt_size = (call["W"], call["H"])
        self._cnt_dev = [st.tensors[("scratch", _native.LSR_BUF_IMAGE)] for st in self.sets]
        self._cnt_host = [torch.zeros((8,), dtype=torch.int32).pin_memory() for _ in self.sets]
        return ViewCache(self.S, budget, _ViewNative(self.sets, self.streams[1], self.params[0].device,
                                                     bound=self.bound, readers=(self.streams[0],) if self.bound else (),
                                                     ev_step=self.ev_step))

    def _view_key(self, r):
        """(key, reference) of the view set r's geometry renders: its camera object, or the fixed view."""
        if self.slots is None:
            return 0, None
        if self._loaded[r] is None:  # no view loaded yet: whatever the set's slot was built with
            return ("slot", r), None
        cam = _as_view(self._loaded[r])[0]
        return id(cam), cam

    def invalidate_views(self):
        """Drop every cached view (e.g. after changing a camera's tensors in place)."""
        if self._views is not None:
            self._views.invalidate()

    def view_cache_stats(self):
        """{"hits", "misses", "packs", "bytes", "drops"} of the view cache since the last capture: restores,
        geometry graphs run, packs held and their bytes, invalidations (zeros while it is inactive)."""
        if self._views is None:
            return {"hits": 0, "misses": 0, "packs": 0, "bytes": 0, "drops": 0}
        return self._views.stats()

    def _capture_rotations(self, caps, comp_phase, fused, step_body):
        """Rotation mode: per group j of R sets (j = 0: sets 0..R-1, j = 1: sets R..2R-1) one graph
        of R full steps, composite + loss + backward + Adam each (and, fused, a variant of group 0
        whose first composite fills its own records, for the first replay after a capture)."""
        R, sa = self.R, self.streams[0]

        def rot(j, first):
            g = torch.cuda.CUDAGraph()
            grads = []
            with graph_capture(g, stream=sa):
                for p in range(j * R, (j + 1) * R):
                    for q in self.params:
                        q.grad = None  # each step's backward assigns its own .grad
                    phase = _native.forward_phase.COMPOSITE if (first and p == 0) else comp_phase
                    with caps[p], self.sets[p], _native.forward_phase(phase):
                        loss = self._fwd(p)
                    step_body(p, loss)
                    grads.append([q.grad for q in self.params])
                    self.static_loss[p] = loss.detach()  # the set's static loss (same tensor in every graph)
                    del loss
            return g, grads

        self.g_rot = [rot(0, False), rot(1, False)]
        self.g_rot0 = rot(0, True) if fused else None
        # each group's R geometries as one stream-B graph as well
        sb = self.streams[1]
        self.g_geo_rot = []
        for j in range(2):
            g = torch.cuda.CUDAGraph()
            with graph_capture(g, stream=sb):
                for p in range(j * R, (j + 1) * R):
                    with caps[p], self.sets[p], _native.forward_phase(_native.forward_phase.GEOMETRY):
                        self._fwd(p)
            self.g_geo_rot.append(g)
        for j in range(2):
            for i, gr in enumerate(self.g_rot[j][1]):
                self.grads[j * R + i] = gr

    def _replay_rotation(self, next_view, wait):
        """replay() in rotation mode: at a rotation start (k % R == 0) the group's R steps are launched
        as one graph on stream A, and the next rotation's geometry (the other group, whose sets the
        previous rotation released) on stream B; the other replays launch nothing."""
        S, R = self.S, self.R
        sa, sb = self.streams
        cur = torch.cuda.current_stream()
        k = self.k
        if next_view is not None:
            if self.slots is None:
                raise RuntimeError("PipelinedGraphStep.replay(next_view=...) needs ViewSlots")
            self._assigned[(k + S - 1) % S] = next_view
        if k % R == 0:
            j = (k // R) % 2
            if not self.primed:  # group 0's geometry (its views were loaded at capture)
                sb.wait_stream(cur)
                with torch.cuda.stream(sb):
                    self.g_geo_rot[0].replay()
                self.ev_geo[0].record(sb)
                self.primed = True
            if wait or self._since_capture == 0:
                sa.wait_stream(cur)  # the caller's earlier work (parameters, learning rates) first
            sa.wait_event(self.ev_geo[j * R])  # the group's geometry graph
            with torch.cuda.stream(sa):
                self.optimizer.sync_lr()
                if self._refill and self.fused and not (k == 0 and self.g_rot0 is not None):
                    self._refill_records(j * R)  # the caller changed the parameter (follow_caller)
                self._refill = False
                g, _ = self.g_rot0 if (k == 0 and self.g_rot0 is not None) else self.g_rot[j]
                g.replay()
            self.ev_rot[j].record(sa)
            # the other group's sets were last read by the previous rotation (none before the first)
            o = 1 - j
            if k >= R:
                sb.wait_event(self.ev_rot[o])
            if self.slots is not None:
                sb.wait_stream(cur)  # the views' tensors
            for p in range(o * R, (o + 1) * R):
                if self.slots is not None and self._assigned[p] is not None:
                    view = _as_view(self._assigned[p])
                    with torch.cuda.stream(sb):
                        self.slots[p].load(*view)
                    for t in self.slots[p].sources(*view):
                        t.record_stream(sb)
                    self._loaded[p] = self._assigned[p]
            with torch.cuda.stream(sb):
                self.g_geo_rot[o].replay()
            self.ev_geo[o * R].record(sb)
            if wait:
                cur.wait_event(self.ev_rot[j])
        elif wait:
            cur.wait_event(self.ev_rot[(k // R) % 2])
        self._since_capture += 1
        self.k += 1
        return self.static_loss[k % S]

    def _collective(self, p):
        """Set p's step collective (N > 1): the deferred backward's language partials, or the .grad
        tensors, with the set's overflow flag."""
        if self.defer:  # the partials carry the set's overflow flag themselves (include/lsr.h)
            self.bucket.all_reduce_partials(self._tails[p].partials(), average=True)
        else:
            self.bucket.all_reduce(average=True, flag=self.overflow[p])

    def _record_ptr(self, p):
        """Device address of where set p's language slots live: its per-Gaussian render records (include/lsr.h
        lsr_state_layout.record), or -- bound -- its plane (lsr_view_bind_layout)."""
        geom = self.sets[p].tensors[("scratch", _native.LSR_BUF_GEOM)]
        _, H, W = self.sets[p].tensors[("out", "color")].shape
        P = int(self.params[0].shape[0])
        if self.bound:
            return geom.data_ptr() + _native.view_bind_layout(P, int(W), int(H))["plane"]
        return geom.data_ptr() + _native.state_layout(P, int(W), int(H), 0)["record"]

    def _geometry(self, r, released=None):
        """Set r's geometry graph on stream B, after everything the caller's stream holds (the set's
        view loaded, its last reader finished) or, with `released` (an event: the set's last reader
        done), after that alone."""
        sb = self.streams[1]
        if released is not None:
            sb.wait_event(released)
        else:
            sb.wait_stream(torch.cuda.current_stream())
        vc = self._views
        if vc is None:
            with torch.cuda.stream(sb):
                self.g_geo[r].replay()
        else:
            key, ref = self._view_key(r)
            if not vc.visit(r, key):  # (a hit enqueued the view's restore instead)
                with torch.cuda.stream(sb):
                    self.g_geo[r].replay()
                # the view's counts and overflow word to the host, for a save when the set is next
                # released: a one-wave kernel before the set's own event.  (Stream B is a first epoch's
                # critical path: a device-to-host copy with an event of its own there measured +0.05 ms
                # per step, the same copy on a third stream +0.07, profiles/view_cache_ab.txt.)
                if not vc.off:
                    _native.view_counts(*self._cnt_size, self._cnt_dev[r], self._cnt_host[r], sb)
                    vc.computed(r, key, ref, self.ev_geo[r], self._cnt_host[r])
        self.ev_geo[r].record(sb)

    def _launcher(self, p, fast):
        """Set p's steady-state stream-A launch (replay): after the caller's mark of replay k - S + 1
        (ev_cur[p + 1], not in the fast form) and set p's geometry, the step graph, then ev_step[p].
        None until every one of those events exists (torch creates an event at its first record)."""
        if not _NATIVE_LAUNCH:
            return None
        key = (p, fast)
        fn = self._launchers.get(key)
        if fn is None:
            S = self.S
            waits = ([] if fast else [self.ev_cur[(p + 1) % S]]) + [self.ev_geo[p]]
            if any(e.cuda_event == 0 for e in waits + [self.ev_step[p]]):
                return None
            fn = _native.GraphLauncher(self.g_comp[p], self.streams[0], waits, self.ev_step[p])
            self._launchers[key] = fn
        return fn

    def replay(self, next_view=None, wait: bool = True) -> torch.Tensor:
        """One language step of the view loaded S - 1 replays ago (or at capture); next_view
        (camera, gt, mask) is the view of the replay S - 1 ahead (ViewSlots only; None: the view of
        its set stays).

        wait=False: the caller's stream is not chained to the replay -- the returned loss (and the
        graph-owned gradients) are valid on it only after synchronize() (and only those of the
        last S replays: a set's next composite rewrites them), and nothing of the replay
        goes through the caller's stream (its queue carries no event or wait per step: on this
        runtime the two streams' packets can share a hardware queue with it, and a wait there held
        stream A ~20-28 us per step).  The caller must not change the parameters
        between such replays without follow_caller().  bench.py times this form, with the
        synchronize() inside the timed region."""
        if self.g_comp[0] is None and getattr(self, "g_rot", None) is None:
            self.capture()
        elif (self.R == 1 or self.k % self.R == 0) and capture_key(self.model, self.optimizer, self.params) != self.key:
            # an SH-degree step or replaced parameters since the capture
            self._recapture(self.rendered, self.entries)
        if self.R > 1:
            return self._replay_rotation(next_view, wait)
        if self._views is not None:
            ts = self._geometry_tensors()
            if ts is None:
                # a geometry tensor became trainable: no cache until the next capture.  The cache is
                # switched off, not discarded: it holds the packs that sets bound ahead still read
                if not self._views.off:
                    self._views.disable()
            else:
                self._views.check(tuple((t.data_ptr(), t._version) for t in ts))
        S = self.S
        sa, sb = self.streams
        p = self.k % S
        r = (self.k + S - 1) % S
        fast = not wait and self._since_capture >= S - 1
        if wait and self._fast:  # back from fast replays: the lagged events were not recorded
            self._since_capture = 0
        # the caller's stream object (~2.4 us of host time) only where it is used before the launch
        cur = torch.cuda.current_stream() if (next_view is not None or not self.primed
                                               or self._since_capture < S - 1) else None
        if not self.primed:  # the first S - 1 views' geometry (nothing ran since the capture)
            for j in range(S - 1):
                self._geometry((self.k + j) % S)
            self.primed = True
        self._fast = fast
        # set r's last reader was step k - 1 (the view S - 1 ahead goes there)
        released = self.ev_step[(self.k - 1) % S] if self.k > 0 else None
        if next_view is not None:
            if self.slots is None:
                raise RuntimeError("PipelinedGraphStep.replay(next_view=...) needs ViewSlots")
            if fast:
                # on stream B, after step k - 1 and after the caller's stream (the view's tensors)
                sb.wait_stream(cur)
                if released is not None:
                    sb.wait_event(released)
                view = _as_view(next_view)
                with torch.cuda.stream(sb):
                    self.slots[r].load(*view)
                for t in self.slots[r].sources(*view):
                    t.record_stream(sb)
            else:
                # the caller's stream waited for step k - 1 at the end of the previous replay
                self.slots[r].load(*_as_view(next_view))
            self._loaded[r] = next_view
        first = self.k == 0 and self.g_comp0 is not None
        refill = self._refill and (self.fused or self.fill_after) and not first
        # Steady state (no update graph, no refill): the stream-A waits, the
        # launch and the step's event in ONE native call (lsr_graph_launch); the Python path below
        # costs ~8 us more host time before the launch, which a loss.item() loop pays every step
        launcher = (self._launcher(p, fast) if self.g_adam[p] is None and not first and not refill
                    and self._since_capture >= S - 1 else None)
        if launcher is not None:
            self._since_capture += 1
            self.optimizer.sync_lr(stream=sa)
            self._refill = False
            launcher()
        else:
            if not fast:
                # Stream A does not wait for the caller's stream as it is now: that stream waits for the
                # previous step (below), so the wait would be a round trip between two queues (measured
                # ~35 us of idle stream A per step at C3).  It waits instead for the
                # caller's work up to the start of replay k - S + 1, long done: the caller's uses of the
                # loss of replay k - S (whose tensor composite k rewrites) precede that.  The first
                # S - 1 replays after a capture wait for the caller's stream itself.  (This replay's own
                # mark on the caller's stream, ev_cur[k], is recorded after the step's launch below: the
                # caller's stream gets nothing from replay() before it, and a synced loop's stream A
                # idles until the launch.)
                if self._since_capture < S - 1:
                    sa.wait_stream(cur)
                else:
                    sa.wait_event(self.ev_cur[(self.k + 1) % S])  # recorded at replay k - S + 1
            self._since_capture += 1
            sa.wait_event(self.ev_geo[p])
            with torch.cuda.stream(sa):
                self.optimizer.sync_lr()  # a changed learning rate: a host-to-device copy on stream A
                if refill:
                    # the caller changed the parameter (follow_caller), or the first composite after an
                    # N > 1 capture (its records were filled by no earlier update)
                    self._refill_records(p)
                self._refill = False
                (self.g_comp0 if first else self.g_comp[p]).replay()
                if self.g_adam[p] is not None:
                    for q, g in zip(self.params, self.grads[p]):
                        q.grad = g
                    self._collective(p)
                    self.g_adam[p].replay()
            self.ev_step[p].record(sa)
        if cur is None:
            cur = torch.cuda.current_stream()
        if not fast:
            self.ev_cur[self.k % S].record(cur)
        # view k + S - 1's geometry into set r
        if fast:
            # the set's view (if any) was loaded on stream B itself
            self._geometry(r, released=self.ev_step[(self.k - 1) % S])
        else:
            self._geometry(r)
            cur.wait_event(self.ev_step[p])
        self.k += 1
        return self.static_loss[p]

    def last_grads(self):
        """The gradient tensors the last replay wrote (graph-owned; the first replay after a fused
        capture has its own)."""
        if self.k == 0:
            raise RuntimeError("PipelinedGraphStep.last_grads: no replay yet")
        if self.R > 1 and self.k <= self.R and self.g_rot0 is not None:
            return self.g_rot0[1][self.k - 1]
        if self.k == 1 and self.g_comp0 is not None:
            return self.grads0
        return self.grads[(self.k - 1) % self.S]

    def follow_caller(self):
        """The next replays wait for everything the caller's stream holds now (e.g. parameters the
        caller changed between replays).  With the fused tail the previous step already wrote the
        updated feature into the next set's records (COMPOSITE_FILLED never re-reads the parameter):
        the next replay refills them from the parameter first."""
        self._since_capture = 0
        self._refill = True

    def _refill_records(self, p):
        """Set p's records' language slots from the parameter as it is now (on the current stream),
        for a composite that would otherwise blend what the previous step's fused tail wrote."""
        radii = self.sets[p].tensors[("out", "radii")]
        _native.fill_language(self.params[0], _native.RAW_LANGUAGE, radii, self._record_ptr(p), plane=self.bound)

    def synchronize(self):
        """The caller's current stream waits for every replay enqueued so far (both streams)."""
        cur = torch.cuda.current_stream()
        for s in self.streams:
            cur.wait_stream(s)

    def sync(self):
        """The optimizer state's step counts from the device (a device-to-host copy)."""
        self.optimizer.sync_steps()

    def check(self) -> bool:
        """True if every replay's view fitted its capacities.  Otherwise re-capture with twice the
        capacities and return False: the over-capacity views were not rasterized, and at N = 1 their
        steps changed nothing (optimizer.skipped_steps() counts them; train those views again).
        Rotation mode: only between rotations (k % R == 0), where no launched step is pending."""
        if self.R > 1 and self.k % self.R != 0:
            raise RuntimeError("PipelinedGraphStep.check: in rotation mode only at a rotation boundary")
        self.synchronize()
        skipped = self.optimizer.skipped_steps() - self._skipped_base
        if skipped == 0 and all(int(o.item()) == 0 for o in self.overflow):
            return True
        for o in self.overflow:
            o.zero_()
        self._recapture(2 * self.rendered, 2 * self.entries)
        return False

    def _recapture(self, min_rendered, min_entries):
        """Capture again, continuing with the views already loaded for the next S - 1 steps."""
        self.synchronize()
        self.sync()
        src = self._assigned if self.R > 1 else self._loaded
        views = [src[(self.k + j) % self.S] for j in range(self.S - 1)] if self.slots else None
        self.capture(min_rendered, min_entries, views=views)
