"""The joint language-levels train step (levels.LevelsStep) captured into HIP graphs.

LevelsStep is eager: the rasterizer waits once per step for the view's tile-instance count, and the
step pays a gradient epilogue, a separate Adam pass and two feature fills around its kernels.
GraphedLevelsStep runs the same step without a host wait (include/lsr.h lsr_levels_step_forward /
lsr_levels_step_backward) as two linear graphs over one static buffer set, replayed on one stream:

    G_geo   lsr_forward(LSR_PHASE_GEOMETRY): preprocess, depth order, binning -- the same for every level;
    G_step  the levels composite (LSR_PHASE_COMPOSITE_FILLED), the L stand-alone masked-L1 losses into
            a static (L,) tensor, the accumulator clear, the gradient walk with the fused loss seed
            (dL_dloss = 1 per level) and the fused tail: gradient, Adam on the (L, P, 3) features and
            the next composite's feature slots, skipped when the view overflowed its capacities.

With view_cache=True a view's geometry is computed once (the geometry is frozen in the language
stage, scene/gaussian_model.py:203-217, and every epoch draws every view again, train.py:85-87): on
its first visit G_geo runs, the host waits once for that view's counts and the set's geometry is
saved into a pack (lsr_view_save); from the second visit on lsr_view_restore replaces G_geo.  The
packs are dropped at every (re-)capture, by invalidate_views(), and when one of the model's six
geometry tensors changed its address or version; the cache is active only while all six are frozen.

The captured tail writes no gradient tensor: between replays the graph owns the features, their
moments and the device step count (sync() copies the count back).  Code that changes the features
outside the graph calls refill() before the next replay.  There is no CPU path.
"""
from __future__ import annotations

import torch

from . import _native
from .graph import ViewSlot, _as_view, capture_key, graph_capture, release_stale_accumulators
from .levels import LevelsStep, render_levels_train
from .pipeline import ViewCache, _ViewNative
from .render import _fusable, camera_settings

_GEOMETRY_TENSORS = ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest")


class LevelsViewSlot(ViewSlot):
    """graph.ViewSlot's camera tensors plus the static per-level targets of a joint step: gts
    (L, 3, H, W) fp32 and masks (L, H, W) bool.  load(camera, gts, masks) copies a view into them on
    the current stream.  CPU tensors raise RuntimeError, wrong shapes ValueError."""

    def __init__(self, camera, gts: torch.Tensor, masks: torch.Tensor, device=None):
        self.gts = self.masks = None
        dev = torch.device(device) if device is not None else camera.world_view_transform.device
        H, W = int(camera.image_height), int(camera.image_width)
        if not torch.is_tensor(gts) or gts.dim() != 4 or not 1 <= int(gts.shape[0]) <= _native.MAX_LEVELS \
                or tuple(gts.shape[1:]) != (3, H, W):
            got = tuple(gts.shape) if torch.is_tensor(gts) else type(gts)
            raise ValueError(f"LevelsViewSlot: gts must be (L, 3, {H}, {W}) with 1 <= L <= {_native.MAX_LEVELS}, got {got}")
        self.levels = int(gts.shape[0])
        if not torch.is_tensor(masks) or masks.numel() != self.levels * H * W:
            raise ValueError(f"LevelsViewSlot: masks must be ({self.levels}, {H}, {W})")
        if dev.type != "cuda" or gts.device.type != "cuda" or masks.device.type != "cuda":
            raise RuntimeError("LevelsViewSlot: the camera and the targets must be on a ROCm GPU device; there is no "
                               "CPU implementation")
        super().__init__(camera, device=dev)  # (its load() call sees no targets yet)
        self.gts = torch.empty((self.levels, 3, H, W), dtype=torch.float32, device=dev)
        self.masks = torch.empty((self.levels, H, W), dtype=torch.bool, device=dev)
        self.load(camera, gts, masks)

    def load(self, camera, gts=None, masks=None):
        super().load(camera)
        if self.gts is None:  # construction: the camera tensors only
            return self
        if gts is None or masks is None:
            raise ValueError("LevelsViewSlot: every view carries its (gts, masks)")
        if gts.device.type != "cuda" or masks.device.type != "cuda":
            raise RuntimeError("LevelsViewSlot: the targets must be on a ROCm GPU device")
        if tuple(gts.shape) != tuple(self.gts.shape):
            raise ValueError(f"LevelsViewSlot: gts must be {tuple(self.gts.shape)}, got {tuple(gts.shape)}")
        if masks.numel() != self.masks.numel():
            raise ValueError(f"LevelsViewSlot: masks must be {tuple(self.masks.shape)}, got {tuple(masks.shape)}")
        self.gts.copy_(gts)
        m = masks if masks.dtype == torch.bool else masks != 0
        self.masks.copy_(m.reshape(self.masks.shape))
        return self


class GraphedLevelsStep:
    """LevelsStep.step as HIP graphs (module doc).  pc: the frozen geometry (GaussianModel-like, on the
    fused-activation path: raw fp32 contiguous tensors with the default activations); language_features:
    the (L, P, 3) torch.nn.Parameter, `optimizer`'s (a langsplat_amd.optim.Adam) one parameter; view: the
    LevelsViewSlot the step renders from; pipe, bg, opt: render()'s (opt.include_feature set).
    headroom, warmup: the capacities are the warm-up steps' counts times headroom (+ 1024).
    view_cache / cache_bytes: keep each view's geometry (default budget: half of the free device
    memory at the capture)."""

    def __init__(self, pc, language_features, optimizer, view: LevelsViewSlot, pipe, bg, opt, headroom: float = 1.125,
                 warmup: int = 2, view_cache: bool = False, cache_bytes=None):
        LevelsStep(pc, language_features, optimizer)  # its checks: Parameter, shape, Adam, the one parameter
        if not isinstance(view, LevelsViewSlot):
            raise ValueError("GraphedLevelsStep: view must be a LevelsViewSlot")
        dev = language_features.device
        if dev.type != "cuda" or pc.get_xyz.device.type != "cuda" or bg.device.type != "cuda":
            raise RuntimeError("GraphedLevelsStep: inputs must be on a ROCm GPU device "
                               f"(got {pc.get_xyz.device}, {dev}, {bg.device}); there is no CPU implementation")
        if view.levels != int(language_features.shape[0]):
            raise ValueError(f"GraphedLevelsStep: the view slot holds {view.levels} levels, the features "
                             f"{int(language_features.shape[0])}")
        if not opt.include_feature:
            raise ValueError("GraphedLevelsStep: needs opt.include_feature")
        if not _fusable(pc, pipe, None, dev):
            raise ValueError("GraphedLevelsStep: needs the fused-activation path (raw model tensors with the default "
                             "activations): the tail steps Adam on the raw features")
        if language_features.dtype != torch.float32 or not language_features.is_contiguous():
            raise ValueError("GraphedLevelsStep: language_features must be contiguous fp32")
        self.pc, self.optimizer, self.view = pc, optimizer, view
        self.language_features = language_features
        self.pipe, self.bg, self.opt = pipe, bg, opt
        self.headroom, self.warmup = float(headroom), int(warmup)
        self.view_cache, self.cache_bytes = bool(view_cache), cache_bytes
        self.G_geo = self.G_step = None
        self.losses = None
        self.captures = self.geo_replays = 0
        self.rendered = self.entries = 0
        self.overflow = torch.zeros((), dtype=torch.int32, device=dev)
        self._skipped_base = 0
        self._views = None
        self._loaded = None
        self._refill = True

    # ------------------------------------------------------------------ the step's pieces
    def _inputs(self):
        """The fused path's raw inputs (render_levels_train's), which the graphs name by address."""
        pc = self.pc
        ts = [pc.get_xyz, pc._features_dc, pc._opacity, pc._scaling, pc._rotation]
        rest = pc._features_rest if pc._features_rest.numel() > 0 else None
        for t in ts + ([rest] if rest is not None else []):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("GraphedLevelsStep: the model's tensors must be contiguous fp32 (the graphs hold "
                                 "their addresses)")
        xyz, dc, opac, scal, rot = (t.detach() for t in ts)
        return xyz, dc, opac, scal, rot, (rest.detach() if rest is not None else None)

    _RAW = _native.RAW_OPACITY | _native.RAW_SCALES | _native.RAW_ROTATIONS | _native.RAW_LANGUAGE

    def _geometry(self):
        xyz, dc, opac, scal, rot, rest = self._in
        with _native.forward_phase(_native.forward_phase.GEOMETRY):
            visible = _native.output_tensor("visible", (int(xyz.shape[0]),), torch.bool, xyz.device)
            _native.rasterize_gaussians(self._rs, xyz, dc, None, self.language_features.detach()[0], opac, scal, rot,
                                        None, raw=self._RAW, shs_rest=rest, flags=_native.FWD_NO_BACKWARD,
                                        visible=visible)

    def _composite(self, phase):
        xyz, dc, opac, scal, rot, rest = self._in
        with _native.forward_phase(phase):
            return _native.levels_step_forward(self._rs, xyz, dc, None, self.language_features.detach(), opac, scal,
                                               rot, None, raw=self._RAW, shs_rest=rest)

    def _losses(self, langs):
        """LevelsStep's L stand-alone masked-L1 launches, into the static loss tensor.  Each level has its
        own reduction scratch, cleared here: a captured launch's epoch word is the same at every replay, so
        only a cleared scratch tells this replay's block sums from the last one's."""
        import ctypes
        lib = _native.load()
        dev = langs.device
        L, _, H, W = langs.shape
        self._loss_scratch.zero_()
        masks = self.view.masks.view(torch.uint8)
        for l in range(L):
            _native._check(lib.lsr_masked_l1_forward(
                3, H * W, _native._ptr(langs[l]), _native._ptr(self.view.gts[l]), _native._ptr(masks[l]), 0,
                ctypes.c_void_p(self.losses[l].data_ptr()), ctypes.c_void_p(self._loss_scratch[l].data_ptr()),
                _native._stream(dev)), "lsr_masked_l1_forward")

    def _step_body(self):
        nr, _, langs, radii, _, geom, binning, image, levels = self._composite(_native.forward_phase.COMPOSITE_FILLED)
        self._losses(langs)
        _native.levels_step_backward(self._rs, self.language_features, radii, nr, geom, binning, image, raw=self._RAW,
                                     images=langs, targets=self.view.gts, masks=self.view.masks, grad_losses=self._ones,
                                     update=self._update, scratch=self._acc, want_grad=False)

    # ------------------------------------------------------------------ capture
    def _measure(self, min_rendered, min_entries):
        """Eager warm-up steps on a side stream that change no parameter (forward, losses, backward; no
        optimizer step); the largest counts they saw, with headroom, become the capacities."""
        lf = self.language_features
        _native.LAST_COUNTS.clear()
        side = torch.cuda.Stream(device=lf.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(self.warmup, 1)):
                lf.grad = None
                pkg = render_levels_train(self.view, self.pc, self.pipe, self.bg, self.opt, lf,
                                          language_targets=(self.view.gts, self.view.masks))
                pkg["language_l1"].sum().backward()
                del pkg
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        lf.grad = None
        r = max(v[0] for v in _native.LAST_COUNTS.values())
        e = max(v[1] for v in _native.LAST_COUNTS.values())
        self.rendered = max(int(r * self.headroom) + 1024, int(min_rendered))
        self.entries = max(int(e * self.headroom) + 1024, int(min_entries))

    def capture(self, min_rendered: int = 0, min_entries: int = 0):
        opt = self.optimizer
        params = [p for g in opt.param_groups for p in g["params"]]
        if len(params) != 1:
            raise ValueError("GraphedLevelsStep: language_features must be the optimizer's one parameter")
        lf = self.language_features = params[0]  # (a replaced parameter: the optimizer's current one)
        dev = lf.device
        L, P = int(lf.shape[0]), int(lf.shape[1])
        if P < 1:
            raise ValueError("GraphedLevelsStep: an empty model has no step to capture")
        self.key = capture_key(self.pc, opt, [lf])
        release_stale_accumulators([lf])
        self._measure(min_rendered, min_entries)
        release_stale_accumulators([lf])  # the warm-up's node (bound to its side stream) is not kept either
        opt.prepare_capture()
        self.G_geo = self.G_step = None  # an earlier capture's pools go before the new one allocates
        self._views = None
        self._in = self._inputs()
        self._rs = camera_settings(self.view, self.pc, self.pipe, self.bg, 1.0, True)
        H, W = self.view.image_height, self.view.image_width
        self.buffers = _native.static_buffers()
        self.losses = torch.zeros((L,), dtype=torch.float32, device=dev)
        self._ones = torch.ones((L,), dtype=torch.float32, device=dev)
        lib = _native.load()
        self._acc = torch.empty((int(lib.lsr_backward_levels_bytes(P, L)),), dtype=torch.uint8, device=dev)
        per = (int(lib.lsr_masked_l1_scratch_bytes(3, H * W)) + 255) // 256 * 256
        self._loss_scratch = torch.zeros((L, per), dtype=torch.uint8, device=dev)
        st = opt.state[lf]
        gi = next(i for i, g in enumerate(opt.param_groups) if any(q is lf for q in g["params"]))
        group = opt.param_groups[gi]
        with _native.capacity(self.rendered, self.entries, self.overflow), self.buffers:
            # one eager pass allocates every static tensor (none may be allocated inside a capture)
            self._geometry()
            _, _, _, _, _, geom, _, _, levels = self._composite(_native.forward_phase.COMPOSITE)
            record = geom.data_ptr() + _native.state_layout(P, W, H, self.rendered)["record"]
            self._update = _native.LevelsUpdate(
                lf.data, st["exp_avg"], st["exp_avg_sq"], group["betas"], group["eps"], opt._step_dev,
                step_offset=opt.step_offset(lf), skip=self.overflow, fill_record=record,
                fill_levels=levels if L > 1 else None)
            g_geo = torch.cuda.CUDAGraph()
            with graph_capture(g_geo):
                self._geometry()
            g_step = torch.cuda.CUDAGraph()
            with graph_capture(g_step):
                opt._register_fused(gi)  # the device block's lr word 0 is this group's (sync_lr keeps it current)
                self._step_body()
        self._skipped_base = opt.skipped_steps()
        self.G_geo, self.G_step = g_geo, g_step
        self._refill = True  # the first replay's slots: from the parameter, for its own view
        self.captures += 1
        self._views = self._make_view_cache()  # (a re-capture starts empty: the layouts changed)
        return self

    def _geometry_stamp(self):
        """The six geometry tensors' (data_ptr, _version) when every one of them is frozen, else None."""
        ts = [getattr(self.pc, n, None) for n in _GEOMETRY_TENSORS]
        if any(not torch.is_tensor(t) or t.requires_grad for t in ts):
            return None
        return tuple((t.data_ptr(), t._version) for t in ts)

    def _make_view_cache(self):
        if not self.view_cache or self._geometry_stamp() is None:
            return None
        dev = self.language_features.device
        budget = self.cache_bytes
        if budget is None:
            budget = torch.cuda.mem_get_info(dev)[0] // 2
        if budget <= 0:
            return None
        self._cnt_host = torch.zeros((8,), dtype=torch.int32).pin_memory()
        self._cnt_event = torch.cuda.Event()
        self._cache_full = False
        return ViewCache(1, budget, _ViewNative([self.buffers], torch.cuda.current_stream(dev), dev))

    # ------------------------------------------------------------------ replay
    def refill(self):
        """The features were changed outside the graph: the next replay writes its view's feature slots
        from them (one eager LSR_PHASE_COMPOSITE call) before the captured step composites."""
        self._refill = True

    def invalidate_views(self):
        """Drop every cached view (e.g. after changing a camera's tensors in place)."""
        if self._views is not None:
            self._views.invalidate()
            self._cache_full = False

    def view_cache_stats(self):
        """{"hits", "misses", "packs", "bytes", "drops"} of the view cache since the last capture."""
        if self._views is None:
            return {"hits": 0, "misses": 0, "packs": 0, "bytes": 0, "drops": 0}
        return self._views.stats()

    def _run_geometry(self):
        """The loaded view's geometry into the buffer set: G_geo, or the restore of its pack."""
        views = self._views
        stamp = self._geometry_stamp() if views is not None else None
        if views is None or stamp is None:
            self.G_geo.replay()
            self.geo_replays += 1
            return
        dev = self.language_features.device
        stream = torch.cuda.current_stream(dev)
        views.native.stream = stream
        drops = views.drops
        views.check(stamp)
        if views.drops != drops:
            self._cache_full = False
        cam = self._loaded
        key = id(cam) if cam is not None else ("slot",)
        if views.restore(0, key):
            return
        self.G_geo.replay()
        self.geo_replays += 1
        if self._cache_full:
            return
        # the view's counts: a one-off host wait per view, then its pack
        call = self.buffers.geometry_call
        image = self.buffers.tensors[("scratch", _native.LSR_BUF_IMAGE)]
        _native.view_counts(call["W"], call["H"], image, self._cnt_host, stream)
        self._cnt_event.record(stream)
        self._cnt_event.synchronize()
        views.computed(0, key, cam, self._cnt_event, self._cnt_host)
        if not views.save_pending(0) and int(self._cnt_host[ViewCache.OVERFLOW]) == 0:
            self._cache_full = True  # the budget: later views keep running G_geo without the wait

    def replay(self, view=None) -> torch.Tensor:
        """One captured step; view=(camera, gts, masks) first loads that view into the slot on the
        current stream.  Returns the static (L,) losses (before the update), valid until the next replay."""
        if view is not None:
            cam, gts, masks = _as_view(view)
            self.view.load(cam, gts, masks)
            self._loaded = cam
        if self.G_step is None:
            self.capture()
        elif capture_key(self.pc, self.optimizer, [self.language_features]) != self.key:
            self.sync()
            self.capture(self.rendered, self.entries)
        self.optimizer.sync_lr()
        self._run_geometry()
        if self._refill:
            with _native.capacity(self.rendered, self.entries, self.overflow), self.buffers:
                self._composite(_native.forward_phase.COMPOSITE)
            self._refill = False
        self.G_step.replay()
        return self.losses

    def sync(self):
        """The optimizer state's step counts from the device (a device-to-host copy)."""
        self.optimizer.sync_steps()

    def check(self) -> bool:
        """True if every replay since the capture fitted its capacities.  Otherwise re-capture with
        twice the capacities and return False; an over-capacity view was not rasterized and its replay
        changed no feature, moment or step count (run that view again)."""
        skipped = self.optimizer.skipped_steps() - self._skipped_base
        if skipped == 0 and int(self.overflow.item()) == 0:
            return True
        self.sync()
        self.capture(2 * self.rendered, 2 * self.entries)
        return False


__all__ = ["LevelsViewSlot", "GraphedLevelsStep"]
