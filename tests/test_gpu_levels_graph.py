"""The joint levels step without a host wait: lsr_levels_step_forward / lsr_levels_step_backward (include/lsr.h)
and langsplat_amd.levels_graph (LevelsViewSlot, GraphedLevelsStep).

Yardsticks.  The capacity-mode forward and the fused tail are exact: torch.equal against render_levels
and against the three-launch sequence (gradient epilogue, lsr_adam_multi, the feature fills).  Gradients:
tests.test_gpu_parity.assert_grad_close against the oracle references test_gpu_levels_train caches
(computed once per scene and level, shared with that file's tests).  Parameter trajectories:
tests.test_gpu_captured_forms.assert_states_close, the existing tolerance of captured against eager
steps (the gradient sums are float atomics: two eager runs differ by as much, which
test_forced_overflow_replay_is_left_out checks before it compares)."""
import ctypes
import functools
import struct

import pytest
import torch

import bench
from langsplat_amd import _native, levels
from langsplat_amd.levels_graph import GraphedLevelsStep, LevelsViewSlot
from langsplat_amd.optim import Adam
from langsplat_amd.render import camera_settings
from langsplat_amd.synthetic import make_cameras
from tests.scenes import POSES, posed_camera, to_device
from tests.test_gpu_captured_forms import assert_states_close
from tests.test_gpu_levels import level_features
from tests.test_gpu_levels_train import _model, _scene, _targets, reference, seeds_for
from tests.test_gpu_parity import assert_grad_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
P, W, H = 3000, 96, 64
RAW = _native.RAW_OPACITY | _native.RAW_SCALES | _native.RAW_ROTATIONS | _native.RAW_LANGUAGE
OVERFLOW_BITS = 0x3F800000
GEOMETRY, COMPOSITE, FILLED = (_native.forward_phase.GEOMETRY, _native.forward_phase.COMPOSITE,
                               _native.forward_phase.COMPOSITE_FILLED)


# ---- shared, read-only fixtures --------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def world():
    """The model (P = 3000), two ring cameras, two cameras inside the cube (the second rolled by 180
    degrees), one looking away from it, the background and every camera's (gts, masks) for L = 4 (tests
    slice the levels they use)."""
    model = _model(P)
    ring = make_cameras(2, W, H, device=DEV)
    inside = posed_camera(*POSES["inside"], W, H).to(DEV)
    flip = posed_camera(*POSES["inside_flip"], W, H).to(DEV)
    away = posed_camera((0.0, 0.0, -3.0), (0.0, 0.0, -10.0), 0.0, W, H).to(DEV)
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    cams = dict(a=ring[0], b=ring[1], inside=inside, away=away, flip=flip)
    targets = {k: _targets(c, model, bench.Pipe, bg, 4, P, H, W, seed=11 + i) for i, (k, c) in enumerate(cams.items())}
    return model, cams, bg, targets


def raw_features(L, n=P):
    """Raw (unnormalised) level features: level_features scaled per Gaussian by 0.5 .. 2."""
    return (level_features(L, n) * torch.linspace(0.5, 2.0, n, device=DEV)[None, :, None]).contiguous()


def model_args(model):
    """(positional inputs before and after the features, keyword inputs) of the fused raw path."""
    d = lambda t: t.detach()  # noqa: E731
    return (d(model.get_xyz), d(model._features_dc), None), (d(model._opacity), d(model._scaling), d(model._rotation),
                                                            None), dict(raw=RAW, shs_rest=d(model._features_rest))


def scene_args(ind):
    """The same for a tests.scenes scene (activated inputs, raw = 0)."""
    return (ind["means3D"], ind.get("shs"), ind.get("colors_precomp")), (
        ind["opacities"], ind.get("scales"), ind.get("rotations"), ind.get("cov3D_precomp")), dict(raw=0)


class Run:
    """One static buffer set in capacity mode: geometry(), forward(phase) and backward() over it."""

    def __init__(self, rs, args, rendered, entries):
        self.rs, (self.pre, self.post, self.kw) = rs, args
        self.buffers = _native.static_buffers()
        self.overflow = torch.zeros((), dtype=torch.int32, device=DEV)
        self.cap = _native.capacity(int(rendered), int(entries), self.overflow)

    def geometry(self, feats):
        with self.cap, self.buffers, _native.forward_phase(GEOMETRY):
            # (the preprocess runs here: it writes the set's visibility tensor, as its radii)
            visible = _native.output_tensor("visible", (feats.shape[1],), torch.bool, DEV)
            _native.rasterize_gaussians(self.rs, *self.pre, feats[0].contiguous(), *self.post,
                                        flags=_native.FWD_NO_BACKWARD, visible=visible, **self.kw)

    def forward(self, feats, phase=0):
        with self.cap, self.buffers, _native.forward_phase(phase):
            self.out = _native.levels_step_forward(self.rs, *self.pre, feats, *self.post, **self.kw)
        return self.out

    def backward(self, feats, **kw):
        nr, _, _, radii, _, geom, binning, image, _ = self.out
        return _native.levels_step_backward(self.rs, feats, radii, nr, geom, binning, image,
                                            raw=self.kw["raw"], **kw)

    def record_ptr(self):
        n = int(self.out[3].shape[0])
        lay = _native.state_layout(n, int(self.rs.image_width), int(self.rs.image_height), self.cap.rendered)
        return self.out[5].data_ptr() + lay["record"]

    def record_slots(self):
        """The (P, 3) language slots of the set's render records."""
        n = int(self.out[3].shape[0])
        lay = _native.state_layout(n, int(self.rs.image_width), int(self.rs.image_height), self.cap.rendered)
        rec = self.out[5][lay["record"]:lay["record"] + 48 * n].view(torch.float32).view(n, 12)
        return rec[:, 9:12]

    def level_rows(self, L):
        """The (P, 4 Q) floats of the set's LSR_BUF_LEVELS array."""
        n = int(self.out[3].shape[0])
        q = (3 * (L - 1) + 3) // 4
        return self.out[8][:16 * q * n].view(torch.float32).view(n, 4 * q)


def capacities(key):
    r, e = _native.LAST_COUNTS[key]
    return int(r * 1.125) + 1024, int(e * 1.125) + 1024


# ---- 1. forward parity -----------------------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_capacity_forward_is_bit_identical_to_render_levels(L):
    model, cams, bg, _ = world()
    feats = raw_features(L)
    ref = levels.render_levels(cams["a"], model, bench.Pipe, bg, bench.Opt, feats)
    rs = camera_settings(cams["a"], model, bench.Pipe, bg, 1.0, True)
    caps = capacities((P, W, H))
    for form in ("all", "split"):
        run = Run(rs, model_args(model), *caps)
        if form == "split":
            run.geometry(feats)
        nr, color, langs, radii, visible = run.forward(feats, COMPOSITE if form == "split" else 0)[:5]
        assert nr == caps[0] and int(run.overflow) == 0
        assert torch.equal(langs, ref["language_feature_images"]), form
        assert torch.equal(color, ref["render"]), form
        assert torch.equal(radii, ref["radii"]) and torch.equal(visible, ref["visibility_filter"]), form
    assert float(langs.abs().max()) > 0


def test_split_forward_walks_several_batches_on_the_long_list_scene():
    st, inp = _scene("long")
    std, ind = to_device(st, inp, DEV)
    feats = level_features(4, 12000)
    pre, post, kw = scene_args(ind)
    nr, color, langs, radii = _native.rasterize_gaussians_levels(std, *pre, feats, *post, **kw)
    assert nr > 8192  # tiles above 256 entries: more than one batch
    run = Run(std, (pre, post, kw), *capacities((12000, 32, 32)))
    run.geometry(feats)
    out = run.forward(feats, COMPOSITE)
    assert int(run.overflow) == 0
    assert torch.equal(out[2], langs) and torch.equal(out[1], color) and torch.equal(out[3], radii)


# ---- 2. gradient parity ----------------------------------------------------------------------------

@pytest.mark.parametrize("name, L", [("ring", 1), ("ring", 2), ("ring", 3), ("ring", 4), ("long", 4), ("inside", 3)])
def test_capacity_backward_matches_the_oracle(name, L):
    st, inp = _scene(name)
    std, ind = to_device(st, inp, DEV)
    n = inp["means3D"].shape[0]
    feats = level_features(L, n)
    args = scene_args(ind)
    _native.rasterize_gaussians_levels(std, *args[0], feats, *args[1], **args[2])  # the view's counts
    run = Run(std, args, *capacities((n, st.image_width, st.image_height)))
    radii = run.forward(feats)[3]
    grad = run.backward(feats, grad_images=seeds_for(L, st.image_height, st.image_width).to(DEV))
    assert int(run.overflow) == 0 and grad.shape == (L, n, 3)
    culled = (radii <= 0).cpu().numpy()
    if name == "inside":
        assert culled.any() and not culled.all()  # Gaussians culled beside visible ones
    for l in range(L):
        got = grad[l].cpu().numpy()
        assert_grad_close(f"{name} level {l}", got, reference(name, l))
        assert not got[culled].any(), f"{name} level {l}: a culled Gaussian has a gradient"


# ---- 3., 4. the tail -------------------------------------------------------------------------------

def lr_bits(lr):
    return struct.unpack("<q", struct.pack("<d", lr))[0]


def step_block(count, lr):
    sd = torch.zeros((_native.ADAM_STEP_WORDS,), dtype=torch.int64, device=DEV)
    sd[0] = count
    sd[_native.ADAM_WORD_LR] = lr_bits(lr)
    return sd


def adam_multi(param, grad, m, v, lr, betas, eps, step_dev):
    """lsr_adam_multi of one tensor in its device form (the launch that follows the gradient epilogue)."""
    t = _native.LsrAdamTensor(param.numel(), param.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), lr, betas[0],
                              betas[1], eps, 0)
    _native._check(_native.load().lsr_adam_multi(1, ctypes.byref(t), 1.0, ctypes.c_void_p(step_dev.data_ptr()), None,
                                                 _native._stream(param.device)), "lsr_adam_multi")


def activated_by_fill(feat):
    """k_fill_language's activated values of a raw (n, 3) feature for EVERY row (radii of ones)."""
    n = feat.shape[0]
    rec = torch.zeros((n, 12), dtype=torch.float32, device=DEV)
    _native.fill_language(feat.contiguous(), _native.RAW_LANGUAGE, torch.ones((n,), dtype=torch.int32, device=DEV),
                          rec.data_ptr())
    return rec[:, 9:12].clone()


def tail_case(n, L, moments=True, skip=None):
    """One lsr_levels_step_backward with update on the inside camera (culled beside visible Gaussians):
    everything the assertions need."""
    model = _model(n) if n != P else world()[0]
    _, cams, bg, _ = world()
    cam = cams["inside"]
    rs = camera_settings(cam, model, bench.Pipe, bg, 1.0, True)
    feats = raw_features(L, n)
    ref = levels.render_levels(cam, model, bench.Pipe, bg, bench.Opt, feats)
    gts = torch.roll(ref["language_feature_images"], 1, dims=3).contiguous()
    masks = (torch.rand((L, H, W), generator=torch.Generator().manual_seed(5)) > 0.3).to(DEV)
    g = torch.Generator().manual_seed(17)
    m = (torch.randn((L, n, 3), generator=g) * 1e-3).to(DEV) if moments else torch.zeros((L, n, 3), device=DEV)
    v = (torch.rand((L, n, 3), generator=g) * 1e-6).to(DEV) if moments else torch.zeros((L, n, 3), device=DEV)
    lr, betas, eps, count = 0.0025, (0.9, 0.999), 1e-15, 6
    sd = step_block(count, lr)
    run = Run(rs, model_args(model), *capacities((n, W, H)))
    out = run.forward(feats)
    assert torch.equal(out[2], ref["language_feature_images"]) and int(run.overflow) == 0
    before = (feats.clone(), m.clone(), v.clone())
    grad = torch.full((L, n, 3), float("nan"), device=DEV)
    upd = _native.LevelsUpdate(feats, m, v, betas, eps, sd, skip=skip, fill_record=run.record_ptr(),
                               fill_levels=out[8] if L > 1 else None)
    run.backward(feats, images=out[2], targets=gts, masks=masks, grad_losses=torch.ones((L,), device=DEV), update=upd,
                 out=grad)
    torch.cuda.synchronize()
    return dict(model=model, rs=rs, run=run, radii=out[3], feats=feats, m=m, v=v, before=before, grad=grad, sd=sd,
                lr=lr, betas=betas, eps=eps, count=count)


def check_fills(c, L):
    """Every Gaussian's feature slots hold the activated current features: against k_fill_language on all
    rows, and on the visible rows against a COMPOSITE call's k_fill_language / k_fill_levels into a second set."""
    run, feats = c["run"], c["feats"]
    assert torch.equal(run.record_slots(), activated_by_fill(feats[0]))
    if L > 1:
        rows = run.level_rows(L)
        for l in range(1, L):
            assert torch.equal(rows[:, 3 * (l - 1):3 * l], activated_by_fill(feats[l])), l
        assert not rows[:, 3 * (L - 1):].any()  # the zero padding
    second = Run(c["rs"], model_args(c["model"]), run.cap.rendered, run.cap.entries)
    second.geometry(feats)
    second.forward(feats, COMPOSITE)
    vis = c["radii"] > 0
    assert vis.any() and not vis.all()
    assert torch.equal(run.record_slots()[vis], second.record_slots()[vis])
    if L > 1:
        assert torch.equal(run.level_rows(L)[vis], second.level_rows(L)[vis])


@pytest.mark.parametrize("L", [1, 3, 4])
@pytest.mark.parametrize("n", [257, P])
def test_tail_is_the_epilogue_adam_and_the_fills_bit_for_bit(n, L):
    c = tail_case(n, L)
    p0, m0, v0 = c["before"]
    grad = c["grad"]
    assert not torch.isnan(grad).any() and float(grad.abs().max()) > 0
    # the gradient is the update == NULL tail's (k_levels_grad_epilogue) on the same forward, up to the atomics' order
    assert not grad[:, c["radii"] <= 0].any()
    # device step block: lsr_adam_multi on clones, from the gradient the call wrote
    p1, m1, v1, sd1 = p0.clone(), m0.clone(), v0.clone(), step_block(c["count"], c["lr"])
    adam_multi(p1, grad, m1, v1, c["lr"], c["betas"], c["eps"], sd1)
    assert torch.equal(c["feats"], p1) and torch.equal(c["m"], m1) and torch.equal(c["v"], v1)
    assert int(c["sd"][0]) == int(sd1[0]) == c["count"] + 1 and int(c["sd"][_native.ADAM_WORD_SKIPPED]) == 0
    assert not torch.equal(c["feats"], p0)
    # host scalars: optim.Adam's eager step on another clone
    twin = torch.nn.Parameter(p0.clone())
    opt = Adam([{"params": [twin], "lr": c["lr"]}], lr=0.0, betas=c["betas"], eps=c["eps"])
    opt.state[twin] = {"step": torch.tensor(float(c["count"])), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    twin.grad = grad.clone()
    opt.step()
    st = opt.state[twin]
    assert torch.equal(c["feats"], twin.detach()) and torch.equal(c["m"], st["exp_avg"])
    assert torch.equal(c["v"], st["exp_avg_sq"])
    check_fills(c, L)


def test_culled_rows_keep_their_parameter_with_zero_moments():
    c = tail_case(P, 3, moments=False)
    culled = c["radii"] <= 0
    assert culled.any()
    assert not c["grad"][:, culled].any()
    assert torch.equal(c["feats"][:, culled], c["before"][0][:, culled])  # zero moments, zero gradient: Adam moves nothing
    assert not c["m"][:, culled].any() and not c["v"][:, culled].any()
    assert not torch.equal(c["feats"][:, ~culled], c["before"][0][:, ~culled])


def test_skip_changes_nothing_but_the_skipped_count_and_still_fills():
    skip = torch.tensor(OVERFLOW_BITS, dtype=torch.int32, device=DEV)
    c = tail_case(P, 3, skip=skip)
    p0, m0, v0 = c["before"]
    assert torch.equal(c["feats"], p0) and torch.equal(c["m"], m0) and torch.equal(c["v"], v0)
    assert int(c["sd"][0]) == c["count"] and int(c["sd"][_native.ADAM_WORD_SKIPPED]) == 1
    assert float(c["grad"].abs().max()) > 0  # the gradient itself is still written
    check_fills(c, 3)


# ---- 5. forced overflow ----------------------------------------------------------------------------

def test_forced_overflow_leaves_background_zero_maps_and_a_zero_gradient():
    model, cams, bg, targets = world()
    L = 3
    feats = raw_features(L)
    rs = camera_settings(cams["a"], model, bench.Pipe, bg, 1.0, True)
    run = Run(rs, model_args(model), 16, capacities((P, W, H))[1])
    nr, color, langs, radii = run.forward(feats)[:4]
    assert nr == 16 and int(run.overflow) == OVERFLOW_BITS
    assert not langs.any()
    assert torch.equal(color, bg[:, None, None].expand(3, H, W))
    assert int((radii > 0).sum()) > 0  # the preprocess ran: the view is visible, only not binned
    gts, masks = (t[:L].contiguous() for t in targets["a"])
    ones = torch.ones((L,), device=DEV)
    grad = run.backward(feats, images=langs, targets=gts, masks=masks, grad_losses=ones,
                        grad_images=seeds_for(L, H, W).to(DEV))
    assert grad.shape == (L, P, 3) and not grad.any()
    # with the update skipping on the flag nothing moves
    m, v, sd = torch.zeros_like(feats), torch.zeros_like(feats), step_block(0, 0.0025)
    before = feats.clone()
    upd = _native.LevelsUpdate(feats, m, v, (0.9, 0.999), 1e-15, sd, skip=run.overflow)
    run.backward(feats, images=langs, targets=gts, masks=masks, grad_losses=ones, update=upd)
    assert torch.equal(feats, before) and not m.any() and not v.any()
    assert int(sd[0]) == 0 and int(sd[_native.ADAM_WORD_SKIPPED]) == 1


def make_step(L, cam_key="a", lr=0.0025, **kw):
    model, cams, bg, targets = world()
    feats = torch.nn.Parameter(raw_features(L).clone())
    opt = Adam([{"params": [feats], "lr": lr, "name": "language_feature"}], lr=0.0, eps=1e-15)
    gts, masks = (t[:L].contiguous() for t in targets[cam_key])
    slot = LevelsViewSlot(cams[cam_key], gts, masks)
    return GraphedLevelsStep(model, feats, opt, slot, bench.Pipe, bg, bench.Opt, **kw), feats, opt


def view_of(key, L):
    _, cams, _, targets = world()
    gts, masks = (t[:L].contiguous() for t in targets[key])
    return cams[key], gts, masks


def eager_run(L, keys, lr=0.0025):
    model, _, bg, _ = world()
    feats = torch.nn.Parameter(raw_features(L).clone())
    opt = Adam([{"params": [feats], "lr": lr, "name": "language_feature"}], lr=0.0, eps=1e-15)
    step = levels.LevelsStep(model, feats, opt)
    losses = [step.step(view_of(k, L)[0], bench.Pipe, bg, bench.Opt, *view_of(k, L)[1:]).clone() for k in keys]
    st = opt.state[feats]
    return losses, (feats.detach(), st["exp_avg"], st["exp_avg_sq"]), int(st["step"].item())


def states_of(feats, opt):
    st = opt.state[feats]
    return feats.detach(), st["exp_avg"], st["exp_avg_sq"]


def test_forced_overflow_replay_is_left_out():
    """Five replays, the third over capacity.  The two cameras inside the cube draw fewer tile instances
    than a ring camera, so the capture's headroom is chosen (from the views' eager counts) to give
    capacities the inside views fit and the ring view does not.  The result is the eager run of the
    other four views."""
    model, cams, bg, _ = world()
    L = 3
    counts = {}
    for k in ("inside", "flip", "a"):
        levels.render_levels(cams[k], model, bench.Pipe, bg, bench.Opt, raw_features(L))
        counts[k] = _native.LAST_COUNTS[(P, W, H)]
    print("tile instances, entries per view:", counts)
    fit = max(counts["inside"][0], counts["flip"][0])
    assert fit + 64 < counts["a"][0], "the ring view must draw more tile instances than the inside views"
    # capacity_rendered = int(headroom * count of the warm-up view) + 1024: halfway between the two
    headroom = ((fit + counts["a"][0]) // 2 - 1024) / counts["inside"][0]
    step, feats, opt = make_step(L, "inside", headroom=headroom)
    step.capture(min_entries=max(counts["inside"][1], counts["flip"][1]) + 16)
    assert fit <= step.rendered < counts["a"][0]
    first_caps = (step.rendered, step.entries)
    for k in ("inside", "flip", "a", "inside", "flip"):
        step.replay(view=view_of(k, L))
    assert step.check() is False and step.captures == 2
    assert (step.rendered, step.entries) == (2 * first_caps[0], 2 * first_caps[1])
    assert step.check() is True and step.captures == 2
    step.sync()
    assert int(opt.state[feats]["step"].item()) == 4 and opt.skipped_steps() == 1
    # two eager runs of the four views stay inside the tolerance (atomics), then the captured run against one
    four = ("inside", "flip", "inside", "flip")
    _, eager_a, n_a = eager_run(L, four)
    _, eager_b, _ = eager_run(L, four)
    assert n_a == 4
    assert_states_close(eager_a, eager_b, "eager twice")
    assert_states_close(states_of(feats, opt), eager_a, "overflowed view left out")
    assert not torch.equal(eager_a[0], raw_features(L))


# ---- 6. empty views --------------------------------------------------------------------------------

def test_fully_culled_view_is_an_adam_step_on_zero_gradients():
    model, cams, bg, _ = world()
    L = 3
    feats = raw_features(L)
    rs = camera_settings(cams["away"], model, bench.Pipe, bg, 1.0, True)
    run = Run(rs, model_args(model), 4096, 4096)
    nr, color, langs, radii = run.forward(feats)[:4]
    assert nr == 4096 and int(run.overflow) == 0 and int(radii.abs().max()) == 0
    assert not langs.any() and torch.equal(color, bg[:, None, None].expand(3, H, W))
    g = torch.Generator().manual_seed(3)
    m = (torch.randn((L, P, 3), generator=g) * 1e-3).to(DEV)
    v = (torch.rand((L, P, 3), generator=g) * 1e-6).to(DEV)
    p1, m1, v1 = feats.clone(), m.clone(), v.clone()
    sd, sd1 = step_block(2, 0.0025), step_block(2, 0.0025)
    grad = torch.full((L, P, 3), float("nan"), device=DEV)
    upd = _native.LevelsUpdate(feats, m, v, (0.9, 0.999), 1e-15, sd, skip=run.overflow)
    run.backward(feats, images=langs, targets=torch.ones_like(langs), grad_losses=torch.ones((L,), device=DEV),
                 masks=torch.ones((L, H, W), dtype=torch.bool, device=DEV), update=upd, out=grad)
    assert not grad.any()
    adam_multi(p1, torch.zeros_like(p1), m1, v1, 0.0025, (0.9, 0.999), 1e-15, sd1)
    assert torch.equal(feats, p1) and torch.equal(m, m1) and torch.equal(v, v1)
    assert int(sd[0]) == 3 and int(sd[_native.ADAM_WORD_SKIPPED]) == 0 and not torch.equal(feats, raw_features(L))


def test_an_empty_model_is_a_no_op():
    """P == 0: the forward leaves zero images, the backward returns without enqueuing anything (the step
    block does not advance), as include/lsr.h says."""
    model, cams, bg, _ = world()
    L = 2
    rs = camera_settings(cams["a"], model, bench.Pipe, bg, 1.0, True)
    (xyz, dc, _), (opac, scal, rot, _), kw = model_args(model)
    args = ((xyz[:0], dc[:0], None), (opac[:0], scal[:0], rot[:0], None), dict(raw=RAW, shs_rest=kw["shs_rest"][:0]))
    run = Run(rs, args, 64, 64)
    feats = torch.zeros((L, 0, 3), device=DEV)
    nr, color, langs = run.forward(feats)[:3]
    assert nr == 0 and not langs.any() and not color.any()
    sd = step_block(5, 0.0025)
    empty = torch.zeros((L, 0, 3), device=DEV)
    upd = _native.LevelsUpdate(feats, empty, empty.clone(), (0.9, 0.999), 1e-15, sd)
    grad = run.backward(feats, images=langs, targets=langs.clone(), grad_losses=torch.ones((L,), device=DEV),
                        masks=torch.ones((L, H, W), dtype=torch.bool, device=DEV), update=upd)
    assert grad.shape == (L, 0, 3)
    assert int(sd[0]) == 5 and int(sd[_native.ADAM_WORD_SKIPPED]) == 0


# ---- 7. replays match eager ------------------------------------------------------------------------

SIX = ("a", "b", "a", "b", "a", "b")


@functools.lru_cache(maxsize=None)
def captured_run(view_cache):
    """Six alternating replays from the standard start: (losses, final states, the step object)."""
    step, feats, opt = make_step(3, "a", view_cache=view_cache)
    losses = [step.replay(view=view_of(k, 3)).clone() for k in SIX]
    assert step.check() is True and step.captures == 1
    step.sync()
    return losses, tuple(t.clone() for t in states_of(feats, opt)), step, int(opt.state[feats]["step"].item())


def test_replays_match_the_eager_step():
    want, want_states, n = eager_run(3, SIX)
    got, got_states, step, steps = captured_run(False)
    assert steps == n == 6 and step.geo_replays == 6
    assert torch.equal(got[0], want[0])  # same maps, same loss kernel
    for i in range(1, 6):
        torch.testing.assert_close(got[i], want[i], rtol=1e-5, atol=0)
    assert_states_close(got_states, want_states, "six replays")
    assert float((got[0] - got[4]).min()) > 0  # the losses of view a fell


def test_view_cache_restores_replace_the_geometry_graph():
    plain, plain_states, _, _ = captured_run(False)
    got, got_states, step, steps = captured_run(True)
    assert steps == 6
    assert step.geo_replays == 2  # steps 3-6 are hits
    assert step.view_cache_stats()["hits"] == 4 and step.view_cache_stats()["packs"] == 2
    assert torch.equal(got[0], plain[0])
    for i in range(1, 6):
        torch.testing.assert_close(got[i], plain[i], rtol=1e-5, atol=0)
    assert_states_close(got_states, plain_states, "view cache")


def test_restored_view_gives_the_geometry_calls_maps():
    """lr = 0: the features stay what they are, so a view's maps must be the same bits whether its
    geometry came from G_geo (first visit) or from its pack."""
    step, feats, opt = make_step(3, "a", lr=0.0, view_cache=True)
    start = feats.detach().clone()
    maps = {}
    for i, k in enumerate(("a", "b", "a", "b")):
        step.replay(view=view_of(k, 3))
        out = step.buffers.tensors[("out", "levels_language")].clone()
        if i < 2:
            maps[k] = out
            assert float(out.abs().max()) > 0
        else:
            assert torch.equal(out, maps[k]), k
    assert step.geo_replays == 2 and torch.equal(feats.detach(), start)
    ref = levels.render_levels(view_of("b", 3)[0], world()[0], bench.Pipe, world()[2], bench.Opt, feats.detach())
    assert torch.equal(maps["b"], ref["language_feature_images"])


# ---- 8. invalidation -------------------------------------------------------------------------------

def test_invalidation_drops_the_packs_and_a_replaced_parameter_recaptures():
    step, feats, opt = make_step(3, "a", view_cache=True)
    model = world()[0]
    for k in ("a", "b", "a"):
        step.replay(view=view_of(k, 3))
    assert step.geo_replays == 2
    with torch.no_grad():
        model._xyz.add_(0.0)  # same values, another version
    step.replay(view=view_of("a", 3))
    assert step.geo_replays == 3 and step.view_cache_stats()["drops"] == 1
    step.replay(view=view_of("a", 3))
    assert step.geo_replays == 3
    step.invalidate_views()
    step.replay(view=view_of("a", 3))
    assert step.geo_replays == 4 and step.view_cache_stats()["drops"] == 2
    assert step.check() is True and step.captures == 1
    # replacing the parameter tensor (as densification does to the optimizer's groups) re-captures
    step.sync()
    new = torch.nn.Parameter(feats.detach().clone())
    opt.param_groups[0]["params"][0] = new
    opt.state[new] = opt.state.pop(feats)
    before = new.detach().clone()
    step.replay(view=view_of("b", 3))
    torch.cuda.synchronize()
    assert step.captures == 2 and step.language_features is new
    assert not torch.equal(new.detach(), before)
    assert step.view_cache_stats()["packs"] == 1  # the re-capture started empty


# ---- 9. another stream, repeatability --------------------------------------------------------------

def test_another_stream_and_a_second_capture_give_the_same_losses():
    plain = captured_run(False)[0]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step, _, _ = make_step(3, "a")
        got = [step.replay(view=view_of(k, 3)).clone() for k in SIX[:2]]
    side.synchronize()
    assert torch.equal(got[0], plain[0])
    torch.testing.assert_close(got[1], plain[1], rtol=1e-5, atol=0)
    again, _, _ = make_step(3, "a")
    assert torch.equal(again.replay(view=view_of("a", 3)), plain[0])
