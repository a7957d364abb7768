"""HIP path vs the CPU oracle at the value edges of the blend and of the activations.

The scenes are tests/scenes.py EDGE_SCENES (census counts and what they are for:
tests/test_oracle_value_edges.py, which pins the oracle itself to float64 autograd on them): blends
with o G > 0.99 -- the straight-through clamp, T recovered through v_rcp_f32(0.01), the background
term at the same point --, opacities of exactly 1 and 0 and on both sides of 1/255, colour channels
clamped at 0 beside unclamped ones, zero and denormal-norm quaternions, zero language vectors,
scales that flush to 0.  Every test first asserts that its scene reaches them
(scenes.assert_reaches_edges) and then compares with the ORACLE, never with another GPU path:
  - the full backward, the backward without a colour gradient and the language step's backward
    (geometry outputs NULL: the five-value replay, whose screen-space gradient multiplies by the
    unclamped o G; with the colour image in the loss too) on activated inputs;
  - the fused raw path (activations inside the kernels) chained through oracle.activate_backward:
    saturated logits (sigmoid' underflows to 0), exp(-100), normalize(0) and the zero-norm language
    rows, whose chained gradient is g / 1e-9;
  - the gradient walk of all levels in one pass;
  - the step bench.py times (fused loss) and one captured step with the fused tail against the
    eager epilogue + Adam.
Tolerances are those of tests/test_gpu_parity.py: forward bit-exact (images, radii, ranges, point
list, final T, contributor counts), gradients by assert_grad_close with outliers = 0.  Where a raw
gradient has rows ~1e9 times the others (zero-norm rows), those rows and the rest are compared
separately: under one floor of 1e-2 max the rest would pass whatever it held.
"""
import numpy as np
import pytest
import torch

from langsplat_amd import _native
from langsplat_amd.graph import GraphedStep, ViewSlot
from langsplat_amd.synthetic import make_cameras
from oracle import oracle
from tests.scenes import assert_reaches_edges, edge_case, grad_seed, to_device
from tests.test_gpu_captured_forms import (_adam, _eager_step, _frozen_model, _slot_forward, _state,
                                           assert_states_close)
from tests.test_gpu_levels import level_features
from tests.test_gpu_levels_train import backward as levels_backward, forward as levels_forward, seeds_for
from tests.test_gpu_parity import assert_grad_close, check_backward, check_forward_exact, state
from tests.test_gpu_timed_step import bench_target, gpu_language_step, oracle_language_step

pytestmark = pytest.mark.gpu
DEV = "cuda"


def case(name):
    c = edge_case(name)
    assert_reaches_edges(c.census, c.include_feature)
    return c


def assert_rows_close(name, gpu, ref, rows):
    """assert_grad_close on `rows` (a bool mask) and on the other rows, each with its own floor."""
    gpu, ref = np.asarray(gpu), np.asarray(ref)
    assert rows.any() and not rows.all(), name
    assert_grad_close(name + " (degenerate rows)", gpu[rows], ref[rows])
    assert_grad_close(name + " (other rows)", gpu[~rows], ref[~rows])


def assert_finite_and_culled_zero(g, run):
    culled = torch.from_numpy(run.radii == 0)
    for k, t in g.items():
        if t is not None:
            assert torch.isfinite(t).all(), k
            assert not t.cpu()[culled].any(), k


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_forward_bit_exact_and_full_backward(name):
    c = case(name)
    run, std, ind, out = check_forward_exact(c.st, c.inp, c.run)
    g, _ = check_backward(c.st, c.inp, run, out)
    assert_finite_and_culled_zero(g, run)
    # a Gaussian that is never blended (o == 0, o < 1/255) has an exactly zero gradient
    o = c.inp["opacities"].numpy().reshape(-1)
    assert not g["opacities"].cpu().numpy()[o < 1.0 / 255.0].any()


@pytest.mark.parametrize("name", ["A", "C"])
def test_backward_without_colour_gradient(name):
    """The nine-value replay against the oracle with a zero colour seed."""
    c = case(name)
    run, std, ind, out = check_forward_exact(c.st, c.inp, c.run)
    _, gl = grad_seed(c.st.image_height, c.st.image_width, seed=11)
    ref = run.backward(torch.zeros_like(gl), gl)
    nr, color, lang, radii, geom, binning, image = out
    g = _native.rasterize_gaussians_backward(
        std, ind["means3D"], ind["shs"], None, ind["language_feature_precomp"], ind["scales"], ind["rotations"],
        None, radii, None, gl.to(DEV), nr, geom, binning, image)
    torch.cuda.synchronize()
    assert not g["colors_precomp"].any()
    for n in ("means2D", "opacities", "means3D", "language_feature_precomp", "shs", "scales", "rotations"):
        assert_grad_close(n, g[n].cpu().numpy(), ref[n])
    assert_finite_and_culled_zero(g, run)


@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("name", ["A", "C"])
def test_language_step_backward(name, colour):
    """Frozen geometry (every geometry output NULL): dL/dmeans2D and dL/dlanguage only, against the
    oracle's.  Without the colour seed this is the five-value replay, whose screen-space partials
    are (o G) dL/dalpha with the UNCLAMPED product: alpha in its place would pass every scene
    without a saturated blend.  colour: the colour image is in the loss too."""
    c = case(name)
    run, std, ind, out = check_forward_exact(c.st, c.inp, c.run)
    gc, gl = grad_seed(c.st.image_height, c.st.image_width, seed=11)
    ref = run.backward(gc if colour else torch.zeros_like(gc), gl)
    nr, _, _, radii, geom, binning, image = out
    g = _native.rasterize_gaussians_backward(
        std, ind["means3D"], ind["shs"], None, ind["language_feature_precomp"], ind["scales"], ind["rotations"],
        None, radii, gc.to(DEV) if colour else None, gl.to(DEV), nr, geom, binning, image, geometry=False)
    torch.cuda.synchronize()
    assert all(g[k] is None for k in ("opacities", "means3D", "shs", "scales", "rotations"))
    assert_grad_close("means2D", g["means2D"].cpu().numpy(), ref["means2D"])
    assert_grad_close("language_feature_precomp", g["language_feature_precomp"].cpu().numpy(),
                      ref["language_feature_precomp"])
    assert_finite_and_culled_zero(g, run)
    assert float(np.abs(ref["means2D"]).max()) > 0


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_fused_raw_path(name):
    """Raw parameters in, activations inside the kernels: the forward bit for bit what
    oracle.activate -> oracle.forward gives (the scene's own oracle run), the backward the oracle's
    chained through oracle.activate_backward."""
    c = case(name)
    g, st, run, inc = c.g, c.st, c.run, c.include_feature
    P, W, H = g.P, st.image_width, st.image_height
    std, _ = to_device(st, {}, DEV)
    gd = g.to(DEV)
    raw = _native.RAW_OPACITY | _native.RAW_SCALES | _native.RAW_ROTATIONS | (_native.RAW_LANGUAGE if inc else 0)
    rest = gd.features_rest.contiguous() if gd.features_rest.shape[1] > 0 else None
    out = _native.rasterize_gaussians(std, gd.xyz, gd.features_dc.contiguous(), None,
                                      gd.language_feature if inc else None, gd.opacity, gd.scaling, gd.rotation,
                                      None, raw=raw, shs_rest=rest)
    nr, color, lang, radii, geom, binning, image = out
    assert nr == run.num_rendered
    np.testing.assert_array_equal(radii.cpu().numpy(), run.radii)
    np.testing.assert_array_equal(color.cpu().numpy(), run.color)
    np.testing.assert_array_equal(lang.cpu().numpy(), run.language)
    s = state(out, P, W, H)
    np.testing.assert_array_equal(s["n_contrib"], run.get("n_contrib"))
    np.testing.assert_array_equal(s["final_T"], run.get("final_T"))
    np.testing.assert_array_equal(s["point_list"], run.get("point_list"))

    gc, gl = grad_seed(H, W, seed=4)
    ref = run.backward(gc, gl if inc else None)
    gr = _native.rasterize_gaussians_backward(
        std, gd.xyz, gd.features_dc.contiguous(), None, gd.language_feature if inc else None, gd.scaling,
        gd.rotation, None, radii, gc.to(DEV), gl.to(DEV) if inc else None, nr, geom, binning, image, raw=raw,
        shs_rest=rest, opacities=gd.opacity)
    torch.cuda.synchronize()
    d_op, d_sc, d_rot, d_lang = oracle.activate_backward(
        oracle.RAW_ALL if inc else oracle.RAW_ALL & ~oracle.RAW_LANGUAGE,
        (g.opacity, g.scaling, g.rotation, g.language_feature),
        (ref["opacities"], ref["scales"], ref["rotations"], ref["language_feature_precomp"]))
    assert_grad_close("opacity_raw", gr["opacities"].cpu().numpy(), d_op)
    assert_grad_close("scaling_raw", gr["scales"].cpu().numpy(), d_sc)
    # rows of norm < 1e-12 are divided by the clamp 1e-12, zero-norm language rows by 1e-9
    assert_rows_close("rotation_raw", gr["rotations"].cpu().numpy(), d_rot,
                      np.linalg.norm(g.rotation.numpy().astype(np.float64), axis=1) < 1e-12)
    if inc:
        assert_rows_close("language_raw", gr["language_feature_precomp"].cpu().numpy(), d_lang,
                          ~g.language_feature.numpy().any(1))
    assert_grad_close("means2D", gr["means2D"].cpu().numpy(), ref["means2D"])
    assert_grad_close("means3D", gr["means3D"].cpu().numpy(), ref["means3D"])
    assert_grad_close("features_dc", gr["shs"].cpu().numpy(), ref["shs"][:, :1])
    if rest is not None:
        assert_grad_close("features_rest", gr["shs_rest"].cpu().numpy(), ref["shs"][:, 1:])
    # the saturated logits' sigmoid' underflows: exactly no gradient, whatever the blend gave
    sat = np.abs(g.opacity.numpy().reshape(-1)) == 100.0
    assert not gr["opacities"].cpu().numpy()[sat].any() and not gr["scales"].cpu().numpy()[g.scaling.numpy() == -100.0].any()
    assert_finite_and_culled_zero({k: v for k, v in gr.items() if k != "colors_precomp"}, run)


@pytest.mark.parametrize("name", ["A", "C"])
def test_levels_forward_and_gradient(name):
    """L = 3 over an edge scene's geometry (level 1 with the scene's zero language rows): every
    map bit-exact and every level's gradient against the oracle run of that level."""
    c = case(name)
    st, inp = c.st, c.inp
    P, W, H, L = c.g.P, st.image_width, st.image_height, 3
    feats = level_features(L, P, device="cpu").clone()
    feats[1, ~inp["language_feature_precomp"].numpy().any(1)] = 0.0
    std, ind = to_device(st, inp, DEV)
    fd = feats.to(DEV)
    fwd = levels_forward(std, ind, fd)
    grad = levels_backward(std, fd, fwd, grad_images=seeds_for(L, H, W).to(DEV))
    torch.cuda.synchronize()
    assert fwd[0] == c.run.num_rendered and grad.shape == (L, P, 3)
    np.testing.assert_array_equal(fwd[1].cpu().numpy(), c.run.color)
    np.testing.assert_array_equal(fwd[3].cpu().numpy(), c.run.radii)
    zeros = torch.zeros((3, H, W))
    for l in range(L):
        run = oracle.forward(st, **dict(inp, language_feature_precomp=feats[l].contiguous()))
        np.testing.assert_array_equal(fwd[2][l].cpu().numpy(), run.language)
        ref = run.backward(zeros, grad_seed(H, W, seed=7 + l)[1])["language_feature_precomp"]
        got = grad[l].cpu().numpy()
        assert_grad_close(f"{name} level {l}", got, ref)
        assert np.isfinite(got).all() and not got[c.run.radii == 0].any()


def test_timed_language_step(monkeypatch):
    """Scene A's raw parameters through the step bench.py times: render() with the activations in
    the preprocess, the fused masked L1 and the five-value backward, against the oracle's step."""
    c = case("A")
    W, H = c.st.image_width, c.st.image_height
    cam = make_cameras(1, W, H)[0]
    gt, mask = bench_target(H, W, 0)
    run, loss_ref, d_lang_ref, d_m2_ref = oracle_language_step(c.g, cam, gt, mask)
    np.testing.assert_array_equal(run.language, c.run.language)
    color, lang, radii, loss, d_lang, d_m2 = gpu_language_step(c.g, cam, gt, mask, monkeypatch)
    np.testing.assert_array_equal(radii, run.radii)
    np.testing.assert_array_equal(color, run.color)
    np.testing.assert_array_equal(lang, run.language)
    assert abs(loss - loss_ref) <= 2e-6 * loss_ref, (loss, loss_ref)
    assert_rows_close("language_feature (raw)", d_lang, d_lang_ref, ~c.g.language_feature.numpy().any(1))
    assert_grad_close("viewspace_points", d_m2, d_m2_ref)
    assert not d_lang[run.radii == 0].any() and not d_m2[run.radii == 0].any()


def test_captured_step_with_fused_tail(monkeypatch):
    """One captured step whose backward ends in the fused tail (gradient epilogue, Adam and fill in
    one pass) on scene A, against the eager step's separate epilogue + Adam: the zero-norm visible
    rows (gradient g / 1e-9) and the o == 0 rows (no gradient: parameter and moments untouched) go
    through the tail."""
    monkeypatch.setenv("LANGSPLAT_AMD_FUSED", "1")
    monkeypatch.setenv("LSR_FUSED_TAIL", "1")
    c = case("A")
    W, H = c.st.image_width, c.st.image_height
    cam = make_cameras(1, W, H, device=DEV)[0]
    gt, mask = (t.to(DEV) for t in bench_target(H, W, 0))
    me = _frozen_model(c.g)
    oe = _adam(me)
    loss_e = _eager_step(me, oe, cam, gt, mask)
    se = _state(me, oe)
    m = _frozen_model(c.g)
    opt = _adam(m)
    slot = ViewSlot(cam, gt, mask)
    fwd = _slot_forward(m)

    def step():
        loss = fwd(slot)
        loss.backward()
        return loss
    gs = GraphedStep(step, [m._language_feature], optimizer=opt, view=slot).capture()
    loss = gs.replay().clone()
    torch.cuda.synchronize()
    assert gs.check() and gs.captures == 1
    gs.sync()
    assert int(opt.state[m._language_feature]["step"].item()) == 1
    assert torch.equal(loss, loss_e)
    sg = _state(m, opt)
    assert_states_close(sg, se, "edge scene, fused tail vs eager")
    raw = c.g.language_feature.to(DEV)
    o = c.inp["opacities"].reshape(-1).to(DEV)
    zero_vis = (~raw.any(1)) & torch.from_numpy(c.run.radii > 0).to(DEV)
    assert torch.isfinite(torch.stack(sg)).all()
    assert int(zero_vis.sum()) >= 5 and float(sg[1][zero_vis].abs().max()) > 0
    assert torch.equal(sg[0][o == 0], raw[o == 0]) and not sg[1][o == 0].any() and not sg[2][o == 0].any()
