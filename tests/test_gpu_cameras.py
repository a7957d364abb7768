"""HIP path vs the CPU oracle under rolled, close-in and off-screen cameras.

Every other GPU parity test looks through make_cameras: from 4 units away, with no roll or pitch,
at a cube that is wholly on screen.  The poses of tests/scenes.py POSES stand inside the scene,
roll, and see Gaussians behind and beside them (the geometry LERF cameras have), so these cases
reach what that camera cannot: the EWA window clamp and its zeroed gradient, the viewmatrix
rotation in cov2d and in the preprocess backward, Gaussians behind the near plane or with an
empty tile rectangle mixed in with visible ones (culled depth keys beside the sort's key range,
exactly-zero gradient rows), negative and very large pixel coordinates in tile_rect, and screen
radii several times the image, so that many Gaussians touch every tile.  tests/test_oracle_cameras.py
checks the oracle itself against float64 autograd under the same poses.

The scenes are the smallest that still reach the multi-tile, all-tile and split-replay paths; each
case asserts, from the oracle run, that its scene has what it is there for (at about half the
counts recorded when the cases were chosen).  Tolerances are those of tests/test_gpu_parity.py:
forward bit-exact (images, radii, ranges, point list, final T, contributor counts), gradients by
assert_grad_close without outliers.
"""
import functools

import numpy as np
import pytest
import torch

from langsplat_amd import _native
from langsplat_amd.rasterizer import GaussianRasterizer
from langsplat_amd.synthetic import make_gaussians
from oracle import oracle
from tests.scenes import POSES, grad_seed, posed_camera, posed_scene, to_device, view_space, window_clamped
from tests.test_gpu_parity import assert_grad_close, check_backward, check_forward_exact, native_forward, state
from tests.test_gpu_timed_step import bench_target, gpu_language_step, oracle_language_step

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = {
    "A": dict(pose="inside", P=3000, W=160, H=120, seed=1, scale_range=(0.02, 0.12)),
    "B": dict(pose="inside_flip", P=3000, W=160, H=120, seed=2, scale_range=(0.02, 0.12), scale_modifier=1.3),
    "C": dict(pose="grazing", P=4000, W=131, H=77, seed=3, scale_range=(0.02, 0.12)),
    "D": dict(pose="rolled", P=2000, W=128, H=96, seed=4, scale_range=(0.03, 0.2)),
    "E": dict(pose="inside", P=20000, W=96, H=80, seed=5, scale_range=(0.02, 0.12)),
}
TINY = [(1, 1), (7, 5), (16, 16), (17, 33)]


@functools.lru_cache(maxsize=None)
def case(name, include_feature=True):
    """(settings, inputs, oracle run) of a case, computed once and shared; nobody changes them."""
    st, inp = posed_scene(sh_degree=3, include_feature=include_feature, **CASES[name])
    return st, inp, oracle.forward(st, **inp)


def facts(st, inp, run):
    """What a scene exercises, from the oracle run and the float64 view-space centres."""
    vis = run.radii > 0
    near = view_space(st, inp["means3D"])[:, 2] <= 0.2
    tiles = run.gx * run.gy
    return dict(visible=int(vis.sum()), near=int(near.sum()), other=int((~vis & ~near).sum()),
                clamped=int((vis & window_clamped(st, inp["means3D"])).sum()),
                all_tiles=int((run.get("tiles_touched") == tiles).sum()), max_radius=int(run.radii.max()),
                n_contrib=int(run.get("n_contrib").max()), instances=run.num_rendered)


def assert_exercises(name, st, inp, run):
    f = facts(st, inp, run)
    if name == "A":  # near-culled, otherwise culled and clamped among visible; radii beyond the image
        assert f["visible"] >= 600 and f["near"] >= 300 and f["other"] >= 500 and f["clamped"] >= 100, f
        assert f["all_tiles"] >= 4 and f["max_radius"] > 160 and f["instances"] >= 7000, f
    elif name == "B":  # the same through a flipped camera and a modifier; past the split replay boundary
        assert f["visible"] >= 700 and f["clamped"] >= 250 and f["all_tiles"] >= 13, f
        assert f["n_contrib"] > 256 and f["max_radius"] > 160, f
    elif name == "C":  # most Gaussians beside the frustum: empty rectangles from far off-screen centres
        assert f["visible"] >= 650 and f["other"] >= 1300 and f["clamped"] >= 90 and f["n_contrib"] > 256, f
    elif name == "D":  # everything visible through a rotation with no zero entry
        assert f["visible"] == CASES["D"]["P"] and f["n_contrib"] > 512, f
        assert (np.abs(st.viewmatrix.numpy()[:3, :3] - np.eye(3)) > 0.1).sum() >= 6
    else:  # E: many Gaussians on every tile (super-tile counts, placed emission, cover masks)
        assert f["visible"] >= 3800 and f["near"] >= 2500 and f["all_tiles"] >= 48 and f["instances"] >= 24000, f


def assert_culled_rows_zero_and_finite(g, run):
    culled = torch.from_numpy(run.radii == 0)
    for name, t in g.items():
        if t is None:
            continue
        t = t.cpu()
        assert torch.isfinite(t).all(), name
        assert not t[culled].any(), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_posed_forward_bit_exact_and_backward(name):
    st, inp, run = case(name)
    assert_exercises(name, st, inp, run)
    run, std, ind, out = check_forward_exact(st, inp, run)
    # a culled Gaussian's depth key is the sentinel, above every visible key (positive floats)
    keys = state(out, CASES[name]["P"], st.image_width, st.image_height)["depth_key"]
    vis = run.radii > 0
    np.testing.assert_array_equal(keys[vis], run.get("depth")[vis].view(np.uint32))
    assert np.all(keys[~vis] == 0xFFFFFFFF) and keys[vis].max() < 0x7F800000
    g, _ = check_backward(st, inp, run, out)
    assert_culled_rows_zero_and_finite(g, run)


@pytest.mark.parametrize("name", ["A", "B"])
def test_posed_without_language_feature(name):
    st, inp, run = case(name, include_feature=False)
    run, std, ind, out = check_forward_exact(st, inp, run)
    g, _ = check_backward(st, inp, run, out)
    assert not run.language.any()
    assert_culled_rows_zero_and_finite({k: v for k, v in g.items() if k != "language_feature_precomp"}, run)


def test_posed_colors_precomp_and_cov3d_precomp():
    """Case A through colors_precomp + cov3D_precomp (test_colors_precomp_and_cov3d_precomp_paths)."""
    st, inp, run0 = case("A")
    inp2 = dict(inp)
    del inp2["shs"], inp2["scales"], inp2["rotations"]
    # the oracle keeps rgb of visible Gaussians only: a culled row's colour is never read
    inp2["colors_precomp"] = torch.tensor(run0.get("rgb"))
    inp2["cov3D_precomp"] = torch.tensor(oracle.cov3d(inp["scales"].numpy(), 1.0, inp["rotations"].numpy()))
    run, std, ind, out = check_forward_exact(st, inp2)
    np.testing.assert_array_equal(run.radii, run0.radii)
    g, _ = check_backward(st, inp2, run, out)
    assert_culled_rows_zero_and_finite(g, run)


def test_posed_backward_without_colour_gradient():
    """Case A through the backward specialised on a zero colour gradient
    (test_backward_without_colour_gradient)."""
    st, inp, run = case("A")
    run, std, ind, out = check_forward_exact(st, inp, run)
    _, gl = grad_seed(st.image_height, st.image_width, seed=11)
    ref = run.backward(torch.zeros_like(gl), gl)
    nr, color, lang, radii, geom, binning, image = out
    g = _native.rasterize_gaussians_backward(
        std, ind["means3D"], ind["shs"], None, ind["language_feature_precomp"], ind["scales"], ind["rotations"],
        None, radii, None, gl.to(DEV), nr, geom, binning, image)
    torch.cuda.synchronize()
    assert not g["colors_precomp"].any()
    for n in ("means2D", "opacities", "means3D", "language_feature_precomp", "shs", "scales", "rotations"):
        assert_grad_close(n, g[n].cpu().numpy(), ref[n])
    assert_culled_rows_zero_and_finite(g, run)


def test_posed_timed_language_step(monkeypatch):
    """Case A's raw parameters and camera through the step bench.py times: render() with the
    activations inside k_preprocess, the fused masked L1 and the 5-value backward.  Criteria of
    test_timed_language_step_matches_oracle."""
    c = CASES["A"]
    W, H = c["W"], c["H"]
    g = make_gaussians(c["P"], seed=c["seed"], sh_degree=3, scale_range=c["scale_range"])
    cam = posed_camera(*POSES[c["pose"]], W, H)
    gt, mask = bench_target(H, W, 0)
    run, loss_ref, d_lang_ref, d_m2_ref = oracle_language_step(g, cam, gt, mask)
    assert run.blends > 0
    assert (run.radii == 0).sum() >= 900 and (run.get("tiles_touched") == run.gx * run.gy).sum() >= 4
    color, lang, radii, loss, d_lang, d_m2 = gpu_language_step(g, cam, gt, mask, monkeypatch)
    np.testing.assert_array_equal(radii, run.radii)
    np.testing.assert_array_equal(color, run.color)
    np.testing.assert_array_equal(lang, run.language)
    assert abs(loss - loss_ref) <= 2e-6 * loss_ref, (loss, loss_ref)
    assert_grad_close("language_feature (raw)", d_lang, d_lang_ref)
    assert_grad_close("viewspace_points", d_m2, d_m2_ref)
    assert np.abs(d_lang).sum() > 0
    assert not d_lang[run.radii == 0].any() and not d_m2[run.radii == 0].any()


@pytest.mark.parametrize("knob", ["LSR_PLACED=0", "LSR_PLACED=1", "LSR_DEPTH_LSD=1", "LSR_MSD_BUCKETS=512"])
@pytest.mark.parametrize("name", ["A", "E"])
def test_posed_emission_and_sort_variants(name, knob, monkeypatch):
    """Both emissions of the super-tile entries and every depth order, on scenes where about half
    the depth keys are the culled sentinel and the visible depths span roughly 0.2 to 2."""
    st, inp, run = case(name)
    depth = run.get("depth")[run.radii > 0]
    assert depth.min() < 0.25 and depth.max() > 1.5 and (run.radii == 0).sum() >= CASES[name]["P"] // 2
    monkeypatch.setenv(*knob.split("="))
    check_forward_exact(st, inp, run)


@pytest.mark.parametrize("W,H", TINY)
def test_images_smaller_than_a_tile(W, H):
    """One pixel, less than a tile, exactly one tile, one tile and a bit (the scenes of
    tests/test_oracle_cameras.py)."""
    st, inp = posed_scene("inside", 200, W, H, 6, sh_degree=3, scale_range=(0.03, 0.2), bg=(0.3, 0.1, 0.7))
    run, std, ind, out = check_forward_exact(st, inp)
    assert run.blends > 0
    g, _ = check_backward(st, inp, run, out)
    assert_culled_rows_zero_and_finite(g, run)


def test_mark_visible_matches_the_near_plane_test():
    """markVisible is the near-plane test view depth > 0.2 of the preprocess (the upstream
    in_frustum): against the float64 depth wherever that is not within 1e-6 of the plane, and
    against the oracle's own fp32 depth on every Gaussian it kept."""
    st, inp, run = case("A")
    std, ind = to_device(st, inp, DEV)
    vis = GaussianRasterizer(std).markVisible(ind["means3D"]).cpu().numpy()
    assert vis.dtype == bool and vis.shape == (CASES["A"]["P"],)
    depth = view_space(st, inp["means3D"])[:, 2]
    decided = np.abs(depth - 0.2) > 1e-6
    assert (~decided).mean() < 0.01
    np.testing.assert_array_equal(vis[decided], (depth > 0.2)[decided])
    assert vis.any() and not vis.all()
    kept = run.radii > 0
    assert (run.get("depth")[kept] > 0.2).all() and vis[kept].all()
    np.testing.assert_allclose(run.get("depth")[kept], depth[kept], atol=1e-6, rtol=0)


def test_prefiltered_error_and_recovery():
    """prefiltered=True promises that every Gaussian passes the frustum test.  Case D keeps the
    promise (same bit-exact forward); case A breaks it: a host-side status return
    (LSR_ERR_PREFILTERED) raised as RuntimeError, after which the same thread's next forward is
    again bit-exact."""
    std_, inpd, rund = case("D")
    sta, inpa, _ = case("A")
    pre = std_._replace(prefiltered=True)
    check_forward_exact(pre, inpd, rund)
    with pytest.raises(RuntimeError, match="prefiltered"):
        native_forward(sta._replace(prefiltered=True), inpa)
    torch.cuda.synchronize()
    run, std, ind, out = check_forward_exact(pre, inpd, rund)
    check_backward(pre, inpd, run, out)
