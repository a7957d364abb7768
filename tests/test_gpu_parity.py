"""HIP path (liblsr.so through the C ABI) vs the CPU oracle -- the parity gate.

Forward: bit-exact (images, radii, per-tile ranges and Gaussian order, final T, contributor
counts), because kernels and oracle evaluate the same IEEE operation sequence.
Backward: the GPU sums per-Gaussian partials with float atomics in arbitrary order, the oracle in
double; tolerance (north_star: 1e-4 relative) is |gpu - oracle| <= 1e-4 * (|oracle| + floor) with
floor = 1e-2 * max|oracle| per tensor, i.e. relative error 1e-4 except near-zero entries.
"""
import math

import numpy as np
import pytest
import torch

from langsplat_amd import _native
from langsplat_amd.rasterizer import GaussianRasterizer
from oracle import oracle
from tests.scenes import grad_seed, scene, settings_for, to_device
from langsplat_amd.camera import look_at_origin, make_camera
from langsplat_amd.synthetic import CONFIGS, activated_inputs, make_cameras, make_gaussians

pytestmark = pytest.mark.gpu
DEV = "cuda"

GRAD_RTOL = 1e-4
GRAD_FLOOR = 1e-2


def native_forward(st, inp):
    std, ind = to_device(st, inp, DEV)
    out = _native.rasterize_gaussians(std, ind["means3D"], ind.get("shs"), ind.get("colors_precomp"),
                                      ind.get("language_feature_precomp") if st.include_feature else None,
                                      ind["opacities"], ind.get("scales"), ind.get("rotations"),
                                      ind.get("cov3D_precomp"))
    torch.cuda.synchronize()
    return std, ind, out


def state(out, P, W, H):
    nr, color, lang, radii, geom, binning, image = out
    lay = _native.state_layout(P, W, H, nr)
    T = ((W + 15) // 16) * ((H + 15) // 16)

    def u32(buf, off, n):
        return buf[off:off + 4 * n].view(torch.int32).cpu().numpy().view(np.uint32)

    return dict(
        ranges=u32(image, lay["ranges"], 2 * T).reshape(T, 2),
        point_list=u32(binning, lay["point_list"], nr),
        final_T=image[lay["final_T"]:lay["final_T"] + 4 * W * H].view(torch.float32).cpu().numpy().reshape(H, W),
        n_contrib=u32(image, lay["n_contrib"], W * H).reshape(H, W),
        depth_key=u32(geom, lay["depth_key"], P),
        counters=u32(image, lay["counters"], 16),
    )


def check_forward_exact(st, inp, run=None):
    P = inp["means3D"].shape[0]
    W, H = st.image_width, st.image_height
    if run is None:
        run = oracle.forward(st, **inp)
    std, ind, out = native_forward(st, inp)
    nr, color, lang, radii, geom, binning, image = out
    assert nr == run.num_rendered
    np.testing.assert_array_equal(radii.cpu().numpy(), run.radii)
    np.testing.assert_array_equal(color.cpu().numpy(), run.color)
    np.testing.assert_array_equal(lang.cpu().numpy(), run.language)
    if P > 0:
        s = state(out, P, W, H)
        rg = run.get("ranges")
        gr = s["ranges"]
        nonempty = rg[:, 1] > rg[:, 0]
        np.testing.assert_array_equal(gr[nonempty], rg[nonempty])
        assert np.all(gr[~nonempty, 1] == gr[~nonempty, 0])
        np.testing.assert_array_equal(s["point_list"], run.get("point_list"))
        np.testing.assert_array_equal(s["final_T"], run.get("final_T"))
        np.testing.assert_array_equal(s["n_contrib"], run.get("n_contrib"))
    return run, std, ind, out


def assert_grad_close(name, gpu, ref, outliers=0.0):
    """|gpu - ref| <= 1e-4 (|ref| + floor) everywhere, or -- `outliers` > 0, the full-size tests --
    on all but that fraction of the entries, which must still be within 1e-3.

    Why full size needs the allowance: the scale/rotation gradients sum many per-pixel terms that
    cancel, so they move by ~1e-4 of the floored scale under ANY 1-ulp change of the fp32
    evaluation.  Measured on the C3 scene with the oracle itself: T * (1/(1-alpha)) instead of
    T / (1-alpha) moves 2 of 4M rotation entries past 1e-4 (worst 1.26e-4); G one ulp up moves the
    worst rotation entry by 7.8e-5.  The GPU's float atomics and v_rcp_f32 are such changes."""
    gpu = np.asarray(gpu, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert gpu.shape == ref.shape, name
    floor = GRAD_FLOOR * (np.max(np.abs(ref)) if ref.size else 0.0) + 1e-30
    # (not `>`: a NaN -- a sum started from uninitialised records, say -- compares false both ways)
    bad = ~(np.abs(gpu - ref) <= GRAD_RTOL * (np.abs(ref) + floor))
    if outliers > 0.0 and bad.sum() <= outliers * bad.size:
        bad = ~(np.abs(gpu - ref) <= 10 * GRAD_RTOL * (np.abs(ref) + floor))
    if bad.any():
        i = np.argmax(np.abs(gpu - ref) / (np.abs(ref) + floor))
        raise AssertionError(f"{name}: {bad.sum()} / {bad.size} entries off; worst gpu={gpu.flat[i]} "
                             f"ref={ref.flat[i]} floor={floor}")


def check_backward(st, inp, run, out, seed=7, outliers=0.0):
    W, H = st.image_width, st.image_height
    gc, gl = grad_seed(H, W, seed=seed)
    ref = run.backward(gc, gl if st.include_feature else None)
    nr, color, lang, radii, geom, binning, image = out
    std, ind = to_device(st, inp, DEV)
    g = _native.rasterize_gaussians_backward(
        std, ind["means3D"], ind.get("shs"), ind.get("colors_precomp"),
        ind.get("language_feature_precomp") if st.include_feature else None, ind.get("scales"),
        ind.get("rotations"), ind.get("cov3D_precomp"), radii, gc.to(DEV), gl.to(DEV) if st.include_feature else None,
        nr, geom, binning, image)
    torch.cuda.synchronize()
    names = ["means2D", "colors_precomp", "opacities", "means3D"]
    if st.include_feature:
        names.append("language_feature_precomp")
    if "shs" in inp:
        names.append("shs")
    if "cov3D_precomp" in inp:
        names.append("cov3D_precomp")
    else:
        names += ["scales", "rotations"]
    for n in names:
        assert_grad_close(n, g[n].cpu().numpy(), ref[n], outliers)
    return g, ref


CASES = [
    dict(P=300, W=64, H=48, seed=0, sh_degree=3),
    dict(P=500, W=67, H=45, seed=1, sh_degree=2, bg=(0.2, 0.5, 0.9)),
    dict(P=400, W=48, H=40, seed=2, sh_degree=1, include_feature=False),
    dict(P=400, W=80, H=64, seed=3, sh_degree=0, scale_modifier=1.3),
    dict(P=2000, W=128, H=96, seed=4, sh_degree=3, bg=(1.0, 1.0, 1.0)),
]


@pytest.mark.parametrize("case", CASES)
def test_forward_bit_exact_and_backward(case):
    st, inp = scene(scale_range=(0.03, 0.2), **case)
    run, std, ind, out = check_forward_exact(st, inp)
    check_backward(st, inp, run, out)


@pytest.mark.parametrize("seed", [0, 5])
def test_backward_without_colour_gradient(seed):
    """LangSplat's language-feature step: the colour image does not reach the loss, autograd hands
    the backward None, and the kernel specialised on a zero colour gradient must match the oracle
    run with dL/dcolor = 0 (and give a zero colour gradient)."""
    st, inp = scene(P=1500, W=96, H=80, seed=seed, sh_degree=3, scale_range=(0.03, 0.2))
    run, std, ind, out = check_forward_exact(st, inp)
    W, H = st.image_width, st.image_height
    _, gl = grad_seed(H, W, seed=11)
    ref = run.backward(torch.zeros_like(gl), gl)
    nr, color, lang, radii, geom, binning, image = out
    g = _native.rasterize_gaussians_backward(
        std, ind["means3D"], ind["shs"], None, ind["language_feature_precomp"], ind["scales"], ind["rotations"],
        None, radii, None, gl.to(DEV), nr, geom, binning, image)
    torch.cuda.synchronize()
    assert not g["colors_precomp"].any()
    for n in ("means2D", "opacities", "means3D", "language_feature_precomp", "shs", "scales", "rotations"):
        assert_grad_close(n, g[n].cpu().numpy(), ref[n])


def test_colors_precomp_and_cov3d_precomp_paths():
    st, inp = scene(P=400, W=64, H=48, seed=11, sh_degree=3, scale_range=(0.03, 0.2))
    run0 = oracle.forward(st, **inp)
    rgb = torch.tensor(run0.get("rgb"))
    inp2 = dict(inp)
    del inp2["shs"]
    inp2["colors_precomp"] = rgb.clone()
    cov = torch.tensor(oracle.cov3d(inp["scales"].numpy(), 1.0, inp["rotations"].numpy()))
    del inp2["scales"], inp2["rotations"]
    inp2["cov3D_precomp"] = cov
    run, std, ind, out = check_forward_exact(st, inp2)
    check_backward(st, inp2, run, out)


def test_empty_and_fully_culled():
    st, inp = scene(P=50, W=32, H=32, seed=0)
    empty = {k: v[:0] for k, v in inp.items()}
    st_bg = st._replace(bg=torch.tensor([0.3, 0.3, 0.3]))
    check_forward_exact(st_bg, empty)
    culled = dict(inp)
    culled["means3D"] = inp["means3D"] * 0.01 + torch.tensor([0.0, 0.0, -3.9])  # behind the near plane
    run, std, ind, out = check_forward_exact(st_bg, culled)
    assert out[0] == 0
    np.testing.assert_array_equal(out[1].cpu().numpy(), np.broadcast_to(np.float32(0.3), (3, 32, 32)))


def test_very_long_tile_lists():
    """> 8192 instances in one tile (dense cluster): long per-tile lists, many LDS batches."""
    P = 12000
    g = torch.Generator().manual_seed(9)
    W = H = 32
    cam = make_cameras(1, W, H)[0]
    st = settings_for(cam, sh_degree=0)
    inp = dict(means3D=(torch.rand((P, 3), generator=g) - 0.5) * 0.05,
               opacities=torch.rand((P, 1), generator=g) * 0.05 + 0.004,
               colors_precomp=torch.rand((P, 3), generator=g),
               language_feature_precomp=torch.nn.functional.normalize(torch.randn((P, 3), generator=g)),
               scales=torch.full((P, 3), 0.01), rotations=torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(P, 1))
    run, std, ind, out = check_forward_exact(st, inp)
    assert np.diff(run.get("ranges").astype(np.int64), axis=1).max() > 8192
    check_backward(st, inp, run, out)


def test_large_gaussian_covering_all_tiles():
    W, H = 100, 70
    cam = make_cameras(1, W, H)[0]
    st = settings_for(cam, sh_degree=0, bg=(0.1, 0.2, 0.3))
    inp = dict(means3D=torch.tensor([[0.0, 0.0, 0.0], [0.1, 0.1, 0.5]]), opacities=torch.tensor([[0.7], [0.5]]),
               colors_precomp=torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]),
               language_feature_precomp=torch.tensor([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]),
               scales=torch.tensor([[3.0, 3.0, 3.0], [0.1, 0.2, 0.3]]),
               rotations=torch.nn.functional.normalize(torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.3, 0.2, 0.1, 0.9]])))
    run, std, ind, out = check_forward_exact(st, inp)
    check_backward(st, inp, run, out)


def test_c1_config_parity():
    """BASELINE.json configs[0]: 10k Gaussians, 400x300, 3-ch language feature."""
    c = CONFIGS["C1"]
    g = make_gaussians(c["P"], seed=0)
    cam = make_cameras(1, c["width"], c["height"])[0]
    st = settings_for(cam, sh_degree=3)
    with torch.no_grad():
        inp = {k: v.contiguous() for k, v in activated_inputs(g).items()}
    run, std, ind, out = check_forward_exact(st, inp)
    check_backward(st, inp, run, out)


def test_autograd_api_end_to_end():
    """GaussianRasterizer + torch.autograd (the render() path) reproduce the oracle gradients,
    including the means2D sink and needs_input_grad handling."""
    st, inp = scene(P=600, W=64, H=48, seed=21, scale_range=(0.03, 0.2))
    run = oracle.forward(st, **inp)
    gc, gl = grad_seed(48, 64, seed=3)
    ref = run.backward(gc, gl)
    std, ind = to_device(st, inp, DEV)
    leaves = {k: v.clone().requires_grad_(True) for k, v in ind.items()}
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    rast = GaussianRasterizer(std)
    color, lang, radii = rast(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"],
                              shs=leaves["shs"], language_feature_precomp=leaves["language_feature_precomp"],
                              scales=leaves["scales"], rotations=leaves["rotations"])
    np.testing.assert_array_equal(color.detach().cpu().numpy(), run.color)
    np.testing.assert_array_equal(lang.detach().cpu().numpy(), run.language)
    ((color * gc.to(DEV)).sum() + (lang * gl.to(DEV)).sum()).backward()
    assert_grad_close("means2D", means2D.grad.cpu().numpy(), ref["means2D"])
    for k in ("means3D", "opacities", "shs", "scales", "rotations", "language_feature_precomp"):
        assert_grad_close(k, leaves[k].grad.cpu().numpy(), ref[k])
    vis = rast.markVisible(ind["means3D"]).cpu().numpy()
    assert vis.dtype == bool and vis.shape == (600,)


def test_forward_is_deterministic():
    st, inp = scene(P=3000, W=160, H=120, seed=5, scale_range=(0.03, 0.2))
    _, _, out1 = native_forward(st, inp)
    _, _, out2 = native_forward(st, inp)
    for a, b in zip(out1[1:4], out2[1:4]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("cfg", ["C2", "C3"])
def test_full_size_oracle_parity(cfg):
    """BASELINE.json configs[1] and [2] at full size against the C oracle (~10-20 s of oracle time):
    forward bit-exact (images, radii, tile ranges, per-tile order, final T, contributor counts),
    every gradient within the 1e-4 relative tolerance on all but 1e-5 of its entries (and those
    within 1e-3: assert_grad_close)."""
    c = CONFIGS[cfg]
    g = make_gaussians(c["P"], seed=0)
    cam = make_cameras(1, c["width"], c["height"])[0]
    st = settings_for(cam, sh_degree=3)
    with torch.no_grad():
        inp = {k: v.contiguous() for k, v in activated_inputs(g).items()}
    run, std, ind, out = check_forward_exact(st, inp)
    assert run.blends > 0
    check_backward(st, inp, run, out, seed=3, outliers=1e-5)


def test_full_size_oracle_parity_C5(monkeypatch):
    """BASELINE.json configs[4]'s scene (3M Gaussians, 1920x1080, camera 0): above 2M Gaussians the
    depth order's MSD pass makes 512 buckets, checked here at full size against the oracle -- forward
    bit-exact (images, radii, tile ranges, per-tile order, final T, contributor counts) and every
    gradient within the tolerance of test_full_size_oracle_parity -- and the LSD passes (the order
    above 4.2M Gaussians, LSR_DEPTH_LSD=1) give the same bit-exact forward."""
    c = CONFIGS["C5"]
    g = make_gaussians(c["P"], seed=0)
    cam = make_cameras(1, c["width"], c["height"])[0]
    st = settings_for(cam, sh_degree=3)
    with torch.no_grad():
        inp = {k: v.contiguous() for k, v in activated_inputs(g).items()}
    run = oracle.forward(st, **inp)
    assert run.blends > 0
    run, std, ind, out = check_forward_exact(st, inp, run)
    check_backward(st, inp, run, out, seed=3, outliers=1e-5)
    del std, ind, out
    monkeypatch.setenv("LSR_DEPTH_LSD", "1")
    check_forward_exact(st, inp, run)


@pytest.mark.parametrize("cfg", ["C2", "C3", "C5"])
def test_full_size_properties(cfg):
    """BASELINE.json full sizes: per-tile lists sorted by (depth, id), instance accounting, and the
    backward is linear in the upstream gradient (size-independent properties)."""
    c = CONFIGS[cfg]
    g = make_gaussians(c["P"], seed=0)
    cam = make_cameras(1, c["width"], c["height"])[0]
    st = settings_for(cam, sh_degree=3)
    with torch.no_grad():
        inp = {k: v.contiguous() for k, v in activated_inputs(g).items()}
    std, ind, out = native_forward(st, inp)
    nr, color, lang, radii, geom, binning, image = out
    P, W, H = c["P"], c["width"], c["height"]
    s = state(out, P, W, H)
    assert s["counters"][1] == nr
    rg = s["ranges"].astype(np.int64)
    assert np.diff(rg, axis=1).sum() == nr
    # sortedness within every tile: (depth key, id) ascending; tiles laid out in tile order
    pl = s["point_list"].astype(np.int64)
    dk = s["depth_key"].astype(np.int64)
    key = dk[pl] * (1 << 32) + pl
    nonempty = np.nonzero(rg[:, 1] > rg[:, 0])[0]
    assert np.all(rg[nonempty[1:], 0] == rg[nonempty[:-1], 1]) and rg[nonempty[0], 0] == 0
    tile_of = np.repeat(nonempty, (rg[nonempty, 1] - rg[nonempty, 0]))
    same = tile_of[1:] == tile_of[:-1]
    assert np.all(key[1:][same] > key[:-1][same])
    # every visible Gaussian appears exactly tiles_touched times
    counts = np.bincount(pl, minlength=P)
    rad = radii.cpu().numpy()
    assert np.all((counts > 0) == (rad > 0))
    # determinism of the full-size forward
    _, _, out2 = native_forward(st, inp)
    assert torch.equal(out2[1], color) and torch.equal(out2[2], lang)
    # linearity of the backward in (dL/dcolor, dL/dlang)
    g1 = grad_seed(H, W, seed=1, scale=1.0 / (3 * H * W))
    g2 = grad_seed(H, W, seed=2, scale=1.0 / (3 * H * W))
    args = (ind["means3D"], ind["shs"], None, ind["language_feature_precomp"], ind["scales"], ind["rotations"],
            None, radii)

    def bwd(gcol, glang):
        return _native.rasterize_gaussians_backward(std, *args, gcol.to(DEV), glang.to(DEV), nr, geom, binning,
                                                    image)
    ga, gb = bwd(*g1), bwd(*g2)
    gab = bwd(g1[0] + g2[0], g1[1] + g2[1])
    for k in ("means2D", "opacities", "language_feature_precomp", "colors_precomp"):
        lhs = gab[k].double()
        rhs = ga[k].double() + gb[k].double()
        scale = rhs.abs().max().item() + 1e-30
        assert (lhs - rhs).abs().max().item() <= 1e-3 * scale, k


@pytest.mark.parametrize("order", ["msd", "msd512", "msd_items8", "msd512_items4", "lsd"])
@pytest.mark.parametrize("kind", ["wide", "narrow", "ties", "cluster"])
def test_depth_sort_pass_counts(kind, order, monkeypatch):
    """The depth sort orders only the bits the visible keys span (key - min): a depth range of
    0.3..80 spans 27 bits, a sliver 12, exact ties none (id order).  cluster: 20k of 30k Gaussians
    within 1e-3 of one depth, the rest over 0.5..50 -- one top-digit bucket far larger than the
    MSD sort's LDS capacity (its global fallback).  The per-tile order (and everything downstream)
    must stay bit-identical to the oracle's.  msd512: the 512-bucket MSD pass of 2M..4.2M Gaussians
    (LSR_MSD_BUCKETS=512, 8-key radix tiles); the _items variants swap the MSD pass's tile sizes
    (LSR_MSD_ITEMS); lsd: the LSD passes larger P uses (LSR_DEPTH_LSD=1), with the host's pass count:
    4 passes, 2, none."""
    if order == "lsd":
        monkeypatch.setenv("LSR_DEPTH_LSD", "1")
    if order.startswith("msd512"):
        monkeypatch.setenv("LSR_MSD_BUCKETS", "512")
    if "_items" in order:
        monkeypatch.setenv("LSR_MSD_ITEMS", order[-1])
    g = torch.Generator().manual_seed({"wide": 31, "narrow": 32, "ties": 33, "cluster": 34}[kind])
    P, W, H = (30000, 160, 120) if kind == "cluster" else (3000, 96, 64)
    cam = make_cameras(1, W, H)[0]  # at (0, 0, -4) looking along +z: view depth = z + 4
    if kind == "wide":
        d = torch.exp(torch.rand(P, generator=g) * (math.log(80.0) - math.log(0.3)) + math.log(0.3))
    elif kind == "narrow":
        d = 4.0 + torch.rand(P, generator=g) * 1e-3
    elif kind == "cluster":
        d = torch.exp(torch.rand(P, generator=g) * (math.log(50.0) - math.log(0.5)) + math.log(0.5))
        d[torch.randperm(P, generator=g)[:20000]] = 4.0 + torch.rand(20000, generator=g) * 1e-3
    else:
        d = torch.full((P,), 4.0)
    u, v = torch.rand(P, generator=g) * 2 - 1, torch.rand(P, generator=g) * 2 - 1
    means = torch.stack([u * d * 0.4, v * d * 0.3, d - 4.0], 1)
    if kind == "ties":
        means[P // 2:] = means[:P - P // 2]  # exact duplicates: equal keys, order by id
    inp = dict(means3D=means, opacities=torch.rand((P, 1), generator=g) * 0.6 + 0.05,
               colors_precomp=torch.rand((P, 3), generator=g),
               language_feature_precomp=torch.nn.functional.normalize(torch.randn((P, 3), generator=g)),
               scales=torch.full((P, 3), 0.02) * d[:, None] / 4.0,
               rotations=torch.nn.functional.normalize(torch.randn((P, 4), generator=g)))
    st = settings_for(cam, sh_degree=0)
    run, std, ind, out = check_forward_exact(st, inp)
    assert out[0] > 0
    check_backward(st, inp, run, out)


def test_lookback_stall_fallback_is_exact():
    """Every single-pass look-back (depth-sort histogram scans, super-tile offset scan, binning
    table scan, the placed emission's per-super-tile prefix sums) forced onto its stall path (spin limit 0: no chunk waits for its predecessors; each
    computes its prefix from the input instead) gives the same bit-exact forward, and the event is
    reported by lsr_debug_scan_stalls."""
    lib = _native.load()
    st, inp = scene(P=40000, W=320, H=240, seed=8, sh_degree=1, scale_range=(0.01, 0.06))
    run = oracle.forward(st, **inp)
    torch.cuda.synchronize()
    lib.lsr_debug_scan_stalls()  # clear
    old = lib.lsr_debug_set_spin_limit(0)
    try:
        run, std, ind, out = check_forward_exact(st, inp, run)
        torch.cuda.synchronize()
        assert lib.lsr_debug_scan_stalls() == 1
    finally:
        lib.lsr_debug_set_spin_limit(old)
    check_forward_exact(st, inp, run)
    torch.cuda.synchronize()
    assert lib.lsr_debug_scan_stalls() == 0


def test_binning_buffer_grows_between_views():
    """The forward requests its binning buffer before the host wait, sized from the thread's last
    forward of the same P and image size; a view with many more tile instances must get a larger
    buffer after the wait.  Far camera first (few instances), then a close one: both bit-exact."""
    P, W, H = 4000, 128, 96
    g = make_gaussians(P, seed=12, scale_range=(0.01, 0.05))
    with torch.no_grad():
        inp = {k: v.contiguous() for k, v in activated_inputs(g).items()}
    far = make_cameras(1, W, H, radius=12.0)[0]
    near = make_cameras(1, W, H, radius=2.5)[0]
    runs = []
    for cam in (far, near, far):
        st = settings_for(cam, sh_degree=3)
        run, std, ind, out = check_forward_exact(st, inp)
        runs.append(run.num_rendered)
    assert runs[1] > 1.2 * runs[0]  # beyond the 12.5 % headroom of the first view's size


def test_forward_requests_the_sizes_the_abi_reports():
    """lsr_geom_bytes / lsr_image_bytes are exactly what lsr_forward requests, and the binning
    request stays within lsr_binning_bytes (include/lsr.h), so a C caller can size its buffers."""
    lib = _native.load()
    for (P, W, H) in ((3000, 160, 120), (2000, 1920, 1080)):
        st, inp = scene(P=P, W=W, H=H, seed=3, scale_range=(0.03, 0.2))
        std, ind, out = native_forward(st, inp)
        nr, color, lang, radii, geom, binning, image = out
        assert geom.numel() == lib.lsr_geom_bytes(P, W, H)
        assert image.numel() == lib.lsr_image_bytes(W, H)
        assert 0 < binning.numel() <= lib.lsr_binning_bytes(W, H, nr) * 1.125 + 256


def test_debug_backward_rejects_flags_its_forward_did_not_prepare():
    """With settings.debug the backward checks what the forward recorded (include/lsr.h): records
    claimed cleared by a forward that did not clear them, records reused by a second backward, and
    a loss gradient for a forward without the fused loss all fail instead of reading stale data."""
    st, inp = scene(P=500, W=64, H=48, seed=2, scale_range=(0.03, 0.2))
    st = st._replace(debug=True)
    std, ind = to_device(st, inp, DEV)
    args = (ind["means3D"], ind["shs"], None, ind["language_feature_precomp"], ind["opacities"], ind["scales"],
            ind["rotations"], None)

    def bwd(out, flags=0, grad_loss=None):
        nr, color, lang, radii, geom, binning, image = out
        return _native.rasterize_gaussians_backward(
            std, ind["means3D"], ind["shs"], None, ind["language_feature_precomp"], ind["scales"],
            ind["rotations"], None, radii, None, torch.ones_like(lang), nr, geom, binning, image, geometry=False,
            flags=flags, grad_loss=grad_loss)
    plain = _native.rasterize_gaussians(std, *args)
    with pytest.raises(RuntimeError, match="did not clear"):
        bwd(plain, flags=_native.BWD_RECORDS_ZEROED)
    with pytest.raises(RuntimeError, match="did not fuse"):
        bwd(plain, grad_loss=torch.ones((), device=DEV))
    zeroed = _native.rasterize_gaussians(std, *args, flags=_native.FWD_ZERO_GRAD_RECORDS)
    g1 = bwd(zeroed, flags=_native.BWD_RECORDS_ZEROED)["language_feature_precomp"].clone()
    with pytest.raises(RuntimeError, match="did not clear"):
        bwd(zeroed, flags=_native.BWD_RECORDS_ZEROED)
    g2 = bwd(zeroed)["language_feature_precomp"]
    assert_grad_close("second backward", g2.cpu().numpy(), g1.cpu().numpy())


@pytest.mark.parametrize("include_feature", [True, False])
def test_split_replay_dense_tiles(include_feature):
    """Split replay (lsr_render.hip): a dense scene whose tiles composite past list entries 256, 512
    and 768 (max contributor count ~4000), so the forward records boundary states and the backward
    replays those tiles as independent chunks started from them -- forward still bit-exact, every
    gradient within the parity tolerance of the oracle's unsplit replay."""
    st, inp = scene(P=40000, W=96, H=80, seed=21, scale_range=(0.02, 0.12), include_feature=include_feature)
    run, std, ind, out = check_forward_exact(st, inp)
    s = state(out, 40000, 96, 80)
    assert int(s["n_contrib"].max()) > 768
    check_backward(st, inp, run, out, seed=11)
