"""distCUDA2: mean squared distance to the 3 nearest other points.

CPU: the oracle's brute force (oracle/lsr_oracle.c lso_knn_mean_dist3) vs numpy in float64, on the
well-behaved clouds and on the edge clouds below; the grid sizing (lsr_knn.hip knn_grid_size, through
lsr_debug_knn_grid on the host) over finite, degenerate and non-finite bounding boxes.
GPU: the grid search (langsplat_amd/csrc/lsr_knn.hip) bit-identical to the oracle on uniform,
clustered, flat and duplicated clouds and N = 1..5; on the edge clouds (isolated outliers, coincident,
collinear, coplanar, lattice-on-cell-faces, offset, scaled, anisotropic, non-finite); for every N up
to 70 and round the block sizes; independent of the input's dtype, layout, stream and order; at
N = 200k and 300k a sample of points is checked against a numpy brute force (rtol 2e-6: numpy does
not use the fma order).  The reference's extension (simple-knn) is absent from the container, so
parity is pinned to its published definition (exact 3-NN, self excluded by index) -- not to its
outputs.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle

FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)
INF = float("inf")


def _clouds():
    g = np.random.default_rng(0)
    yield "uniform", g.uniform(-1, 1, (3000, 3)).astype(np.float32)
    centers = g.uniform(-10, 10, (20, 3))
    yield "clustered", (centers[g.integers(0, 20, 4000)] + g.normal(0, 0.05, (4000, 3))).astype(np.float32)
    flat = g.uniform(-2, 2, (2000, 3)).astype(np.float32)
    flat[:, 2] = 0.5
    yield "flat", flat
    dup = g.uniform(0, 1, (1500, 3)).astype(np.float32)
    dup[500:700] = dup[:200]
    yield "duplicates", dup
    yield "far", (g.uniform(-1, 1, (1000, 3)) * 1000 + 5000).astype(np.float32)


# ---- edge clouds ---------------------------------------------------------------------------------
# Rows a check on the first 800 points must see (isolated points, non-finite rows) sit below 800.
ORDER_ONLY = ("offset_1e4", "offset_1e6", "scale_1e-12", "scale_1e-19")  # see test_oracle_knn_ordering_...
NONFINITE = ("nonfinite", "all_nan", "x_inf")


def _unit():
    return np.random.default_rng(11).uniform(0, 1, (2000, 3)).astype(np.float32)


def _nonfinite_cloud():
    p = np.random.default_rng(12).uniform(-1, 1, (3000, 3)).astype(np.float32)
    rows = [0, 17, 256, 511, 640, 799, 1024, 1500, 2047, 2048, 2600, 2999]
    vals = [(0, INF), (1, INF), (2, INF), (0, INF), (0, -INF), (1, -INF), (2, -INF), (0, np.nan), (1, np.nan),
            (2, np.nan)]
    for r, (c, v) in zip(rows[1:11], vals):  # one coordinate each: 4 x +inf, 3 x -inf, 3 x NaN
        p[r, c] = v
    p[rows[0]] = np.nan  # all-NaN rows at both ends
    p[rows[11]] = np.nan
    return p


@functools.lru_cache(maxsize=None)
def _edge_clouds():
    g = np.random.default_rng(5)
    c = {}
    out = g.uniform(0, 1, (2003, 3)).astype(np.float32)  # 2000 in the unit cube + 3 isolated points
    out[5], out[300], out[700] = (1e3, 0.5, 0.5), (0.5, 1e4, 0.5), (0.5, 0.5, 1e5)
    c["outliers"] = out
    c["coincident"] = np.tile(np.array([[0.3, -1.7, 2.5]], np.float32), (500, 1))
    c["pairs"] = np.array([[0.25, 0.5, 0.75], [0.25, 0.5, 0.75], [1000.25, 0.5, 0.75], [1000.25, 0.5, 0.75]],
                          np.float32)
    t = g.uniform(-1, 1, 3000)
    c["collinear_x"] = np.stack([t, np.zeros_like(t), np.zeros_like(t)], 1).astype(np.float32)
    t = g.uniform(-1, 1, 3000).astype(np.float32)
    c["collinear_diag"] = np.stack([t, t, t], 1)
    uv = g.uniform(-1, 1, (2000, 2))
    a, b = np.array([1.0, 0.5, -0.25]), np.array([-0.3, 1.0, 0.7])
    c["tilted_plane"] = (uv[:, :1] * a + uv[:, 1:] * b + np.array([0.1, 0.2, 0.3])).astype(np.float32)
    ax = np.arange(9, dtype=np.float32)
    lattice = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    # N = 1024 in [0, 8]^3: h = cbrt(512 / 512) = 1, every lattice point lies on cell faces
    c["lattice"] = np.concatenate([lattice, g.uniform(0, 8, (295, 3)).astype(np.float32)])
    u = _unit()
    c["offset_1e4"] = u + np.float32(1e4)
    c["offset_1e6"] = u + np.float32(1e6)  # slack > h: every thread scans the whole grid
    c["scale_1e-12"] = u * np.float32(1e-12)
    c["scale_1e-19"] = u * np.float32(1e-19)  # squared distances in the fp32 denormals
    c["scale_1e19"] = u * np.float32(1e19)  # squared distances near FLT_MAX, some overflow to inf
    c["anisotropic"] = (g.uniform(0, 1, (3000, 3)) * np.array([1000.0, 1.0, 0.001])).astype(np.float32)
    c["nonfinite"] = _nonfinite_cloud()
    c["all_nan"] = np.full((5, 3), np.nan, np.float32)
    xi = g.uniform(-1, 1, (300, 3)).astype(np.float32)
    xi[:, 0] = INF
    c["x_inf"] = xi
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _edge_oracle(name):
    out = oracle.knn_mean_dist3(_edge_clouds()[name])
    out.setflags(write=False)
    return out


def _numpy_knn(p, idx=None):
    p64 = p.astype(np.float64)
    idx = np.arange(len(p)) if idx is None else idx
    out = []
    for i in idx:
        d = ((p64 - p64[i]) ** 2).sum(1)
        d[i] = np.inf
        k = np.sort(d)[:3]
        k = np.where(np.isinf(k), np.float64(np.finfo(np.float32).max), k)
        out.append(k.mean())
    return np.array(out)


def test_oracle_knn_matches_numpy():
    for name, p in _clouds():
        mine = oracle.knn_mean_dist3(p[:800]).astype(np.float64)
        ref = _numpy_knn(p[:800])
        np.testing.assert_allclose(mine, ref, rtol=2e-6, atol=1e-12, err_msg=name)
    for name, p in _edge_clouds().items():
        if name in ORDER_ONLY or name in NONFINITE:
            continue
        p = p[:800]
        mine = oracle.knn_mean_dist3(p).astype(np.float64)
        with np.errstate(over="ignore"):
            ref = _numpy_knn(p)
        if name == "scale_1e19":  # the fp64 mean may exceed FLT_MAX, where fp32 gives inf
            ref = np.where(ref > FLT_MAX, np.inf, ref)
        # atol 1e-12 as above, but never more than 2e-6 of the cloud's own distances
        np.testing.assert_allclose(mine, ref, rtol=2e-6, atol=min(1e-12, 2e-6 * float(ref.min())), err_msg=name)


def test_oracle_knn_ordering_on_offset_and_tiny_clouds():
    """The offset and the 1e-12 / 1e-19 scaled clouds lose digits of their fp32 squared distances to
    cancellation or underflow, so they are compared with numpy by ordering: the fp64 brute force picks
    the 3 neighbours, and the oracle's own code on the 4-point cloud {i, its 3 neighbours} evaluates
    them in its fp32 operation order.  The oracle's result on the whole cloud can only be smaller (its
    k-th smallest fp32 distance over all points is at most that of any 3 of them, and fp32 + and / are
    monotone), and by no more than the rounding of the distances: each fp32 squared distance is within
    2 ulp (2^-23 relative, 2^-149 absolute in the denormals) of the fp64 one, hence 4 of each below."""
    clouds = _edge_clouds()
    for name in ORDER_ONLY:
        p = clouds[name][:800]
        mine = oracle.knn_mean_dist3(p)
        p64 = p.astype(np.float64)
        sel = np.empty_like(mine)
        for i in range(len(p)):
            d = ((p64 - p64[i]) ** 2).sum(1)
            d[i] = np.inf
            nn = np.argsort(d, kind="stable")[:3]
            sel[i] = oracle.knn_mean_dist3(p[np.concatenate([[i], nn])])[0]
        gap = sel.astype(np.float64) - mine.astype(np.float64)
        assert np.all(np.isfinite(mine)) and np.all(gap >= 0), name
        assert np.all(gap <= 4 * (2.0 ** -23 * sel + 2.0 ** -149)), (name, gap.max())


def test_oracle_knn_nonfinite_points():
    """A point with a non-finite coordinate is nobody's neighbour and its own result is inf; the
    finite points get what the cloud of the finite points alone gives."""
    for name in NONFINITE:
        p = _edge_clouds()[name][:800]
        mine = oracle.knn_mean_dist3(p)
        fin = np.isfinite(p).all(1)
        assert np.all(np.isposinf(mine[~fin])), name
        if fin.any():
            np.testing.assert_allclose(mine[fin].astype(np.float64), _numpy_knn(p[fin]), rtol=2e-6, atol=1e-12,
                                       err_msg=name)
    fin = np.isfinite(_edge_clouds()["nonfinite"][:800]).all(1)
    assert 0 < (~fin).sum() < 800 and not fin[0]


def test_oracle_knn_small_n():
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3]], np.float32)
    out = oracle.knn_mean_dist3(p)
    np.testing.assert_allclose(out, [(1 + 4 + 9) / 3, (1 + 5 + 10) / 3, (4 + 5 + 13) / 3, (9 + 10 + 13) / 3])
    # missing neighbours count as FLT_MAX: N = 1 overflows to inf, N = 3 gives (d0 + d1 + FLT_MAX) / 3
    assert np.isinf(oracle.knn_mean_dist3(p[:1])[0])
    fm = np.float32(np.finfo(np.float32).max)
    np.testing.assert_allclose(oracle.knn_mean_dist3(p[:3]), np.float32(fm / 3), rtol=1e-6)


# ---- grid sizing on the host ---------------------------------------------------------------------
def _cube(lo, hi):
    return (lo, lo, lo, hi, hi, hi)


GRID_BOXES = {
    "unit": _cube(0.0, 1.0),
    "coincident": _cube(0.7, 0.7),
    "one_zero_extent": (0.0, 0.0, 0.5, 1.0, 1.0, 0.5),
    "two_zero_extents": (0.0, -2.0, 0.5, 1.0, -2.0, 0.5),
    "inf_one": (-1.0, -1.0, -1.0, INF, 1.0, 1.0),
    "neg_inf_one": (-1.0, -INF, -1.0, 1.0, 1.0, 1.0),
    "inf_three": (-1.0, -1.0, -1.0, INF, INF, INF),
    "inf_six": (-INF, -INF, -INF, INF, INF, INF),
    "inf_six_same_sign": _cube(INF, INF),
    "nan_one": (0.0, 0.0, 0.0, 1.0, float("nan"), 1.0),
    "untouched": (FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX),
    "untouched_x": (FLT_MAX, 0.0, 0.0, -FLT_MAX, 1.0, 1.0),
    "extent_1e-38": _cube(0.0, 1e-38),
    "extent_1e-19": _cube(0.0, 1e-19),
    "extent_1e19": _cube(0.0, 1e19),
    "extent_6e38": _cube(-3e38, 3e38),
    "outlier": (0.0, 0.0, 0.0, 1e5, 1.0, 1.0),
}
GRID_NS = (1, 2, 3, 4, 5, 3000, 262145, 0x3FFFFFFF)


def _parent_grid(box, N):
    """The sizing formula before it was bounded, in float64, for a finite box with min <= max:
    (h, (nx, ny, nz))."""
    b = [np.float64(np.float32(v)) for v in box]
    ex, ey, ez = b[3] - b[0], b[4] - b[1], b[5] - b[2]
    ext = max(ex, ey, ez)
    if not ext > 0:
        ext = 1.0
    fx, fy, fz = max(ex, 0.01 * ext), max(ey, 0.01 * ext), max(ez, 0.01 * ext)
    h = float(np.cbrt(fx * fy * fz / max(0.5 * N, 1.0)))
    while True:
        n = tuple(int(min(e / h + 1.0, 1048576.0)) for e in (ex, ey, ez))
        if n[0] * n[1] * n[2] <= 2 * N + 64:
            return h, n
        h *= 1.26


@pytest.mark.parametrize("name", list(GRID_BOXES))
def test_knn_grid_sizing_is_total(name):
    """knn_grid_size returns for every box, with h and 1 / h positive finite floats, dimensions >= 1 and
    at most 2 N + 64 cells.  For a finite box with min <= max the dimensions are those of the formula
    before it was bounded -- unless that formula's h or 1 / h is no normal float (extent 1e-38: 1 / h
    overflows; extent 6e38 at small N: h overflows), where the grid is the one-cell fallback."""
    from langsplat_amd import _native
    box = GRID_BOXES[name]
    b32 = np.array(box, np.float32)
    for N in GRID_NS:
        g = _native.debug_knn_grid(box, N)
        nx, ny, nz = g["dims"]
        assert 0 < g["h"] < INF and 0 < g["inv_h"] < INF, (N, g)
        assert min(nx, ny, nz) >= 1 and nx * ny * nz <= 2 * N + 64, (N, g)
        assert all(np.isfinite(o) for o in g["origin"]), (N, g)
        if not np.isfinite(b32).all():
            assert (nx, ny, nz) == (1, 1, 1), (N, g)
        elif np.all(b32[:3] <= b32[3:]):
            h, dims = _parent_grid(box, N)
            with np.errstate(over="ignore", under="ignore"):
                usable = FLT_MIN <= float(np.float32(h)) <= FLT_MAX and FLT_MIN <= float(np.float32(1.0 / h)) <= FLT_MAX
            assert (nx, ny, nz) == (dims if usable else (1, 1, 1)), (N, g, dims)
            assert g["origin"] == tuple(float(v) for v in b32[:3])
            if usable:
                assert g["h"] == float(np.float32(h)) or abs(g["h"] - h) <= 1e-6 * h, (N, g, h)
        else:  # an axis no finite coordinate was seen on: origin 0, zero extent
            for k in range(3):
                if b32[k] > b32[k + 3]:
                    assert g["origin"][k] == 0.0 and g["dims"][k] == 1, (N, g)


def test_knn_grid_sizing_cases_reach_both_outcomes():
    """The sweep above is not vacuous: it holds boxes that keep the formula's grid and boxes that fall
    back, and the fallbacks the comment names are fallbacks."""
    from langsplat_amd import _native
    assert _native.debug_knn_grid(GRID_BOXES["unit"], 3000)["dims"] == (12, 12, 12)
    assert _native.debug_knn_grid(GRID_BOXES["outlier"], 3000)["dims"][1:] == (1, 1)
    assert _native.debug_knn_grid(GRID_BOXES["outlier"], 3000)["dims"][0] > 100
    assert _native.debug_knn_grid(GRID_BOXES["extent_1e-38"], 3000)["dims"] == (1, 1, 1)
    assert _native.debug_knn_grid(GRID_BOXES["extent_6e38"], 5)["dims"] == (1, 1, 1)
    assert _native.debug_knn_grid(GRID_BOXES["extent_6e38"], 3000)["dims"] == (12, 12, 12)
    g = _native.debug_knn_grid(_cube(0.0, 8.0), 1024)  # the lattice cloud: cells of exactly 1
    assert g["h"] == 1.0 and g["dims"] == (9, 9, 9)
    lib = _native.load()
    assert lib.lsr_debug_knn_grid(None, 5, None, None) != 0 and "invalid" in _native.last_error()


# ---- GPU -----------------------------------------------------------------------------------------
def _gpu(p):
    from langsplat_amd.knn import dist_cuda2
    return dist_cuda2(torch.from_numpy(np.array(p)).cuda()).cpu().numpy()  # a copy: the shared clouds are read-only


@pytest.mark.gpu
def test_gpu_knn_bit_exact_vs_oracle():
    from langsplat_amd.knn import dist_cuda2
    for name, p in _clouds():
        got = dist_cuda2(torch.from_numpy(p).cuda()).cpu().numpy()
        np.testing.assert_array_equal(got, oracle.knn_mean_dist3(p), err_msg=name)
    for n in range(1, 6):
        p = np.random.default_rng(n).normal(size=(n, 3)).astype(np.float32)
        np.testing.assert_array_equal(dist_cuda2(torch.from_numpy(p).cuda()).cpu().numpy(),
                                      oracle.knn_mean_dist3(p), err_msg=f"N={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in _edge_clouds() if n not in NONFINITE])
def test_gpu_knn_edge_clouds_bit_exact_vs_oracle(name):
    """Clouds that leave the shell the search starts in: isolated points that walk many shells, clouds
    collapsed into a line, a plane or a point, points on cell faces with six-way ties, offsets up to
    where slack > h, and scales from the fp32 denormals to the overflow of the squared distance."""
    ref = _edge_oracle(name)
    np.testing.assert_array_equal(_gpu(_edge_clouds()[name]), ref)
    if name == "coincident":
        assert not ref.any()
    if name == "scale_1e19":
        assert np.isfinite(ref).all()  # overflowed pairs were not inserted
    if name == "scale_1e-19":
        assert 0 < ref.max() < FLT_MIN  # the results are denormal: neither side flushes them


@pytest.mark.gpu
@pytest.mark.parametrize("name", NONFINITE)
def test_gpu_knn_nonfinite_points(name):
    """inf and NaN coordinates: the call returns, rows with one are inf, every finite row is
    bit-identical to the oracle (test_oracle_knn_nonfinite_points pins the oracle)."""
    p = _edge_clouds()[name]
    got = _gpu(p)
    fin = np.isfinite(p).all(1)
    assert np.all(np.isposinf(got[~fin]))
    np.testing.assert_array_equal(got, _edge_oracle(name))


@pytest.mark.gpu
def test_gpu_knn_every_small_n():
    """Grids of a handful of cells and the block and wave boundaries of every kernel."""
    for n in list(range(1, 71)) + [255, 256, 257, 1023, 1024, 1025]:
        p = np.random.default_rng(1000 + n).normal(size=(n, 3)).astype(np.float32)
        np.testing.assert_array_equal(_gpu(p), oracle.knn_mean_dist3(p), err_msg=f"N={n}")


@pytest.mark.gpu
def test_gpu_knn_input_dtype_layout_stream():
    """dist_cuda2 gives exactly the tensor of the contiguous float32 call on the same values for
    float64 / float16 input, a transposed view, a strided slice, a requires_grad input and under a
    non-default current stream."""
    from langsplat_amd.knn import dist_cuda2
    g = torch.Generator().manual_seed(3)
    x64 = torch.randn((1500, 3), generator=g, dtype=torch.float64).cuda()
    x32 = x64.float().contiguous()
    ref = dist_cuda2(x32)
    assert ref.dtype == torch.float32 and ref.shape == (1500,)
    assert torch.equal(dist_cuda2(x64), ref)
    x16 = x64.half()
    assert torch.equal(dist_cuda2(x16), dist_cuda2(x16.float()))
    xt = x32.t().contiguous().t()  # (3, N).T: same values, strides (1, N)
    assert not xt.is_contiguous() and torch.equal(xt, x32)
    assert torch.equal(dist_cuda2(xt), ref)
    wide = torch.zeros((3000, 3), device="cuda")
    wide[::2] = x32
    wide[1::2] = 7.0
    assert torch.equal(dist_cuda2(wide[::2]), ref)
    xg = x32.clone().requires_grad_(True)
    out = dist_cuda2(xg)
    assert torch.equal(out, ref) and not out.requires_grad
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        on_s = dist_cuda2(x32)
    s.synchronize()
    assert torch.equal(on_s, ref)


@pytest.mark.gpu
def test_gpu_knn_repeatable_and_permutation_equivariant():
    """The order of the points inside a cell is set by atomics and the order of the cells by the
    input's; neither may show: two calls agree bit for bit, and a permuted input permutes the output."""
    g = np.random.default_rng(21)
    p = np.concatenate([g.normal(0, 1, (3000, 3)), g.uniform(-0.01, 0.01, (1000, 3))]).astype(np.float32)
    a, b = _gpu(p), _gpu(p)
    np.testing.assert_array_equal(a, b)
    perm = g.permutation(len(p))
    np.testing.assert_array_equal(_gpu(p[perm]), a[perm])


@pytest.mark.gpu
def test_gpu_knn_large_and_simple_knn_import_path():
    from simple_knn._C import distCUDA2  # the reference's import (scene/gaussian_model.py:20)
    g = np.random.default_rng(7)
    p = np.concatenate([g.normal(0, 1, (150000, 3)), g.uniform(-5, 5, (50000, 3))]).astype(np.float32)
    got = distCUDA2(torch.from_numpy(p).cuda()).cpu().numpy()
    idx = g.choice(len(p), 300, replace=False)
    np.testing.assert_allclose(got[idx].astype(np.float64), _numpy_knn(p, idx), rtol=2e-6)
    assert got.shape == (len(p),) and np.all(got > 0)


@pytest.mark.gpu
def test_gpu_knn_bounding_box_beyond_one_pass():
    """N = 300000: 1172 blocks of points for a bounding box of 1024 blocks, so its grid-stride loop
    takes a second pass over the points from index 262144 on -- where the six extreme coordinates are."""
    g = np.random.default_rng(9)
    N = 300000
    p = g.uniform(-5, 5, (N, 3)).astype(np.float32)
    ext = np.arange(262144 + 100, 262144 + 106)
    for k, i in enumerate(ext):
        p[i, k % 3] = -7.0 if k < 3 else 7.0
    assert p.min(0).tolist() == [-7.0] * 3 and p.max(0).tolist() == [7.0] * 3
    assert np.all(p[:262144].min(0) > -5.0) and np.all(p[:262144].max(0) < 5.0)
    got = _gpu(p)
    idx = np.concatenate([ext, g.choice(262144, 294, replace=False)])
    np.testing.assert_allclose(got[idx].astype(np.float64), _numpy_knn(p, idx), rtol=2e-6)
    assert got.shape == (N,) and np.all(got > 0) and np.all(np.isfinite(got))


@pytest.mark.gpu
def test_gpu_knn_scan_stall_fallback_is_exact():
    """The cell-count scan forced onto its stall path (spin limit 0) gives the same distances."""
    from langsplat_amd import _native
    from langsplat_amd.knn import dist_cuda2
    lib = _native.load()
    p = np.random.default_rng(3).uniform(-1, 1, (20000, 3)).astype(np.float32)
    ref = dist_cuda2(torch.from_numpy(p).cuda()).cpu().numpy()
    lib.lsr_debug_scan_stalls()
    old = lib.lsr_debug_set_spin_limit(0)
    try:
        got = dist_cuda2(torch.from_numpy(p).cuda()).cpu().numpy()
        assert lib.lsr_debug_scan_stalls() == 1
    finally:
        lib.lsr_debug_set_spin_limit(old)
    np.testing.assert_array_equal(got, ref)
