"""Small seeded scenes shared by the CPU and GPU tests (SURVEY.md §8d generators, reduced)."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from langsplat_amd.camera import make_camera
from langsplat_amd.synthetic import activated_inputs, make_cameras, make_gaussians
from oracle import oracle


def settings_for(cam, sh_degree=3, bg=(0.0, 0.0, 0.0), include_feature=True, scale_modifier=1.0,
                 device="cpu", debug=False, prefiltered=False):
    from langsplat_amd.rasterizer import GaussianRasterizationSettings
    cam = cam.to(device)
    return GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width),
        tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
        bg=torch.tensor(bg, dtype=torch.float32, device=device), scale_modifier=scale_modifier,
        viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=sh_degree,
        campos=cam.camera_center, prefiltered=prefiltered, debug=debug, include_feature=include_feature)


def scene(P=300, W=64, H=48, seed=0, view=0, n_views=1, sh_degree=3, extent=1.0, scale_range=(0.02, 0.12),
          include_feature=True, bg=(0.0, 0.0, 0.0), scale_modifier=1.0, cam=None):
    """Returns (settings (CPU tensors), inputs dict of activated CPU float32 tensors).  `cam`
    replaces the ring camera `view` of make_cameras (its size must be W x H)."""
    g = make_gaussians(P, seed=seed, sh_degree=sh_degree, extent=extent, scale_range=scale_range)
    if cam is None:
        cam = make_cameras(n_views, W, H)[view]
    assert (int(cam.image_width), int(cam.image_height)) == (W, H)
    st = settings_for(cam, sh_degree=sh_degree, bg=bg, include_feature=include_feature,
                      scale_modifier=scale_modifier)
    with torch.no_grad():
        inp = activated_inputs(g, include_feature=include_feature)
    inp = {k: v.detach().clone().contiguous() for k, v in inp.items()}
    return st, inp


def posed_camera(pos, target, roll_deg, W, H, fovy_deg=50.0):
    """A camera at `pos` looking at `target`, rolled by `roll_deg` about its viewing axis: the axes
    of look_at_origin (COLMAP-style, R's columns are the camera axes in world space), then x and y
    turned in their plane."""
    pos = np.asarray(pos, dtype=np.float64)
    z = np.asarray(target, dtype=np.float64) - pos
    z /= np.linalg.norm(z)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    a = math.radians(roll_deg)
    xr = math.cos(a) * x + math.sin(a) * y
    yr = -math.sin(a) * x + math.cos(a) * y
    R = np.stack([xr, yr, z], axis=1)
    T = -R.T @ pos
    fovy = math.radians(fovy_deg)
    fovx = 2 * math.atan(math.tan(fovy / 2) * W / H)
    return make_camera(R, T, fovx, fovy, W, H)


# (pos, target, roll in degrees) against the unit cube of make_gaussians(extent=1): `rolled` sees
# the whole cube from outside through a rotation with no zero entry; `inside*` stand in the cube
# (Gaussians behind the near plane, beside the frustum and a few tenths of a unit away, so the EWA
# window clamp fires and radii exceed the image); `grazing` looks along a face from beside it.
POSES = {
    "rolled": ((2.0, 1.5, -3.0), (0.1, -0.2, 0.0), 35.0),
    "inside": ((0.3, 0.2, -0.6), (0.0, 0.1, 0.5), -20.0),
    "inside_flip": ((0.3, 0.2, -0.6), (0.0, 0.1, 0.5), 160.0),
    "grazing": ((1.4, 0.2, -1.2), (1.5, 0.0, 1.0), 10.0),
}


def posed_scene(pose, P, W, H, seed, **kw):
    """scene() through the camera POSES[pose]."""
    pos, target, roll = POSES[pose]
    return scene(P=P, W=W, H=H, seed=seed, cam=posed_camera(pos, target, roll, W, H), **kw)


def view_space(st, means3D):
    """pv = [means, 1] @ viewmatrix in float64 (row-vector convention), (P, 3)."""
    m = np.asarray(means3D, dtype=np.float64)
    v = np.asarray(st.viewmatrix, dtype=np.float64)
    return (np.concatenate([m, np.ones((m.shape[0], 1))], 1) @ v)[:, :3]


def window_clamped(st, means3D):
    """Rows whose t.x/t.z or t.y/t.z lies outside the EWA window +-1.3 tan(fov/2) (float64)."""
    pv = view_space(st, means3D)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.abs(pv[:, 0] / pv[:, 2]) > 1.3 * st.tanfovx) | (np.abs(pv[:, 1] / pv[:, 2]) > 1.3 * st.tanfovy)


def edge_gaussians(P, seed, sh_degree=3, big=(0.8, 2.0), big_frac=0.06):
    """make_gaussians(scale_range=(0.03, 0.2)) with seeded subsets of the RAW parameters moved to the
    value edges of the blend and of the activations (the same scene serves the activated and the
    fused raw path):
      - opacity logits +100 (sigmoid exactly 1), +8, +4.6 (~0.99), -100 (exactly 0), -5.6 / -5.5 (just
        under / over 1/255);
      - `big_frac` of the rows as large Gaussians (scales in `big`) that carry +100 / +8 / +4.6 logits:
        alpha clamps only where G > 0.99, the innermost 0.14 sigma, so small Gaussians rarely saturate;
      - a random third of the f_dc entries at -2.5 (0.282 dc + 0.5 < 0: clamped colour channels next
        to unclamped ones of the same Gaussian);
      - all-zero and (1e-20, 0, 0, 0) quaternions, all-zero language vectors, log-scales of -100
        (exp flushes to 0) on all axes or on one."""
    g = make_gaussians(P, seed=seed, sh_degree=sh_degree, scale_range=(0.03, 0.2))
    r = torch.Generator().manual_seed(1000003 * (seed + 1))
    rows = torch.randperm(P, generator=r)
    at = [0]

    def take(frac, least=6):
        n = max(least, int(round(frac * P)))
        out = rows[at[0]:at[0] + n]
        at[0] += n
        return out

    big_rows = take(big_frac, 12)
    lo, hi = math.log(big[0]), math.log(big[1])
    g.scaling[big_rows] = torch.rand((big_rows.numel(), 3), generator=r) * (hi - lo) + lo
    g.opacity[big_rows, 0] = torch.tensor([100.0, 100.0, 8.0, 100.0, 4.6])[torch.arange(big_rows.numel()) % 5]
    for logit, frac in ((100.0, 0.03), (8.0, 0.02), (4.6, 0.02), (-100.0, 0.04), (-5.6, 0.04), (-5.5, 0.03)):
        g.opacity[take(frac), 0] = logit
    g.features_dc[torch.rand((P, 1, 3), generator=r) < 1.0 / 3.0] = -2.5
    # the degenerate rows below are drawn from all rows again: they overlap the opacity edges
    rows = torch.randperm(P, generator=r)
    at[0] = 0
    g.rotation[take(0.04)] = 0.0
    g.rotation[take(0.04)] = torch.tensor([1e-20, 0.0, 0.0, 0.0])
    g.language_feature[take(0.06)] = 0.0
    g.scaling[take(0.02)] = -100.0
    g.scaling[take(0.02), 1] = -100.0
    assert float(g.scaling.max()) <= 1.0
    return g


def edge_inputs(g, include_feature=True):
    """The oracle's activation (oracle.activate, the fused kernels' operation sequence: saturated
    logits give exactly 1.0 / 0.0, exp(-100) flushes to 0) of raw parameters, as scene()'s inputs."""
    op, sc, rot, lang = oracle.activate(oracle.RAW_ALL, g.opacity, g.scaling, g.rotation, g.language_feature)
    inp = dict(means3D=g.xyz.clone(), opacities=torch.from_numpy(op), scales=torch.from_numpy(sc),
               rotations=torch.from_numpy(rot), shs=torch.cat((g.features_dc, g.features_rest), dim=1).contiguous())
    inp["language_feature_precomp"] = torch.from_numpy(lang) if include_feature else torch.zeros((1,))
    return inp


def edge_scene(P=400, W=64, H=48, seed=0, sh_degree=3, include_feature=True, bg=(0.0, 0.0, 0.0), pose=None,
               **kw):
    """(raw GaussianParams, settings, activated inputs) of an edge_gaussians scene through ring
    camera 0 or POSES[pose]."""
    g = edge_gaussians(P, seed, sh_degree, **kw)
    cam = make_cameras(1, W, H)[0] if pose is None else posed_camera(*POSES[pose], W, H)
    st = settings_for(cam, sh_degree=sh_degree, bg=bg, include_feature=include_feature)
    return g, st, edge_inputs(g, include_feature)


def blend_census(st, inp, run):
    """What a scene's blends reach, from the oracle's state: every tile list walked up to n_contrib
    with o G recomputed from xy / conic_opacity (numpy's float32 exp: a blend within an ulp of a
    threshold may be counted on the other side; the counts are conditions with margin, not bits).
    A Gaussian is `visible` with radius > 0 and `blended` when some pixel blends it."""
    xy, co = run.get("xy"), run.get("conic_opacity")
    pl, rg = run.get("point_list").astype(np.int64), run.get("ranges").astype(np.int64)
    nc, P, W, H = run.get("n_contrib").astype(np.int64), run.P, run.W, run.H
    blended_g, sat_g = np.zeros(P, bool), np.zeros(P, bool)
    c = dict(blends=0, saturated=0, saturated_tiles=0, after_saturated=0, terminated=0, not_terminated=0)
    for t in range(run.gx * run.gy):
        x0, y0 = (t % run.gx) * 16, (t // run.gx) * 16
        py, px = np.mgrid[y0:min(y0 + 16, H), x0:min(x0 + 16, W)]
        px, py = px.reshape(-1), py.reshape(-1)
        ids = pl[rg[t, 0]:rg[t, 1]]
        if ids.size == 0:
            c["not_terminated"] += px.size
            continue
        dx = xy[ids, 0][:, None] - px[None].astype(np.float32)
        dy = xy[ids, 1][:, None] - py[None].astype(np.float32)
        power = -0.5 * (co[ids, 0:1] * dx * dx + co[ids, 2:3] * dy * dy) - co[ids, 1:2] * dx * dy
        oG = co[ids, 3:4] * np.exp(np.minimum(power, 0.0))
        valid = (power <= 0) & (np.minimum(np.float32(0.99), oG) >= np.float32(1.0 / 255.0))
        k = np.arange(ids.size)[:, None]
        blended = valid & (k < nc[py, px][None])
        sat = blended & (oG > np.float32(0.99))
        c["blends"] += int(blended.sum())
        c["saturated"] += int(sat.sum())
        c["saturated_tiles"] += int(sat.any())
        c["after_saturated"] += int((blended & ((np.cumsum(sat, 0) - sat) > 0)).sum())
        term = (valid & (k >= nc[py, px][None])).any(0)
        c["terminated"] += int(term.sum())
        c["not_terminated"] += int((~term).sum())
        blended_g[ids[blended.any(1)]] = True
        sat_g[ids[sat.any(1)]] = True
    vis = run.radii > 0
    clamped = run.get("clamped").astype(bool)
    o = np.asarray(inp["opacities"]).reshape(-1)
    c["saturated_gaussians"] = int(sat_g.sum())
    c["clamped_channels"] = int(clamped[blended_g].sum())
    c["mixed_clamp"] = int((blended_g & clamped.any(1) & ~clamped.all(1)).sum())
    c["o_one"] = int((blended_g & (o == 1.0)).sum())
    c["o_zero"] = int((vis & (o == 0.0)).sum())
    c["o_below_cutoff"] = int((vis & (o > 0.0) & (o < 1.0 / 255.0)).sum())
    c["zero_quat"] = int((blended_g & (np.linalg.norm(np.asarray(inp["rotations"]), axis=1) < 1e-6)).sum())
    lang = np.asarray(inp["language_feature_precomp"])
    c["zero_lang"] = int((blended_g & ~lang.any(1)).sum()) if lang.ndim == 2 else 0
    c["pixels"] = W * H
    return c


# what every value-edge test asserts of its scene before it compares anything: conditions on what the
# scene must reach, not measurements of what it happens to reach
EDGE_MINIMUMS = dict(saturated=100, saturated_gaussians=5, saturated_tiles=4, after_saturated=50, clamped_channels=100,
                     mixed_clamp=5, o_one=5, o_zero=5, o_below_cutoff=5, zero_quat=5)


def assert_reaches_edges(census, include_feature=True):
    for key, least in EDGE_MINIMUMS.items():
        assert census[key] >= least, (key, census)
    if include_feature:
        assert census["zero_lang"] >= 5, census
    assert census["not_terminated"] >= 0.1 * census["pixels"] and census["terminated"] > 0, census


# The committed edge scenes (census counts in tests/test_oracle_value_edges.py): A the plain case at
# SH degree 3; B degree 0, odd image size, a background and no language feature; C from inside the
# cube, where the EWA window clamp and radii beyond the image meet saturation (smaller `big`
# Gaussians: from that close the default ones terminate every pixel).
EDGE_SCENES = {
    "A": dict(P=400, W=96, H=64, seed=0, sh_degree=3),
    "B": dict(P=350, W=93, H=61, seed=2, sh_degree=0, bg=(0.2, 0.5, 0.9), include_feature=False),
    "C": dict(P=400, W=96, H=64, seed=4, sh_degree=3, pose="inside", bg=(0.3, 0.1, 0.7), big=(0.1, 0.3),
              big_frac=0.08),
}


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """SimpleNamespace(g, st, inp, run, census) of EDGE_SCENES[name]: computed once and shared by the
    tests of a process; nobody changes it."""
    g, st, inp = edge_scene(**EDGE_SCENES[name])
    run = oracle.forward(st, **inp)
    return SimpleNamespace(g=g, st=st, inp=inp, run=run, census=blend_census(st, inp, run),
                           include_feature=EDGE_SCENES[name].get("include_feature", True))


def to_device(settings, inputs, device):
    st = settings._replace(bg=settings.bg.to(device), viewmatrix=settings.viewmatrix.to(device),
                           projmatrix=settings.projmatrix.to(device), campos=settings.campos.to(device))
    return st, {k: v.to(device) for k, v in inputs.items()}


def grad_seed(H, W, seed=1, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((3, H, W), generator=g) * scale, torch.randn((3, H, W), generator=g) * scale)
