"""Small seeded scenes shared by the CPU and GPU tests (SURVEY.md §8d generators, reduced)."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from langsplat_amd.camera import make_camera
from langsplat_amd.synthetic import activated_inputs, make_cameras, make_gaussians


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


def to_device(settings, inputs, device):
    st = settings._replace(bg=settings.bg.to(device), viewmatrix=settings.viewmatrix.to(device),
                           projmatrix=settings.projmatrix.to(device), campos=settings.campos.to(device))
    return st, {k: v.to(device) for k, v in inputs.items()}


def grad_seed(H, W, seed=1, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((3, H, W), generator=g) * scale, torch.randn((3, H, W), generator=g) * scale)
