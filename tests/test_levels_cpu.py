"""lsr_forward_levels and langsplat_amd.levels without a GPU: the ctypes mirror, the constants, every
refusal the header lists (before any device work: dummy pointers, never dereferenced), the level
buffer's size, stack_levels' geometry check and render_levels' argument checks."""
import ctypes
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

from langsplat_amd import _native, levels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ctypes_mirror_matches_the_header(tmp_path):
    cls, cname = _native.LsrForwardLevelsArgs, "lsr_forward_levels_args"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lsr.h"', "int main(void) {",
             f'printf("sizeof %zu\\n", sizeof({cname}));']
    for f in cls._fields_:
        lines.append(f'printf("{f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines.append(f'printf("fwd_size %zu\\n", sizeof(((({cname}*)0)->fwd)));')
    lines.append("return 0; }")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict((k, int(v)) for k, v in
               (ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                    text=True).stdout.splitlines()))
    assert got["sizeof"] == ctypes.sizeof(cls)
    assert got["fwd_size"] == ctypes.sizeof(_native.LsrForwardArgs)
    for f in cls._fields_:
        assert got[f[0]] == getattr(cls, f[0]).offset, f[0]


def test_constants_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "lsr.h")).read()
    assert int(re.search(r"#define LSR_MAX_LEVELS (\d+)", hdr).group(1)) == _native.MAX_LEVELS == 4
    assert int(re.search(r"LSR_BUF_LEVELS = (\d+)", hdr).group(1)) == _native.LSR_BUF_LEVELS == 4
    assert int(re.search(r"#define LSR_ABI_VERSION (\d+)", hdr).group(1)) == 18  # additive: detected by symbol
    lib = _native.load()
    for name in ("lsr_forward_levels", "lsr_levels_bytes"):
        assert hasattr(lib, name) and name in _native.SIGNATURES


def _call(levels_=3, include_feature=1, more=True, **kw):
    lib = _native.load()
    dummy = ctypes.c_void_p(256)
    s = _native.LsrSettings()
    s.image_height, s.image_width, s.tanfovx, s.tanfovy, s.sh_degree = 8, 8, 0.5, 0.5, 0
    s.include_feature = include_feature
    s.bg = s.viewmatrix = s.projmatrix = s.campos = dummy
    la = _native.LsrForwardLevelsArgs()
    a = la.fwd
    a.P, a.M = 4, 1
    a.means3D = a.shs = a.opacities = a.scales = a.rotations = a.language_feature = dummy
    a.out_color = a.out_language_feature = a.radii = dummy
    a.flags = _native.FWD_NO_BACKWARD
    la.levels = levels_
    if more:
        la.more_language_feature = la.more_out_language_feature = dummy
    for k, v in kw.items():
        setattr(la if k in ("reserved", "more_language_feature", "more_out_language_feature") else a, k, v)
    nr = ctypes.c_int64(0)
    rc = lib.lsr_forward_levels(ctypes.byref(s), ctypes.byref(la), _native._ALLOC_CB, None, None, ctypes.byref(nr))
    return rc, _native.last_error()


@pytest.mark.parametrize("kw, field", [
    (dict(levels_=0), "levels"),
    (dict(levels_=5), "levels"),
    (dict(levels_=-1), "levels"),
    (dict(reserved=1), "reserved"),
    (dict(include_feature=0), "include_feature"),
    (dict(flags=0), "fwd.flags"),
    (dict(flags=_native.FWD_ZERO_GRAD_RECORDS), "fwd.flags"),
    (dict(flags=_native.FWD_NO_BACKWARD | _native.FWD_NO_COLOR_GRAD), "fwd.flags"),
    (dict(loss_target=ctypes.c_void_p(256)), "loss_target"),
    (dict(loss_mask=ctypes.c_void_p(256)), "loss_mask"),
    (dict(out_loss=ctypes.c_void_p(256)), "out_loss"),
    (dict(language_ready=ctypes.c_void_p(256)), "language_ready"),
    (dict(phase=_native.forward_phase.GEOMETRY), "phase"),
    (dict(phase=_native.forward_phase.COMPOSITE, capacity_rendered=16, capacity_entries=16), "phase"),
    (dict(capacity_rendered=16, capacity_entries=16), "capacity_rendered"),
    (dict(language_feature=None), "fwd.language_feature"),
    (dict(more_language_feature=None), "more_language_feature"),
    (dict(more_out_language_feature=None), "more_out_language_feature"),
    (dict(more=False), "more_"),
])
def test_refusals_name_their_field(kw, field):
    rc, msg = _call(**kw)
    assert rc == 1, (kw, rc, msg)  # LSR_ERR_INVALID, before any device work
    assert "lsr_forward_levels" in msg and field in msg, msg


def test_null_arguments_are_refused():
    lib = _native.load()
    assert lib.lsr_forward_levels(None, None, _native._ALLOC_CB, None, None, None) == 1
    assert "lsr_forward_levels" in _native.last_error()


def test_levels_bytes():
    lib = _native.load()
    for P in (1, 1000, 3001):
        assert lib.lsr_levels_bytes(P, 1) == 0
        sizes = [lib.lsr_levels_bytes(P, L) for L in (2, 3, 4)]
        assert sizes[0] < sizes[1] < sizes[2] or P == 1
        # ceil(3 (L - 1) / 4) float4 per Gaussian
        for L, n in zip((2, 3, 4), sizes):
            assert n >= 16 * ((3 * (L - 1) + 3) // 4) * P and n % 256 == 0
    assert lib.lsr_levels_bytes(2000, 3) > lib.lsr_levels_bytes(1000, 3)
    assert lib.lsr_levels_bytes(1000, 5) == 0 and lib.lsr_levels_bytes(0, 3) == 0
    assert _call(levels_=5)[0] == 1


def _cpu_model(P=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    return SimpleNamespace(
        _xyz=torch.randn((P, 3), generator=g), _features_dc=torch.randn((P, 1, 3), generator=g),
        _features_rest=torch.randn((P, 15, 3), generator=g), _opacity=torch.randn((P, 1), generator=g),
        _scaling=torch.randn((P, 3), generator=g), _rotation=torch.randn((P, 4), generator=g),
        _language_feature=torch.randn((P, 3), generator=g), active_sh_degree=3, max_sh_degree=3)


def _level_models(n=3, P=40):
    base = _cpu_model(P)
    out = []
    for l in range(n):
        m = SimpleNamespace(**{k: (v.clone() if torch.is_tensor(v) else v) for k, v in vars(base).items()})
        m._language_feature = torch.randn((P, 3), generator=torch.Generator().manual_seed(100 + l))
        out.append(m)
    return out


def test_stack_levels_accepts_identical_geometry():
    models = _level_models()
    geo, feats = levels.stack_levels(models)
    assert geo is models[0] and feats.shape == (3, 40, 3)
    for l, m in enumerate(models):
        assert torch.equal(feats[l], m._language_feature)


def test_stack_levels_names_the_first_differing_field():
    models = _level_models()
    s = models[2]._scaling
    s[7, 1] = torch.nextafter(s[7, 1], torch.tensor(float("inf")))  # one ulp
    models[2]._rotation[0, 0] += 1.0  # a later field also differs: _scaling is named
    with pytest.raises(ValueError, match=r"level model 2 .* _scaling"):
        levels.stack_levels(models)
    models = _level_models()
    models[1].active_sh_degree = 2
    with pytest.raises(ValueError, match="active_sh_degree"):
        levels.stack_levels(models)
    with pytest.raises(ValueError, match="1 to 4"):
        levels.stack_levels(_level_models(5))


def test_render_levels_checks_shape_then_device():
    m = _cpu_model()
    m.get_xyz = m._xyz
    cam = SimpleNamespace(image_height=8, image_width=8, FoVx=1.0, FoVy=1.0, world_view_transform=torch.eye(4),
                          full_proj_transform=torch.eye(4), camera_center=torch.zeros(3))
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    opt = SimpleNamespace(include_feature=True)
    for bad in (torch.zeros((40, 3)), torch.zeros((5, 40, 3)), torch.zeros((2, 39, 3)), torch.zeros((0, 40, 3))):
        with pytest.raises(ValueError, match=r"\(L, P, 3\)"):
            levels.render_levels(cam, m, pipe, torch.zeros(3), opt, bad)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        levels.render_levels(cam, m, pipe, torch.zeros(3), opt, torch.zeros((3, 40, 3)))
    import langsplat_amd
    assert langsplat_amd.render_levels is levels.render_levels and langsplat_amd.stack_levels is levels.stack_levels
    assert callable(langsplat_amd.render_levels_relevancy)
