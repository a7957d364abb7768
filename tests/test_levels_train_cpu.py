"""lsr_backward_levels and the training side of langsplat_amd.levels without a GPU: the symbols, the
ctypes mirror (a compiled sizeof / offsetof probe), the scratch size, every refusal the header lists
(before any device work: dummy pointers, never dereferenced), render_levels_train's argument checks
and split_levels."""
import ctypes
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

from langsplat_amd import _native, levels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = 256  # a non-NULL device "pointer" no refusal path reads


def test_header_declares_and_library_exports_the_symbols():
    hdr = open(os.path.join(ROOT, "include", "lsr.h")).read()
    lib = _native.load()
    for name in ("lsr_backward_levels", "lsr_backward_levels_bytes"):
        assert re.search(r"\b%s\(" % name, hdr), name
        assert hasattr(lib, name) and name in _native.SIGNATURES
    assert "typedef struct lsr_backward_levels_args" in hdr
    assert int(re.search(r"#define LSR_ABI_VERSION (\d+)", hdr).group(1)) == 18 == _native.ABI_VERSION
    # the header keeps the rule that the training backward may not follow the levels forward
    assert "lsr_backward still must NOT" in hdr


def test_ctypes_mirror_matches_the_header(tmp_path):
    cls, cname = _native.LsrBackwardLevelsArgs, "lsr_backward_levels_args"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lsr.h"', "int main(void) {",
             f'printf("sizeof %zu\\n", sizeof({cname}));']
    for f in cls._fields_:
        lines.append(f'printf("{f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines.append("return 0; }")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict((k, int(v)) for k, v in
               (ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                    text=True).stdout.splitlines()))
    assert got["sizeof"] == ctypes.sizeof(cls)
    for f in cls._fields_:
        assert got[f[0]] == getattr(cls, f[0]).offset, f[0]
    # every field of the header's struct is mirrored, in order
    body = re.search(r"typedef struct lsr_backward_levels_args \{(.*?)\} lsr_backward_levels_args;",
                     open(os.path.join(ROOT, "include", "lsr.h")).read(), re.S).group(1)
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in cls._fields_]


def test_backward_levels_bytes():
    lib = _native.load()
    for P in (0, -1):
        for L in (1, 3):
            assert lib.lsr_backward_levels_bytes(P, L) == 0
    for L in (0, -1, 5):
        assert lib.lsr_backward_levels_bytes(1000, L) == 0
    for P in (1, 1000, 3001):
        sizes = [lib.lsr_backward_levels_bytes(P, L) for L in (1, 2, 3, 4)]
        for L, n in zip((1, 2, 3, 4), sizes):
            assert n >= 4 * 3 * L * P and n % 256 == 0  # one row of 3 L floats per Gaussian
        assert sizes == sorted(sizes) and (P == 1 or len(set(sizes)) == 4)
    for L in (1, 2, 3, 4):
        a, b, c = (lib.lsr_backward_levels_bytes(P, L) for P in (1000, 2000, 40000))
        assert a < b < c


def _call(settings=True, args=True, include_feature=1, **kw):
    lib = _native.load()
    s = _native.LsrSettings()
    s.image_height, s.image_width, s.tanfovx, s.tanfovy, s.sh_degree = 8, 8, 0.5, 0.5, 0
    s.include_feature = include_feature
    s.bg = s.viewmatrix = s.projmatrix = s.campos = DUMMY
    a = _native.LsrBackwardLevelsArgs()
    a.P, a.levels, a.num_rendered = 4, 3, 10
    for name in ("geom_buffer", "binning_buffer", "image_buffer", "radii", "language_feature",
                 "dL_dout_language_feature", "scratch", "dL_dlanguage_feature"):
        setattr(a, name, DUMMY)
    for k, v in kw.items():
        setattr(a, k, v)
    rc = lib.lsr_backward_levels(ctypes.byref(s) if settings else None, ctypes.byref(a) if args else None, None)
    return rc, _native.last_error()


FUSED = ("out_language_feature", "loss_target", "loss_mask", "dL_dloss")


@pytest.mark.parametrize("kw, field", [
    (dict(settings=False), "settings"),
    (dict(args=False), "args"),
    (dict(levels=0), "levels"),
    (dict(levels=5), "levels"),
    (dict(levels=-1), "levels"),
    (dict(reserved=1), "reserved"),
    (dict(P=-1), "P "),
    (dict(num_rendered=-1), "num_rendered"),
    (dict(include_feature=0), "include_feature"),
    (dict(geom_buffer=None), "geom_buffer"),
    (dict(binning_buffer=None), "binning_buffer"),
    (dict(image_buffer=None), "image_buffer"),
    (dict(radii=None), "radii"),
    (dict(scratch=None), "scratch"),
    (dict(dL_dlanguage_feature=None), "dL_dlanguage_feature"),
    (dict(raw=_native.RAW_LANGUAGE, language_feature=None), "language_feature"),
    (dict(dL_dout_language_feature=None), "dL_dout_language_feature"),  # neither seed
    (dict(P=0, dL_dout_language_feature=None), "seed"),                 # refused with P == 0 too
] + [(dict({n: DUMMY for n in FUSED if n != miss}), miss) for miss in FUSED]      # three of the four
  + [(dict({n: DUMMY}, dL_dout_language_feature=None), "all four") for n in FUSED])  # one of the four
def test_refusals_name_their_field(kw, field):
    rc, msg = _call(**kw)
    assert rc == 1, (kw, rc, msg)  # LSR_ERR_INVALID, before any device work
    assert "lsr_backward_levels" in msg and field in msg, msg


def test_nothing_to_do_returns_ok_without_device_work():
    """P == 0 with a seed: LSR_OK, and no pointer is read (every buffer NULL)."""
    rc, msg = _call(P=0, geom_buffer=None, binning_buffer=None, image_buffer=None, radii=None, scratch=None,
                    dL_dlanguage_feature=None, language_feature=None, raw=_native.RAW_LANGUAGE)
    assert rc == 0, msg
    # a raw feature is not needed unless raw says so
    rc, msg = _call(P=0, language_feature=None, **{n: DUMMY for n in FUSED})
    assert rc == 0, msg


def _cpu_model(P=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    m = SimpleNamespace(
        _xyz=torch.randn((P, 3), generator=g), _features_dc=torch.randn((P, 1, 3), generator=g),
        _features_rest=torch.randn((P, 15, 3), generator=g), _opacity=torch.randn((P, 1), generator=g),
        _scaling=torch.randn((P, 3), generator=g), _rotation=torch.randn((P, 4), generator=g),
        _language_feature=torch.randn((P, 3), generator=g), active_sh_degree=3, max_sh_degree=3)
    m.get_xyz = m._xyz
    return m


def test_render_levels_train_checks_shape_then_device_then_frozen_geometry():
    """On this side only CPU tensors exist, so the device refusal is the last one reachable: a wrong
    shape wins over it, and it wins over a geometry parameter that requires grad (the frozen-geometry
    refusal itself is exercised on the GPU, tests/test_gpu_levels_train.py)."""
    m = _cpu_model()
    m._scaling.requires_grad_(True)
    cam = SimpleNamespace(image_height=8, image_width=8, FoVx=1.0, FoVy=1.0, world_view_transform=torch.eye(4),
                          full_proj_transform=torch.eye(4), camera_center=torch.zeros(3))
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    opt = SimpleNamespace(include_feature=True)
    for bad in (torch.zeros((40, 3)), torch.zeros((5, 40, 3)), torch.zeros((2, 39, 3)), torch.zeros((0, 40, 3))):
        with pytest.raises(ValueError, match=r"\(L, P, 3\)"):
            levels.render_levels_train(cam, m, pipe, torch.zeros(3), opt, bad)
    assert torch.is_grad_enabled()
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        levels.render_levels_train(cam, m, pipe, torch.zeros(3), opt, torch.zeros((3, 40, 3), requires_grad=True))
    import langsplat_amd
    assert langsplat_amd.render_levels_train is levels.render_levels_train
    assert langsplat_amd.LevelsStep is levels.LevelsStep and langsplat_amd.split_levels is levels.split_levels


def test_levels_step_checks_its_arguments():
    from langsplat_amd.optim import Adam
    m = _cpu_model()
    feats = torch.nn.Parameter(torch.zeros((3, 40, 3)))
    opt = Adam([{"params": [feats], "lr": 0.0025}], lr=0.0, eps=1e-15)
    assert levels.LevelsStep(m, feats, opt).language_features is feats
    with pytest.raises(ValueError, match="Parameter"):
        levels.LevelsStep(m, torch.zeros((3, 40, 3)), opt)
    with pytest.raises(ValueError, match=r"\(L, P, 3\)"):
        levels.LevelsStep(m, torch.nn.Parameter(torch.zeros((3, 39, 3))), opt)
    with pytest.raises(ValueError, match="langsplat_amd.optim.Adam"):
        levels.LevelsStep(m, feats, torch.optim.Adam([feats]))
    with pytest.raises(ValueError, match="one parameter"):
        levels.LevelsStep(m, feats, Adam([feats, torch.nn.Parameter(torch.zeros(3))]))


def test_split_levels_inverts_stacking():
    models = []
    for l in range(3):
        m = _cpu_model()
        m._language_feature = torch.randn((40, 3), generator=torch.Generator().manual_seed(100 + l))
        models.append(m)
    _, feats = levels.stack_levels(models)
    parts = levels.split_levels(torch.nn.Parameter(feats))
    assert len(parts) == 3
    for p, m in zip(parts, models):
        assert torch.equal(p, m._language_feature) and p.is_contiguous() and not p.requires_grad
        assert p.data_ptr() != feats.data_ptr()
    assert torch.equal(torch.stack(parts), feats)
    with pytest.raises(ValueError, match=r"\(L, P, 3\)"):
        levels.split_levels(torch.zeros((40, 3)))
