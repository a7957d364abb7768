"""lsr_levels_step_forward / lsr_levels_step_backward and langsplat_amd.levels_graph without a GPU: the
symbols, the ctypes mirrors (a compiled sizeof / offsetof probe), the unchanged ABI version, every
refusal the header lists (before any device work: dummy pointers, never dereferenced) and the argument
checks of LevelsViewSlot and GraphedLevelsStep."""
import ctypes
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

from langsplat_amd import _native, levels_graph
from langsplat_amd.optim import Adam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = 256  # a non-NULL device "pointer" no refusal path reads
HEADER = open(os.path.join(ROOT, "include", "lsr.h")).read()


def test_abi_version_is_unchanged_and_the_symbols_exist():
    assert int(re.search(r"#define LSR_ABI_VERSION (\d+)", HEADER).group(1)) == 18 == _native.ABI_VERSION
    lib = _native.load()
    assert lib.lsr_abi_version() == 18
    for name in ("lsr_levels_step_forward", "lsr_levels_step_backward"):
        assert re.search(r"\b%s\(" % name, HEADER), name
        assert hasattr(lib, name) and name in _native.SIGNATURES


@pytest.mark.parametrize("cls, cname", [(_native.LsrLevelsStepForwardArgs, "lsr_levels_step_forward_args"),
                                        (_native.LsrLevelsStepBackwardArgs, "lsr_levels_step_backward_args")])
def test_ctypes_mirrors_match_the_header(tmp_path, cls, cname):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lsr.h"', "int main(void) {",
             f'printf("sizeof %zu\\n", sizeof({cname}));',
             'printf("levels_args %zu\\n", sizeof(lsr_forward_levels_args));',
             'printf("backward_levels_args %zu\\n", sizeof(lsr_backward_levels_args));']
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
    # the existing structs keep their sizes
    assert got["levels_args"] == ctypes.sizeof(_native.LsrForwardLevelsArgs)
    assert got["backward_levels_args"] == ctypes.sizeof(_native.LsrBackwardLevelsArgs)
    # every field of the header's struct is mirrored, in order
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), HEADER, re.S).group(1)
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in cls._fields_]


def _settings(include_feature=1):
    s = _native.LsrSettings()
    s.image_height, s.image_width, s.tanfovx, s.tanfovy, s.sh_degree = 8, 8, 0.5, 0.5, 0
    s.include_feature = include_feature
    s.bg = s.viewmatrix = s.projmatrix = s.campos = DUMMY
    return s


def _forward(levels_=3, include_feature=1, more=True, outer_reserved=0, **kw):
    lib = _native.load()
    s = _settings(include_feature)
    sa = _native.LsrLevelsStepForwardArgs()
    sa.reserved = outer_reserved
    la = sa.levels
    a = la.fwd
    a.P, a.M = 4, 1
    a.means3D = a.shs = a.opacities = a.scales = a.rotations = a.language_feature = DUMMY
    a.out_color = a.out_language_feature = a.radii = DUMMY
    a.flags = _native.FWD_NO_BACKWARD
    a.capacity_rendered = a.capacity_entries = 64
    a.overflow = DUMMY
    la.levels = levels_
    if more:
        la.more_language_feature = la.more_out_language_feature = DUMMY
    for k, v in kw.items():
        setattr(la if k in ("reserved", "more_language_feature", "more_out_language_feature") else a, k, v)
    nr = ctypes.c_int64(0)
    rc = lib.lsr_levels_step_forward(ctypes.byref(s), ctypes.byref(sa), _native._ALLOC_CB, None, None, ctypes.byref(nr))
    return rc, _native.last_error()


@pytest.mark.parametrize("kw, field", [
    (dict(levels_=0), "levels"),
    (dict(levels_=5), "levels"),
    (dict(reserved=1), "reserved"),
    (dict(outer_reserved=1), "reserved"),
    (dict(include_feature=0), "include_feature"),
    (dict(flags=0), "fwd.flags"),
    (dict(flags=_native.FWD_NO_BACKWARD | _native.FWD_ZERO_GRAD_RECORDS), "fwd.flags"),
    (dict(loss_target=DUMMY), "loss_target"),
    (dict(loss_mask=DUMMY), "loss_mask"),
    (dict(out_loss=DUMMY), "out_loss"),
    (dict(language_ready=DUMMY), "language_ready"),
    (dict(capacity_rendered=0), "capacity_rendered"),
    (dict(capacity_rendered=-1), "capacity_rendered"),
    (dict(capacity_entries=0), "capacity_entries"),
    (dict(overflow=None), "fwd.overflow"),
    (dict(phase=_native.forward_phase.GEOMETRY), "lsr_forward with that phase"),
    (dict(phase=4), "fwd.phase"),
    (dict(phase=-1), "fwd.phase"),
    (dict(language_feature=None), "fwd.language_feature"),
    (dict(more_language_feature=None), "more_language_feature"),
    (dict(more_out_language_feature=None), "more_out_language_feature"),
])
def test_forward_refusals_name_their_field(kw, field):
    rc, msg = _forward(**kw)
    assert rc == 1, (kw, rc, msg)  # LSR_ERR_INVALID, before any device work
    assert "lsr_levels_step_forward" in msg and field in msg, msg


def test_forward_null_arguments_are_refused():
    lib = _native.load()
    assert lib.lsr_levels_step_forward(None, None, _native._ALLOC_CB, None, None, None) == 1
    assert "lsr_levels_step_forward" in _native.last_error()


def _backward(settings=True, args=True, include_feature=1, update=None, **kw):
    """update: None, or a dict of lsr_adam_tensor overrides ("param", "n", ...) for a fused update."""
    lib = _native.load()
    s = _settings(include_feature)
    a = _native.LsrLevelsStepBackwardArgs()
    a.P, a.levels, a.num_rendered = 4, 3, 64
    for name in ("geom_buffer", "binning_buffer", "image_buffer", "radii", "language_feature",
                 "dL_dout_language_feature", "scratch", "dL_dlanguage_feature"):
        setattr(a, name, DUMMY)
    keep = None
    if update is not None:
        u = dict(n=3 * 3 * 4, param=DUMMY, exp_avg=DUMMY, exp_avg_sq=DUMMY)
        u.update(update)
        keep = _native.LsrAdamTensor(u["n"], u["param"], None, u["exp_avg"], u["exp_avg_sq"], 0.0, 0.9, 0.999, 1e-15, 0)
        a.update = ctypes.pointer(keep)
        a.raw = _native.RAW_LANGUAGE
        a.update_step_dev = DUMMY
    for k, v in kw.items():
        setattr(a, k, v)
    rc = lib.lsr_levels_step_backward(ctypes.byref(s) if settings else None, ctypes.byref(a) if args else None, None)
    return rc, _native.last_error()


FUSED = ("out_language_feature", "loss_target", "loss_mask", "dL_dloss")


@pytest.mark.parametrize("kw, field", [
    # lsr_backward_levels' list
    (dict(settings=False), "settings"),
    (dict(args=False), "args"),
    (dict(levels=0), "levels"),
    (dict(levels=5), "levels"),
    (dict(reserved=1), "reserved"),
    (dict(reserved2=1), "reserved"),
    (dict(P=-1), "P "),
    (dict(num_rendered=-1), "num_rendered"),
    (dict(num_rendered=0), "num_rendered"),  # the capacity, never 0 with P > 0
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
    # the additions
    (dict(update={}, raw=0), "LSR_RAW_LANGUAGE"),
    (dict(update=dict(param=512)), "update->param"),
    (dict(update=dict(n=3 * 4)), "update->n"),
    (dict(update=dict(n=3 * 3 * 4 + 1)), "update->n"),
    (dict(update=dict(exp_avg=None)), "exp_avg"),
    (dict(update=dict(exp_avg_sq=None)), "exp_avg_sq"),
    (dict(update={}, update_step_dev=None), "update_step_dev"),
    (dict(update={}, fill_record=DUMMY), "fill_levels"),           # levels > 1, fill_record set, no fill_levels
    (dict(update={}, fill_levels=DUMMY), "fill_record"),
    (dict(fill_record=DUMMY), "need update"),
    (dict(fill_levels=DUMMY), "need update"),
    (dict(update_step_dev=DUMMY), "need update"),
    (dict(update_skip=DUMMY), "need update"),
] + [(dict({n: DUMMY for n in FUSED if n != miss}), miss) for miss in FUSED]
  + [(dict({n: DUMMY}, dL_dout_language_feature=None), "all four") for n in FUSED])
def test_backward_refusals_name_their_field(kw, field):
    rc, msg = _backward(**kw)
    assert rc == 1, (kw, rc, msg)  # LSR_ERR_INVALID, before any device work
    assert "lsr_levels_step_backward" in msg and field in msg, msg


def test_backward_with_update_accepts_a_null_gradient_and_p_zero_is_a_no_op():
    """P == 0: LSR_OK without device work (every buffer NULL), with and without a fused update."""
    rc, msg = _backward(P=0, geom_buffer=None, binning_buffer=None, image_buffer=None, radii=None, scratch=None,
                        dL_dlanguage_feature=None, num_rendered=0)
    assert rc == 0, msg
    rc, msg = _backward(update=dict(n=0), P=0, geom_buffer=None, binning_buffer=None, image_buffer=None, radii=None,
                        scratch=None, dL_dlanguage_feature=None, num_rendered=0)
    assert rc == 0, msg
    # with update a NULL dL_dlanguage_feature is no refusal: the next check (a wrong n) is what answers
    rc, msg = _backward(update=dict(n=1), dL_dlanguage_feature=None)
    assert rc == 1 and "update->n" in msg


# ---- Python ----------------------------------------------------------------------------------------

def _cam(W=8, H=8):
    return SimpleNamespace(image_height=H, image_width=W, FoVx=1.0, FoVy=1.0, world_view_transform=torch.eye(4),
                           full_proj_transform=torch.eye(4), camera_center=torch.zeros(3))


def test_levels_view_slot_refuses_wrong_shapes_then_cpu_tensors():
    ok_m = torch.ones((2, 8, 8), dtype=torch.bool)
    for bad in (torch.zeros((3, 8, 8)), torch.zeros((2, 3, 8, 9)), torch.zeros((5, 3, 8, 8)), torch.zeros((0, 3, 8, 8)),
                torch.zeros((2, 4, 8, 8))):
        with pytest.raises(ValueError, match="gts must be"):
            levels_graph.LevelsViewSlot(_cam(), bad, ok_m)
    with pytest.raises(ValueError, match="masks must be"):
        levels_graph.LevelsViewSlot(_cam(), torch.zeros((2, 3, 8, 8)), torch.ones((3, 8, 8), dtype=torch.bool))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        levels_graph.LevelsViewSlot(_cam(), torch.zeros((2, 3, 8, 8)), ok_m)


def test_graphed_levels_step_checks_its_arguments_then_the_device():
    P, L = 40, 2
    g = torch.Generator().manual_seed(0)
    m = SimpleNamespace(
        _xyz=torch.randn((P, 3), generator=g), _features_dc=torch.randn((P, 1, 3), generator=g),
        _features_rest=torch.randn((P, 15, 3), generator=g), _opacity=torch.randn((P, 1), generator=g),
        _scaling=torch.randn((P, 3), generator=g), _rotation=torch.randn((P, 4), generator=g),
        active_sh_degree=3, max_sh_degree=3)
    m.get_xyz = m._xyz
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    opt = SimpleNamespace(include_feature=True)
    feats = torch.nn.Parameter(torch.randn((L, P, 3), generator=g))
    adam = Adam([feats], lr=0.01)
    slot = object.__new__(levels_graph.LevelsViewSlot)  # (a real slot needs a GPU: its checks are tested above)
    slot.levels = L
    bg = torch.zeros(3)
    make = levels_graph.GraphedLevelsStep
    with pytest.raises(ValueError, match="Parameter"):
        make(m, feats.detach(), adam, slot, pipe, bg, opt)
    with pytest.raises(ValueError, match=r"\(L, P, 3\)"):
        bad = torch.nn.Parameter(torch.zeros((L, P + 1, 3)))
        make(m, bad, Adam([bad], lr=0.01), slot, pipe, bg, opt)
    with pytest.raises(ValueError, match="langsplat_amd.optim.Adam"):
        make(m, feats, torch.optim.Adam([feats]), slot, pipe, bg, opt)
    with pytest.raises(ValueError, match="one parameter"):
        make(m, feats, Adam([feats, torch.nn.Parameter(torch.zeros(3))], lr=0.01), slot, pipe, bg, opt)
    with pytest.raises(ValueError, match="LevelsViewSlot"):
        make(m, feats, adam, _cam(), pipe, bg, opt)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        make(m, feats, adam, slot, pipe, bg, opt)
    import langsplat_amd
    assert langsplat_amd.GraphedLevelsStep is make and langsplat_amd.LevelsViewSlot is levels_graph.LevelsViewSlot
