"""The RGB loss without a GPU: the restatement of tests/rgb_loss_ref.py against bench.ssim, the
kernels' closed-form gradient against fp64 autograd, and the C ABI of
lsr_rgb_loss_* (exports, struct layouts, argument checks before any device work)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import bench
from langsplat_amd import _native
from tests import rgb_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH, TW = _native.RGB_LOSS_TILE
SHAPES = [(1, 1, 1), (3, 3, 7), (3, 5, 5), (1, 11, 11), (3, TH, TW), (3, TH + 1, TW + 1), (3, 2 * TH + 1, TW - 1),
          (2, 40, 130), (3, 96, 128), (2, 3, 17, 65)]
SYMBOLS = ("lsr_rgb_loss_scratch_bytes", "lsr_rgb_loss_forward", "lsr_rgb_loss_backward")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("kind", R.KINDS)
def test_restatement_equals_bench_ssim_in_fp64(kind, shape):
    image, gt = (t.double() for t in R.make_case(kind, shape))
    _, l1, ssim, smap = R.loss_terms(image, gt)
    x, y = image.reshape(-1, *shape[-2:]), gt.reshape(-1, *shape[-2:])  # bench.ssim takes (C,H,W)
    assert abs(float(ssim) - float(bench.ssim(x, y))) <= 1e-12
    assert float(l1) == float(torch.abs(image - gt).mean())
    assert smap.shape == image.shape


def test_taps_are_bench_ssims():
    gv, _ = bench._ssim_taps(R.WINDOW, 1, "cpu")
    assert torch.equal(R.taps(torch.float32), gv.flatten())
    assert abs(float(R.taps().sum()) - 1.0) < 1e-7


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("kind", R.KINDS)
def test_three_map_gradient_equals_fp64_autograd(kind, shape):
    """The derivation the backward kernel rests on: 1e-10 relative to the largest gradient entry."""
    image, gt = (t.double() for t in R.make_case(kind, shape))
    x = image.clone().requires_grad_(True)
    loss = R.loss_terms(x, gt, 0.2)[0]
    (auto,) = torch.autograd.grad(loss, x)
    closed = R.closed_form_grad(image, gt, 0.2)
    scale = float(auto.abs().max())
    if kind == "equal":
        # the fp64 gradient of x == y is zero up to rounding: on the scale of the L1 term's weight
        scale = 0.8 / image.numel()
    assert float((closed - auto).abs().max()) <= 1e-10 * scale


def test_library_exports_the_rgb_loss_symbols():
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "lsr.h")).read()
    assert (int(re.search(r"#define LSR_RGB_LOSS_TILE_H (\d+)", hdr).group(1)),
            int(re.search(r"#define LSR_RGB_LOSS_TILE_W (\d+)", hdr).group(1))) == _native.RGB_LOSS_TILE


def test_rgb_loss_struct_layouts_match_header(tmp_path):
    structs = {"lsr_rgb_loss_args": _native.LsrRgbLossArgs, "lsr_rgb_loss_bwd_args": _native.LsrRgbLossBwdArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lsr.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for f in cls._fields_:
            lines.append(f'printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        s, f, v = ln.split()
        got[(s, f)] = int(v)
    for cname, cls in structs.items():
        assert got[(cname, "sizeof")] == ctypes.sizeof(cls), cname
        for f in cls._fields_:
            assert got[(cname, f[0])] == getattr(cls, f[0]).offset, (cname, f[0])


def test_rgb_loss_argument_checks_without_gpu():
    """NULL args, a NULL required pointer and sizes below 1 are LSR_ERR_INVALID (1) with a message,
    before any device work (dummy non-null pointers, never dereferenced)."""
    lib = _native.load()
    d = 256
    assert lib.lsr_rgb_loss_forward(None, None) == 1 and "lsr_rgb_loss_forward" in _native.last_error()
    assert lib.lsr_rgb_loss_backward(None, None) == 1 and "lsr_rgb_loss_backward" in _native.last_error()

    def fwd(planes=3, H=8, W=8, **kw):
        a = _native.LsrRgbLossArgs(planes, H, W, 0.2, d, d, d, None, None, d)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.lsr_rgb_loss_forward(ctypes.byref(a), None)

    def bwd(planes=3, H=8, W=8, **kw):
        a = _native.LsrRgbLossBwdArgs(planes, H, W, 0.2, d, d, d, d, d)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.lsr_rgb_loss_backward(ctypes.byref(a), None)

    for f in ("image", "target", "out_terms", "scratch"):
        assert fwd(**{f: None}) == 1 and "null pointer" in _native.last_error(), f
    for f in ("image", "target", "maps", "dL_dloss", "out_dL_dimage"):
        assert bwd(**{f: None}) == 1 and "null pointer" in _native.last_error(), f
    for call in (fwd, bwd):
        for size in ({"planes": 0}, {"H": 0}, {"W": 0}, {"planes": -1}, {"H": -3}):
            assert call(**size) == 1 and "invalid size" in _native.last_error(), size
    assert fwd(scratch=260) == 1 and "8-byte" in _native.last_error()
    assert fwd(planes=1 << 30, H=1 << 20, W=1 << 20) == 1 and "tiles" in _native.last_error()
    assert lib.lsr_rgb_loss_scratch_bytes(0, 8, 8) == 0
    tiles = 3 * -(-(2 * TH + 1) // TH) * -(-(TW - 1) // TW)
    assert lib.lsr_rgb_loss_scratch_bytes(3, 2 * TH + 1, TW - 1) == 16 * tiles


def test_python_front_end_errors_without_gpu():
    from langsplat_amd import rgb_loss, ssim
    a = torch.zeros(3, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rgb_loss(a, a)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ssim(a, a)
