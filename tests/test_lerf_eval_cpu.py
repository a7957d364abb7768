"""LERF evaluation, the parts that need no GPU: the CPU references against the fixture made from the
reference's own smooth() (tests/golden/make_lerf_eval_golden.py) and against scipy, the ctypes
mirrors of the lsr_eval_* structs, and the argument validation of lsr_eval_filter / lsr_eval_masks."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from langsplat_amd import _native, lerf_eval
from tests import lerf_eval_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lerf_eval.npz")


def test_smooth_closed_form_equals_the_reference_fixture():
    g = np.load(GOLDEN)
    keys = sorted(k[len("mask_"):] for k in g.files if k.startswith("mask_"))
    assert len(keys) == 30  # 6 shapes x 5 densities
    changed = 0
    for k in keys:
        got = ref.smooth_closed_form(g[f"mask_{k}"])
        np.testing.assert_array_equal(got, g[f"smooth_{k}"], err_msg=k)
        changed += int((got != g[f"mask_{k}"]).sum())
    assert changed > 100  # the fixture exercises the filter: it is not the identity on these masks
    # the quirk: an all-ones mask stays all ones, though the last row / column are in no window
    ones = g["smooth_33x65_d10"]
    assert ones.all()


def test_box_f64_agrees_with_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    for (H, W) in [(16, 16), (17, 31), (33, 65), (97, 61)]:
        x = ref.relevancy_like(H, W, seed=5)[0].astype(np.float64)
        want = ndimage.correlate(x, np.ones((30, 30)) / 900, mode="mirror")
        assert np.abs(ref.box_f64(x) - want).max() <= 1e-14, (H, W)


def test_reflection_and_the_fp32_yardstick():
    """reflect101 restates gfedcb|abcdefgh|gfedcba with repeated reflection; box_torch32 (F.pad reflect
    where it applies, reflection by index below 16) stays within fp32 rounding of box_f64."""
    np.testing.assert_array_equal(ref.reflect101(np.arange(-6, 14), 8),
                                  [6, 5, 4, 3, 2, 1, 0, 1, 2, 3, 4, 5, 6, 7, 6, 5, 4, 3, 2, 1])
    np.testing.assert_array_equal(ref.reflect101(np.arange(-5, 6), 2), [1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1])
    np.testing.assert_array_equal(ref.reflect101(np.arange(-5, 8), 3), [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1])
    for (H, W) in [(2, 2), (5, 3), (16, 16), (33, 65)]:
        c = ref.filter_case(H, W, seed=5)
        assert 0 < c["e_ref"] < 1e-5, (H, W, c["e_ref"])
    # a tap range of -15 .. +14, not -14 .. +15: an impulse at column 20 reaches outputs 6 .. 35
    x = np.zeros((40, 60))
    x[20, 20] = 900.0
    a = ref.box_f64(x)
    assert a[20, 6] == 1.0 and a[20, 35] == 1.0 and a[20, 5] == 0.0 and a[20, 36] == 0.0
    assert a[6, 20] == 1.0 and a[35, 20] == 1.0 and a[5, 20] == 0.0 and a[36, 20] == 0.0


def test_generated_maps_give_masks_that_are_neither_empty_nor_full():
    for (H, W) in [(33, 65), (48, 80)]:
        for seed in range(4):
            b = ref.filter_case(H, W, seed)["blend64"][0]
            for t in (0.4, 0.5):
                frac = (np.clip(ref.normalised_f64(b), 0, 1) > t).mean()
                assert 0.02 <= frac <= 0.5, (H, W, seed, t, frac)


@pytest.mark.parametrize("cls,cname", [(_native.LsrEvalStats, "lsr_eval_stats"),
                                       (_native.LsrEvalFilterArgs, "lsr_eval_filter_args"),
                                       (_native.LsrEvalMaskArgs, "lsr_eval_mask_args")])
def test_eval_struct_layouts_match_header(tmp_path, cls, cname):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lsr.h"', "int main(void) {",
             f'printf("sizeof %zu\\n", sizeof({cname}));']
    for f in cls._fields_:
        lines.append(f'printf("{f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                   text=True).stdout.splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(cls)
    assert len(got) == len(cls._fields_) + 1
    for f in cls._fields_:
        assert int(got[f[0]]) == getattr(cls, f[0]).offset, f[0]
    if cls is _native.LsrEvalStats:
        assert ctypes.sizeof(cls) == 16  # lerf_eval views the records as rows of 4 words


def test_eval_entry_points_are_exported_without_an_abi_bump():
    lib = _native.load()
    for name in ("lsr_eval_filter", "lsr_eval_masks"):
        assert hasattr(lib, name) and name in _native.SIGNATURES
    assert lib.lsr_abi_version() == 18


DUMMY = ctypes.c_void_p(256)


def _filter_call(**kw):
    a = _native.LsrEvalFilterArgs()
    a.n_maps, a.H, a.W = 6, 33, 65
    a.maps = a.out_avg = a.out_blend = a.out_stats = DUMMY
    for k, v in kw.items():
        setattr(a, k, v)
    return _native.load().lsr_eval_filter(ctypes.byref(a), None)


def _mask_call(**kw):
    a = _native.LsrEvalMaskArgs()
    a.n_maps, a.H, a.W, a.thresh, a.n_prompts = 6, 33, 65, 0.4, 2
    a.blend = a.stats = a.gt_mask = a.out_mask = a.out_mask_raw = a.out_counts = DUMMY
    for k, v in kw.items():
        setattr(a, k, v)
    return _native.load().lsr_eval_masks(ctypes.byref(a), None)


def test_invalid_eval_arguments_report_errors_without_gpu():
    """LSR_ERR_INVALID with a message before any device work (dummy pointers, never dereferenced)."""
    lib, err = _native.load(), _native.last_error
    assert lib.lsr_eval_filter(None, None) == 1 and "lsr_eval_filter: null args" in err()
    assert lib.lsr_eval_masks(None, None) == 1 and "lsr_eval_masks: null args" in err()
    for call, name in ((_filter_call, "lsr_eval_filter"), (_mask_call, "lsr_eval_masks")):
        assert call(H=1) == 1 and name in err() and "at least 2" in err()
        assert call(W=1) == 1 and name in err() and "at least 2" in err()
        assert call(W=0) == 1 and "at least 2" in err()
        assert call(H=1 << 16, W=1 << 15) == 1 and name in err() and "2^31" in err()
        assert call(H=46341, W=46341) == 1 and "2^31" in err()
        assert call(n_maps=-1) == 1 and name in err() and "n_maps" in err()
    assert _filter_call(maps=None) == 1 and "null pointer" in err()
    assert _filter_call(out_stats=None) == 1 and "null pointer" in err()
    assert _filter_call(out_stats=ctypes.c_void_p(260)) == 1 and "8-byte" in err()
    assert _mask_call(blend=None) == 1 and "null pointer" in err()
    assert _mask_call(stats=None) == 1 and "null pointer" in err()
    assert _mask_call(out_mask=None) == 1 and "null pointer" in err()
    assert _mask_call(out_counts=None) == 1 and "null pointer" in err()  # required with gt_mask
    assert _mask_call(n_prompts=0) == 1 and "n_prompts" in err()
    assert _mask_call(n_prompts=-2) == 1 and "n_prompts" in err()
    assert _mask_call(n_prompts=4) == 1 and "n_prompts" in err()  # 6 maps are no multiple of 4 prompts


def test_zero_maps_are_valid_and_enqueue_nothing():
    assert _filter_call(n_maps=0) == 0
    assert _filter_call(n_maps=0, out_avg=None, out_blend=None) == 0
    assert _mask_call(n_maps=0) == 0
    assert _mask_call(n_maps=0, gt_mask=None, out_counts=None, out_mask_raw=None, n_prompts=0) == 0


def test_cpu_tensors_are_rejected_loudly():
    vm = torch.zeros(3, 2, 8, 8)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        lerf_eval.smooth_relevancy(vm)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        lerf_eval.activate_stream(vm)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        lerf_eval.activate_stream(vm, torch.zeros(2, 8, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        lerf_eval.lerf_localization(vm, [np.zeros((1, 4))] * 2)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        lerf_eval.evaluate_frame(torch.zeros(3, 8, 8, 3), None, None, None, None, [])
    import langsplat_amd
    for name in ("smooth_relevancy", "activate_stream", "lerf_localization", "evaluate_frame"):
        assert getattr(langsplat_amd, name) is getattr(lerf_eval, name) and name in langsplat_amd.__all__
