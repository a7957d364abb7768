"""Open-vocabulary semantic map and label statistics, the parts that need no GPU: the CPU references against
the fixture made from the reference's own get_semantic_map (tests/golden/make_semantic_golden.py), the
conditions the GPU parity test puts on its inputs (from the references alone), the ctypes mirrors of the
two argument structs, the argument validation of lsr_query_semantic / lsr_label_stats and label_stats'
derived metrics."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from langsplat_amd import _native
from langsplat_amd.query import Decoder, label_metrics, label_stats, semantic_map
from tests import query_ref, semantic_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "semantic.npz")
# the GPU parity test's cases (tests/test_gpu_semantic.py)
WIDTHS = [query_ref.CANONICAL, [16, 32, 32], [16]]
SIZES = [1, 63, 64, 65, 257, 1000]
PHRASES = [(1, 1), (3, 4), (17, 4), (28, 4), (29, 4), (60, 4)]


@pytest.mark.parametrize("name", ["canonical", "small"])
def test_references_reproduce_the_reference_fixture(name):
    g = np.load(GOLDEN)
    widths = [int(w) for w in g[f"{name}_widths"]]
    n_labels, n_neg, seed = int(g[f"{name}_n_labels"]), int(g[f"{name}_n_neg"]), int(g[f"{name}_seed"])
    c = query_ref.make_case(widths, 64, n_labels, n_neg, seed)
    np.testing.assert_array_equal(c["pixels"], g[f"{name}_pixels"])
    want = g[f"{name}_labels"]
    assert want.dtype == np.int64 and want.shape == (1, 8, 8)
    want = want.reshape(64)
    assert (want == -1).any() and len(set(want[want >= 0].tolist())) >= 2  # what the seeds were picked for
    args = (c["pixels"], c["weights"], c["biases"], c["pos"], c["neg"])
    _, l32, _ = semantic_ref.semantic_torch32(*args)
    assert l32.dtype == torch.int64
    np.testing.assert_array_equal(l32.numpy(), want)
    _, l64, s64 = semantic_ref.semantic_f64(*args)
    np.testing.assert_array_equal(l64, want)
    assert ((s64 > 1.0 / (n_labels + n_neg)) & (s64 <= 1.0)).all()  # the winner's share of a softmax


@pytest.mark.parametrize("phr", PHRASES, ids=lambda p: f"lab{p[0]}neg{p[1]}")
@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "x".join(map(str, w)))
def test_gpu_cases_are_decided_and_the_fp32_reference_agrees(widths, phr):
    """The conditions on the GPU parity cases, from the references alone: at most 1 % of a case's
    pixels undecided (none when N < 100); on every decided pixel the reference's fp32 evaluation has
    the fp64 label; -1 and labels both occur wherever the set has more than one phrase per side."""
    n_labels, n_neg = phr
    c = semantic_ref.references(widths, max(SIZES), n_labels, n_neg)
    for N in SIZES:
        e_sim, e_score, decided = semantic_ref.yardsticks(c, N)
        undecided = int((~decided).sum())
        print(f"semantic inputs {widths} lab={n_labels} neg={n_neg} N={N}: e_sim {e_sim:.2e} e_score {e_score:.2e} "
              f"smallest gap {c['gap'][:N].min():.2e} undecided {undecided}")
        assert 0 < e_sim < 1e-6 and 0 < e_score < 2e-6
        assert undecided <= (N // 100 if N >= 100 else 0)
        np.testing.assert_array_equal(c["label32"][:N][decided], c["label64"][:N][decided])
    lab = c["label64"]
    assert (lab >= 0).any()
    if (tuple(widths), n_labels) not in semantic_ref.NO_NEGATIVE:
        assert (lab == -1).any()
    # the score's spread over the pixels dwarfs its tolerance: a kernel that ignored its input cannot pass
    assert c["score64"].std() > 100 * 8 * semantic_ref.yardsticks(c, max(SIZES))[1]


@pytest.mark.parametrize("cls,cname", [(_native.LsrQuerySemanticArgs, "lsr_query_semantic_args"),
                                       (_native.LsrLabelStatsArgs, "lsr_label_stats_args")])
def test_args_layouts_match_header(tmp_path, cls, cname):
    """The ctypes mirrors have the C header's field offsets and sizes (gcc on lsr.h)."""
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


def test_entry_points_are_exported_without_an_abi_bump():
    lib = _native.load()
    for name in ("lsr_query_semantic", "lsr_label_stats"):
        assert hasattr(lib, name) and name in _native.SIGNATURES
    assert lib.lsr_abi_version() == 18


def test_invalid_semantic_arguments_report_errors_without_gpu():
    """LSR_ERR_INVALID with a message before any device work (dummy pointers, never dereferenced)."""
    lib = _native.load()
    dummy = ctypes.c_void_p(256)

    def call(widths=(16, 32, 32), **kw):
        a = _native.LsrQuerySemanticArgs()
        a.N, a.channel_stride, a.pixel_stride = 100, 100, 1
        a.feature = a.weights = a.phrases = a.out_label = dummy
        w = (ctypes.c_int32 * max(len(widths), 1))(*widths)
        a.n_layers, a.widths = len(widths), w
        a.n_labels, a.n_neg = 3, 4
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.lsr_query_semantic(ctypes.byref(a), None)

    err = _native.last_error
    assert lib.lsr_query_semantic(None, None) == 1 and "lsr_query_semantic: null args" in err()
    assert call(N=-1) == 1 and "invalid N" in err()
    assert call(widths=()) == 1 and "n_layers" in err()
    assert call(widths=(16,) * 9) == 1 and "n_layers" in err()
    assert call(widths=(16, 24, 32)) == 1 and "width" in err()
    assert call(widths=(16, 1024)) == 1 and "width" in err()
    assert call(n_labels=0) == 1 and "phrase counts" in err()
    assert call(n_neg=0) == 1 and "phrase counts" in err()
    assert call(n_labels=61, n_neg=4) == 1 and "phrase counts" in err()
    assert call(out_label=None) == 1 and "null pointer" in err()
    assert call(weights=ctypes.c_void_p(260)) == 1 and "16-byte" in err()
    assert call(N=0) == 0  # valid: enqueues nothing, touches no pointer


def test_invalid_label_stats_arguments_report_errors_without_gpu():
    lib = _native.load()
    dummy = ctypes.c_void_p(256)

    def call(**kw):
        a = _native.LsrLabelStatsArgs()
        a.N, a.n_maps, a.gt_maps, a.n_classes = 100, 3, 3, 7
        a.pred = a.gt = a.out_counts = a.out_totals = dummy
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.lsr_label_stats(ctypes.byref(a), None)

    err = _native.last_error
    assert lib.lsr_label_stats(None, None) == 1 and "lsr_label_stats: null args" in err()
    assert call(n_classes=0) == 1 and "n_classes" in err()
    assert call(n_classes=65) == 1 and "n_classes" in err()
    assert call(gt_maps=2) == 1 and "gt_maps" in err()
    assert call(out_counts=None) == 1 and "null pointer" in err()
    assert call(out_totals=None) == 1 and "null pointer" in err()
    assert call(pred=None) == 1 and "null pointer" in err()
    assert call(N=-1) == 1 and "invalid size" in err()
    assert call(n_maps=-1, gt_maps=1) == 1 and "invalid size" in err()
    assert call(out_totals=ctypes.c_void_p(260)) == 1 and "8-byte" in err()
    assert call(N=0) == 0 and call(n_maps=0, gt_maps=1) == 0  # valid: enqueue nothing


def test_cpu_tensors_are_rejected_loudly():
    c = query_ref.make_case([16], 4, 1, 1, seed=0)
    d = Decoder.from_arrays(c["weights"], c["biases"], device="cpu")
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        semantic_map(torch.zeros(3, 2, 2), d, torch.from_numpy(c["pos"]), torch.from_numpy(c["neg"]))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        label_stats(torch.zeros(2, 4, 4, dtype=torch.int64), torch.zeros(4, 4, dtype=torch.int64), 3)


def test_label_metrics_match_numpy():
    """iou, miou and accuracy from given counts; class 2 of map 0 has an empty union (NaN, left out of
    miou) and map 1 has no valid pixel at all (every metric NaN)."""
    counts = np.array([[[5, 9, 7], [0, 4, 3], [0, 0, 0], [6, 6, 6]],
                       [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]], np.int64)
    totals = np.array([[11, 16], [0, 0]], np.int64)
    got = label_metrics(torch.from_numpy(counts), torch.from_numpy(totals))
    inter, pred, truth = (counts[..., i].astype(np.float64) for i in range(3))
    union = pred + truth - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = np.where(union > 0, inter / union, np.nan)
        miou = np.array([np.nanmean(iou[0]), np.nan])
        acc = totals[:, 0] / totals[:, 1].astype(np.float64)
    for k in ("iou", "miou", "accuracy"):
        assert got[k].dtype == torch.float64
    np.testing.assert_array_equal(got["iou"].numpy(), iou)
    np.testing.assert_array_equal(got["miou"].numpy(), miou)
    np.testing.assert_array_equal(got["accuracy"].numpy(), acc)
    assert np.isnan(iou[0, 2]) and got["miou"][0].item() == (5 / 11 + 0 / 7 + 1.0) / 3
