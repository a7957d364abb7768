"""Open-vocabulary query, the parts that need no GPU: the CPU references against the fixture made from
the reference's own code (tests/golden/make_query_golden.py), the Decoder's checkpoint parsing, the
ctypes mirror of lsr_query_args and the argument validation of lsr_query_relevancy."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from langsplat_amd import _native
from langsplat_amd.query import Decoder, relevancy_map
from tests import query_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "query.npz")
# 8 x the largest error of the reference's own fp32 evaluation against fp64 measured on these
# generators (3.7e-7 for the relevancy, 1.4e-7 for a decoded component): the GPU tests' bound
FP32_BOUND_REL, FP32_BOUND_DEC = 8 * 3.7e-7, 8 * 1.4e-7


@pytest.mark.parametrize("name", ["canonical", "small"])
def test_references_reproduce_the_reference_fixture(name):
    g = np.load(GOLDEN)
    widths = [int(w) for w in g[f"{name}_widths"]]
    n_pos, n_neg, seed = int(g[f"{name}_n_pos"]), int(g[f"{name}_n_neg"]), int(g[f"{name}_seed"])
    c = query_ref.make_case(widths, 64, n_pos, n_neg, seed)
    np.testing.assert_array_equal(c["pixels"], g[f"{name}_pixels"])
    want = g[f"{name}_relevancy"].reshape(n_pos, 64)  # (1, n_pos, 8, 8): one level, 64 pixels as 8 x 8
    args = (c["pixels"], c["weights"], c["biases"])
    rel32 = query_ref.relevancy_torch32(*args, c["pos"], c["neg"]).numpy()
    dec32 = query_ref.decode_torch32(*args).numpy()
    assert np.abs(rel32 - want).max() <= 1e-6
    assert np.abs(dec32[:8] - g[f"{name}_decoded"]).max() <= 1e-6
    rel64 = query_ref.relevancy_f64(*args, c["pos"], c["neg"])
    dec64 = query_ref.decode_f64(*args)
    assert np.abs(rel64 - want).max() <= FP32_BOUND_REL
    assert np.abs(dec64[:8] - g[f"{name}_decoded"]).max() <= FP32_BOUND_DEC
    np.testing.assert_allclose(np.linalg.norm(dec64, axis=1), 1.0, atol=1e-12)
    assert rel64.std(axis=1).mean() >= 0.02  # the relevancy depends on the pixel


@pytest.mark.parametrize("widths,floor", [(query_ref.CANONICAL, 0.04), ([16, 32, 32], 0.08), ([16], 0.08)])
def test_generated_inputs_spread_the_relevancy(widths, floor):
    """A kernel that ignored its input or dropped a layer cannot pass a parity test on these inputs."""
    c = query_ref.references(widths, 257, 3, 4, seed=11)
    assert c["rel64"].std(axis=1).mean() >= floor


def _autoencoder_state_dict(widths):
    """The layout of the reference's Autoencoder().state_dict() (autoencoder/model.py:5-25), from plain
    nn.Linears: encoder Linear / BatchNorm1d / ReLU, decoder Linear, [ReLU, Linear]*."""
    nn = torch.nn
    enc_dims = [256, 128, 64, 32, 3]
    enc = []
    for i, d in enumerate(enc_dims):
        if i == 0:
            enc.append(nn.Linear(512, d))
        else:
            enc += [nn.BatchNorm1d(enc_dims[i - 1]), nn.ReLU(), nn.Linear(enc_dims[i - 1], d)]
    dec = []
    for i, d in enumerate(widths):
        if i == 0:
            dec.append(nn.Linear(3, d))
        else:
            dec += [nn.ReLU(), nn.Linear(widths[i - 1], d)]

    class AE(nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder = nn.ModuleList(enc)
            self.decoder = nn.ModuleList(dec)
    return AE().state_dict()


def test_decoder_parses_the_autoencoder_state_dict():
    torch.manual_seed(0)
    sd = _autoencoder_state_dict(query_ref.CANONICAL)
    assert "encoder.0.weight" in sd and "decoder.12.bias" in sd and "decoder.1.weight" not in sd
    d = Decoder.from_state_dict(sd, device="cpu")
    assert d.widths == query_ref.CANONICAL and d.dim == 512
    want = torch.cat([sd[f"decoder.{2 * i}.{k}"].reshape(-1) for i in range(7) for k in ("weight", "bias")])
    assert d.packed.dtype == torch.float32 and torch.equal(d.packed, want)
    assert d.packed.numel() == 241440  # weights and biases: ~966 KB at the canonical widths
    # from_arrays packs the same buffer
    ws = [sd[f"decoder.{2 * i}.weight"].numpy() for i in range(7)]
    bs = [sd[f"decoder.{2 * i}.bias"].numpy() for i in range(7)]
    assert torch.equal(Decoder.from_arrays(ws, bs, device="cpu").packed, want)


def test_decoder_rejects_what_the_kernel_does_not_support():
    sd = _autoencoder_state_dict([16, 32, 32])
    missing = {k: v for k, v in sd.items() if k != "decoder.2.bias"}
    with pytest.raises(ValueError, match="missing decoder.2.bias"):
        Decoder.from_state_dict(missing, device="cpu")
    with pytest.raises(ValueError, match="multiples of 16"):
        Decoder.from_state_dict(_autoencoder_state_dict([16, 24]), device="cpu")
    with pytest.raises(ValueError, match="multiples of 16"):
        Decoder.from_state_dict(_autoencoder_state_dict([16, 1024]), device="cpu")
    bad_in = {"decoder.0.weight": torch.zeros(16, 4), "decoder.0.bias": torch.zeros(16)}
    with pytest.raises(ValueError, match="input width 4, expected 3"):
        Decoder.from_state_dict(bad_in, device="cpu")
    with pytest.raises(ValueError, match="no decoder"):
        Decoder.from_state_dict({k: v for k, v in sd.items() if k.startswith("encoder.")}, device="cpu")
    with pytest.raises(ValueError, match="1 to 8 layers"):
        Decoder.from_arrays([np.zeros((16, 3))] + [np.zeros((16, 16))] * 8, [np.zeros(16)] * 9, device="cpu")


def test_cpu_map_is_rejected_loudly():
    c = query_ref.make_case([16], 4, 1, 1, seed=0)
    d = Decoder.from_arrays(c["weights"], c["biases"], device="cpu")
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        relevancy_map(torch.zeros(3, 2, 2), d, torch.from_numpy(c["pos"]), torch.from_numpy(c["neg"]))


def test_query_args_layout_matches_header(tmp_path):
    """The ctypes mirror of lsr_query_args has the C header's field offsets and size (gcc on lsr.h)."""
    cls = _native.LsrQueryArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lsr.h"', "int main(void) {",
             'printf("sizeof %zu\\n", sizeof(lsr_query_args));']
    for f in cls._fields_:
        lines.append(f'printf("{f[0]} %zu\\n", offsetof(lsr_query_args, {f[0]}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                   text=True).stdout.splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(cls)
    for f in cls._fields_:
        assert int(got[f[0]]) == getattr(cls, f[0]).offset, f[0]


def test_query_entry_point_is_exported_without_an_abi_bump():
    lib = _native.load()
    assert hasattr(lib, "lsr_query_relevancy") and "lsr_query_relevancy" in _native.SIGNATURES
    assert lib.lsr_abi_version() == 18  # 17 when the query was added; 18 removed a measurement hook


def test_invalid_query_arguments_report_errors_without_gpu():
    """LSR_ERR_INVALID with a message before any device work (dummy pointers, never dereferenced)."""
    lib = _native.load()
    dummy = ctypes.c_void_p(256)

    def call(widths=(16, 32, 32), **kw):
        a = _native.LsrQueryArgs()
        a.N, a.channel_stride, a.pixel_stride = 100, 100, 1
        a.feature = a.weights = a.phrases = a.out_relevancy = dummy
        w = (ctypes.c_int32 * max(len(widths), 1))(*widths)
        a.n_layers, a.widths = len(widths), w
        a.n_pos, a.n_neg = 3, 4
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.lsr_query_relevancy(ctypes.byref(a), None)

    assert lib.lsr_query_relevancy(None, None) == 1 and "null args" in _native.last_error()
    assert call(N=-1) == 1 and "invalid N" in _native.last_error()
    assert call(widths=()) == 1 and "n_layers" in _native.last_error()
    assert call(widths=(16,) * 9) == 1 and "n_layers" in _native.last_error()
    assert call(widths=(16, 24, 32)) == 1 and "width" in _native.last_error()
    assert call(widths=(16, 1024)) == 1 and "width" in _native.last_error()
    assert call(n_neg=0) == 1 and "phrase counts" in _native.last_error()
    assert call(n_pos=0) == 1 and "phrase counts" in _native.last_error()
    assert call(n_pos=61, n_neg=4) == 1 and "phrase counts" in _native.last_error()
    assert call(out_relevancy=None) == 1 and "null pointer" in _native.last_error()
    assert call(weights=ctypes.c_void_p(260)) == 1 and "16-byte" in _native.last_error()
