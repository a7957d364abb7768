"""Open-vocabulary query on the GPU: lsr_query_relevancy (decoder MLP + normalisation + phrase
similarities + relevancy in one kernel) against the CPU references of tests/query_ref.py.

Tolerance: e_ref = max |fp32 torch restatement of the reference - fp64| on the test's own inputs
(computed on the CPU, independent of the kernel); the kernel must stay within 8 e_ref of the fp64
reference, for the relevancy and for the decoded vectors separately.  The factor covers the
different accumulation order and the device's exp / sqrt / division.

The parity cases of one decoder and phrase set share ONE input set of 1000 pixels and its references
(computed once); a case with N pixels runs the first N of them and takes e_ref over those N, its own
inputs.  The exception is N = 1, which takes e_ref over the whole set: a maximum over a single pixel
is no yardstick (there the fp32 restatement happens to land within 3.4e-10 of fp64, below half an
ulp of the result, which no fp32 evaluation can promise)."""
import numpy as np
import pytest
import torch

from langsplat_amd import query
from langsplat_amd.query import Decoder, decode, relevancy_map, render_relevancy
from tests import query_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = -77.25
WIDTHS = [query_ref.CANONICAL, [16, 32, 32], [16]]
SIZES = [1, 63, 64, 65, 257, 1000]
PHRASES = [(1, 1), (3, 4), (17, 4), (60, 4)]
SEED = 7


def _run(c, n_pos, n_neg, layout, with_decoded=True, N=None):
    """One launch over the case's first N pixels through the binding, with oversized, canary-filled
    outputs -> (relevancy, decoded)."""
    dec = Decoder.from_arrays(c["weights"], c["biases"], device=DEV)
    N, D = c["pixels"].shape[0] if N is None else N, dec.dim
    pix = torch.from_numpy(c["pixels"][:N]).to(DEV)
    feat, cs, ps = (pix.t().contiguous(), N, 1) if layout == "chw" else (pix.contiguous(), 1, 3)
    phrases = torch.from_numpy(np.concatenate([c["pos"], c["neg"]])).to(DEV)
    out = torch.full((n_pos * N + 64,), CANARY, device=DEV)
    decoded = torch.full((N * D + 64,), CANARY, device=DEV) if with_decoded else None
    query._launch(dec, feat, 0, N, cs, ps, phrases, n_pos, n_neg, out, 0, decoded=decoded)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[n_pos * N:] == CANARY).all(), "relevancy written past n_pos * N"
    assert (out[:n_pos * N] != CANARY).all(), "relevancy not written in full"
    if with_decoded:
        decoded = decoded.cpu().numpy()
        assert (decoded[N * D:] == CANARY).all(), "decoded rows written past N * D"
        decoded = decoded[:N * D].reshape(N, D)
    return out[:n_pos * N].reshape(n_pos, N), decoded


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("phr", PHRASES, ids=lambda p: f"pos{p[0]}neg{p[1]}")
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "x".join(map(str, w)))
def test_relevancy_and_decoded_match_the_references(widths, N, phr, layout):
    n_pos, n_neg = phr
    c = query_ref.references(widths, max(SIZES), n_pos, n_neg, SEED)
    rel, dec = _run(c, n_pos, n_neg, layout, N=N)
    err_rel = float(np.abs(rel.astype(np.float64) - c["rel64"][:, :N]).max())
    err_dec = float(np.abs(dec.astype(np.float64) - c["dec64"][:N]).max())
    M = N if N > 1 else max(SIZES)  # the pixels e_ref is taken over (module docstring)
    e_rel = float(np.abs(c["rel32"][:, :M].astype(np.float64) - c["rel64"][:, :M]).max())
    e_dec = float(np.abs(c["dec32"][:M].astype(np.float64) - c["dec64"][:M]).max())
    print(f"query parity {widths} N={N} pos={n_pos} neg={n_neg} {layout}: relevancy {err_rel:.3e} "
          f"(e_ref {e_rel:.3e}), decoded {err_dec:.3e} (e_ref {e_dec:.3e})")
    assert c["rel64"].std(axis=1).mean() >= 0.02  # the spread over pixels: the output depends on the input
    assert err_rel <= 8 * e_rel
    assert err_dec <= 8 * e_dec


# decoders that take the kernel's other paths: weight chunks of 4 and 8 input columns (a wide hidden
# layer leaves less LDS for the staging), widths of 16 mod 32 (a half-filled feature tile, as a hidden
# and as the last layer), the most layers, and more than 32 phrases on a narrow last layer
EXTRA = [([48, 512, 16], (3, 4)), ([16, 448, 64], (3, 4)), ([16] * 8, (3, 4)), ([32, 48], (40, 4))]


@pytest.mark.parametrize("widths,phr", EXTRA, ids=lambda v: "x".join(map(str, v)))
def test_other_decoder_shapes(widths, phr):
    n_pos, n_neg = phr
    c = query_ref.references(widths, 257, n_pos, n_neg, SEED)
    rel, dec = _run(c, n_pos, n_neg, "chw")
    err_rel = float(np.abs(rel.astype(np.float64) - c["rel64"]).max())
    err_dec = float(np.abs(dec.astype(np.float64) - c["dec64"]).max())
    print(f"query parity {widths} N=257 pos={n_pos} neg={n_neg}: relevancy {err_rel:.3e} "
          f"(e_ref {c['e_rel']:.3e}), decoded {err_dec:.3e} (e_ref {c['e_dec']:.3e})")
    assert c["rel64"].std(axis=1).mean() >= 0.02
    assert err_rel <= 8 * c["e_rel"]
    assert err_dec <= 8 * c["e_dec"]


def test_two_calls_are_bit_identical_and_streams_agree():
    c = query_ref.references(query_ref.CANONICAL, 1000, 3, 4, SEED)
    a, da = _run(c, 3, 4, "chw")
    b, db = _run(c, 3, 4, "chw")
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(da, db)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s, ds = _run(c, 3, 4, "chw")
    np.testing.assert_array_equal(a, s)
    np.testing.assert_array_equal(da, ds)
    # without out_decoded the relevancy is the same
    n, _ = _run(c, 3, 4, "chw", with_decoded=False)
    np.testing.assert_array_equal(a, n)


def test_public_api_levels_layouts_and_decode():
    """relevancy_map over 2 levels in both layouts and a single (3, H, W) map; embeddings in fp16 and
    fp64 are converted to fp32 first; decode() returns the unit vectors."""
    H, W, n_pos, n_neg = 9, 13, 3, 4
    N = H * W
    cs = [query_ref.references([16, 32, 32], N, n_pos, n_neg, SEED + i) for i in range(2)]
    c = cs[0]
    dec = Decoder.from_state_dict(query_ref.state_dict_of(c["weights"], c["biases"]), device=DEV)
    pix = np.stack([cs[0]["pixels"], cs[1]["pixels"]])  # (2, N, 3): level 1 has other pixels
    want = np.stack([query_ref.relevancy_f64(p, c["weights"], c["biases"], c["pos"], c["neg"]) for p in pix])
    hwc = torch.from_numpy(pix).view(2, H, W, 3).to(DEV)
    chw = hwc.permute(0, 3, 1, 2).contiguous()
    pos, neg = torch.from_numpy(c["pos"]).to(DEV), torch.from_numpy(c["neg"]).to(DEV)
    r_chw = relevancy_map(chw, dec, pos, neg)
    r_hwc = relevancy_map(hwc, dec, pos, neg, layout="hwc")
    r_one = relevancy_map(chw[1], dec, pos, neg)
    r_f64 = relevancy_map(chw, dec, pos.double(), neg.double().cpu())
    assert r_chw.shape == (2, n_pos, H, W) and r_one.shape == (1, n_pos, H, W)
    assert torch.equal(r_chw, r_hwc) and torch.equal(r_chw[1:], r_one) and torch.equal(r_chw, r_f64)
    tol = 8 * max(c["e_rel"], cs[1]["e_rel"])
    assert np.abs(r_chw.cpu().numpy().reshape(2, n_pos, N) - want).max() <= tol
    r_f16 = relevancy_map(chw, dec, pos.half(), neg.half())
    want16 = np.stack([query_ref.relevancy_f64(p, c["weights"], c["biases"], c["pos"].astype(np.float16),
                                               c["neg"].astype(np.float16)) for p in pix])
    assert np.abs(r_f16.cpu().numpy().reshape(2, n_pos, N) - want16).max() <= tol
    d = decode(torch.from_numpy(c["pixels"]).to(DEV), dec)
    assert d.shape == (N, 32) and np.abs(d.cpu().numpy() - c["dec64"]).max() <= 8 * c["e_dec"]
    with pytest.raises(ValueError, match="layout"):
        relevancy_map(chw, dec, pos, neg, layout="nhwc")
    with pytest.raises(ValueError, match="at most 64"):
        relevancy_map(chw, dec, pos.repeat(21, 1), neg)


def test_render_relevancy_matches_the_reference_on_the_oracle_image():
    """End to end on tests.scenes.scene(P=2000, W=96, H=64): render_relevancy equals query_ref applied
    to the ORACLE's language image (the forward is bit-exact, so the kernel's inputs are identical);
    the pixels the scene leaves empty (feature 0, 0, 0) are included."""
    import bench
    from langsplat_amd.synthetic import make_cameras, make_gaussians
    from oracle import oracle
    from tests.scenes import scene
    P, W, H, n_pos, n_neg = 2000, 96, 64, 3, 4
    st, _ = scene(P=P, W=W, H=H)
    g = make_gaussians(P, seed=0, sh_degree=3, extent=1.0, scale_range=(0.02, 0.12))  # scene()'s Gaussians, raw
    a_op, a_sc, a_rot, a_lang = oracle.activate(oracle.RAW_ALL, g.opacity, g.scaling, g.rotation, g.language_feature)
    run = oracle.forward(st, means3D=g.xyz.clone(), opacities=torch.from_numpy(a_op), scales=torch.from_numpy(a_sc),
                         rotations=torch.from_numpy(a_rot), shs=torch.cat((g.features_dc, g.features_rest), 1),
                         language_feature_precomp=torch.from_numpy(a_lang))
    c = query_ref.make_case(query_ref.CANONICAL, 1, n_pos, n_neg, SEED)
    dec = Decoder.from_arrays(c["weights"], c["biases"], device=DEV)
    model = bench.Model(g.to(DEV), include_feature=True)
    cam = make_cameras(1, W, H, device=DEV)[0]
    pkg = render_relevancy(cam, model, bench.Pipe, torch.zeros(3, device=DEV), bench.Opt, dec,
                           torch.from_numpy(c["pos"]).to(DEV), torch.from_numpy(c["neg"]).to(DEV))
    torch.cuda.synchronize()
    assert not pkg["language_feature_image"].requires_grad
    np.testing.assert_array_equal(pkg["language_feature_image"].cpu().numpy(), run.language)
    pix = run.language.reshape(3, H * W).T.copy()
    empty = int((np.abs(pix).sum(axis=1) == 0).sum())
    assert 0 < empty < H * W
    args = (pix, c["weights"], c["biases"])
    rel64 = query_ref.relevancy_f64(*args, c["pos"], c["neg"])
    e_ref = float(np.abs(query_ref.relevancy_torch32(*args, c["pos"], c["neg"]).numpy() - rel64).max())
    got = pkg["relevancy"].cpu().numpy()
    assert got.shape == (1, n_pos, H, W)
    err = float(np.abs(got.reshape(n_pos, H * W) - rel64).max())
    print(f"render_relevancy: {empty} empty pixels, error {err:.3e} (e_ref {e_ref:.3e})")
    assert rel64.std(axis=1).mean() >= 0.02
    assert err <= 8 * e_ref


def test_relevancy_map_keeps_the_decoded_map_on_chip():
    """416 x 632, canonical decoder, n_pos = 4: the decoded map alone would be 538 MB; relevancy_map's
    peak allocation stays below 64 MB (a composition of torch ops cannot)."""
    H, W, n_pos, n_neg = 416, 632, 4, 4
    c = query_ref.make_case(query_ref.CANONICAL, 1, n_pos, n_neg, SEED)
    dec = Decoder.from_arrays(c["weights"], c["biases"], device=DEV)
    pos, neg = torch.from_numpy(c["pos"]).to(DEV), torch.from_numpy(c["neg"]).to(DEV)
    gen = torch.Generator().manual_seed(3)
    sem = (torch.nn.functional.normalize(torch.randn((1, 3, H, W), generator=gen), dim=1)
           * torch.rand((1, 1, H, W), generator=gen)).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = relevancy_map(sem, dec, pos, neg)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - base
    print(f"relevancy_map 416x632 peak allocation delta: {delta / 2 ** 20:.1f} MiB")
    assert delta < 64 * 2 ** 20
    r = r.cpu().numpy()
    assert r.shape == (1, n_pos, H, W) and np.isfinite(r).all() and r.std() >= 0.02
    # a sample of pixels against the fp64 reference
    idx = np.random.default_rng(0).choice(H * W, 512, replace=False)
    pix = sem[0].reshape(3, H * W).t()[torch.from_numpy(idx).to(DEV)].cpu().numpy()
    rel64 = query_ref.relevancy_f64(pix, c["weights"], c["biases"], c["pos"], c["neg"])
    e_ref = float(np.abs(query_ref.relevancy_torch32(pix, c["weights"], c["biases"], c["pos"], c["neg"]).numpy()
                         - rel64).max())
    assert np.abs(r.reshape(n_pos, H * W)[:, idx] - rel64).max() <= 8 * e_ref
