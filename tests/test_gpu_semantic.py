"""Open-vocabulary semantic maps on the GPU: lsr_query_semantic (decoder MLP + normalisation + phrase
similarities + label and score in one kernel) and lsr_label_stats (per-class counts against ground truth)
against the CPU references of tests/semantic_ref.py.

Yardsticks (tests/semantic_ref.py): e_sim and e_score, the errors of the reference's own fp32 evaluation
against fp64 on the case's inputs.  A pixel is decided when the fp64 gap between its two largest
similarities exceeds 8 e_sim; the kernel's label must equal the fp64 label on EVERY decided pixel and its
score must be within 8 e_score of fp64 on every pixel.  tests/test_semantic_cpu.py asserts, from the
references alone, that at most 1 % of a case's pixels are undecided (none below 100 pixels).

A parity case is the first N pixels of query_ref.make_case(widths, 1000, n_labels, n_neg, seed) with
seed = 20240 + n_labels, except the canonical decoder's 28-label set, whose seed is 30268 (20268 never
picks a negative); the references of a set are computed once and shared.  The counts of lsr_label_stats
are integers and must equal numpy's exactly."""
import numpy as np
import pytest
import torch

from langsplat_amd import query
from langsplat_amd.query import (Decoder, label_stats, relevancy_map, render_levels_semantic, render_semantic,
                                 semantic_map)
from tests import query_ref, semantic_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = -77.25
ICANARY = -123456
WIDTHS = [query_ref.CANONICAL, [16, 32, 32], [16]]
SIZES = [1, 63, 64, 65, 257, 1000]
PHRASES = [(1, 1), (3, 4), (17, 4), (28, 4), (29, 4), (60, 4)]  # 32 and 33 phrases straddle the second phrase tile


def _run(c, layout="chw", with_score=True, N=None, phrases=None, n_labels=None):
    """One launch over the case's first N pixels through the binding, with oversized, canary-filled
    outputs -> (label int32 (N,), score (N,) or None)."""
    dec = Decoder.from_arrays(c["weights"], c["biases"], device=DEV)
    N = c["pixels"].shape[0] if N is None else N
    pix = torch.from_numpy(c["pixels"][:N]).to(DEV)
    feat, cs, ps = (pix.t().contiguous(), N, 1) if layout == "chw" else (pix.contiguous(), 1, 3)
    if phrases is None:
        phrases, n_labels = np.concatenate([c["pos"], c["neg"]]), len(c["pos"])
    ph = torch.from_numpy(np.ascontiguousarray(phrases)).to(DEV)
    label = torch.full((N + 64,), ICANARY, dtype=torch.int32, device=DEV)
    score = torch.full((N + 64,), CANARY, device=DEV) if with_score else None
    query._launch_semantic(dec, feat, 0, N, cs, ps, ph, n_labels, ph.shape[0] - n_labels, label, 0, score, 0)
    torch.cuda.synchronize()
    label = label.cpu().numpy()
    assert (label[N:] == ICANARY).all(), "labels written past N"
    assert (label[:N] != ICANARY).all(), "labels not written in full"
    if with_score:
        score = score.cpu().numpy()
        assert (score[N:] == CANARY).all(), "scores written past N"
        assert (score[:N] != CANARY).all(), "scores not written in full"
        score = score[:N]
    return label[:N], score


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("phr", PHRASES, ids=lambda p: f"lab{p[0]}neg{p[1]}")
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "x".join(map(str, w)))
def test_labels_and_scores_match_the_references(widths, N, phr, layout):
    n_labels, n_neg = phr
    c = semantic_ref.references(widths, max(SIZES), n_labels, n_neg)
    label, score = _run(c, layout, N=N)
    e_sim, e_score, decided = semantic_ref.yardsticks(c, N)
    wrong = int((label[decided] != c["label64"][:N][decided]).sum())
    err = float(np.abs(score.astype(np.float64) - c["score64"][:N]).max())
    print(f"semantic parity {widths} N={N} lab={n_labels} neg={n_neg} {layout}: {wrong} wrong labels of "
          f"{int(decided.sum())} decided ({N - int(decided.sum())} undecided), score error {err:.3e} "
          f"= {err / e_score:.2f} e_score (e_score {e_score:.3e}, e_sim {e_sim:.3e})")
    assert ((label >= -1) & (label < n_labels)).all()
    assert wrong == 0
    assert err <= 8 * e_score


def _tie_case(n_base):
    """The base set's most frequent label d, repeated as one more label (index n_base) and as the first
    negative (index n_base + 1): the phrase matrix, its label count, d and the labels the base set's fp64
    labels imply (d wins both ties; everything else is unchanged)."""
    c = semantic_ref.references([16, 32, 32], 257, n_base, 4, seed=77 + n_base)
    base = c["label64"]
    d = int(np.bincount(base[base >= 0]).argmax())
    assert (base == d).sum() >= 10
    row = c["pos"][d:d + 1]
    phrases = np.concatenate([c["pos"], row, row, c["neg"]])
    return c, phrases, n_base + 1, d


@pytest.mark.parametrize("n_base", [3, 32], ids=["inside_the_first_32_rows", "across_the_32_row_boundary"])
def test_the_smaller_index_wins_a_tie(n_base):
    """Exact duplicates of a label row, as another label and as a negative: two equal rows run the same
    operations in the same order, so their similarities are equal bit for bit and the scan's strict >
    keeps the first.  With 32 base labels the duplicates sit at rows 32 and 33, in the second phrase tile."""
    c, phrases, n_labels, d = _tie_case(n_base)
    assert d < 32 and (n_base < 32 or n_labels > 32)
    label, _ = _run(c, phrases=phrases, n_labels=n_labels)
    _, _, decided = semantic_ref.yardsticks(c, 257)
    assert (label != n_base).all(), "the duplicate label won a tie against the smaller index"
    assert (label == d).sum() >= 10
    np.testing.assert_array_equal(label[decided], c["label64"][decided])  # the negative duplicate never wins either


def test_zero_norm_pixel_gets_label_zero_and_a_nan_score():
    c = dict(query_ref.make_case([16, 32, 32], 65, 3, 4, seed=5))
    c["biases"] = [np.zeros_like(b) for b in c["biases"]]
    c["pixels"] = c["pixels"].copy()
    c["pixels"][[0, 64]] = 0.0
    label, score = _run(c)
    assert label[0] == 0 and label[64] == 0 and np.isnan(score[0]) and np.isnan(score[64])
    assert np.isfinite(score[1:64]).all()
    with torch.no_grad():  # what the reference's ops give for such a pixel, on the CPU
        nan = torch.full((1, 7), float("nan"))
        assert int(torch.argmax(torch.softmax(10 * nan, dim=-1), dim=-1)) == 0


def test_two_calls_are_bit_identical_and_streams_agree():
    c = semantic_ref.references(query_ref.CANONICAL, 1000, 3, 4)
    la, sa = _run(c)
    lb, sb = _run(c)
    np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(sa, sb)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ls, ss = _run(c)
    np.testing.assert_array_equal(la, ls)
    np.testing.assert_array_equal(sa, ss)
    ln, _ = _run(c, with_score=False)
    ln2, _ = _run(c, with_score=False)
    np.testing.assert_array_equal(la, ln)
    np.testing.assert_array_equal(ln, ln2)


def test_relevancy_is_unchanged_by_a_semantic_call_on_the_same_stream():
    """The two kernels share the LDS plan and each opts into large dynamic LDS for itself (the canonical
    decoder needs more than 64 KiB)."""
    n_pos, n_neg = 3, 4
    c = semantic_ref.references(query_ref.CANONICAL, 1000, n_pos, n_neg)
    dec = Decoder.from_arrays(c["weights"], c["biases"], device=DEV)
    sem = torch.from_numpy(c["pixels"]).to(DEV).t().contiguous().view(1, 3, 25, 40)
    pos, neg = torch.from_numpy(c["pos"]).to(DEV), torch.from_numpy(c["neg"]).to(DEV)
    before = relevancy_map(sem, dec, pos, neg)
    lab = semantic_map(sem, dec, pos, neg)
    after = relevancy_map(sem, dec, pos, neg)
    torch.cuda.synchronize()
    assert torch.equal(before, after)
    _, _, decided = semantic_ref.yardsticks(c, 1000)
    np.testing.assert_array_equal(lab.cpu().numpy().reshape(-1)[decided], c["label64"][decided])


def test_public_api_levels_layouts_and_dtypes():
    H, W, n_labels, n_neg = 9, 13, 3, 4
    N = H * W
    cs = [semantic_ref.references([16, 32, 32], N, n_labels, n_neg, seed=7 + i) for i in range(2)]
    c = cs[0]
    dec = Decoder.from_state_dict(query_ref.state_dict_of(c["weights"], c["biases"]), device=DEV)
    pix = np.stack([cs[0]["pixels"], cs[1]["pixels"]])  # (2, N, 3): level 1 has other pixels
    hwc = torch.from_numpy(pix).view(2, H, W, 3).to(DEV)
    chw = hwc.permute(0, 3, 1, 2).contiguous()
    lab, neg = torch.from_numpy(c["pos"]).to(DEV), torch.from_numpy(c["neg"]).to(DEV)
    l_chw = semantic_map(chw, dec, lab, neg)
    l_hwc = semantic_map(hwc, dec, lab, neg, layout="hwc")
    l_32, s_32 = semantic_map(chw, dec, lab, neg, return_score=True, dtype=torch.int32)
    assert l_chw.dtype == torch.int64 and l_32.dtype == torch.int32 and s_32.dtype == torch.float32
    assert l_chw.shape == l_32.shape == s_32.shape == (2, H, W)
    assert torch.equal(l_chw, l_hwc) and torch.equal(l_chw, l_32.long())
    for i in range(2):  # the per-level calls
        one, s_one = semantic_map(chw[i], dec, lab, neg, return_score=True)
        assert one.shape == (1, H, W) and torch.equal(one[0], l_chw[i]) and torch.equal(s_one[0], s_32[i])
        want = semantic_ref.semantic_f64(pix[i], c["weights"], c["biases"], c["pos"], c["neg"])
        s32 = semantic_ref.semantic_torch32(pix[i], c["weights"], c["biases"], c["pos"], c["neg"])
        e_sim = float(np.abs(s32[0].numpy() - want[0]).max())
        e_score = float(np.abs(s32[2].numpy() - want[2]).max())
        decided = semantic_ref.top_gap(want[0]) > 8 * e_sim
        np.testing.assert_array_equal(l_chw[i].cpu().numpy().reshape(-1)[decided], want[1][decided])
        assert np.abs(s_32[i].cpu().numpy().reshape(-1) - want[2]).max() <= 8 * e_score
    with pytest.raises(ValueError, match="layout"):
        semantic_map(chw, dec, lab, neg, layout="nhwc")
    with pytest.raises(ValueError, match="at most 64"):
        semantic_map(chw, dec, lab.repeat(21, 1), neg)
    with pytest.raises(ValueError, match="dtype"):
        semantic_map(chw, dec, lab, neg, dtype=torch.int16)


def test_render_semantic_matches_the_reference_on_the_oracle_image():
    """End to end on tests.scenes.scene(P=2000, W=96, H=64): render_semantic equals the fp64 labels of
    the ORACLE's language image (the forward is bit-exact) on the decided pixels; the pixels the scene
    leaves empty (feature 0, 0, 0) are included."""
    import bench
    from langsplat_amd.synthetic import make_cameras, make_gaussians
    from oracle import oracle
    from tests.scenes import scene
    P, W, H, n_labels, n_neg = 2000, 96, 64, 3, 4
    st, _ = scene(P=P, W=W, H=H)
    g = make_gaussians(P, seed=0, sh_degree=3, extent=1.0, scale_range=(0.02, 0.12))  # scene()'s Gaussians, raw
    a_op, a_sc, a_rot, a_lang = oracle.activate(oracle.RAW_ALL, g.opacity, g.scaling, g.rotation, g.language_feature)
    run = oracle.forward(st, means3D=g.xyz.clone(), opacities=torch.from_numpy(a_op), scales=torch.from_numpy(a_sc),
                         rotations=torch.from_numpy(a_rot), shs=torch.cat((g.features_dc, g.features_rest), 1),
                         language_feature_precomp=torch.from_numpy(a_lang))
    c = query_ref.make_case(query_ref.CANONICAL, 1, n_labels, n_neg, 7)
    dec = Decoder.from_arrays(c["weights"], c["biases"], device=DEV)
    model = bench.Model(g.to(DEV), include_feature=True)
    cam = make_cameras(1, W, H, device=DEV)[0]
    pkg = render_semantic(cam, model, bench.Pipe, torch.zeros(3, device=DEV), bench.Opt, dec,
                          torch.from_numpy(c["pos"]).to(DEV), torch.from_numpy(c["neg"]).to(DEV), return_score=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(pkg["language_feature_image"].cpu().numpy(), run.language)
    pix = run.language.reshape(3, H * W).T.copy()
    empty = int((np.abs(pix).sum(axis=1) == 0).sum())
    assert 0 < empty < H * W
    args = (pix, c["weights"], c["biases"], c["pos"], c["neg"])
    s64, l64, p64 = semantic_ref.semantic_f64(*args)
    s32, _, p32 = semantic_ref.semantic_torch32(*args)
    e_sim = float(np.abs(s32.numpy() - s64).max())
    e_score = float(np.abs(p32.numpy() - p64).max())
    decided = semantic_ref.top_gap(s64) > 8 * e_sim
    assert pkg["semantic"].shape == (1, H, W) and pkg["semantic"].dtype == torch.int64
    assert pkg["semantic_score"].shape == (1, H, W)
    got = pkg["semantic"].cpu().numpy().reshape(-1)
    err = float(np.abs(pkg["semantic_score"].cpu().numpy().reshape(-1) - p64).max())
    print(f"render_semantic: {empty} empty pixels, {int((~decided).sum())} undecided, labels {np.unique(l64).tolist()}, "
          f"score error {err:.3e} (e_score {e_score:.3e})")
    assert (~decided).sum() <= H * W // 100
    assert len(np.unique(l64)) >= 2
    np.testing.assert_array_equal(got[decided], l64[decided])
    assert err <= 8 * e_score
    assert "semantic_score" not in render_semantic(cam, model, bench.Pipe, torch.zeros(3, device=DEV), bench.Opt, dec,
                                                   torch.from_numpy(c["pos"]).to(DEV), torch.from_numpy(c["neg"]).to(DEV))


def test_render_levels_semantic_equals_semantic_map_of_render_levels():
    import bench
    from langsplat_amd import levels
    from langsplat_amd.synthetic import make_cameras, make_gaussians
    P, W, H, L, n_labels, n_neg = 2000, 64, 48, 3, 3, 4
    c = query_ref.make_case([16, 32, 32], 1, n_labels, n_neg, 7)
    dec = Decoder.from_arrays(c["weights"], c["biases"], device=DEV)
    lab, neg = torch.from_numpy(c["pos"]).to(DEV), torch.from_numpy(c["neg"]).to(DEV)
    model = bench.Model(make_gaussians(P, seed=0, sh_degree=3, extent=1.0, scale_range=(0.02, 0.12)).to(DEV),
                        include_feature=True)
    cam = make_cameras(1, W, H, device=DEV)[0]
    bg = torch.zeros(3, device=DEV)
    feats = torch.stack([torch.nn.functional.normalize(torch.randn((P, 3), generator=torch.Generator().manual_seed(100 + l)))
                         for l in range(L)]).to(DEV)
    pkg = render_levels_semantic(cam, model, bench.Pipe, bg, bench.Opt, feats, dec, lab, neg, return_score=True)
    plain = levels.render_levels(cam, model, bench.Pipe, bg, bench.Opt, feats)
    want, want_score = semantic_map(plain["language_feature_images"], dec, lab, neg, return_score=True)
    assert pkg["semantic"].shape == (L, H, W) and pkg["semantic"].dtype == torch.int64
    assert torch.equal(pkg["language_feature_images"], plain["language_feature_images"])
    assert torch.equal(pkg["semantic"], want) and torch.equal(pkg["semantic_score"], want_score)
    assert len(torch.unique(want)) >= 2


# ---- lsr_label_stats ----------------------------------------------------------------------------

# a workgroup takes 2048 pixels per sweep and a map gets at most 1024 workgroups: from this N on the
# first workgroup takes a second sweep
SECOND_SWEEP_N = 1024 * 2048 + 1
STATS_SIZES = [1, 255, 256, 257, SECOND_SWEEP_N]
_LABELS = {}


def _label_maps(N, n_classes):
    """3 predicted and 3 ground-truth maps, shared by the cases (read-only): predictions from -1 to
    n_classes + 1 (-1 and values >= n_classes included), ground truth with -1 and 255 as ignore labels."""
    key = (N, n_classes)
    if key not in _LABELS:
        rng = np.random.default_rng(N % 1000 + n_classes)
        gt = rng.integers(0, n_classes, (3, N)).astype(np.int32)
        pred = np.where(rng.random((3, N)) < 0.6, gt, rng.integers(-1, n_classes + 2, (3, N))).astype(np.int32)
        ignore = rng.random((3, N))
        gt[ignore < 0.1] = -1
        gt[ignore > 0.9] = 255
        _LABELS[key] = (pred, gt)
    return _LABELS[key]


def _stats(pred, gt, n_classes):
    """lsr_label_stats through the binding on numpy (maps, N) inputs, outputs pre-filled with garbage and
    followed by a canary -> (counts, totals)."""
    maps, N = pred.shape
    p, g = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    counts = torch.full((maps * n_classes * 3 + 8,), 0x5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    totals = torch.full((maps * 2 + 8,), -99, dtype=torch.int64, device=DEV)
    query._label_stats_into(p, g, N, maps, gt.shape[0], n_classes, counts, totals)
    torch.cuda.synchronize()
    counts, totals = counts.cpu().numpy(), totals.cpu().numpy()
    assert (counts[maps * n_classes * 3:] == 0x5A5A5A5A5A5A).all() and (totals[maps * 2:] == -99).all()
    return counts[:maps * n_classes * 3].reshape(maps, n_classes, 3), totals[:maps * 2].reshape(maps, 2)


@pytest.mark.parametrize("n_classes", [1, 7, 64])
@pytest.mark.parametrize("shared_gt", [True, False], ids=["shared_gt", "gt_per_map"])
@pytest.mark.parametrize("maps", [1, 3])
@pytest.mark.parametrize("N", STATS_SIZES)
def test_label_counts_equal_numpy(N, maps, shared_gt, n_classes):
    pred, gt = _label_maps(N, n_classes)
    pred, gt = pred[:maps], gt[:1] if shared_gt else gt[:maps]
    if N > 1:
        assert (pred == -1).any() and (pred >= n_classes).any() and (gt == -1).any() and (gt == 255).any()
    want_c, want_t = semantic_ref.label_counts(pred, gt, n_classes)
    got_c, got_t = _stats(pred, gt, n_classes)
    np.testing.assert_array_equal(got_c, want_c)
    np.testing.assert_array_equal(got_t, want_t)
    again_c, again_t = _stats(pred, gt, n_classes)
    np.testing.assert_array_equal(got_c, again_c)
    np.testing.assert_array_equal(got_t, again_t)
    if N >= 255:
        assert want_t[:, 1].min() > 0 and (want_t[:, 0] < want_t[:, 1]).all() and want_t[:, 0].min() > 0


def test_a_map_without_a_valid_pixel_counts_nothing():
    pred, gt = _label_maps(257, 7)
    gt = gt.copy()
    gt[1] = np.where(gt[1] % 2 == 0, -1, 255)
    got_c, got_t = _stats(pred, gt, 7)
    assert (got_c[1] == 0).all() and (got_t[1] == 0).all() and got_t[0, 1] > 0 and got_t[2, 1] > 0
    want_c, want_t = semantic_ref.label_counts(pred, gt, 7)
    np.testing.assert_array_equal(got_c, want_c)
    np.testing.assert_array_equal(got_t, want_t)


def test_label_stats_of_a_semantic_map_end_to_end():
    """label_stats(semantic_map(...), gt) at 33 x 65 with 3 levels, against numpy on the same label maps."""
    H, W, L, n_labels, n_neg = 33, 65, 3, 3, 4
    N = H * W
    c = query_ref.make_case([16, 32, 32], L * N, n_labels, n_neg, 7)
    dec = Decoder.from_arrays(c["weights"], c["biases"], device=DEV)
    lab, neg = torch.from_numpy(c["pos"]).to(DEV), torch.from_numpy(c["neg"]).to(DEV)
    sem = torch.from_numpy(c["pixels"]).view(L, H, W, 3).to(DEV)
    pred = semantic_map(sem, dec, lab, neg, layout="hwc")
    rng = np.random.default_rng(3)
    gt = pred[0].cpu().numpy().copy()
    flip = rng.random((H, W))
    gt[flip < 0.2] = rng.integers(0, n_labels, (H, W))[flip < 0.2]
    gt[flip > 0.95] = 255
    out = label_stats(pred, torch.from_numpy(gt).to(DEV), n_labels)
    want_c, want_t = semantic_ref.label_counts(pred.cpu().numpy().reshape(L, N), gt.reshape(1, N), n_labels)
    np.testing.assert_array_equal(out["counts"].cpu().numpy(), want_c)
    np.testing.assert_array_equal(out["totals"].cpu().numpy(), want_t)
    inter, predicted, truth = (want_c[..., i].astype(np.float64) for i in range(3))
    union = predicted + truth - inter
    assert (union > 0).all()
    np.testing.assert_array_equal(out["iou"].cpu().numpy(), inter / union)
    np.testing.assert_allclose(out["miou"].cpu().numpy(), (inter / union).mean(axis=1), rtol=1e-14)  # a sum of 3
    np.testing.assert_array_equal(out["accuracy"].cpu().numpy(), want_t[:, 0] / want_t[:, 1].astype(np.float64))
    assert out["accuracy"][0] > out["accuracy"][1]  # level 0 is what the ground truth was made from
    # per-map ground truth and a single map
    per_map = label_stats(pred, pred, n_labels)
    assert torch.equal(per_map["counts"][..., 0], per_map["counts"][..., 1])
    one = label_stats(pred[1].to(torch.int32), torch.from_numpy(gt).to(DEV), n_labels)
    assert torch.equal(one["counts"][0], out["counts"][1])
