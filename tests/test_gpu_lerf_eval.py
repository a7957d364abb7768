"""LERF evaluation on the GPU: lsr_eval_filter (30 x 30 mean filter, blend, statistics) and
lsr_eval_masks (threshold, smooth(), intersection / union) against the CPU references of
tests/lerf_eval_ref.py, and the public functions of langsplat_amd.lerf_eval on top of them.

Tolerance of the filter: e_ref = max |fp32 torch restatement - fp64| on the case's own map (computed
on the CPU, independent of the kernel); avg and blend must stay within 8 e_ref of fp64 (the factor
covers the summation order).  Maps under 256 pixels take e_ref over the 33 x 65 case: a maximum over
a handful of pixels is no yardstick.  Everything after the filter is discrete and is checked EXACTLY
against numpy restatements applied to the kernel's own avg / blend; the end-to-end test against the
fp64 pipeline first asserts, on the CPU, that the reference alone has no pixel near the threshold.

Measured on an MI355X: avg is 3.2e-8 to 1.4e-7 from fp64 against e_ref of 5.3e-7 to 1.5e-6 (the table is
in DESIGN.md section 6b).

Each shape runs the kernels once (_gpu_case, cached); outputs are allocated oversized and
canary-filled."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from langsplat_amd import lerf_eval
from tests import lerf_eval_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY, CANARY_U8, PAD = -77.25, 0xAB, 64
SEED = 11
# tile and reflection edges: narrower than the kernel (reflected more than once), one tap short of /
# equal to / past a 32 x 64 tile, more than one tile in both axes; 6 maps = 3 levels x 2 prompts
CASES = [(2, 2, 1), (2, 9, 1), (5, 3, 1), (16, 16, 1), (17, 31, 1), (33, 65, 1), (64, 64, 1), (97, 61, 1), (33, 65, 6)]
IDS = [f"{h}x{w}x{n}" for h, w, n in CASES]


def _run_filter(maps, with_avg=True, with_blend=True):
    """lsr_eval_filter through the binding on (n, H, W) numpy maps -> dict of device tensors and
    numpy copies; the outputs are oversized and canary-filled."""
    n, H, W = maps.shape
    N = n * H * W
    m = torch.tensor(maps, device=DEV)  # a copy: the shared references are read-only
    avg = torch.full((N + PAD,), CANARY, device=DEV) if with_avg else None
    blend = torch.full((N + PAD,), CANARY, device=DEV) if with_blend else None
    stats = torch.full((4 * n + PAD,), CANARY, device=DEV)
    f = lerf_eval._filter(m, with_avg, with_blend,
                          out=(avg[:N].view(n, H, W) if with_avg else None,
                               blend[:N].view(n, H, W) if with_blend else None, stats))
    torch.cuda.synchronize()
    out = {"dev": f}
    for name, buf in (("avg", avg), ("blend", blend)):
        if buf is not None:
            h = buf.cpu().numpy()
            assert (h[N:] == CANARY).all(), f"{name} written past n_maps * H * W"
            assert (h[:N] != CANARY).all(), f"{name} not written in full"
            out[name] = h[:N].reshape(n, H, W)
    h = stats.cpu().numpy()
    assert (h[4 * n:] == CANARY).all(), "statistics written past n_maps records"
    out["stats"] = h[:4 * n].reshape(n, 4).copy()
    out["argmax"] = out["stats"].view(np.int32)[:, 3].copy()
    return out


def _run_masks(blend, stats, thresh, gt=None, with_raw=True):
    """lsr_eval_masks on device tensors blend (n, H, W) and stats -> numpy (mask, raw, counts)."""
    n, H, W = blend.shape
    N = n * H * W
    mask = torch.full((N + PAD,), CANARY_U8, dtype=torch.uint8, device=DEV)
    raw = torch.full((N + PAD,), CANARY_U8, dtype=torch.uint8, device=DEV) if with_raw else None
    counts = torch.full((2 * n + PAD,), -7, dtype=torch.int64, device=DEV) if gt is not None else None
    g = torch.from_numpy(np.ascontiguousarray(gt)).to(DEV) if gt is not None else None
    lerf_eval._masks(blend, stats, thresh, g, with_raw,
                     out=(mask[:N].view(n, H, W), raw[:N].view(n, H, W) if with_raw else None, counts))
    torch.cuda.synchronize()
    res = []
    for name, buf in (("mask", mask), ("raw mask", raw)):
        if buf is None:
            res.append(None)
            continue
        h = buf.cpu().numpy()
        assert (h[N:] == CANARY_U8).all(), f"{name} written past n_maps * H * W"
        assert (h[:N] <= 1).all(), f"{name} not written in full, or not 0 / 1"
        res.append(h[:N].reshape(n, H, W))
    if counts is not None:
        h = counts.cpu().numpy()
        assert (h[2 * n:] == -7).all(), "counts written past n_maps pairs"
        res.append(h[:2 * n].reshape(n, 2))
    else:
        res.append(None)
    return tuple(res)


@lru_cache(maxsize=None)
def _gpu_case(H, W, n):
    """The CPU references of one case and one run of the filter on it (shared by the tests; read-only)."""
    c = ref.filter_case(H, W, SEED, n)
    e_ref = c["e_ref"] if H * W >= 256 else ref.filter_case(33, 65, SEED, 1)["e_ref"]
    return c, e_ref, _run_filter(c["maps"])


@pytest.mark.parametrize("H,W,n", CASES, ids=IDS)
def test_filter_matches_the_references(H, W, n):
    c, e_ref, g = _gpu_case(H, W, n)
    err_avg = float(np.abs(g["avg"].astype(np.float64) - c["avg64"]).max())
    err_blend = float(np.abs(g["blend"].astype(np.float64) - c["blend64"]).max())
    print(f"eval filter parity {H}x{W} n_maps={n}: avg {err_avg:.3e}, blend {err_blend:.3e} (e_ref {e_ref:.3e})")
    assert c["maps"].std() >= 0.02  # the input depends on the position
    assert err_avg <= 8 * e_ref
    assert err_blend <= 8 * e_ref


@pytest.mark.parametrize("H,W,n", CASES, ids=IDS)
def test_statistics_are_exact_on_the_kernels_own_maps(H, W, n):
    c, e_ref, g = _gpu_case(H, W, n)
    for m in range(n):
        avg, blend, st = g["avg"][m], g["blend"][m], g["stats"][m]
        assert st[0].tobytes() == blend.min().tobytes(), "blend_min"
        assert st[1].tobytes() == blend.max().tobytes(), "blend_max"
        assert st[2].tobytes() == avg.max().tobytes(), "avg_max"
        assert int(g["argmax"][m]) == int(np.argmax(avg)), "avg_argmax is the first index of the maximum"
        a64 = c["avg64"][m]
        assert a64.max() - a64.reshape(-1)[g["argmax"][m]] <= 2 * 8 * e_ref
    # the public function returns the same, the arg-max as (y, x)
    s = lerf_eval.smooth_relevancy(torch.tensor(c["maps"], device=DEV))
    np.testing.assert_array_equal(s["avg"].cpu().numpy(), g["avg"])
    np.testing.assert_array_equal(s["blend"].cpu().numpy(), g["blend"])
    np.testing.assert_array_equal(s["blend_min"].cpu().numpy(), g["stats"][:, 0])
    np.testing.assert_array_equal(s["blend_max"].cpu().numpy(), g["stats"][:, 1])
    np.testing.assert_array_equal(s["avg_max"].cpu().numpy(), g["stats"][:, 2])
    np.testing.assert_array_equal(s["avg_argmax"].cpu().numpy(), np.stack(np.divmod(g["argmax"], W), axis=-1))


@pytest.mark.parametrize("H,W,n", CASES, ids=IDS)
def test_masks_are_exact_on_the_kernels_own_blend(H, W, n):
    c, e_ref, g = _gpu_case(H, W, n)
    n_prompts = 2 if n == 6 else 1
    gt = (np.random.default_rng(SEED + 1).random((n_prompts, H, W)) < 0.4).astype(np.uint8) * 3  # non-zero = set
    set_pixels = 0
    for thresh in (0.4, 0.5):
        mask, raw, counts = _run_masks(g["dev"]["blend"], g["dev"]["stats"], thresh, gt)
        for m in range(n):
            want_raw = ref.normalise_threshold_f32(g["blend"][m], g["stats"][m, 0], g["stats"][m, 1], thresh)
            np.testing.assert_array_equal(raw[m], want_raw)
            np.testing.assert_array_equal(mask[m], ref.smooth_closed_form(raw[m]))
            gm = gt[m % n_prompts] != 0
            assert counts[m, 0] == np.logical_and(gm, mask[m]).sum()
            assert counts[m, 1] == np.logical_or(gm, mask[m]).sum()
        set_pixels += int(raw.sum())
        # without the optional outputs the smoothed mask is the same
        mask2, _, _ = _run_masks(g["dev"]["blend"], g["dev"]["stats"], thresh, None, with_raw=False)
        np.testing.assert_array_equal(mask, mask2)
    assert set_pixels > 0
    # threshold -1: an all-ones raw mask keeps the closed form's last-row / last-column behaviour
    mask, raw, _ = _run_masks(g["dev"]["blend"], g["dev"]["stats"], -1.0)
    assert raw.all()
    for m in range(n):
        np.testing.assert_array_equal(mask[m], ref.smooth_closed_form(raw[m]))


def test_constant_map_gives_an_empty_mask():
    """max == min: the divisor is 1e-9f, the normalised map -1 everywhere."""
    H, W = 17, 31
    g = _run_filter(np.full((1, H, W), 0.625, dtype=np.float32))
    assert g["stats"][0, 0] == g["stats"][0, 1] == 0.625 and g["stats"][0, 2] == 0.625 and g["argmax"][0] == 0
    mask, raw, counts = _run_masks(g["dev"]["blend"], g["dev"]["stats"], 0.4, np.ones((1, H, W), dtype=np.uint8))
    assert not raw.any() and not mask.any()
    assert counts.tolist() == [[0, H * W]]


def test_last_row_and_column_are_in_no_window():
    """A blend that is high only in the last two rows and columns, with hand-made statistics: the raw
    mask has them set; smooth() never looks at the last row / column, so only the second-to-last
    contribute."""
    H, W = 40, 70
    blend = np.zeros((1, H, W), dtype=np.float32)
    blend[0, H - 2:, :] = 1.0
    blend[0, :, W - 2:] = 1.0
    stats = torch.tensor([[0.0, 1.0, 1.0, 0.0]], dtype=torch.float32, device=DEV)
    mask, raw, _ = _run_masks(torch.from_numpy(blend).to(DEV), stats, 0.4)
    np.testing.assert_array_equal(raw[0], (blend[0] > 0.5).astype(np.uint8))
    want = ref.smooth_closed_form(raw[0])
    np.testing.assert_array_equal(mask[0], want)
    full = np.ones((H, W), dtype=np.uint8)  # what a window that included the last row / column would see
    assert (want != full).any() and want[H - 1, W - 1] == 1 and want[H - 5, 0] == 0


E2E_SEED = 23  # no pixel of the fp64 reference within the margin of either threshold (asserted below)


@pytest.mark.parametrize("thresh", [0.4, 0.5])
def test_public_api_equals_the_fp64_pipeline(thresh):
    """activate_stream and lerf_localization at 33 x 65, 3 levels x 2 prompts, against the fp64
    pipeline.  The threshold is discontinuous, so the inputs are ones for which the REFERENCE ALONE
    has no pixel within m = 4 * 8 e_ref / (max - min) of it in normalised units (the kernel's blend,
    minimum and maximum are each within 8 e_ref of fp64, which moves a normalised value by less than
    m), and whose level scores differ by more than 2 * 8 e_ref: then every discrete result must be equal."""
    H, W, L, P = 33, 65, 3, 2
    c = ref.filter_case(H, W, E2E_SEED, L * P)
    e = c["e_ref"]
    t = float(np.float32(thresh))
    for b in c["blend64"]:
        margin = 4 * 8 * e / (b.max() - b.min())
        assert not (np.abs(ref.normalised_f64(b) - t) <= margin).any(), "pick another seed, not another margin"
    for score in (c["blend64"].reshape(L, P, -1).max(axis=2), c["avg64"].reshape(L, P, -1).max(axis=2)):
        s = np.sort(score, axis=0)
        assert (s[-1] - s[-2]).min() > 2 * 8 * e
    vm = c["maps"].reshape(L, P, H, W)
    gt = np.zeros((P, H, W), dtype=np.uint8)
    gt[0, 5:20, 10:40] = 1
    gt[1, 15:33, 30:65] = 255
    # boxes: prompt 0's holds every pixel whose fp64 avg is within 2 * 8 e_ref of the chosen level's
    # maximum (so it holds the kernel's arg-max whichever of them that is): a hit, given with its
    # corners swapped; prompt 1's holds none of them: a miss
    avg = c["avg64"].reshape(L, P, H, W)
    lv = avg.reshape(L, P, -1).max(axis=2).argmax(axis=0)
    near = [np.argwhere(avg[lv[k], k] >= avg[lv[k], k].max() - 2 * 8 * e) for k in range(P)]
    y0, x0 = near[0].min(axis=0)
    y1, x1 = near[0].max(axis=0)
    far_x = 0 if near[1][:, 1].min() > 4 else W - 1
    assert not (np.abs(near[1][:, 1] - far_x) <= 2).any()
    boxes = [np.array([[0, 0, 0, 0], [x1, y1, x0, y0]]), np.array([[far_x - 2, 0, far_x + 2, H - 1]])]
    want = ref.pipeline_f64(vm, gt, thresh, boxes)
    assert want["hits"].tolist() == [True, False]
    assert 0 < want["masks"].mean() < 0.5

    vm_d = torch.tensor(vm, device=DEV)
    before = vm_d.clone()
    got = lerf_eval.activate_stream(vm_d, torch.from_numpy(gt).to(DEV), thresh)
    loc = lerf_eval.lerf_localization(vm_d, boxes)
    assert torch.equal(vm_d, before), "valid_map is not modified"
    assert got["masks"].shape == (L, P, H, W) and got["masks"].dtype == torch.uint8
    np.testing.assert_array_equal(got["masks"].cpu().numpy(), want["masks"])
    np.testing.assert_array_equal(got["counts"].cpu().numpy(), want["counts"])
    np.testing.assert_array_equal(got["levels"].cpu().numpy(), want["levels"])
    np.testing.assert_array_equal(got["iou"].cpu().numpy(), want["iou"])
    assert got["iou"].dtype == torch.float64 and np.isfinite(want["iou"]).all() and (want["iou"] > 0).any()
    np.testing.assert_array_equal(loc["levels"], want["loc_levels"])
    np.testing.assert_array_equal(loc["hits"], want["hits"])
    assert loc["acc_num"] == 1
    for k in range(P):  # the kernel's coordinates are among the near-maximal pixels of the fp64 map
        assert loc["coords"][k].shape[1] == 2 and len(loc["coords"][k]) >= 1
        for x, y in loc["coords"][k]:
            assert [y, x] in near[k].tolist()
    # without ground truth: levels and masks only; a float ground truth and an empty union
    plain = lerf_eval.activate_stream(vm_d, thresh=thresh)
    assert sorted(plain) == ["levels", "masks"] and torch.equal(plain["masks"], got["masks"])
    empty = lerf_eval.activate_stream(torch.full((1, 1, H, W), 0.5, device=DEV), torch.zeros((1, H, W), device=DEV))
    assert np.isnan(empty["iou"].cpu().numpy()).all() and empty["counts"].cpu().numpy().tolist() == [[[0, 0]]]
    with pytest.raises(ValueError, match="box lists"):
        lerf_eval.lerf_localization(vm_d, boxes[:1])
    with pytest.raises(ValueError, match="gt_masks"):
        lerf_eval.activate_stream(vm_d, torch.zeros((P, H, W + 1), device=DEV))


def test_two_calls_are_bit_identical_and_streams_agree():
    c, _, a = _gpu_case(97, 61, 1)
    gt = (np.random.default_rng(3).random((1, 97, 61)) < 0.5).astype(np.uint8)

    def run():
        g = _run_filter(c["maps"])
        return g, _run_masks(g["dev"]["blend"], g["dev"]["stats"], 0.4, gt)

    b, mb = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s, ms = run()
    side.synchronize()
    for other in (b, s):
        for k in ("avg", "blend", "stats"):
            assert a[k].tobytes() == other[k].tobytes(), k
    for x, y in zip(mb, ms):
        np.testing.assert_array_equal(x, y)
    # without the optional outputs the rest is the same
    only_avg = _run_filter(c["maps"], with_blend=False)
    only_blend = _run_filter(c["maps"], with_avg=False)
    none = _run_filter(c["maps"], with_avg=False, with_blend=False)
    assert only_avg["avg"].tobytes() == a["avg"].tobytes() and only_blend["blend"].tobytes() == a["blend"].tobytes()
    for other in (only_avg, only_blend, none):
        assert other["stats"].tobytes() == a["stats"].tobytes()


def test_evaluate_frame_on_the_oracle_scene():
    """The oracle scene of test_gpu_query's render_relevancy test, rendered once and stacked into 3
    levels in the renders_npy (hwc) layout: evaluate_frame returns the documented keys and shapes and
    agrees with relevancy_map, activate_stream and lerf_localization called separately."""
    import bench
    from langsplat_amd.query import Decoder, relevancy_map, render_relevancy
    from langsplat_amd.synthetic import make_cameras, make_gaussians
    from tests import query_ref
    P_, W, H, n_pos, n_neg, L = 2000, 96, 64, 3, 4, 3
    g = make_gaussians(P_, seed=0, sh_degree=3, extent=1.0, scale_range=(0.02, 0.12))
    c = query_ref.make_case(query_ref.CANONICAL, 1, n_pos, n_neg, 7)
    dec = Decoder.from_arrays(c["weights"], c["biases"], device=DEV)
    pos, neg = torch.from_numpy(c["pos"]).to(DEV), torch.from_numpy(c["neg"]).to(DEV)
    model = bench.Model(g.to(DEV), include_feature=True)
    cam = make_cameras(1, W, H, device=DEV)[0]
    pkg = render_relevancy(cam, model, bench.Pipe, torch.zeros(3, device=DEV), bench.Opt, dec, pos, neg)
    img = pkg["language_feature_image"].permute(1, 2, 0)            # (H, W, 3)
    sem = torch.stack([img, img.flip(1), 0.5 * img]).contiguous()   # (L, H, W, 3)
    gt = torch.zeros((n_pos, H, W), dtype=torch.bool, device=DEV)
    gt[:, 16:48, 24:72] = True
    boxes = [np.array([[0, 0, W - 1, H - 1]]), np.array([[-5, -5, -1, -1]]), np.zeros((0, 4))]
    out = lerf_eval.evaluate_frame(sem, dec, pos, neg, gt, boxes)
    assert sorted(out) == sorted(["relevancy", "chosen_level", "masks", "iou", "iou_levels", "counts", "loc_level",
                                  "coords", "hits", "acc_num"])
    assert out["relevancy"].shape == (L, n_pos, H, W) and out["masks"].shape == (L, n_pos, H, W)
    assert out["chosen_level"].shape == (n_pos,) and out["iou"].shape == (n_pos,)
    assert out["iou_levels"].shape == (L, n_pos) and out["counts"].shape == (L, n_pos, 2)
    assert out["loc_level"].shape == (n_pos,) and len(out["coords"]) == n_pos
    assert out["hits"].tolist() == [True, False, False] and out["acc_num"] == 1
    vm = relevancy_map(sem, dec, pos, neg, layout="hwc")
    assert torch.equal(vm[:1], pkg["relevancy"]) and torch.equal(vm, out["relevancy"])
    a = lerf_eval.activate_stream(vm, gt, 0.4)
    loc = lerf_eval.lerf_localization(vm, boxes)
    assert torch.equal(a["levels"], out["chosen_level"]) and torch.equal(a["masks"], out["masks"])
    assert torch.equal(a["counts"], out["counts"])
    np.testing.assert_array_equal(a["iou"].cpu().numpy(), out["iou"].cpu().numpy())
    np.testing.assert_array_equal(loc["levels"], out["loc_level"])
    np.testing.assert_array_equal(loc["hits"], out["hits"])
    for x, y in zip(loc["coords"], out["coords"]):
        np.testing.assert_array_equal(x, y)
    s = lerf_eval.smooth_relevancy(vm)
    for k in range(n_pos):
        y, x = s["avg_argmax"][int(out["loc_level"][k]), k].tolist()
        assert out["coords"][k][0].tolist() == [x, y]  # the first coordinate is the first row-major arg-max
