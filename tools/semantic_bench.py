"""Open-vocabulary semantic map and label statistics: the fused kernels against torch compositions
(measurement aid; sibling of query_bench.py).

    python3 tools/semantic_bench.py [--out profiles/semantic_bench.json]

At 1920x1080 and 832x1264 (the reference's evaluation size), one level, 8 labels and 4 negatives, the
canonical decoder widths, on the same GPU in the same process and run, in this order:
  relevancy (round 1)  langsplat_amd.relevancy_map with the same 12 phrases (8 positives)
  semantic             langsplat_amd.semantic_map, dtype int32 (one lsr_query_semantic launch), without
                       and with the score
  relevancy (round 2)  again: the semantic kernel has the relevancy kernel's body, so its time should lie
                       within the two rounds' spread
  torch                Autoencoder.decode + OpenCLIPNetwork.get_semantic_map as torch ops (F.linear, relu,
                       x / x.norm, mm, softmax, argmax, the -1 assignment), chunked over pixels so that
                       the decoded map fits (CHUNK pixels per chunk)
  label_stats          langsplat_amd.label_stats over 3 maps and one shared ground truth, against a
                       torch composition: per map a bincount of gt * C + pred over the valid pixels whose
                       prediction is a class, and one of gt
Each: 5 warm-up calls, then the median of 20 calls timed with device events, and the peak-allocation
delta of one call.  Also the accuracy table of the parity cases of tests/test_gpu_semantic.py at 1000
pixels: wrong labels on decided pixels and the worst score error in units of e_score.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.query_bench import CALLS, CHUNK, WARMUP, measure  # noqa: E402

N_LABELS, N_NEG, STAT_MAPS = 8, 4, 3


def torch_semantic(sem, weights, biases, labels, neg):
    """(1, 3, H, W) -> (1, H, W) int64: the reference's ops, chunked over pixels."""
    import torch
    import torch.nn.functional as F
    _, _, H, W = sem.shape
    pix = sem[0].reshape(3, H * W).t()
    pos_num = labels.shape[0]
    p = torch.cat([labels, neg], dim=0)
    out = torch.zeros(H * W, device=sem.device)
    for s in range(0, H * W, CHUNK):
        x = pix[s:s + CHUNK]
        for i, (w, b) in enumerate(zip(weights, biases)):
            if i > 0:
                x = F.relu(x)
            x = F.linear(x, w, b)
        x = x / x.norm(dim=-1, keepdim=True)
        softmax = torch.softmax(10 * torch.mm(x, p.T), dim=-1)
        out[s:s + CHUNK] = torch.argmax(softmax, dim=-1)
    out[out >= pos_num] = -1
    return out.long().view(1, H, W)


def torch_label_stats(pred, gt, C):
    """pred (maps, N), gt (N,) -> (counts (maps, C, 3), totals (maps, 2)) with bincounts."""
    import torch
    valid = (gt >= 0) & (gt < C)
    g = gt[valid].long()
    truth = torch.bincount(g, minlength=C)
    counts, totals = [], []
    for m in range(pred.shape[0]):
        p = pred[m][valid].long()
        cls = (p >= 0) & (p < C)
        conf = torch.bincount(g[cls] * C + p[cls], minlength=C * C).view(C, C)
        inter = conf.diagonal()
        counts.append(torch.stack([inter, conf.sum(dim=0), truth], dim=1))
        totals.append(torch.stack([inter.sum(), valid.sum()]))
    return torch.stack(counts), torch.stack(totals)


def accuracy_table():
    import numpy as np
    import torch
    from langsplat_amd import query
    from tests import query_ref, semantic_ref
    rows = []
    for widths in (query_ref.CANONICAL, [16, 32, 32], [16]):
        for n_labels, n_neg in ((1, 1), (3, 4), (17, 4), (28, 4), (29, 4), (60, 4)):
            c = semantic_ref.references(widths, 1000, n_labels, n_neg)
            dec = query.Decoder.from_arrays(c["weights"], c["biases"], device="cuda")
            sem = torch.from_numpy(c["pixels"]).cuda().view(1, 25, 40, 3)
            lab, score = query.semantic_map(sem, dec, torch.from_numpy(c["pos"]).cuda(), torch.from_numpy(c["neg"]).cuda(),
                                            layout="hwc", return_score=True)
            lab, score = lab.cpu().numpy().reshape(-1), score.cpu().numpy().reshape(-1).astype(np.float64)
            e_sim, e_score, decided = semantic_ref.yardsticks(c, 1000)
            rows.append({"widths": list(widths), "n_labels": n_labels, "n_neg": n_neg, "seed": semantic_ref.case_seed(widths, n_labels),
                         "pixels": 1000, "undecided": int((~decided).sum()),
                         "wrong_labels_on_decided": int((lab[decided] != c["label64"][decided]).sum()),
                         "wrong_labels_fp32_reference": int((c["label32"][decided] != c["label64"][decided]).sum()),
                         "labels_differing_anywhere": int((lab != c["label64"]).sum()),
                         "smallest_gap": float(c["gap"].min()), "e_sim": e_sim, "e_score": e_score,
                         "score_error": float(np.abs(score - c["score64"]).max()),
                         "score_error_in_e_score": round(float(np.abs(score - c["score64"]).max()) / e_score, 3)})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semantic_bench.json"))
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from langsplat_amd.query import Decoder, label_stats, relevancy_map, semantic_map
    from tests import query_ref
    dev = torch.device("cuda", 0)
    rows = []
    for (W, H) in ((1920, 1080), (832, 1264)):
        c = query_ref.make_case(query_ref.CANONICAL, 1, N_LABELS, N_NEG, seed=7)
        dec = Decoder.from_arrays(c["weights"], c["biases"], device=dev)
        ws = [torch.from_numpy(w).to(dev) for w in c["weights"]]
        bs = [torch.from_numpy(b).to(dev) for b in c["biases"]]
        lab, neg = torch.from_numpy(c["pos"]).to(dev), torch.from_numpy(c["neg"]).to(dev)
        gen = torch.Generator().manual_seed(3)
        sem = (torch.nn.functional.normalize(torch.randn((1, 3, H, W), generator=gen), dim=1)
               * torch.rand((1, 1, H, W), generator=gen)).to(dev)
        with torch.no_grad():
            r1 = measure(lambda: relevancy_map(sem, dec, lab, neg))
            s0 = measure(lambda: semantic_map(sem, dec, lab, neg, dtype=torch.int32))
            s1 = measure(lambda: semantic_map(sem, dec, lab, neg, return_score=True, dtype=torch.int32))
            r2 = measure(lambda: relevancy_map(sem, dec, lab, neg))
            t = measure(lambda: torch_semantic(sem, ws, bs, lab, neg))
        differ = int((s0[3].long() != t[3]).sum())
        assert torch.equal(s0[3], s1[3][0]) and torch.equal(r1[3], r2[3])
        macs = sum(a * b for a, b in zip([3] + query_ref.CANONICAL[:-1], query_ref.CANONICAL)) + 512 * (N_LABELS + N_NEG)
        row = {"what": "semantic_map", "width": W, "height": H, "n_labels": N_LABELS, "n_neg": N_NEG,
               "widths": query_ref.CANONICAL, "warmup": WARMUP, "calls": CALLS, "torch_chunk_pixels": CHUNK,
               "relevancy_round1_ms_median": round(r1[0], 4), "relevancy_round1_ms_min": round(r1[1], 4),
               "semantic_ms_median": round(s0[0], 4), "semantic_ms_min": round(s0[1], 4),
               "semantic_score_ms_median": round(s1[0], 4), "semantic_score_ms_min": round(s1[1], 4),
               "relevancy_round2_ms_median": round(r2[0], 4), "relevancy_round2_ms_min": round(r2[1], 4),
               "torch_ms_median": round(t[0], 4), "torch_ms_min": round(t[1], 4),
               "relevancy_peak_bytes": int(r1[2]), "semantic_peak_bytes": int(s0[2]),
               "semantic_score_peak_bytes": int(s1[2]), "torch_peak_bytes": int(t[2]),
               "semantic_tflops": round(2.0 * macs * W * H / (s0[0] * 1e-3) / 1e12, 2),
               "labels_differing_from_torch": differ,
               "label_minus_one_share": round(float((s0[3] == -1).float().mean()), 4)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        # label statistics: the level's map and two perturbed copies against a ground truth made from it
        N = H * W
        g = torch.Generator().manual_seed(5)
        base = s0[3].reshape(N).cpu()
        pred = torch.stack([base] + [torch.where(torch.rand(N, generator=g) < 0.2,
                                                 torch.randint(-1, N_LABELS, (N,), generator=g, dtype=torch.int32), base)
                                     for _ in range(STAT_MAPS - 1)]).to(dev).view(STAT_MAPS, H, W)
        gt = torch.where(torch.rand(N, generator=g) < 0.3, torch.randint(0, N_LABELS, (N,), generator=g, dtype=torch.int32),
                         base)
        gt = torch.where(torch.rand(N, generator=g) < 0.05, torch.full_like(gt, 255), gt).to(dev).view(H, W)
        with torch.no_grad():
            f = measure(lambda: label_stats(pred, gt, N_LABELS))
            k = measure(lambda: (label_stats(pred, gt, N_LABELS)["counts"]))  # the same call: a second round
            tt = measure(lambda: torch_label_stats(pred.view(STAT_MAPS, N), gt.view(N), N_LABELS))
        same = bool(torch.equal(f[3]["counts"], tt[3][0]) and torch.equal(f[3]["totals"], tt[3][1]))
        row = {"what": "label_stats", "width": W, "height": H, "maps": STAT_MAPS, "n_classes": N_LABELS,
               "fused_ms_median": round(f[0], 4), "fused_ms_min": round(f[1], 4),
               "fused_round2_ms_median": round(k[0], 4),
               "torch_ms_median": round(tt[0], 4), "torch_ms_min": round(tt[1], 4),
               "fused_peak_bytes": int(f[2]), "torch_peak_bytes": int(tt[2]), "counts_equal_torch": same,
               "valid_share": round(float(f[3]["totals"][0, 1]) / N, 4),
               "miou": [round(float(v), 4) for v in f[3]["miou"]]}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del sem, r1, r2, s0, s1, t
    acc = accuracy_table()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows, "accuracy": acc}, fh, indent=1)
        fh.write("\n")
    assert np.isfinite([r.get("semantic_ms_median", r.get("fused_ms_median")) for r in rows]).all()


if __name__ == "__main__":
    main()
