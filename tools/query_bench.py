"""Open-vocabulary query: the fused kernel against the reference's op sequence in torch (measurement aid).

    python3 tools/query_bench.py [--out profiles/query_bench.json]

At 1920x1080 and 832x1264 (the reference's evaluation size), one level, n_pos = 1 and 8, 4 negatives,
the canonical decoder widths, on the same GPU in the same run:
  fused   langsplat_amd.relevancy_map (one lsr_query_relevancy launch)
  torch   Autoencoder.decode + OpenCLIPNetwork.get_max_across as torch ops (F.linear, relu, x / x.norm,
          mm, stack, softmax, argmin, gather: the restatement of tests/query_ref.py, every positive
          batched), chunked over pixels so that the decoded map fits (CHUNK pixels per chunk, 256 MB
          of decoded vectors)
Each: 5 warm-up calls, then the median of 20 calls timed with device events, and the peak-allocation
delta of one call.  Also reports the largest difference between the two results.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 131072
WARMUP, CALLS = 5, 20


def torch_composition(sem, weights, biases, pos, neg):
    """(1, 3, H, W) -> (1, n_pos, H, W): the reference's ops, chunked over pixels."""
    import torch
    import torch.nn.functional as F
    from tests import query_ref
    _, _, H, W = sem.shape
    pix = sem[0].reshape(3, H * W).t()
    n_pos = pos.shape[0]
    p = torch.cat([pos, neg], dim=0)
    out = torch.empty((n_pos, H * W), dtype=torch.float32, device=sem.device)
    for s in range(0, H * W, CHUNK):
        x = pix[s:s + CHUNK]
        for i, (w, b) in enumerate(zip(weights, biases)):
            if i > 0:
                x = F.relu(x)
            x = F.linear(x, w, b)
        x = x / x.norm(dim=-1, keepdim=True)
        out[:, s:s + CHUNK] = query_ref.relevancy_from_decoded_torch32(x, p, n_pos)
    return out.view(1, n_pos, H, W)


def measure(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return statistics.median(times), min(times), peak, r


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_bench.json"))
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from langsplat_amd.query import Decoder, relevancy_map
    from tests import query_ref
    dev = torch.device("cuda", 0)
    rows = []
    for (W, H) in ((1920, 1080), (832, 1264)):
        for n_pos in (1, 8):
            c = query_ref.make_case(query_ref.CANONICAL, 1, n_pos, 4, seed=7)
            dec = Decoder.from_arrays(c["weights"], c["biases"], device=dev)
            ws = [torch.from_numpy(w).to(dev) for w in c["weights"]]
            bs = [torch.from_numpy(b).to(dev) for b in c["biases"]]
            pos, neg = torch.from_numpy(c["pos"]).to(dev), torch.from_numpy(c["neg"]).to(dev)
            gen = torch.Generator().manual_seed(3)
            sem = (torch.nn.functional.normalize(torch.randn((1, 3, H, W), generator=gen), dim=1)
                   * torch.rand((1, 1, H, W), generator=gen)).to(dev)
            with torch.no_grad():
                f_med, f_min, f_peak, f_out = measure(lambda: relevancy_map(sem, dec, pos, neg))
                t_med, t_min, t_peak, t_out = measure(lambda: torch_composition(sem, ws, bs, pos, neg))
            diff = float((f_out - t_out).abs().max())
            macs = sum(a * b for a, b in zip([3] + query_ref.CANONICAL[:-1], query_ref.CANONICAL)) + 512 * (n_pos + 4)
            row = {"width": W, "height": H, "n_pos": n_pos, "n_neg": 4, "widths": query_ref.CANONICAL,
                   "fused_ms_median": round(f_med, 4), "fused_ms_min": round(f_min, 4),
                   "torch_ms_median": round(t_med, 4), "torch_ms_min": round(t_min, 4),
                   "fused_peak_bytes": int(f_peak), "torch_peak_bytes": int(t_peak),
                   "fused_tflops": round(2.0 * macs * W * H / (f_med * 1e-3) / 1e12, 2),
                   "torch_chunk_pixels": CHUNK, "max_abs_diff": diff, "warmup": WARMUP, "calls": CALLS}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del sem, f_out, t_out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        f.write("\n")
    assert np.isfinite([r["fused_ms_median"] for r in rows]).all()


if __name__ == "__main__":
    main()
