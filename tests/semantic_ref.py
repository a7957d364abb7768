"""CPU references of the open-vocabulary semantic map (decode + get_semantic_map) and of the label counts.

Two restatements of OpenCLIPNetwork.get_semantic_map (eval/openclip_encoder.py:82-94) on
Autoencoder.decode's output, over tests/query_ref.py's generators and decoders:

  semantic_f64      numpy float64 on query_ref.decode_f64: the similarities, the label (the first index of
                    the largest softmax value, -1 from n_labels on) and the winner's softmax value
  semantic_torch32  torch float32 with the reference's literal op sequence: mm, softmax(10 .), argmax, the
                    >= pos_num -> -1 assignment on a float tensor, .long()

The GPU tests' yardsticks are the fp32 restatement's own errors against fp64 on a case's inputs:
e_sim for the similarities, e_score for the winner's softmax value.  A pixel is DECIDED when the fp64
gap between its two largest similarities exceeds 8 e_sim; only there is a label a property of the
inputs and not of the rounding.
"""
import numpy as np
import torch

from tests import query_ref


def semantic_from_decoded_f64(decoded, phrases, n_labels):
    """decoded (N, D) float64 unit rows -> (sims (N, K), label (N,) int64, score (N,))."""
    s = np.asarray(decoded, np.float64) @ np.asarray(phrases, np.float64).T
    z = 10.0 * s
    prob = np.exp(z - z.max(axis=1, keepdims=True))
    prob /= prob.sum(axis=1, keepdims=True)
    idx = prob.argmax(axis=1)
    score = prob[np.arange(len(idx)), idx]
    return s, np.where(idx >= n_labels, -1, idx).astype(np.int64), score


def semantic_f64(pixels, weights, biases, labels, neg):
    phrases = np.concatenate([labels, neg])
    return semantic_from_decoded_f64(query_ref.decode_f64(pixels, weights, biases), phrases, len(labels))


def semantic_from_decoded_torch32(decoded, phrases, n_labels):
    """The reference's get_semantic_map for one level, op for op: decoded (N, D) fp32 tensor ->
    (sims (N, K), label (N,) int64, score (N,)); the score is the softmax value the argmax picked."""
    output = torch.mm(decoded, phrases.to(decoded.dtype).T)
    softmax = torch.softmax(10 * output, dim=-1)
    sem_pred = torch.zeros(decoded.shape[0])
    sem_pred[:] = torch.argmax(softmax, dim=-1)
    score = softmax.gather(1, torch.argmax(softmax, dim=-1)[:, None])[:, 0]
    sem_pred[sem_pred >= n_labels] = -1
    return output, sem_pred.long(), score


def semantic_torch32(pixels, weights, biases, labels, neg):
    phrases = torch.cat([torch.from_numpy(labels), torch.from_numpy(neg)], dim=0)
    return semantic_from_decoded_torch32(query_ref.decode_torch32(pixels, weights, biases), phrases, len(labels))


def top_gap(sims):
    """(N,) gap between the two largest similarities of each pixel (inf with a single phrase)."""
    if sims.shape[1] < 2:
        return np.full(sims.shape[0], np.inf)
    top = np.sort(sims, axis=1)[:, -2:]
    return top[:, 1] - top[:, 0]


SEED0 = 20240  # a case's seed is SEED0 + n_labels ...
# ... except where that seed's 1000 pixels never pick a negative although the set has several phrases
# per side: the canonical decoder with 28 labels (seed 20268 gives no -1; 30268 gives 419)
SEED_CHANGED = {(tuple(query_ref.CANONICAL), 28): 30268}
# sets whose labels hold no -1 and are left so: 16-32-32 with 60 labels, the canonical decoder with 1 + 1 phrases
NO_NEGATIVE = {((16, 32, 32), 60), (tuple(query_ref.CANONICAL), 1)}
_REFS = {}


def case_seed(widths, n_labels):
    return SEED_CHANGED.get((tuple(widths), n_labels), SEED0 + n_labels)


def references(widths, n, n_labels, n_neg, seed=None):
    """query_ref.make_case(widths, n, n_labels, n_neg, seed) with its references, computed once and
    shared (treat as read-only): sims64 (n, K), label64, score64; the fp32 restatement's sims32,
    label32, score32; gap (n,), the fp64 gap between the two largest similarities."""
    seed = case_seed(widths, n_labels) if seed is None else seed
    key = (tuple(widths), n, n_labels, n_neg, seed)
    if key not in _REFS:
        c = query_ref.make_case(widths, n, n_labels, n_neg, seed)
        args = (c["pixels"], c["weights"], c["biases"], c["pos"], c["neg"])
        c["sims64"], c["label64"], c["score64"] = semantic_f64(*args)
        s32, l32, p32 = semantic_torch32(*args)
        c["sims32"], c["label32"], c["score32"] = s32.numpy(), l32.numpy(), p32.numpy()
        c["gap"] = top_gap(c["sims64"])
        _REFS[key] = c
    return _REFS[key]


def yardsticks(c, N):
    """(e_sim, e_score, decided) over the case's first N pixels; N = 1 takes the errors over the whole
    set, since a maximum over a single pixel is no yardstick (tests/test_gpu_query.py's rule)."""
    M = N if N > 1 else c["sims64"].shape[0]
    e_sim = float(np.abs(c["sims32"][:M].astype(np.float64) - c["sims64"][:M]).max())
    e_score = float(np.abs(c["score32"][:M].astype(np.float64) - c["score64"][:M]).max())
    return e_sim, e_score, c["gap"][:N] > 8 * e_sim


def label_counts(pred, gt, n_classes):
    """numpy restatement of lsr_label_stats: pred (maps, N), gt (1 or maps, N) ->
    (counts (maps, n_classes, 3) = intersection, predicted, ground truth; totals (maps, 2) = correct, valid)."""
    pred, gt = np.asarray(pred, np.int64), np.asarray(gt, np.int64)
    maps = pred.shape[0]
    counts = np.zeros((maps, n_classes, 3), np.int64)
    totals = np.zeros((maps, 2), np.int64)
    for m in range(maps):
        g = gt[m if gt.shape[0] > 1 else 0]
        p = pred[m]
        valid = (g >= 0) & (g < n_classes)
        counts[m, :, 0] = np.bincount(g[valid & (p == g)], minlength=n_classes)
        counts[m, :, 1] = np.bincount(p[valid & (p >= 0) & (p < n_classes)], minlength=n_classes)
        counts[m, :, 2] = np.bincount(g[valid], minlength=n_classes)
        totals[m] = np.count_nonzero(valid & (p == g)), np.count_nonzero(valid)
    return counts, totals
