"""CPU references of the open-vocabulary query (decode + relevancy) and the generators of its test inputs.

Two restatements of eval/evaluate_iou_loc.py:258-266 -- Autoencoder.decode (autoencoder/model.py:42-46)
followed by OpenCLIPNetwork.get_max_across / get_relevancy (eval/openclip_encoder.py:42-56, 96-112):

  *_f64      numpy float64, the relevancy written out: min over negatives of 1 / (1 + exp(10 (s_n - s_j)))
  *_torch32  torch float32 following the reference's op sequence literally (F.linear, relu, x / x.norm,
             mm, stack, softmax(10 .), argmin, gather), every positive batched

max |torch32 - f64| on a test's own inputs is the yardstick e_ref of the GPU tests: the error the
reference's own fp32 evaluation has, independent of the kernel under test.

Test decoders are generated, not stored: W ~ N(0, 2 / fan_in), b ~ N(0, 0.1^2), cast to fp32; phrases are
random unit rows; pixel features are random directions scaled by U(0, 1).
"""
import numpy as np
import torch
import torch.nn.functional as F

CANONICAL = [16, 32, 64, 128, 256, 256, 512]  # the reference's decoder_hidden_dims (autoencoder/train.py)


def make_decoder(widths, rng):
    weights, biases, fan_in = [], [], 3
    for out in widths:
        weights.append(rng.normal(0.0, np.sqrt(2.0 / fan_in), (out, fan_in)).astype(np.float32))
        biases.append(rng.normal(0.0, 0.1, (out,)).astype(np.float32))
        fan_in = out
    return weights, biases


def unit_rows(n, dim, rng):
    x = rng.normal(size=(n, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def make_pixels(n, rng):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * rng.uniform(0.0, 1.0, (n, 1))).astype(np.float32)


def make_case(widths, n, n_pos, n_neg, seed):
    """One seeded test case: decoder, phrases (positives first) and (n, 3) pixel features."""
    rng = np.random.default_rng(seed)
    weights, biases = make_decoder(widths, rng)
    pos = unit_rows(n_pos, widths[-1], rng)
    neg = unit_rows(n_neg, widths[-1], rng)
    return dict(weights=weights, biases=biases, pos=pos, neg=neg, pixels=make_pixels(n, rng))


def state_dict_of(weights, biases):
    """The reference checkpoint's decoder keys (Linears at the even ModuleList indices)."""
    sd = {}
    for i, (w, b) in enumerate(zip(weights, biases)):
        sd[f"decoder.{2 * i}.weight"] = torch.from_numpy(w)
        sd[f"decoder.{2 * i}.bias"] = torch.from_numpy(b)
    return sd


def decode_f64(pixels, weights, biases):
    x = np.asarray(pixels, np.float64)
    for i, (w, b) in enumerate(zip(weights, biases)):
        if i > 0:
            x = np.maximum(x, 0.0)
        x = x @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def relevancy_f64(pixels, weights, biases, pos, neg):
    """(n_pos, N) float64."""
    y = decode_f64(pixels, weights, biases)
    sp = y @ np.asarray(pos, np.float64).T   # (N, n_pos)
    sn = y @ np.asarray(neg, np.float64).T   # (N, n_neg)
    r = 1.0 / (1.0 + np.exp(10.0 * (sn[:, None, :] - sp[:, :, None])))  # (N, n_pos, n_neg)
    return r.min(axis=2).T


def decode_torch32(pixels, weights, biases):
    x = torch.from_numpy(np.ascontiguousarray(pixels, np.float32))
    for i, (w, b) in enumerate(zip(weights, biases)):
        if i > 0:
            x = F.relu(x)
        x = F.linear(x, torch.from_numpy(w), torch.from_numpy(b))
    return x / x.norm(dim=-1, keepdim=True)


def relevancy_from_decoded_torch32(decoded, phrases, n_pos):
    """The reference's relevancy step as torch fp32 ops, all positives at once: decoded (N, D) unit
    rows, phrases (n_pos + n_neg, D) with the positives first -> (n_pos, N).

    Same op sequence as get_relevancy (mm, stack, softmax(10 .), argmin, gather), batched: the
    (positive, negative) similarity pairs form an (N, n_pos, n_neg, 2) tensor, the softmax runs over
    the pair, and per pixel and positive the pair whose positive probability is smallest is gathered
    along the negative axis."""
    cos = torch.mm(decoded, phrases.to(decoded.dtype).T)                       # (N, n_pos + n_neg)
    n_neg = cos.shape[1] - n_pos
    pos_side = cos[:, :n_pos, None].expand(-1, -1, n_neg)
    neg_side = cos[:, None, n_pos:].expand(-1, n_pos, -1)
    pair_prob = torch.softmax(10 * torch.stack((pos_side, neg_side), dim=-1), dim=-1)
    worst = pair_prob[..., 0].argmin(dim=2)                                     # (N, n_pos)
    picked = torch.gather(pair_prob, 2, worst[:, :, None, None].expand(-1, -1, 1, 2))
    return picked[:, :, 0, 0].T


def relevancy_torch32(pixels, weights, biases, pos, neg):
    """(n_pos, N) float32 tensor."""
    phrases = torch.cat([torch.from_numpy(pos), torch.from_numpy(neg)], dim=0)
    return relevancy_from_decoded_torch32(decode_torch32(pixels, weights, biases), phrases, len(pos))


_REFS = {}


def references(widths, n, n_pos, n_neg, seed):
    """The case with its references, computed once and shared (treat as read-only):
    rel64 (n_pos, N), dec64 (N, D), the fp32 restatement's rel32 and dec32, e_rel and e_dec = max
    |torch32 - f64| over all N pixels."""
    key = (tuple(widths), n, n_pos, n_neg, seed)
    if key not in _REFS:
        c = make_case(widths, n, n_pos, n_neg, seed)
        c["rel64"] = relevancy_f64(c["pixels"], c["weights"], c["biases"], c["pos"], c["neg"])
        c["dec64"] = decode_f64(c["pixels"], c["weights"], c["biases"])
        rel32 = relevancy_torch32(c["pixels"], c["weights"], c["biases"], c["pos"], c["neg"]).numpy()
        dec32 = decode_torch32(c["pixels"], c["weights"], c["biases"]).numpy()
        c["rel32"], c["dec32"] = rel32, dec32
        c["e_rel"] = float(np.abs(rel32.astype(np.float64) - c["rel64"]).max())
        c["e_dec"] = float(np.abs(dec32.astype(np.float64) - c["dec64"]).max())
        _REFS[key] = c
    return _REFS[key]
