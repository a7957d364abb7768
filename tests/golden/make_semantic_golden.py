"""Generate tests/golden/semantic.npz from the reference's own decoder and get_semantic_map.

Run on the build machine only, with a checkout of the reference (it is not needed to run the tests):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_semantic_golden.py <path to the reference>

Imports from the reference, as make_query_golden.py does:
  - autoencoder/model.py: Autoencoder (decode)
  - eval/openclip_encoder.py: OpenCLIPNetwork (get_semantic_map).  Its module imports open_clip and
    torchvision, which only its constructor uses: where they are not importable, empty stand-in modules
    are registered first, and the network object is created with __new__ and given only
    semantic_embeds and neg_embeds.
The decoder weights, phrases and pixels come from tests/query_ref.py's seeded generators.  The output is
a plain .npz data file: per configuration the seed, the 64 input pixels and get_semantic_map's int64
(1, 8, 8) output for them (1 level, the pixels viewed as 8 x 8).  The seeds are the first from 20250 on
for which the stored labels contain -1 and at least two different classes.
"""
import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from tests import query_ref  # noqa: E402

CONFIGS = {"canonical": dict(widths=query_ref.CANONICAL, n_labels=3, n_neg=4),
           "small": dict(widths=[16, 32, 32], n_labels=3, n_neg=4)}
FIRST_SEED = 20250
ENCODER_DIMS = [256, 128, 64, 32, 3]  # the reference's default encoder; only its last width matters here


def _import_reference(ref):
    for name in ("open_clip", "torchvision"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    sys.path.insert(0, os.path.join(ref, "autoencoder"))
    sys.path.insert(0, os.path.join(ref, "eval"))
    from model import Autoencoder
    from openclip_encoder import OpenCLIPNetwork
    return Autoencoder, OpenCLIPNetwork


def _reference_labels(Autoencoder, OpenCLIPNetwork, cfg, case):
    with contextlib.redirect_stdout(io.StringIO()):  # the constructor prints its module lists
        model = Autoencoder(ENCODER_DIMS, cfg["widths"])
    sd = model.state_dict()
    sd.update(query_ref.state_dict_of(case["weights"], case["biases"]))
    model.load_state_dict(sd)
    model.eval()
    net = OpenCLIPNetwork.__new__(OpenCLIPNetwork)
    net.semantic_embeds = torch.from_numpy(case["pos"])
    net.neg_embeds = torch.from_numpy(case["neg"])
    with torch.no_grad():
        decoded = model.decode(torch.from_numpy(case["pixels"]))            # (64, D)
        return net.get_semantic_map(decoded.view(1, 8, 8, -1))               # (1, 8, 8) int64


def main(ref):
    Autoencoder, OpenCLIPNetwork = _import_reference(ref)
    out = {}
    for name, cfg in CONFIGS.items():
        for seed in range(FIRST_SEED, FIRST_SEED + 100):
            case = query_ref.make_case(cfg["widths"], 64, cfg["n_labels"], cfg["n_neg"], seed)
            labels = _reference_labels(Autoencoder, OpenCLIPNetwork, cfg, case).numpy()
            if (labels == -1).any() and len(set(labels[labels >= 0].tolist())) >= 2:
                break
        else:
            raise SystemExit(f"{name}: no seed with -1 and two classes")
        assert labels.dtype == np.int64 and labels.shape == (1, 8, 8)
        out[f"{name}_seed"] = np.int64(seed)
        out[f"{name}_widths"] = np.asarray(cfg["widths"], np.int64)
        out[f"{name}_n_labels"] = np.int64(cfg["n_labels"])
        out[f"{name}_n_neg"] = np.int64(cfg["n_neg"])
        out[f"{name}_pixels"] = case["pixels"]
        out[f"{name}_labels"] = labels
        print(name, seed, np.unique(labels, return_counts=True))
    np.savez(os.path.join(OUT, "semantic.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
