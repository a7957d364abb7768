"""bench.py as a command: a plain run times the headline form alone and prints one JSON line;
--dump-outputs writes the last timed step's loss; --full adds the side figures.  At C1 (BASELINE.json
configs[0]: 10k Gaussians, 400x300) with a few steps: the command's structure, not its timings."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("ms_per_step_eager", "ms_per_step_all_gradients", "ms_forward_only", "ms_per_step_with_sync",
             "pipelined_graph_reps_ms", "ms_per_step_rgb", "stages_ms_per_step", "roofline", "cpu_baseline")


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C1", *args],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_the_headline_form_and_dumps_its_loss(tmp_path):
    out = tmp_path / "dump"
    d = _bench("--steps", "6", "--warmup", "2", "--dump-outputs", str(out))
    assert all(k in d for k in HEADLINE) and not any(k in d for k in FULL_ONLY)
    assert d["steps"] == 6 and d["warmup"] == 2 and d["full"] is False
    assert d["unit"] == "blends/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    # one form timed, and `value` is its rate
    forms = {k: v for k, v in d["ms_per_step_forms"].items() if v is not None}
    assert forms == {"pipelined_graph": d["ms_per_step"]} and d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["blends_per_step"] / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    assert sorted(os.listdir(out)) == ["loss.npy"]
    loss = np.load(out / "loss.npy")
    assert loss.dtype == np.float32 and loss.size == 1 and np.isfinite(loss).all() and float(loss) > 0.0


def test_full_run_adds_the_side_figures(tmp_path):
    d = _bench("--steps", "4", "--warmup", "1", "--full", "--dump-outputs", str(tmp_path / "dump"))
    assert all(k in d for k in HEADLINE + FULL_ONLY) and d["full"] is True and d["steps"] == 4
    forms = d["ms_per_step_forms"]
    assert all(forms[k] is not None for k in ("eager", "pipelined", "pipelined_graph"))
    assert d["ms_per_step"] == min(forms.values())
    assert d["cpu_baseline"]["value"] > 0 and d["stages_ms_per_step"]["render backward"] > 0
    assert np.load(tmp_path / "dump" / "loss.npy").dtype == np.float32
