"""GPU: the driver's own bench command prints ONE JSON line; with --full (the default extras: eval forward, roofline, PMC
summaries, CPU baseline) it carries every object the contract names.
(Round 3 never ran bench.py without --profile-steps 0 / --no-cpu-baseline on the final tree; the driver did, and it crashed.)"""
import json
import os
import subprocess
import sys

import pytest
import torch

from _util import ROOT

pytestmark = pytest.mark.gpu


def _run(extra):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"] + extra
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_the_drivers_default_bench_command_prints_its_line():
    rec = _run(["--full"])
    assert rec["metric"].startswith("images/sec fwd+bwd QuadtreeCNN") and rec["unit"] == "images/s"
    assert rec["n_gpus"] == 1 and rec["steps"] == 2 and rec["warmup"] == 1 and rec["value"] > 0
    assert rec["dtype"] == "bf16" and rec["config"]["per_gpu_batch"] == 256 and rec["vs_baseline"] is None
    roof = rec["roofline"]
    assert roof["bound"] == "mfma" and 0 < roof["frac"] < 1 and roof["unit"] == "TFLOP/s"
    assert "traffic" in roof and isinstance(roof["traffic_source"], str)
    cpu = rec["cpu_baseline"]
    assert cpu["value"] > 0 and cpu["cores"] >= 1 and cpu["kind"] == "port" and cpu["sample"]
    assert rec["forward"]["value"] > 0 and 0 < rec["forward"]["model_mfma_util"] < 1
    for key in ("hbm", "mfma_pmc"):   # read from profiles/: a number or a stated reason, never an error
        assert isinstance(rec[key], dict) and "error" not in rec[key]


def test_the_clip_model_line_also_prints():
    rec = _run(["--full", "--model", "quadtree3d", "--batch", "16", "--no-cpu-baseline"])
    assert rec["value"] > 0 and rec["roofline"]["frac"] > 0 and "traffic" in rec["roofline"]


def test_a_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """Without --full the line carries the timed steps only; --dump-outputs writes the last timed step's logits / loss and
    samples of the updated parameters, gradients and running statistics.  Two runs with the same arguments get the same
    inputs and compute the same step: their dumps are identical (every reduction of the step sums in a fixed order -- an
    order-dependent last bit of one gradient grows, through Adam, into differences far beyond rounding)."""
    import numpy as np
    from _util import rel_err
    recs, dumps = [], []
    for run in ("a", "b"):
        d = tmp_path / run
        rec = _run(["--steps", "3", "--dump-outputs", str(d)])
        recs.append(rec)
        dumps.append({f.stem: np.load(f) for f in sorted(d.glob("*.npy"))})
    rec, out = recs[0], dumps[0]
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["dtype"] == "bf16"
    assert rec["metric"].startswith("images/sec fwd+bwd QuadtreeCNN") and rec["higher_is_better"] is True
    assert abs(rec["value"] - 256e3 / rec["ms_per_step"]) <= 1e-3 * rec["value"] + 0.2
    assert rec["roofline"] is None and rec["forward"] is None and rec["hbm"] is None and rec["mfma_pmc"] is None
    assert "cpu_baseline" not in rec
    assert sorted(out) == ["buffers", "grads", "logits", "loss", "params"]
    assert out["logits"].shape == (256, 12) and out["loss"].shape == (1,)
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    for k, a in out.items():
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), k
    # the loss is the cross-entropy of the dumped logits against bench.py's labels (cuda generator seeded 1234)
    g = torch.Generator(device="cuda").manual_seed(1234)
    torch.randn(256, 3, 224, 224, device="cuda", generator=g)
    torch.randn(256, 47, device="cuda", generator=g)
    labels = torch.randint(0, 12, (256,), device="cuda", generator=g).cpu()
    ce = float(torch.nn.functional.cross_entropy(torch.from_numpy(out["logits"]), labels))
    assert abs(ce - float(out["loss"][0])) <= 1e-4 * abs(ce) + 1e-5, (ce, out["loss"])
    for k in out:
        assert out[k].shape == dumps[1][k].shape, k
        assert np.array_equal(dumps[1][k], out[k]), (k, rel_err(dumps[1][k], out[k]))
