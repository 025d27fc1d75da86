"""bench.py's plain run on the GPU: the result line, and --dump-outputs.

One small run (2 commits, Ne=24, Nc=10, 4 timed steps after 1 warm-up step) in a child
process: the plain line carries the headline fields and none of the --full side
measurements, and DIR/<name>.npy holds what the last timed training step left a caller
(the pair probabilities, the stats row, the updated parameters), i.e. the state of an
Engine stepped warm-up + steps times from the same seeds.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from hdgnn import layout
from hdgnn.synth import seed_for, synth_commits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_line_and_dumped_outputs(tmp_path):
    from hdgnn.engine import Engine
    B, ne, nc, steps, warm = 2, 24, 10, 4, 1
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    d = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
           "--warmup", str(warm), "--batch", str(B), "--ne", str(ne), "--nc", str(nc),
           "--dump-outputs", str(d)]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == warm and line["dtype"] == "f32"
    assert line["unit"] == "commits/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0
    np.testing.assert_allclose(line["value"], B / (line["ms_per_step"] * 1e-3), rtol=1e-3)
    for k in ("steady_state", "roofline", "cpu_baseline", "kernels_ms", "e2e",
              "upload_prepare_ms"):
        assert k not in line, k                    # side measurements: --full only

    assert sorted(os.listdir(d)) == ["params.npy", "probs.npy", "stats.npy"]
    got = {k: np.load(d / (k + ".npy")) for k in ("params", "probs", "stats")}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["probs"].shape == (B, 2, nc * (nc - 1))
    # the same steps in this process: same seeds, same kernels, so the same bits
    eng = Engine(ne, nc, B)
    eng.set_params(layout.init_flat(0, 2))
    db = eng.upload(synth_commits(B, ne, nc, seed_for(1, 0)))
    for _ in range(warm + steps):
        eng.train_step(db)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got["params"], eng.get_params())
    np.testing.assert_array_equal(got["probs"], eng.probs.cpu().numpy())
    np.testing.assert_array_equal(got["stats"], eng.stats.cpu().numpy())
    assert all(np.isfinite(a).all() for a in got.values())
