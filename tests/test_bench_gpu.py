"""A plain `python bench.py --steps N --warmup W` run: exactly N timed steps, the side measurements (--full) left out, and
--dump-outputs writing the block records of the last timed step -- the same arrays from two runs with the same arguments."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(extra):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "SPANGPU_BENCH_SPAWN", "SPANGPU_BENCH_FORCE_GATHER"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + extra, env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def load_dump(d):
    return {os.path.basename(f)[:-4]: np.load(f) for f in sorted(glob.glob(os.path.join(d, "*.npy")))}


def test_plain_run_times_exactly_steps_and_dumps_the_same_outputs_twice(built, tmp_path):
    args = ["--steps", "23", "--warmup", "5", "--channels", "16384"]
    dumps = []
    for name in ("a", "b"):
        r = run_bench(args + ["--dump-outputs", str(tmp_path / name)])
        assert r["steps"] == 23 and r["timed_steps"] == 23 and r["warmup"] == 5
        assert r["ms_per_step"] > 0 and abs(r["ms_per_step"] - r["timed_region_ms"]/23) < 1e-9
        assert r["value"] > 0 and r["unit"] == "Msamples/s" and r["higher_is_better"] is True
        for k in ("roofline", "roofline_valu", "cpu_baseline", "e2e", "e2e_g711", "paths", "large_bank", "frames_per_launch"):
            assert r[k] is None, k
        dumps.append(load_dump(str(tmp_path / name)))
    a, b = dumps
    assert set(a) == {"blocks_channel", "blocks_block", "blocks_hit", "blocks_code", "blocks_flags", "blocks_duration",
                      "blocks_energy"}
    n = len(a["blocks_channel"])
    assert n >= 16384                       # every channel completes at least one 102-sample block in a 160-sample frame
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k, v in a.items():
        assert v.dtype in (np.float32, np.float64) and v.shape == (n,), k
        assert np.array_equal(v, b[k]), k
    assert np.all(np.diff(a["blocks_channel"]) >= 0) and a["blocks_channel"][-1] == 16383
