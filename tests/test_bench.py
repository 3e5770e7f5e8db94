"""GPU: the benchmark's own contract -- a plain run times exactly --steps steps and reports ms_per_step without the
extras, and --dump-outputs writes what the last timed step computed, identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args), env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


def _load(d):
    return {name: np.load(os.path.join(d, name + ".npy")) for name in ("residuals", "x_sample", "x_sample_index")}


def test_plain_bench_times_the_steps_and_dumps_reproducible_outputs(tmp_path):
    outs = []
    for i in range(2):
        d = str(tmp_path / ("run%d" % i))
        line = _bench("--grid", "40", "--steps", "3", "--warmup", "2", "--dump-outputs", d)
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["unit"] == "V-cycle iterations/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
        assert line["roofline"] is None and line["cpu_baseline"] is None          # the extras are --full's
        o = _load(d)
        assert all(a.dtype == np.float64 for a in o.values())
        assert o["residuals"][-1] == line["config"]["residuals"][-1]
        assert np.array_equal(o["x_sample_index"], np.arange(40 ** 3))          # small enough: the whole iterate
        assert np.all(np.isfinite(o["x_sample"])) and np.any(o["x_sample"] != 0)
        outs.append(o)
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


def test_dump_outputs_samples_a_large_iterate(tmp_path):
    d = str(tmp_path / "dump")
    _bench("--grid", "130", "--steps", "2", "--warmup", "1", "--dump-outputs", d)
    o = _load(d)
    idx = o["x_sample_index"]
    assert 0 < len(idx) <= 1 << 21 and len(o["x_sample"]) == len(idx)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 130 ** 3
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
