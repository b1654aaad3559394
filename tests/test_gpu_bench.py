"""-m gpu: bench.py's command line at a small size (m = 20 000): the plain result line, `--dump-outputs`, and what `--steps` /
`--warmup` count.  The restart state and every seed are fixed, so the vector after w + s iterations depends on w + s alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 20000


def _bench(out, steps, warmup, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--m", str(M), "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(out)]
    res = subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = res.stdout.splitlines()
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench")
    return {"a": _bench(d / "a", 3, 2), "a2": _bench(d / "a2", 3, 2), "b": _bench(d / "b", 4, 1)}


def test_plain_result_line(runs):
    r, _ = runs["a"]
    assert r["metric"] == "fri_iterations_per_s" and r["unit"] == "iterations/s" and r["higher_is_better"] is True and r["dtype"] == "f64"
    assert r["steps"] == 3 and r["warmup"] == 2 and r["n_gpus"] == 1
    assert r["ms_per_step"] > 0 and abs(r["value"] * r["ms_per_step"] - 1e3) < 1e-6 * 1e3
    for k in ("roofline", "cpu_baseline", "parity", "top_kernels", "config4"):      # these take runs of their own: --full
        assert k not in r, k


def test_dumped_outputs_are_the_vector_of_the_last_step(runs):
    _, out = runs["a"]
    assert sorted(out) == ["dets", "vals", "vec_info"]
    assert out["vals"].dtype == np.float64 and out["dets"].dtype == np.float64 and out["vec_info"].dtype == np.float64
    curr_size, n_nonz, _ = out["vec_info"]
    assert out["vals"].shape == out["dets"].shape == (int(curr_size),)
    assert int(np.count_nonzero(out["vals"])) == int(n_nonz) and 0 < n_nonz <= M
    d = out["dets"].astype(np.uint64)
    assert np.array_equal(d.astype(np.float64), out["dets"])
    nz = d[out["vals"] != 0]
    assert np.unique(nz).size == nz.size                                 # one slot per determinant
    pop = np.zeros(nz.size, dtype=np.int64)
    for o in range(52):
        pop += ((nz >> np.uint64(o)) & np.uint64(1)).astype(np.int64)
    assert np.all(pop == 10)                                              # N2 shape: 10 electrons in 2 x 26 spin orbitals
    assert sum(a.nbytes for a in out.values()) <= 64 * 1000 * 1000


def test_same_arguments_same_outputs(runs):
    (_, a), (_, a2) = runs["a"], runs["a2"]
    assert sorted(a) == sorted(a2)
    for k in a:
        assert np.array_equal(a[k], a2[k]), k


def test_steps_and_warmup_count_iterations(runs):
    """3 timed steps after 2 of warm-up and 4 after 1 are the same five iterations from the same restart state."""
    (ra, a), (rb, b) = runs["a"], runs["b"]
    assert rb["steps"] == 4 and rb["warmup"] == 1
    for k in a:
        assert np.array_equal(a[k], b[k]), k
