"""What the one-body density matrix between replicas costs (run on the GPU box; writes plain text to stdout -> profiles/rdm1_cost.txt).

From the bench's state on the N2 shape at vec_nonz = mat_nonz = target = m, after the bench's warm-up of 10 iterations (the set-up of
gpu_replica_cost.py): fries_rdm1 between two replicas (a != b) and of one vector with itself (a = b), and fries_h_dot on the same vectors
in the same process as the yardstick: ms per call, probes (n_terms) per second, n_hits / n_terms, and n_terms * 16 bytes -- the first
16-byte probe of every candidate -- over the measured time.  The kernels' own times come from the engine's event profiler in a second
pass, so that the host's share of a call (allocation of the scratch, two synchronisations, the copy of the matrix) can be told from
the device's.  Every figure is the median of at least 5 repeats.  Each step is a process of its own under its own time limit; a step that
fails ends the script.

usage: python tests/scripts/gpu_rdm1_cost.py [m] [repeats]
"""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT = {"state": 240, "rdm1": 300}


def step_rdm1(m, repeats, state):
    import gpu_replica_cost as rc
    reps = rc._replicas(m, 2, state)
    a, b = reps.engines
    size = [e.vec_info() for e in (a, b)]
    print(f"after the warm-up: a holds {size[0][0]} positions ({size[0][1]} non-zero), b {size[1][0]} ({size[1][1]})")

    def timed(call):
        call()
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = call()
            ms.append(1e3 * (time.perf_counter() - t0))
        return res, float(np.median(ms)), min(ms), max(ms)

    for tag, x, y in (("a != b", a, b), ("a = b ", a, a)):
        res, med, lo, hi = timed(lambda: x.rdm1(y))
        again = x.rdm1(y)
        assert np.array_equal(again.gamma, res.gamma) and again[1:] == res[1:]
        print(f"fries_rdm1  {tag}: {med:8.2f} ms per call (min {lo:.2f}, max {hi:.2f}); n_src {res.n_src}, n_terms {res.n_terms} = {res.n_terms / med * 1e3:.3e} probes per second, "
              f"n_hits {res.n_hits}, n_hits / n_terms = {res.n_hits / res.n_terms:.4f}; first probes {res.n_terms * 16 / 1e9:.2f} GB = {res.n_terms * 16 / med / 1e9:.3f} TB/s; "
              f"trace / ovlp = {np.trace(res.gamma) / res.ovlp:.12f}", flush=True)
        hres, hmed, hlo, hhi = timed(lambda: x.h_dot(y))
        print(f"fries_h_dot {tag}: {hmed:8.2f} ms per call (min {hlo:.2f}, max {hhi:.2f}); n_terms {hres.n_terms} = {hres.n_terms / hmed * 1e3:.3e} probes per second, "
              f"n_hits / n_terms = {hres.n_hits / hres.n_terms:.4f}; first probes {hres.n_terms * 16 / hmed / 1e9:.3f} TB/s; rdm1 / h_dot: time {med / hmed:.3f}, probes {res.n_terms / hres.n_terms:.3f}", flush=True)
    # the kernels alone (HIP events around every launch; the calls above ran without them)
    a.prof_enable(True)
    for _ in range(repeats):
        a.rdm1(b)
        a.h_dot(b)
    rep = a.prof_report()
    for name in ("k_rdm1", "k_rdm1_reduce", "k_hdot", "k_hdot_reduce"):
        if name in rep:
            ms, calls = rep[name]
            print(f"  {name:14s}: {ms / repeats:8.3f} ms per call of the estimator over {calls // repeats} launch(es)")
    a.prof_enable(False)
    reps.close()


def main():
    import gpu_replica_cost as rc
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        name, m, repeats, state = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
        if name == "state":
            rc.step_state(m, repeats, state)
        else:
            step_rdm1(m, repeats, state)
        return
    m = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000
    repeats = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    with tempfile.TemporaryDirectory(prefix="fries_rdm1_cost_") as tmp:
        state = os.path.join(tmp, "state.npz")
        for name in ("state", "rdm1"):
            # a fresh process per step (this one never opens the device), ended at the step's own limit
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, str(m), str(repeats), state], timeout=STEP_LIMIT[name])
            if p.returncode != 0:
                raise SystemExit(f"step {name} failed with status {p.returncode}: nothing further is run")


if __name__ == "__main__":
    main()
