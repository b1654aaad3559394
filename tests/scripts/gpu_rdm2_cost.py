"""What the two-body density matrix between replicas costs (run on the GPU box; writes plain text to stdout -> profiles/rdm2_cost.txt).

From the bench's state on the N2 shape at vec_nonz = mat_nonz = target = m, after the bench's warm-up of 10 iterations (the set-up of
gpu_replica_cost.py): fries_rdm2 between two replicas (a != b) and of one vector with itself (a = b), with fries_rdm1 and fries_h_dot on
the same vectors in the same process as yardsticks: ms per call, probes (n_terms) per second, hits.  The records, chunks and scratch
bytes are what the call itself reports under FRIES_DBG=1.  The kernels' own times come from the engine's event profiler in a second
pass.  Every figure is the median of at least 5 repeats after one call that is not counted.  The step is then repeated, a != b only and
with 3 repeats, at other capacities of a chunk (FRIES_RDM2_RECORDS, read when the context is created): what the default was chosen
against.  Each step is a process of its own under its own time limit; a step that fails ends the script.

usage: python tests/scripts/gpu_rdm2_cost.py [m] [repeats] [capacity ...]
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
STEP_LIMIT = {"state": 240, "rdm2": 420}
KERNELS = ("k_rdm2_count", "k_rdm2_emit", "k_r2_hist", "k_r2_scan", "k_r2_scatter", "k_r2_piece", "k_r2_fold", "k_rdm1", "k_rdm1_reduce", "k_hdot", "k_hdot_reduce")


def step_rdm2(m, repeats, state, full):
    import gpu_replica_cost as rc
    reps = rc._replicas(m, 2, state)
    a, b = reps.engines
    size = [e.vec_info() for e in (a, b)]
    print(f"capacity {os.environ.get('FRIES_RDM2_RECORDS', 'default')}: after the warm-up a holds {size[0][0]} positions ({size[0][1]} non-zero), b {size[1][0]} ({size[1][1]})", flush=True)

    def timed(call):
        call()
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = call()
            ms.append(1e3 * (time.perf_counter() - t0))
        return res, float(np.median(ms)), min(ms), max(ms)

    for tag, x, y in (("a != b", a, b), ("a = b ", a, a)) if full else (("a != b", a, b),):
        res, med, lo, hi = timed(lambda: x.rdm2(y))
        n_elec = x.mol.n_elec
        print(f"fries_rdm2  {tag}: {med:9.2f} ms per call (min {lo:.2f}, max {hi:.2f}); n_src {res.n_src}, n_terms {res.n_terms} = {res.n_terms / med * 1e3:.3e} probes per second per call "
              f"(every probe is issued twice: counting and emitting), n_hits {res.n_hits}, n_hits / n_terms = {res.n_hits / res.n_terms:.4f}; "
              f"full trace / ovlp = {np.einsum('pprr->', res.gamma2) / res.ovlp:.10f} (n_elec (n_elec - 1) = {n_elec * (n_elec - 1)})", flush=True)
        if not full:
            continue
        again = x.rdm2(y)
        assert np.array_equal(again.gamma2, res.gamma2) and again[1:] == res[1:]
        assert np.array_equal(res.gamma2, res.gamma2.transpose(2, 3, 0, 1))
        r1, med1, lo1, hi1 = timed(lambda: x.rdm1(y))
        print(f"fries_rdm1  {tag}: {med1:9.2f} ms per call (min {lo1:.2f}, max {hi1:.2f}); n_terms {r1.n_terms}; rdm2 / rdm1: time {med / med1:.1f}, probes {res.n_terms / r1.n_terms:.1f}; "
              f"largest |sum_r Gamma[p,q,r,r] / (n_elec - 1) - gamma[p,q]| = {np.abs(res.partial_trace(n_elec) - r1.gamma).max():.3e} against a largest |gamma[p,q]| of {np.abs(r1.gamma).max():.3e}", flush=True)
        hres, hmed, hlo, hhi = timed(lambda: x.h_dot(y))
        print(f"fries_h_dot {tag}: {hmed:9.2f} ms per call (min {hlo:.2f}, max {hhi:.2f}); n_terms {hres.n_terms}; rdm2 / h_dot: time {med / hmed:.1f}, probes {res.n_terms / hres.n_terms:.1f}", flush=True)
    # the kernels alone (HIP events around every launch; the calls above ran without them)
    n_prof = repeats if full else 1
    a.prof_enable(True)
    for _ in range(n_prof):
        a.rdm2(b)
        if full:
            a.rdm1(b)
            a.h_dot(b)
    rep = a.prof_report()
    for name in KERNELS:
        if name in rep:
            ms, calls = rep[name]
            print(f"  {name:14s}: {ms / n_prof:9.3f} ms per call of the estimator over {calls // n_prof} launch(es)")
    a.prof_enable(False)
    reps.close()


def main():
    import gpu_replica_cost as rc
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        name, m, repeats, state = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
        if name == "state":
            rc.step_state(m, repeats, state)
        else:
            step_rdm2(m, repeats, state, full=name == "rdm2")
        return
    m = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000
    repeats = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    capacities = [int(x) for x in sys.argv[3:]]
    with tempfile.TemporaryDirectory(prefix="fries_rdm2_cost_") as tmp:
        state = os.path.join(tmp, "state.npz")
        for name, cap in [("state", None), ("rdm2", None)] + [("rdm2cap", c) for c in capacities]:
            env = dict(os.environ, FRIES_DBG="1")
            if cap is not None:
                env["FRIES_RDM2_RECORDS"] = str(cap)
            # a fresh process per step (this one never opens the device), ended at the step's own limit
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, str(m), str(3 if cap is not None else repeats), state],
                               timeout=STEP_LIMIT["state" if name == "state" else "rdm2"], env=env, stderr=subprocess.STDOUT)
            if p.returncode != 0:
                raise SystemExit(f"step {name} failed with status {p.returncode}: nothing further is run")


if __name__ == "__main__":
    main()
