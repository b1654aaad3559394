"""What the replica estimator and concurrent replicas cost (run on the GPU box; writes plain text to stdout -> profiles/replica_cost.txt).

From the bench's state on the N2 shape at vec_nonz = mat_nonz = target = m, after the bench's warm-up of 10 iterations:
  (a) fries_h_dot between two replicas (a != b) and of one vector with itself (a = b): ms per call, n_terms per second, n_hits / n_terms,
      and what share of k_hdot's candidate slots is rejected (by symmetry or occupation; counted on the host for a sample of sources);
  (b) aggregate iterations per second of FriReplicas for R = 1, 2, 4 -- R fused loops at once, one thread and one stream each -- beside
      R times one plain run, i.e. the same R engines iterated one after the other, in alternating blocks of the same session.
Every figure is the median of at least 5 repeats.  Each step is a process of its own under its own time limit; a step that fails ends
the script.

usage: python tests/scripts/gpu_replica_cost.py [m] [repeats]
"""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SEED = 20250215
STEP_LIMIT = {"state": 240, "hdot": 240, "repl1": 240, "repl2": 300, "repl4": 400}


def _par(m):
    return dict(epsilon=0.01, vec_nonz=m, mat_nonz=m, max_dets=4 * m, target_norm=float(m), initiator=1.0, distribution="HB_unnorm")


def _replicas(m, n, state):
    """n replicas that start from the bench's state and part ways through their seeds"""
    from fries_amd import fcidump
    from fries_amd.replicas import FriReplicas
    st = np.load(state)
    reps = FriReplicas(fcidump.synthetic("N2"), n, SEED, **_par(m))
    for r, e in enumerate(reps.engines):
        e.vec_load(st["dets"], st["vals"])
        e.restart(777 + r, 0.0, 0.0, 0)
    reps.iterate(10)        # the bench's warm-up
    for e in reps.engines:
        e.vec_info()
    return reps


def _allowed_share(mol, dets):
    """symmetry- and occupation-allowed excitations of each determinant over the candidate slots k_enum / k_hdot walk"""
    n, ne = mol.n_orb, mol.n_elec
    h = ne // 2
    irr = np.asarray(mol.irreps, dtype=np.int64)
    n_cand = ne * n + h * h * n * n + 2 * (h * (h - 1) // 2) * n * n
    out = []
    for d in dets:
        d = int(d)
        occ = [[o for o in range(n) if d >> (o + s * n) & 1] for s in (0, 1)]
        virt = [np.bincount(irr[[o for o in range(n) if not d >> (o + s * n) & 1]], minlength=8) for s in (0, 1)]
        tot = sum(int(virt[s][irr[o]]) for s in (0, 1) for o in occ[s])
        for i in occ[0]:
            for j in occ[1]:
                g = irr[i] ^ irr[j]
                tot += sum(int(virt[0][x]) * int(virt[1][x ^ g]) for x in range(8))
        for s in (0, 1):
            for a in range(h):
                for b in range(a + 1, h):
                    g = irr[occ[s][a]] ^ irr[occ[s][b]]
                    if g:
                        tot += sum(int(virt[s][x]) * int(virt[s][x ^ g]) for x in range(8)) // 2
                    else:
                        tot += sum(int(virt[s][x]) * (int(virt[s][x]) - 1) // 2 for x in range(8))
        out.append(tot / n_cand)
    return float(np.mean(out)), n_cand


def step_state(m, repeats, state):
    import bench
    from fries_amd import fcidump
    dets, vals = bench.build_state(fcidump.synthetic("N2"), m, 4 * m, SEED, 0, None, None)
    np.savez(state, dets=dets, vals=vals)
    print(f"N2 shape, m = {m}: state of {len(vals)} determinants, one-norm {np.abs(vals).sum():.1f}; every figure below is the median of {repeats} repeats", flush=True)


def step_hdot(m, repeats, state):
    from fries_amd import fcidump
    reps = _replicas(m, 2, state)
    a, b = reps.engines
    print("(a) fries_h_dot after the warm-up:")
    for tag, x, y in (("a != b", a, b), ("a = b ", a, a)):
        x.h_dot(y)
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = x.h_dot(y)
            ms.append(1e3 * (time.perf_counter() - t0))
        med = float(np.median(ms))
        print(f"  {tag}: {med:8.2f} ms per call (min {min(ms):.2f}, max {max(ms):.2f}); n_src {res.n_src}, n_terms {res.n_terms} = {res.n_terms / med * 1e3:.3e} per second, "
              f"n_hits {res.n_hits}, n_hits / n_terms = {res.n_hits / res.n_terms:.4f}; h / ovlp = {res.h / res.ovlp:.6f}", flush=True)
        assert x.h_dot(y) == res
    d, v = a.vector()
    d = d[v != 0]
    sample = d[np.random.RandomState(1).choice(d.size, size=min(2000, d.size), replace=False)]
    share, n_cand = _allowed_share(fcidump.synthetic("N2"), sample)
    print(f"  candidate slots per source: {n_cand}; allowed (symmetry and occupation) on {sample.size} sampled sources: {100 * share:.2f} %, rejected: {100 * (1 - share):.2f} %; "
          f"slots with a non-zero element: {100 * res.n_terms / (res.n_src * n_cand):.2f} %")
    reps.close()


def step_repl(m, repeats, state, n):
    reps = _replicas(m, n, state)
    k = 20

    def drain():
        for e in reps.engines:
            e.vec_info()

    def concurrent():
        t0 = time.perf_counter()
        reps.iterate(k)
        drain()
        return n * k / (time.perf_counter() - t0)

    def sequential():
        t0 = time.perf_counter()
        for e in reps.engines:
            e.iterate(k, want_logs=False)
            e.vec_info()
        return n * k / (time.perf_counter() - t0)

    con, seq = [], []
    for _ in range(repeats):
        con.append(concurrent())
        seq.append(sequential())
    con, seq = np.array(con), np.array(seq)
    print(f"(b) R = {n}: FriReplicas {np.median(con):7.1f} iterations/s in all (min {con.min():.1f}, max {con.max():.1f}); the same {n} engines one after the other "
          f"{np.median(seq):7.1f} (min {seq.min():.1f}, max {seq.max():.1f}); concurrent / sequential = {np.median(con) / np.median(seq):.3f}", flush=True)
    reps.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        name, m, repeats, state = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
        if name == "state":
            step_state(m, repeats, state)
        elif name == "hdot":
            step_hdot(m, repeats, state)
        else:
            step_repl(m, repeats, state, int(name[4:]))
        return
    m = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000
    repeats = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    with tempfile.TemporaryDirectory(prefix="fries_replica_cost_") as tmp:
        state = os.path.join(tmp, "state.npz")
        for name in ("state", "hdot", "repl1", "repl2", "repl4"):
            # a fresh process per step (this one never opens the device), ended at the step's own limit
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, str(m), str(repeats), state], timeout=STEP_LIMIT[name])
            if p.returncode != 0:
                raise SystemExit(f"step {name} failed with status {p.returncode}: nothing further is run")


if __name__ == "__main__":
    main()
