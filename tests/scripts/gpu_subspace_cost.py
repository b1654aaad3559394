"""What the operators of the subspace iteration cost (run on the GPU box; writes profiles/subspace_cost.txt and prints the same).

From the bench's state on the N2 shape at vec_nonz = mat_nonz = target = m, after the bench's warm-up of 10 iterations (the set-up of
gpu_replica_cost.py), medians of `repeats` calls after one that is not counted:
  * fries_vec_axpy_snapshot with every entry of the snapshot stored already, and with none of them stored (an empty vector);
  * fries_snapshot_dot beside fries_h_dot of the same pair;
  * a restart of FriSubspace with 2 and with 4 states (snapshots, scales, axpys, one-norms);
  * one FriSubspace iteration per state beside one iterate_stepwise iteration of the same vector;
  * "refdev": on MIN6 at vec_nonz = 60, mat_nonz = 200 over 2000 iterations, the deviation of the single-vector estimator (mean of numer
    over mean of denom from iteration 500 on, iterate_stepwise) from the ground-state energy of numpy.linalg.eigh -- the literal that
    tests/test_gpu_subspace.py::test_compressed_run_against_eigh scales its allowance from;
  * the compiler's resource report for the new kernels (no GPU).
Each step is a process of its own under its own time limit; a step that fails ends the script.

usage: python tests/scripts/gpu_subspace_cost.py [m] [repeats] [step ...]
"""
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
STEPS = ("state", "ops", "restart2", "restart4", "iteration", "refdev", "resources")
STEP_LIMIT = {"state": 240, "ops": 300, "restart2": 300, "restart4": 400, "iteration": 400, "refdev": 300, "resources": 400}
REFDEV = dict(epsilon=0.1, vec_nonz=60, mat_nonz=200, max_dets=2000, n_iter=2000, burn_in=500, seed=20261021)


def _median(call, repeats, before=None):
    if before:
        before()
    call()
    ms = []
    for _ in range(repeats):
        if before:
            before()
        t0 = time.perf_counter()
        call()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms)), min(ms), max(ms)


def _fmt(t):
    return f"{t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


def step_ops(m, repeats, state):
    import gpu_replica_cost as rc
    from fries_amd.engine import VecSnapshot
    reps = rc._replicas(m, 2, state)
    a, b = reps.engines
    d, v = a.vector()
    d, v = d[v != 0], v[v != 0]
    print(f"a holds {a.vec_info()[1]} non-zero determinants, b {b.vec_info()[1]}", flush=True)
    with VecSnapshot([a]) as sa, VecSnapshot([b]) as sb:
        n = sa.info.n_entries
        t = _median(lambda: (a.axpy_snapshot(0, 1e-3, sa), a.vec_info()), repeats)
        print(f"fries_vec_axpy_snapshot, all {n} entries present (a += 1e-3 a): {_fmt(t)}", flush=True)
        empty = np.zeros(0, dtype=np.uint64), np.zeros(0)
        t = _median(lambda: (b.axpy_snapshot(0, 1.0, sa), b.vec_info()), repeats, before=lambda: b.vec_load(*empty))
        print(f"fries_vec_axpy_snapshot, all {n} entries new (into an empty vector):   {_fmt(t)}", flush=True)
        b.vec_load(*sb.vector())
        a.vec_load(d, v)
        t = _median(lambda: sb.dot([a]), repeats)
        r = sb.dot([a])
        print(f"fries_snapshot_dot (a, snapshot of b): {_fmt(t)}; n_src {r.n_src}, n_hits {r.n_hits}", flush=True)
        t = _median(lambda: a.h_dot(b), repeats)
        print(f"fries_h_dot (a, b), for comparison:    {_fmt(t)}", flush=True)
        t = _median(lambda: a.one_norm(0), repeats)
        print(f"fries_vec_one_norm: {_fmt(t)}", flush=True)
        t = _median(lambda: (a.scale(0, 1.0), a.vec_info()), repeats)
        print(f"fries_vec_scale:    {_fmt(t)}", flush=True)
    reps.close()


def _subspace(m, n, state):
    import gpu_replica_cost as rc
    from fries_amd import fcidump
    from fries_amd.subspace import FriSubspace
    st = np.load(state)
    par = rc._par(m)
    order = np.argsort(-np.abs(st["vals"]))[:4 * n]
    rng = np.random.RandomState(3)
    trials = [(st["dets"][order], rng.standard_normal(order.size)) for _ in range(n)]
    sub = FriSubspace(fcidump.synthetic("N2"), trials, epsilon=par["epsilon"], vec_nonz=m, mat_nonz=m, max_dets=par["max_dets"], restart_int=10, initiator=1.0, seed=rc.SEED)
    for k, e in enumerate(sub.engines):     # the bench's state with another sign pattern per state, so that the states differ
        e.vec_load(st["dets"], st["vals"] * np.where(rng.random_sample(st["vals"].size) < 0.05 * k, -1.0, 1.0))
    return sub


def step_restart(m, repeats, state, n):
    sub = _subspace(m, n, state)
    d_mat, h_mat = sub.measure()
    t = _median(lambda: (sub._restart(d_mat, h_mat), [e.vec_info() for e in sub.engines]), repeats)
    print(f"a restart of {n} states: {_fmt(t)}; sizes afterwards {[e.vec_info()[1] for e in sub.engines]}", flush=True)
    sub.close()


def step_iteration(m, repeats, state):
    import gpu_replica_cost as rc
    sub = _subspace(m, 2, state)
    sub.restart_int = 10 ** 9       # the iterations timed here hold no restart
    t = _median(lambda: (sub.iterate(1), [e.vec_info() for e in sub.engines]), repeats)
    print(f"one FriSubspace iteration of 2 states: {_fmt(t)}, i.e. {t[0] / 2:.3f} ms per state", flush=True)
    sub.close()
    reps = rc._replicas(m, 1, state)
    e = reps.engines[0]
    t = _median(lambda: (e.iterate_stepwise(1), e.vec_info()), repeats)
    print(f"one iterate_stepwise iteration:        {_fmt(t)}", flush=True)
    reps.close()


def step_refdev():
    from fries_amd import fcidump
    from fries_amd.engine import FriEngine
    from fries_amd.subspace import dense_h
    mol = fcidump.synthetic("MIN6")
    n = mol.n_orb
    dets = np.array([a | (b << n) for a in range(1 << n) for b in range(1 << n) if bin(a).count("1") == 2 and bin(b).count("1") == 2], dtype=np.uint64)
    e0 = float(np.linalg.eigvalsh(dense_h(mol, dets))[0])
    p = REFDEV
    eng = FriEngine(mol)
    eng.setup(epsilon=p["epsilon"], vec_nonz=p["vec_nonz"], mat_nonz=p["mat_nonz"], max_dets=p["max_dets"], target_norm=1000.0, initiator=0.0, seed=p["seed"], distribution="HB_unnorm")
    t0 = time.perf_counter()
    lg = eng.iterate_stepwise(p["n_iter"])
    wall = time.perf_counter() - t0
    est = float(np.mean(lg["numer"][p["burn_in"]:]) / np.mean(lg["denom"][p["burn_in"]:])) + eng.hf_energy
    print(f"MIN6 {p}: eigh ground state {e0!r}; single-vector estimator {est!r}; deviation {abs(est - e0):.6e} ({wall:.1f} s)", flush=True)
    eng.close()


def step_resources():
    from fries_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    want = ("k_axpy_count", "k_axpy_write", "k_snap_dot", "k_vec_scale", "k_snap_scan")
    for src in ("snapshot.hip", "api_vec.hip"):
        with tempfile.TemporaryDirectory(prefix="fries_subspace_rr_") as tmp:
            p = subprocess.run([hipcc] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, src), "-o", os.path.join(tmp, "s.o")],
                               capture_output=True, text=True)
        if p.returncode != 0:
            raise SystemExit(p.stderr[-2000:])
        cur, lines = None, []
        for line in p.stderr.splitlines():
            mt = re.search(r"remark: +(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
            if not mt or src not in line.split(" remark:")[0]:
                continue
            if mt.group(1) == "Function Name":
                cur = mt.group(2) + ":"
                lines.append(cur)
            elif cur:
                lines[-1] += f" {mt.group(1)} {mt.group(2)};"
        for ln in lines:
            if any(k in ln for k in want):
                print("  " + ln)


def main():
    import gpu_replica_cost as rc
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        name, m, repeats, state = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
        if name == "state":
            rc.step_state(m, repeats, state)
        elif name == "ops":
            step_ops(m, repeats, state)
        elif name.startswith("restart"):
            step_restart(m, repeats, state, int(name[7:]))
        elif name == "iteration":
            step_iteration(m, repeats, state)
        elif name == "refdev":
            step_refdev()
        else:
            step_resources()
        return
    m = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000
    repeats = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    steps = [s for s in sys.argv[3:] if s in STEPS] or list(STEPS)
    if "state" not in steps and any(s in steps for s in ("ops", "restart2", "restart4", "iteration")):
        steps.insert(0, "state")
    out = os.path.join(ROOT, "profiles", "subspace_cost.txt" if set(steps) == set(STEPS) else "subspace_cost_partial.txt")
    with tempfile.TemporaryDirectory(prefix="fries_subspace_cost_") as tmp, open(out, "w") as f:
        state = os.path.join(tmp, "state.npz")
        for name in [s for s in STEPS if s in steps]:
            # a fresh process per step (this one never opens the device), ended at the step's own limit
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, str(m), str(repeats), state], timeout=STEP_LIMIT[name],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            head = {"resources": "compiler's resource report for gfx950:\n"}.get(name, "")
            f.write(head + p.stdout)
            f.flush()
            print(head + p.stdout, end="", flush=True)
            if p.returncode != 0:
                raise SystemExit(f"step {name} failed with status {p.returncode}: nothing further is run")


if __name__ == "__main__":
    main()
