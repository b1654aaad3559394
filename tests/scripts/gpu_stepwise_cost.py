"""What keeping the loop on the host costs once nothing bulky crosses PCIe (run on the GPU box; writes plain text to stdout).

From the bench's state at vec_nonz = mat_nonz = target = m, in one process: FriEngine.iterate_stepwise (one iteration = the single-operator
calls of include/fries_hip.h, driven from Python) against the fused FriEngine.iterate, in alternating blocks of at least 0.5 s each that end
in a synchronisation, after a warm-up; median and spread over the blocks.  Then where the stepwise iteration's time goes: wall time per
call, and the kernels' own time from fries_prof_enable.  Last, frisys_mol_device_loop (tests/cpp/frisys_mol_device_loop.cpp, the C++ loop on include/FRIES/device_loop.hpp)
restarted from the same state: time per iteration by the difference of two run lengths, PCIe bytes per iteration from FRIES_FACADE_STATS=1.

usage: python tests/scripts/gpu_stepwise_cost.py [m] [blocks]
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


def main():
    m = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000
    n_blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    import bench
    from fries_amd import build, fcidump
    from fries_amd.engine import FriEngine

    mol = fcidump.synthetic("N2")
    max_dets = 4 * m
    dets, vals = bench.build_state(mol, m, max_dets, 20250215, 0, None, None)
    print(f"state: {len(vals)} determinants, one-norm {np.abs(vals).sum():.1f}", flush=True)
    par = dict(epsilon=0.01, vec_nonz=m, mat_nonz=m, max_dets=max_dets, target_norm=float(m), initiator=1.0, seed=20250215, distribution="HB_unnorm")

    def fresh():
        eng = FriEngine(mol, device=0)
        eng.setup(**par)
        eng.vec_load(dets, vals)
        eng.restart(777, 0.0, 0.0, 0)
        return eng

    step, fused = fresh(), fresh()
    step.iterate_stepwise(10)
    fused.iterate(10, want_logs=False)
    fused.vec_info()

    def block(eng, stepwise):
        n, t0 = 0, time.perf_counter()
        while True:
            if stepwise:
                eng.iterate_stepwise(20)
            else:
                eng.iterate(20, want_logs=False)
            eng.vec_info()          # drains the stream
            n += 20
            dt = time.perf_counter() - t0
            if dt >= 0.5:
                return n / dt

    rates = {"stepwise": [], "fused": []}
    for _ in range(n_blocks):
        rates["stepwise"].append(block(step, True))
        rates["fused"].append(block(fused, False))
    print(f"m = {m}, {n_blocks} alternating blocks of >= 0.5 s each, same state, one process:")
    for k in ("stepwise", "fused"):
        r = np.array(rates[k])
        print(f"  {k:9s} {np.median(r):7.1f} iterations/s (median; min {r.min():.1f}, max {r.max():.1f})")
    print(f"  stepwise / fused = {np.median(rates['stepwise']) / np.median(rates['fused']):.3f}")

    # where the stepwise iteration's time goes: wall time per call ...
    names = ["next_draw", "apply_hbpp_sys_device", "vec_info", "spawn_from_comp", "dense_apply", "death_clone", "dots", "find_preserve", "sys_comp"]
    wall = {k: 0.0 for k in names}
    for k in names:
        fn = getattr(step, k)

        def timed(*a, _fn=fn, _k=k, **kw):
            t0 = time.perf_counter()
            out = _fn(*a, **kw)
            wall[_k] += time.perf_counter() - t0
            return out
        setattr(step, k, timed)
    n_prof = 40
    step.prof_enable(True)
    t0 = time.perf_counter()
    step.iterate_stepwise(n_prof)
    tot = time.perf_counter() - t0
    rep = step.prof_report()
    step.prof_enable(False)
    print(f"stepwise iteration with per-kernel events on ({n_prof} iterations): {tot / n_prof * 1e3:.3f} ms wall per iteration, of which per call:")
    for k in names:
        print(f"  {k:22s} {wall[k] / n_prof * 1e3:7.3f} ms")
    kern = sum(v[0] for v in rep.values())
    print(f"  kernels' own time (HIP events): {kern / n_prof:.3f} ms per iteration over {sum(v[1] for v in rep.values()) / n_prof:.1f} launches; the rest is launch gaps and host waits")
    for name, (ms, calls) in sorted(rep.items(), key=lambda kv: -kv[1][0])[:6]:
        print(f"    {name:20s} {ms / n_prof:7.3f} ms  {calls / n_prof:6.1f} calls")
    # what the C++ loop below pays beside these calls: DistVec::dot uploads its list on every call (fries_vec_dot_list), twice per iteration
    import ctypes as C
    hd, hv = step.htrial()
    out = C.c_double()
    t0 = time.perf_counter()
    for _ in range(50):
        step._ck(step.lib.fries_vec_dot_list(step.h, 0, hd.ctypes.data_as(C.c_void_p), hv.ctypes.data_as(C.c_void_p), hd.size, C.byref(out)))
    print(f"  fries_vec_dot_list with the {hd.size} elements of H * trial (what DistVec::dot of include/FRIES calls): {(time.perf_counter() - t0) / 50 * 1e3:.3f} ms per call")
    step.close()
    fused.close()

    # the C++ consumer of include/FRIES/device_loop.hpp from the same state (a checkpoint in the reference's format)
    exe = build.DEVICE_LOOP_DRIVER
    tmp = tempfile.mkdtemp(prefix="fries_stepwise_")
    ck = os.path.join(tmp, "ck") + "/"
    os.makedirs(ck)
    fc = os.path.join(tmp, "mol.FCIDUMP")
    fcidump.write_fcidump(fc, mol)
    det_size = (2 * mol.n_orb + 7) // 8
    np.ascontiguousarray(dets, dtype=np.uint64).view(np.uint8).reshape(-1, 8)[:, :det_size].tofile(ck + "dets0.dat")
    np.concatenate([np.asarray(vals, dtype=np.float64), np.zeros(len(vals))]).tofile(ck + "vals0.dat")
    np.random.default_rng(5).integers(0, 2 ** 32, size=2 * mol.n_orb, dtype=np.uint32).tofile(ck + "hash.dat")
    open(ck + "dense.txt", "w").write("0\n")
    open(ck + "S.txt", "w").write("0\n")

    def run(iters):
        out = tempfile.mkdtemp(prefix=f"out{iters}_", dir=tmp) + "/"
        cmd = [exe, "--fcidump_path", fc, "--point_group", mol.point_group, "--distribution", "HB_unnorm", "--vec_nonz", str(m), "--mat_nonz", str(m),
               "--max_dets", str(max_dets), "--target", repr(float(m)), "--initiator", "1", "--epsilon", "0.01", "--max_iter", str(iters),
               "--load_dir", ck, "--result_dir", out, "--seed", "777"]
        t0 = time.perf_counter()
        p = subprocess.run(cmd, env=dict(os.environ, FRIES_FACADE_STATS="1", FRIES_DEVICE="0"), capture_output=True, text=True, timeout=600)
        dt = time.perf_counter() - t0
        if p.returncode != 0:
            raise SystemExit(f"frisys_mol_device_loop failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        mm = re.search(r"fries facade: (\d+) bytes host->device, (\d+) bytes device->host", p.stderr)
        # the closing save() fetches the determinants and both columns, 24 bytes per stored position of a vector whose size differs
        # between the two runs: not the loop's traffic, taken off
        n_saved = os.path.getsize(out + "dets0.dat") // det_size
        return dt, int(mm.group(1)), int(mm.group(2)) - 24 * n_saved, len(np.loadtxt(out + "nkept.txt", ndmin=1))

    # both lengths below the driver's save interval of 100 iterations (a checkpoint fetches the whole vector: not the loop's cost);
    # the faster of three runs each, the processes' start-up varying more than 60 iterations take
    a, b = (min((run(n) for _ in range(3)), key=lambda r: r[0]) for n in (30, 95))
    d_it = b[3] - a[3]
    per_it = (b[0] - a[0]) / d_it
    print(f"frisys_mol_device_loop (tests/cpp/frisys_mol_device_loop.cpp: the reference's loop shape on include/FRIES/device_loop.hpp), m = {m}:")
    print(f"  runs of {a[3]} and {b[3]} iterations: {a[0]:.2f} s and {b[0]:.2f} s  ->  {per_it * 1e3:.2f} ms per iteration = {1.0 / per_it:.1f} iterations/s (set-up excluded by the difference)")
    print(f"  PCIe per iteration: {(b[1] - a[1]) / d_it:.0f} bytes host->device, {(b[2] - a[2]) / d_it:.0f} bytes device->host (the closing save() excluded)")


if __name__ == "__main__":
    main()
