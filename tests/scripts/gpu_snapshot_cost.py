"""What a vector snapshot and the estimators over ranks cost (run on the GPU box; writes profiles/snapshot_cost.txt and prints the same).

From the bench's state on the N2 shape at vec_nonz = mat_nonz = target = m, after the bench's warm-up of 10 iterations (the set-up of
gpu_replica_cost.py), two replicas a and b:
  * the build of a snapshot of b: wall time of fries_snapshot_create and its split into compaction, copy and insert by HIP events
    (fries_snapshot_info), medians of `repeats` builds after one that is not counted;
  * fries_h_dot, fries_rdm1 and fries_rdm2 through the snapshot beside the direct two-context call in the same process, alternating, medians
    of `repeats` after a call each that is not counted, with the spread (min, max) of both -- with `a` as one shard, and with the same
    vector dealt over 2 and 4 shards on the one GPU (contexts of a LocalGroup, each loaded with the determinants its rank owns);
  * the compiler's resource report for the new kernels (hipcc -Rpass-analysis=kernel-resource-usage on csrc/snapshot.hip; no GPU).
Each step is a process of its own under its own time limit; a step that fails ends the script.

usage: python tests/scripts/gpu_snapshot_cost.py [m] [repeats]
"""
import os
import re
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT = {"state": 240, "shards1": 300, "shards2": 300, "shards4": 300, "resources": 300}
KINDS = ("h_dot", "rdm1", "rdm2")


def _deal(a, P, m):
    """a's vector over the P contexts of a LocalGroup on the same GPU: every rank loaded with the determinants it owns"""
    import gpu_replica_cost as rc
    from fries_amd.comm import LocalGroup
    from fries_amd.engine import FriEngine
    par = rc._par(m)
    grp = LocalGroup(P, par["mat_nonz"])
    eng = [FriEngine(a.mol, device=0, comm=grp.comm(k, 0)) for k in range(P)]
    th = [threading.Thread(target=lambda e=e: e.setup(seed=rc.SEED, **par)) for e in eng]      # the set-up holds collectives
    for t in th:
        t.start()
    for t in th:
        t.join()
    d, v = a.vector()
    d, v = d[v != 0], v[v != 0]
    proc = eng[0].idx_to_proc(d)
    for k, e in enumerate(eng):
        e.vec_load(d[proc == k], v[proc == k])
    return grp, eng


def step_shards(m, repeats, state, P):
    import gpu_replica_cost as rc
    from fries_amd.engine import VecSnapshot
    reps = rc._replicas(m, 2, state)
    a, b = reps.engines
    print(f"a holds {a.vec_info()[1]} non-zero determinants, b {b.vec_info()[1]}; `a` as {P} shard(s)", flush=True)
    if P == 1:
        shards, grp = [a], None
        VecSnapshot([b]).close()
        wall, parts = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            sn = VecSnapshot([b])
            wall.append(1e3 * (time.perf_counter() - t0))
            info = sn.info
            parts.append((info.ms_compact, info.ms_copy, info.ms_insert))
            sn.close()
        parts = np.median(np.array(parts), axis=0)
        print(f"fries_snapshot_create of b: {np.median(wall):.3f} ms per call on the host (min {min(wall):.3f}, max {max(wall):.3f}); by HIP events: compaction {parts[0]:.3f} ms, "
              f"copy {parts[1]:.3f} ms, clear + insert {parts[2]:.3f} ms; {info.n_entries} entries, {info.n_slots} slots, {info.device_bytes} device bytes", flush=True)
    else:
        grp, shards = _deal(a, P, m)
        print(f"  shard sizes {[e.vec_info()[1] for e in shards]}", flush=True)
    snap = VecSnapshot([b])
    for kind in KINDS:
        direct, through = (lambda: getattr(a, kind)(b)), (lambda: getattr(snap, kind)(shards))
        want, got = direct(), through()
        ms = {"direct": [], "snapshot": []}
        for _ in range(repeats):
            for tag, call in (("direct", direct), ("snapshot", through)):
                t0 = time.perf_counter()
                call()
                ms[tag].append(1e3 * (time.perf_counter() - t0))
        assert (got.n_src, got.n_terms, got.n_hits) == (want.n_src, want.n_terms, want.n_hits)
        if P == 1:
            assert got[-5:] == want[-5:] and np.array_equal(np.asarray(got[0]), np.asarray(want[0])), kind       # one shard: the same bits
        md, msn = float(np.median(ms["direct"])), float(np.median(ms["snapshot"]))
        spread = max(ms["direct"]) - min(ms["direct"])
        print(f"fries_{kind:5s}: direct {md:9.2f} ms (min {min(ms['direct']):.2f}, max {max(ms['direct']):.2f}, spread {spread:.2f}); through the snapshot with {P} shard(s) {msn:9.2f} ms "
              f"(min {min(ms['snapshot']):.2f}, max {max(ms['snapshot']):.2f}); difference {msn - md:+.2f} ms = {100 * (msn - md) / md:+.2f} %, "
              f"{'inside' if abs(msn - md) <= spread else 'outside'} the direct call's spread; n_terms {got.n_terms}, n_hits {got.n_hits}", flush=True)
    snap.close()
    if grp is not None:
        for e in shards:
            e.close()
        grp.destroy()
    reps.close()


def step_resources():
    from fries_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory(prefix="fries_snapshot_rr_") as tmp:
        p = subprocess.run([hipcc] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, "snapshot.hip"), "-o", os.path.join(tmp, "s.o")],
                           capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit(p.stderr[-2000:])
    cur = None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: +(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m or "snapshot.hip" not in line.split(" remark:")[0]:
            continue
        if m.group(1) == "Function Name":
            if cur:
                print("  " + cur)
            cur = m.group(2) + ":"
        elif cur:
            cur += f" {m.group(1)} {m.group(2)};"
    if cur:
        print("  " + cur)


def main():
    import gpu_replica_cost as rc
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        name, m, repeats, state = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
        if name == "state":
            rc.step_state(m, repeats, state)
        elif name == "resources":
            step_resources()
        else:
            step_shards(m, repeats, state, int(name[6:]))
        return
    m = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000
    repeats = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    out = os.path.join(ROOT, "profiles", "snapshot_cost.txt")
    with tempfile.TemporaryDirectory(prefix="fries_snapshot_cost_") as tmp, open(out, "w") as f:
        state = os.path.join(tmp, "state.npz")
        for name in ("state", "shards1", "shards2", "shards4", "resources"):
            # a fresh process per step (this one never opens the device), ended at the step's own limit
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, str(m), str(repeats), state], timeout=STEP_LIMIT[name],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(os.environ, FRIES_SNAPSHOT_EVENTS="1"))      # (the build's event split)
            head = {"resources": "compiler's resource report for gfx950, csrc/snapshot.hip:\n"}.get(name, "")
            f.write(head + p.stdout)
            f.flush()
            print(head + p.stdout, end="", flush=True)
            if p.returncode != 0:
                raise SystemExit(f"step {name} failed with status {p.returncode}: nothing further is run")


if __name__ == "__main__":
    main()
