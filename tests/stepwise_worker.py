"""One rank of a hash-sharded FRI run driven step by step (launched by torch.distributed.run from test_gpu_stepwise.py).

Like ranks_worker.py, but the iteration is FriEngine.iterate_stepwise: every rank makes the single-operator calls in the same order, so
fries_spawn_from_comp, fries_dense_apply and fries_dense_norm are entered as collectives.  What THIS rank logs is compared with what the
same rank of the reference logged under mpiexec: scalars, shard sizes, and the digest of the shard.
"""
import datetime
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    import torch
    import torch.distributed as dist
    import golden_io
    from fries_amd import fcidump
    from fries_amd.comm import TorchComm
    from fries_amd.engine import FriEngine

    name, backend, out_dir = sys.argv[1], sys.argv[2], sys.argv[3]
    rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"]); local = int(os.environ.get("LOCAL_RANK", "0"))
    dev = local % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, timeout=datetime.timedelta(seconds=180))     # a dead peer must surface as an error, not a hang
    man = golden_io.manifest()
    r = next(man[k][name] for k in ("mpi_runs", "dense_mpi_runs", "adder_runs") if name in man.get(k, {}))
    assert r["n_ranks"] == world, (r["n_ranks"], world)
    g = golden_io.read_traj(name, rank=rank)
    res = dict(rank=rank, ok=True, fails=[])
    mol = fcidump.synthetic(r["shape"])
    comm = TorchComm(r["mat_nonz"], torch.device("cuda", dev))
    eng = FriEngine(mol, device=dev, comm=comm)
    space = None
    if "det_space" in r:
        space = np.array([int(x) for x in open(os.path.join(golden_io.GOLD, r["det_space"])).read().split()], dtype=np.uint64)
    eng.setup(epsilon=r["epsilon"], vec_nonz=r["vec_nonz"], mat_nonz=r["mat_nonz"], max_dets=r["max_dets"], target_norm=r["target_norm"],
              initiator=r["initiator"], seed=r["seed"], distribution=r["distribution"], det_space=space)
    if eng.p_doub != g["p_doub"]:
        res["fails"].append(("p_doub", eng.p_doub, g["p_doub"]))
    rows = g["rows"]
    for row in rows:
        lg = eng.iterate_stepwise(1)[0]
        for f in ("norm", "shift"):
            if float(lg[f]) != row[f]:
                res["fails"].append((row["it"], f, float(lg[f]), row[f]))
        for f in ("numer", "denom"):       # as ranks_worker.py: 1e-10 relative with ranks
            if abs(float(lg[f]) - row[f]) > 1e-10 * max(1.0, abs(row[f])):
                res["fails"].append((row["it"], f, float(lg[f]), row[f]))
        for f in ("nkept", "n_nonz", "curr_size", "num_success"):
            if int(lg[f]) != row[f]:
                res["fails"].append((row["it"], f, int(lg[f]), row[f]))
        del res["fails"][8:]       # (no early exit: the other ranks would wait in their next collective)
    d, v = eng.vector()
    if not res["fails"] and golden_io.vec_hash(d, v) != rows[-1]["hash"]:
        res["fails"].append(("digest",))
    res["ok"] = not res["fails"]
    res["n_allgather"] = comm.n_allgather; res["n_alltoallv"] = comm.n_alltoallv; res["iters"] = len(rows)
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(res, f, default=str)
    dist.barrier()
    eng.close()
    dist.destroy_process_group()
    sys.exit(0 if res["ok"] else 1)


if __name__ == "__main__":
    main()
