"""Independent replicas of one frisys_mol run on one MI355X, and the replica estimator between them.

A FRI run is one Markov chain; error bars, and any estimator built from two uncorrelated vectors, need several.  ``FriReplicas``
holds ``n`` engines with seeds ``seed, seed + 1, ...``; each has its own context and HIP stream, so their fused loops run side by
side from one Python thread each (ctypes releases the GIL for the length of a call).  Replica ``r`` computes exactly what a lone
``FriEngine`` with seed ``seed + r`` computes.  ``pair_estimates`` evaluates ``fries_h_dot`` (the reference's calc_h_dot as
obs_repl_mol uses it) for every pair of replicas, ``pair_rdm1`` the one-body density matrix ``fries_rdm1``,
``pair_rdm2`` the two-body density matrix ``fries_rdm2``.

With ``ranks > 1`` every replica is a hash-sharded run of ``ranks`` engines over the native local transport
(``fries_amd.comm.LocalGroup``), each rank driven from its own thread, and the three ``pair_*`` calls go through ``VecSnapshot``:
the probed replica is frozen into one look-up table on the enumerating replica's device, and the enumerating replica's shards run
the same kernels against it one after the other (``fries_*_ranks``).
"""
from __future__ import annotations

import threading

from .engine import FriEngine, VecSnapshot


def _in_threads(jobs):
    """jobs[0] on the calling thread, the others on a thread each; the first exception (in job order) is raised once all have ended"""
    errs = [None] * len(jobs)

    def run(j):
        try:
            jobs[j]()
        except BaseException as ex:     # handed to the caller below
            errs[j] = ex

    threads = [threading.Thread(target=run, args=(j,)) for j in range(1, len(jobs))]
    for t in threads:
        t.start()
    run(0)
    for t in threads:
        t.join()
    for ex in errs:
        if ex is not None:
            raise ex


class FriReplicas:
    def __init__(self, mol, n: int, seed: int, device: int = 0, ranks: int = 1, devices=None, **setup_kwargs):
        """n replicas, replica r set up with FriEngine.setup(seed=seed + r, **setup_kwargs).  ranks == 1: one engine per replica on
        `device`.  ranks > 1: replica r is a LocalGroup of `ranks` engines (vec_nonz / mat_nonz / target_norm are then global, max_dets
        is per rank).  devices: the device of every replica (n entries; default `device` for all) -- the ranks of one replica share a
        device, because the estimators over ranks want the enumerating side in one place.
        engines: every engine, replica-major; shards[r]: the engines of replica r in rank order.
        The set-up and the iterations of a sharded replica hold collectives.  The ranks of a replica get the same arguments, so a call
        that is refused is refused on all of them; a rank that fails alone (a device error, an exhausted capacity) leaves its partners
        waiting in their next collective, as it does for any rank-thread host of the local transport: such a call does not return."""
        if n < 1:
            raise ValueError("FriReplicas needs at least one replica")
        if ranks < 1:
            raise ValueError("FriReplicas needs at least one rank per replica")
        if "seed" in setup_kwargs:
            raise TypeError("the seed is FriReplicas' own argument: replica r runs with seed + r")
        if ranks > 1 and "mat_nonz" not in setup_kwargs:
            raise TypeError("FriReplicas with ranks > 1 needs mat_nonz among the set-up arguments: it sizes the ranks' exchange buffers")
        devices = [device] * n if devices is None else list(devices)
        if len(devices) != n:
            raise ValueError("devices names one device per replica")
        self.ranks = ranks
        self.engines, self.shards, self.groups = [], [], []
        try:
            if ranks == 1:
                for r in range(n):
                    e = FriEngine(mol, device=devices[r])
                    self.engines.append(e)
                    self.shards.append([e])
                    e.setup(seed=seed + r, **setup_kwargs)
            else:
                from .comm import LocalGroup
                for r in range(n):
                    grp = LocalGroup(ranks, setup_kwargs["mat_nonz"])
                    self.groups.append(grp)
                    sh = [FriEngine(mol, device=devices[r], comm=grp.comm(k, devices[r])) for k in range(ranks)]
                    self.engines.extend(sh)
                    self.shards.append(sh)
                # the set-up of a sharded run holds collectives: every rank on its own thread
                _in_threads([(lambda e=e, r=r: e.setup(seed=seed + r, **setup_kwargs)) for r, sh in enumerate(self.shards) for e in sh])
        except Exception:
            self.close()
            raise

    def iterate(self, k: int):
        """k iterations of every replica, concurrently; returns the per-replica logs (FriEngine.iterate's records; with ranks > 1 a
        list of every rank's)."""
        logs = [[None] * len(sh) for sh in self.shards]

        def job(r, j):
            def go():
                logs[r][j] = self.shards[r][j].iterate(k)
            return go

        _in_threads([job(r, j) for r, sh in enumerate(self.shards) for j in range(len(sh))])
        return [lg[0] for lg in logs] if self.ranks == 1 else logs

    _BACK = {"h_dot": None, "rdm1": lambda x: x.transposed(), "rdm2": lambda x: x.transposed()}

    def _pairwise(self, kinds):
        """{kind: [result per pair]} for the estimators named in `kinds` ("h_dot", "rdm1", "rdm2": the methods of FriEngine and of
        VecSnapshot), for all pairs r < s in the order of pairs().  The replica with fewer stored determinants is a, the enumerating
        side (a tie goes to r); where that is s, the result is turned into that of (r, s) (H is symmetric; the density matrices are
        transposed back).  ranks == 1: the two-context calls on the engines.  ranks > 1: the probed replica is a VecSnapshot on a's
        device -- one per (replica, device) for the whole call, serving every estimator asked for and every partner, closed at the end."""
        sizes = [sum(e.vec_info()[1] for e in sh) for sh in self.shards]
        out, snaps = {k: [] for k in kinds}, {}
        try:
            for r, s in self.pairs():
                a, b = (r, s) if sizes[r] <= sizes[s] else (s, r)
                if self.ranks == 1:
                    probed, arg = self.shards[a][0], self.shards[b][0]
                else:
                    dev = self.shards[a][0].device
                    if (b, dev) not in snaps:
                        snaps[(b, dev)] = VecSnapshot(self.shards[b], device=dev)
                    probed, arg = snaps[(b, dev)], self.shards[a]
                for k in kinds:
                    res = getattr(probed, k)(arg)
                    back = self._BACK[k]
                    out[k].append(res if a == r or back is None else back(res))
        finally:
            for sn in snaps.values():
                sn.close()
        return out

    def pair_estimates(self):
        """fries_h_dot for all pairs r < s, in the order of pairs(): a list of HDot.  The replica with fewer stored determinants
        is the enumerating side (H is symmetric, so the estimate is the same up to rounding; a tie goes to r)."""
        return self._pairwise(["h_dot"])["h_dot"]

    def pair_rdm1(self):
        """fries_rdm1 for all pairs r < s, in the order of pairs(): a list of Rdm1 whose gamma is always gamma(r, s).  The replica with
        fewer stored determinants enumerates (a tie goes to r); where that is s, the matrix is transposed back."""
        return self._pairwise(["rdm1"])["rdm1"]

    def pair_rdm2(self):
        """fries_rdm2 for all pairs r < s, in the order of pairs(): a list of Rdm2 whose gamma2 is always gamma2(r, s).  The replica with
        fewer stored determinants enumerates (a tie goes to r); where that is s, the result is transposed back ([p,q,r,s] -> [q,p,s,r])."""
        return self._pairwise(["rdm2"])["rdm2"]

    def pair_all(self):
        """(pair_estimates(), pair_rdm1(), pair_rdm2()) of one meeting: with ranks > 1 every snapshot is built once and serves all three
        estimators; the results are the bits the three calls return one by one."""
        out = self._pairwise(["h_dot", "rdm1", "rdm2"])
        return out["h_dot"], out["rdm1"], out["rdm2"]

    def pairs(self):
        """(0,1), (0,2), ..., (1,2), ...: the pairs pair_estimates() reports, in its order."""
        n = len(self.shards)
        return [(r, s) for r in range(n) for s in range(r + 1, n)]

    def close(self):
        for e in self.engines:
            e.close()
        for g in self.groups:
            g.destroy()
        self.engines, self.shards, self.groups = [], [], []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
