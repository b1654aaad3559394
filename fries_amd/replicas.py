"""Independent replicas of one frisys_mol run on one MI355X, and the replica estimator between them.

A FRI run is one Markov chain; error bars, and any estimator built from two uncorrelated vectors, need several.  ``FriReplicas``
holds ``n`` engines with seeds ``seed, seed + 1, ...``; each has its own context and HIP stream, so their fused loops run side by
side from one Python thread each (ctypes releases the GIL for the length of a call).  Replica ``r`` computes exactly what a lone
``FriEngine`` with seed ``seed + r`` computes.  ``pair_estimates`` evaluates ``fries_h_dot`` (the reference's calc_h_dot as
obs_repl_mol uses it) for every pair of replicas, ``pair_rdm1`` the one-body density matrix ``fries_rdm1``,
``pair_rdm2`` the two-body density matrix ``fries_rdm2``.
"""
from __future__ import annotations

import threading

from .engine import FriEngine


class FriReplicas:
    def __init__(self, mol, n: int, seed: int, device: int = 0, **setup_kwargs):
        """n engines on `device`, replica r set up with FriEngine.setup(seed=seed + r, **setup_kwargs)."""
        if n < 1:
            raise ValueError("FriReplicas needs at least one replica")
        if "seed" in setup_kwargs:
            raise TypeError("the seed is FriReplicas' own argument: replica r runs with seed + r")
        self.engines = []
        try:
            for r in range(n):
                e = FriEngine(mol, device=device)
                self.engines.append(e)
                e.setup(seed=seed + r, **setup_kwargs)
        except Exception:
            self.close()
            raise

    def iterate(self, k: int):
        """k iterations of every replica, concurrently; returns the per-replica logs (FriEngine.iterate's records)."""
        logs = [None] * len(self.engines)
        errs = [None] * len(self.engines)

        def run(r):
            try:
                logs[r] = self.engines[r].iterate(k)
            except BaseException as ex:     # handed to the caller below
                errs[r] = ex

        threads = [threading.Thread(target=run, args=(r,)) for r in range(1, len(self.engines))]
        for t in threads:
            t.start()
        run(0)
        for t in threads:
            t.join()
        for ex in errs:
            if ex is not None:
                raise ex
        return logs

    def _pairwise(self, call, back=None):
        """call(a, b) for all pairs r < s, in the order of pairs().  The replica with fewer stored determinants is a, the enumerating
        side (a tie goes to r); where that is s, back(result) turns the result into that of (r, s)."""
        sizes = [e.vec_info()[1] for e in self.engines]
        out = []
        for r, s in self.pairs():
            if sizes[r] <= sizes[s]:
                out.append(call(self.engines[r], self.engines[s]))
            else:
                res = call(self.engines[s], self.engines[r])
                out.append(back(res) if back else res)
        return out

    def pair_estimates(self):
        """fries_h_dot for all pairs r < s, in the order of pairs(): a list of HDot.  The replica with fewer stored determinants
        is the enumerating side (H is symmetric, so the estimate is the same up to rounding; a tie goes to r)."""
        return self._pairwise(lambda a, b: a.h_dot(b))

    def pair_rdm1(self):
        """fries_rdm1 for all pairs r < s, in the order of pairs(): a list of Rdm1 whose gamma is always gamma(r, s).  The replica with
        fewer stored determinants enumerates (a tie goes to r); where that is s, the matrix is transposed back."""
        return self._pairwise(lambda a, b: a.rdm1(b), lambda x: x.transposed())

    def pair_rdm2(self):
        """fries_rdm2 for all pairs r < s, in the order of pairs(): a list of Rdm2 whose gamma2 is always gamma2(r, s).  The replica with
        fewer stored determinants enumerates (a tie goes to r); where that is s, the result is transposed back ([p,q,r,s] -> [q,p,s,r])."""
        return self._pairwise(lambda a, b: a.rdm2(b), lambda x: x.transposed())

    def pairs(self):
        """(0,1), (0,2), ..., (1,2), ...: the pairs pair_estimates() reports, in its order."""
        n = len(self.engines)
        return [(r, s) for r in range(n) for s in range(r + 1, n)]

    def close(self):
        for e in self.engines:
            e.close()
        self.engines = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
