"""Excited states: the reference's subspace iteration (FRIES_bin/subsp_mol.cpp:398-631) over several engines.

``FriSubspace`` iterates one vector per state, measures D = T^T X and H = T^T H X against fixed trial vectors every iteration and, every
``restart_int`` iterations, replaces X by X R^-1 with R the triangular factor of D - eps H.  The reference keeps all states as columns of
one DistVec; here a vector has two value columns throughout the merge, the compressions and the exchange, so every state is a
``FriEngine`` of its own and the one step that mixes states is a device axpy from a frozen snapshot of one state into another
(fries_vec_axpy_snapshot).  Everything else is a device operator that existed: compress_vec_piv, apply_hbpp_piv, spawn_from_comp,
death_clone with shift 0, vec_dot_list.

What this is not:
  * The states do not share an index set.  A determinant leaves a state's vector when that state's compression drops it, not when all
    states' do, and the compressions walk each vector in its own position order.  The trajectories are therefore not the reference's
    bit for bit, and no golden trajectory from subsp_mol exists for it.
  * No time reversal, no subspfull_mol (H applied in full), no --load_dir, no C++ driver (it would need a QR of its own), no ranks.

The small linear algebra (``rinv``, ``gen_eigvals``, ``adjust_shift2``) and ``dense_model``, the same loop for a dense matrix with
every compression the identity and H x a matrix product, are plain numpy and need no GPU.
"""
from __future__ import annotations

import numpy as np

SHIFT_DAMPING = 0.5         # subsp_mol.cpp:55-56
SHIFT_INTERVAL = 1
INITIAL_NORM = 1000.0       # :389-396: every state starts at one-norm 1000


# ---------------------------------------------------------------------------------------------- host arithmetic
def adjust_shift2(norm_factor, one_norm, last_norm, damp=SHIFT_DAMPING):
    """compress_utils.cpp:695-700 -> (new norm factor, new last norm)"""
    new_factor = norm_factor ** (1 - damp) * (one_norm / last_norm) ** damp
    new_last = last_norm ** damp * (one_norm / norm_factor) ** (1 - damp)
    return new_factor, new_last


def rinv(mat):
    """invr_inplace (LAPACK/lapack_wrappers.cpp:140-): the inverse of the R factor of mat = Q R, so that mat @ rinv(mat) = Q has
    orthonormal columns.  The sign convention of R's diagonal is the QR routine's own."""
    mat = np.asarray(mat)
    r = np.linalg.qr(mat.astype(np.float64), mode="r")
    n = r.shape[0]
    out = np.zeros((n, n))
    for k in range(n):                  # back substitution, column by column: R out[:, k] = e_k
        out[k, k] = 1.0 / r[k, k]
        for j in range(k - 1, -1, -1):
            out[j, k] = -np.dot(r[j, j + 1:k + 1], out[j + 1:k + 1, k]) / r[j, j]
    return out


def gen_eigvals(d_mat, h_mat):
    """The generalised eigenvalues of H c = lambda D c, ascending (real parts: D and H are projections of a symmetric problem)"""
    ev = np.linalg.eigvals(np.linalg.solve(np.asarray(d_mat, dtype=np.float64), np.asarray(h_mat, dtype=np.float64)))
    return np.sort(ev.real)


def averaged_energies(d_mats, h_mats, burn_in, offset=0.0):
    d = np.mean(np.asarray(d_mats, dtype=np.float64)[burn_in:], axis=0)
    h = np.mean(np.asarray(h_mats, dtype=np.float64)[burn_in:], axis=0)
    return gen_eigvals(d, h) + offset


def restart_mix(x, r_inv):
    """x_k <- x_k * Rinv[k][k] + sum over j != k, ascending, of x_j * Rinv[j][k]: the order FriSubspace's restart adds in"""
    n = x.shape[1]
    out = np.empty_like(x)
    for k in range(n):
        col = x[:, k] * r_inv[k, k]
        for j in range(n):
            if j != k:
                col = col + x[:, j] * r_inv[j, k]
        out[:, k] = col
    return out


def dense_model(h, trials, n_iter, *, epsilon, restart_int, dtype=np.float64, record=None):
    """The loop of FriSubspace.iterate for a dense matrix h (symmetric up to rounding; the diagonal offset already subtracted) and trial vectors
    trials[k] (rows), with every compression the identity and H x a matrix product -> (d_mats, h_mats), [n_iter, n, n] each, in
    `dtype`.  The small inverse is formed in float64 whatever the dtype, as the loop on the device forms it.
    record: a list that receives, per restart, (iteration, D - eps H before, R^-1, norms before, norms after the mixing)."""
    h = np.asarray(h, dtype=dtype)
    t = np.asarray(trials, dtype=dtype)
    n = t.shape[0]
    eps = dtype(epsilon)
    ht = t @ h.T                                 # rows: H trial_k
    x = t.T.copy()
    for k in range(n):
        x[:, k] *= dtype(INITIAL_NORM) / np.sum(np.abs(x[:, k]))
    factors = [1.0] * n
    last = [0.0] * n
    d_mats, h_mats = np.zeros((n_iter, n, n), dtype=dtype), np.zeros((n_iter, n, n), dtype=dtype)
    for it in range(n_iter):
        norms = [float(np.sum(np.abs(x[:, k]))) for k in range(n)]
        if it == 0:
            last = list(norms)
        if (it + 1) % SHIFT_INTERVAL == 0:
            for k in range(n):
                factors[k], last[k] = adjust_shift2(factors[k], norms[k], last[k])
        for k in range(n):
            x[:, k] *= dtype(1.0 / factors[k])
        d_mats[it] = t @ x
        h_mats[it] = ht @ x
        if (it + 1) % restart_int == 0:
            m = d_mats[it] - eps * h_mats[it]
            r_inv = rinv(m)
            before = np.sum(np.abs(x), axis=0)
            x = restart_mix(x, r_inv.astype(dtype))
            after = np.sum(np.abs(x), axis=0)
            if record is not None:
                record.append((it, np.array(m, dtype=np.float64), r_inv, np.array(before, dtype=np.float64), np.array(after, dtype=np.float64)))
            for k in range(n):
                x[:, k] *= before[k] / after[k]
        x = x - eps * (h @ x)
    return d_mats, h_mats


def dense_h(mol, dets, device=0):
    """H in the span of a determinant list as a dense matrix, from the engine's own matrix elements (matrel for the diagonal,
    h_offdiag_list for a column): needs a GPU."""
    from .engine import FriEngine
    dets = np.ascontiguousarray(dets, dtype=np.uint64)
    index = {int(d): i for i, d in enumerate(dets)}
    if len(index) != dets.size:
        raise ValueError("a determinant is listed twice")
    eng = FriEngine(mol, device=device)
    try:
        eng.setup(epsilon=0.01, vec_nonz=10, mat_nonz=10, max_dets=100, distribution="HB_unnorm")
        h = np.diag(eng.matrel(0, dets)[0])
        for j, d in enumerate(dets):
            od, ov = eng.h_offdiag_list(dets[j:j + 1], np.ones(1))
            for x, v in zip(od, ov):
                i = index.get(int(x))
                if i is not None and i != j:
                    h[i, j] = v
    finally:
        eng.close()
    return h


# ---------------------------------------------------------------------------------------------- the loop on the device
class FriSubspace:
    """subsp_mol's loop over one FriEngine per state.  trials: a list of (dets, vals), one per state; state k takes trial k as its trial
    and its initial vector and seed + k as its seed.  d_mats / h_mats: the matrices of every iteration so far.  One rank per state: there
    is no `ranks` or `comm` argument, and passing one raises (TypeError)."""

    def __init__(self, mol, trials, *, epsilon, vec_nonz, mat_nonz, max_dets, restart_int, initiator=0.0, seed=0, device=0):
        from .engine import FriEngine
        if not trials:
            raise ValueError("at least one trial vector is needed")
        if restart_int < 1:
            raise ValueError("restart_int must be at least 1")
        self.mol, self.eps, self.restart_int = mol, float(epsilon), int(restart_int)
        self.vec_nonz, self.mat_nonz, self.initiator = int(vec_nonz), int(mat_nonz), float(initiator)
        self.trials = [(np.ascontiguousarray(d, dtype=np.uint64), np.ascontiguousarray(v, dtype=np.float64)) for d, v in trials]
        self.engines = []
        try:
            for k, tr in enumerate(self.trials):
                eng = FriEngine(mol, device=device)
                self.engines.append(eng)
                eng.setup(epsilon=epsilon, vec_nonz=vec_nonz, mat_nonz=mat_nonz, max_dets=max_dets, initiator=initiator, seed=seed + k,
                          distribution="HB_unnorm", trial=tr, ini=tr)
            # every engine's own trial list and H times it, read once
            self.htrials = [eng.htrial() for eng in self.engines]
            for eng in self.engines:        # subsp_mol.cpp:389-396
                eng.scale(0, INITIAL_NORM / eng.one_norm(0))
        except Exception:
            self.close()
            raise
        n = len(self.engines)
        self.hf_energy = self.engines[0].hf_energy
        self.norm_factors = [1.0] * n
        self.last_norms = [0.0] * n
        self.iteration = 0
        self.d_mats, self.h_mats = [], []
        self.restarts = []      # per restart: (iteration, D - eps H, R^-1, norms before, norms after the mixing)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        for eng in self.engines:
            eng.close()
        self.engines = []

    def measure(self):
        """(d_mat, h_mat) of the states as they stand: d_mat[t][v] = <trial_t|x_v>, h_mat[t][v] = <H trial_t|x_v> (fries_vec_dot_list)"""
        n = len(self.engines)
        d_mat, h_mat = np.zeros((n, n)), np.zeros((n, n))
        for t in range(n):
            (td, tv), (hd, hv) = self.trials[t], self.htrials[t]
            for v, eng in enumerate(self.engines):
                d_mat[t, v] = eng.dot_list(0, td, tv)
                h_mat[t, v] = eng.dot_list(0, hd, hv)
        return d_mat, h_mat

    def _restart(self, d_mat, h_mat):
        from .engine import VecSnapshot
        m = d_mat - self.eps * h_mat
        r_inv = rinv(m)
        before = [eng.one_norm(0) for eng in self.engines]
        snaps = [VecSnapshot([eng]) for eng in self.engines]
        try:
            for k, eng in enumerate(self.engines):
                eng.scale(0, float(r_inv[k, k]))
                for j, snap in enumerate(snaps):
                    if j != k:
                        eng.axpy_snapshot(0, float(r_inv[j, k]), snap)
        finally:
            for snap in snaps:
                snap.close()
        after = [eng.one_norm(0) for eng in self.engines]
        for k, eng in enumerate(self.engines):          # :502-509
            eng.scale(0, before[k] / after[k])
        self.restarts.append((self.iteration, m, r_inv, np.array(before), np.array(after)))

    def iterate(self, n_iter: int):
        """n_iter iterations of subsp_mol.cpp:398-631; returns the (d_mats, h_mats) of these iterations as arrays."""
        first = len(self.d_mats)
        for _ in range(n_iter):
            it = self.iteration
            norms = [eng.one_norm(0) for eng in self.engines]                          # :403-407
            if it == 0:
                self.last_norms = list(norms)
            if (it + 1) % SHIFT_INTERVAL == 0:                                         # :412-415
                for k in range(len(norms)):
                    self.norm_factors[k], self.last_norms[k] = adjust_shift2(self.norm_factors[k], norms[k], self.last_norms[k])
            for k, eng in enumerate(self.engines):                                     # :431-436
                eng.scale(0, 1.0 / self.norm_factors[k])
            d_mat, h_mat = self.measure()                                             # :439-452
            self.d_mats.append(d_mat)
            self.h_mats.append(h_mat)
            if (it + 1) % self.restart_int == 0:                                       # :480-510
                self._restart(d_mat, h_mat)
            for eng in self.engines:                                                   # :513
                eng.compress_vec_piv(self.vec_nonz)
            for eng in self.engines:                                                   # :516-630
                one_norm = eng.one_norm(0)
                size_before = eng.vec_info()[0]
                eng.apply_hbpp_piv_device(self.mat_nonz)
                eng.spawn_from_comp(self.eps, self.initiator * one_norm / self.mat_nonz)
                eng.death_clone(self.eps, 0.0, size_before)
            self.iteration += 1
        return np.array(self.d_mats[first:]), np.array(self.h_mats[first:])

    def energies(self, burn_in: int = 0):
        """The generalised eigenvalues of the matrices averaged from iteration burn_in on, plus the run's offset (hf_energy), ascending"""
        if burn_in >= len(self.d_mats):
            raise ValueError("burn_in leaves no iteration to average")
        return averaged_energies(self.d_mats, self.h_mats, burn_in, self.hf_energy)

    @staticmethod
    def trials_from_dets(mol, dets, n, device=0):
        """The n lowest eigenvectors of H in the span of a determinant list, as a list of (dets, vals) (needs a GPU: dense_h)"""
        dets = np.ascontiguousarray(dets, dtype=np.uint64)
        if not 0 < n <= dets.size:
            raise ValueError("n must be between 1 and the number of determinants")
        _, vec = np.linalg.eigh(dense_h(mol, dets, device))
        return [(dets.copy(), np.ascontiguousarray(vec[:, k])) for k in range(n)]
