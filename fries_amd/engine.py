"""Host-side mirror of the reference's driver surface over the C ABI (include/fries_hip.h).

``FriEngine`` plays the role of frisys_mol's ``main`` (FRIES_bin/frisys_mol.cpp): it owns a
context, hands it the parsed FCIDUMP, and runs the iteration loop on the MI355X.  There is no
CPU path: importing works anywhere, creating an engine without libfries_hip.so or without a
HIP device raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FRIES_LIB") or os.path.join(_HERE, "libfries_hip.so")      # FRIES_LIB: another build of the same library (A/B timing of kernel variants)

# every symbol include/fries_hip.h declares
EXPORTS = [
    "fries_last_error", "fries_device_count", "fries_ctx_create", "fries_ctx_destroy", "fries_set_molecule",
    "fries_get_hb_tensor", "fries_set_hb_tensor", "fries_hf_energy", "fries_matrel_batch", "fries_frisys_setup",
    "fries_frisys_iterate", "fries_p_doub", "fries_kernel_launches", "fries_vec_info", "fries_vec_download",
    "fries_vec_add", "fries_vec_load", "fries_htrial_download", "fries_apply_hbpp_sys", "fries_apply_hbpp_piv", "fries_rng_set_state", "fries_rng_get_state", "fries_compress_vec",
    "fries_test_teeth", "fries_test_seqsum", "fries_frisys_restart", "fries_prof_enable", "fries_prof_count", "fries_prof_get", "fries_counters",
    "fries_set_comm", "fries_stream", "fries_idx_to_proc", "fries_hh_setup", "fries_hh_iterate", "fries_get_scramblers", "fries_fciqmc_setup", "fries_fciqmc_iterate", "fries_frimulti_setup", "fries_frimulti_iterate",
    "fries_compress_vec_piv", "fries_next_draw", "fries_test_piv_adjust", "fries_frifull_setup", "fries_frifull_iterate",
    "fries_rccl_unique_id", "fries_rccl_create", "fries_local_group_create", "fries_local_group_destroy", "fries_local_create", "fries_transport_comm", "fries_transport_counts", "fries_transport_destroy",
    "fries_set_proc_scrambler", "fries_tie_margins", "fries_measure_copy_bandwidth", "fries_piv_stats", "fries_set_trial_vector", "fries_set_initial_vector", "fries_set_ham_shift", "fries_vec_add_to", "fries_death_clone", "fries_dots", "fries_find_preserve", "fries_sys_comp",
    "fries_vec_column_download", "fries_vec_column_upload", "fries_vec_column_zero", "fries_vec_diag_download", "fries_vec_dot_list", "fries_vec_add_vecs", "fries_set_det_space", "fries_vec_set_dense", "fries_dense_sizes", "fries_hostcomm_create", "fries_set_vec_scrambler", "fries_hh_comp_sub", "fries_hh_ref_ovlp", "fries_set_spin_parity", "fries_h_offdiag_list",
    "fries_spawn_from_comp", "fries_dense_apply", "fries_dense_norm", "fries_dense_h_count", "fries_comp_download",
    "fries_h_dot", "fries_rdm1", "fries_rdm2",
    "fries_snapshot_create", "fries_snapshot_info", "fries_snapshot_vector", "fries_snapshot_destroy", "fries_h_dot_ranks", "fries_rdm1_ranks", "fries_rdm2_ranks",
    "fries_vec_axpy_snapshot", "fries_snapshot_dot", "fries_vec_scale", "fries_vec_one_norm",
]


class FrisysParams(C.Structure):
    _fields_ = [("epsilon", C.c_double), ("target_norm", C.c_double), ("initiator", C.c_double),
                ("vec_nonz", C.c_uint32), ("mat_nonz", C.c_uint32), ("max_dets", C.c_uint32),
                ("seed", C.c_uint32), ("hb_unnorm", C.c_int32)]


class FrifullParams(C.Structure):
    _fields_ = [("epsilon", C.c_double), ("target_norm", C.c_double), ("vec_nonz", C.c_uint32), ("max_dets", C.c_uint32),
                ("seed", C.c_uint32), ("spawn_cap", C.c_uint32)]


class HHParams(C.Structure):
    """struct fries_hh_params"""
    _fields_ = [("n_elec", C.c_uint32), ("n_sites", C.c_uint32), ("eps", C.c_double), ("U", C.c_double), ("omega", C.c_double), ("g", C.c_double),
                ("gs_energy", C.c_double), ("target_norm", C.c_double), ("initiator", C.c_double), ("vec_nonz", C.c_uint32), ("max_dets", C.c_uint32),
                ("seed", C.c_uint32), ("full", C.c_uint32)]


class FrimultiParams(C.Structure):
    """struct fries_frimulti_params"""
    _fields_ = [("epsilon", C.c_double), ("target_norm", C.c_double), ("initiator", C.c_double), ("vec_nonz", C.c_uint32), ("mat_nonz", C.c_uint32),
                ("max_dets", C.c_uint32), ("seed", C.c_uint32)]


class FciqmcParams(C.Structure):
    """struct fries_fciqmc_params"""
    _fields_ = [("epsilon", C.c_double), ("target_walkers", C.c_uint32), ("initiator", C.c_uint32), ("max_dets", C.c_uint32), ("seed", C.c_uint32),
                ("heat_bath", C.c_int32), ("real_walkers", C.c_int32)]


FCIQMC_LOG_DTYPE = np.dtype([("numer", "f8"), ("denom", "f8"), ("shift", "f8"), ("norm", "f8"), ("n_nonz", "i4"), ("n_ini", "u4"), ("curr_size", "u4"),
                             ("n_spawn", "u4"), ("n_attempts", "u4"), ("err", "u4")], align=True)


class IterLog(C.Structure):
    _fields_ = [("numer", C.c_double), ("denom", C.c_double), ("shift", C.c_double), ("norm", C.c_double),
                ("nkept", C.c_uint32), ("n_nonz", C.c_int32), ("curr_size", C.c_uint32), ("num_success", C.c_uint32),
                ("comp_len", C.c_uint32 * 5), ("err", C.c_uint32)]


class HdotResult(C.Structure):
    """struct fries_hdot_result"""
    _fields_ = [("h", C.c_double), ("ovlp", C.c_double), ("abs_sum", C.c_double), ("n_src", C.c_uint64), ("n_terms", C.c_uint64), ("n_hits", C.c_uint64)]


class HDot(NamedTuple):
    """fries_h_dot's result: h = <a|H|b>, ovlp = <a|b>, abs_sum = the sum of the magnitudes of h's terms; the counts of sources,
    non-zero excitations and excitations found in b."""
    h: float
    ovlp: float
    abs_sum: float
    n_src: int
    n_terms: int
    n_hits: int

    @property
    def energy(self) -> float:
        return self.h / self.ovlp


class Rdm1Result(C.Structure):
    """struct fries_rdm1_result and, with the same fields, struct fries_rdm2_result"""
    _fields_ = [("ovlp", C.c_double), ("abs_sum", C.c_double), ("n_src", C.c_uint64), ("n_terms", C.c_uint64), ("n_hits", C.c_uint64)]


Rdm2Result = Rdm1Result


class Rdm1(NamedTuple):
    """fries_rdm1's result: gamma[p, q] = <a| sum_sigma c+_{p sigma} c_{q sigma} |b> (an [n_orb, n_orb] array, the number operator on the
    diagonal), ovlp = <a|b>, abs_sum = the sum of the magnitudes of the off-diagonal terms; the counts of sources, probes and probes
    that found a non-zero value in b."""
    gamma: np.ndarray
    ovlp: float
    abs_sum: float
    n_src: int
    n_terms: int
    n_hits: int

    def expectation(self, op) -> float:
        """<a| O |b> / <a|b> of the one-electron operator with the [n_orb, n_orb] matrix op[p, q] = <p|o|q>."""
        op = np.asarray(op, dtype=np.float64)
        if op.shape != self.gamma.shape:
            raise ValueError(f"the operator matrix must have shape {self.gamma.shape}")
        return float(np.sum(op * self.gamma) / self.ovlp)

    def natural_occupations(self) -> np.ndarray:
        """Eigenvalues of the symmetrised, normalised density matrix (gamma + gamma.T) / (2 ovlp), descending."""
        return np.linalg.eigvalsh((self.gamma + self.gamma.T) / (2.0 * self.ovlp))[::-1].copy()

    def transposed(self) -> "Rdm1":
        """gamma(b, a) from gamma(a, b): the matrix transposed, everything else as it is."""
        return self._replace(gamma=np.ascontiguousarray(self.gamma.T))


class Rdm2(NamedTuple):
    """fries_rdm2's result: gamma2[p, q, r, s] = sum over sigma, tau of <a| c+_{p sigma} c+_{r tau} c_{s tau} c_{q sigma} |b> (chemists'
    order, an [n_orb] * 4 array), ovlp = <a|b>, abs_sum = the sum of |a_i b_j| over the hits; the counts of sources, probes and probes
    that found a non-zero value in b.  The methods are host arithmetic on the array."""
    gamma2: np.ndarray
    ovlp: float
    abs_sum: float
    n_src: int
    n_terms: int
    n_hits: int

    def transposed(self) -> "Rdm2":
        """gamma2(b, a) from gamma2(a, b): the adjoint, [p, q, r, s] -> [q, p, s, r]; everything else as it is."""
        return self._replace(gamma2=np.ascontiguousarray(self.gamma2.transpose(1, 0, 3, 2)))

    def partial_trace(self, n_elec: int) -> np.ndarray:
        """sum_r gamma2[p, q, r, r] / (n_elec - 1): the one-body density matrix gamma[p, q] of fries_rdm1, up to rounding."""
        return np.einsum("pqrr->pq", self.gamma2) / (n_elec - 1)

    def expectation(self, op4) -> float:
        """<a| O |b> / <a|b> of the two-electron operator 1/2 sum op4[p, q, r, s] c+_p c+_r c_s c_q (chemists' order, spin-summed)."""
        op4 = np.asarray(op4, dtype=np.float64)
        if op4.shape != self.gamma2.shape:
            raise ValueError(f"the operator array must have shape {self.gamma2.shape}")
        return float(0.5 * np.sum(op4 * self.gamma2) / self.ovlp)

    def energy(self, h_core, eri4, gamma1) -> float:
        """(sum(h_core * gamma1) + 1/2 sum(eri4 * gamma2)) / ovlp with eri4[p, q, r, s] = (pq|rs) and gamma1 the matrix of fries_rdm1
        for the same pair: the total electronic energy <a|H|b> / <a|b>."""
        h_core, eri4, gamma1 = (np.asarray(x, dtype=np.float64) for x in (h_core, eri4, gamma1))
        if eri4.shape != self.gamma2.shape or h_core.shape != self.gamma2.shape[:2] or gamma1.shape != h_core.shape:
            raise ValueError(f"h_core and gamma1 must have shape {self.gamma2.shape[:2]}, eri4 {self.gamma2.shape}")
        return float((np.sum(h_core * gamma1) + 0.5 * np.sum(eri4 * self.gamma2)) / self.ovlp)

    def spin_squared(self, n_elec: int) -> float:
        """<S^2> = -N (N - 4) / 4 - 1/2 sum_pq gamma2[p, q, q, p] / ovlp"""
        return float(-n_elec * (n_elec - 4) / 4.0 - 0.5 * np.einsum("pqqp->", self.gamma2) / self.ovlp)


class VdotResult(C.Structure):
    """struct fries_vdot_result"""
    _fields_ = [("dot", C.c_double), ("abs_sum", C.c_double), ("n_src", C.c_uint64), ("n_hits", C.c_uint64)]


class VDot(NamedTuple):
    """fries_snapshot_dot's result: dot = <a|snapshot>, abs_sum = the sum of the magnitudes of its products; the positions of a with a
    non-zero value and those of them found in the snapshot with a non-zero value."""
    dot: float
    abs_sum: float
    n_src: int
    n_hits: int


class SnapshotInfoStruct(C.Structure):
    """struct fries_snapshot_info_t"""
    _fields_ = [("n_entries", C.c_uint64), ("n_shards", C.c_uint32), ("n_slots", C.c_uint32), ("device_bytes", C.c_uint64), ("device", C.c_int32),
                ("ms_compact", C.c_float), ("ms_copy", C.c_float), ("ms_insert", C.c_float)]


class SnapshotInfo(NamedTuple):
    """fries_snapshot_info's result: the entries, the shards they came from, the look-up table's slots, the device bytes the snapshot owns,
    its device, and what compaction (summed over the shards), copy and insert took on the device, in milliseconds."""
    n_entries: int
    n_shards: int
    n_slots: int
    device_bytes: int
    device: int
    ms_compact: float
    ms_copy: float
    ms_insert: float


ITERLOG_DTYPE = np.dtype([("numer", "f8"), ("denom", "f8"), ("shift", "f8"), ("norm", "f8"), ("nkept", "u4"), ("n_nonz", "i4"),
                          ("curr_size", "u4"), ("num_success", "u4"), ("comp_len", "u4", (5,)), ("err", "u4")], align=True)

_lib = None


def load_library() -> C.CDLL:
    """Loads libfries_hip.so; raises if it has not been built (no fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
                           "The FRI engine has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    lib.fries_last_error.restype = C.c_char_p
    lib.fries_hf_energy.restype = C.c_double
    lib.fries_p_doub.restype = C.c_double
    lib.fries_kernel_launches.restype = C.c_uint64
    lib.fries_ctx_destroy.restype = None
    for name in ("fries_hf_energy", "fries_p_doub", "fries_kernel_launches", "fries_ctx_destroy"):
        getattr(lib, name).argtypes = [C.c_void_p]
    lib.fries_ctx_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    lib.fries_set_molecule.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.fries_get_hb_tensor.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.fries_set_hb_tensor.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    lib.fries_matrel_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.fries_frisys_setup.argtypes = [C.c_void_p, C.POINTER(FrisysParams)]
    lib.fries_frisys_iterate.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.fries_vec_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
    lib.fries_vec_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.fries_htrial_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.fries_vec_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.fries_vec_column_download.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.fries_vec_column_upload.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    lib.fries_vec_column_zero.argtypes = [C.c_void_p, C.c_int]
    lib.fries_vec_add_vecs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double]
    lib.fries_set_det_space.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.fries_vec_diag_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.fries_vec_dot_list.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_double)]
    lib.fries_vec_load.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.fries_rng_set_state.argtypes = [C.c_void_p, C.c_char_p]
    lib.fries_rng_get_state.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.fries_apply_hbpp_piv.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.fries_apply_hbpp_sys.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.POINTER(C.c_size_t), C.c_void_p]
    lib.fries_compress_vec.argtypes = [C.c_void_p, C.c_uint32, C.c_double, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
    lib.fries_compress_vec_piv.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
    lib.fries_test_piv_adjust.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_double, C.c_uint32, C.c_double, C.POINTER(C.c_double), C.c_void_p]
    lib.fries_measure_copy_bandwidth.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_double)]
    lib.fries_piv_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.fries_set_trial_vector.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.fries_set_initial_vector.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.fries_set_ham_shift.argtypes = [C.c_void_p, C.c_double]
    lib.fries_next_draw.restype = C.c_uint32
    lib.fries_next_draw.argtypes = [C.c_void_p]
    lib.fries_test_teeth.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.fries_test_seqsum.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p, C.POINTER(C.c_double),
                                      C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.fries_frisys_restart.argtypes = [C.c_void_p, C.c_uint32, C.c_double, C.c_double, C.c_uint32]
    lib.fries_prof_enable.argtypes = [C.c_void_p, C.c_int]
    lib.fries_prof_count.argtypes = [C.c_void_p]
    lib.fries_prof_get.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.fries_counters.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 5
    lib.fries_get_scramblers.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.fries_frimulti_setup.argtypes = [C.c_void_p, C.POINTER(FrimultiParams)]
    lib.fries_frimulti_iterate.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.fries_fciqmc_setup.argtypes = [C.c_void_p, C.POINTER(FciqmcParams)]
    lib.fries_fciqmc_iterate.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.fries_frifull_setup.argtypes = [C.c_void_p, C.POINTER(FrifullParams)]
    lib.fries_frifull_iterate.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.fries_hh_setup.argtypes = [C.c_void_p, C.POINTER(HHParams)]
    lib.fries_hh_iterate.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.fries_set_comm.argtypes = [C.c_void_p, C.c_void_p]
    lib.fries_tie_margins.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.fries_rccl_unique_id.argtypes = [C.c_void_p]
    lib.fries_rccl_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint64]
    lib.fries_local_group_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_uint64]
    lib.fries_local_group_destroy.argtypes = [C.c_void_p]
    lib.fries_local_group_destroy.restype = None
    lib.fries_local_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int]
    lib.fries_transport_comm.argtypes = [C.c_void_p, C.c_void_p]
    lib.fries_transport_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.fries_transport_destroy.argtypes = [C.c_void_p]
    lib.fries_transport_destroy.restype = None
    lib.fries_stream.restype = C.c_void_p
    lib.fries_stream.argtypes = [C.c_void_p]
    lib.fries_idx_to_proc.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.fries_vec_add_to.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.fries_death_clone.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_uint32]
    lib.fries_dots.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.fries_find_preserve.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
    lib.fries_sys_comp.argtypes = [C.c_void_p, C.c_uint32, C.c_double]
    lib.fries_dense_sizes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.fries_spawn_from_comp.argtypes = [C.c_void_p, C.c_double, C.c_double]
    lib.fries_dense_apply.argtypes = [C.c_void_p]
    lib.fries_dense_norm.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    lib.fries_dense_h_count.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    lib.fries_comp_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.fries_h_dot.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(HdotResult)]
    lib.fries_rdm1.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Rdm1Result)]
    lib.fries_rdm2.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Rdm2Result)]
    lib.fries_snapshot_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_uint32, C.c_int]
    lib.fries_snapshot_info.argtypes = [C.c_void_p, C.POINTER(SnapshotInfoStruct)]
    lib.fries_snapshot_vector.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.fries_snapshot_destroy.argtypes = [C.c_void_p]
    lib.fries_h_dot_ranks.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.POINTER(HdotResult)]
    lib.fries_rdm1_ranks.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Rdm1Result)]
    lib.fries_rdm2_ranks.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Rdm2Result)]
    lib.fries_vec_axpy_snapshot.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.POINTER(C.c_uint64)]
    lib.fries_snapshot_dot.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_int, C.c_void_p, C.POINTER(VdotResult)]
    lib.fries_vec_scale.argtypes = [C.c_void_p, C.c_int, C.c_double]
    lib.fries_vec_one_norm.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    _lib = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class FriEngine:
    """One MI355X running the FRI iteration for one molecular Hamiltonian -- or, with ``comm`` (fries_amd.comm.TorchComm),
    one rank of a hash-sharded run: vec_nonz / mat_nonz / target_norm are then global, max_dets is per rank."""

    def __init__(self, mol, device: int = 0, comm=None):
        self.lib = load_library()
        if self.lib.fries_device_count() <= 0:
            raise RuntimeError("no HIP device visible: the FRI engine runs on MI355X only (no CPU fallback)")
        self.h = C.c_void_p()
        self._ck(self.lib.fries_ctx_create(C.byref(self.h), device))
        self.mol = mol
        self.device = device
        if mol is not None:         # mol=None: a lattice-model run (setup_hh) needs no integrals
            irr = np.ascontiguousarray(mol.irreps, dtype=np.uint8)
            hc = np.ascontiguousarray(mol.h_core, dtype=np.float64)
            er = np.ascontiguousarray(mol.eris, dtype=np.float64)
            self._ck(self.lib.fries_set_molecule(self.h, mol.n_orb, mol.n_elec, _ptr(irr), _ptr(hc), _ptr(er)))
        self.max_dets = 0
        self.comm = comm
        if comm is not None:
            self._ck(self.lib.fries_set_comm(self.h, C.byref(comm.struct)))

    def _ck(self, rc):
        if rc != 0:
            raise RuntimeError(self.lib.fries_last_error().decode())

    def close(self):
        if self.h:
            if self.comm is not None:
                self.comm.release()
            self.lib.fries_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- molecule
    @property
    def hf_energy(self) -> float:
        return self.lib.fries_hf_energy(self.h)

    @property
    def p_doub(self) -> float:
        return self.lib.fries_p_doub(self.h)

    @property
    def kernel_launches(self) -> int:
        return int(self.lib.fries_kernel_launches(self.h))

    def hb_tensor(self, which: int) -> np.ndarray:
        n = self.mol.n_orb
        out = np.zeros(max(n * n, 1))
        ln = C.c_size_t()
        self._ck(self.lib.fries_get_hb_tensor(self.h, which, _ptr(out), out.size, C.byref(ln)))
        return out[:ln.value].copy()

    def set_hb_tensor(self, which: int, arr) -> None:
        a = np.ascontiguousarray(arr, dtype=np.float64)
        self._ck(self.lib.fries_set_hb_tensor(self.h, which, _ptr(a), a.size))

    def matrel(self, kind: int, dets, orbs=None):
        d = np.ascontiguousarray(dets, dtype=np.uint64)
        o = np.ascontiguousarray(orbs, dtype=np.uint8) if orbs is not None else None
        out = np.zeros(d.size)
        sg = np.zeros(d.size, dtype=np.int32)
        self._ck(self.lib.fries_matrel_batch(self.h, kind, _ptr(d), _ptr(o), d.size, _ptr(out), _ptr(sg)))
        return out, sg

    # ---- frisys_mol
    def setup(self, *, epsilon, vec_nonz, mat_nonz, max_dets, target_norm=0.0, initiator=0.0, seed=0, distribution="HB_unnorm",
              trial=None, ini=None, ham_shift=None, det_space=None):
        """frisys_mol setup.  trial / ini: (dets, vals) of --trial_vec / --ini_vec; ham_shift: the diagonal offset that replaces
        the HF energy (--ham_shift minus the core energy); det_space: the determinants of --det_space (semi-stochastic dense space)."""
        if distribution not in ("HB", "HB_unnorm"):
            raise RuntimeError('"dist_str" argument must be either "HB" or "HB_unnorm"')
        for pair, fn in ((trial, self.lib.fries_set_trial_vector), (ini, self.lib.fries_set_initial_vector)):
            if pair is not None:
                d = np.ascontiguousarray(pair[0], dtype=np.uint64)
                v = np.ascontiguousarray(pair[1], dtype=np.float64)
                self._ck(fn(self.h, _ptr(d), _ptr(v), min(d.size, v.size)))
        if ham_shift is not None:
            self._ck(self.lib.fries_set_ham_shift(self.h, float(ham_shift)))
        if det_space is not None:
            d = np.ascontiguousarray(det_space, dtype=np.uint64)
            self._ck(self.lib.fries_set_det_space(self.h, _ptr(d), d.size))
        if self.comm is not None and self.comm.big_bytes < 16 * (mat_nonz + 4096):
            raise RuntimeError("TorchComm was sized for a smaller mat_nonz")
        p = FrisysParams(epsilon, target_norm, initiator, vec_nonz, mat_nonz, max_dets, seed, 1 if distribution == "HB_unnorm" else 0)
        self._ck(self.lib.fries_frisys_setup(self.h, C.byref(p)))
        self.max_dets = max_dets
        # what iterate_stepwise needs of the run: the parameters, and the driver's own loop state (frisys_mol.cpp:112-113, 405)
        self._step = dict(eps=float(epsilon), init_thresh=float(initiator), target_norm=float(target_norm), vec_nonz=int(vec_nonz), mat_nonz=int(mat_nonz),
                          shift=0.0, last_one_norm=0.0, iterat=0, dense=None)

    # ---- fciqmc_mol
    def setup_fciqmc(self, *, epsilon, target_walkers, max_dets, initiator=0, seed=0, distribution="NU", trial=None, ini=None, fp=False):
        """fciqmc_mol with the near-uniform excitation generator (FRIES_bin/fciqmc_mol.cpp, --distribution NU): HF trial vector,
        100 walkers on HF to start; uniforms from a counter-based stream (see csrc/fciqmc.hip)."""
        if distribution not in ("NU", "HB"):
            raise RuntimeError('"dist_str" argument must be either "NU" or "HB"')
        for pair, fn in ((trial, self.lib.fries_set_trial_vector), (ini, self.lib.fries_set_initial_vector)):
            if pair is not None:
                d = np.ascontiguousarray(pair[0], dtype=np.uint64)
                v = np.ascontiguousarray(pair[1], dtype=np.float64)
                self._ck(fn(self.h, _ptr(d), _ptr(v), min(d.size, v.size)))
        p = FciqmcParams(epsilon, target_walkers, initiator, max_dets, seed, 1 if distribution == "HB" else 0, 1 if fp else 0)      # fp: fciqmc_fp_mol
        self._ck(self.lib.fries_fciqmc_setup(self.h, C.byref(p)))
        self.max_dets = max_dets

    def iterate_fciqmc(self, n_iter: int):
        logs = np.zeros(n_iter, dtype=FCIQMC_LOG_DTYPE)
        self._ck(self.lib.fries_fciqmc_iterate(self.h, n_iter, _ptr(logs)))
        return logs

    # ---- frimulti_mol
    def setup_multi(self, *, epsilon, vec_nonz, mat_nonz, max_dets, target_norm=0.0, initiator=0.0, seed=0, trial=None, ini=None):
        """frimulti_mol (FRIES_bin/frimulti_mol.cpp, --distribution HB): multinomial matrix compression, systematic vector compression.
        ini: (dets, vals) of --ini_vec; trial: --trial_vec, which the reference refuses ("Insufficient memory allocated in adder") and so does this."""
        for pair, fn in ((trial, self.lib.fries_set_trial_vector), (ini, self.lib.fries_set_initial_vector)):
            if pair is not None:
                d = np.ascontiguousarray(pair[0], dtype=np.uint64)
                v = np.ascontiguousarray(pair[1], dtype=np.float64)
                self._ck(fn(self.h, _ptr(d), _ptr(v), min(d.size, v.size)))
        p = FrimultiParams(epsilon, target_norm, initiator, vec_nonz, mat_nonz, max_dets, seed)
        self._ck(self.lib.fries_frimulti_setup(self.h, C.byref(p)))
        self.max_dets = max_dets

    def iterate_multi(self, n_iter: int):
        logs = np.zeros(n_iter, dtype=FCIQMC_LOG_DTYPE)
        self._ck(self.lib.fries_frimulti_iterate(self.h, n_iter, _ptr(logs)))
        return logs

    # ---- frifull_mol
    def setup_full(self, *, epsilon, vec_nonz, max_dets, target_norm=0.0, seed=0, spawn_cap=0):
        """frifull_mol (FRIES_bin/frifull_mol.cpp): vector compression + the Hamiltonian applied in full, start from 100 x HF."""
        p = FrifullParams(epsilon, target_norm, vec_nonz, max_dets, seed, spawn_cap)
        self._ck(self.lib.fries_frifull_setup(self.h, C.byref(p)))
        self.max_dets = max_dets

    def iterate_full(self, n_iter: int, want_logs: bool = True):
        logs = np.zeros(n_iter, dtype=ITERLOG_DTYPE) if want_logs else None
        self._ck(self.lib.fries_frifull_iterate(self.h, n_iter, _ptr(logs) if want_logs else None))
        return logs

    # ---- frisys_hh
    def setup_hh(self, *, n_elec, n_sites, eps, U, omega, g, gs_energy, vec_nonz, max_dets, target_norm=0.0, initiator=0.0, seed=0, full=False):
        """frisys_hh (FRIES_bin/frisys_hh.cpp): 1-D Hubbard-Holstein chain, open boundaries, t = 1, start from 100 x Neel.
        full=True: frifull_hh (FRIES_bin/frifull_hh.cpp), the Hamiltonian applied in full instead of compressed."""
        p = HHParams(n_elec, n_sites, eps, U, omega, g, gs_energy, target_norm, initiator, vec_nonz, max_dets, seed, 1 if full else 0)
        self._ck(self.lib.fries_hh_setup(self.h, C.byref(p)))
        self.max_dets = max_dets

    def iterate_hh(self, n_iter: int, want_logs: bool = True):
        logs = np.zeros(n_iter, dtype=ITERLOG_DTYPE) if want_logs else None
        self._ck(self.lib.fries_hh_iterate(self.h, n_iter, _ptr(logs) if want_logs else None))
        return logs

    def idx_to_proc(self, dets) -> np.ndarray:
        """DistVec::idx_to_proc: the rank that owns each determinant."""
        d = np.ascontiguousarray(dets, dtype=np.uint64)
        out = np.zeros(d.size, dtype=np.int32)
        self._ck(self.lib.fries_idx_to_proc(self.h, _ptr(d), d.size, _ptr(out)))
        return out

    def iterate(self, n_iter: int, want_logs: bool = True):
        logs = np.zeros(n_iter, dtype=ITERLOG_DTYPE) if want_logs else None
        assert ITERLOG_DTYPE.itemsize == C.sizeof(IterLog)
        self._ck(self.lib.fries_frisys_iterate(self.h, n_iter, _ptr(logs) if want_logs else None))
        return logs

    # ---- frisys_mol step by step: the operators of one iteration as single calls (nothing but scalars crosses PCIe)
    def apply_hbpp_sys_device(self, n_samp: int, rn):
        """apply_HBPP_sys with the result left on the device (for spawn_from_comp / comp_download); returns (num_success, comp_len[5])."""
        rn = np.ascontiguousarray(rn, dtype=np.float64)
        m = C.c_size_t()
        cl = np.zeros(5, dtype=np.uint32)
        self._ck(self.lib.fries_apply_hbpp_sys(self.h, n_samp, _ptr(rn), 0, None, None, None, C.c_size_t(-1).value, C.byref(m), _ptr(cl)))
        return m.value, cl

    def spawn_from_comp(self, eps: float, init_thresh: float):
        """frisys_mol.cpp:429-471 on the compression result pending on the device; raises when none is pending."""
        self._ck(self.lib.fries_spawn_from_comp(self.h, eps, init_thresh))

    def dense_apply(self):
        """frisys_mol.cpp:480-485: the dense block of H times column 0 into column 1 (no-op without a dense space)."""
        self._ck(self.lib.fries_dense_apply(self.h))

    def dense_norm(self) -> float:
        out = C.c_double()
        self._ck(self.lib.fries_dense_norm(self.h, C.byref(out)))
        return out.value

    def dense_h_count(self) -> int:
        """tot_dense_h: matrix elements inside the dense space over all ranks."""
        out = C.c_uint32()
        self._ck(self.lib.fries_dense_h_count(self.h, C.byref(out)))
        return out.value

    def dense_sizes(self):
        """Every rank's dense-space size (dense.txt)."""
        out = np.zeros(64, dtype=np.uint32)
        n = C.c_size_t()
        self._ck(self.lib.fries_dense_sizes(self.h, _ptr(out), out.size, C.byref(n)))
        return out[:n.value].copy()

    def comp_download(self, cap: int = None):
        """The compression result pending on the device: (positions, orbitals, values)."""
        m = C.c_size_t()
        if cap is None:
            if self.lib.fries_comp_download(self.h, None, None, None, 0, C.byref(m)) != 0 and m.value == 0:
                raise RuntimeError(self.lib.fries_last_error().decode())
            cap = m.value
        pos = np.zeros(max(cap, 1), dtype=np.uint32)
        orbs = np.zeros((max(cap, 1), 4), dtype=np.uint8)
        vals = np.zeros(max(cap, 1))
        self._ck(self.lib.fries_comp_download(self.h, _ptr(pos), _ptr(orbs), _ptr(vals), cap, C.byref(m)))
        k = m.value
        return pos[:k].copy(), orbs[:k].copy(), vals[:k].copy()

    def vec_add_to(self, column: int, dets, vals, ini):
        """DistVec::add x n + perform_add into `column` (what this rank received, in arrival order)."""
        d = np.ascontiguousarray(dets, dtype=np.uint64)
        v = np.ascontiguousarray(vals, dtype=np.float64)
        f = np.ascontiguousarray(ini, dtype=np.uint8)
        self._ck(self.lib.fries_vec_add_to(self.h, column, _ptr(d), _ptr(v), _ptr(f), d.size))

    def death_clone(self, eps: float, shift: float, vec_size: int):
        """frisys_mol.cpp:487-499."""
        self._ck(self.lib.fries_death_clone(self.h, eps, shift, vec_size))

    def dots(self):
        """(numerator, denominator) of the projected energy (frisys_mol.cpp:511-517)."""
        a, b = C.c_double(), C.c_double()
        self._ck(self.lib.fries_dots(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def find_preserve(self, n_samp: int):
        """find_preserve on column 0 with budget n_samp; returns (samples left, one-norm before compression)."""
        ns = C.c_uint32(n_samp)
        gn = C.c_double()
        self._ck(self.lib.fries_find_preserve(self.h, C.byref(ns), C.byref(gn)))
        return ns.value, gn.value

    def sys_comp(self, n_samp: int, rn: float):
        """sys_comp after find_preserve, with the driver's deletes."""
        self._ck(self.lib.fries_sys_comp(self.h, n_samp, rn))

    def iterate_stepwise(self, n_iter: int):
        """frisys_mol.cpp:405-552 written out over the single-operator calls -- the loop a host that keeps its own driver would write.
        Same log fields as iterate().  The shift, the last one-norm and the iteration count of this loop are kept here, as the
        reference's driver keeps them in its own variables: continue a run with the loop it was started with."""
        import math
        st = self._step
        eps, shift_interval, shift_damping = st["eps"], 10, 0.05
        if st["dense"] is None:
            st["dense_h"] = self.dense_h_count()
            st["dense"] = bool(st["dense_h"]) or bool(self.dense_sizes().any())
        logs = np.zeros(n_iter, dtype=ITERLOG_DTYPE)
        for k in range(n_iter):
            rn = [self.next_draw() / 2.0 ** 32 for _ in range(5)]
            num_success, comp_len = self.apply_hbpp_sys_device(st["mat_nonz"] - st["dense_h"], rn)       # :414-422
            vec_size = self.vec_info()[0]
            self.spawn_from_comp(eps, st["init_thresh"])                                                # :429-471
            self.dense_apply()                                                                          # :480-485
            self.death_clone(eps, st["shift"], vec_size)                                                # :487-499
            numer, denom = self.dots()                                                                  # :511-517
            n_samp, glob_norm = self.find_preserve(st["vec_nonz"])                                      # :503
            if st["dense"]:
                glob_norm += self.dense_norm()                                                          # :504
            if (st["iterat"] + 1) % shift_interval == 0:                                                # adjust_shift, compress_utils.cpp:684-693
                damp = shift_damping / shift_interval / eps
                if st["last_one_norm"]:
                    st["shift"] -= damp * math.log(glob_norm / st["last_one_norm"])
                    st["last_one_norm"] = glob_norm
                if st["last_one_norm"] == 0 and glob_norm > st["target_norm"]:
                    st["last_one_norm"] = glob_norm
            self.sys_comp(n_samp, self.next_draw() / 2.0 ** 32)                                         # :526-539
            st["iterat"] += 1
            curr_size, n_nonz, _ = self.vec_info()
            lg = logs[k]
            lg["numer"], lg["denom"], lg["shift"], lg["norm"] = numer, denom, st["shift"], glob_norm
            lg["nkept"], lg["n_nonz"], lg["curr_size"], lg["num_success"] = st["vec_nonz"] - n_samp, n_nonz, curr_size, num_success
            lg["comp_len"] = comp_len
        return logs

    def vec_info(self):
        a, b, c = C.c_uint32(), C.c_int32(), C.c_uint32()
        self._ck(self.lib.fries_vec_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def vector(self):
        n = self.vec_info()[0]
        d = np.zeros(max(n, 1), dtype=np.uint64)
        v = np.zeros(max(n, 1))
        m = C.c_size_t()
        self._ck(self.lib.fries_vec_download(self.h, _ptr(d), _ptr(v), d.size, C.byref(m)))
        return d[:m.value], v[:m.value]

    def htrial(self):
        cap = 4 * self.mol.n_orb ** 2 * self.mol.n_elec ** 2 + 16
        d = np.zeros(cap, dtype=np.uint64)
        v = np.zeros(cap)
        m = C.c_size_t()
        self._ck(self.lib.fries_htrial_download(self.h, _ptr(d), _ptr(v), cap, C.byref(m)))
        return d[:m.value].copy(), v[:m.value].copy()

    def set_spin_parity(self, spin_parity: int):
        """Time-reversal symmetrised vectors (spin_parity = +-1; 0 = off): see fries_set_spin_parity."""
        self._ck(self.lib.fries_set_spin_parity(self.h, int(spin_parity)))

    def h_offdiag_list(self, dets, vals):
        """h_op_offdiag (dest column 1, h_fac 1, the context's spin parity) on a fresh vector holding (dets, vals): stored determinants, column 1."""
        d = np.ascontiguousarray(dets, dtype=np.uint64)
        v = np.ascontiguousarray(vals, dtype=np.float64)
        cap = d.size * (self.mol.n_orb ** 2 * self.mol.n_elec ** 2 + 2) + 64
        od = np.zeros(cap, dtype=np.uint64)
        ov = np.zeros(cap)
        m = C.c_size_t()
        self._ck(self.lib.fries_h_offdiag_list(self.h, _ptr(d), _ptr(v), d.size, _ptr(od), _ptr(ov), cap, C.byref(m)))
        return od[:m.value].copy(), ov[:m.value].copy()

    def h_dot(self, other=None) -> HDot:
        """<self|H|other> and <self|other> over column 0 of the two engines' vectors (fries_h_dot; calc_h_dot, molecule.cpp:667-885).
        self is the enumerating side; other=None means the engine itself.  Neither engine may be inside another call on another thread."""
        r = HdotResult()
        self._ck(self.lib.fries_h_dot(self.h, (self if other is None else other).h, C.byref(r)))
        return HDot(r.h, r.ovlp, r.abs_sum, int(r.n_src), int(r.n_terms), int(r.n_hits))

    def rdm1(self, other=None) -> Rdm1:
        """The one-body density matrix <self| sum_sigma c+_{p sigma} c_{q sigma} |other> over column 0 of the two engines' vectors
        (fries_rdm1; one_elec_op, molecule.cpp:222-252, for every orbital pair at once).  self is the enumerating side; other=None
        means the engine itself.  Neither engine may be inside another call on another thread."""
        n = self.mol.n_orb if self.mol is not None else 0
        g = np.zeros((max(n, 1), max(n, 1)))        # (a context without a molecule is refused by the call itself)
        r = Rdm1Result()
        self._ck(self.lib.fries_rdm1(self.h, (self if other is None else other).h, _ptr(g), C.byref(r)))
        return Rdm1(g, r.ovlp, r.abs_sum, int(r.n_src), int(r.n_terms), int(r.n_hits))

    def rdm2(self, other=None) -> Rdm2:
        """The two-body density matrix between column 0 of the two engines' vectors (fries_rdm2), spin-summed, chemists' order.  self is
        the enumerating side; other=None means the engine itself.  Neither engine may be inside another call on another thread."""
        n = max(self.mol.n_orb if self.mol is not None else 0, 1)       # (a context without a molecule is refused by the call itself)
        g = np.zeros((n, n, n, n))
        r = Rdm2Result()
        self._ck(self.lib.fries_rdm2(self.h, (self if other is None else other).h, _ptr(g), C.byref(r)))
        return Rdm2(g, r.ovlp, r.abs_sum, int(r.n_src), int(r.n_terms), int(r.n_hits))

    def axpy_snapshot(self, column: int, coeff: float, snap) -> int:
        """column[det] += coeff * snap[det] over the entries of the snapshot this engine owns (fries_vec_axpy_snapshot), merged on the
        device like a vec_add_to of the same list with initiator flags 1; returns the number of entries merged."""
        n = C.c_uint64()
        self._ck(self.lib.fries_vec_axpy_snapshot(self.h, column, coeff, snap.h if snap is not None else None, C.byref(n)))
        return int(n.value)

    def scale(self, column: int, factor: float) -> None:
        """v[column] *= factor over the stored positions (fries_vec_scale)"""
        self._ck(self.lib.fries_vec_scale(self.h, column, factor))

    def one_norm(self, column: int = 0) -> float:
        """The sum of |v[column]| in position order, then over the ranks in rank order (fries_vec_one_norm; a collective with ranks)"""
        out = C.c_double()
        self._ck(self.lib.fries_vec_one_norm(self.h, column, C.byref(out)))
        return out.value

    def variational_energy(self) -> float:
        """The Rayleigh quotient <v|H|v> / <v|v> of the current vector, on the scale of numer / denom."""
        r = self.h_dot()
        return r.h / r.ovlp

    def vec_add(self, dets, vals, ini):
        d = np.ascontiguousarray(dets, dtype=np.uint64)
        v = np.ascontiguousarray(vals, dtype=np.float64)
        f = np.ascontiguousarray(ini, dtype=np.uint8)
        self._ck(self.lib.fries_vec_add(self.h, _ptr(d), _ptr(v), _ptr(f), d.size))

    def vec_load(self, dets, vals):
        d = np.ascontiguousarray(dets, dtype=np.uint64)
        v = np.ascontiguousarray(vals, dtype=np.float64)
        self._ck(self.lib.fries_vec_load(self.h, _ptr(d), _ptr(v), d.size))

    def apply_hbpp_sys(self, n_samp: int, rn, unit_matrel: bool = False):
        rn = np.ascontiguousarray(rn, dtype=np.float64)
        cap = n_samp + 4096
        pos = np.zeros(cap, dtype=np.uint32)
        orbs = np.zeros((cap, 4), dtype=np.uint8)
        vals = np.zeros(cap)
        m = C.c_size_t()
        cl = np.zeros(5, dtype=np.uint32)
        self._ck(self.lib.fries_apply_hbpp_sys(self.h, n_samp, _ptr(rn), int(unit_matrel), _ptr(pos), _ptr(orbs), _ptr(vals), cap, C.byref(m), _ptr(cl)))
        k = m.value
        return pos[:k].copy(), orbs[:k].copy(), vals[:k].copy(), cl

    def rng_state(self) -> str:
        """The driver generator in std::mt19937's text form."""
        need = C.c_size_t()
        self._ck(self.lib.fries_rng_get_state(self.h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        self._ck(self.lib.fries_rng_get_state(self.h, buf, need.value, None))
        return buf.value.decode()

    def set_rng_state(self, text: str):
        self._ck(self.lib.fries_rng_set_state(self.h, text.encode()))

    def apply_hbpp_piv(self, n_samp: int, unit_matrel: bool = False):
        """apply_HBPP_piv (heat_bathPP.cpp:1014-1419) on the stored vector; the uniforms come from the engine's generator (restart(seed))."""
        cap = n_samp + 4096
        pos = np.zeros(cap, dtype=np.uint32)
        orbs = np.zeros((cap, 4), dtype=np.uint8)
        vals = np.zeros(cap)
        m = C.c_size_t()
        sl = np.zeros(5, dtype=np.uint32)
        self._ck(self.lib.fries_apply_hbpp_piv(self.h, n_samp, int(unit_matrel), _ptr(pos), _ptr(orbs), _ptr(vals), cap, C.byref(m), _ptr(sl)))
        k = m.value
        return pos[:k].copy(), orbs[:k].copy(), vals[:k].copy(), sl

    def apply_hbpp_piv_device(self, n_samp: int):
        """apply_HBPP_piv with the result left on the device (for spawn_from_comp / comp_download); returns (num_success, stage_len[5])."""
        m = C.c_size_t()
        sl = np.zeros(5, dtype=np.uint32)
        self._ck(self.lib.fries_apply_hbpp_piv(self.h, n_samp, 0, None, None, None, C.c_size_t(-1).value, C.byref(m), _ptr(sl)))
        return m.value, sl

    def dot_list(self, column: int, dets, vals) -> float:
        """DistVec::dot: the sum over the list, in list order, of vals[i] * v[column][det_i] (fries_vec_dot_list)"""
        d = np.ascontiguousarray(dets, dtype=np.uint64)
        v = np.ascontiguousarray(vals, dtype=np.float64)
        out = C.c_double()
        self._ck(self.lib.fries_vec_dot_list(self.h, column, _ptr(d), _ptr(v), min(d.size, v.size), C.byref(out)))
        return out.value

    def compress_vec(self, n_samp: int, rn: float):
        nk = C.c_uint32()
        gn = C.c_double()
        self._ck(self.lib.fries_compress_vec(self.h, n_samp, rn, C.byref(nk), C.byref(gn)))
        return nk.value, gn.value

    def compress_vec_piv(self, n_samp: int):
        """compress_vecs with one vector (vec_utils.cpp:9-32): pivotal compression of column 0 to at most n_samp
        non-zeros, drawing from the engine's mt19937; returns (elements preserved exactly, one-norm before)."""
        nk = C.c_uint32()
        gn = C.c_double()
        self._ck(self.lib.fries_compress_vec_piv(self.h, n_samp, C.byref(nk), C.byref(gn)))
        return nk.value, gn.value

    def test_piv_adjust(self, n_loc: int, exp_loc: float, n_tot: int, tot_norm: float):
        nl = C.c_uint32(n_loc)
        nn = C.c_double()
        fl = np.zeros(max(self.vec_info()[0], 1), dtype=np.uint8)
        self._ck(self.lib.fries_test_piv_adjust(self.h, C.byref(nl), exp_loc, n_tot, tot_norm, C.byref(nn), _ptr(fl)))
        return nl.value, nn.value, fl

    def copy_bandwidth(self, nbytes: int = 1 << 30, reps: int = 5) -> float:
        out = C.c_double()
        self._ck(self.lib.fries_measure_copy_bandwidth(self.h, nbytes, reps, C.byref(out)))
        return out.value

    def piv_stats(self):
        a, b = C.c_uint64(), C.c_uint64()
        self.last_piv_reason = self.lib.fries_piv_stats(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def next_draw(self) -> int:
        return int(self.lib.fries_next_draw(self.h))

    def test_teeth(self, r0: float, unit: float, n: int, queries):
        q = np.ascontiguousarray(queries, dtype=np.float64)
        pos = np.zeros(max(n, 1))
        below = np.zeros(max(q.size, 1), dtype=np.uint32)
        self._ck(self.lib.fries_test_teeth(self.h, r0, unit, n, _ptr(pos), _ptr(q), q.size, _ptr(below)))
        return pos[:n], below[:q.size]

    def test_seqsum(self, vals, start: float = 0.0):
        a = np.ascontiguousarray(vals, dtype=np.float64)
        out = np.zeros(max(a.size, 1))
        tot = C.c_double()
        dt, ds = C.c_uint32(), C.c_uint32()
        self._ck(self.lib.fries_test_seqsum(self.h, _ptr(a), a.size, start, _ptr(out), C.byref(tot), C.byref(dt), C.byref(ds)))
        return out[:a.size], tot.value, dt.value, ds.value

    def restart(self, seed: int, en_shift: float = 0.0, last_one_norm: float = 0.0, iterat: int = 0):
        self._ck(self.lib.fries_frisys_restart(self.h, seed, en_shift, last_one_norm, iterat))

    def tie_margins(self, enable: bool = True):
        """(smallest relative margin of a find_keep_sub comparison, of a find_preserve comparison) since the last call."""
        a, b = C.c_double(), C.c_double()
        self._ck(self.lib.fries_tie_margins(self.h, int(enable), C.byref(a), C.byref(b)))
        return a.value, b.value

    def prof_enable(self, on: bool = True):
        self._ck(self.lib.fries_prof_enable(self.h, int(on)))

    def prof_report(self):
        """{kernel: (total_ms, calls)} from HIP events on the engine's stream."""
        out = {}
        buf = C.create_string_buffer(128)
        for i in range(self.lib.fries_prof_count(self.h)):
            ms, calls = C.c_double(), C.c_uint64()
            self._ck(self.lib.fries_prof_get(self.h, i, buf, 128, C.byref(ms), C.byref(calls)))
            out[buf.value.decode()] = (ms.value, calls.value)
        return out

    def counters(self):
        v = [C.c_uint64() for _ in range(5)]
        self.lib.fries_counters(self.h, *[C.byref(x) for x in v])
        return dict(zip(("iters", "spawns", "launches", "fks_replays", "stage_elems"), (x.value for x in v)))


def _handles(engines):
    engines = list(engines)
    return engines, (C.c_void_p * max(len(engines), 1))(*[e.h for e in engines])


class VecSnapshot:
    """A frozen, device-resident copy of column 0 of a vector (fries_snapshot): `shards` are the engines that hold it -- one engine, or
    ranks 0 .. P - 1 of one sharded run in order, all in this process.  It is the probed side of the estimators over ranks: h_dot,
    rdm1 and rdm2 take the enumerating vector as its list of shards and return what FriEngine.h_dot / rdm1 / rdm2 return.  The
    snapshot does not change when its source iterates on; it holds device memory until close()."""

    def __init__(self, shards, device=None):
        shards, arr = _handles(shards)
        self.lib = load_library()
        self.n_orb = shards[0].mol.n_orb if shards and shards[0].mol is not None else 0
        self.h = C.c_void_p()
        dev = device if device is not None else (shards[0].device if shards else 0)      # default: the first shard's device
        self._ck(self.lib.fries_snapshot_create(C.byref(self.h), arr, len(shards), dev))

    def _ck(self, rc):
        if rc != 0:
            raise RuntimeError(self.lib.fries_last_error().decode())

    @property
    def info(self) -> SnapshotInfo:
        r = SnapshotInfoStruct()
        self._ck(self.lib.fries_snapshot_info(self.h, C.byref(r)))
        return SnapshotInfo(int(r.n_entries), int(r.n_shards), int(r.n_slots), int(r.device_bytes), int(r.device), r.ms_compact, r.ms_copy, r.ms_insert)

    def vector(self):
        """The entries in the snapshot's order: the shards in rank order, each shard's live entries in position order."""
        n = self.info.n_entries
        d, v = np.zeros(n, dtype=np.uint64), np.zeros(n)
        m = C.c_uint64()
        self._ck(self.lib.fries_snapshot_vector(self.h, _ptr(d), _ptr(v), n, C.byref(m)))
        return d, v

    def h_dot(self, a_shards) -> HDot:
        """<a|H|snapshot> and <a|snapshot> (fries_h_dot_ranks): a_shards enumerate, one after the other; no engine among them may be
        inside another call meanwhile."""
        shards, arr = _handles(a_shards)
        r = HdotResult()
        self._ck(self.lib.fries_h_dot_ranks(arr, len(shards), self.h, C.byref(r)))
        return HDot(r.h, r.ovlp, r.abs_sum, int(r.n_src), int(r.n_terms), int(r.n_hits))

    def dot(self, a_shards, column: int = 0) -> VDot:
        """<a|snapshot> with `column` of a (fries_snapshot_dot): one look-up per stored position of a_shards, no Hamiltonian."""
        shards, arr = _handles(a_shards)
        r = VdotResult()
        self._ck(self.lib.fries_snapshot_dot(arr, len(shards), column, self.h, C.byref(r)))
        return VDot(r.dot, r.abs_sum, int(r.n_src), int(r.n_hits))

    def rdm1(self, a_shards) -> Rdm1:
        """The one-body density matrix <a| ... |snapshot> (fries_rdm1_ranks)"""
        shards, arr = _handles(a_shards)
        n = max(self.n_orb, 1)
        g = np.zeros((n, n))
        r = Rdm1Result()
        self._ck(self.lib.fries_rdm1_ranks(arr, len(shards), self.h, _ptr(g), C.byref(r)))
        return Rdm1(g, r.ovlp, r.abs_sum, int(r.n_src), int(r.n_terms), int(r.n_hits))

    def rdm2(self, a_shards) -> Rdm2:
        """The two-body density matrix <a| ... |snapshot> (fries_rdm2_ranks), spin-summed, chemists' order"""
        shards, arr = _handles(a_shards)
        n = max(self.n_orb, 1)
        g = np.zeros((n, n, n, n))
        r = Rdm2Result()
        self._ck(self.lib.fries_rdm2_ranks(arr, len(shards), self.h, _ptr(g), C.byref(r)))
        return Rdm2(g, r.ovlp, r.abs_sum, int(r.n_src), int(r.n_terms), int(r.n_hits))

    def close(self):
        if self.h:
            self.lib.fries_snapshot_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
