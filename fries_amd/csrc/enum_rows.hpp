// Full single / double enumeration from one source determinant, shared by k_enum (system.hip: H * vector as a list) and
// k_hdot (hdot.hip: <a|H|b> by enumerate-and-probe): candidate index -> orbitals in the reference's loop order
// (FRIES/Hamiltonians/molecule.cpp:108-203, 448-665), Slater-Condon element, fermionic sign, time-reversal adjustment.
#pragma once
#include "fries_dev.hpp"
#include "hbpp_rows.hpp"

// candidate slots of one source: mode 0 singles (electron, orbital), mode 1 doubles (opposite spin, then the two same-spin blocks)
__device__ __forceinline__ uint32_t fr_enum_n_cand(unsigned n, unsigned ne, int mode) {
    const unsigned h = ne / 2;
    return mode == 0 ? ne * n : h * h * n * n + 2 * (h * (h - 1) / 2) * n * n;
}

__device__ __forceinline__ bool fr_enum_candidate(const HbTables &T, det_t det, int mode, uint32_t idx, unsigned *o1, unsigned *o2, unsigned *u1, unsigned *u2) {
    const unsigned n = T.n_orb, ne = T.n_elec, h = ne / 2;
    if (mode == 0) {
        // (electron i, orbital a of the same spin)
        unsigned i = idx / n, a = idx % n;
        if (i >= ne) return false;
        unsigned sp = i / h, io = fr_nth_bit(det, i), ao = a + sp * n;
        if (fr_bit(det, ao) || T.irrep[io % n] != T.irrep[a]) return false;
        *o1 = io; *u1 = ao; *o2 = 0; *u2 = 0;
        return true;
    }
    const uint32_t n_os = h * h * n * n, npair = h * (h - 1) / 2, n_ss = npair * n * n;
    if (idx < n_os) {
        unsigned l = idx % n, k = (idx / n) % n, j = (idx / (n * n)) % h, i = idx / (n * n * h);
        unsigned io = fr_nth_bit(det, i), jo = fr_nth_bit(det, h + j), ko = k, lo = l + n;
        if (fr_bit(det, ko) || fr_bit(det, lo)) return false;
        if ((T.irrep[io] ^ T.irrep[jo - n] ^ T.irrep[k] ^ T.irrep[l]) != 0) return false;
        *o1 = io; *o2 = jo; *u1 = ko; *u2 = lo;
        return true;
    }
    idx -= n_os;
    unsigned sp = 0;
    if (idx >= n_ss) { idx -= n_ss; sp = 1; if (idx >= n_ss) return false; }
    unsigned l = idx % n, k = (idx / n) % n, pr = idx / (n * n);
    if (l <= k) return false;
    // pair index -> (i < j) in the order i outer, j inner
    unsigned i = 0, rem = pr;
    while (rem >= h - 1 - i) { rem -= h - 1 - i; i++; }
    unsigned j = i + 1 + rem;
    unsigned io = fr_nth_bit(det, sp * h + i), jo = fr_nth_bit(det, sp * h + j), ko = k + sp * n, lo = l + sp * n;
    if (fr_bit(det, ko) || fr_bit(det, lo)) return false;
    if ((T.irrep[io % n] ^ T.irrep[jo % n] ^ T.irrep[k] ^ T.irrep[l]) != 0) return false;
    *o1 = io; *o2 = jo; *u1 = ko; *u2 = lo;
    return true;
}

// Candidate idx of `det`: false when the slot holds no symmetry-allowed excitation.  Otherwise *nd = the determinant the element goes to
// and *m = <nd|H|det> with its sign -- under S.spin_parity the representative and the element between the symmetrised functions, 0 when
// the pair does not contribute.
__device__ __forceinline__ bool fr_enum_element(const HbTables &T, const SysDev &S, det_t det, int mode, uint32_t idx, det_t *nd_out, double *m_out,
                                                unsigned *o1, unsigned *o2, unsigned *u1, unsigned *u2) {
    if (!fr_enum_candidate(T, det, mode, idx, o1, o2, u1, u2)) return false;
    const unsigned n = T.n_orb;
    double m;
    det_t nd;
    if (mode == 0) {
        m = fr_sing_matrel(det, *o1, *u1, S.h_core, S.eris, n);
        nd = det & ~(1ull << *o1);
        int sgn = (fr_bits_between(nd, *o1, *u1) & 1) ? -1 : 1;       // sing_det_parity, fci_utils.c:46-51
        nd |= 1ull << *u1;
        m *= sgn;
    }
    else {
        m = fr_doub_matrel(*o1, *o2, *u1, *u2, S.eris, n);
        m *= fr_doub_parity(det, *o1, *o2, *u1, *u2);                   // doub_det_parity, fci_utils.c:66-75
        nd = (det & ~(1ull << *o1) & ~(1ull << *o2)) | (1ull << *u1) | (1ull << *u2);
    }
    // time-reversal symmetrised vectors: the element between the symmetrised functions, added to the pair's representative
    if (S.spin_parity) { det_t tgt = nd; if (fr_adjust_tr(T, S, det, nd, &m, S.spin_parity, &tgt, 0, nullptr, 0.0)) nd = tgt; else m = 0; }
    *nd_out = nd; *m_out = m;
    return true;
}
