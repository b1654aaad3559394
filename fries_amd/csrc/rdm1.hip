// The spin-summed one-body density matrix between the solution vectors of two contexts, gamma[p][q] = <a| sum_sigma c+_{p sigma} c_{q sigma} |b>
// (what the reference forms one orbital pair at a time: one_elec_op, FRIES/Hamiltonians/molecule.cpp:222-252, then DistVec::internal_dot,
// as observables_mol and obs_repl_mol do).  Every stored determinant i of `a` with a non-zero value enumerates its same-spin single
// replacements -- occupied p, empty q, both spins: n_elec * (n_orb - n_elec / 2) of them, no rejection and no symmetry table -- and
// looks |j> = |i with p emptied and q filled> up in `b`'s hash table; a_i * sign * b_j goes to bin (p, q).  The diagonal is the number
// operator: a_i * b_i to bin (p, p) for every occupied spin orbital of i.
//
// Shape: a workgroup of four waves owns RD_BPOS contiguous positions, a wave RD_WPOS = 64 of them.  The wave loads its 64 sources in one
// coalesced pass and walks them in order, the source broadcast from the lane that holds it.  The candidates of a source form one index
// space, each spin padded to a multiple of 64 so that the 64 lanes of a step hold candidates of one spin -- and so 64 different bins.
// A lane takes RD_ILP candidates per round and issues their first probes (one 16-byte HSlot each) together before it resolves any.
//
// Accumulation and determinism: no floating-point atomics anywhere.  Each wave keeps a private n_orb x n_orb matrix in LDS and adds
// into it by plain read-modify-write: within a step the bins are distinct, and the steps follow each other in program order (alpha
// before beta, source after source).  The four waves' matrices are added in wave order, the workgroups' matrices by k_rdm1_reduce,
// RD_FAN of them per workgroup in index order, level by level until one is left.  The order in which every bin's terms are associated is
// a function of curr_size and the positions alone: two calls on the same vectors return the same bits.
#include "ctx.hpp"
#include "rdm1_plan.hpp"
#include "pair_frame.hpp"

#ifndef RD_ILP
#define RD_ILP 4                // probes a lane has in flight per round
#endif
#ifndef RD_LDS_ORB
#define RD_LDS_ORB FR_MAX_ORB   // edge of a wave's matrix in LDS (diagnostic builds: a larger one lowers the occupancy)
#endif

// part: [gridDim.x][n_orb^2 + RD_NSCAL] (the matrix, ovlp, abs_sum); cnt: [gridDim.x][RD_NCNT] (n_src, n_terms, n_hits)
__global__ void __launch_bounds__(FR_BLOCK) k_rdm1(VecDev A, VecDev B, uint32_t n_orb, uint32_t n_pos, double *part, unsigned long long *cnt) {
    __shared__ double G[4][RD_LDS_ORB * RD_LDS_ORB];
    __shared__ double shs[4][RD_NSCAL];
    __shared__ unsigned long long shc[4][RD_NCNT];
    const unsigned w = threadIdx.x >> 6, lane = fr_lane();
    const unsigned n2 = n_orb * n_orb;
    double *g = G[w];
    for (unsigned k = lane; k < n2; k += FR_WAVE) g[k] = 0.0;
    fr_wave_step_fence();
    const size_t mine = (size_t)blockIdx.x * RD_BPOS + (size_t)w * RD_WPOS + lane;
    unsigned long long my_det = 0; double my_val = 0;
    if (mine < n_pos) { my_det = A.dets[mine]; my_val = A.v0[mine]; }
    const det_t lowmask = (1ull << n_orb) - 1ull;       // n_orb <= 32
    double ov = 0, ab = 0;
    uint32_t n_src = 0, n_terms = 0, n_hits = 0;
    for (int s = 0; s < RD_WPOS; s++) {
        PairSrc src;
        if (!src.load(B, my_val, my_det, s, n_orb, lowmask)) continue;
        n_src++;
        const double av = src.av;
        const det_t det = src.det, occ0 = src.occ0, occ1 = src.occ1;
        const unsigned no0 = src.no0, no1 = src.no1;
        const unsigned nc0 = no0 * (n_orb - no0), nc1 = no1 * (n_orb - no1);
        const unsigned pad0 = (nc0 + FR_WAVE - 1) & ~(FR_WAVE - 1u), n_idx = pad0 + ((nc1 + FR_WAVE - 1) & ~(FR_WAVE - 1u));
        for (unsigned c0 = 0; c0 < n_idx; c0 += FR_WAVE * RD_ILP) {
            det_t nd[RD_ILP]; double sg[RD_ILP]; uint32_t sl[RD_ILP], bin[RD_ILP]; HSlot e[RD_ILP];
#pragma unroll
            for (int k = 0; k < RD_ILP; k++) {
                const unsigned idx = c0 + k * FR_WAVE + lane;
                const unsigned spin = idx >= pad0, c = spin ? idx - pad0 : idx;
                sg[k] = 0; nd[k] = det; bin[k] = 0; sl[k] = 0;
                e[k].key = FR_EMPTY_KEY; e[k].val = FR_NOPOS;
                if (idx < n_idx && c < (spin ? nc1 : nc0)) {
                    const det_t occ = spin ? occ1 : occ0, holes = ~occ & lowmask;
                    const unsigned nh = n_orb - (spin ? no1 : no0);
                    const unsigned p = fr_nth_bit(occ, c / nh), q = fr_nth_bit(holes, c % nh);
                    const unsigned P = p + spin * n_orb, Q = q + spin * n_orb;
                    sg[k] = fr_sing_parity(det, P, Q);
                    nd[k] = det ^ (1ull << P) ^ (1ull << Q);
                    bin[k] = p * n_orb + q;
                    sl[k] = fr_hash_slot(nd[k], B.hcap);
                    e[k] = B.hs[sl[k]];         // the round's first probes are independent of each other
                }
            }
#pragma unroll
            for (int k = 0; k < RD_ILP; k++) {
                if (sg[k] != 0) {
                    n_terms++;
                    const double bv = hd_resolve(B, nd[k], sl[k], e[k]);
                    if (bv != 0) {
                        const double t = av * sg[k] * bv;
                        g[bin[k]] += t;         // the 64 candidates of a step have one spin: 64 different bins
                        ab += fabs(t); n_hits++;
                    }
                }
                fr_wave_step_fence();
            }
        }
        const double t = av * hd_resolve(B, det, src.sl0, src.e0);
        if (t != 0) {
            if (lane == 0) ov += t;
            for (int spin = 0; spin < 2; spin++) {
                if (lane < (spin ? no1 : no0)) { const unsigned p = fr_nth_bit(spin ? occ1 : occ0, lane); g[p * n_orb + p] += t; }
                fr_wave_step_fence();
            }
        }
    }
    ab = fr_wave_sum(ab);
    n_terms = fr_wave_sum_u32(n_terms); n_hits = fr_wave_sum_u32(n_hits);
    if (lane == 0) { shs[w][0] = ov; shs[w][1] = ab; shc[w][0] = n_src; shc[w][1] = n_terms; shc[w][2] = n_hits; }
    __syncthreads();
    // the waves' partials in wave order
    double *row = part + (size_t)blockIdx.x * (n2 + RD_NSCAL);
    for (unsigned k = threadIdx.x; k < n2; k += FR_BLOCK) row[k] = ((G[0][k] + G[1][k]) + G[2][k]) + G[3][k];
    if (threadIdx.x < RD_NSCAL) row[n2 + threadIdx.x] = ((shs[0][threadIdx.x] + shs[1][threadIdx.x]) + shs[2][threadIdx.x]) + shs[3][threadIdx.x];
    if (threadIdx.x < RD_NCNT) cnt[(size_t)blockIdx.x * RD_NCNT + threadIdx.x] = shc[0][threadIdx.x] + shc[1][threadIdx.x] + shc[2][threadIdx.x] + shc[3][threadIdx.x];
}

// one level of the fold: workgroup b adds rows [b * RD_FAN, (b + 1) * RD_FAN) of the level below, every element in row order
__global__ void __launch_bounds__(FR_BLOCK) k_rdm1_reduce(const double *in_d, const unsigned long long *in_c, uint32_t n_in, uint32_t stride, double *out_d, unsigned long long *out_c) {
    const size_t lo = (size_t)blockIdx.x * RD_FAN, hi = lo + RD_FAN < n_in ? lo + RD_FAN : n_in;
    for (unsigned k = threadIdx.x; k < stride; k += FR_BLOCK) {
        double x = in_d[lo * stride + k];
        for (size_t j = lo + 1; j < hi; j++) x += in_d[j * stride + k];
        out_d[(size_t)blockIdx.x * stride + k] = x;
    }
    if (threadIdx.x < RD_NCNT) {
        unsigned long long y = 0;
        for (size_t j = lo; j < hi; j++) y += in_c[j * RD_NCNT + threadIdx.x];
        out_c[(size_t)blockIdx.x * RD_NCNT + threadIdx.x] = y;
    }
}

void fr_rdm1(FriesCtx *a, FriesCtx *b, double *gamma, fries_rdm1_result *out) {
    const uint32_t n_pos = fr_pair_begin_rdm("fries_rdm1", a, b);
    fr_rdm1_core("fries_rdm1", a, b->vec, n_pos, gamma, out);
}

// The estimator behind its refusals, as fr_h_dot_core: the first n_pos positions of `a` against B (hs, hcap, v0 and cap are read)
void fr_rdm1_core(const char *who, FriesCtx *a, const VecDev &B, uint32_t n_pos, double *gamma, fries_rdm1_result *out) {
    hipStream_t st = a->stream;
    const size_t n2 = (size_t)a->n_orb * a->n_orb;
    *out = fries_rdm1_result{};
    std::fill(gamma, gamma + n2, 0.0);
    if (n_pos == 0) return;
    // the levels of the fold back to back; sized from n_pos and checked against what the device has left before anything is launched
    const Rdm1Plan plan = fr_rdm1_plan(n_pos, a->n_orb);
    fr_need_free(who, plan.bytes(), "the partial matrices", n_pos);
    DevMem tmp;
    double *d_part = tmp.alloc<double>(plan.total_rows * plan.stride);
    unsigned long long *d_cnt = tmp.alloc<unsigned long long>(plan.total_rows * RD_NCNT);
    FR_LAUNCH(a, "k_rdm1", k_rdm1, dim3(plan.rows[0]), dim3(FR_BLOCK), a->vec, B, a->n_orb, n_pos, d_part, d_cnt);
    size_t off = 0;
    for (size_t l = 0; l + 1 < plan.rows.size(); l++) {
        const size_t nxt = off + plan.rows[l];
        FR_LAUNCH(a, "k_rdm1_reduce", k_rdm1_reduce, dim3(plan.rows[l + 1]), dim3(FR_BLOCK), d_part + off * plan.stride, d_cnt + off * RD_NCNT, plan.rows[l],
                  (uint32_t)plan.stride, d_part + nxt * plan.stride, d_cnt + nxt * RD_NCNT);
        off = nxt;
    }
    std::vector<double> hd(plan.stride); unsigned long long hc[RD_NCNT];
    FR_HIP(hipMemcpyAsync(hd.data(), d_part + plan.last_row() * plan.stride, plan.stride * sizeof(double), hipMemcpyDeviceToHost, st));
    FR_HIP(hipMemcpyAsync(hc, d_cnt + plan.last_row() * RD_NCNT, sizeof(hc), hipMemcpyDeviceToHost, st));
    FR_HIP(hipStreamSynchronize(st));
    std::copy(hd.begin(), hd.begin() + n2, gamma);
    out->ovlp = hd[n2]; out->abs_sum = hd[n2 + 1];
    out->n_src = hc[0]; out->n_terms = hc[1]; out->n_hits = hc[2];
}
