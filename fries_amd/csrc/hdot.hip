// <a|H|b> and <a|b> between the solution vectors of two contexts (the reference's calc_h_dot, FRIES/Hamiltonians/molecule.cpp:667-885,
// with DistVec::internal_dot for the overlap): every stored determinant of `a` enumerates its symmetry-allowed singles and doubles
// exactly as k_enum does (enum_rows.hpp), and each target with a non-zero element is looked up in `b`'s hash table.  Nothing is
// merged and nothing per excitation is written: the traffic is the sources, the integrals and one 16-byte probe per non-zero element.
//
// Shape: one workgroup per position of `a` (a hole or a zeroed entry leaves at once), the singles and doubles of the source as one
// candidate index space walked in strides of the block, rejection over the candidate index as in k_enum.  A lane takes HD_ILP
// candidates per round and issues their first probes together before it resolves any of them: most probes end on an empty slot, so
// the round costs one memory latency, not HD_ILP of them.
//
// Determinism: no floating-point atomics.  A lane adds its terms in ascending candidate order; the block combines the lanes in the
// fixed tree of fr_block_sum; the per-source partials are reduced in chunks of HD_CHUNK by the same tree, level by level, until one
// value is left.  The association order is a function of curr_size alone, so two calls on the same vectors return the same bits.
#include "ctx.hpp"
#include "enum_rows.hpp"
#include "pair_frame.hpp"       // fr_pair_begin, hd_resolve: shared with fr_rdm1 and fr_rdm2

#define HD_ILP 4
#define HD_CHUNK 4096

// part: [6][n_pos] as doubles h, ovlp, abs_sum and (in cnt) n_src, n_terms, n_hits of every position
__global__ void __launch_bounds__(FR_BLOCK) k_hdot(VecDev A, VecDev B, SysDev S, uint32_t n_pos, double *part, unsigned long long *cnt) {
    __shared__ HbTables T;
    __shared__ double shd[4];
    __shared__ uint32_t shu[4];
    const uint32_t i = blockIdx.x;
    if (i >= n_pos) return;
    const double av = A.v0[i];
    if (av == 0) {      // hole or zeroed entry (uniform over the block)
        if (threadIdx.x < 3) { part[(size_t)threadIdx.x * n_pos + i] = 0.0; cnt[(size_t)threadIdx.x * n_pos + i] = 0ull; }
        return;
    }
    fr_stage_tables(&T, S.hb);
    const det_t det = A.dets[i];
    const unsigned n = T.n_orb, ne = T.n_elec;
    double h = 0, ov = 0, ab = 0;
    uint32_t n_terms = 0, n_hits = 0;
    if (threadIdx.x == 0) {
        // the diagonal, as the engine caches it (minus hf_en); `a` is not written, so an entry that has none yet is evaluated here
        const uint32_t s = fr_hash_slot(det, B.hcap);
        const double bv = hd_resolve(B, det, s, B.hs[s]);
        if (bv != 0) {
            double d = A.diag[i];
            if (d != d) d = fr_diag_matrel(det, S.h_core, S.eris, S.n_orb) - S.hf_en;
            const double t = av * d * bv;
            ov = av * bv; h = t; ab = fabs(t);
        }
    }
    const uint32_t n_sing = fr_enum_n_cand(n, ne, 0), n_cand = n_sing + fr_enum_n_cand(n, ne, 1);
    for (uint32_t c0 = 0; c0 < n_cand; c0 += FR_BLOCK * HD_ILP) {
        det_t nd[HD_ILP]; double m[HD_ILP]; uint32_t sl[HD_ILP]; HSlot e[HD_ILP];
#pragma unroll
        for (int k = 0; k < HD_ILP; k++) {
            const uint32_t idx = c0 + k * FR_BLOCK + threadIdx.x;
            unsigned o1, o2, u1, u2;
            m[k] = 0; nd[k] = det;
            const bool ok = idx < n_cand && fr_enum_element(T, S, det, idx < n_sing ? 0 : 1, idx < n_sing ? idx : idx - n_sing, &nd[k], &m[k], &o1, &o2, &u1, &u2);
            if (!ok) m[k] = 0;
            sl[k] = fr_hash_slot(nd[k], B.hcap);
            e[k].key = FR_EMPTY_KEY; e[k].val = FR_NOPOS;
            if (m[k] != 0) e[k] = B.hs[sl[k]];         // the round's first probes are independent of each other
        }
#pragma unroll
        for (int k = 0; k < HD_ILP; k++) {
            if (m[k] == 0) continue;
            n_terms++;
            const double bv = hd_resolve(B, nd[k], sl[k], e[k]);
            if (bv != 0) {
                const double t = av * m[k] * bv;
                h += t; ab += fabs(t); n_hits++;
            }
        }
    }
    h = fr_block_sum(h, shd); ov = fr_block_sum(ov, shd); ab = fr_block_sum(ab, shd);
    n_terms = fr_block_sum_u32(n_terms, shu); n_hits = fr_block_sum_u32(n_hits, shu);
    if (threadIdx.x == 0) {
        part[i] = h; part[(size_t)n_pos + i] = ov; part[2 * (size_t)n_pos + i] = ab;
        cnt[i] = 1ull; cnt[(size_t)n_pos + i] = n_terms; cnt[2 * (size_t)n_pos + i] = n_hits;
    }
}

// one level of the fixed reduction tree: block b folds entries [b * HD_CHUNK, (b + 1) * HD_CHUNK) of each of the six rows ([row][n_in] ->
// [row][gridDim.x]); a lane adds its strided slice in index order, the block combines the lanes as fr_block_sum does
__global__ void __launch_bounds__(FR_BLOCK) k_hdot_reduce(const double *in_d, const unsigned long long *in_c, uint32_t n_in, double *out_d, unsigned long long *out_c) {
    __shared__ double shd[4];
    __shared__ unsigned long long shc[4];
    const size_t lo = (size_t)blockIdx.x * HD_CHUNK, hi = lo + HD_CHUNK < n_in ? lo + HD_CHUNK : n_in;
    for (int row = 0; row < 3; row++) {
        double x = 0; unsigned long long y = 0;
        for (size_t j = lo + threadIdx.x; j < hi; j += FR_BLOCK) { x += in_d[(size_t)row * n_in + j]; y += in_c[(size_t)row * n_in + j]; }
        x = fr_block_sum(x, shd);
        for (int off = 32; off > 0; off >>= 1) y += __shfl_xor(y, off);
        if (fr_lane() == 0) shc[threadIdx.x >> 6] = y;
        __syncthreads();
        y = shc[0] + shc[1] + shc[2] + shc[3];
        __syncthreads();
        if (threadIdx.x == 0) { out_d[(size_t)row * gridDim.x + blockIdx.x] = x; out_c[(size_t)row * gridDim.x + blockIdx.x] = y; }
    }
}

void fr_h_dot(FriesCtx *a, FriesCtx *b, fries_hdot_result *out) {
    const uint32_t n_pos = fr_pair_begin("fries_h_dot", a, b);
    if (a->hf_en != b->hf_en) throw FriesError("fries_h_dot: the two contexts differ in hf_en, the offset of the diagonal (different molecules or --ham_shift)");
    if (a->spin_parity != b->spin_parity) throw FriesError("fries_h_dot: the two contexts differ in spin_parity");
    fr_h_dot_core(a, b->vec, n_pos, out);
}

// The estimator behind its refusals: the first n_pos positions of `a` against B, of which the kernels read hs, hcap, v0 and cap only
// (another context's vector, or a snapshot's view); on a's stream, back when the result is on the host.
void fr_h_dot_core(FriesCtx *a, const VecDev &B, uint32_t n_pos, fries_hdot_result *out) {
    hipStream_t st = a->stream;
    *out = fries_hdot_result{};
    if (n_pos == 0) return;
    const SysDev S = fr_sysdev(a);
    // the levels of the tree back to back: [3][n_pos], [3][ceil(n_pos / HD_CHUNK)], ... down to [3][1]
    size_t total = n_pos;
    for (uint32_t n = n_pos;;) { n = fr_blocks(n, HD_CHUNK); total += n; if (n <= 1) break; }
    DevMem tmp;
    double *d_part = tmp.alloc<double>(3 * total);
    unsigned long long *d_cnt = tmp.alloc<unsigned long long>(3 * total);
    FR_LAUNCH(a, "k_hdot", k_hdot, dim3(n_pos), dim3(FR_BLOCK), a->vec, B, S, n_pos, d_part, d_cnt);
    size_t off = 0;
    uint32_t n = n_pos;
    do {
        const uint32_t nb = fr_blocks(n, HD_CHUNK);
        FR_LAUNCH(a, "k_hdot_reduce", k_hdot_reduce, dim3(nb), dim3(FR_BLOCK), d_part + 3 * off, d_cnt + 3 * off, n, d_part + 3 * (off + n), d_cnt + 3 * (off + n));
        off += n; n = nb;
    } while (n > 1);
    double hd[3]; unsigned long long hc[3];
    FR_HIP(hipMemcpyAsync(hd, d_part + 3 * off, sizeof(hd), hipMemcpyDeviceToHost, st));
    FR_HIP(hipMemcpyAsync(hc, d_cnt + 3 * off, sizeof(hc), hipMemcpyDeviceToHost, st));
    FR_HIP(hipStreamSynchronize(st));
    out->h = hd[0]; out->ovlp = hd[1]; out->abs_sum = hd[2];
    out->n_src = hc[0]; out->n_terms = hc[1]; out->n_hits = hc[2];
}
