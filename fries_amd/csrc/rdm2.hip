// The spin-summed two-body density matrix between the solution vectors of two contexts, chemists' order:
//   Gamma[p][q][r][s] = sum over sigma, tau of <a| c+_{p sigma} c+_{r tau} c_{s tau} c_{q sigma} |b>.
// Every stored determinant i of `a` with a non-zero value enumerates its same-spin singles, same-spin doubles and opposite-spin doubles
// from bit operations on the determinant -- no rejection and no symmetry table --, looks |j> up in `b`'s hash table and, on a hit, expands
// a_i * sign * b_j into bin records: a double into its direct and (same spin) exchange pairing, a single into one direct and (same spin)
// one exchange record per spectator, the source's own probe into one direct and (same spin) one exchange record per occupied pair.
// Only one of the two records (p,q,r,s) / (r,s,p,q) that every term owns is written: the host adds the accumulated matrix to its own
// pair transpose at the end, so that the two bins are the same bits.
//
// Accumulation and determinism: no floating-point atomics anywhere, kernel boundaries are the only synchronisation.
//   1. k_rdm2_probe<false> probes and counts, per wave, the records its hits expand to (and ovlp, abs_sum and the counters).
//   2. The host cuts the workgroups into chunks whose records fit the capacity (rdm2_plan.hpp) and scans the waves' offsets.
//   3. Per chunk k_rdm2_probe<true> probes again and writes (bin, value) at those offsets, in (position, candidate) order;
//   4. a stable LSD radix sort on the bin (8-bit digits, radix_sort.hpp, shared with the merge's k_rs_* in vec.hip) carries the record's index;
//   5. k_r2_piece adds every bin's records in sorted order in pieces that end at multiples of R2_PIECE, k_r2_fold the pieces in order
//      onto what the chunks before left in the bin.
// The order in which a bin's terms are associated is a function of the positions and the capacity alone.
#include "ctx.hpp"
#include "rdm2_plan.hpp"
#include "pair_frame.hpp"
#include "radix_sort.hpp"

#ifndef R2_ILP
#define R2_ILP 4                // probes a lane has in flight per round
#endif

__device__ __forceinline__ unsigned r2_below(det_t d, unsigned x) { return __popcll(d & ((1ull << x) - 1ull)); }
// t -> (i < j) with t = j (j - 1) / 2 + i
__device__ __forceinline__ void r2_tri(unsigned t, unsigned *i, unsigned *j) {
    unsigned k = (unsigned)((1.0f + sqrtf(1.0f + 8.0f * (float)t)) * 0.5f);
    while (k * (k - 1) / 2 > t) k--;
    while ((k + 1) * k / 2 <= t) k++;
    *j = k; *i = t - k * (k - 1) / 2;
}

struct R2Out { uint32_t *key, *pay; double *val; uint32_t n_rec; };
__device__ __forceinline__ void r2_put(const R2Out &O, uint32_t o, uint32_t bin, double v) {
    if (o < O.n_rec) { O.key[o] = bin; O.pay[o] = o; O.val[o] = v; }
}

// EMIT = false: cnt[wave][R2_NCNT], scal[wave][R2_NSCAL].  EMIT = true: workgroup wg0 + blockIdx.x writes its records at wave_off[wave] + ...
template <bool EMIT>
__global__ void __launch_bounds__(FR_BLOCK) k_rdm2_probe(VecDev A, VecDev B, uint32_t n_orb, uint32_t n_pos, uint32_t wg0,
                                                         unsigned long long *cnt, double *scal, const uint32_t *wave_off, R2Out O) {
    __shared__ uint8_t L[R2_WAVES][4][FR_MAX_ORB];      // per wave: the source's occupied / empty spin orbitals, alpha then beta
    const unsigned w = threadIdx.x >> 6, lane = fr_lane();
    const size_t wave = (size_t)(wg0 + blockIdx.x) * R2_WAVES + w;
    const size_t mine = wave * R2_WPOS + lane;
    unsigned long long my_det = 0; double my_val = 0;
    if (lane < R2_WPOS && mine < n_pos) { my_det = A.dets[mine]; my_val = A.v0[mine]; }
    const det_t lowmask = (1ull << n_orb) - 1ull;       // n_orb <= 32
    const unsigned n2 = n_orb * n_orb, n3 = n2 * n_orb;
    double ov = 0, ab = 0;
    uint32_t n_src = 0, n_hits = 0;
    unsigned long long n_terms = 0, n_rec = 0;
    uint32_t base = EMIT ? wave_off[wave] : 0u;
    for (int s = 0; s < R2_WPOS; s++) {
        PairSrc src;
        if (!src.load(B, my_val, my_det, s, n_orb, lowmask)) continue;
        n_src++;
        const double av = src.av;
        const det_t det = src.det, occ0 = src.occ0, occ1 = src.occ1;
        const unsigned no0 = src.no0, no1 = src.no1, nh0 = n_orb - no0, nh1 = n_orb - no1, n_el = no0 + no1;
        fr_wave_step_fence();
        if (lane < n_orb) {
            const bool o0 = (occ0 >> lane) & 1ull, o1 = (occ1 >> lane) & 1ull;
            L[w][o0 ? 0 : 1][r2_below(o0 ? occ0 : ~occ0 & lowmask, lane)] = (uint8_t)lane;
            L[w][o1 ? 2 : 3][r2_below(o1 ? occ1 : ~occ1 & lowmask, lane)] = (uint8_t)(lane + n_orb);
        }
        fr_wave_step_fence();
        const unsigned ns0 = no0 * nh0, ns1 = no1 * nh1;
        const unsigned nq0 = nh0 * (nh0 - 1) / 2, nq1 = nh1 * (nh1 - 1) / 2;
        const unsigned nd0 = no0 * (no0 - 1) / 2 * nq0, nd1 = no1 * (no1 - 1) / 2 * nq1;
        const unsigned e_s1 = ns0 + ns1, e_d0 = e_s1 + nd0, e_d1 = e_d0 + nd1, n_cand = e_d1 + ns0 * ns1;
        n_terms += n_cand;
        for (unsigned c0 = 0; c0 < n_cand; c0 += FR_WAVE * R2_ILP) {
            det_t nd[R2_ILP]; double sg[R2_ILP]; uint32_t sl[R2_ILP], orbs[R2_ILP]; HSlot e[R2_ILP];
#pragma unroll
            for (int k = 0; k < R2_ILP; k++) {
                const unsigned idx = c0 + k * FR_WAVE + lane;
                sg[k] = 0; nd[k] = det; orbs[k] = 0; sl[k] = 0;
                e[k].key = FR_EMPTY_KEY; e[k].val = FR_NOPOS;
                if (idx < n_cand) {
                    unsigned P, Q, R = 64, S = 64;      // c+_P c+_R c_S c_Q |j>; R = S = 64: a single
                    if (idx < e_s1) {
                        const unsigned sp = idx >= ns0, c = sp ? idx - ns0 : idx, nh = sp ? nh1 : nh0;
                        P = L[w][2 * sp][c / nh]; Q = L[w][2 * sp + 1][c % nh];
                    } else if (idx < e_d1) {
                        const unsigned sp = idx >= e_d0, c = sp ? idx - e_d0 : idx - e_s1, nq = sp ? nq1 : nq0;
                        unsigned i1, i2, j1, j2;
                        r2_tri(c / nq, &i1, &i2); r2_tri(c % nq, &j1, &j2);
                        P = L[w][2 * sp][i1]; R = L[w][2 * sp][i2]; Q = L[w][2 * sp + 1][j1]; S = L[w][2 * sp + 1][j2];
                    } else {
                        const unsigned c = idx - e_d1, ca = c / ns1, cb = c % ns1;
                        P = L[w][0][ca / nh0]; Q = L[w][1][ca % nh0]; R = L[w][2][cb / nh1]; S = L[w][3][cb % nh1];
                    }
                    det_t j = det ^ (1ull << P) ^ (1ull << Q);
                    if (R < 64) j ^= (1ull << R) ^ (1ull << S);
                    nd[k] = j;
                    // the sign of c+_P c+_R c_S c_Q |j>: every operator counts the occupied spin orbitals below it at its turn
                    unsigned par = r2_below(j, Q); j ^= 1ull << Q;
                    if (R < 64) { par += r2_below(j, S); j ^= 1ull << S; par += r2_below(j, R); j ^= 1ull << R; }
                    par += r2_below(j, P);
                    sg[k] = (par & 1u) ? -1.0 : 1.0;
                    orbs[k] = P | (Q << 8) | (R << 16) | (S << 24);
                    sl[k] = fr_hash_slot(nd[k], B.hcap);
                    e[k] = B.hs[sl[k]];         // the round's first probes are independent of each other
                }
            }
#pragma unroll
            for (int k = 0; k < R2_ILP; k++) {
                double t = 0; uint32_t nr = 0;
                const unsigned P = orbs[k] & 255u, Q = (orbs[k] >> 8) & 255u, R = (orbs[k] >> 16) & 255u, S = orbs[k] >> 24;
                if (sg[k] != 0) {
                    const double bv = hd_resolve(B, nd[k], sl[k], e[k]);
                    if (bv != 0) {
                        t = av * sg[k] * bv;
                        ab += fabs(t); n_hits++;
                        if (R == 64) nr = (n_el - 1) + ((P >= n_orb ? no1 : no0) - 1);
                        else nr = ((P >= n_orb) == (R >= n_orb)) ? 2u : 1u;
                    }
                }
                if (__ballot(nr != 0) == 0ull) continue;        // uniform
                uint32_t tot;
                uint32_t o = base + fr_wave_excl_u32(nr, &tot);
                base += tot; n_rec += tot;
                if (EMIT && nr) {
                    const unsigned p = P % n_orb, q = Q % n_orb;
                    if (R == 64) {
                        const bool beta = P >= n_orb;
                        for (det_t m = det & ~(1ull << P); m; m &= m - 1) {         // the spectators: occupied in both
                            const unsigned K = __ffsll((long long)m) - 1, kk = K % n_orb;
                            r2_put(O, o++, p * n3 + q * n2 + kk * n_orb + kk, t);
                            if ((K >= n_orb) == beta) r2_put(O, o++, p * n3 + kk * n2 + kk * n_orb + q, -t);
                        }
                    } else {
                        const unsigned r = R % n_orb, ss = S % n_orb;
                        r2_put(O, o++, p * n3 + q * n2 + r * n_orb + ss, t);
                        if (nr == 2) r2_put(O, o++, p * n3 + ss * n2 + r * n_orb + q, -t);
                    }
                }
            }
        }
        // the source itself in b: the overlap and the diagonal, one direct and (same spin) one exchange record per occupied pair P < R
        const double t = av * hd_resolve(B, det, src.sl0, src.e0);
        if (t != 0) {
            if (lane == 0) ov += t;
            const unsigned n_pair = n_el * (n_el - 1) / 2;
            for (unsigned c0 = 0; c0 < n_pair; c0 += FR_WAVE) {
                const unsigned c = c0 + lane;
                unsigned i1 = 0, i2 = 0, P = 0, R = 0; uint32_t nr = 0;
                if (c < n_pair) {
                    r2_tri(c, &i1, &i2);
                    P = i1 < no0 ? L[w][0][i1] : L[w][2][i1 - no0];
                    R = i2 < no0 ? L[w][0][i2] : L[w][2][i2 - no0];
                    nr = ((P >= n_orb) == (R >= n_orb)) ? 2u : 1u;
                }
                uint32_t tot;
                uint32_t o = base + fr_wave_excl_u32(nr, &tot);
                base += tot; n_rec += tot;
                if (EMIT && nr) {
                    const unsigned p = P % n_orb, r = R % n_orb;
                    r2_put(O, o++, p * n3 + p * n2 + r * n_orb + r, t);
                    if (nr == 2) r2_put(O, o++, p * n3 + r * n2 + r * n_orb + p, -t);
                }
            }
        }
    }
    if (!EMIT) {
        ab = fr_wave_sum(ab);
        n_hits = fr_wave_sum_u32(n_hits);
        if (lane == 0) {
            cnt[wave * R2_NCNT + 0] = n_src; cnt[wave * R2_NCNT + 1] = n_terms; cnt[wave * R2_NCNT + 2] = n_hits; cnt[wave * R2_NCNT + 3] = n_rec;
            scal[wave * R2_NSCAL + 0] = ov; scal[wave * R2_NSCAL + 1] = ab;
        }
    }
}

// ------------------------------------------------------------------ stable LSD radix sort, 8-bit digits (radix_sort.hpp; the length by value)
static_assert(R2_TILE == RS_TILE, "fr_rdm2_scratch sizes the histograms in R2_TILE");
__global__ void __launch_bounds__(FR_BLOCK) k_r2_hist(const uint32_t *key, uint32_t n, uint32_t *hist, int shift, uint32_t nblk) {
    fr_rs_hist_tile(key, n, hist, shift, nblk);
}
// one block per digit
__global__ void __launch_bounds__(FR_BLOCK) k_r2_scan(uint32_t *hist, uint32_t nblk) {
    fr_rs_scan_digit(hist, nblk, nblk);
}
__global__ void __launch_bounds__(FR_BLOCK) k_r2_scatter(const uint32_t *key, const uint32_t *pay, uint32_t *key_out, uint32_t *pay_out,
                                                         uint32_t n, const uint32_t *hist, int shift, uint32_t nblk) {
    fr_rs_scatter_tile(key, pay, key_out, pay_out, n, hist, shift, nblk);
}

// ------------------------------------------------------------------ segmented in-order sum
// the record that starts a piece -- its bin differs from the one before, or its sorted index is a multiple of R2_PIECE -- adds its piece up
__global__ void __launch_bounds__(FR_BLOCK) k_r2_piece(const uint32_t *key, const uint32_t *pay, const double *val, uint32_t n, double *psum) {
    const size_t j = (size_t)blockIdx.x * FR_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t k = key[j];
    if (j % R2_PIECE != 0 && key[j - 1] == k) return;
    double x = val[pay[j]];
    for (size_t m = j + 1; m < n && m % R2_PIECE != 0 && key[m] == k; m++) x += val[pay[m]];
    psum[j] = x;
}
// the record that starts a bin adds the bin's pieces, in order, onto what the chunks before left in G
__global__ void __launch_bounds__(FR_BLOCK) k_r2_fold(const uint32_t *key, uint32_t n, const double *psum, double *G, uint32_t n_bins) {
    const size_t j = (size_t)blockIdx.x * FR_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t k = key[j];
    if ((j != 0 && key[j - 1] == k) || k >= n_bins) return;
    double x = G[k] + psum[j];
    for (size_t m = (j / R2_PIECE + 1) * R2_PIECE; m < n && key[m] == k; m += R2_PIECE) x += psum[m];
    G[k] = x;
}

void fr_rdm2(FriesCtx *a, FriesCtx *b, double *gamma2, fries_rdm2_result *out) {
    const uint32_t n_pos = fr_pair_begin_rdm("fries_rdm2", a, b);
    fr_rdm2_core("fries_rdm2", a, b->vec, n_pos, gamma2, out);
}

// The estimator behind its refusals, as fr_h_dot_core: the first n_pos positions of `a` against B (hs, hcap, v0 and cap are read);
// the matrix it returns is already added to its own pair transpose.  In two halves, so that a caller with several enumerating vectors
// (fr_rdm2_ranks) can run every counting pass and make every capacity refusal before a single record is written.
void fr_rdm2_core(const char *who, FriesCtx *a, const VecDev &B, uint32_t n_pos, double *gamma2, fries_rdm2_result *out) {
    Rdm2Pass p;
    fr_rdm2_count(who, a, B, n_pos, p, gamma2, out);
    fr_rdm2_refuse(who, a, p, "");
    fr_rdm2_emit(who, a, B, p, gamma2);
}

// The counting pass: zeroes the outputs, probes everything once, adds the waves' scalars and counts into *out and cuts the workgroups
// into chunks.  A workgroup beyond the capacity is left in p.plan.bad_wg for fr_rdm2_refuse.
void fr_rdm2_count(const char *who, FriesCtx *a, const VecDev &B, uint32_t n_pos, Rdm2Pass &p, double *gamma2, fries_rdm2_result *out) {
    hipStream_t st = a->stream;
    const uint32_t n = a->n_orb;
    const size_t n2 = (size_t)n * n, n4 = n2 * n2;
    *out = fries_rdm2_result{};
    std::fill(gamma2, gamma2 + n4, 0.0);
    p.n_pos = n_pos;
    if (n_pos == 0) return;
    const uint32_t n_wg = p.n_wg = fr_blocks(n_pos, R2_BPOS);
    const size_t n_waves = p.n_waves = (size_t)n_wg * R2_WAVES;
    // the counting pass: its arrays and the matrix are sized from n_pos and n_orb and checked before anything is launched
    fr_need_free(who, n_waves * (R2_NCNT + R2_NSCAL + 1) * 8 + n4 * 8, "the matrix and the counters", n_pos);
    DevMem &tmp = p.tmp;
    unsigned long long *d_cnt = tmp.alloc<unsigned long long>(n_waves * R2_NCNT);
    double *d_scal = tmp.alloc<double>(n_waves * R2_NSCAL);
    p.d_G = tmp.alloc<double>(n4);
    p.d_off = tmp.alloc<uint32_t>(n_waves);
    FR_LAUNCH(a, "k_rdm2_count", (k_rdm2_probe<false>), dim3(n_wg), dim3(FR_BLOCK), a->vec, B, n, n_pos, 0u, d_cnt, d_scal, (const uint32_t *)nullptr, R2Out{});
    std::vector<unsigned long long> hc(n_waves * R2_NCNT);
    std::vector<double> hs(n_waves * R2_NSCAL);
    FR_HIP(hipMemcpyAsync(hc.data(), d_cnt, hc.size() * 8, hipMemcpyDeviceToHost, st));
    FR_HIP(hipMemcpyAsync(hs.data(), d_scal, hs.size() * 8, hipMemcpyDeviceToHost, st));
    FR_HIP(hipStreamSynchronize(st));
    // the waves' scalars in wave order
    std::vector<uint64_t> wave_rec(n_waves);
    for (size_t w = 0; w < n_waves; w++) {
        out->n_src += hc[w * R2_NCNT]; out->n_terms += hc[w * R2_NCNT + 1]; out->n_hits += hc[w * R2_NCNT + 2];
        wave_rec[w] = hc[w * R2_NCNT + 3];
        out->ovlp += hs[w * R2_NSCAL]; out->abs_sum += hs[w * R2_NSCAL + 1];
    }
    p.plan = fr_rdm2_cut(wave_rec.data(), n_wg, a->rdm2_records);
}

// where = "" or which of several enumerating vectors is meant (" of shard 1")
void fr_rdm2_refuse(const char *who, const FriesCtx *a, const Rdm2Pass &p, const char *where) {
    if (p.plan.bad_wg < 0) return;
    std::ostringstream os;
    os << who << ": the " << R2_BPOS << " positions from " << (uint64_t)p.plan.bad_wg * R2_BPOS << where << " expand to " << p.plan.bad_need
       << " bin records, the capacity of a chunk is " << a->rdm2_records << " (FRIES_RDM2_RECORDS)";
    throw FriesError(os.str());
}

// Per chunk: emit, sort, sum; then the matrix plus its pair transpose into gamma2 (which fr_rdm2_count zeroed)
void fr_rdm2_emit(const char *who, FriesCtx *a, const VecDev &B, Rdm2Pass &p, double *gamma2) {
    if (p.n_pos == 0 || p.plan.total_rec == 0) return;
    hipStream_t st = a->stream;
    const uint32_t n = a->n_orb, n_pos = p.n_pos;
    const size_t n2 = (size_t)n * n, n4 = n2 * n2, n_waves = p.n_waves;
    const Rdm2Plan &plan = p.plan;
    const uint64_t cap = a->rdm2_records;
    DevMem &tmp = p.tmp;
    double *d_G = p.d_G; uint32_t *d_off = p.d_off;
    const Rdm2Scratch sc = fr_rdm2_scratch(plan.max_rec);
    if (a->dbg >= 1)
        fprintf(stderr, "[fries] %s: %llu bin records in %zu chunks of at most %llu (capacity %llu), scratch %zu bytes\n", who, (unsigned long long)plan.total_rec,
                plan.chunks.size(), (unsigned long long)plan.max_rec, (unsigned long long)cap, sc.bytes);
    fr_need_free(who, sc.bytes, "the bin records", n_pos);
    uint8_t *d_sc = tmp.alloc<uint8_t>(sc.bytes);
    FR_HIP(hipMemsetAsync(d_G, 0, n4 * 8, st));
    FR_HIP(hipMemcpyAsync(d_off, plan.wave_off.data(), n_waves * 4, hipMemcpyHostToDevice, st));
    const int passes = fr_rdm2_passes(n);
    for (const Rdm2Chunk &ch : plan.chunks) {
        if (ch.n_rec == 0) continue;
        const uint32_t nr = (uint32_t)ch.n_rec, nblk = fr_blocks(nr, R2_TILE);
        uint32_t *key[2] = {(uint32_t *)(d_sc + sc.key(0)), (uint32_t *)(d_sc + sc.key(1))};
        uint32_t *pay[2] = {(uint32_t *)(d_sc + sc.pay(0, plan.max_rec)), (uint32_t *)(d_sc + sc.pay(1, plan.max_rec))};
        double *val = (double *)(d_sc + sc.val);
        uint32_t *hist = (uint32_t *)(d_sc + sc.hist);
        FR_LAUNCH(a, "k_rdm2_emit", (k_rdm2_probe<true>), dim3(ch.wg_hi - ch.wg_lo), dim3(FR_BLOCK), a->vec, B, n, n_pos, ch.wg_lo,
                  (unsigned long long *)nullptr, (double *)nullptr, (const uint32_t *)d_off, R2Out{key[0], pay[0], val, nr});
        int src = 0;
        for (int p = 0; p < passes; p++, src ^= 1) {
            FR_LAUNCH(a, "k_r2_hist", k_r2_hist, dim3(nblk), dim3(FR_BLOCK), key[src], nr, hist, 8 * p, nblk);
            FR_LAUNCH(a, "k_r2_scan", k_r2_scan, dim3(256), dim3(FR_BLOCK), hist, nblk);
            FR_LAUNCH(a, "k_r2_scatter", k_r2_scatter, dim3(nblk), dim3(FR_BLOCK), key[src], pay[src], key[src ^ 1], pay[src ^ 1], nr, hist, 8 * p, nblk);
        }
        double *psum = (double *)(d_sc + sc.blk[src ^ 1]);
        FR_LAUNCH(a, "k_r2_piece", k_r2_piece, dim3(fr_blocks(nr, FR_BLOCK)), dim3(FR_BLOCK), key[src], pay[src], val, nr, psum);
        FR_LAUNCH(a, "k_r2_fold", k_r2_fold, dim3(fr_blocks(nr, FR_BLOCK)), dim3(FR_BLOCK), key[src], nr, psum, d_G, (uint32_t)n4);
    }
    std::vector<double> hg(n4);
    FR_HIP(hipMemcpyAsync(hg.data(), d_G, n4 * 8, hipMemcpyDeviceToHost, st));
    FR_HIP(hipStreamSynchronize(st));
    // every term owns the records (p,q,r,s) and (r,s,p,q), one of which was written: the two bins are the same sum
    for (size_t pq = 0; pq < n2; pq++)
        for (size_t rs = 0; rs < n2; rs++) gamma2[pq * n2 + rs] = hg[pq * n2 + rs] + hg[rs * n2 + pq];
}
