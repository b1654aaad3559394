// The extern "C" boundary of the test hooks, the profiling helpers, the statistics and the generator's state (include/fries_hip.h),
// with the kernels only the test hooks launch.
#include "api.hpp"
#include <cmath>

extern "C" int fries_test_piv_adjust(fries_ctx *h, uint32_t *n_samp_loc, double exp_nsamp_loc, uint32_t n_samp_tot, double tot_norm, double *new_norm, uint8_t *flags_out) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        fr_test_piv_adjust(c, n_samp_loc, exp_nsamp_loc, n_samp_tot, tot_norm, new_norm, flags_out);
        fr_check_dev_err(c);
    });
}

__global__ void k_test_teeth(Teeth *t, double r0, double unit, uint32_t n, double *pos, const double *q, uint32_t nq, uint32_t *below) {
    if (blockIdx.x == 0 && threadIdx.x == 0) fr_build_teeth(t, r0, unit, n, 0.0);
}
__global__ void k_test_teeth_eval(const Teeth *t, uint32_t n, double *pos, const double *q, uint32_t nq, uint32_t *below) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) pos[i] = fr_tooth(t, i);
    if (i < nq) below[i] = fr_teeth_below(t, q[i]);
}

extern "C" int fries_test_teeth(fries_ctx *h, double r0, double unit, uint32_t n, double *out_pos, const double *query, uint32_t nq, uint32_t *out_below) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        DevMem tmp;
        Teeth *t = tmp.alloc<Teeth>(1);
        double *dp = tmp.alloc<double>(n), *dq = tmp.alloc<double>(nq);
        uint32_t *db = tmp.alloc<uint32_t>(nq);
        if (nq) FR_HIP(hipMemcpy(dq, query, 8 * (size_t)nq, hipMemcpyHostToDevice));
        FR_LAUNCH(c, "k_test_teeth", k_test_teeth, dim3(1), dim3(1), t, r0, unit, n, dp, dq, nq, db);
        uint32_t m = n > nq ? n : nq;
        FR_LAUNCH(c, "k_test_teeth_eval", k_test_teeth_eval, dim3(fr_blocks(m ? m : 1, FR_BLOCK)), dim3(FR_BLOCK), t, n, dp, dq, nq, db);
        FR_HIP(hipStreamSynchronize(c->stream));
        if (n) FR_HIP(hipMemcpy(out_pos, dp, 8 * (size_t)n, hipMemcpyDeviceToHost));
        if (nq) FR_HIP(hipMemcpy(out_below, db, 4 * (size_t)nq, hipMemcpyDeviceToHost));
    });
}

// ------------------------------------------------------------------ test hook: exact in-order prefix sums
struct AccArr {
    const double *a; unsigned n;
    __device__ unsigned count() const { return n; }
    __device__ double get(size_t i) const { return a[i]; }
};
__global__ void __launch_bounds__(FR_BLOCK) k_test_seq_apply(SeqWork Q, AccArr acc, double *out) {
    __shared__ SeqShared sh;
    double S[4], Sb;
    fr_seq_prefix4(Q, acc, blockIdx.x, &sh, S, &Sb);
    size_t base = (size_t)blockIdx.x * FR_SEQ_TILE + (size_t)threadIdx.x * 4;
    for (int it = 0; it < 4; it++) if (base + it < acc.n) out[base + it] = S[it];
}

extern "C" int fries_test_seqsum(fries_ctx *h, const double *vals, uint32_t n, double start, double *out_prefix, double *out_total, uint32_t *n_dirty_tiles, uint32_t *n_dirty_subs) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        unsigned ntile = fr_blocks(n ? n : 1, FR_SEQ_TILE);
        if (ntile > FR_MAX_PART) throw FriesError("too many elements");
        DevMem tmp;
        SeqWork Q;
        Q.tiles = tmp.alloc<SeqRec>(ntile); Q.subs = tmp.alloc<SeqRec>((size_t)ntile * FR_SUBS_PER_TILE); Q.total = tmp.alloc<double>(1); Q.tsum = tmp.alloc<double>(ntile);
        double *da = tmp.alloc<double>(n), *dout = tmp.alloc<double>(n);
        FR_HIP(hipMemcpy(da, vals, 8 * (size_t)n, hipMemcpyHostToDevice));
        FR_HIP(hipMemset(Q.subs, 0, sizeof(SeqRec) * (size_t)ntile * FR_SUBS_PER_TILE));
        AccArr acc{da, n};
        double *dstart = tmp.alloc<double>(1);
        FR_HIP(hipMemcpy(dstart, &start, 8, hipMemcpyHostToDevice));
        SeqStart from; from.norms = dstart; from.n = 1;      // 0 + start == start
        FR_LAUNCH(c, "k_seq_sums", (k_seq_sums<AccArr>), dim3(ntile), dim3(FR_BLOCK), Q, acc);
        FR_LAUNCH(c, "k_seq_maps", (k_seq_maps<AccArr>), dim3(ntile), dim3(FR_BLOCK), Q, acc, from);
        FR_LAUNCH(c, "k_seq_chain", (k_seq_chain<AccArr>), dim3(1), dim3(FR_BLOCK), Q, acc, from);
        FR_LAUNCH(c, "k_test_seq_apply", k_test_seq_apply, dim3(ntile), dim3(FR_BLOCK), Q, acc, dout);
        FR_HIP(hipStreamSynchronize(c->stream));
        FR_HIP(hipMemcpy(out_prefix, dout, 8 * (size_t)n, hipMemcpyDeviceToHost));
        FR_HIP(hipMemcpy(out_total, Q.total, 8, hipMemcpyDeviceToHost));
        std::vector<SeqRec> tl(ntile), sb((size_t)ntile * FR_SUBS_PER_TILE);
        FR_HIP(hipMemcpy(tl.data(), Q.tiles, sizeof(SeqRec) * ntile, hipMemcpyDeviceToHost));
        FR_HIP(hipMemcpy(sb.data(), Q.subs, sizeof(SeqRec) * sb.size(), hipMemcpyDeviceToHost));
        uint32_t dt = 0, ds = 0;
        for (unsigned t = 0; t < ntile; t++) if (tl[t].dirty) { dt++; for (int j = 0; j < FR_SUBS_PER_TILE; j++) if (sb[(size_t)t * FR_SUBS_PER_TILE + j].dirty) ds++; }
        if (n_dirty_tiles) *n_dirty_tiles = dt;
        if (n_dirty_subs) *n_dirty_subs = ds;
    });
}

// ------------------------------------------------------------------ profiling
extern "C" int fries_prof_enable(fries_ctx *h, int on) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        fr_prof_collect(c);
        c->prof_on = on != 0;
        if (on) c->prof_agg.clear();
    });
}
extern "C" int fries_prof_count(fries_ctx *h) {
    if (fr_api_dev(h, [&](FriesCtx *c) { fr_prof_collect(c); })) return -1;     // spans recorded by the single-operator entry points
    return (int)h->c.prof_agg.size();
}
extern "C" int fries_prof_get(fries_ctx *h, int i, char *name, size_t name_cap, double *total_ms, uint64_t *calls) {
    return fr_api_host(h, [&](FriesCtx *c) {
        if (i < 0 || i >= (int)c->prof_agg.size()) throw FriesError("profile index out of range");
        const ProfAgg &a = c->prof_agg[i];
        snprintf(name, name_cap, "%s", a.name.c_str());
        *total_ms = a.ms; *calls = a.calls;
    });
}
// device-to-device copy bandwidth of this GPU (bytes read + bytes written per second), the measured denominator beside the
// nominal HBM peak
extern "C" int fries_measure_copy_bandwidth(fries_ctx *h, size_t bytes, int reps, double *gb_per_s) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        DevMem tmp;
        void *a = tmp.alloc<uint8_t>(bytes), *b = tmp.alloc<uint8_t>(bytes);
        FR_HIP(hipMemsetAsync(a, 1, bytes, c->stream));
        FR_HIP(hipMemcpyAsync(b, a, bytes, hipMemcpyDeviceToDevice, c->stream));
        hipEvent_t e0, e1;
        FR_HIP(hipEventCreate(&e0)); FR_HIP(hipEventCreate(&e1));
        FR_HIP(hipEventRecord(e0, c->stream));
        for (int k = 0; k < reps; k++) FR_HIP(hipMemcpyAsync(b, a, bytes, hipMemcpyDeviceToDevice, c->stream));
        FR_HIP(hipEventRecord(e1, c->stream));
        FR_HIP(hipStreamSynchronize(c->stream));
        float ms = 0;
        FR_HIP(hipEventElapsedTime(&ms, e0, e1));
        *gb_per_s = 2.0 * (double)bytes * reps / (ms * 1e-3) / 1e9;
        hipEventDestroy(e0); hipEventDestroy(e1);
    });
}

// ------------------------------------------------------------------ statistics
extern "C" int fries_tie_margins(fries_ctx *h, int enable, double *fks_min_rel, double *fp_min_rel) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        const uint32_t inf2[2] = {0x7F800000u, 0x7F800000u};
        if (c->d_tie) {
            uint32_t v[2];
            FR_HIP(hipMemcpyAsync(v, c->d_tie, 8, hipMemcpyDeviceToHost, c->stream));
            FR_HIP(hipStreamSynchronize(c->stream));
            float f0, f1; memcpy(&f0, &v[0], 4); memcpy(&f1, &v[1], 4);
            if (fks_min_rel) *fks_min_rel = f0;
            if (fp_min_rel) *fp_min_rel = f1;
            FR_HIP(hipMemcpyAsync(c->d_tie, inf2, 8, hipMemcpyHostToDevice, c->stream));       // the statistics restart
            FR_HIP(hipStreamSynchronize(c->stream));
        }
        else { if (fks_min_rel) *fks_min_rel = INFINITY; if (fp_min_rel) *fp_min_rel = INFINITY; }
        if (enable && !c->d_tie) { c->d_tie = c->mem.alloc<uint32_t>(2); FR_HIP(hipMemcpy(c->d_tie, inf2, 8, hipMemcpyHostToDevice)); }
        if (!enable) c->mem.release(c->d_tie);
    });
}
extern "C" int fries_piv_stats(fries_ctx *h, uint64_t *n_certified, uint64_t *n_fallback) {
    if (n_certified) *n_certified = h->c.piv.n_certified;
    if (n_fallback) *n_fallback = h->c.piv.n_fallback;
    return (int)h->c.piv.last_reason;      // why the last fallback happened: 1 cut point near a border, 2 divmod, 4 walk, 8 candidate draw, 16 pass draw
}
extern "C" int fries_counters(fries_ctx *h, uint64_t *iters, uint64_t *spawns, uint64_t *launches, uint64_t *fks_replays, uint64_t *stage_elems) {
    FriesCtx *c = &h->c;
    if (iters) *iters = c->tot_iters;
    if (spawns) *spawns = c->tot_spawns;
    if (launches) *launches = c->n_kernel_launch;
    if (fks_replays) *fks_replays = c->tot_fks_iters;
    if (stage_elems) *stage_elems = c->tot_stage_elems;
    return 0;
}

// ------------------------------------------------------------------ the generator
extern "C" uint32_t fries_next_draw(fries_ctx *h) { return (uint32_t)h->c.mt(); }
// the generator as std::mt19937's own text form (operator<< / operator>>): a caller that owns a std::mt19937, like the reference's
// drivers, lends it to an operator whose number of draws depends on the data and takes it back afterwards
extern "C" int fries_rng_set_state(fries_ctx *h, const char *text) {
    return fr_api_host(h, [&](FriesCtx *c) {
        std::istringstream is(text ? text : "");
        std::mt19937 m;
        is >> m;
        if (is.fail()) throw FriesError("fries_rng_set_state: not a std::mt19937 state");
        c->mt = m;
    });
}
extern "C" int fries_rng_get_state(fries_ctx *h, char *buf, size_t cap, size_t *need) {
    return fr_api_host(h, [&](FriesCtx *c) {
        std::ostringstream os;
        os << c->mt;
        const std::string s = os.str();
        if (need) *need = s.size() + 1;
        if (buf) {
            if (cap < s.size() + 1) throw FriesError("fries_rng_get_state: buffer too small");
            memcpy(buf, s.c_str(), s.size() + 1);
        }
    });
}
