// frisys_mol and frifull_mol iteration loops (FRIES_bin/frisys_mol.cpp:76-552, FRIES_bin/frifull_mol.cpp) on the device-resident engine,
// the host steps every driver shares (hh.hip and fciqmc.hip hold the other loops) and the per-kernel timing behind FR_LAUNCH.
#include "ctx.hpp"
#include <cmath>

// ------------------------------------------------------------------ per-kernel HIP-event timing
void fr_prof_begin(FriesCtx *c, const char *name) {
    ProfSpan sp; sp.name = name;
    for (int k = 0; k < 2; k++) {
        hipEvent_t e;
        if (!c->prof_pool.empty()) { e = c->prof_pool.back(); c->prof_pool.pop_back(); }
        else if (hipEventCreate(&e) != hipSuccess) throw FriesError("hipEventCreate failed");
        (k ? sp.b : sp.a) = e;
    }
    hipEventRecord(sp.a, c->stream);
    c->prof_spans.push_back(sp);
}
void fr_prof_end(FriesCtx *c) { hipEventRecord(c->prof_spans.back().b, c->stream); }
void fr_prof_collect(FriesCtx *c) {
    if (c->prof_spans.empty()) return;
    FR_HIP(hipStreamSynchronize(c->stream));
    for (auto &sp : c->prof_spans) {
        float ms = 0;
        hipEventElapsedTime(&ms, sp.a, sp.b);
        ProfAgg *a = nullptr;
        for (auto &x : c->prof_agg) if (x.name == sp.name) { a = &x; break; }
        if (!a) { c->prof_agg.push_back(ProfAgg{sp.name, 0.0, 0}); a = &c->prof_agg.back(); }
        a->ms += ms; a->calls++;
        c->prof_pool.push_back(sp.a); c->prof_pool.push_back(sp.b);
    }
    c->prof_spans.clear();
}

// ------------------------------------------------------------------ spawn assembly (frisys_mol.cpp:435-464)
__global__ void __launch_bounds__(FR_BLOCK) k_spawn_build(VecDev V, SpawnBuf S, const uint32_t *c_pos, const uint32_t *c_orbs, const double *c_val,
                                                          const uint32_t *n_succ, double eps, double init_thresh) {
    const uint32_t n = *n_succ;
    uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0) *S.n_spawn = n;
    if (j >= n) return;
    uint32_t pos = c_pos[j], ob = c_orbs[j];
    double cur = V.v0[pos];
    det_t d = V.dets[pos];
    unsigned a = fr_c(ob, 0), b = fr_c(ob, 1), u = fr_c(ob, 2), w = fr_c(ob, 3);
    double add_el = -eps * c_val[j];
    if (cur < 0) add_el *= -1;
    if (!(u == 0 && w == 0)) d = (d & ~(1ull << a) & ~(1ull << b)) | (1ull << u) | (1ull << w);     // doub_det
    else d = (d & ~(1ull << a)) | (1ull << b);                                                        // sing_det
    S.det[j] = d; S.val[j] = add_el; S.ini[j] = fabs(cur) >= init_thresh;
}

void fr_check_dev_err(FriesCtx *c) {
    uint32_t e = 0;
    FR_HIP(hipMemcpyAsync(&e, c->d_err, 4, hipMemcpyDeviceToHost, c->stream));
    FR_HIP(hipStreamSynchronize(c->stream));
    e |= c->h_vst.err;
    if (!e) return;
    std::string m = "device error:";
    if (e & FR_ERR_CAP) m += " vector capacity (max_dets) exceeded;";
    if (e & FR_ERR_SPAWN_CAP) m += " insufficient memory allocated for matrix compression;";
    if (e & FR_ERR_NELEC) m += " determinant created with an incorrect number of electrons;";
    if (e & FR_ERR_HASH_FULL) m += " determinant hash table full;";
    if (e & FR_ERR_ROUNDS) m += " exact-preservation rounds did not converge;";
    if (e & FR_ERR_BACKLOG) m += " too many comb repairs;";
    if (e & FR_ERR_PIV) m += " pivotal compression met an unpreserved element of two sampling units or more;";
    throw FriesError(m);
}

const void *fr_allgather(FriesCtx *c, size_t bytes) {
    if (!c->use_comm) return c->comm.small_send;
    if (bytes > 2048) throw FriesError("all-gather block exceeds FRIES_COMM_SMALL_BYTES");
    if (c->comm.allgather(c->comm.user, bytes, (void *)c->stream)) throw FriesError("fries_comm.allgather failed");
    c->n_collectives++;
    return c->comm.small_recv;
}

// DistVec::idx_to_proc (vec_utils.hpp:360-379): hash_fxn over the occupied orbitals with the proc scrambler, mod n_procs
int fr_host_idx_to_proc(const FriesCtx *c, det_t d) {
    if (c->n_ranks == 1) return 0;
    uint64_t hash = 0;
    uint32_t i = 0;
    if (c->hh_mode) {       // HubHolVec::idx_to_proc (hh_vec.hpp:56-66): occupied orbitals, then every site's phonon number
        const unsigned L = c->hh.n_sites;
        for (det_t a = d & ((1ull << (2 * L)) - 1ull); a; a &= a - 1, i++)
            hash = 1099511628211ULL * hash + (uint32_t)((i + 1u) * c->proc_scr[(unsigned)__builtin_ctzll(a)]);
        for (unsigned s = 0; s < L; s++) hash = 1099511628211ULL * hash + (uint32_t)((s + 1u) * c->proc_scr[(d >> (2 * L + 3 * s)) & 7u]);
        return (int)(hash % (uint64_t)c->n_ranks);
    }
    while (d) {
        unsigned orb = (unsigned)__builtin_ctzll(d);
        d &= d - 1;
        uint32_t term = (i + 1u) * c->proc_scr[orb];
        hash = 1099511628211ULL * hash + term;
        i++;
    }
    return (int)(hash % (uint64_t)c->n_ranks);
}


// DistVec::add x m + perform_add from the host: m (determinant, value, initiator flag) triples into the spawn buffers, merged into the
// vector's own column (same_column) or into column 1 under the initiator rule.  The callers check the capacity and decide what to wait for.
void fr_spawn_upload_merge(FriesCtx *c, const det_t *det, const double *val, const uint8_t *ini, uint32_t m, bool same_column) {
    FR_HIP(hipMemcpyAsync(c->sp.det, det, 8 * (size_t)m, hipMemcpyHostToDevice, c->stream));
    FR_HIP(hipMemcpyAsync(c->sp.val, val, 8 * (size_t)m, hipMemcpyHostToDevice, c->stream));
    FR_HIP(hipMemcpyAsync(c->sp.ini, ini, m, hipMemcpyHostToDevice, c->stream));
    FR_HIP(hipMemcpyAsync(c->sp.n_spawn, &m, 4, hipMemcpyHostToDevice, c->stream));
    fr_vec_merge(c, &c->vec, m, same_column);
}
// the drivers start from 100 x the reference determinant on the rank that owns it
void fr_spawn_reference_det(FriesCtx *c) {
    const double v = 100; const uint8_t ini = 1;
    fr_spawn_upload_merge(c, &c->hf_det, &v, &ini, 1, true);        // perform_add(0) into column 0
}

// What every driver's setup begins with: the generator seeded, the two scramblers -- proc_scr drawn before vec_scr, and nothing drawn for
// one the caller supplied where the driver takes it (--load_dir's hash.dat, a host that drew them itself) --, the one-rank send block, the
// proc scrambler on the device, the Adder's capacity per destination and the owner of the reference determinant (c->hf_det).
void fr_driver_prologue(FriesCtx *c, uint32_t seed, bool take_proc_scr, bool take_vec_scr, uint32_t adder_cap) {
    c->mt.seed(seed);
    c->proc_scr.resize(2 * c->n_orb); c->vec_scr.resize(2 * c->n_orb);
    if (take_proc_scr && c->in_proc_scr.size() == c->proc_scr.size()) c->proc_scr = c->in_proc_scr; else for (auto &x : c->proc_scr) x = c->mt();
    if (take_vec_scr && c->in_vec_scr.size() == c->vec_scr.size()) c->vec_scr = c->in_vec_scr; else for (auto &x : c->vec_scr) x = c->mt();
    c->adder_cap = adder_cap;
    if (!c->comm.small_send) { c->own_small = c->mem.alloc<uint8_t>(2048); c->comm.small_send = c->own_small; }
    if (!c->d_proc_scr) c->d_proc_scr = c->mem.alloc<uint32_t>(64);
    FR_HIP(hipMemcpyAsync(c->d_proc_scr, c->proc_scr.data(), 4 * c->proc_scr.size(), hipMemcpyHostToDevice, c->stream));
    c->hf_proc = fr_host_idx_to_proc(c, c->hf_det);
}
// min(1e6, spawn_length) (frisys_mol.cpp:109-110, frifull_mol.cpp:68-70); FRIES_ADDER_SIZE: a smaller Adder (the DistVec constructor's
// adder_size) -- the early perform_add rounds at test sizes
static uint32_t adder_cap_mol(uint32_t spawn_length) {
    if (getenv("FRIES_ADDER_SIZE")) return (uint32_t)atol(getenv("FRIES_ADDER_SIZE"));
    return spawn_length > 1000000u ? 1000000u : spawn_length;
}

// adjust_shift (compress_utils.cpp:684-693) every tenth iteration, as frisys_mol, frifull_mol, frimulti_mol and frisys_hh call it
void fr_adjust_shift(FriesCtx *c, double glob_norm) {
    const unsigned shift_interval = 10;
    const double shift_damping = 0.05;
    if ((c->iterat + 1) % shift_interval != 0) return;
    double damp = shift_damping / shift_interval / c->eps;
    if (c->last_one_norm) { c->en_shift -= damp * log(glob_norm / c->last_one_norm); c->last_one_norm = glob_norm; }
    if (c->last_one_norm == 0 && glob_norm > c->target_norm) c->last_one_norm = glob_norm;
}
// the error word of an iteration's log: the device's flags and the vector state's
uint32_t fr_log_err(FriesCtx *c) {
    uint32_t e = 0;
    FR_HIP(hipMemcpy(&e, c->d_err, 4, hipMemcpyDeviceToHost));
    return e | c->h_vst.err;
}
// an iteration's log from the context's observables and the host's copy of the vector state; the first n_comp_len stage lengths, zeros behind them
void fr_log_fill(FriesCtx *c, fries_iter_log *lg, int n_comp_len) {
    lg->numer = c->numer; lg->denom = c->denom; lg->shift = c->en_shift; lg->norm = c->glob_norm;
    lg->nkept = c->nkept; lg->n_nonz = c->h_vst.n_nonz; lg->curr_size = c->h_vst.curr_size;
    lg->num_success = c->num_success;
    for (int k = 0; k < 5; k++) lg->comp_len[k] = k < n_comp_len ? c->comp_len[k] : 0;
    lg->err = fr_log_err(c);
}

// The first n positions of the vector become the dense (semi-stochastic) space: H inside it is tabulated (fr_dense_h_setup), every rank learns
// tot_dense_h = sum_mpi(n_determ_h) (frisys_mol.cpp:399: what the matrix sample budget is reduced by) and every rank's n_dense (what
// DistVec::save writes to dense.txt, vec_utils.hpp:736-745).  zero: init_dense zeroes the values (:876-879), DistVec::load keeps them.
void fr_dense_declare(FriesCtx *c, uint32_t n, bool zero) {
    if (n > c->h_vst.curr_size) throw FriesError("dense space larger than the stored vector");
    c->vec.n_dense = n;
    if (n && zero) FR_HIP(hipMemsetAsync(c->vec.v0, 0, 8 * (size_t)n, c->stream));
    fr_dense_h_setup(c, c->mem);
    c->n_dense_h_glob = c->n_dense_h;
    c->dense_sizes.assign((size_t)c->n_ranks, n);
    if (c->use_comm) {
        const uint32_t mine[2] = {c->n_dense_h, n};
        FR_HIP(hipMemcpyAsync(c->comm.small_send, mine, 8, hipMemcpyHostToDevice, c->stream));
        const uint32_t *all = (const uint32_t *)fr_allgather(c, 8);
        std::vector<uint32_t> got(2 * (size_t)c->n_ranks);
        FR_HIP(hipMemcpyAsync(got.data(), all, 8 * (size_t)c->n_ranks, hipMemcpyDeviceToHost, c->stream));
        FR_HIP(hipStreamSynchronize(c->stream));
        uint64_t tot = 0;
        for (int r = 0; r < c->n_ranks; r++) { tot += got[2 * r]; c->dense_sizes[r] = got[2 * r + 1]; }
        if (tot > 0xffffffffull) throw FriesError("dense block of H too large");
        c->n_dense_h_glob = (uint32_t)tot;
    }
    if (c->n_dense_h_glob >= c->mat_nonz) throw FriesError("mat_nonz must exceed the number of matrix elements inside the dense space (the compression gets mat_nonz minus that many samples)");
}

void fr_frisys_setup(FriesCtx *c, const fries_frisys_params *p) {
    if (!c->d_eris) throw FriesError("fries_set_molecule must be called first");
    c->eps = p->epsilon; c->target_norm = p->target_norm; c->init_thresh = p->initiator;
    c->vec_nonz = p->vec_nonz; c->mat_nonz = p->mat_nonz; c->new_hb = p->hb_unnorm != 0;
    c->en_shift = 0; c->last_one_norm = 0; c->iterat = 0; c->comp_pending = false;
    if (p->max_dets == 0 || p->mat_nonz == 0 || p->vec_nonz == 0) throw FriesError("max_dets, mat_nonz and vec_nonz must be positive");
    // scramblers: frisys_mol.cpp:133-135, :142-144; --load_dir: load_proc_hash (:128-130), no draws.  Adder: :109-110
    fr_driver_prologue(c, p->seed, true, false, adder_cap_mol((uint32_t)((uint64_t)p->mat_nonz * 4 / c->n_ranks)));
    // A shard can in principle emit the whole (global) sample budget, so the work arrays are sized for it; the
    // reference sizes them mat_nonz * 4 / n_procs and throws when a shard outgrows that (:109, heat_bathPP.cpp:700-704).
    uint32_t wcap = p->max_dets > p->mat_nonz + 4096 ? p->max_dets : p->mat_nonz + 4096;
    fr_vec_alloc(c, c->mem, &c->vec, p->max_dets);
    fr_hbpp_alloc(c, c->mem, wcap);
    fr_spawn_alloc(c, c->mem, p->mat_nonz + 4096);
    fr_xch_alloc(c, c->mem, p->mat_nonz + 4096);
    fr_vcomp_alloc(c, c->mem, p->max_dets);
    if (c->ham_shift_set) c->hf_en = c->ham_shift_hf_en;        // --ham_shift (:95-98)
    fr_h_trial_setup(c);        // replicated: every rank enumerates H * trial (the reference gathers the shards, vec_utils.hpp:920-952)
    if (!c->in_det_space.empty()) {
        // --det_space (frisys_mol.cpp:236-239): DistVec::init_dense adds every determinant of the file with value 1 (they take positions
        // 0 .. n - 1 of the empty vector), then zeroes the values; the entries stay
        // With ranks: rank 0 adds the whole file and the adds travel to their owners (vec_utils.hpp:866-872), i.e. every rank receives the
        // determinants it owns in file order; each rank then has a dense space of its own length.
        std::vector<det_t> mine;
        for (det_t d : c->in_det_space) if (fr_host_idx_to_proc(c, d) == c->rank) mine.push_back(d);
        const uint32_t m = (uint32_t)mine.size();
        if (m > c->sp.cap || m > p->max_dets) throw FriesError("dense space larger than the vector / spawn buffer");
        if (m) {
            std::vector<double> v(m, 1.0); std::vector<uint8_t> f(m, 1);
            fr_spawn_upload_merge(c, mine.data(), v.data(), f.data(), m, true);
        }
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        fr_dense_declare(c, c->h_vst.curr_size, true);          // (a determinant listed twice takes one position)
    }
    if (!c->in_ini_det.empty()) {
        // --ini_vec (:264-274): rank 0 add()s every entry in file order; each rank receives the ones it owns in that order
        std::vector<det_t> d; std::vector<double> v;
        for (size_t i = 0; i < c->in_ini_det.size(); i++)
            if (c->in_ini_val[i] != 0 && fr_host_idx_to_proc(c, c->in_ini_det[i]) == c->rank) { d.push_back(c->in_ini_det[i]); v.push_back(c->in_ini_val[i]); }
        uint32_t m = (uint32_t)d.size();
        if (m > c->sp.cap) throw FriesError("initial vector larger than the spawn buffer");
        if (m) {
            std::vector<uint8_t> f(m, 1);
            fr_spawn_upload_merge(c, d.data(), v.data(), f.data(), m, true);
            FR_HIP(hipStreamSynchronize(c->stream));
        }
    }
    // start from 100 * |HF> on the rank that owns it (:277-281)
    else if (c->rank == c->hf_proc) fr_spawn_reference_det(c);
    fr_vec_sync_state(c, &c->vec, &c->h_vst);
    fr_check_dev_err(c);
}

static inline double uni(std::mt19937 &mt) { return mt() / (1. + UINT32_MAX); }

// the non-zero products of the dense block of H with column 0, in the stored order (one workgroup: ordered compaction)
static __global__ void __launch_bounds__(FR_BLOCK) k_dense_spawn(VecDev V, SpawnBuf P, const uint32_t *from, const det_t *to, const double *el, uint32_t n) {
    __shared__ uint32_t shu[4];
    uint32_t written = 0;
    for (uint32_t base = 0; base < n; base += FR_BLOCK) {
        const uint32_t k = base + threadIdx.x;
        double mv = 0;
        if (k < n) mv = V.v0[from[k]] * el[k];
        const uint32_t f = mv != 0 ? 1u : 0u;       // DistVec::add drops zero values (vec_utils.hpp:418-423)
        uint32_t tot;
        const uint32_t incl = fr_block_scan_u32(f, shu, &tot);
        if (f) { const uint32_t o = written + incl - 1; P.det[o] = to[k]; P.val[o] = mv; P.ini[o] = 1; }
        written += tot;
    }
    if (threadIdx.x == 0) *P.n_spawn = written;
}
// DistVec::dense_norm (vec_utils.hpp:903-918): the magnitudes of the dense space added up in position order
static __global__ void k_dense_norm(VecDev V, double *out) {
    double r = 0;
    for (uint32_t i = 0; i < V.n_dense; i++) { const double e = V.v0[i]; r += e >= 0 ? e : -e; }
    *out = r;
}

// The three pieces of the iteration that fries_frisys_iterate and the stepwise entry points (fries_spawn_from_comp, fries_dense_apply,
// fries_dense_norm) share: each enqueues one fixed sequence, whoever calls it.
// Spawning + annihilation (:429-471) from the compression result in c_pos / c_orbs / c_val / d_nsucc; -> an upper bound of the positions taken.
uint32_t fr_spawn_comp_result(FriesCtx *c, double eps, double init_thresh) {
    if (c->num_success > c->sp.cap) throw FriesError("spawn buffer too small");
    if (c->num_success) FR_LAUNCH(c, "k_spawn_build", k_spawn_build, dim3(fr_blocks(c->num_success, FR_BLOCK)), dim3(FR_BLOCK), c->vec, c->sp, c->c_pos, c->c_orbs, c->c_val, c->d_nsucc, eps, init_thresh);
    uint32_t n_merge = c->num_success;
    bool merged = false;            // the Adder filled up: the passes went through several perform_add rounds, each merged on arrival
    if (c->use_comm) n_merge = fr_spawn_exchange(c, c->num_success, 0, &merged);      // every rank takes part, also with nothing to send
    if (n_merge && !merged) fr_vec_merge(c, &c->vec, n_merge, false);
    return n_merge;
}
// The dense block of H applied exactly (:480-485): value at the origin x stored element, added as initiator contributions in the stored
// order, as a perform_add of its own (with ranks: an exchange of its own, every rank taking part); -> an upper bound of the positions taken.
uint32_t fr_dense_multiply(FriesCtx *c) {
    if (!c->n_dense_h_glob) return 0;
    uint32_t m = 0;
    if (c->n_dense_h_nz) {
        FR_LAUNCH(c, "k_dense_spawn", k_dense_spawn, dim3(1), dim3(FR_BLOCK), c->vec, c->sp, c->d_dh_from, c->d_dh_to, c->d_dh_el, c->n_dense_h_nz);
        FR_HIP(hipMemcpyAsync(&m, c->sp.n_spawn, 4, hipMemcpyDeviceToHost, c->stream));
        FR_HIP(hipStreamSynchronize(c->stream));
    }
    const uint32_t n_merge_dense = c->use_comm ? fr_spawn_exchange(c, m) : m;      // all of them carry the initiator flag: one pass in effect
    if (n_merge_dense) fr_vec_merge(c, &c->vec, n_merge_dense, false);
    return n_merge_dense;
}
// sol_vec.dense_norm() (:503, vec_utils.hpp:903-918: sum_mpi of the ranks' sums); 0 without a dense space
double fr_dense_norm_all(FriesCtx *c) {
    if (!(c->n_dense_h_glob || c->vec.n_dense)) return 0;
    hipStream_t st = c->stream;
    FR_LAUNCH(c, "k_dense_norm", k_dense_norm, dim3(1), dim3(1), c->vec, c->d_dense_norm);
    const double *src = c->d_dense_norm;
    if (c->use_comm) {
        FR_HIP(hipMemcpyAsync(c->comm.small_send, c->d_dense_norm, 8, hipMemcpyDeviceToDevice, st));
        src = (const double *)fr_allgather(c, 8);
    }
    double h[FR_MAX_RANKS];
    FR_HIP(hipMemcpyAsync(h, src, 8 * (size_t)c->n_ranks, hipMemcpyDeviceToHost, st));
    FR_HIP(hipStreamSynchronize(st));
    double dn = 0;
    for (int p = 0; p < c->n_ranks; p++) dn += h[p];
    return dn;
}

void fr_frisys_iterate(FriesCtx *c, fries_iter_log *lg) {
    fr_vec_sync_state(c, &c->vec, &c->h_vst);
    fr_vec_maybe_rebuild(c, &c->vec);
    // systematic matrix compression (:414-422)
    double rn[5];
    for (int k = 0; k < 5; k++) rn[k] = uni(c->mt);
    fr_hbpp_apply(c, c->mat_nonz - c->n_dense_h_glob, rn);      // :421 matr_samp - tot_dense_h
    uint32_t vec_size = c->h_vst.curr_size;
    // spawning + annihilation (:429-471), then the dense block (:480-485)
    const uint32_t n_merge = fr_spawn_comp_result(c, c->eps, c->init_thresh);
    const uint32_t n_merge_dense = fr_dense_multiply(c);
    // no host look at the vector's state here: the kernels read the stored size themselves, the launches only need an upper bound of it
    // (every merged spawn may have taken a new position); an overflow raised by the merge is reported at the end of the iteration
    {
        const uint64_t ub = (uint64_t)c->h_vst.curr_size + n_merge + n_merge_dense;
        c->h_vst.curr_size = ub < c->vec.cap ? (uint32_t)ub : c->vec.cap;
    }
    // death / cloning, column add (:487-499)
    fr_death_clone(c, vec_size);
    // the projected-energy dot products are taken here -- find_preserve does not touch the values -- so that their readback rides on
    // the synchronisation find_preserve needs anyway (the reference forms them after it, frisys_mol.cpp:511-517)
    const void *h_dots = fr_dots_enqueue(c);
    // vector compression (:501-539)
    uint32_t n_samp = c->vec_nonz;
    double glob_norm = 0;
    fr_find_preserve(c, &n_samp, &glob_norm);
    fr_dots_collect(c, h_dots, &c->numer, &c->denom);
    if (c->n_dense_h_glob || c->vec.n_dense) glob_norm += fr_dense_norm_all(c);       // glob_norm += sol_vec.dense_norm() (:503)
    c->glob_norm = glob_norm;
    c->nkept = c->vec_nonz - n_samp;
    fr_adjust_shift(c, glob_norm);
    double rn_sys = uni(c->mt);
    fr_sys_comp(c, n_samp, rn_sys);
    c->iterat++;
    c->tot_iters++; c->tot_spawns += c->num_success;
    for (int k = 0; k < 5; k++) c->tot_stage_elems += c->comp_len[k];
    for (int k = 1; k <= 5; k++) c->tot_fks_iters += c->fks_iters[k];
    if (c->prof_on) fr_prof_collect(c);
    if (lg) {
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        fr_log_fill(c, lg, 5);
    }
}

// ------------------------------------------------------------------ frifull_mol (FRIES_bin/frifull_mol.cpp)
void fr_frifull_setup(FriesCtx *c, const fries_frifull_params *p) {
    if (!c->d_eris) throw FriesError("fries_set_molecule must be called first");
    if (p->max_dets == 0 || p->vec_nonz == 0) throw FriesError("max_dets and vec_nonz must be positive");
    c->eps = p->epsilon; c->target_norm = p->target_norm; c->init_thresh = 0;
    c->vec_nonz = p->vec_nonz; c->mat_nonz = 0; c->full_mode = true;
    c->en_shift = 0; c->last_one_norm = 0; c->iterat = 0;
    uint32_t scap = p->spawn_cap ? p->spawn_cap : 8000000u;
    if (scap > 8000000u) scap = 8000000u;           // one merge handles FR_MAX_PART tiles of spawns
    {   // frifull_mol.cpp:68-70: the Adder holds min(1e6, target_nonz / n_procs * num_ex / n_procs / 4) elements per destination (32-bit arithmetic there)
        const uint32_t nv = c->n_orb - c->n_elec / 2;
        const uint32_t num_ex = c->n_elec * c->n_elec * nv * nv;
        const uint32_t spawn_len = p->vec_nonz / (uint32_t)c->n_ranks * num_ex / (uint32_t)c->n_ranks / 4u;
        fr_driver_prologue(c, p->seed, false, false, adder_cap_mol(spawn_len));     // both scramblers always drawn (frifull_mol.cpp:96-98, :104-107)
    }
    fr_vec_alloc(c, c->mem, &c->vec, p->max_dets);
    fr_spawn_alloc(c, c->mem, scap);
    fr_xch_alloc(c, c->mem, scap);
    fr_vcomp_alloc(c, c->mem, p->max_dets);
    c->W.kin = c->mem.alloc<uint32_t>(p->max_dets);     // sys_comp's tooth-index scratch (the HB-PP arrays are not allocated here)
    if (!c->d_norms_keep) { c->d_norms_keep = c->mem.alloc<double>(FR_MAX_RANKS); c->d_seq_scratch = c->mem.alloc<double>(1); }        // sys_comp over ranks: the other ranks' norms, the second in-order sum
    // trial vector = HF (:121-147); there is no H * trial in this driver
    c->n_trial = 1; c->n_htrial = 0;
    c->tr_det = c->mem.alloc<det_t>(1); c->tr_val = c->mem.alloc<double>(1);
    c->htr_det = c->mem.alloc<det_t>(1); c->htr_val = c->mem.alloc<double>(1);
    double one = 1.0;
    FR_HIP(hipMemcpyAsync(c->tr_det, &c->hf_det, 8, hipMemcpyHostToDevice, c->stream));
    FR_HIP(hipMemcpyAsync(c->tr_val, &one, 8, hipMemcpyHostToDevice, c->stream));
    if (c->rank == (int)c->hf_proc) fr_spawn_reference_det(c);      // start from 100 * |HF> on the rank that owns it (:186-190)
    fr_vec_sync_state(c, &c->vec, &c->h_vst);
    fr_check_dev_err(c);
}

// one iteration of frifull_mol.cpp:258-304.  The reference alternates between its two value columns; here the current
// vector is always "column 0" and the two device arrays trade places at the end of the iteration.
void fr_frifull_iterate(FriesCtx *c, fries_iter_log *lg) {
    fr_vec_sync_state(c, &c->vec, &c->h_vst);
    fr_vec_maybe_rebuild(c, &c->vec);
    double unused = 0, denom = 0, numer = 0;
    fr_dots(c, &unused, &denom);                      // :259-260
    fr_abs_sums(c);
    uint32_t n_samp = c->vec_nonz;
    double glob_norm = 0;
    fr_find_preserve(c, &n_samp, &glob_norm);         // :263-264
    c->glob_norm = glob_norm;
    c->nkept = c->vec_nonz - n_samp;
    fr_adjust_shift(c, glob_norm);                    // :272-278
    double rn_sys = uni(c->mt);
    fr_sys_comp(c, n_samp, rn_sys);                   // :283-289 (an element leaves the table only when it is zero in both columns)
    fr_vec_sync_state(c, &c->vec, &c->h_vst);
    fr_h_diag_vec(c, 1 + c->eps * c->en_shift, -c->eps);            // :291
    uint64_t n_add = fr_h_offdiag_vec(c, -c->eps);                  // :293
    std::swap(c->vec.v0, c->vec.v1);                                // :294
    fr_vec_sync_state(c, &c->vec, &c->h_vst);
    if (c->h_vst.err) fr_check_dev_err(c);
    fr_dots(c, &unused, &numer);
    numer = ((1 + c->eps * c->en_shift) * denom - numer) / c->eps;  // :296-298
    c->numer = numer; c->denom = denom;
    c->num_success = (uint32_t)(n_add > 0xffffffffull ? 0xffffffffull : n_add);
    c->iterat++; c->tot_iters++; c->tot_spawns += n_add;
    if (c->prof_on) fr_prof_collect(c);
    if (lg) fr_log_fill(c, lg, 0);
}
