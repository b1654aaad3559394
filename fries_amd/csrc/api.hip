// The extern "C" boundary (include/fries_hip.h): context lifetime, the drivers' inputs, set-up and iterate entry points, the stepwise
// operators and the estimators between two contexts.  The vector's entry points are in api_vec.hip, test hooks and statistics in api_test.hip.
#include "api.hpp"
#include "rdm2_plan.hpp"

static thread_local std::string g_err;
void fr_set_error(const std::string &m) { g_err = m; }
extern "C" const char *fries_last_error(void) { return g_err.c_str(); }

// ------------------------------------------------------------------ context lifetime
extern "C" int fries_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int fries_ctx_create(fries_ctx **out, int device) {
    return fr_api([&] {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n == 0) throw FriesError("no HIP device available: the FRI engine has no CPU fallback");
        if (device < 0 || device >= n) throw FriesError("device index out of range");
        FR_HIP(hipSetDevice(device));
        fries_ctx *h = new fries_ctx();
        h->c.device = device;
        if (getenv("FRIES_DBG")) h->c.dbg = atoi(getenv("FRIES_DBG"));
        if (getenv("FRIES_FKS_REC_AT")) h->c.fks_rec_at = atoi(getenv("FRIES_FKS_REC_AT"));
        if (getenv("FRIES_GROUP_WARM_ALL")) h->c.fks_group_warm_all = atoi(getenv("FRIES_GROUP_WARM_ALL")) != 0;
        if (getenv("FRIES_NO_GROUP_WARM")) h->c.fks_no_group_warm = true;
        if (getenv("FRIES_FKS_NO_EXT")) h->c.fks_no_ext = true;
        if (getenv("FRIES_FKS_LIGHT_FULL_GRID")) h->c.fks_light_full_grid = atoi(getenv("FRIES_FKS_LIGHT_FULL_GRID")) != 0;
        if (getenv("FRIES_FKS_FUSE_TOTALS")) h->c.fks_fuse_totals = atoi(getenv("FRIES_FKS_FUSE_TOTALS")) != 0;
        if (getenv("FRIES_FKS_NO_LIGHT")) h->c.fks_no_light = atoi(getenv("FRIES_FKS_NO_LIGHT")) != 0;
        if (getenv("FRIES_FKS_NO_SPECULATION")) h->c.fks_no_speculation = atoi(getenv("FRIES_FKS_NO_SPECULATION")) != 0;
        if (getenv("FRIES_FKS_NO_CLOSING")) h->c.fks_no_closing = atoi(getenv("FRIES_FKS_NO_CLOSING")) != 0;
        if (getenv("FRIES_FKS_COLLAPSE_WALK")) h->c.fks_no_collapse_walk = atoi(getenv("FRIES_FKS_COLLAPSE_WALK")) == 0;
        if (getenv("FRIES_FKS_SEQ")) h->c.fks_force_seq = atoi(getenv("FRIES_FKS_SEQ")) != 0;
        if (getenv("FRIES_FKS_NO_MERGED_NORM")) h->c.fks_no_merged_norm = atoi(getenv("FRIES_FKS_NO_MERGED_NORM")) != 0;
        if (getenv("FRIES_NO_WARM")) h->c.warm_start = false;
        if (getenv("FRIES_RDM2_RECORDS")) h->c.rdm2_records = std::min<uint64_t>(strtoull(getenv("FRIES_RDM2_RECORDS"), nullptr, 10), R2_MAX_RECORDS);
        {
            hipDeviceProp_t pr;
            FR_HIP(hipGetDeviceProperties(&pr, device));
            h->c.fks_grid = (unsigned)FR_FKS_WPE1 * (unsigned)pr.multiProcessorCount;      // k_fks_sweep: <= 92 VGPRs -> 5 waves/SIMD = 5 workgroups per CU
            h->c.fks_grid0 = ((unsigned)FR_FKS_WPE0 + 1u) * (unsigned)pr.multiProcessorCount;     // the lean replay: one workgroup per CU more than fit at once (measured: 60.8 against 62.6 us)
            if (getenv("FRIES_FKS_GRID0")) h->c.fks_grid0 = (unsigned)atoi(getenv("FRIES_FKS_GRID0"));
            if (getenv("FRIES_FKS_GRID")) h->c.fks_grid = (unsigned)atoi(getenv("FRIES_FKS_GRID"));
        }
        FR_HIP(hipStreamCreate(&h->c.stream));
        h->c.d_err = h->c.mem.alloc<uint32_t>(1);
        FR_HIP(hipMemset(h->c.d_err, 0, 4));
        *out = h;
    });
}

extern "C" void fries_ctx_destroy(fries_ctx *h) {
    if (!h) return;
    FriesCtx &c = h->c;
    hipSetDevice(c.device);
    hipDeviceSynchronize();
    if (c.dbg >= 1 && c.n_fks_sequential) {
        FksSqCtl hc{};
        hipMemcpy(&hc, c.fsq.ctl, sizeof(hc), hipMemcpyDeviceToHost);
        fprintf(stderr, "[fries] find_keep_sub in the reference's order: %llu stages; %llu guess rounds, %llu exact rounds over %llu tiles (touched tiles taken as one integer step: %llu, element by element: %llu), %llu walks over %llu tiles\n",
                (unsigned long long)c.n_fks_sequential, (unsigned long long)c.n_fsq_guess, (unsigned long long)c.n_fsq_exact, (unsigned long long)c.n_fsq_chain_tiles,
                hc.n_fast, hc.n_dense, (unsigned long long)c.n_fsq_walk, (unsigned long long)c.n_fsq_walk_tiles);
    }
    for (hipEvent_t e : c.prof_pool) hipEventDestroy(e);
    for (ProfSpan &sp : c.prof_spans) { hipEventDestroy(sp.a); hipEventDestroy(sp.b); }
    if (c.stream) hipStreamDestroy(c.stream);
    delete h;       // c.mem frees every device and pinned array the context allocated
}
extern "C" void *fries_stream(fries_ctx *h) { return (void *)h->c.stream; }
extern "C" uint64_t fries_kernel_launches(fries_ctx *h) { return h->c.n_kernel_launch; }

// ------------------------------------------------------------------ the system and the drivers' optional inputs; the inputs must precede the driver's setup
extern "C" int fries_set_molecule(fries_ctx *h, uint32_t n_orb, uint32_t n_elec, const uint8_t *irreps, const double *h_core, const double *eris) {
    return fr_api_dev(h, [&](FriesCtx *c) { fr_system_upload(c, n_orb, n_elec, irreps, h_core, eris); });
}
extern "C" int fries_set_trial_vector(fries_ctx *h, const uint64_t *dets, const double *vals, size_t n) {
    return fr_api_host(h, [&](FriesCtx *c) {
        if (c->vec.dets) throw FriesError("fries_set_trial_vector must be called before the driver's setup");
        c->in_trial_det.assign(dets, dets + n); c->in_trial_val.assign(vals, vals + n);
    });
}
extern "C" int fries_set_initial_vector(fries_ctx *h, const uint64_t *dets, const double *vals, size_t n) {
    return fr_api_host(h, [&](FriesCtx *c) {
        if (c->vec.dets) throw FriesError("fries_set_initial_vector must be called before the driver's setup");
        c->in_ini_det.assign(dets, dets + n); c->in_ini_val.assign(vals, vals + n);
    });
}
extern "C" int fries_set_det_space(fries_ctx *h, const uint64_t *dets, size_t n) {
    return fr_api_host(h, [&](FriesCtx *c) {
        if (c->vec.dets) throw FriesError("fries_set_det_space must come before fries_frisys_setup");
        c->in_det_space.assign(dets, dets + n);
    });
}
extern "C" int fries_set_ham_shift(fries_ctx *h, double hf_en) {
    return fr_api_host(h, [&](FriesCtx *c) {
        if (c->vec.dets) throw FriesError("fries_set_ham_shift must be called before fries_frisys_setup");
        c->ham_shift_set = true; c->ham_shift_hf_en = hf_en;
    });
}
extern "C" int fries_set_proc_scrambler(fries_ctx *h, const uint32_t *proc_scr, size_t n) {
    return fr_api_host(h, [&](FriesCtx *c) {
        if (c->vec.dets) throw FriesError("fries_set_proc_scrambler must be called before fries_frisys_setup");
        c->in_proc_scr.assign(proc_scr, proc_scr + n);
    });
}
extern "C" int fries_set_vec_scrambler(fries_ctx *h, const uint32_t *vec_scr, size_t n) {
    return fr_api_host(h, [&](FriesCtx *c) {
        if (c->vec.dets) throw FriesError("fries_set_vec_scrambler must be called before the driver's setup");
        c->in_vec_scr.assign(vec_scr, vec_scr + n);
    });
}
// Time-reversal symmetry (the subspace drivers' spin_parity argument of h_op_offdiag / apply_HBPP_piv, molecule.cpp:298-369, heat_bathPP.cpp:1326-1407)
extern "C" int fries_set_spin_parity(fries_ctx *h, int spin_parity) {
    return fr_api_host(h, [&](FriesCtx *c) {
        if (spin_parity < -1 || spin_parity > 1) throw FriesError("spin_parity must be -1, 0 or 1");
        c->spin_parity = spin_parity;
    });
}
extern "C" int fries_set_comm(fries_ctx *h, const fries_comm *cm) {
    return fr_api_host(h, [&](FriesCtx *c) {
        if (c->vec.dets) throw FriesError("fries_set_comm must be called before fries_frisys_setup");
        if (!cm || cm->size < 1 || cm->size > FR_MAX_RANKS || cm->rank < 0 || cm->rank >= cm->size) throw FriesError("bad rank / size");
        const bool have = cm->allgather && cm->alltoallv && cm->small_send && cm->small_recv && cm->big_send && cm->big_recv;
        if (cm->size > 1 && (!cm->allgather || !cm->alltoallv || !cm->small_send || !cm->small_recv || !cm->big_send || !cm->big_recv))
            throw FriesError("fries_comm needs both collectives and all four staging buffers");
        c->comm.user = cm->user; c->comm.rank = cm->rank; c->comm.size = cm->size;
        c->comm.small_send = cm->small_send; c->comm.small_recv = cm->small_recv; c->comm.big_send = cm->big_send; c->comm.big_recv = cm->big_recv;
        c->comm.big_bytes = cm->big_bytes; c->comm.allgather = cm->allgather; c->comm.alltoallv = cm->alltoallv;
        c->rank = cm->rank; c->n_ranks = cm->size;
        c->use_comm = cm->size > 1 || have;      // a one-rank communicator still routes everything through the callbacks
    });
}
extern "C" int fries_idx_to_proc(fries_ctx *h, const uint64_t *dets, size_t n, int32_t *proc) {
    return fr_api_host(h, [&](FriesCtx *c) {
        if (c->proc_scr.empty()) throw FriesError("fries_frisys_setup must be called first");
        for (size_t i = 0; i < n; i++) proc[i] = fr_host_idx_to_proc(c, dets[i]);
    });
}
extern "C" int fries_get_scramblers(fries_ctx *h, uint32_t *proc_scr, uint32_t *vec_scr, size_t n) {
    return fr_api_host(h, [&](FriesCtx *c) {
        if (c->proc_scr.empty()) throw FriesError("no run has been set up");
        if (n < c->proc_scr.size()) throw FriesError("scrambler buffer too small");
        if (proc_scr) memcpy(proc_scr, c->proc_scr.data(), 4 * c->proc_scr.size());
        if (vec_scr) memcpy(vec_scr, c->vec_scr.data(), 4 * c->vec_scr.size());
    });
}

static double *hb_field(HbTables &T, int which, size_t *len) {
    size_t n = T.n_orb;
    switch (which) {
        case 0: *len = n; return T.s_tens;
        case 1: *len = n * (n - 1) / 2; return T.d_same;
        case 2: *len = n * n; return T.d_diff;
        case 3: *len = n * (n - 1) / 2; return T.exch_sqrt;
        case 4: *len = n; return T.diag_sqrt;
        case 5: *len = n; return T.exch_norms;
        case 6: *len = 1; return &T.s_norm;
    }
    throw FriesError("unknown tensor id");
}
extern "C" int fries_get_hb_tensor(fries_ctx *h, int which, double *out, size_t cap, size_t *len) {
    return fr_api_host(h, [&](FriesCtx *c) {
        size_t n;
        double *src = hb_field(c->h_hb, which, &n);
        if (len) *len = n;
        if (cap < n) throw FriesError("output buffer too small");
        memcpy(out, src, 8 * n);
    });
}
extern "C" int fries_set_hb_tensor(fries_ctx *h, int which, const double *in, size_t len) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        size_t n;
        double *dst = hb_field(c->h_hb, which, &n);
        if (len != n) throw FriesError("tensor length mismatch");
        memcpy(dst, in, 8 * n);
        FR_HIP(hipMemcpy(c->d_hb, &c->h_hb, sizeof(HbTables), hipMemcpyHostToDevice));
    });
}
extern "C" double fries_hf_energy(fries_ctx *h) { return h->c.hf_en; }
extern "C" double fries_p_doub(fries_ctx *h) { return h->c.p_doub; }

// ------------------------------------------------------------------ the drivers: set-up and iterate
extern "C" int fries_frisys_setup(fries_ctx *h, const fries_frisys_params *p) {
    return fr_api_dev(h, [&](FriesCtx *c) { fr_frisys_setup(c, p); });
}
extern "C" int fries_frisys_iterate(fries_ctx *h, uint32_t n_iter, fries_iter_log *logs) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        if (c->hh_mode) throw FriesError("this context runs frisys_hh: use fries_hh_iterate");
        if (c->fq_mode) throw FriesError("this context runs fciqmc_mol: use fries_fciqmc_iterate");
        for (uint32_t i = 0; i < n_iter; i++) fr_frisys_iterate(c, logs ? &logs[i] : nullptr);
        if (n_iter && !logs) fr_vec_sync_state(c, &c->vec, &c->h_vst);       // the last iteration's merges may have raised a flag in the vector state: one readback per batch
        fr_check_dev_err(c);
    });
}
// restart support: re-seed the driver's mt19937 without redrawing the scramblers, set the shift
// (what --load_dir restores from S.txt, frisys_mol.cpp:257-263) and the iteration counter
extern "C" int fries_frisys_restart(fries_ctx *h, uint32_t seed, double en_shift, double last_one_norm, uint32_t iterat) {
    return fr_api_host(h, [&](FriesCtx *c) {
        c->mt.seed(seed);
        c->en_shift = en_shift; c->last_one_norm = last_one_norm; c->iterat = iterat;
    });
}

extern "C" int fries_frifull_setup(fries_ctx *h, const fries_frifull_params *p) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        if (c->vec.dets) throw FriesError("this context already holds a driver; create a new one");
        fr_frifull_setup(c, p);
    });
}
extern "C" int fries_frifull_iterate(fries_ctx *h, uint32_t n_iter, fries_iter_log *logs) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        if (!c->full_mode) throw FriesError("fries_frifull_setup must be called first");
        for (uint32_t k = 0; k < n_iter; k++) {
            fr_frifull_iterate(c, logs ? &logs[k] : nullptr);
            fr_check_dev_err(c);
        }
    });
}

extern "C" int fries_fciqmc_setup(fries_ctx *h, const fries_fciqmc_params *p) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        if (c->vec.dets) throw FriesError("this context already holds a run");
        fr_fq_setup(c, p);
        fr_check_dev_err(c);
    });
}
extern "C" int fries_fciqmc_iterate(fries_ctx *h, uint32_t n_iter, fries_fciqmc_log *logs) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        if (!c->fq_mode || c->fqw.multi == 1) throw FriesError("fries_fciqmc_setup must be called first");
        for (uint32_t i = 0; i < n_iter; i++) fr_fq_iterate(c, logs ? &logs[i] : nullptr);
        fr_check_dev_err(c);
    });
}

extern "C" int fries_frimulti_setup(fries_ctx *h, const fries_frimulti_params *p) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        if (c->vec.dets) throw FriesError("this context already holds a run");
        fr_multi_setup(c, p);
        fr_check_dev_err(c);
    });
}
extern "C" int fries_frimulti_iterate(fries_ctx *h, uint32_t n_iter, fries_fciqmc_log *logs) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        if (!c->fq_mode || c->fqw.multi != 1) throw FriesError("fries_frimulti_setup must be called first");
        for (uint32_t i = 0; i < n_iter; i++) fr_multi_iterate(c, logs ? &logs[i] : nullptr);
        fr_check_dev_err(c);
    });
}

extern "C" int fries_hh_setup(fries_ctx *h, const fries_hh_params *p) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        if (c->vec.dets) throw FriesError("this context already holds a run");
        fr_hh_setup(c, p);
        fr_check_dev_err(c);
    });
}
extern "C" int fries_hh_iterate(fries_ctx *h, uint32_t n_iter, fries_iter_log *logs) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        if (!c->hh_mode) throw FriesError("fries_hh_setup must be called first");
        for (uint32_t i = 0; i < n_iter; i++) fr_hh_iterate(c, logs ? &logs[i] : nullptr);
        fr_check_dev_err(c);
    });
}
extern "C" int fries_hh_comp_sub(fries_ctx *h, int stage, uint32_t n_samp, double rn, uint32_t *idx0, uint32_t *idx1, double *vals, size_t cap, size_t *n_out) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        if (!c->hh_mode) throw FriesError("fries_hh_setup must be called first");
        if (stage != 1 && stage != 2) throw FriesError("stage must be 1 or 2");
        if (stage == 1) { fr_vec_sync_state(c, &c->vec, &c->h_vst); fr_vec_maybe_rebuild(c, &c->vec); }
        fr_hh_stage(c, stage, n_samp, rn);
        const size_t m = c->comp_len[stage - 1];
        if (m > cap || m > c->W.cap) throw FriesError("Error: insufficient memory allocated for matrix compression.");
        if (m) {
            FR_HIP(hipMemcpyAsync(idx0, c->W.e_wi, 4 * m, hipMemcpyDeviceToHost, c->stream));
            FR_HIP(hipMemcpyAsync(idx1, c->W.e_sub, 4 * m, hipMemcpyDeviceToHost, c->stream));
            FR_HIP(hipMemcpyAsync(vals, c->W.e_val, 8 * m, hipMemcpyDeviceToHost, c->stream));
            FR_HIP(hipStreamSynchronize(c->stream));
        }
        *n_out = m;
        fr_check_dev_err(c);
    });
}
extern "C" int fries_hh_ref_ovlp(fries_ctx *h, double *ovlp) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        if (!c->hh_mode) throw FriesError("fries_hh_setup must be called first");
        double o3[3];
        fr_hh_ref_ovlp(c, o3);
        *ovlp = o3[0];
    });
}

// ------------------------------------------------------------------ the stepwise operators
// frisys_mol.cpp:487-499: v0[i] *= 1 - eps (H_ii - shift) for the first vec_size positions, add_vecs(0, 1), zero_vec on column 1
extern "C" int fries_death_clone(fries_ctx *h, double eps, double shift, uint32_t vec_size) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        const double se = c->eps, ss = c->en_shift;
        c->eps = eps; c->en_shift = shift;
        fr_death_clone(c, vec_size);
        c->eps = se; c->en_shift = ss;
        fr_check_dev_err(c);
    });
}

// DistVec::dot with H * trial and with the trial vector (frisys_mol.cpp:511-517, vec_utils.hpp:228-238)
extern "C" int fries_dots(fries_ctx *h, double *numer, double *denom) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        double nu = 0, de = 0;
        fr_dots(c, &nu, &de);
        if (numer) *numer = nu;
        if (denom) *denom = de;
    });
}

// find_preserve on column 0 (compress_utils.cpp:29-105): *n_samp in = budget, out = samples left; the preserved set stays on
// the device for fries_sys_comp.  Returns through glob_norm the one-norm before compression.
extern "C" int fries_find_preserve(fries_ctx *h, uint32_t *n_samp, double *glob_norm) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        const uint32_t save = c->vec_nonz;
        c->vec_nonz = *n_samp;
        fr_abs_sums(c);
        c->vec_nonz = save;
        double gn = 0;
        fr_find_preserve(c, n_samp, &gn);
        if (glob_norm) *glob_norm = gn;
        fr_check_dev_err(c);
    });
}
// sys_comp (compress_utils.cpp:283-327) after fries_find_preserve, followed by the driver's deletes (frisys_mol.cpp:534-539)
extern "C" int fries_sys_comp(fries_ctx *h, uint32_t n_samp, double rn) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        if (c->hh_mode) c->hh_keep0 = c->rank == 0;      // frisys_hh.cpp:356: position 0 of rank 0 (the Neel state) is never released
        fr_sys_comp(c, n_samp, rn);
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        fr_check_dev_err(c);
    });
}
extern "C" int fries_compress_vec(fries_ctx *h, uint32_t n_samp_in, double rn, uint32_t *n_kept, double *glob_norm) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        uint32_t save = c->vec_nonz;
        c->vec_nonz = n_samp_in;
        fr_death_clone(c, 0);                    // publishes the |v| block sums; v1 is zero so values are unchanged
        uint32_t n_samp = n_samp_in;
        double gn = 0;
        fr_find_preserve(c, &n_samp, &gn);
        fr_sys_comp(c, n_samp, rn);
        c->vec_nonz = save;
        if (n_kept) *n_kept = n_samp_in - n_samp;
        if (glob_norm) *glob_norm = gn;
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        fr_check_dev_err(c);
    });
}
extern "C" int fries_compress_vec_piv(fries_ctx *h, uint32_t n_samp_in, uint32_t *n_kept, double *glob_norm) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        fr_piv_comp(c, n_samp_in, n_kept, glob_norm);
        fr_check_dev_err(c);
    });
}

// the compression result (c_pos / c_orbs / c_val, num_success entries) to the host arrays that were asked for
static void comp_copy_out(FriesCtx *c, uint32_t *det_pos, uint8_t *orbs, double *vals, size_t cap, bool sync_first = false) {
    const size_t m = c->num_success;
    if (cap < m) throw FriesError("output buffer too small");
    if (sync_first) FR_HIP(hipStreamSynchronize(c->stream));
    if (det_pos) FR_HIP(hipMemcpy(det_pos, c->c_pos, 4 * m, hipMemcpyDeviceToHost));
    if (orbs) FR_HIP(hipMemcpy(orbs, c->c_orbs, 4 * m, hipMemcpyDeviceToHost));
    if (vals) FR_HIP(hipMemcpy(vals, c->c_val, 8 * m, hipMemcpyDeviceToHost));
}
extern "C" int fries_apply_hbpp_sys(fries_ctx *h, uint32_t n_samp, const double rn[5], int unit_matrel,
                                    uint32_t *det_pos, uint8_t *orbs, double *vals, size_t cap, size_t *n_out, uint32_t comp_len[5]) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        c->comp_pending = false;
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        if (unit_matrel) fr_hbpp_apply_unit(c, n_samp, rn); else fr_hbpp_apply(c, n_samp, rn);
        size_t m = c->num_success;
        if (n_out) *n_out = m;
        if (comp_len) for (int k = 0; k < 5; k++) comp_len[k] = c->comp_len[k];
        fr_check_dev_err(c);
        c->comp_pending = true;     // the result stays in c_pos / c_orbs / c_val / d_nsucc for fries_spawn_from_comp and fries_comp_download
        comp_copy_out(c, det_pos, orbs, vals, cap);
    });
}
extern "C" int fries_apply_hbpp_piv(fries_ctx *h, uint32_t n_samp, int unit_matrel, uint32_t *det_pos, uint8_t *orbs, double *vals, size_t cap, size_t *n_out,
                                    uint32_t stage_len[5]) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        if (c->hh_mode || c->fq_mode || !c->W.cap) throw FriesError("fries_apply_hbpp_piv needs a context set up by fries_frisys_setup");
        if (c->spin_parity && !c->new_hb) throw FriesError("Time-reversal symmetry is only implemented for the unnormalized heat-bath distribution");       // heat_bathPP.cpp:1019-1021
        uint32_t sl[5] = {0, 0, 0, 0, 0};
        c->comp_pending = false;
        fr_hbpp_piv_apply(c, n_samp, unit_matrel, sl);
        size_t m = c->num_success;
        if (n_out) *n_out = m;
        if (stage_len) for (int k = 0; k < 5; k++) stage_len[k] = sl[k];
        fr_check_dev_err(c);
        c->comp_pending = true;
        comp_copy_out(c, det_pos, orbs, vals, cap);
    });
}

// ---- the loop body between apply_HBPP_sys and death / cloning (frisys_mol.cpp:424-485) for a host that keeps its own loop
static void need_frisys(FriesCtx *c, const char *who) {
    if (c->hh_mode || c->fq_mode || c->full_mode || !c->W.cap) throw FriesError(std::string(who) + " needs a context set up by fries_frisys_setup");
}
// frisys_mol.cpp:429-471 on the result the last fries_apply_hbpp_sys / fries_apply_hbpp_piv left on the device
extern "C" int fries_spawn_from_comp(fries_ctx *h, double eps, double init_thresh) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        need_frisys(c, "fries_spawn_from_comp");
        if (!c->comp_pending) throw FriesError("fries_spawn_from_comp: no compression result is pending -- call fries_apply_hbpp_sys or fries_apply_hbpp_piv first "
                                               "(a merge, a vector compression, fries_vec_load and fries_spawn_from_comp itself discard the result: its positions are those of the vector as it stood)");
        c->comp_pending = false;
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        fr_vec_maybe_rebuild(c, &c->vec);           // tombstones of earlier deletes (the fused loop does this once per iteration)
        fr_spawn_comp_result(c, eps, init_thresh);
        fr_check_dev_err(c);
    });
}
// frisys_mol.cpp:480-485
extern "C" int fries_dense_apply(fries_ctx *h) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        need_frisys(c, "fries_dense_apply");
        if (!c->n_dense_h_glob) return;
        fr_dense_multiply(c);
        fr_check_dev_err(c);
    });
}
// sol_vec.dense_norm() of frisys_mol.cpp:504
extern "C" int fries_dense_norm(fries_ctx *h, double *norm) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        need_frisys(c, "fries_dense_norm");
        const double dn = fr_dense_norm_all(c);
        if (norm) *norm = dn;
    });
}
extern "C" int fries_dense_h_count(fries_ctx *h, uint32_t *global_count) {
    return fr_api_host(h, [&](FriesCtx *c) {
        need_frisys(c, "fries_dense_h_count");
        if (global_count) *global_count = c->n_dense_h_glob;
    });
}
extern "C" int fries_dense_sizes(fries_ctx *h, uint32_t *sizes, size_t cap, size_t *n_ranks) {
    return fr_api_host(h, [&](FriesCtx *c) {
        if (n_ranks) *n_ranks = (size_t)c->n_ranks;
        if (cap < (size_t)c->n_ranks) throw FriesError("fries_dense_sizes: buffer smaller than the number of ranks");
        for (int r = 0; r < c->n_ranks; r++) sizes[r] = (size_t)r < c->dense_sizes.size() ? c->dense_sizes[r] : 0u;
    });
}
extern "C" int fries_comp_download(fries_ctx *h, uint32_t *det_pos, uint8_t *orbs, double *vals, size_t cap, size_t *n_out) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        need_frisys(c, "fries_comp_download");
        if (!c->comp_pending) throw FriesError("fries_comp_download: no compression result is pending");
        const size_t m = c->num_success;
        if (n_out) *n_out = m;
        comp_copy_out(c, det_pos, orbs, vals, cap, true);
    });
}

// ------------------------------------------------------------------ estimators between two contexts (the device is selected inside: fr_pair_begin)
// calc_h_dot (molecule.cpp:667-885) between two contexts' vectors: hdot.hip
extern "C" int fries_h_dot(fries_ctx *a, fries_ctx *b, fries_hdot_result *out) {
    return fr_api([&] {
        if (!a || !b || !out) throw FriesError("fries_h_dot: null argument");
        fr_h_dot(&a->c, &b->c, out);
    });
}
// one_elec_op (molecule.cpp:222-252) for every orbital pair at once, dotted with the other vector: rdm1.hip
extern "C" int fries_rdm1(fries_ctx *a, fries_ctx *b, double *gamma, fries_rdm1_result *out) {
    return fr_api([&] {
        if (!a || !b || !gamma || !out) throw FriesError("fries_rdm1: null argument");
        fr_rdm1(&a->c, &b->c, gamma, out);
    });
}
// the two-body density matrix between two contexts' vectors: rdm2.hip
extern "C" int fries_rdm2(fries_ctx *a, fries_ctx *b, double *gamma2, fries_rdm2_result *out) {
    return fr_api([&] {
        if (!a || !b || !gamma2 || !out) throw FriesError("fries_rdm2: null argument");
        fr_rdm2(&a->c, &b->c, gamma2, out);
    });
}

// ------------------------------------------------------------------ vector snapshots and the estimators over ranks: snapshot.hip
// the handles of a shard list as contexts; refuses a null list, a count outside 1 .. FR_MAX_RANKS and a null entry
static std::vector<FriesCtx *> shard_list(const char *who, fries_ctx *const *h, uint32_t n) {
    if (!h) throw FriesError(std::string(who) + ": null argument");
    if (n == 0 || n > FR_MAX_RANKS) throw FriesError(std::string(who) + ": the number of shards must be between 1 and " + std::to_string(FR_MAX_RANKS));
    std::vector<FriesCtx *> c(n);
    for (uint32_t k = 0; k < n; k++) {
        if (!h[k]) throw FriesError(std::string(who) + ": null argument (a shard)");
        c[k] = &h[k]->c;
    }
    return c;
}
extern "C" int fries_snapshot_create(fries_snapshot **s, fries_ctx *const *shards, uint32_t n_shards, int device) {
    return fr_api([&] {
        if (!s) throw FriesError("fries_snapshot_create: null argument");
        *s = nullptr;
        const std::vector<FriesCtx *> c = shard_list("fries_snapshot_create", shards, n_shards);
        *s = fr_snapshot_create(c.data(), n_shards, device);
    });
}
extern "C" int fries_snapshot_info(const fries_snapshot *s, fries_snapshot_info_t *out) {
    return fr_api([&] {
        if (!s || !out) throw FriesError("fries_snapshot_info: null argument");
        fr_snapshot_info(s, out);
    });
}
extern "C" int fries_snapshot_vector(const fries_snapshot *s, uint64_t *dets, double *vals, uint64_t cap, uint64_t *n) {
    return fr_api([&] {
        if (!s) throw FriesError("fries_snapshot_vector: null argument");
        fr_snapshot_vector(s, dets, vals, cap, n);
    });
}
extern "C" int fries_snapshot_destroy(fries_snapshot *s) {
    return fr_api([&] { fr_snapshot_destroy(s); });
}
extern "C" int fries_h_dot_ranks(fries_ctx *const *a, uint32_t n_a, const fries_snapshot *b, fries_hdot_result *out) {
    return fr_api([&] {
        if (!b || !out) throw FriesError("fries_h_dot_ranks: null argument");
        const std::vector<FriesCtx *> c = shard_list("fries_h_dot_ranks", a, n_a);
        fr_h_dot_ranks(c.data(), n_a, b, out);
    });
}
// column += coeff * snapshot, and the plain overlap with a snapshot: snapshot.hip
extern "C" int fries_vec_axpy_snapshot(fries_ctx *h, int column, double coeff, const fries_snapshot *x, uint64_t *n_taken) {
    return fr_api([&] {
        if (!h || !x || !n_taken) throw FriesError("fries_vec_axpy_snapshot: null argument");
        fr_vec_axpy_snapshot(&h->c, column, coeff, x, n_taken);
    });
}
extern "C" int fries_snapshot_dot(fries_ctx *const *a, uint32_t n_a, int column, const fries_snapshot *b, fries_vdot_result *out) {
    return fr_api([&] {
        if (!b || !out) throw FriesError("fries_snapshot_dot: null argument");
        const std::vector<FriesCtx *> c = shard_list("fries_snapshot_dot", a, n_a);
        fr_snapshot_dot(c.data(), n_a, column, b, out);
    });
}
extern "C" int fries_rdm1_ranks(fries_ctx *const *a, uint32_t n_a, const fries_snapshot *b, double *gamma, fries_rdm1_result *out) {
    return fr_api([&] {
        if (!b || !gamma || !out) throw FriesError("fries_rdm1_ranks: null argument");
        const std::vector<FriesCtx *> c = shard_list("fries_rdm1_ranks", a, n_a);
        fr_rdm1_ranks(c.data(), n_a, b, gamma, out);
    });
}
extern "C" int fries_rdm2_ranks(fries_ctx *const *a, uint32_t n_a, const fries_snapshot *b, double *gamma2, fries_rdm2_result *out) {
    return fr_api([&] {
        if (!b || !gamma2 || !out) throw FriesError("fries_rdm2_ranks: null argument");
        const std::vector<FriesCtx *> c = shard_list("fries_rdm2_ranks", a, n_a);
        fr_rdm2_ranks(c.data(), n_a, b, gamma2, out);
    });
}
