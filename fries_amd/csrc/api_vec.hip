// The extern "C" boundary of the solution vector (include/fries_hip.h): what a host that keeps DistVec's pointer semantics reads, writes and
// adds, matrix elements by the batch and H applied to a list -- with the kernels only these entry points launch.
#include "api.hpp"
#include "pair_frame.hpp"

// at most 2048 workgroups for the grid-stride kernels over the stored positions
static inline unsigned vec_grid(size_t m) { const unsigned nb = fr_blocks(m, FR_BLOCK); return nb > 2048 ? 2048 : nb; }

extern "C" int fries_vec_info(fries_ctx *h, uint32_t *curr_size, int32_t *n_nonz, uint32_t *n_free) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        if (curr_size) *curr_size = c->h_vst.curr_size;
        if (n_nonz) *n_nonz = c->h_vst.n_nonz;
        if (n_free) *n_free = c->h_vst.n_free;
    });
}

extern "C" int fries_vec_download(fries_ctx *h, uint64_t *dets, double *vals, size_t cap, size_t *n) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        size_t m = c->h_vst.curr_size;
        if (n) *n = m;
        if (cap < m) throw FriesError("output buffer too small");
        if (dets) FR_HIP(hipMemcpy(dets, c->vec.dets, 8 * m, hipMemcpyDeviceToHost));
        if (vals) FR_HIP(hipMemcpy(vals, c->vec.v0, 8 * m, hipMemcpyDeviceToHost));
    });
}

extern "C" int fries_vec_load(fries_ctx *h, const uint64_t *dets, const double *vals, size_t n) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        VecDev &v = c->vec;
        if (n > v.cap) throw FriesError("vector larger than max_dets");
        c->comp_pending = false;
        FR_HIP(hipMemsetAsync(v.v0, 0, 8 * (size_t)v.cap, c->stream));
        FR_HIP(hipMemsetAsync(v.v1, 0, 8 * (size_t)v.cap, c->stream));
        FR_HIP(hipMemsetAsync(v.diag, 0xff, 8 * (size_t)v.cap, c->stream));
        FR_HIP(hipMemsetAsync(v.active, 0, v.cap, c->stream));
        FR_HIP(hipMemsetAsync(v.active, 1, n, c->stream));
        FR_HIP(hipMemcpyAsync(v.dets, dets, 8 * n, hipMemcpyHostToDevice, c->stream));
        FR_HIP(hipMemcpyAsync(v.v0, vals, 8 * n, hipMemcpyHostToDevice, c->stream));
        VecState s{};
        s.curr_size = (uint32_t)n; s.n_nonz = (int32_t)n; s.n_used = (uint32_t)(v.hcap);   // forces the rebuild below
        FR_HIP(hipMemcpyAsync(v.st, &s, sizeof(s), hipMemcpyHostToDevice, c->stream));
        FR_HIP(hipMemsetAsync(v.stat_part, 0, 8 * (size_t)FR_STAT_STRIPES * FR_STAT_STRIDE, c->stream));
        c->h_vst = s;
        fr_vec_maybe_rebuild(c, &v);
        fr_vec_sync_state(c, &v, &c->h_vst);
        fr_check_dev_err(c);
    });
}

extern "C" int fries_vec_set_dense(fries_ctx *h, uint32_t n_dense) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        if (!c->vec.dets || c->hh_mode || c->fq_mode || c->full_mode) throw FriesError("fries_vec_set_dense needs a frisys_mol context (after fries_frisys_setup and fries_vec_load)");
        c->mem.release(c->d_dh_from); c->mem.release(c->d_dh_to); c->mem.release(c->d_dh_el);
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        fr_dense_declare(c, n_dense, false);
        fr_check_dev_err(c);
    });
}

static void need_column(int column) {
    if (column != 0 && column != 1) throw FriesError("column must be 0 or 1");
}
// ---- column mirrors for hosts that keep DistVec::values() / operator[] / matr_el_at_pos pointer semantics (include/FRIES/vec_utils.hpp)
extern "C" int fries_vec_column_download(fries_ctx *h, int column, double *out, size_t cap, size_t *n) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        need_column(column);
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        size_t m = c->h_vst.curr_size;
        if (n) *n = m;
        if (cap < m) throw FriesError("output buffer too small");
        if (out && m) FR_HIP(hipMemcpy(out, column ? c->vec.v1 : c->vec.v0, 8 * m, hipMemcpyDeviceToHost));
    });
}
extern "C" int fries_vec_column_upload(fries_ctx *h, int column, const double *in, size_t n) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        need_column(column);
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        if (n > c->h_vst.curr_size) throw FriesError("more values than stored positions");
        if (n) FR_HIP(hipMemcpy(column ? c->vec.v1 : c->vec.v0, in, 8 * n, hipMemcpyHostToDevice));
    });
}
extern "C" int fries_vec_column_zero(fries_ctx *h, int column) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        need_column(column);
        FR_HIP(hipMemsetAsync(column ? c->vec.v1 : c->vec.v0, 0, 8 * (size_t)c->vec.cap, c->stream));      // DistVec::zero_vec: the whole row (vec_utils.hpp:577-579)
    });
}
// DistVec::add_vecs(idx1, idx2, c) (vec_utils.hpp:553-557): v[idx1][i] += v[idx2][i] * c over the stored positions
__global__ void __launch_bounds__(FR_BLOCK) k_add_vecs(VecDev V, int idx1, int idx2, double cf) {
    const uint32_t n = V.st->curr_size;
    double *a = idx1 ? V.v1 : V.v0; const double *b = idx2 ? V.v1 : V.v0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) a[i] += b[i] * cf;
}
extern "C" int fries_vec_add_vecs(fries_ctx *h, int idx1, int idx2, double cf) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        need_column(idx1); need_column(idx2);
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        const uint32_t m = c->h_vst.curr_size;
        if (m) FR_LAUNCH(c, "k_add_vecs", k_add_vecs, dim3(vec_grid(m)), dim3(FR_BLOCK), c->vec, idx1, idx2, cf);
    });
}
// DistVec::matr_el_at_pos for every stored position (vec_utils.hpp:672-677): the cached diagonal element - hf_en, computed where missing
__global__ void __launch_bounds__(FR_BLOCK) k_fill_diag(VecDev V, SysDev S) {
    const uint32_t n = V.st->curr_size;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        if (!V.active[i]) continue;
        double d = V.diag[i];
        if (d != d) V.diag[i] = fr_diag_matrel(V.dets[i], S.h_core, S.eris, S.n_orb) - S.hf_en;
    }
}
extern "C" int fries_vec_diag_download(fries_ctx *h, double *out, size_t cap, size_t *n) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        size_t m = c->h_vst.curr_size;
        if (n) *n = m;
        if (cap < m) throw FriesError("output buffer too small");
        if (m) {
            FR_LAUNCH(c, "k_fill_diag", k_fill_diag, dim3(vec_grid(m)), dim3(FR_BLOCK), c->vec, fr_sysdev(c));
            FR_HIP(hipStreamSynchronize(c->stream));
            FR_HIP(hipMemcpy(out, c->vec.diag, 8 * m, hipMemcpyDeviceToHost));
        }
    });
}
// ---- a scale and a one-norm of a column (include/fries_hip.h: beside fries_vec_axpy_snapshot)
// what both refuse, by name and before anything is launched: the single-context frame of pair_frame.hpp
static void need_mol_vec(const char *who, const fries_ctx *h, int column) {
    const std::string w = std::string(who) + ": ";
    if (!h) throw FriesError(w + "null argument");
    fr_ctx_check(w, &h->c);
    fr_column_check(w, column);
}
// two positions per step where the pair is whole (the columns are 16-byte aligned), the odd last one on its own
__global__ void __launch_bounds__(FR_BLOCK) k_vec_scale(VecDev V, int column, double f) {
    const uint32_t n = V.st->curr_size < V.cap ? V.st->curr_size : V.cap, n2 = n >> 1;
    double *a = column ? V.v1 : V.v0;
    double2 *a2 = (double2 *)a;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (size_t)gridDim.x * blockDim.x) {
        double2 x = a2[i];
        x.x *= f; x.y *= f;
        a2[i] = x;
    }
    if ((n & 1u) && blockIdx.x == 0 && threadIdx.x == 0) a[n - 1] *= f;
}
extern "C" int fries_vec_scale(fries_ctx *h, int column, double factor) {
    return fr_api([&] {
        need_mol_vec("fries_vec_scale", h, column);
        FriesCtx *c = &h->c;
        FR_HIP(hipSetDevice(c->device));
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        const uint32_t m = c->h_vst.curr_size;
        c->comp_pending = false;        // a compression result left on the device was formed from the values as they stood
        if (m) FR_LAUNCH(c, "k_vec_scale", k_vec_scale, dim3(vec_grid((m + 1) / 2)), dim3(FR_BLOCK), c->vec, column, factor);
    });
}
extern "C" int fries_vec_one_norm(fries_ctx *h, int column, double *norm) {
    return fr_api([&] {
        need_mol_vec("fries_vec_one_norm", h, column);
        if (!norm) throw FriesError("fries_vec_one_norm: null argument");
        FriesCtx *c = &h->c;
        if (!c->vc.seq.total) throw FriesError("fries_vec_one_norm: the context has no compression scratch for the in-order sum (run a setup first)");
        FR_HIP(hipSetDevice(c->device));
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        *norm = fr_one_norm(c, column);
    });
}
// DistVec::dot(idx2, vals2, num2, hashes2) (vec_utils.hpp:228-238): sum over the list IN LIST ORDER of vals2[i] * v[column][pos(idx2[i])],
// absent determinants skipped -- bit-identical to the reference's loop (products in parallel, the additions by one lane in order)
__global__ void __launch_bounds__(FR_BLOCK) k_dot_list(VecDev V, int column, const det_t *dets, const double *w, uint32_t n, double *out) {
    __shared__ double prod[FR_BLOCK];
    const double *col = column ? V.v1 : V.v0;
    double acc = 0;
    for (uint32_t base = 0; base < n; base += FR_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        double p = 0;
        if (i < n) {
            uint32_t s = fr_hash_find(V, dets[i]);
            if (s != FR_NOPOS) { uint32_t pos = V.hs[s].val; if (pos < V.cap) p = w[i] * col[pos]; }
        }
        prod[threadIdx.x] = p;
        __syncthreads();
        if (threadIdx.x == 0) { const uint32_t m = n - base < FR_BLOCK ? n - base : FR_BLOCK; for (uint32_t j = 0; j < m; j++) acc += prod[j]; }   // + (+-0) leaves acc as it is
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = acc;
}
extern "C" int fries_vec_dot_list(fries_ctx *h, int column, const uint64_t *dets, const double *vals, size_t n, double *out) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        need_column(column);
        if (n > 0xffffffffull) throw FriesError("list too long");
        double r = 0;
        if (n) {
            DevMem tmp;
            det_t *dd = tmp.alloc<det_t>(n); double *dw = tmp.alloc<double>(n + 1);
            FR_HIP(hipMemcpy(dd, dets, 8 * n, hipMemcpyHostToDevice));
            FR_HIP(hipMemcpy(dw, vals, 8 * n, hipMemcpyHostToDevice));
            FR_LAUNCH(c, "k_dot_list", k_dot_list, dim3(1), dim3(FR_BLOCK), c->vec, column, dd, dw, (uint32_t)n, dw + n);
            FR_HIP(hipStreamSynchronize(c->stream));
            FR_HIP(hipMemcpy(&r, dw + n, 8, hipMemcpyDeviceToHost));
        }
        if (out) *out = r;
    });
}

extern "C" int fries_htrial_download(fries_ctx *h, uint64_t *dets, double *vals, size_t cap, size_t *n) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        if (n) *n = c->n_htrial;
        if (cap < c->n_htrial) throw FriesError("output buffer too small");
        FR_HIP(hipMemcpy(dets, c->htr_det, 8 * (size_t)c->n_htrial, hipMemcpyDeviceToHost));
        FR_HIP(hipMemcpy(vals, c->htr_val, 8 * (size_t)c->n_htrial, hipMemcpyDeviceToHost));
    });
}

// DistVec::add drops zero values before they reach the adder (vec_utils.hpp:418-423)
struct HostAdds {
    std::vector<det_t> d; std::vector<double> v; std::vector<uint8_t> f; uint32_t m;
    HostAdds(const uint64_t *dets, const double *vals, const uint8_t *ini, size_t n) {
        for (size_t i = 0; i < n; i++) if (vals[i] != 0) { d.push_back(dets[i]); v.push_back(vals[i]); f.push_back(ini[i]); }
        m = (uint32_t)d.size();
    }
};
extern "C" int fries_vec_add(fries_ctx *h, const uint64_t *dets, const double *vals, const uint8_t *ini, size_t n) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        if (n > c->sp.cap) throw FriesError("Too many elements added to Adder - must call perform_add() more frequently.");
        if (c->use_comm) throw FriesError("fries_vec_add is a one-rank entry point; with ranks, adds travel inside fries_frisys_iterate");
        const HostAdds a(dets, vals, ini, n);
        if (a.m) fr_spawn_upload_merge(c, a.d.data(), a.v.data(), a.f.data(), a.m, true);
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        fr_check_dev_err(c);
    });
}

// DistVec::add x n + perform_add(0) with curr_vec_idx = column: column 1 is where the drivers collect the spawns, judged by the
// initiator rule against column 0 (frisys_mol.cpp:424-471, vec_utils.hpp:606-641)
extern "C" int fries_vec_add_to(fries_ctx *h, int column, const uint64_t *dets, const double *vals, const uint8_t *ini, size_t n) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        need_column(column);
        if (n > c->sp.cap) throw FriesError("Too many elements added to Adder - must call perform_add() more frequently.");
        const HostAdds a(dets, vals, ini, n);
        if (a.m) {
            fr_vec_sync_state(c, &c->vec, &c->h_vst);
            fr_vec_maybe_rebuild(c, &c->vec);           // tombstones of earlier deletes (the fused loop does this once per iteration)
            fr_spawn_upload_merge(c, a.d.data(), a.v.data(), a.f.data(), a.m, column == 0);
        }
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        fr_check_dev_err(c);
    });
}

__global__ void k_matrel_batch(int kind, const det_t *dets, const uint8_t *orbs, size_t n, const double *hc, const double *eris, unsigned n_orb, double *out, int32_t *sign) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    det_t d = dets[i];
    const uint8_t *o = orbs ? orbs + 4 * i : nullptr;
    if (kind == 0) { out[i] = fr_diag_matrel(d, hc, eris, n_orb); if (sign) sign[i] = 1; }
    else if (kind == 1) { out[i] = fr_sing_matrel(d, o[0], o[1], hc, eris, n_orb); if (sign) sign[i] = fr_sing_parity(d, o[0], o[1]); }
    else { out[i] = fr_doub_matrel(o[0], o[1], o[2], o[3], eris, n_orb); if (sign) sign[i] = fr_doub_parity(d, o[0], o[1], o[2], o[3]); }
}
extern "C" int fries_matrel_batch(fries_ctx *h, int kind, const uint64_t *dets, const uint8_t *orbs, size_t n, double *out, int32_t *sign) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        if (!c->d_eris) throw FriesError("fries_set_molecule must be called first");
        if (n == 0) return;
        DevMem tmp;
        det_t *dd = tmp.alloc<det_t>(n); uint8_t *dob = tmp.alloc<uint8_t>(4 * n); double *dout = tmp.alloc<double>(n); int32_t *ds = tmp.alloc<int32_t>(n);
        FR_HIP(hipMemcpy(dd, dets, 8 * n, hipMemcpyHostToDevice));
        if (orbs) FR_HIP(hipMemcpy(dob, orbs, 4 * n, hipMemcpyHostToDevice));
        FR_LAUNCH(c, "k_matrel_batch", k_matrel_batch, dim3(fr_blocks(n, FR_BLOCK)), dim3(FR_BLOCK), kind, dd, orbs ? dob : nullptr, n, c->d_h, c->d_eris, c->n_orb, dout, ds);
        FR_HIP(hipStreamSynchronize(c->stream));
        FR_HIP(hipMemcpy(out, dout, 8 * n, hipMemcpyDeviceToHost));
        if (sign) FR_HIP(hipMemcpy(sign, ds, 4 * n, hipMemcpyDeviceToHost));
    });
}
// h_op_offdiag(vec, ..., dest_idx = 1, h_fac = 1, spin_parity) on a fresh two-column vector that holds the list in column 0 (molecule.cpp:448-665):
// the stored determinants in position order and column 1
extern "C" int fries_h_offdiag_list(fries_ctx *h, const uint64_t *dets, const double *vals, size_t n, uint64_t *out_dets, double *out_vals, size_t cap, size_t *n_out) {
    return fr_api_dev(h, [&](FriesCtx *c) {
        if (!c->d_eris) throw FriesError("fries_set_molecule must be called first");
        std::vector<det_t> src(dets, dets + n), od;
        std::vector<double> val(vals, vals + n), ov;
        fr_h_apply_list(c, src, val, od, ov, nullptr, nullptr, false);
        if (od.size() > cap) throw FriesError("fries_h_offdiag_list: output buffers too small");
        std::copy(od.begin(), od.end(), out_dets); std::copy(ov.begin(), ov.end(), out_vals);
        *n_out = od.size();
    });
}
