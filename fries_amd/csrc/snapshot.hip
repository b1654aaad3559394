// Vector snapshots, and the estimators between replicas over ranks (include/fries_hip.h: fries_snapshot_*, fries_*_ranks).
//
// The probing kernels of hdot.hip, rdm1.hip and rdm2.hip read four fields of the probed side: B.hs, B.hcap, B.v0 and B.cap.  A snapshot
// is exactly that for a whole (sharded) vector: the shards' live entries -- value != 0 -- as one (determinant, value) list and one
// open-addressed table over it, on one device, frozen.  It is built in three steps:
//   1. compaction, per shard on the shard's own stream: k_snap_count counts the live positions of every tile of SNAP_TILE positions,
//      k_snap_scan (one workgroup) turns the counts into the tiles' offsets, k_snap_write writes (det, val) in position order;
//   2. copy: the lists go to the snapshot's device behind each other, in rank order (hipMemcpyPeerAsync);
//   3. insert: k_snap_insert puts entry i under its determinant as k_hash_reinsert does -- fr_hash_slot, a 64-bit atomicCAS on the key,
//      linear probing, a plain store of the position.  Which slot a key ends in can depend on timing where two keys collide; what a
//      look-up returns cannot: every key is in the table once and hd_resolve probes until it finds it or an empty slot.
// Two more calls read a snapshot (below the estimators): fries_vec_axpy_snapshot adds coeff * snapshot into a context's vector -- the entries
// the context owns, filtered into its spawn buffers by the same count / scan / write and merged like any perform_add --, and
// fries_snapshot_dot is the plain overlap of a sharded vector with it, one look-up per position.
// Nothing reads the table before fr_snapshot_create has synchronised.  The sizes follow from the shards' curr_size (snapshot_plan.hpp)
// and are checked against the free memory of every device involved before the first allocation.
#include "ctx.hpp"
#include "snapshot_plan.hpp"
#include "axpy_plan.hpp"
#include "pair_frame.hpp"
#include <map>
#include <memory>

enum { SNAP_ERR_DUP = 1, SNAP_ERR_FULL = 2, SNAP_ERR_KEY = 4 };

struct fries_snapshot {
    DevMem mem;                         // owns the one allocation below
    int device = 0;
    uint32_t n_shards = 0, hcap = 0;
    uint64_t n_entries = 0;
    size_t bytes = 0;
    det_t *dets = nullptr; double *vals = nullptr; HSlot *hs = nullptr;
    // of the source, for the refusals of the estimators
    uint32_t n_orb = 0, n_elec = 0; uint8_t irrep[FR_MAX_ORB] = {}; double hf_en = 0; int spin_parity = 0;
    float ms[3] = {0, 0, 0};            // compaction (summed over the shards), copy, insert: measured under FRIES_SNAPSHOT_EVENTS=1 only
    // what the probing kernels take as B
    VecDev view() const {
        VecDev V{};
        V.cap = (uint32_t)n_entries; V.hcap = hcap; V.v0 = vals; V.hs = hs;
        return V;
    }
};

// ------------------------------------------------------------------ compaction
// thread t of tile b holds positions b * SNAP_TILE + 4 t .. + 3 -> their values (0 past the end), and how many are live
__device__ __forceinline__ uint32_t snap_load4(const double *v0, uint32_t n, double v[4]) {
    const size_t i0 = (size_t)blockIdx.x * SNAP_TILE + 4 * (size_t)threadIdx.x;
    if (i0 + 4 <= n) {
        const double2 x = *(const double2 *)(v0 + i0), y = *(const double2 *)(v0 + i0 + 2);
        v[0] = x.x; v[1] = x.y; v[2] = y.x; v[3] = y.y;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = i0 + j < n ? v0[i0 + j] : 0.0;
    }
    return (uint32_t)(v[0] != 0) + (uint32_t)(v[1] != 0) + (uint32_t)(v[2] != 0) + (uint32_t)(v[3] != 0);
}
__global__ void __launch_bounds__(FR_BLOCK) k_snap_count(const double *v0, uint32_t n, uint32_t *tile_cnt) {
    __shared__ uint32_t sh[4];
    double v[4];
    const uint32_t c = fr_block_sum_u32(snap_load4(v0, n, v), sh);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = c;
}
// one workgroup: the exclusive scan of the tiles' counts in tile order, FR_BLOCK tiles per step; *n_live = the list's length
__global__ void __launch_bounds__(FR_BLOCK) k_snap_scan(const uint32_t *tile_cnt, uint32_t n_tiles, uint32_t *tile_off, uint32_t *n_live) {
    __shared__ uint32_t sh[4];
    uint32_t base = 0;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += FR_BLOCK) {
        const uint32_t t = t0 + threadIdx.x, x = t < n_tiles ? tile_cnt[t] : 0u;
        uint32_t tot;
        const uint32_t incl = fr_block_scan_u32(x, sh, &tot);
        if (t < n_tiles) tile_off[t] = base + incl - x;
        base += tot;
    }
    if (threadIdx.x == 0) *n_live = base;
}
// out_det / out_val hold n entries; an offset is below the number of live positions, so below n
__global__ void __launch_bounds__(FR_BLOCK) k_snap_write(const det_t *dets, const double *v0, uint32_t n, const uint32_t *tile_off, det_t *out_det, double *out_val) {
    __shared__ uint32_t sh[4];
    double v[4];
    const uint32_t c = snap_load4(v0, n, v);
    uint32_t tot;
    uint32_t o = tile_off[blockIdx.x] + fr_block_scan_u32(c, sh, &tot) - c;
    const size_t i0 = (size_t)blockIdx.x * SNAP_TILE + 4 * (size_t)threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (v[j] != 0 && o < n) { out_det[o] = dets[i0 + j]; out_val[o] = v[j]; o++; }
}

// ------------------------------------------------------------------ the table
// every slot empty, as the vector's own table: key FR_EMPTY_KEY (0), position FR_NOPOS
__global__ void __launch_bounds__(FR_BLOCK) k_snap_clear(uint4 *hs, uint32_t hcap) {
    const uint4 e = make_uint4(0u, 0u, FR_NOPOS, 0u);
    for (size_t s = (size_t)blockIdx.x * FR_BLOCK + threadIdx.x; s < hcap; s += (size_t)gridDim.x * FR_BLOCK) hs[s] = e;
}
// entry i under dets[i] (k_hash_reinsert's loop).  A key met twice, a key that is no determinant, a full table: the error word.
__global__ void __launch_bounds__(FR_BLOCK) k_snap_insert(const det_t *dets, uint32_t n, HSlot *hs, uint32_t hcap, uint32_t *err) {
    const size_t i = (size_t)blockIdx.x * FR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const det_t d = dets[i];
    if (d == FR_EMPTY_KEY || d == FR_TOMB_KEY) { atomicOr(err, (uint32_t)SNAP_ERR_KEY); return; }
    uint32_t s = fr_hash_slot(d, hcap);
    for (uint32_t probe = 0; probe < hcap; probe++) {
        const det_t old = atomicCAS((unsigned long long *)&hs[s].key, (unsigned long long)FR_EMPTY_KEY, (unsigned long long)d);
        if (old == FR_EMPTY_KEY) { hs[s].val = (uint32_t)i; return; }
        if (old == d) { atomicOr(err, (uint32_t)SNAP_ERR_DUP); return; }
        s = (s + 1) & (hcap - 1);
    }
    atomicOr(err, (uint32_t)SNAP_ERR_FULL);
}

// ------------------------------------------------------------------ host
namespace {
struct Stream {
    hipStream_t s = nullptr;
    ~Stream() { if (s) hipStreamDestroy(s); }
};
struct Events {
    std::vector<hipEvent_t> ev;
    ~Events() { for (hipEvent_t e : ev) hipEventDestroy(e); }
    hipEvent_t make() { hipEvent_t e = nullptr; FR_HIP(hipEventCreate(&e)); ev.push_back(e); return e; }
};
float elapsed(hipEvent_t a, hipEvent_t b) { float ms = 0; FR_HIP(hipEventElapsedTime(&ms, a, b)); return ms; }
// the calling thread's current device, put back when the call leaves (these calls select devices of their own)
struct DeviceGuard {
    int dev = -1;
    DeviceGuard() { if (hipGetDevice(&dev) != hipSuccess) dev = -1; }
    ~DeviceGuard() { if (dev >= 0) hipSetDevice(dev); }
};
// FRIES_SNAPSHOT_EVENTS=1: fries_snapshot_create times its three steps with HIP events (fries_snapshot_info; tests/scripts/gpu_snapshot_cost.py)
bool snap_events() { static const bool on = getenv("FRIES_SNAPSHOT_EVENTS") && atoi(getenv("FRIES_SNAPSHOT_EVENTS")) != 0; return on; }
// FRIES_HASH_FILL, as vec.hip's hash_slots_for reads it: percent of the slots the entries may take
int snap_fill() { static const int fill = getenv("FRIES_HASH_FILL") ? atoi(getenv("FRIES_HASH_FILL")) : SNAP_FILL_PCT; return fill > 0 && fill <= 100 ? fill : SNAP_FILL_PCT; }
}

fries_snapshot *fr_snapshot_create(FriesCtx *const *sh, uint32_t n_sh, int device) {
    const char *who = "fries_snapshot_create";
    const std::string w = std::string(who) + ": ";
    DeviceGuard dg;
    const bool timed = snap_events();
    fr_shards_check(who, sh, n_sh);
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) throw FriesError(w + "device index out of range");
    // the shards' sizes (a copy and a wait each), then every size of the build
    std::vector<uint32_t> n_pos(n_sh);
    for (uint32_t k = 0; k < n_sh; k++) { FR_HIP(hipSetDevice(sh[k]->device)); n_pos[k] = fr_pair_n_pos(w, sh[k]); }
    const SnapPlan plan = fr_snap_plan(n_pos.data(), n_sh, snap_fill());
    if (plan.too_many) {
        std::ostringstream os;
        os << w << plan.n_bound << " positions are more than one look-up table holds (at most " << SNAP_MAX_ENTRIES << ", and " << SNAP_MAX_SLOTS << " slots at " << snap_fill() << " % fill)";
        throw FriesError(os.str());
    }
    std::map<int, size_t> need;
    need[device] += plan.bytes;
    for (uint32_t k = 0; k < n_sh; k++) if (n_pos[k]) need[sh[k]->device] += plan.stage[k].bytes;
    for (const auto &dv : need) { FR_HIP(hipSetDevice(dv.first)); fr_need_free(who, dv.second, "the snapshot and its staging", (uint32_t)plan.n_bound); }

    std::unique_ptr<fries_snapshot> s(new fries_snapshot());
    const FriesCtx *c0 = sh[0];
    s->device = device; s->n_shards = n_sh; s->hcap = plan.slots; s->bytes = plan.bytes;
    s->n_orb = c0->n_orb; s->n_elec = c0->n_elec; s->hf_en = c0->hf_en; s->spin_parity = c0->spin_parity;
    memcpy(s->irrep, c0->h_hb.irrep, sizeof(s->irrep));
    FR_HIP(hipSetDevice(device));
    uint8_t *base = s->mem.alloc<uint8_t>(plan.bytes);
    s->dets = (det_t *)(base + plan.det); s->vals = (double *)(base + plan.val); s->hs = (HSlot *)(base + plan.hs);
    uint32_t *d_err = (uint32_t *)(base + plan.err);
    Stream st;
    FR_HIP(hipStreamCreate(&st.s));
    Events evs;
    hipEvent_t e_copy0 = nullptr, e_copy1 = nullptr, e_ins = nullptr;
    if (timed) { e_copy0 = evs.make(); e_copy1 = evs.make(); e_ins = evs.make(); }

    // 1. compaction on every shard's own stream
    DevMem stage;
    std::vector<uint8_t *> sbase(n_sh, nullptr);
    std::vector<uint32_t> n_live(n_sh, 0);
    std::vector<hipEvent_t> e0(n_sh, nullptr), e1(n_sh, nullptr);
    for (uint32_t k = 0; k < n_sh; k++) {
        if (!n_pos[k]) continue;
        FriesCtx *c = sh[k];
        const SnapStage &g = plan.stage[k];
        FR_HIP(hipSetDevice(c->device));
        uint8_t *b = sbase[k] = stage.alloc<uint8_t>(g.bytes);
        if (timed) { e0[k] = evs.make(); e1[k] = evs.make(); }
        uint32_t *tile_cnt = (uint32_t *)(b + g.tile_cnt), *tile_off = (uint32_t *)(b + g.tile_off), *d_live = (uint32_t *)(b + g.n_live);
        if (timed) FR_HIP(hipEventRecord(e0[k], c->stream));
        FR_LAUNCH(c, "k_snap_count", k_snap_count, dim3(g.n_tiles), dim3(FR_BLOCK), (const double *)c->vec.v0, g.n_pos, tile_cnt);
        FR_LAUNCH(c, "k_snap_scan", k_snap_scan, dim3(1), dim3(FR_BLOCK), (const uint32_t *)tile_cnt, g.n_tiles, tile_off, d_live);
        FR_LAUNCH(c, "k_snap_write", k_snap_write, dim3(g.n_tiles), dim3(FR_BLOCK), (const det_t *)c->vec.dets, (const double *)c->vec.v0, g.n_pos, (const uint32_t *)tile_off,
                  (det_t *)(b + g.det), (double *)(b + g.val));
        if (timed) FR_HIP(hipEventRecord(e1[k], c->stream));
        FR_HIP(hipMemcpyAsync(&n_live[k], d_live, 4, hipMemcpyDeviceToHost, c->stream));
    }
    for (uint32_t k = 0; k < n_sh; k++) {
        if (!n_pos[k]) continue;
        FR_HIP(hipSetDevice(sh[k]->device));
        FR_HIP(hipStreamSynchronize(sh[k]->stream));
        if (n_live[k] > n_pos[k]) throw FriesError(w + "a shard's live entries exceed its size");
        if (timed) s->ms[0] += elapsed(e0[k], e1[k]);
    }
    // 2. the lists behind each other on the snapshot's device, in rank order
    const std::vector<uint64_t> off = fr_snap_concat(n_live.data(), n_sh);
    s->n_entries = off[n_sh];
    if (s->n_entries > plan.n_bound) throw FriesError(w + "more entries than planned");
    FR_HIP(hipSetDevice(device));
    if (timed) FR_HIP(hipEventRecord(e_copy0, st.s));
    for (uint32_t k = 0; k < n_sh; k++) {
        if (!n_live[k]) continue;
        const SnapStage &g = plan.stage[k];
        FR_HIP(hipMemcpyPeerAsync(s->dets + off[k], device, sbase[k] + g.det, sh[k]->device, 8 * (size_t)n_live[k], st.s));
        FR_HIP(hipMemcpyPeerAsync(s->vals + off[k], device, sbase[k] + g.val, sh[k]->device, 8 * (size_t)n_live[k], st.s));
    }
    if (timed) FR_HIP(hipEventRecord(e_copy1, st.s));
    // 3. the table
    FR_HIP(hipMemsetAsync(d_err, 0, 4, st.s));
    hipLaunchKernelGGL(k_snap_clear, dim3(std::min<unsigned>(fr_blocks(plan.slots, FR_BLOCK), 4096u)), dim3(FR_BLOCK), 0, st.s, (uint4 *)s->hs, plan.slots);
    if (s->n_entries)
        hipLaunchKernelGGL(k_snap_insert, dim3(fr_blocks(s->n_entries, FR_BLOCK)), dim3(FR_BLOCK), 0, st.s, (const det_t *)s->dets, (uint32_t)s->n_entries, s->hs, plan.slots, d_err);
    FR_HIP(hipGetLastError());
    if (timed) FR_HIP(hipEventRecord(e_ins, st.s));
    uint32_t err = 0;
    FR_HIP(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, st.s));
    FR_HIP(hipStreamSynchronize(st.s));
    if (timed) { s->ms[1] = elapsed(e_copy0, e_copy1); s->ms[2] = elapsed(e_copy1, e_ins); }
    if (err) {
        std::ostringstream os;
        os << w << "the look-up table could not be built:" << ((err & SNAP_ERR_DUP) ? " a determinant is stored twice (in two shards?)" : "")
           << ((err & SNAP_ERR_KEY) ? " a stored index is no determinant" : "") << ((err & SNAP_ERR_FULL) ? " the table is full" : "");
        throw FriesError(os.str());
    }
    return s.release();         // `stage` frees the shards' staging here
}

void fr_snapshot_info(const fries_snapshot *s, fries_snapshot_info_t *out) {
    *out = fries_snapshot_info_t{};
    out->n_entries = s->n_entries; out->n_shards = s->n_shards; out->n_slots = s->hcap; out->device_bytes = s->bytes; out->device = s->device;
    out->ms_compact = s->ms[0]; out->ms_copy = s->ms[1]; out->ms_insert = s->ms[2];
}

void fr_snapshot_vector(const fries_snapshot *s, uint64_t *dets, double *vals, uint64_t cap, uint64_t *n) {
    if (n) *n = s->n_entries;
    if (cap < s->n_entries) throw FriesError("fries_snapshot_vector: output buffer too small");
    DeviceGuard dg;
    FR_HIP(hipSetDevice(s->device));
    if (dets && s->n_entries) FR_HIP(hipMemcpy(dets, s->dets, 8 * (size_t)s->n_entries, hipMemcpyDeviceToHost));
    if (vals && s->n_entries) FR_HIP(hipMemcpy(vals, s->vals, 8 * (size_t)s->n_entries, hipMemcpyDeviceToHost));
}

void fr_snapshot_destroy(fries_snapshot *s) {
    if (!s) return;
    DeviceGuard dg;
    hipSetDevice(s->device);
    delete s;
}

// ------------------------------------------------------------------ the estimators with `a` sharded, against a snapshot
// Everything that refuses comes before the first launch; -> every shard's curr_size.  rdm: the density matrices' own refusals on top.
static std::vector<uint32_t> ranks_begin(const char *who, FriesCtx *const *a, uint32_t n_a, const fries_snapshot *b, bool rdm) {
    const std::string w = std::string(who) + ": ";
    fr_shards_check(who, a, n_a);
    const FriesCtx *a0 = a[0];
    for (uint32_t k = 0; k < n_a; k++)
        if (a[k]->device != b->device) throw FriesError(w + "a shard of `a` and the snapshot are on different devices");
    if (a0->n_orb != b->n_orb || a0->n_elec != b->n_elec) throw FriesError(w + "`a` and the snapshot differ in n_orb or n_elec (different molecules)");
    if (memcmp(a0->h_hb.irrep, b->irrep, a0->n_orb)) throw FriesError(w + "`a` and the snapshot differ in their orbital irreps (different molecules)");
    if (rdm) {
        if (a0->n_orb > FR_MAX_ORB) throw FriesError(w + "more than 32 orbitals");
        if (a0->spin_parity != 0 || b->spin_parity != 0)
            throw FriesError(w + "a vector with spin_parity != 0 stores one representative per time-reversal pair; unfolding it is out of scope");
    } else {
        if (a0->hf_en != b->hf_en) throw FriesError(w + "`a` and the snapshot differ in hf_en, the offset of the diagonal (different molecules or --ham_shift)");
        if (a0->spin_parity != b->spin_parity) throw FriesError(w + "`a` and the snapshot differ in spin_parity");
    }
    FR_HIP(hipSetDevice(b->device));
    std::vector<uint32_t> n_pos(n_a);
    for (uint32_t k = 0; k < n_a; k++) n_pos[k] = fr_pair_n_pos(w, a[k]);
    return n_pos;
}

void fr_h_dot_ranks(FriesCtx *const *a, uint32_t n_a, const fries_snapshot *b, fries_hdot_result *out) {
    DeviceGuard dg;
    const std::vector<uint32_t> n_pos = ranks_begin("fries_h_dot_ranks", a, n_a, b, false);
    const VecDev B = b->view();
    *out = fries_hdot_result{};
    for (uint32_t k = 0; k < n_a; k++) {
        fries_hdot_result r;
        fr_h_dot_core(a[k], B, n_pos[k], &r);
        if (k == 0) { *out = r; continue; }
        out->h += r.h; out->ovlp += r.ovlp; out->abs_sum += r.abs_sum;
        out->n_src += r.n_src; out->n_terms += r.n_terms; out->n_hits += r.n_hits;
    }
}

void fr_rdm1_ranks(FriesCtx *const *a, uint32_t n_a, const fries_snapshot *b, double *gamma, fries_rdm1_result *out) {
    DeviceGuard dg;
    const std::vector<uint32_t> n_pos = ranks_begin("fries_rdm1_ranks", a, n_a, b, true);
    const VecDev B = b->view();
    const size_t n2 = (size_t)b->n_orb * b->n_orb;
    std::vector<double> g(n_a > 1 ? n2 : 0);
    for (uint32_t k = 0; k < n_a; k++) {
        fries_rdm1_result r;
        fr_rdm1_core("fries_rdm1_ranks", a[k], B, n_pos[k], k == 0 ? gamma : g.data(), &r);
        if (k == 0) { *out = r; continue; }
        for (size_t j = 0; j < n2; j++) gamma[j] += g[j];
        out->ovlp += r.ovlp; out->abs_sum += r.abs_sum;
        out->n_src += r.n_src; out->n_terms += r.n_terms; out->n_hits += r.n_hits;
    }
}

void fr_rdm2_ranks(FriesCtx *const *a, uint32_t n_a, const fries_snapshot *b, double *gamma2, fries_rdm2_result *out) {
    const char *who = "fries_rdm2_ranks";
    DeviceGuard dg;
    const std::vector<uint32_t> n_pos = ranks_begin(who, a, n_a, b, true);
    const VecDev B = b->view();
    const size_t n2 = (size_t)b->n_orb * b->n_orb, n4 = n2 * n2;
    std::vector<double> g(n_a > 1 ? n4 : 0);
    // every shard's counting pass and every capacity refusal first: a call that is refused has written no record, and leaves gamma2 and *out zero
    std::vector<std::unique_ptr<Rdm2Pass>> pass(n_a);
    std::vector<fries_rdm2_result> r(n_a);
    *out = fries_rdm2_result{};
    std::fill(gamma2, gamma2 + n4, 0.0);
    for (uint32_t k = 0; k < n_a; k++) {
        pass[k].reset(new Rdm2Pass());
        fr_rdm2_count(who, a[k], B, n_pos[k], *pass[k], k == 0 ? gamma2 : g.data(), &r[k]);
    }
    for (uint32_t k = 0; k < n_a; k++) fr_rdm2_refuse(who, a[k], *pass[k], (" of shard " + std::to_string(k)).c_str());
    for (uint32_t k = 0; k < n_a; k++) {
        if (k > 0) std::fill(g.begin(), g.end(), 0.0);
        fr_rdm2_emit(who, a[k], B, *pass[k], k == 0 ? gamma2 : g.data());      // (symmetrised per shard: bins [pq][rs] and [rs][pq] see the same additions)
        pass[k].reset();
        if (k == 0) { *out = r[0]; continue; }
        for (size_t j = 0; j < n4; j++) gamma2[j] += g[j];
        out->ovlp += r[k].ovlp; out->abs_sum += r[k].abs_sum;
        out->n_src += r[k].n_src; out->n_terms += r[k].n_terms; out->n_hits += r[k].n_hits;
    }
}

// ------------------------------------------------------------------ column += coeff * snapshot (fries_vec_axpy_snapshot)
static_assert(AXPY_TILE == 4 * FR_BLOCK && AXPY_TILE == SNAP_TILE, "a thread holds 4 contiguous entries of its tile");
static_assert(AXPY_MAX_TILES <= FR_MAX_PART, "the tiles' counts live in SpawnBuf::pcnt");
// thread t of tile b holds entries b * AXPY_TILE + 4 t .. + 3 of the chunk -> their determinants and products fl(coeff * x), 0 past the
// end and for an entry another rank owns; and how many are taken (a product of 0 is dropped, as HostAdds drops zero values)
__device__ __forceinline__ uint32_t axpy_load4(const det_t *dets, const double *vals, uint32_t n, double coeff, const uint32_t *scr, uint32_t n_ranks, uint32_t rank,
                                               det_t d[4], double p[4]) {
    const size_t i0 = (size_t)blockIdx.x * AXPY_TILE + 4 * (size_t)threadIdx.x;
    const bool al16 = (((uintptr_t)dets | (uintptr_t)vals) & 15u) == 0;      // a chunk starts at a multiple of the spawn capacity, which may be odd
    if (i0 + 4 <= n && al16) {
        const double2 x = *(const double2 *)(vals + i0), y = *(const double2 *)(vals + i0 + 2);
        const ulonglong2 a = *(const ulonglong2 *)(dets + i0), b = *(const ulonglong2 *)(dets + i0 + 2);
        p[0] = x.x; p[1] = x.y; p[2] = y.x; p[3] = y.y;
        d[0] = a.x; d[1] = a.y; d[2] = b.x; d[3] = b.y;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) { const bool in = i0 + j < n; p[j] = in ? vals[i0 + j] : 0.0; d[j] = in ? dets[i0 + j] : 0ull; }
    }
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        p[j] = coeff * p[j];
        if (p[j] != 0 && n_ranks > 1 && fr_proc_of(d[j], scr, n_ranks) != rank) p[j] = 0.0;
        c += (uint32_t)(p[j] != 0);
    }
    return c;
}
__global__ void __launch_bounds__(FR_BLOCK) k_axpy_count(const det_t *dets, const double *vals, uint32_t n, double coeff, const uint32_t *scr, uint32_t n_ranks, uint32_t rank,
                                                         uint32_t *tile_cnt) {
    __shared__ uint32_t sh[4];
    det_t d[4]; double p[4];
    const uint32_t c = fr_block_sum_u32(axpy_load4(dets, vals, n, coeff, scr, n_ranks, rank, d, p), sh);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = c;
}
// the taken entries in list order into the spawn list, every one with the initiator flag; out_* hold n entries and an offset is below
// the number of taken entries, so below n
__global__ void __launch_bounds__(FR_BLOCK) k_axpy_write(const det_t *dets, const double *vals, uint32_t n, double coeff, const uint32_t *scr, uint32_t n_ranks, uint32_t rank,
                                                         const uint32_t *tile_off, det_t *out_det, double *out_val, uint8_t *out_ini) {
    __shared__ uint32_t sh[4];
    det_t d[4]; double p[4];
    const uint32_t c = axpy_load4(dets, vals, n, coeff, scr, n_ranks, rank, d, p);
    uint32_t tot;
    uint32_t o = tile_off[blockIdx.x] + fr_block_scan_u32(c, sh, &tot) - c;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (p[j] != 0 && o < n) { out_det[o] = d[j]; out_val[o] = p[j]; out_ini[o] = 1; o++; }
}

// what fries_vec_axpy_snapshot and fries_snapshot_dot refuse of a context (list) against a snapshot, beyond fr_shards_check's own
static void snap_match(const std::string &w, const FriesCtx *c, const fries_snapshot *b) {
    if (c->device != b->device) throw FriesError(w + "the context and the snapshot are on different devices");
    if (c->n_orb != b->n_orb || c->n_elec != b->n_elec) throw FriesError(w + "the context and the snapshot differ in n_orb or n_elec (different molecules)");
    if (memcmp(c->h_hb.irrep, b->irrep, c->n_orb)) throw FriesError(w + "the context and the snapshot differ in their orbital irreps (different molecules)");
    if (c->spin_parity != b->spin_parity) throw FriesError(w + "the context and the snapshot differ in spin_parity");
}

void fr_vec_axpy_snapshot(FriesCtx *c, int column, double coeff, const fries_snapshot *x, uint64_t *n_taken) {
    const std::string w = "fries_vec_axpy_snapshot: ";
    // one shard of a run, with or without a communicator: fr_ctx_check, not fr_shards_check's completeness rule
    fr_ctx_check(w, c);
    if (!c->sp.det) throw FriesError(w + "the context has no spawn buffers (run a setup first)");
    fr_column_check(w, column);
    snap_match(w, c, x);
    if (c->n_ranks > 1 && !c->d_proc_scr) throw FriesError(w + "a context of several ranks without its rank scrambler (run a setup first)");
    *n_taken = 0;
    if (coeff == 0 || x->n_entries == 0) return;
    const AxpyPlan plan = fr_axpy_plan(x->n_entries, c->sp.cap);
    if (plan.refused) throw FriesError(w + "the context's spawn capacity cannot stage a chunk");
    FR_HIP(hipSetDevice(c->device));
    SpawnBuf &S = c->sp;
    uint32_t *tile_cnt = S.pcnt, *tile_off = S.flag;        // [n_tiles] each: n_tiles <= AXPY_MAX_TILES and <= the chunk's entries <= S.cap
    const uint32_t n_ranks = c->use_comm ? (uint32_t)c->n_ranks : 1u;
    uint64_t taken = 0;
    for (const AxpyChunk &k : plan.chunk) {
        fr_vec_sync_state(c, &c->vec, &c->h_vst);
        fr_vec_maybe_rebuild(c, &c->vec);           // tombstones of earlier deletes, as fries_vec_add_to
        const det_t *dets = x->dets + k.off; const double *vals = x->vals + k.off;
        FR_LAUNCH(c, "k_axpy_count", k_axpy_count, dim3(k.n_tiles), dim3(FR_BLOCK), dets, vals, k.n, coeff, (const uint32_t *)c->d_proc_scr, n_ranks, (uint32_t)c->rank, tile_cnt);
        FR_LAUNCH(c, "k_snap_scan", k_snap_scan, dim3(1), dim3(FR_BLOCK), (const uint32_t *)tile_cnt, k.n_tiles, tile_off, S.n_spawn);
        FR_LAUNCH(c, "k_axpy_write", k_axpy_write, dim3(k.n_tiles), dim3(FR_BLOCK), dets, vals, k.n, coeff, (const uint32_t *)c->d_proc_scr, n_ranks, (uint32_t)c->rank,
                  (const uint32_t *)tile_off, S.det, S.val, S.ini);
        uint32_t m = 0;
        FR_HIP(hipMemcpyAsync(&m, S.n_spawn, 4, hipMemcpyDeviceToHost, c->stream));
        FR_HIP(hipStreamSynchronize(c->stream));
        if (m > k.n) throw FriesError(w + "more entries taken than the chunk holds");
        if (m) fr_vec_merge(c, &c->vec, m, column == 0);
        taken += m;
    }
    *n_taken = taken;
    fr_vec_sync_state(c, &c->vec, &c->h_vst);
    fr_check_dev_err(c);
}

// ------------------------------------------------------------------ <a|snapshot> (fries_snapshot_dot)
// One workgroup per tile of AXPY_TILE positions of the shard; a thread takes 4 contiguous positions, issues the first probes of those
// with a non-zero value together and resolves them afterwards (hd_resolve).  No floating-point atomics: a thread adds its products in
// position order, fr_block_sum combines the lanes of a wave by the fixed butterfly and the four waves in order, and the tiles' partials
// are added in tile order on the host -- the association order is a function of curr_size alone.
__global__ void __launch_bounds__(FR_BLOCK) k_snap_dot(const det_t *dets, const double *col, uint32_t n, VecDev B, double *p_dot, double *p_abs, uint32_t *p_src, uint32_t *p_hits) {
    __shared__ double shd[4];
    __shared__ uint32_t shu[4];
    double v[4];
    uint32_t n_src = snap_load4(col, n, v), n_hits = 0;
    const size_t i0 = (size_t)blockIdx.x * AXPY_TILE + 4 * (size_t)threadIdx.x;
    det_t d[4]; uint32_t sl[4]; HSlot e[4];
    if (i0 + 4 <= n) {
        const ulonglong2 a = *(const ulonglong2 *)(dets + i0), b = *(const ulonglong2 *)(dets + i0 + 2);
        d[0] = a.x; d[1] = a.y; d[2] = b.x; d[3] = b.y;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) d[j] = i0 + j < n ? dets[i0 + j] : 0ull;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        sl[j] = fr_hash_slot(d[j], B.hcap);
        e[j].key = FR_EMPTY_KEY; e[j].val = FR_NOPOS;
        if (v[j] != 0) e[j] = B.hs[sl[j]];
    }
    double acc = 0, ab = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (v[j] == 0) continue;
        const double bv = hd_resolve(B, d[j], sl[j], e[j]);
        if (bv != 0) { const double t = v[j] * bv; acc += t; ab += fabs(t); n_hits++; }
    }
    acc = fr_block_sum(acc, shd); ab = fr_block_sum(ab, shd);
    n_src = fr_block_sum_u32(n_src, shu); n_hits = fr_block_sum_u32(n_hits, shu);
    if (threadIdx.x == 0) { p_dot[blockIdx.x] = acc; p_abs[blockIdx.x] = ab; p_src[blockIdx.x] = n_src; p_hits[blockIdx.x] = n_hits; }
}

void fr_snapshot_dot(FriesCtx *const *a, uint32_t n_a, int column, const fries_snapshot *b, fries_vdot_result *out) {
    const char *who = "fries_snapshot_dot";
    const std::string w = std::string(who) + ": ";
    DeviceGuard dg;
    fr_shards_check(who, a, n_a);
    fr_column_check(w, column);
    for (uint32_t k = 0; k < n_a; k++) snap_match(w, a[k], b);
    FR_HIP(hipSetDevice(b->device));
    std::vector<uint32_t> n_pos(n_a);
    for (uint32_t k = 0; k < n_a; k++) n_pos[k] = fr_pair_n_pos(w, a[k]);
    *out = fries_vdot_result{};
    const VecDev B = b->view();
    // every shard's pass on its own stream, then the shards' partials in rank order
    DevMem tmp;
    std::vector<VdotPlan> plan(n_a);
    std::vector<uint8_t *> base(n_a, nullptr);
    for (uint32_t k = 0; k < n_a; k++) {
        if (!n_pos[k]) continue;
        FriesCtx *c = a[k];
        const VdotPlan &g = plan[k] = fr_vdot_plan(n_pos[k]);
        uint8_t *p = base[k] = tmp.alloc<uint8_t>(g.bytes);
        FR_LAUNCH(c, "k_snap_dot", k_snap_dot, dim3(g.n_tiles), dim3(FR_BLOCK), (const det_t *)c->vec.dets, (const double *)(column ? c->vec.v1 : c->vec.v0), n_pos[k], B,
                  (double *)(p + g.dot), (double *)(p + g.abs_sum), (uint32_t *)(p + g.n_src), (uint32_t *)(p + g.n_hits));
    }
    std::vector<uint8_t> h;
    for (uint32_t k = 0; k < n_a; k++) {
        if (!n_pos[k]) continue;
        const VdotPlan &g = plan[k];
        h.resize(g.bytes);
        FR_HIP(hipMemcpyAsync(h.data(), base[k], g.bytes, hipMemcpyDeviceToHost, a[k]->stream));
        FR_HIP(hipStreamSynchronize(a[k]->stream));
        const double *hd = (const double *)(h.data() + g.dot), *ha = (const double *)(h.data() + g.abs_sum);
        const uint32_t *hs = (const uint32_t *)(h.data() + g.n_src), *hh = (const uint32_t *)(h.data() + g.n_hits);
        double dot = 0, ab = 0;
        for (uint32_t t = 0; t < g.n_tiles; t++) { dot += hd[t]; ab += ha[t]; out->n_src += hs[t]; out->n_hits += hh[t]; }
        out->dot += dot; out->abs_sum += ab;
    }
}
