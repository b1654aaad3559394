// What the estimators between the solution vectors of two contexts share (hdot.hip: fr_h_dot / k_hdot, rdm1.hip: fr_rdm1 / k_rdm1,
// rdm2.hip: fr_rdm2 / k_rdm2_probe): on the host how a call begins, on the device how `b` is looked up.  `who` is the entry point's name.
// snapshot.hip begins its calls with fr_shards_check and fr_pair_n_pos: there a list of shards stands where one context stands here.
#pragma once
#include "ctx.hpp"
#include <cstring>
#include <sstream>

// ------------------------------------------------------------------ host
// a's curr_size, read back on its stream (a copy and a wait, no launch) and checked against the capacity.  w = "<entry point>: "
static inline uint32_t fr_pair_n_pos(const std::string &w, FriesCtx *a) {
    uint32_t n_pos = 0;
    FR_HIP(hipMemcpyAsync(&n_pos, &a->vec.st->curr_size, 4, hipMemcpyDeviceToHost, a->stream));
    FR_HIP(hipStreamSynchronize(a->stream));
    if (n_pos > a->vec.cap) throw FriesError(w + "the vector's size exceeds its capacity");
    return n_pos;
}
// Refuses what no such estimator handles -- everything that refuses comes before the first launch --, makes a's stream wait for what
// b's stream has enqueued so far (`b` is only read: it must have run before the probes start) and reads a's curr_size back.
// -> n_pos, checked against the capacity; the caller adds its own refusals, zeroes its outputs and leaves at once when n_pos == 0.
static inline uint32_t fr_pair_begin(const char *who, FriesCtx *a, FriesCtx *b) {
    const std::string w = std::string(who) + ": ";
    for (const FriesCtx *c : {a, b}) {
        if (c->hh_mode || c->vec.hh_sites) throw FriesError(w + "a Hubbard-Holstein context is not a molecular one (out of scope)");
        if (!c->d_eris || !c->d_hb) throw FriesError(w + "fries_set_molecule must be called on both contexts first");
        if (!c->vec.dets || !c->vec.hs) throw FriesError(w + "both contexts need a solution vector (run a setup first)");
    }
    for (const FriesCtx *c : {a, b})
        if (c->use_comm || c->n_ranks > 1) throw FriesError(w + "a context with a communicator holds one shard of its vector; the estimator over ranks is out of scope");
    if (a->device != b->device) throw FriesError(w + "the two contexts are on different devices");
    if (a->n_orb != b->n_orb || a->n_elec != b->n_elec) throw FriesError(w + "the two contexts differ in n_orb or n_elec (different molecules)");
    if (memcmp(a->h_hb.irrep, b->h_hb.irrep, a->n_orb)) throw FriesError(w + "the two contexts differ in their orbital irreps (different molecules)");
    FR_HIP(hipSetDevice(a->device));
    if (a != b) {
        struct Ev { hipEvent_t e = nullptr; ~Ev() { if (e) hipEventDestroy(e); } } ev;
        FR_HIP(hipEventCreateWithFlags(&ev.e, hipEventDisableTiming));
        FR_HIP(hipEventRecord(ev.e, b->stream));
        FR_HIP(hipStreamWaitEvent(a->stream, ev.e, 0));
    }
    return fr_pair_n_pos(w, a);
}
// ... and what the density matrices refuse on top: their kernels split a determinant into two n_orb-bit halves and walk it as it is stored
static inline uint32_t fr_pair_begin_rdm(const char *who, FriesCtx *a, FriesCtx *b) {
    const uint32_t n_pos = fr_pair_begin(who, a, b);
    const std::string w = std::string(who) + ": ";
    if (a->n_orb > FR_MAX_ORB) throw FriesError(w + "more than 32 orbitals");
    for (const FriesCtx *c : {a, b})
        if (c->spin_parity != 0) throw FriesError(w + "a context with spin_parity != 0 stores one representative per time-reversal pair; unfolding it is out of scope");
    return n_pos;
}
// What every entry point that reads or writes the solution vector of a molecular context refuses of that context, before it launches
// anything (fr_shards_check below; fries_vec_axpy_snapshot in snapshot.hip; fries_vec_scale and fries_vec_one_norm in api_vec.hip).  w = "<entry point>: "
static inline void fr_ctx_check(const std::string &w, const FriesCtx *c) {
    if (c->hh_mode || c->vec.hh_sites) throw FriesError(w + "a Hubbard-Holstein context is not a molecular one (out of scope)");
    if (!c->d_eris || !c->d_hb) throw FriesError(w + "fries_set_molecule must be called on every context first");
    if (!c->vec.dets || !c->vec.hs) throw FriesError(w + "every context needs a solution vector (run a setup first)");
}
static inline void fr_column_check(const std::string &w, int column) {
    if (column != 0 && column != 1) throw FriesError(w + "column must be 0 or 1");
}
// What a list of contexts must be to stand for ONE vector (fries_snapshot_create, the *_ranks estimators; snapshot.hip): molecular contexts
// with a solution vector that are exactly ranks 0 .. n - 1 of one run, in order, and agree in everything the estimators compare.  A context
// without a communicator is the one shard of a run of one.  "One run" is decided by what determines a run's content: the rank scramblers
// (drawn from the seed) and the iteration count -- two groups set up alike and iterated alike hold the same shards, bit for bit.
static inline void fr_shards_check(const char *who, FriesCtx *const *sh, uint32_t n) {
    const std::string w = std::string(who) + ": ";
    for (uint32_t k = 0; k < n; k++) fr_ctx_check(w, sh[k]);
    const FriesCtx *c0 = sh[0];
    for (uint32_t k = 0; k < n; k++) {
        const FriesCtx *c = sh[k];
        if ((uint32_t)c->n_ranks != n || (uint32_t)c->rank != k) {
            std::ostringstream os;
            os << w << "the shards must be ranks 0 .. P - 1 of one run, all of them and in order: entry " << k << " of " << n << " is rank " << c->rank << " of " << c->n_ranks;
            throw FriesError(os.str());
        }
        if (c->n_orb != c0->n_orb || c->n_elec != c0->n_elec) throw FriesError(w + "the shards differ in n_orb or n_elec (different molecules)");
        if (memcmp(c->h_hb.irrep, c0->h_hb.irrep, c0->n_orb)) throw FriesError(w + "the shards differ in their orbital irreps (different molecules)");
        if (c->proc_scr != c0->proc_scr) throw FriesError(w + "the shards belong to different runs (their rank scramblers differ)");
        if (c->iterat != c0->iterat) throw FriesError(w + "the shards belong to different runs or moments of a run (their iteration counts differ)");
        if (c->hf_en != c0->hf_en) throw FriesError(w + "the shards differ in hf_en, the offset of the diagonal (different molecules or --ham_shift)");
        if (c->spin_parity != c0->spin_parity) throw FriesError(w + "the shards differ in spin_parity");
    }
}
// refuses, before anything is launched, a scratch array sized from n_pos that the device has no room for
static inline void fr_need_free(const char *who, size_t bytes, const char *what, uint32_t n_pos) {
    size_t free_b = 0, total_b = 0;
    FR_HIP(hipMemGetInfo(&free_b, &total_b));
    if (bytes > free_b) {
        std::ostringstream os;
        os << who << ": " << what << " of " << n_pos << " positions need " << bytes << " bytes of device memory, " << free_b << " are free";
        throw FriesError(os.str());
    }
}

// ------------------------------------------------------------------ device
// The look-up: the caller loads the first 16-byte slot of every candidate of a round itself, so that those loads are independent of
// each other, and resolves them afterwards.
// -> value of determinant d in column 0 of V; 0 for a miss.  e = the slot the first probe returned.
__device__ __forceinline__ double hd_resolve(const VecDev &V, det_t d, uint32_t s, HSlot e) {
    const uint32_t mask = V.hcap - 1;
    for (uint32_t probe = 0; probe < V.hcap; probe++) {
        if (e.key == d) return e.val < V.cap ? V.v0[e.val] : 0.0;
        if (e.key == FR_EMPTY_KEY) return 0.0;
        s = (s + 1) & mask;
        e = V.hs[s];
    }
    return 0.0;
}

// One source of a wave of k_rdm1 / k_rdm2_probe: every lane holds one position's (value, determinant), the wave walks them in order.
struct PairSrc {
    double av; det_t det;       // the source, broadcast from the lane that holds it
    uint32_t sl0; HSlot e0;     // the first probe of the source itself in B (overlap, diagonal): in flight while the candidates are formed
    det_t occ0, occ1;           // the alpha / beta halves (n_orb <= 32)
    unsigned no0, no1;          // ... and their electrons
    // false: a hole, a zeroed entry or past the end (uniform over the wave); nothing else is set then
    // lowmask = the low n_orb bits
    __device__ __forceinline__ bool load(const VecDev &B, double my_val, unsigned long long my_det, int s, uint32_t n_orb, det_t lowmask) {
        av = __shfl(my_val, s);
        if (av == 0) return false;
        det = __shfl(my_det, s);
        sl0 = fr_hash_slot(det, B.hcap);
        e0 = B.hs[sl0];
        occ0 = det & lowmask; occ1 = (det >> n_orb) & lowmask;
        no0 = __popcll(occ0); no1 = __popcll(occ1);
        return true;
    }
};
