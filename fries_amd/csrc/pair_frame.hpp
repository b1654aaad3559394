// What an estimator between the solution vectors of two contexts (fr_h_dot, fr_rdm1) begins with.  `who` is the entry point's name.
#pragma once
#include "ctx.hpp"
#include <cstring>

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
    uint32_t n_pos = 0;
    FR_HIP(hipMemcpyAsync(&n_pos, &a->vec.st->curr_size, 4, hipMemcpyDeviceToHost, a->stream));
    FR_HIP(hipStreamSynchronize(a->stream));
    if (n_pos > a->vec.cap) throw FriesError(w + "the vector's size exceeds its capacity");
    return n_pos;
}
