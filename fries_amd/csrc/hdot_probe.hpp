// The look-up the estimators between two vectors share (hdot.hip: k_hdot, rdm1.hip: k_rdm1): the caller loads the first 16-byte slot of
// every candidate of a round itself, so that those loads are independent of each other, and resolves them afterwards.
#pragma once
#include "fries_dev.hpp"

// value of determinant d in column 0 of V; 0 for a miss.  e = the slot the first probe returned.
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
