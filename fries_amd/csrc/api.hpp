// What the extern "C" files (api.hip, api_vec.hip, api_test.hip) share: the handle, and the frame an entry point of include/fries_hip.h
// stands in -- an exception becomes -1 with its text in the slot fries_last_error reads (api.hip), anything else 0.
#pragma once
#include "ctx.hpp"
#include <cstring>

struct fries_ctx { FriesCtx c; };
void fr_set_error(const std::string &msg);      // the calling thread's error slot

template <class Body> static inline int fr_api(Body &&body) {
    try { body(); } catch (const std::exception &e) { fr_set_error(e.what()); return -1; }
    return 0;
}
// an entry point that only touches host state
template <class Body> static inline int fr_api_host(fries_ctx *h, Body &&body) {
    return fr_api([&] { body(&h->c); });
}
// an entry point that launches, copies or synchronises: the context's device is selected before anything else
template <class Body> static inline int fr_api_dev(fries_ctx *h, Body &&body) {
    return fr_api([&] { FR_HIP(hipSetDevice(h->c.device)); body(&h->c); });
}
