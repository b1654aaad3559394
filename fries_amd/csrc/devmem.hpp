// The one place that allocates and frees device and pinned host memory.  A DevMem owns what it hands out until release() or its
// destructor; it caches nothing and sub-allocates nothing -- every alloc is one hipMalloc, every release one hipFree, at the moment
// of the call.  (Included by ctx.hpp, behind FR_HIP.)
#pragma once
#include <algorithm>
#include <vector>

class DevMem {
    std::vector<void *> dev_, host_;
public:
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    ~DevMem() {
        for (void *p : dev_) hipFree(p);
        for (void *p : host_) hipHostFree(p);
    }
    // n elements of T in device memory (one element when n == 0, so that every array has an address)
    template <class T> T *alloc(size_t n) {
        void *p = nullptr;
        FR_HIP(hipMalloc(&p, (n ? n : 1) * sizeof(T)));
        dev_.push_back(p);
        return (T *)p;
    }
    // pinned host memory; mapped: host-coherent and mapped into the device's address space (the blocks kernels write for the host)
    template <class T> T *alloc_pinned(size_t n, bool mapped = false) {
        void *p = nullptr;
        FR_HIP(hipHostMalloc(&p, (n ? n : 1) * sizeof(T), mapped ? hipHostMallocMapped | hipHostMallocCoherent : hipHostMallocDefault));
        host_.push_back(p);
        return (T *)p;
    }
    // frees p now (an array that is outgrown or switched off) and clears the caller's pointer; a null pointer is left alone
    template <class T> void release(T *&p) {
        if (!p) return;
        auto d = std::find(dev_.begin(), dev_.end(), (void *)p);
        if (d != dev_.end()) { dev_.erase(d); FR_HIP(hipFree((void *)p)); }
        else {
            auto h = std::find(host_.begin(), host_.end(), (void *)p);
            if (h == host_.end()) throw FriesError("DevMem::release: not an allocation of this owner");
            host_.erase(h); FR_HIP(hipHostFree((void *)p));
        }
        p = nullptr;
    }
};
