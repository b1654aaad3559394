// One pass of the stable LSD radix sort on 32-bit keys with a 32-bit payload, 8-bit digits: the bodies of the three kernels of a pass.
// The merge (vec.hip: k_rs_*, the length on the device) and fries_rdm2 (rdm2.hip: k_r2_*, the length by value) wrap them in kernels
// of their own.  A tile is RS_TILE consecutive keys and one workgroup of FR_BLOCK threads; hist is [256][stride] counts, digit-major,
// followed by the 256 digit totals at hist[256 * stride], with stride >= the number of tiles.
#pragma once
#include "fries_dev.hpp"

#define RS_TILE 1024            // keys per workgroup: every wave owns 256 consecutive keys
static_assert(FR_BLOCK == 256 && RS_TILE == 4 * FR_BLOCK, "one thread per digit; four waves of 256 keys");

// histogram of tile blockIdx.x
__device__ __forceinline__ void fr_rs_hist_tile(const uint32_t *key, uint32_t n, uint32_t *hist, int shift, uint32_t stride) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    size_t base = (size_t)blockIdx.x * RS_TILE;
    for (int it = 0; it < RS_TILE / FR_BLOCK; it++) {
        size_t j = base + it * FR_BLOCK + threadIdx.x;
        if (j < n) atomicAdd(&h[(key[j] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * stride + blockIdx.x] = h[threadIdx.x];
}

// digit blockIdx.x: exclusive scan of its counts over the nblk tiles; total -> hist tail
__device__ __forceinline__ void fr_rs_scan_digit(uint32_t *hist, uint32_t nblk, uint32_t stride) {
    __shared__ uint32_t shu[4];
    uint32_t *row = hist + (size_t)blockIdx.x * stride;
    uint32_t carry = 0;
    for (unsigned b0 = 0; b0 < nblk; b0 += FR_BLOCK) {
        unsigned b = b0 + threadIdx.x;
        uint32_t x = b < nblk ? row[b] : 0, tot;
        uint32_t incl = fr_block_scan_u32(x, shu, &tot);
        if (b < nblk) row[b] = carry + incl - x;
        carry += tot;
    }
    if (threadIdx.x == 0) hist[(size_t)256 * stride + blockIdx.x] = carry;
}

// scatter of tile blockIdx.x.  The stores are not guarded by o < n: the n destinations of a pass are a permutation of [0, n) -- a
// digit's base is the number of keys with a smaller digit, the tile's offset the number with that digit in the tiles before, and the
// rank the number with it before the key in its tile, all three counted over the same n keys that the pass's histogram counted.
__device__ __forceinline__ void fr_rs_scatter_tile(const uint32_t *key, const uint32_t *pay, uint32_t *key_out, uint32_t *pay_out,
                                                   uint32_t n, const uint32_t *hist, int shift, uint32_t stride) {
    __shared__ uint32_t wcount[4][256];
    __shared__ uint32_t gbase[256];
    __shared__ uint32_t shu[4];
    const int lane = fr_lane(), w = threadIdx.x >> 6;
    for (int q = 0; q < 4; q++) wcount[q][threadIdx.x] = 0;
    {   // digit bases: exclusive scan of the 256 totals + this tile's offset within the digit
        uint32_t t = hist[(size_t)256 * stride + threadIdx.x], tot;
        uint32_t incl = fr_block_scan_u32(t, shu, &tot);
        gbase[threadIdx.x] = incl - t + hist[(size_t)threadIdx.x * stride + blockIdx.x];
    }
    __syncthreads();
    // each wave owns 256 consecutive keys, visited as 4 rounds of 64 consecutive keys
    size_t wbase = (size_t)blockIdx.x * RS_TILE + (size_t)w * 256;
    uint32_t kk[4], pp[4], rk[4];
    for (int r = 0; r < 4; r++) {
        size_t j = wbase + r * 64 + lane;
        bool ok = j < n;
        kk[r] = ok ? key[j] : 0xFFFFFFFFu; pp[r] = ok ? pay[j] : 0;
        uint32_t dg = (kk[r] >> shift) & 255u;
        unsigned long long m = __ballot(ok);
        for (int b = 0; b < 8; b++) {
            unsigned long long bal = __ballot((dg >> b) & 1u);
            m &= ((dg >> b) & 1u) ? bal : ~bal;
        }
        if (!ok) m = 0;
        uint32_t before = __popcll(m & ((1ull << lane) - 1ull));
        uint32_t prev = ok ? wcount[w][dg] : 0;
        rk[r] = prev + before;
        __builtin_amdgcn_wave_barrier();
        if (ok && before == 0) wcount[w][dg] = prev + (uint32_t)__popcll(m);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    // cross-wave exclusive prefix per digit (thread d handles digit d)
    {
        uint32_t a0 = wcount[0][threadIdx.x], a1 = wcount[1][threadIdx.x], a2 = wcount[2][threadIdx.x];
        __syncthreads();
        wcount[0][threadIdx.x] = 0; wcount[1][threadIdx.x] = a0; wcount[2][threadIdx.x] = a0 + a1; wcount[3][threadIdx.x] = a0 + a1 + a2;
    }
    __syncthreads();
    for (int r = 0; r < 4; r++) {
        size_t j = wbase + r * 64 + lane;
        if (j < n) {
            uint32_t dg = (kk[r] >> shift) & 255u;
            uint32_t o = gbase[dg] + wcount[w][dg] + rk[r];
            key_out[o] = kk[r]; pay_out[o] = pp[r];
        }
    }
}
