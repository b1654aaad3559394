// Host-only geometry of fries_rdm2's scratch (rdm2.hip): how the positions are cut into chunks whose bin records fit a fixed capacity,
// where every wave's records start inside its chunk, and how the scratch of the largest chunk is laid out.  No HIP in here, so that a
// plain C++ program can check it (tests/cpp/rdm2_plan_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#define R2_WPOS 8                   // positions one wave walks (a source has thousands of candidates: the wave's 64 lanes share each source)
#define R2_WAVES 4                  // waves per workgroup
#define R2_BPOS (R2_WAVES * R2_WPOS)    // positions per workgroup: the smallest chunk
#define R2_NCNT 4                   // counters of every wave: n_src, n_terms, n_hits, records
#define R2_NSCAL 2                  // doubles of every wave: ovlp, abs_sum
#define R2_TILE 1024                // records per workgroup of the radix sort
#define R2_PIECE 512                // a bin's records are added in pieces that end at multiples of this (of the sorted index), the pieces then in order
// capacity of a chunk in records (FRIES_RDM2_RECORDS; 24 bytes each).  A tuning value: on the N2 shape at m = 1e6 (6.4e8 records) a call takes
// 1289 / 937 / 968 ms at 2^22 / 2^25 / 2^28 -- small chunks starve the emitting pass, large ones lengthen the bins' gathers (profiles/rdm2_cost.txt)
#define R2_DEFAULT_RECORDS (1ull << 25)
#define R2_MAX_RECORDS ((1ull << 31) - 1)   // offsets inside a chunk are 32-bit

struct Rdm2Chunk { uint32_t wg_lo, wg_hi; uint64_t n_rec; };       // workgroups [wg_lo, wg_hi)

struct Rdm2Plan {
    std::vector<Rdm2Chunk> chunks;      // cover [0, n_wg) in order, none empty of workgroups; n_rec <= capacity
    std::vector<uint32_t> wave_off;     // per wave: where its records start inside its chunk
    uint64_t max_rec = 0, total_rec = 0;
    int64_t bad_wg = -1;                // a workgroup whose own records exceed the capacity (the call is refused)
    uint64_t bad_need = 0;
};

// wave_rec[n_wg * R2_WAVES]: records every wave will write.  Greedy: a chunk takes workgroups while their records fit.
static inline Rdm2Plan fr_rdm2_cut(const uint64_t *wave_rec, uint32_t n_wg, uint64_t capacity, uint32_t waves = R2_WAVES) {
    Rdm2Plan p;
    p.wave_off.assign((size_t)n_wg * waves, 0u);
    Rdm2Chunk cur{0, 0, 0};
    for (uint32_t g = 0; g < n_wg; g++) {
        uint64_t tot = 0;
        for (uint32_t w = 0; w < waves; w++) tot += wave_rec[(size_t)g * waves + w];
        if (tot > capacity) { if (p.bad_wg < 0) { p.bad_wg = g; p.bad_need = tot; } continue; }
        if (cur.n_rec + tot > capacity) { cur.wg_hi = g; p.chunks.push_back(cur); cur = Rdm2Chunk{g, g, 0}; }
        for (uint32_t w = 0; w < waves; w++) {
            p.wave_off[(size_t)g * waves + w] = (uint32_t)cur.n_rec;
            cur.n_rec += wave_rec[(size_t)g * waves + w];
        }
        p.total_rec += tot;
    }
    cur.wg_hi = n_wg;
    if (cur.wg_hi > cur.wg_lo) p.chunks.push_back(cur);
    for (const Rdm2Chunk &c : p.chunks) if (c.n_rec > p.max_rec) p.max_rec = c.n_rec;
    return p;
}

// The scratch of one chunk of at most n_rec records, as byte offsets into one allocation: two (key, index) blocks the sort ping-pongs
// between -- the one it does not end in holds the pieces' sums afterwards, 8 bytes per record either way --, the values, the histograms.
struct Rdm2Scratch {
    size_t blk[2], val, hist, bytes;
    uint32_t nblk;                      // tiles of the sort at n_rec
    size_t key(int s) const { return blk[s]; }
    size_t pay(int s, uint64_t n_rec) const { return blk[s] + 4 * (size_t)n_rec; }
};
static inline Rdm2Scratch fr_rdm2_scratch(uint64_t n_rec) {
    Rdm2Scratch s;
    const size_t n = (size_t)(n_rec ? n_rec : 1);
    const size_t blk = (8 * n + 255) & ~(size_t)255;
    s.blk[0] = 0; s.blk[1] = blk; s.val = 2 * blk;
    s.hist = s.val + blk;
    s.nblk = (uint32_t)((n + R2_TILE - 1) / R2_TILE);
    s.bytes = s.hist + ((((size_t)256 * s.nblk + 256) * 4 + 255) & ~(size_t)255);
    return s;
}

// 8-bit passes of the sort over bins < n_orb^4
static inline int fr_rdm2_passes(uint32_t n_orb) {
    const uint64_t n4 = (uint64_t)n_orb * n_orb * n_orb * n_orb;
    int bits = 1;
    while ((1ull << bits) < n4) bits++;
    return (bits + 7) / 8;
}
