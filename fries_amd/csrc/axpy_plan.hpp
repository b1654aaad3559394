// Host-only geometry of fries_vec_axpy_snapshot and fries_snapshot_dot (snapshot.hip): how a snapshot's entry list is cut into chunks of
// at most the spawn capacity, how many tiles of AXPY_TILE entries each chunk's ownership filter (count / scan / write) runs over, and what
// every array of a chunk must hold.  Everything follows from the snapshot's entry count and the context's spawn capacity, so the sizes
// are known before anything is launched.  No HIP in here, so that a plain C++ program can check it (tests/cpp/axpy_plan_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#define AXPY_TILE 1024                  // entries (positions) per workgroup: 256 threads, 4 contiguous ones each -- SNAP_TILE's shape
#define AXPY_MAX_TILES 131072u          // tiles of one chunk: what the spawn buffers' block-count array holds (FR_MAX_PART)

static inline uint32_t fr_axpy_tiles(uint64_t n) { return (uint32_t)((n + AXPY_TILE - 1) / AXPY_TILE); }

// one chunk: entries [off, off + n) of the snapshot's list, filtered over n_tiles tiles into at most n spawns
struct AxpyChunk {
    uint64_t off = 0;
    uint32_t n = 0, n_tiles = 0;
};
struct AxpyPlan {
    std::vector<AxpyChunk> chunk;       // in list order; none for an empty snapshot
    uint32_t max_n = 0;                 // the largest chunk: <= the spawn capacity, what the staged list (det, val, ini) must hold
    uint32_t max_tiles = 0;             // ... and what the tiles' counts and offsets must hold
    bool refused = false;               // no capacity at all, or more tiles per chunk than the count array holds
};

static inline AxpyPlan fr_axpy_plan(uint64_t n_entries, uint32_t cap) {
    AxpyPlan p;
    if (n_entries == 0) return p;
    if (cap == 0 || fr_axpy_tiles(cap) > AXPY_MAX_TILES) { p.refused = true; return p; }
    for (uint64_t off = 0; off < n_entries; off += cap) {
        AxpyChunk k;
        k.off = off;
        k.n = (uint32_t)(n_entries - off < cap ? n_entries - off : cap);
        k.n_tiles = fr_axpy_tiles(k.n);
        if (k.n > p.max_n) p.max_n = k.n;
        if (k.n_tiles > p.max_tiles) p.max_tiles = k.n_tiles;
        p.chunk.push_back(k);
    }
    return p;
}

// fries_snapshot_dot: one shard's partials, as byte offsets into one allocation -- per tile of AXPY_TILE positions the sum of the
// products, of their magnitudes, and the counts of sources and hits
struct VdotPlan {
    uint32_t n_tiles = 0;
    size_t dot = 0, abs_sum = 0, n_src = 0, n_hits = 0, bytes = 0;
};
static inline VdotPlan fr_vdot_plan(uint32_t n_pos) {
    VdotPlan p;
    p.n_tiles = fr_axpy_tiles(n_pos);
    const size_t d = (8 * (size_t)p.n_tiles + 255) & ~(size_t)255, u = (4 * (size_t)p.n_tiles + 255) & ~(size_t)255;
    p.dot = 0; p.abs_sum = d; p.n_src = 2 * d; p.n_hits = 2 * d + u;
    p.bytes = 2 * d + 2 * u;
    return p;
}
