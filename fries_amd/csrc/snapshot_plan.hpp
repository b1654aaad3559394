// Host-only geometry of a vector snapshot (snapshot.hip): where every shard's compacted (determinant, value) list may start in the
// concatenation, how many hash slots the table gets, and how the snapshot's one allocation and every shard's staging are laid out.
// Everything follows from the shards' curr_size -- an upper bound of their live entries --, so the sizes are known, and checked against
// the free device memory, before anything is allocated or launched.  No HIP in here, so that a plain C++ program can check it
// (tests/cpp/snapshot_plan_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#define SNAP_TILE 1024                  // positions per workgroup of the compaction: 256 threads, 4 contiguous positions each
#define SNAP_MIN_SLOTS (1u << 14)       // as the vector's own table (vec.hip hash_slots_for)
#define SNAP_MAX_SLOTS (1u << 31)       // hcap is 32-bit and a power of two
#define SNAP_FILL_PCT 40                // percent of the slots the entries may take, unless the caller passes what FRIES_HASH_FILL says (as vec.hip reads it)
#define SNAP_MAX_ENTRIES 0xFFFFFFFEull  // a slot holds a 32-bit position; FR_NOPOS is not one

static inline size_t fr_snap_round(size_t b) { return (b + 255) & ~(size_t)255; }

// hash_slots_for's rule: the smallest power of two >= 2^14 of which n_entries fill at most `fill` per cent (40 unless FRIES_HASH_FILL says otherwise); 0 = no such table
static inline uint32_t fr_snap_slots(uint64_t n_entries, int fill = SNAP_FILL_PCT) {
    uint64_t want = SNAP_MIN_SLOTS;
    while (want * (uint64_t)fill < n_entries * 100u) {
        if (want >= SNAP_MAX_SLOTS) return 0;
        want <<= 1;
    }
    return (uint32_t)want;
}

// one shard's staging on its own device, as byte offsets into one allocation: the compacted lists (at most n_pos entries), the tiles'
// counts and offsets, the list's length
struct SnapStage {
    uint32_t n_pos = 0, n_tiles = 0;
    size_t det = 0, val = 0, tile_cnt = 0, tile_off = 0, n_live = 0, bytes = 0;
};

struct SnapPlan {
    std::vector<uint64_t> bound_off;    // [n_shards + 1]: prefix sums of curr_size; shard k's entries start at or before bound_off[k]
    std::vector<SnapStage> stage;       // per shard
    uint64_t n_bound = 0;               // = bound_off[n_shards]: the most entries the snapshot can hold
    uint32_t slots = 0;                 // hash slots for n_bound entries
    size_t det = 0, val = 0, hs = 0, err = 0, bytes = 0;       // the snapshot's allocation on its device
    bool too_many = false;              // more than SNAP_MAX_ENTRIES positions, or no table of <= SNAP_MAX_SLOTS slots holds them at 40 % (the call is refused)
};

static inline SnapPlan fr_snap_plan(const uint32_t *n_pos, uint32_t n_shards, int fill = SNAP_FILL_PCT) {
    SnapPlan p;
    p.bound_off.assign((size_t)n_shards + 1, 0);
    p.stage.resize(n_shards);
    for (uint32_t k = 0; k < n_shards; k++) {
        p.bound_off[k + 1] = p.bound_off[k] + n_pos[k];
        SnapStage &s = p.stage[k];
        s.n_pos = n_pos[k];
        s.n_tiles = (uint32_t)(((uint64_t)n_pos[k] + SNAP_TILE - 1) / SNAP_TILE);
        const size_t list = fr_snap_round(8 * (size_t)n_pos[k]), tiles = fr_snap_round(4 * (size_t)s.n_tiles);
        s.det = 0; s.val = list; s.tile_cnt = 2 * list; s.tile_off = s.tile_cnt + tiles; s.n_live = s.tile_off + tiles;
        s.bytes = s.n_live + 256;
    }
    p.n_bound = p.bound_off[n_shards];
    p.slots = fr_snap_slots(p.n_bound, fill);
    if (p.n_bound > SNAP_MAX_ENTRIES || p.slots == 0) { p.too_many = true; return p; }
    const size_t list = fr_snap_round(8 * (size_t)p.n_bound);
    p.det = 0; p.val = list; p.hs = 2 * list;
    p.err = p.hs + 16 * (size_t)p.slots;
    p.bytes = p.err + 256;
    return p;
}

// where the lists really start once the shards' live counts are known: rank order, no gaps.  -> [n_shards + 1]; the last is the number of entries
static inline std::vector<uint64_t> fr_snap_concat(const uint32_t *n_live, uint32_t n_shards) {
    std::vector<uint64_t> off((size_t)n_shards + 1, 0);
    for (uint32_t k = 0; k < n_shards; k++) off[k + 1] = off[k] + n_live[k];
    return off;
}
