// Host check of the snapshot's layout (csrc/snapshot_plan.hpp), built with -fsanitize=address,undefined: for small geometries it replays
// what snapshot.hip does with the plan -- every shard counts its tiles, scans the counts, writes its compacted lists into its staging;
// the lists are copied behind each other into the snapshot's allocation; every entry is inserted into the table by linear probing and
// found again -- on arrays of exactly the planned size, so that any index past an array is reported.  No GPU, no library.
#include "../../fries_amd/csrc/snapshot_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

static int fail(const char *what, uint64_t a, uint64_t b) { std::printf("FAILED: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b); return 1; }

struct Slot { uint64_t key; uint32_t val, pad; };
static_assert(sizeof(Slot) == 16, "a slot is 16 bytes");
static uint32_t slot_of(uint64_t d, uint32_t slots) { d ^= d >> 33; d *= 0xff51afd7ed558ccdull; d ^= d >> 33; return (uint32_t)d & (slots - 1); }     // (any mixer: the layout is under test)

// live[k][i]: position i of shard k holds a non-zero value
static int replay(const std::vector<std::vector<uint8_t>> &live) {
    const uint32_t P = (uint32_t)live.size();
    std::vector<uint32_t> n_pos(P);
    for (uint32_t k = 0; k < P; k++) n_pos[k] = (uint32_t)live[k].size();
    const SnapPlan plan = fr_snap_plan(n_pos.data(), P);
    if (plan.too_many) return fail("a small geometry was refused", plan.n_bound, 0);
    if (plan.slots < SNAP_MIN_SLOTS || (plan.slots & (plan.slots - 1))) return fail("slot count", plan.slots, 0);
    if ((uint64_t)plan.slots * SNAP_FILL_PCT < plan.n_bound * 100u) return fail("more than 40 % full", plan.slots, plan.n_bound);
    if (plan.slots > SNAP_MIN_SLOTS && (uint64_t)(plan.slots / 2) * SNAP_FILL_PCT >= plan.n_bound * 100u) return fail("twice the slots needed", plan.slots, plan.n_bound);
    if (plan.val < plan.det + 8 * plan.n_bound || plan.hs < plan.val + 8 * plan.n_bound || plan.err < plan.hs + 16 * (size_t)plan.slots || plan.bytes < plan.err + 4) return fail("blocks overlap", plan.hs, plan.err);
    if (plan.hs % 16) return fail("the table is not 16-byte aligned", plan.hs, 0);
    std::vector<uint8_t> mem(plan.bytes);
    uint64_t *dets = (uint64_t *)(mem.data() + plan.det);
    double *vals = (double *)(mem.data() + plan.val);
    Slot *hs = (Slot *)(mem.data() + plan.hs);
    uint32_t *err = (uint32_t *)(mem.data() + plan.err);
    // 1. every shard's compaction into its own staging
    std::vector<std::vector<uint8_t>> stage(P);
    std::vector<uint32_t> n_live(P, 0);
    for (uint32_t k = 0; k < P; k++) {
        const SnapStage &g = plan.stage[k];
        if (g.n_pos != n_pos[k] || (uint64_t)g.n_tiles * SNAP_TILE < n_pos[k] || (g.n_tiles && (uint64_t)(g.n_tiles - 1) * SNAP_TILE >= n_pos[k])) return fail("tiles", g.n_tiles, n_pos[k]);
        if (plan.bound_off[k + 1] != plan.bound_off[k] + n_pos[k]) return fail("bound offsets", k, plan.bound_off[k + 1]);
        if (!n_pos[k]) continue;        // an empty shard launches nothing and has no staging
        if (g.val < g.det + 8 * (size_t)n_pos[k] || g.tile_cnt < g.val + 8 * (size_t)n_pos[k] || g.tile_off < g.tile_cnt + 4 * (size_t)g.n_tiles || g.n_live < g.tile_off + 4 * (size_t)g.n_tiles || g.bytes < g.n_live + 4)
            return fail("staging blocks overlap", k, g.bytes);
        stage[k].assign(g.bytes, 0);
        uint8_t *b = stage[k].data();
        uint64_t *sd = (uint64_t *)(b + g.det); double *sv = (double *)(b + g.val);
        uint32_t *cnt = (uint32_t *)(b + g.tile_cnt), *off = (uint32_t *)(b + g.tile_off), *nl = (uint32_t *)(b + g.n_live);
        for (uint32_t t = 0; t < g.n_tiles; t++) {
            cnt[t] = 0;
            for (uint64_t i = (uint64_t)t * SNAP_TILE; i < (uint64_t)(t + 1) * SNAP_TILE && i < n_pos[k]; i++) cnt[t] += live[k][i];
        }
        uint32_t base = 0;
        for (uint32_t t = 0; t < g.n_tiles; t++) { off[t] = base; base += cnt[t]; }
        *nl = base;
        for (uint32_t t = 0; t < g.n_tiles; t++) {
            uint32_t o = off[t];
            for (uint64_t i = (uint64_t)t * SNAP_TILE; i < (uint64_t)(t + 1) * SNAP_TILE && i < n_pos[k]; i++)
                if (live[k][i]) { sd[o] = ((uint64_t)(k + 1) << 40) | (i + 1); sv[o] = (double)(i + 1); o++; }
        }
        n_live[k] = *nl;
    }
    // 2. the lists behind each other
    const std::vector<uint64_t> off = fr_snap_concat(n_live.data(), P);
    const uint64_t n = off[P];
    if (n > plan.n_bound) return fail("more entries than planned", n, plan.n_bound);
    for (uint32_t k = 0; k < P; k++) {
        if (off[k] > plan.bound_off[k]) return fail("a list starts past its bound", off[k], plan.bound_off[k]);
        if (!n_live[k]) continue;
        std::memcpy(dets + off[k], stage[k].data() + plan.stage[k].det, 8 * (size_t)n_live[k]);
        std::memcpy(vals + off[k], stage[k].data() + plan.stage[k].val, 8 * (size_t)n_live[k]);
    }
    // rank-major, position order
    uint64_t j = 0;
    for (uint32_t k = 0; k < P; k++)
        for (uint64_t i = 0; i < n_pos[k]; i++)
            if (live[k][i]) { if (dets[j] != (((uint64_t)(k + 1) << 40) | (i + 1)) || vals[j] != (double)(i + 1)) return fail("order", j, i); j++; }
    if (j != n) return fail("count", j, n);
    // 3. the table
    *err = 0;
    for (uint32_t s = 0; s < plan.slots; s++) hs[s] = Slot{0, 0xFFFFFFFFu, 0};
    for (uint64_t i = 0; i < n; i++) {
        uint32_t s = slot_of(dets[i], plan.slots), probe = 0;
        for (; probe < plan.slots; probe++, s = (s + 1) & (plan.slots - 1)) {
            if (hs[s].key == 0) { hs[s].key = dets[i]; hs[s].val = (uint32_t)i; break; }
            if (hs[s].key == dets[i]) { *err |= 1; break; }
        }
        if (probe == plan.slots) *err |= 2;
    }
    if (*err) return fail("insert", *err, n);
    for (uint64_t i = 0; i < n; i++) {
        uint32_t s = slot_of(dets[i], plan.slots);
        while (hs[s].key != dets[i]) { if (hs[s].key == 0) return fail("an entry is not found", i, s); s = (s + 1) & (plan.slots - 1); }
        if (hs[s].val != i || vals[hs[s].val] != vals[i]) return fail("an entry's position", i, hs[s].val);
    }
    return 0;
}

static std::vector<uint8_t> shard(uint32_t n_pos, uint32_t pct_live, std::mt19937 &rng) {
    std::vector<uint8_t> v(n_pos);
    for (uint8_t &x : v) x = rng() % 100 < pct_live;
    return v;
}

int main() {
    std::mt19937 rng(20261021);
    int bad = 0, n = 0;
    // one entry; one entry among three shards of which two are empty
    bad += replay({{1}}); n++;
    bad += replay({{}, {1}, {}}); n++;
    bad += replay({{}}); n++;
    // an empty shard between full ones; a shard of zeros only
    bad += replay({shard(3000, 100, rng), {}, shard(2500, 100, rng)}); n++;
    bad += replay({shard(1500, 60, rng), shard(700, 0, rng), shard(1025, 60, rng)}); n++;
    // counts that cross a slot-count doubling: 6553 positions fill 2^14 slots to 40 %, 6554 need 2^15; and the next doubling
    for (uint32_t tot : {6553u, 6554u, 13107u, 13108u, 26215u}) {
        bad += replay({shard(tot, 100, rng)}); n++;
        bad += replay({shard(tot / 2, 90, rng), shard(tot - tot / 2, 100, rng)}); n++;
    }
    if (fr_snap_slots(0) != (1u << 14) || fr_snap_slots(6553) != (1u << 14) || fr_snap_slots(6554) != (1u << 15) || fr_snap_slots(13107) != (1u << 15) || fr_snap_slots(13108) != (1u << 16))
        bad += fail("slots by hand", fr_snap_slots(6553), fr_snap_slots(6554));
    if (fr_snap_slots(858993459ull) != (1u << 31) || fr_snap_slots(858993460ull) != 0) bad += fail("the largest table", fr_snap_slots(858993459ull), fr_snap_slots(858993460ull));
    // another fill (FRIES_HASH_FILL, as the vector's own table reads it): 20 % halves what a table holds
    if (fr_snap_slots(3276, 20) != (1u << 14) || fr_snap_slots(3277, 20) != (1u << 15) || fr_snap_slots(6553, 80) != (1u << 14) || fr_snap_slots(13108, 80) != (1u << 15))
        bad += fail("slots at another fill", fr_snap_slots(3277, 20), fr_snap_slots(13108, 80));
    {
        const uint32_t np20[2] = {2000u, 2000u};
        if (fr_snap_plan(np20, 2, 20).slots != (1u << 15) || fr_snap_plan(np20, 2).slots != (1u << 14)) bad += fail("the plan at another fill", 0, 0);
    }
    // tile edges and random geometries
    for (uint32_t P : {1u, 2u, 3u, 5u})
        for (uint32_t max_pos : {1u, 4u, 1023u, 1024u, 1025u, 5000u})
            for (uint32_t pct : {0u, 10u, 70u, 100u}) {
                std::vector<std::vector<uint8_t>> live;
                for (uint32_t k = 0; k < P; k++) live.push_back(shard(rng() % 3 == 0 ? max_pos : rng() % (max_pos + 1), pct, rng));
                bad += replay(live); n++;
            }
    // refusals: more positions than a 32-bit position names
    {
        const uint32_t big[2] = {0xFFFFFFFFu, 16u};
        if (!fr_snap_plan(big, 2).too_many) bad += fail("too many positions were planned", 0, 0);
        const uint32_t huge[1] = {900000000u};
        if (!fr_snap_plan(huge, 1).too_many) bad += fail("a table above 2^31 slots was planned", 0, 0);
    }
    std::printf("%d geometries, %d failures\n", n, bad);
    return bad ? 1 : 0;
}
