// Host check of fries_rdm2's chunk cutting and scratch layout (csrc/rdm2_plan.hpp), built with -fsanitize=address,undefined: for small
// geometries it replays what rdm2.hip does with the plan -- every wave writes its records at its offset inside its chunk, the sort
// ping-pongs between the two (key, index) blocks, the histograms are indexed by digit and tile, the pieces' sums land in the block the
// sort did not end in -- on arrays of exactly the planned size, so that any index past an array is reported.  No GPU, no library.
#include "../../fries_amd/csrc/rdm2_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

static int fail(const char *what, uint64_t a, uint64_t b) { std::printf("FAILED: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b); return 1; }

static int replay(uint32_t n_wg, uint32_t waves, uint64_t capacity, uint32_t max_per_wave, uint32_t n_orb, std::mt19937 &rng) {
    std::vector<uint64_t> wave_rec((size_t)n_wg * waves);
    for (uint64_t &x : wave_rec) x = rng() % 3 == 0 ? 0 : rng() % (max_per_wave + 1);
    const Rdm2Plan plan = fr_rdm2_cut(wave_rec.data(), n_wg, capacity, waves);
    uint64_t total = 0;
    for (uint64_t x : wave_rec) total += x;
    if (plan.bad_wg >= 0) {
        uint64_t tot = 0;
        for (uint32_t w = 0; w < waves; w++) tot += wave_rec[(size_t)plan.bad_wg * waves + w];
        if (tot <= capacity || tot != plan.bad_need) return fail("a workgroup was refused that fits", tot, capacity);
        return 0;
    }
    for (uint32_t g = 0; g < n_wg; g++) {
        uint64_t tot = 0;
        for (uint32_t w = 0; w < waves; w++) tot += wave_rec[(size_t)g * waves + w];
        if (tot > capacity) return fail("a workgroup that does not fit was not refused", tot, capacity);
    }
    if (plan.total_rec != total) return fail("total", plan.total_rec, total);
    // the chunks cover the workgroups in order; greedy: the next workgroup would not have fitted
    uint32_t next = 0; uint64_t seen = 0;
    for (size_t k = 0; k < plan.chunks.size(); k++) {
        const Rdm2Chunk &c = plan.chunks[k];
        if (c.wg_lo != next || c.wg_hi <= c.wg_lo || c.wg_hi > n_wg) return fail("chunk bounds", c.wg_lo, c.wg_hi);
        if (c.n_rec > capacity || c.n_rec > plan.max_rec) return fail("chunk records", c.n_rec, capacity);
        if (c.wg_hi < n_wg) {
            uint64_t tot = 0;
            for (uint32_t w = 0; w < waves; w++) tot += wave_rec[(size_t)c.wg_hi * waves + w];
            if (c.n_rec + tot <= capacity) return fail("a chunk was closed early", c.n_rec, tot);
        }
        next = c.wg_hi; seen += c.n_rec;
    }
    if (next != n_wg || seen != total) return fail("cover", next, seen);
    // the scratch, exactly as large as planned, written as the kernels write it
    const Rdm2Scratch sc = fr_rdm2_scratch(plan.max_rec);
    std::vector<uint8_t> mem(sc.bytes);
    if (sc.blk[1] < sc.blk[0] + 8 * plan.max_rec || sc.val < sc.blk[1] + 8 * plan.max_rec || sc.hist < sc.val + 8 * plan.max_rec) return fail("blocks overlap", sc.val, sc.hist);
    const int passes = fr_rdm2_passes(n_orb);
    const uint32_t n_bins = n_orb * n_orb * n_orb * n_orb;
    if (passes < 1 || passes > 3 || (passes < 4 && (1ull << (8 * passes)) < n_bins)) return fail("passes", (uint64_t)passes, n_bins);
    for (const Rdm2Chunk &c : plan.chunks) {
        if (!c.n_rec) continue;
        const uint32_t nr = (uint32_t)c.n_rec, nblk = (nr + R2_TILE - 1) / R2_TILE;
        if (nblk > sc.nblk) return fail("tiles", nblk, sc.nblk);
        uint32_t *key[2] = {(uint32_t *)(mem.data() + sc.key(0)), (uint32_t *)(mem.data() + sc.key(1))};
        uint32_t *pay[2] = {(uint32_t *)(mem.data() + sc.pay(0, plan.max_rec)), (uint32_t *)(mem.data() + sc.pay(1, plan.max_rec))};
        double *val = (double *)(mem.data() + sc.val);
        uint32_t *hist = (uint32_t *)(mem.data() + sc.hist);
        std::vector<uint8_t> hit(nr, 0);
        for (uint32_t g = c.wg_lo; g < c.wg_hi; g++)
            for (uint32_t w = 0; w < waves; w++) {
                const size_t wave = (size_t)g * waves + w;
                for (uint64_t k = 0; k < wave_rec[wave]; k++) {
                    const uint64_t o = plan.wave_off[wave] + k;
                    if (o >= nr) return fail("a record past its chunk", o, nr);
                    if (hit[o]++) return fail("two records in one place", o, wave);
                    key[0][o] = rng() % n_bins; pay[0][o] = (uint32_t)o; val[o] = 1.0;
                }
            }
        for (uint32_t o = 0; o < nr; o++) if (!hit[o]) return fail("a place without a record", o, nr);
        int src = 0;
        for (int p = 0; p < passes; p++, src ^= 1) {
            for (uint32_t d = 0; d < 256; d++) for (uint32_t t = 0; t < nblk; t++) hist[(size_t)d * nblk + t] = 0;
            for (uint32_t d = 0; d < 256; d++) hist[(size_t)256 * nblk + d] = 0;
            std::memcpy(key[src ^ 1], key[src], 4 * (size_t)nr);
            std::memcpy(pay[src ^ 1], pay[src], 4 * (size_t)nr);
        }
        double *psum = (double *)(mem.data() + sc.blk[src ^ 1]);
        for (uint32_t o = 0; o < nr; o++) psum[o] = val[pay[src][o]];
    }
    return 0;
}

int main() {
    std::mt19937 rng(20251021);
    int bad = 0, n = 0;
    for (uint32_t n_wg : {1u, 2u, 3u, 7u, 33u})
        for (uint32_t waves : {1u, 4u})
            for (uint64_t capacity : {1ull, 5ull, 64ull, 1000ull, 5000ull})
                for (uint32_t max_per_wave : {0u, 1u, 3u, 40u, 1500u})
                    for (uint32_t n_orb : {1u, 2u, 4u, 5u, 16u}) { bad += replay(n_wg, waves, capacity, max_per_wave, n_orb, rng); n++; }
    // three chunks with a partial last one, by hand: workgroups of 6, 5, 4, 4, 3 records at capacity 9 -> {6}, {5, 4}, {4, 3}
    {
        const uint64_t rec[5] = {6, 5, 4, 4, 3};
        const Rdm2Plan p = fr_rdm2_cut(rec, 5, 9, 1);
        if (p.chunks.size() != 3 || p.chunks[0].n_rec != 6 || p.chunks[1].n_rec != 9 || p.chunks[2].n_rec != 7 || p.max_rec != 9 || p.wave_off[2] != 5 || p.wave_off[4] != 4)
            bad += fail("the hand-made cut", p.chunks.size(), p.max_rec);
        const Rdm2Plan q = fr_rdm2_cut(rec, 5, 5, 1);
        if (q.bad_wg != 0 || q.bad_need != 6) bad += fail("the hand-made refusal", (uint64_t)q.bad_wg, q.bad_need);
    }
    if (fr_rdm2_passes(4) != 1 || fr_rdm2_passes(5) != 2 || fr_rdm2_passes(16) != 2 || fr_rdm2_passes(22) != 3 || fr_rdm2_passes(32) != 3) bad += fail("passes by hand", 0, 0);
    std::printf("%d geometries, %d failures\n", n, bad);
    return bad ? 1 : 0;
}
