// Host check of fries_vec_axpy_snapshot's and fries_snapshot_dot's geometry (csrc/axpy_plan.hpp), built with -fsanitize=address,undefined:
// it replays what snapshot.hip does with the plan -- the snapshot's list is cut into chunks of at most the spawn capacity; per chunk
// the ownership filter counts the taken entries of every tile, scans the counts and writes the taken entries into the staged spawn list
// -- on arrays of exactly the planned sizes, so that any index past an array is reported.  No GPU, no library.
#include "../../fries_amd/csrc/axpy_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <random>

static int fail(const char *what, uint64_t a, uint64_t b) { std::printf("FAILED: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b); return 1; }

// owner[i]: the rank that owns entry i; val[i] * coeff == 0 drops the entry.  -> what rank `rank` stages and "merges", checked against
// the plain filter of the whole list
static int replay(const std::vector<uint32_t> &owner, const std::vector<double> &val, double coeff, uint32_t rank, uint32_t cap) {
    const uint64_t n = owner.size();
    const AxpyPlan plan = fr_axpy_plan(n, cap);
    if (plan.refused) return fail("a small geometry was refused", n, cap);
    if (n == 0) return plan.chunk.empty() && plan.max_n == 0 && plan.max_tiles == 0 ? 0 : fail("chunks of nothing", plan.chunk.size(), 0);
    // the cuts: in list order, without gaps, none above the capacity, all but the last full
    uint64_t at = 0;
    for (size_t k = 0; k < plan.chunk.size(); k++) {
        const AxpyChunk &c = plan.chunk[k];
        if (c.off != at || c.n == 0 || c.n > cap || (k + 1 < plan.chunk.size() && c.n != cap)) return fail("chunk cut", c.off, c.n);
        if ((uint64_t)c.n_tiles * AXPY_TILE < c.n || (uint64_t)(c.n_tiles - 1) * AXPY_TILE >= c.n) return fail("tiles", c.n_tiles, c.n);
        if (c.n > plan.max_n || c.n_tiles > plan.max_tiles || c.n_tiles > AXPY_MAX_TILES || c.n_tiles > c.n) return fail("maxima", c.n, c.n_tiles);
        at += c.n;
    }
    if (at != n || plan.chunk.size() != (n + cap - 1) / cap) return fail("the chunks do not cover the list", at, n);
    if (plan.max_n > cap) return fail("a chunk above the capacity", plan.max_n, cap);
    // the arrays the kernels are given: the spawn list of the largest chunk, the tiles' counts and offsets
    std::vector<uint64_t> sp_det(plan.max_n);
    std::vector<double> sp_val(plan.max_n);
    std::vector<uint8_t> sp_ini(plan.max_n);
    std::vector<uint32_t> tile_cnt(plan.max_tiles), tile_off(plan.max_tiles);
    auto taken = [&](uint64_t i) { return coeff * val[i] != 0 && owner[i] == rank; };
    std::vector<uint64_t> merged;       // the entries in the order they reach the merges
    for (const AxpyChunk &c : plan.chunk) {
        for (uint32_t t = 0; t < c.n_tiles; t++) {         // k_axpy_count
            tile_cnt[t] = 0;
            for (uint64_t i = (uint64_t)t * AXPY_TILE; i < (uint64_t)(t + 1) * AXPY_TILE && i < c.n; i++) tile_cnt[t] += taken(c.off + i);
        }
        uint32_t base = 0;                                  // k_snap_scan
        for (uint32_t t = 0; t < c.n_tiles; t++) { tile_off[t] = base; base += tile_cnt[t]; }
        const uint32_t n_spawn = base;
        if (n_spawn > c.n) return fail("more spawns than entries", n_spawn, c.n);
        for (uint32_t t = 0; t < c.n_tiles; t++) {         // k_axpy_write
            uint32_t o = tile_off[t];
            for (uint64_t i = (uint64_t)t * AXPY_TILE; i < (uint64_t)(t + 1) * AXPY_TILE && i < c.n; i++)
                if (taken(c.off + i) && o < c.n) { sp_det[o] = c.off + i; sp_val[o] = coeff * val[c.off + i]; sp_ini[o] = 1; o++; }
        }
        for (uint32_t j = 0; j < n_spawn; j++) {
            if (sp_val[j] == 0 || sp_ini[j] != 1) return fail("a staged entry", c.off, j);
            merged.push_back(sp_det[j]);
        }
    }
    // stable: exactly the taken entries, in list order
    size_t j = 0;
    for (uint64_t i = 0; i < n; i++)
        if (taken(i)) { if (j >= merged.size() || merged[j] != i) return fail("order", i, j); j++; }
    if (j != merged.size()) return fail("count", j, merged.size());
    return 0;
}

static int dot_plan(uint32_t n_pos) {
    const VdotPlan p = fr_vdot_plan(n_pos);
    if ((uint64_t)p.n_tiles * AXPY_TILE < n_pos || (p.n_tiles && (uint64_t)(p.n_tiles - 1) * AXPY_TILE >= n_pos)) return fail("dot tiles", p.n_tiles, n_pos);
    if (p.abs_sum < p.dot + 8 * (size_t)p.n_tiles || p.n_src < p.abs_sum + 8 * (size_t)p.n_tiles || p.n_hits < p.n_src + 4 * (size_t)p.n_tiles || p.bytes < p.n_hits + 4 * (size_t)p.n_tiles)
        return fail("dot blocks overlap", p.n_hits, p.bytes);
    if (p.abs_sum % 8 || p.n_src % 4 || p.n_hits % 4) return fail("dot alignment", p.abs_sum, p.n_src);
    std::vector<uint8_t> mem(p.bytes);
    double *d = (double *)(mem.data() + p.dot), *a = (double *)(mem.data() + p.abs_sum);
    uint32_t *s = (uint32_t *)(mem.data() + p.n_src), *h = (uint32_t *)(mem.data() + p.n_hits);
    for (uint32_t t = 0; t < p.n_tiles; t++) { d[t] = 1; a[t] = 1; s[t] = 1; h[t] = 1; }
    return 0;
}

int main() {
    std::mt19937 rng(20261021);
    int bad = 0, n = 0;
    auto lists = [&](uint64_t len, uint32_t n_ranks, uint32_t pct_zero, std::vector<uint32_t> &owner, std::vector<double> &val) {
        owner.resize(len); val.resize(len);
        for (uint64_t i = 0; i < len; i++) { owner[i] = rng() % n_ranks; val[i] = rng() % 100 < pct_zero ? 0.0 : 1.0 + (double)(rng() % 1000); }
    };
    std::vector<uint32_t> owner; std::vector<double> val;
    const uint32_t cap = 5096;          // mat_nonz = 1000: the capacity of tests/test_gpu_subspace_ops.py::test_axpy_in_chunks
    // 0 entries, 1 entry, a tile edge, the capacity exactly, the capacity plus one, several chunks
    for (uint64_t len : {0ull, 1ull, 1023ull, 1024ull, 1025ull, (unsigned long long)cap - 1, (unsigned long long)cap, (unsigned long long)cap + 1, 2ull * cap, 2ull * cap + 1, 3ull * cap + 1025})
        for (uint32_t P : {1u, 2u, 3u})
            for (uint32_t pct : {0u, 30u, 100u}) {
                lists(len, P, pct, owner, val);
                for (uint32_t r = 0; r < P; r++) { bad += replay(owner, val, -0.37, r, cap); n++; }
                // a rank that owns nothing
                bad += replay(owner, val, -0.37, P, cap); n++;
            }
    // capacities at and around a tile, and of one entry
    for (uint32_t c : {1u, 2u, 1023u, 1024u, 1025u, 2048u})
        for (uint64_t len : {1ull, 1024ull, 1025ull, 4097ull}) {
            lists(len, 2, 20, owner, val);
            bad += replay(owner, val, 1.0, 0, c); n++;
        }
    // every product zero: the smallest subnormal times values of at most 1/2
    lists(3000, 1, 0, owner, val);
    for (double &x : val) x = 0.5 / x;
    bad += replay(owner, val, 4.9406564584124654e-324, 0, cap); n++;
    // refusals: no capacity; more tiles per chunk than the count array holds
    if (!fr_axpy_plan(5, 0).refused) bad += fail("a plan without capacity", 0, 0);
    if (fr_axpy_plan(5, AXPY_MAX_TILES * AXPY_TILE).refused || !fr_axpy_plan(5, AXPY_MAX_TILES * AXPY_TILE + 1).refused) bad += fail("the largest capacity", 0, 0);
    if (fr_axpy_plan(0, 0).refused) bad += fail("an empty snapshot needs no capacity", 0, 0);
    for (uint32_t n_pos : {0u, 1u, 1023u, 1024u, 1025u, 70000u, 1000000u}) { bad += dot_plan(n_pos); n++; }
    std::printf("%d geometries, %d failures\n", n, bad);
    return bad ? 1 : 0;
}
