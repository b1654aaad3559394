// Host-only check of fries_rdm1's scratch geometry (fries_amd/csrc/rdm1_plan.hpp), no GPU and no HIP:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o rdm1_plan_check tests/cpp/rdm1_plan_check.cpp && ./rdm1_plan_check
// It replays the host loop of fr_rdm1 (rdm1.hip) on a heap array of exactly the planned size: every row a level writes and reads must
// lie inside it (the sanitizer sees any that does not), every level's input must be the previous level's output, every position must
// be covered once, and the last row must be the single row of the last level.
#include "../../fries_amd/csrc/rdm1_plan.hpp"
#include <cstdio>
#include <cstdlib>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

// the fold on row indices: row r of level 0 "holds" the number of positions its workgroup covers; the sums must add up to n_pos
static void walk(uint32_t n_pos, uint32_t n_orb, uint32_t bpos, uint32_t fan) {
    const Rdm1Plan p = fr_rdm1_plan(n_pos, n_orb, bpos, fan);
    CHECK(p.stride == (size_t)n_orb * n_orb + RD_NSCAL);
    CHECK(!p.rows.empty() && p.rows.back() == 1);
    CHECK(p.rows[0] == (n_pos + (uint64_t)bpos - 1) / bpos);
    size_t sum = 0;
    for (uint32_t r : p.rows) sum += r;
    CHECK(sum == p.total_rows && p.last_row() == p.total_rows - 1);
    CHECK(p.bytes() == p.total_rows * (p.stride * 8 + RD_NCNT * 8));
    std::vector<uint64_t> *rows = new std::vector<uint64_t>(p.total_rows, 0);       // one word per row stands for its stride doubles
    uint64_t *d = rows->data();
    for (uint32_t b = 0; b < p.rows[0]; b++) {      // k_rdm1: workgroup b covers positions [b * bpos, (b + 1) * bpos) below n_pos
        const uint64_t lo = (uint64_t)b * bpos, hi = lo + bpos < n_pos ? lo + bpos : n_pos;
        CHECK(lo < n_pos);
        d[b] = hi - lo;
    }
    size_t off = 0;
    for (size_t l = 0; l + 1 < p.rows.size(); l++) {        // k_rdm1_reduce, as fr_rdm1 launches it
        const size_t nxt = off + p.rows[l];
        CHECK(p.rows[l + 1] == (p.rows[l] + (uint64_t)fan - 1) / fan && p.rows[l + 1] < p.rows[l]);
        for (uint32_t b = 0; b < p.rows[l + 1]; b++) {
            const size_t lo = (size_t)b * fan, hi = lo + fan < p.rows[l] ? lo + fan : p.rows[l];
            CHECK(lo < hi);
            uint64_t x = 0;
            for (size_t j = lo; j < hi; j++) x += d[off + j];
            d[nxt + b] = x;
        }
        off = nxt;
    }
    CHECK(off == p.last_row());
    CHECK(d[p.last_row()] == n_pos);
    delete rows;
}

int main() {
    // small geometries exhaustively: one block, exact multiples, one more than a multiple, several levels
    for (uint32_t bpos : {1u, 3u, 4u})
        for (uint32_t fan : {2u, 3u, 5u})
            for (uint32_t n_pos = 1; n_pos <= 400; n_pos++) walk(n_pos, 2, bpos, fan);
    // the shipped geometry around its edges, and the sizes the tests and the benchmark use
    const uint32_t edges[] = {1, 2, RD_BPOS - 1, RD_BPOS, RD_BPOS + 1, RD_BPOS * RD_FAN - 1, RD_BPOS * RD_FAN, RD_BPOS * RD_FAN + 1, 34147, 34130, 1000000,
                              RD_BPOS * RD_FAN * RD_FAN, RD_BPOS * RD_FAN * RD_FAN + 1, 134000000u, 0xFFFFFFFFu};
    for (uint32_t n_pos : edges) walk(n_pos, 26, RD_BPOS, RD_FAN);
    {
        const Rdm1Plan p = fr_rdm1_plan(34147, 26);        // the N2 test: 134 workgroups, then 3, then 1 -- two levels of the fold, a last block that is not full
        CHECK(p.rows.size() == 3 && p.rows[0] == 134 && p.rows[1] == 3 && p.rows[2] == 1 && 34147 % RD_BPOS != 0);
        const Rdm1Plan q = fr_rdm1_plan(0xFFFFFFFFu, 32);  // the largest call: no overflow of the byte count
        CHECK(q.rows[0] == 16777216u && q.bytes() > (size_t)q.rows[0] * 1026 * 8);
    }
    printf(fails ? "rdm1_plan_check: %d FAILED\n" : "rdm1_plan_check: ok\n", fails);
    return fails ? 1 : 0;
}
