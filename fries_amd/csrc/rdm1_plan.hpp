// Host-only geometry of fries_rdm1's scratch (rdm1.hip): how many partial matrices every level of the fold holds.  No HIP in here, so
// that a plain C++ program can check it (tests/cpp/rdm1_plan_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#define RD_WPOS 64                  // positions one wave walks: one coalesced load of its sources
#define RD_BPOS (4 * RD_WPOS)       // positions per workgroup of four waves
#define RD_FAN 64                   // partial matrices one workgroup of the fold adds, in index order
#define RD_NSCAL 2                  // doubles behind every partial matrix: ovlp, abs_sum
#define RD_NCNT 3                   // counters of every partial: n_src, n_terms, n_hits

struct Rdm1Plan {
    std::vector<uint32_t> rows;     // rows[0] = workgroups of k_rdm1; rows[l + 1] = workgroups of the l-th k_rdm1_reduce; the last is 1
    size_t stride = 0;              // doubles per row: n_orb^2 + RD_NSCAL
    size_t total_rows = 0;
    size_t last_row() const { return total_rows - 1; }
    size_t bytes() const { return total_rows * (stride * sizeof(double) + RD_NCNT * sizeof(unsigned long long)); }
};

// n_pos > 0.  bpos / fan are arguments so that the check can walk small geometries.
static inline Rdm1Plan fr_rdm1_plan(uint32_t n_pos, uint32_t n_orb, uint32_t bpos = RD_BPOS, uint32_t fan = RD_FAN) {
    Rdm1Plan p;
    p.stride = (size_t)n_orb * n_orb + RD_NSCAL;
    uint32_t n = (uint32_t)(((uint64_t)n_pos + bpos - 1) / bpos);
    p.rows.push_back(n);
    p.total_rows = n;
    while (n > 1) {
        n = (uint32_t)(((uint64_t)n + fan - 1) / fan);
        p.rows.push_back(n);
        p.total_rows += n;
    }
    return p;
}
