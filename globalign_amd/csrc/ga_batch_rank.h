// ga_batch_rank.h -- co-optimal alignments by rank (ga_batch_rank) as a pure CPU model (no HIP): the
// saturating count table batch_rank_table_kernel keeps, the unranking walk batch_rank_walk_kernel makes over it
// (ga_batch_rank.hip), and where a cell's counts lie in a pair's table -- the one address function both kernels and
// the model use.  Built into the kernels' translation units and into ga_batch_rank_selftest.cpp.
//
// The alignments of a pair are the paths of the state DAG (i, j, L) from (m, n, 0) to row 0 or column 0
// (ga_batch_count.h).  They are ordered by their level sequence as the traceback emits it, from the alignment's last
// column backwards, lexicographically with level 0 (diagonal) < 1 (left) < 2 (up).  The walk for rank r goes, at a
// state, through the selected moves k of S_L in the order 0, 1, 2: if r < T_k it takes move k, else r -= T_k.  The
// counts are u64 and saturate at 2^64 - 1; a saturated T_k exceeds any legal r and an unsaturated one is the true
// value, so the walk is exact for every r < min(count, 2^64 - 1).
#pragma once
#include <stdint.h>

#include <vector>

#include "ga_batch_layout.h"

namespace gabatch {

constexpr uint64_t kRankCap = ~0ull;  // the counts saturate here

// a slot's status as batch_rank_walk_kernel reports it
constexpr int kRankOk = 0, kRankOutOfRange = 1, kRankBadItem = 2;

// ---------------------------------------------------------------- the count table's layout
// batch_rank_table_kernel's wave sits, at step t of stripe s, with lane l on row t - l + 1 of its T columns
// s * 64 * T + l * T + k + 1 (ga_count_stripe.h): 64 different rows, so a row-major table would make every store a
// 64-way scatter.  The table is step-major instead, structure-of-arrays:
//   u64 index ((s * (m + 63) + t) * 3 T + 3 k + plane) * 64 + l,   t = i - 1 + l,   plane = L of N(i, j, L),
// so each of a step's 3 T stores is 64 consecutive u64 (512 bytes).  Rows outside 1 .. m leave holes nobody reads.

// the first entry of step t of stripe s
GA_LAYOUT_HD unsigned long long rank_table_step(int m, int T, int s, int t) {
    return ((unsigned long long)s * (unsigned)(m + 63) + (unsigned)t) * (unsigned)(3 * T) * 64ull;
}
// N(i, j, plane) of an interior cell, 1 <= i <= m, 1 <= j <= n
GA_LAYOUT_HD unsigned long long rank_table_index(int m, int T, int i, int j, int plane) {
    const int s = (j - 1) / (64 * T), jj = (j - 1) - s * 64 * T, l = jj / T, k = jj - l * T;
    return rank_table_step(m, T, s, i - 1 + l) + (unsigned)(3 * k + plane) * 64ull + (unsigned)l;
}
// u64 entries of a pair's table
inline int64_t rank_table_entries(int64_t m, int T, int nstripes) { return (int64_t)nstripes * (m + 63) * 3 * T * 64; }

// ---------------------------------------------------------------- the saturating recurrence
inline uint64_t sat_add(uint64_t a, uint64_t b, uint64_t cap) {
    const uint64_t s = a + b;
    return (s < a || s > cap) ? cap : s;
}

// N[((i - 1) * n + (j - 1)) * 3 + L] = min(N(i, j, L), cap) of every interior cell, every addition saturating at cap;
// sets as count_paths takes them (ga_batch_count.h).  -> min(count, cap)
inline uint64_t rank_table(const uint16_t* sets, int64_t m, int64_t n, uint64_t cap, std::vector<uint64_t>& N) {
    N.assign((size_t)(m * n * 3), 0);
    auto at = [&](int64_t i, int64_t j, int L) -> uint64_t {
        return (i == 0 || j == 0) ? 1 : N[(size_t)(((i - 1) * n + (j - 1)) * 3 + L)];
    };
    for (int64_t i = 1; i <= m; i++)
        for (int64_t j = 1; j <= n; j++) {
            const unsigned s = sets[(i - 1) * n + (j - 1)];
            const uint64_t t0 = at(i - 1, j - 1, 0), t1 = at(i, j - 1, 1), t2 = at(i - 1, j, 2);
            for (int L = 0; L < 3; L++) {
                const unsigned set = s >> (3 * L);
                uint64_t v = 0;
                if (set & 1u) v = sat_add(v, t0, cap);
                if (set & 2u) v = sat_add(v, t1, cap);
                if (set & 4u) v = sat_add(v, t2, cap);
                N[(size_t)(((i - 1) * n + (j - 1)) * 3 + L)] = v;
            }
        }
    return at(m, n, 0);
}

// ---------------------------------------------------------------- the unranking walk
// The move out of a state whose set is S (bit k: move k) under rank r: the selected moves in the order 0, 1, 2, move
// k taken when r < term(k), else r -= term(k).  The last selected move is taken without reading its count (a legal
// rank is below it), so a state with one selected move reads nothing, and any S, r and counts give a move: an empty
// set, which no filled cell has, gives the diagonal.
template <typename Term>
GA_LAYOUT_HD int rank_choose(unsigned S, unsigned long long& r, Term term) {
    int lvl = 0;
    for (int k = 0; k < 3; k++) {
        if (!((S >> k) & 1u)) continue;
        lvl = k;
        if (((S & 7u) >> (k + 1)) == 0) break;
        const unsigned long long tk = term(k);
        if (r < tk) break;
        r -= tk;
    }
    return lvl;
}

struct RankWalk {
    int32_t D = 0, i_end = 0, j_end = 0, reason = 0;  // batch_walk's {dispatches, i_end, j_end, reason}
    int status = kRankOk;
};

// The walk for rank r from (m, n, 0).  sets(i, j): the cell's packed sets; count(i, j, L): N(i, j, L) of an interior
// cell as the table holds it (anything: the walk makes at most m + n - 1 dispatches and stays in rows and columns >= 1
// until it ends, whatever the two return).  Levels go to ops as batch_walk packs them: 16 a u32, level D at bits
// 30 - 2 * (D & 15) of word D >> 4.  r >= count(m, n, 0): kRankOutOfRange, and no walk.
template <typename Sets, typename Count>
inline RankWalk rank_walk(Sets sets, Count count, int32_t m, int32_t n, uint64_t r, uint32_t* ops) {
    RankWalk w;
    if (r >= count(m, n, 0)) {
        w.status = kRankOutOfRange;
        return w;
    }
    int32_t i = m, j = n, D = 0;
    int L = 0;
    uint32_t opsw = 0;
    unsigned long long rr = r;
    while (i > 0 && j > 0 && D < m + n) {
        const unsigned S = ((unsigned)sets(i, j) >> (3 * L)) & 7u;
        const int lvl = rank_choose(S, rr, [&](int k) -> unsigned long long {
            const int32_t pi = i - (k != 1), pj = j - (k != 2);
            return (pi == 0 || pj == 0) ? 1ull : count(pi, pj, k);
        });
        opsw |= (uint32_t)lvl << (30 - 2 * (D & 15));
        if ((D & 15) == 15) {
            ops[D >> 4] = opsw;
            opsw = 0;
        }
        D++;
        i -= lvl != 1;
        j -= lvl != 2;
        L = lvl;
    }
    if (D & 15) ops[D >> 4] = opsw;
    w.D = D;
    w.i_end = i;
    w.j_end = j;
    w.reason = i == 0 ? (j == 0 ? 0 : 1) : 2;
    return w;
}

}  // namespace gabatch
