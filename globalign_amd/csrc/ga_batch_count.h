// ga_batch_count.h -- the count recurrence of ga_batch_count as a pure CPU model (no HIP): what batch_count_kernel
// (ga_batch_count.hip) computes per pair, over any number type with 1 and +.  Built into
// ga_batch_count_selftest.cpp, in double and in 128-bit integers.
#pragma once
#include <stdint.h>

#include <vector>

namespace gabatch {

// sets[(i - 1) * n + (j - 1)], 1 <= i <= m, 1 <= j <= n: the three rank sets of cell (i, j) as sets_from_code
// (ga_walk.h) packs them, S_L at bits 3L .. 3L + 2 with bit 0 level 0 (diagonal), bit 1 level 1 (left), bit 2 level 2
// (up).  -> N(m, n, 0) of
//   T0 = N(i-1, j-1, 0)   T1 = N(i, j-1, 1)   T2 = N(i-1, j, 2)
//   N(i, j, L) = sum of T_k over k in S_L(i, j), the selected terms added in the order T0, T1, T2;  N = 1 in row 0
//   and column 0.
template <typename Num>
inline Num count_paths(const uint16_t* sets, int64_t m, int64_t n) {
    // row i - 1 of N(., ., 0) and N(., ., 2), columns 0 .. n
    std::vector<Num> N0((size_t)n + 1, Num(1)), N2((size_t)n + 1, Num(1));
    for (int64_t i = 1; i <= m; i++) {
        Num diag = N0[0], left1 = Num(1);  // N(i-1, j-1, 0) and N(i, j-1, 1); column 0 holds 1
        for (int64_t j = 1; j <= n; j++) {
            const unsigned s = sets[(i - 1) * n + (j - 1)];
            const Num t0 = diag, t1 = left1, t2 = N2[(size_t)j];
            auto terms = [&](unsigned set) {
                Num v = Num(0);
                if (set & 1u) v = v + t0;
                if (set & 2u) v = v + t1;
                if (set & 4u) v = v + t2;
                return v;
            };
            diag = N0[(size_t)j];
            N0[(size_t)j] = terms(s);
            left1 = terms(s >> 3);
            N2[(size_t)j] = terms(s >> 6);
        }
    }
    return N0[(size_t)n];
}

}  // namespace gabatch
