// ga_batch_support.h -- match support (ga_batch_support) as a pure model: how many of a pair's
// co-optimal alignments pair letter i of seq_1 with letter j of seq_2.  What batch_flow_kernel (ga_batch_support.hip)
// computes per pair: the cell's recurrence and a lane's step are __host__ __device__ and built into the kernel's
// translation unit and into ga_batch_support_selftest.cpp, which also runs the wave's loop on the CPU (support_wave).
//
// The alignments of a pair are the paths of the state DAG (i, j, L) from (m, n, 0) to row 0 or column 0
// (ga_batch_count.h): N(i, j, L) counts the paths from a state on.  F(i, j, L) counts the walk prefixes from (m, n, 0)
// to a state:
//   F(m, n, .) = (1, 0, 0)
//   F(i, j, 0) = A_0(i+1, j+1)   F(i, j, 1) = A_1(i, j+1)   F(i, j, 2) = A_2(i+1, j)      (0 outside the matrix)
//   A_k(i, j) = (f_0 + f_1) + f_2,  f_L = F(i, j, L) if k in S_L(i, j) else 0: the flow leaving cell (i, j) by move k
//   support(i, j) = A_0(i, j) * N(i-1, j-1, 0)                                             (N = 1 in row 0, column 0)
// Every F, A, N and product is at most the pair's count, so all are exact integers in double while count < 2^53.
#pragma once
#include <stdint.h>

#include <vector>

#include "ga_batch_layout.h"
#include "ga_batch_rank.h"

#if defined(__HIPCC__)
#define GA_SUPPORT_UNROLL _Pragma("unroll")
#else
#define GA_SUPPORT_UNROLL
#endif

namespace gabatch {

// The flows leaving a cell: sets as sets_from_code (ga_walk.h) packs them, S_L at bits 3L .. 3L + 2 with bit k move
// k; f0 .. f2 = F(i, j, 0 .. 2).  The selected terms are added in the order f0, f1, f2 (an unselected one adds 0,
// which is exact).
template <typename Num>
GA_LAYOUT_HD void flow_cell(unsigned sets, Num f0, Num f1, Num f2, Num& a0, Num& a1, Num& a2) {
    const Num z = Num(0);
    a0 = (((sets & 0x001u) ? f0 : z) + ((sets & 0x008u) ? f1 : z)) + ((sets & 0x040u) ? f2 : z);
    a1 = (((sets & 0x002u) ? f0 : z) + ((sets & 0x010u) ? f1 : z)) + ((sets & 0x080u) ? f2 : z);
    a2 = (((sets & 0x004u) ? f0 : z) + ((sets & 0x020u) ? f1 : z)) + ((sets & 0x100u) ? f2 : z);
}

// N0[i * (n + 1) + j] = N(i, j, 0), 0 <= i <= m, 0 <= j <= n, by count_paths' recurrence and addition order
template <typename Num>
inline void count_plane0(const uint16_t* sets, int64_t m, int64_t n, std::vector<Num>& N0) {
    const size_t W = (size_t)n + 1;
    N0.assign((size_t)(m + 1) * W, Num(1));
    std::vector<Num> N2(W, Num(1));
    for (int64_t i = 1; i <= m; i++) {
        Num left1 = Num(1);
        for (int64_t j = 1; j <= n; j++) {
            const unsigned s = sets[(i - 1) * n + (j - 1)];
            const Num t0 = N0[(size_t)(i - 1) * W + (size_t)(j - 1)], t1 = left1, t2 = N2[(size_t)j];
            auto terms = [&](unsigned set) {
                Num v = Num(0);
                if (set & 1u) v = v + t0;
                if (set & 2u) v = v + t1;
                if (set & 4u) v = v + t2;
                return v;
            };
            N0[(size_t)i * W + (size_t)j] = terms(s);
            left1 = terms(s >> 3);
            N2[(size_t)j] = terms(s >> 6);
        }
    }
}

// support[(i - 1) * n + (j - 1)] of every interior cell; min(m, n) >= 1.  -> N(m, n, 0), the pair's count
template <typename Num>
inline Num support_matrix(const uint16_t* sets, int64_t m, int64_t n, std::vector<Num>& support) {
    const size_t W = (size_t)n + 2;
    std::vector<Num> N0;
    count_plane0(sets, m, n, N0);
    support.assign((size_t)(m * n), Num(0));
    // A_0 and A_2 of row i + 1, columns 1 .. n + 1 (row m + 1 and column n + 1 hold 0)
    std::vector<Num> A0(W, Num(0)), A2(W, Num(0));
    for (int64_t i = m; i >= 1; i--) {
        Num diag = Num(0), right1 = Num(0);  // A_0(i + 1, j + 1) and A_1(i, j + 1)
        for (int64_t j = n; j >= 1; j--) {
            Num f0 = diag, f1 = right1, f2 = A2[(size_t)j];
            if (i == m && j == n) f0 = Num(1), f1 = Num(0), f2 = Num(0);
            Num a0, a1, a2;
            flow_cell<Num>(sets[(i - 1) * n + (j - 1)], f0, f1, f2, a0, a1, a2);
            support[(size_t)((i - 1) * n + (j - 1))] = a0 * N0[(size_t)(i - 1) * ((size_t)n + 1) + (size_t)(j - 1)];
            diag = A0[(size_t)j];
            A0[(size_t)j] = a0;
            right1 = a1;
            A2[(size_t)j] = a2;
        }
    }
    return N0[(size_t)m * ((size_t)n + 1) + (size_t)n];
}

// ---------------------------------------------------------------- a lane of batch_flow_kernel's wave
// The wave walks a stripe of 64 * T columns with lane l on row t - l + 1 at step t, t = m + 62 .. 0: lane 63 leads.
// A lane keeps, of its T columns, the flows of the row below, and hands its first column's to the lane on its left.
template <int T>
struct FlowLane {
    double A0[T], A2[T];  // A_0(i + 1, column) and A_2(i + 1, column)
    double o0, o1;        // A_0 and A_1 of the lane's first column in the row it made last: what the lane to the left takes
    double diag;          // A_0(i + 1, the column right of the lane's last)
    GA_LAYOUT_HD void reset() {
        GA_SUPPORT_UNROLL
        for (int k = 0; k < T; k++) A0[k] = A2[k] = 0.0;
        o0 = o1 = diag = 0.0;
    }
};

// One step of a lane on row i.  in0, in1: A_0 and A_1 of the column right of the lane's last in row i (the right
// lane's o0 and o1, lane 63: the stripe's edge; 0 where there is none).  sets[k]: the cell's sets in column k;
// live: bit k set when the cell exists (row in 1 .. m, column k at most n); seed: the column that is cell (m, n) in
// this row, or -1.  a0[k] receives A_0(i, column k).  A cell that does not exist hands on ZERO flow: in this
// direction a cell does take from its right and from below.
template <int T>
GA_LAYOUT_HD void flow_lane_step(FlowLane<T>& st, double in0, double in1, const unsigned* sets, unsigned live, int seed,
                                 double* a0) {
    double f0 = st.diag, f1 = in1;
    GA_SUPPORT_UNROLL
    for (int k = T - 1; k >= 0; k--) {
        double f2 = st.A2[k];
        if (k == seed) f0 = 1.0, f1 = 0.0, f2 = 0.0;
        double x0, x1, x2;
        flow_cell<double>(sets[k], f0, f1, f2, x0, x1, x2);
        const bool ok = (live >> k) & 1u;
        x0 = ok ? x0 : 0.0;
        x1 = ok ? x1 : 0.0;
        x2 = ok ? x2 : 0.0;
        a0[k] = x0;
        f0 = st.A0[k];  // A_0(i + 1, this column): the diagonal of the column to its left
        f1 = x1;
        st.A0[k] = x0;
        st.A2[k] = x2;
    }
    st.o1 = f1;
    st.o0 = st.A0[0];
    st.diag = in0;
}

// N(i - 1, j - 1, 0) as the flow kernel takes it: 1 in row 0 and column 0, else the N table's entry (plane 0)
template <typename Table>
GA_LAYOUT_HD double support_n(const Table& table, int m, int T, int i, int j) {
    return (i == 1 || j == 1) ? 1.0 : table[rank_table_index(m, T, i - 1, j - 1, 0)];
}
// where support(i, j) goes in the pair's table: plane 1 of the cell's own entry, which the N-table launch leaves alone
GA_LAYOUT_HD unsigned long long support_index(int m, int T, int i, int j) { return rank_table_index(m, T, i, j, 1); }

// The wave's loop on the CPU, lane by lane: what batch_flow_kernel's flow_pair does with DPP moves and an edge column.
// table: the pair's N table in rank_table_index's layout, plane 0 filled; plane 1 receives support.  sets_at(i, j):
// the sets of a cell with 1 <= i <= m and 1 <= j <= n (never asked for another).
template <int T, typename Sets>
inline void support_wave(Sets sets_at, int m, int n, int nstripes, std::vector<double>& table) {
    std::vector<double> edge0((size_t)m, 0.0), edge1((size_t)m, 0.0);
    for (int s = nstripes - 1; s >= 0; s--) {
        const int j0 = s * 64 * T;
        FlowLane<T> st[64];
        for (auto& x : st) x.reset();
        std::vector<double> next0((size_t)m, 0.0), next1((size_t)m, 0.0);
        for (int t = m + 62; t >= 0; t--) {
            // the moves read every lane's o0 / o1 of the step before: take them all first
            double in0[64], in1[64];
            for (int l = 0; l < 64; l++) {
                const int i = t - l + 1;
                const bool edge = l == 63 && s < nstripes - 1 && i >= 1 && i <= m;
                in0[l] = l < 63 ? st[l + 1].o0 : edge ? edge0[(size_t)(i - 1)] : 0.0;
                in1[l] = l < 63 ? st[l + 1].o1 : edge ? edge1[(size_t)(i - 1)] : 0.0;
            }
            for (int l = 0; l < 64; l++) {
                const int i = t - l + 1;
                const bool act = i >= 1 && i <= m;
                unsigned sets[T], live = 0;
                int seed = -1;
                for (int k = 0; k < T; k++) {
                    const int j = j0 + l * T + k + 1;
                    sets[k] = act ? (unsigned)sets_at(i, j < n ? j : n) : 0x1ffu;
                    if (act && j <= n) live |= 1u << k;
                    if (i == m && j == n) seed = k;
                }
                double a0[T];
                flow_lane_step<T>(st[l], in0[l], in1[l], sets, live, seed, a0);
                for (int k = 0; k < T; k++)
                    if ((live >> k) & 1u) {
                        const int j = j0 + l * T + k + 1;
                        table[(size_t)support_index(m, T, i, j)] = a0[k] * support_n(table, m, T, i, j);
                    }
                if (l == 0 && act) next0[(size_t)(i - 1)] = st[0].o0, next1[(size_t)(i - 1)] = st[0].o1;
            }
        }
        edge0.swap(next0);
        edge1.swap(next1);
    }
}

}  // namespace gabatch
