// ga_count_stripe.h -- the stripe loop of the path-count recurrence, one pair by one wave (gfx950): what
// batch_count_kernel (ga_batch_count.hip) and batch_rank_table_kernel (ga_batch_rank.hip, DESIGN.md
// 5.14) share, and batch_support_table_kernel (ga_batch_support.hip).  The number type comes in as a
// policy: CountF64 adds IEEE doubles and keeps nothing but N(m, n, 0); CountU64Sat adds u64s that saturate at 2^64 - 1
// and stores N(i, j, 0 .. 2) of every interior cell to the pair's count table (gabatch::rank_table_index,
// ga_batch_rank.h); CountF64Keep adds as CountF64 does and stores N(i, j, 0), the one plane the flow pass reads, to the
// same places.
//
//   T0 = N(i-1, j-1, 0)   T1 = N(i, j-1, 1)   T2 = N(i-1, j, 2)
//   N(i, j, L) = sum of T_k over k in S_L(i, j),   N = 1 in row 0 and column 0,   count = N(m, n, 0).
//
// A wave counts a pair in stripes of 64 * T columns, left to right, lane-skewed: lane l owns T adjacent columns and
// works on row t - l + 1 at step t, so T1 (and the first column's T0) arrive from the left neighbour one step after it
// made them, two 32-bit DPP wave_shr:1 moves per number; T2 and the other T0s are the lane's own previous row.  A
// stripe hands its right edge, N(i, edge, 0) and N(i, edge, 1), to the next through the wave's LDS share while m
// fits, else through two HBM slices of its own, as batch_pair does.  A stripe takes m + 63 steps.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ga_batch.h"
#include "ga_batch_layout.h"
#include "ga_batch_rank.h"
#include "ga_walk.h"

namespace ga {

// IEEE double additions only, the selected terms in the order T0, T1, T2 (an unselected one adds 0.0, which is
// exact): bit for bit what the recurrence gives in double anywhere, exact below 2^53, +inf past the double range and
// never NaN.
struct CountF64 {
    using Num = double;
    using Edge = double2;
    static constexpr bool kStore = false;
    static __device__ __forceinline__ Num zero() { return 0.0; }
    static __device__ __forceinline__ Num one() { return 1.0; }
    static __device__ __forceinline__ Num add(Num a, Num b) { return a + b; }
    static __device__ __forceinline__ Edge edge(Num x, Num y) { return make_double2(x, y); }
    static __device__ __forceinline__ int lo(Num x) { return __double2loint(x); }
    static __device__ __forceinline__ int hi(Num x) { return __double2hiint(x); }
    static __device__ __forceinline__ Num join(int h, int l) { return __hiloint2double(h, l); }
};

// u64 additions that saturate at 2^64 - 1 (an add, a carry and a select on gfx950), and every cell's three counts kept
struct CountU64Sat {
    using Num = unsigned long long;
    using Edge = ulonglong2;
    static constexpr bool kStore = true;
    static constexpr bool kStoreAll = true;
    static __device__ __forceinline__ unsigned long long bits(Num x) { return x; }
    static __device__ __forceinline__ Num zero() { return 0ull; }
    static __device__ __forceinline__ Num one() { return 1ull; }
    static __device__ __forceinline__ Num add(Num a, Num b) { return __builtin_elementwise_add_sat(a, b); }
    static __device__ __forceinline__ Edge edge(Num x, Num y) { return make_ulonglong2(x, y); }
    static __device__ __forceinline__ int lo(Num x) { return (int)(unsigned)x; }
    static __device__ __forceinline__ int hi(Num x) { return (int)(unsigned)(x >> 32); }
    static __device__ __forceinline__ Num join(int h, int l) { return ((Num)(unsigned)h << 32) | (unsigned)l; }
};

// CountF64's additions, and N(i, j, 0) of every interior cell kept as the double's bits in plane 0 of the cell's
// entry; planes 1 and 2 are left as they are (batch_flow_kernel puts its result in plane 1)
struct CountF64Keep : CountF64 {
    static constexpr bool kStore = true;
    static constexpr bool kStoreAll = false;
    static __device__ __forceinline__ unsigned long long bits(Num x) { return (unsigned long long)__double_as_longlong(x); }
};

// x of the lane to the left (lane 0: `edge`)
template <typename P>
__device__ __forceinline__ typename P::Num shr1_num(typename P::Num edge, typename P::Num x) {
    const int lo = __builtin_amdgcn_update_dpp(P::lo(edge), P::lo(x), 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(P::hi(edge), P::hi(x), 0x138, 0xf, 0xf, false);
    return P::join(hi, lo);
}

// the terms of one rank set (bit 0: T0, bit 1: T1, bit 2: T2), added in that order
template <typename P>
__device__ __forceinline__ typename P::Num count_terms(int set, typename P::Num t0, typename P::Num t1,
                                                       typename P::Num t2) {
    return P::add(P::add((set & 1) ? t0 : P::zero(), (set & 2) ? t1 : P::zero()), (set & 4) ? t2 : P::zero());
}

// One pair by one wave -> N(m, n, 0), the same in every lane.  tbw: the pair's words in LAYOUT (ga_batch_layout.h) at
// gap-open cost o (`tc`: LAYOUT_STRIPE's 16-byte words per lane); HBM: the edge column lies in the wave's HBM slices
// edge_g of `srows` rows each (batch_pair's rule), else in LDS at edge_l.  P::kStore: `table` is the pair's count table.
template <typename P, int T, int CB, int LAYOUT, bool HBM>
__device__ typename P::Num count_pair(int o, int tc, long long srows, const ga_batch_item& it, const uint32_t* tbw,
                                      typename P::Edge* edge_l, typename P::Edge* edge_g, int lane,
                                      unsigned long long* table = nullptr) {
    using Addr = gabatch::TbAddr<CB, LAYOUT>;
    using Num = typename P::Num;
    using Edge = typename P::Edge;
    constexpr int RPW = 4 / CB;
    constexpr unsigned MASK = CB == 4 ? 0xffffffffu : (1u << (8 * CB)) - 1u;
    const int m = it.m, n = it.n;
    const int geom = LAYOUT == gabatch::LAYOUT_BATCH ? 64 * it.T * it.nstripes : tc;
    Num total = P::zero();
    for (int s = 0; s < it.nstripes; s++) {
        const int j0 = s * 64 * T;
        const bool last = s == it.nstripes - 1;
        // the edge column: in LDS one column read and rewritten in place (lane 0 reads a row 64 steps before lane 63
        // rewrites it), in HBM the two slices by stripe parity
        const Edge* gin = edge_g + (long long)(s & 1) * srows;
        Edge* gout = edge_g + (long long)((s + 1) & 1) * srows;
        // this lane's columns; one past n (the last stripe's) reads column n's words and counts garbage nobody
        // reads: a cell takes nothing from its right
        int jc[T];
#pragma unroll
        for (int k = 0; k < T; k++) jc[k] = min(j0 + lane * T + k + 1, n);
        Num N0[T], N2[T];  // N(i - 1, column, 0) and N(i - 1, column, 2): row 0 holds 1
#pragma unroll
        for (int k = 0; k < T; k++) N0[k] = N2[k] = P::one();
        Num o0 = P::one(), o1 = P::one();  // N(i, the lane's last column, 0 and 1): what the lane to the right takes
        Num diag = P::one();               // N(i - 1, the column left of the lane's first, 0)
        // a u32 holds RPW rows of a column: `cur` the rows being counted, `nxt` the next ones, on their way
        uint32_t cur[T], nxt[T];
#pragma unroll
        for (int k = 0; k < T; k++) {
            cur[k] = 0;
            nxt[k] = tbw[Addr::word(1, jc[k], geom)];
        }
        // lane 0: the left edge of its row, (N(i, edge, 0), N(i, edge, 1)), one row ahead; stripe 0: column 0's 1
        Edge en = P::edge(P::one(), P::one());
        if (s > 0 && lane == 0) en = HBM ? gin[0] : edge_l[0];
        // (kStore) the lane's first entry of step 0 in the pair's table, and which of its columns exist
        unsigned long long* tp = nullptr;
        if constexpr (P::kStore)
            tp = table + gabatch::rank_table_step(m, T, s, 0) + lane;
        for (int t = 0; t < m + 63; t++) {
            const int i = t - lane + 1;
            const bool act = i >= 1 && i <= m;
            const Edge e = en;
            if (s > 0 && lane == 0 && t + 1 < m) en = HBM ? gin[t + 1] : edge_l[t + 1];
            // (the DPPs run in every lane)
            const Num in1 = shr1_num<P>(e.y, o1);  // N(i, left, 1)
            const Num in0 = shr1_num<P>(e.x, o0);  // N(i, left, 0): the next step's diagonal
            if (act && ((i - 1) & (RPW - 1)) == 0) {
#pragma unroll
                for (int k = 0; k < T; k++) cur[k] = nxt[k];
                if (i + RPW <= m) {
#pragma unroll
                    for (int k = 0; k < T; k++) nxt[k] = tbw[Addr::word(i + RPW, jc[k], geom)];
                }
            }
            const int sh = Addr::shift(i);
            Num t0 = diag, t1 = in1;
#pragma unroll
            for (int k = 0; k < T; k++) {
                const int sets = sets_from_code((cur[k] >> sh) & MASK, CB, o);
                const Num t2 = N2[k];
                const Num n0 = count_terms<P>(sets, t0, t1, t2);
                const Num n1 = count_terms<P>(sets >> 3, t0, t1, t2);
                const Num n2 = count_terms<P>(sets >> 6, t0, t1, t2);
                if constexpr (P::kStore) {
                    // the step's 3 T (kStoreAll; else T) stores are 64 consecutive u64 each (a lane off the matrix
                    // leaves its hole)
                    if (act && j0 + lane * T + k + 1 <= n) {
                        tp[(3 * k + 0) * 64] = P::bits(n0);
                        if constexpr (P::kStoreAll) {
                            tp[(3 * k + 1) * 64] = P::bits(n1);
                            tp[(3 * k + 2) * 64] = P::bits(n2);
                        }
                    }
                }
                t0 = N0[k];  // N(i - 1, this column, 0): the next column's diagonal
                t1 = n1;
                // a lane above row 1 keeps row 0's values, one past row m keeps row m's
                N0[k] = act ? n0 : N0[k];
                N2[k] = act ? n2 : N2[k];
            }
            if constexpr (P::kStore) tp += 3 * T * 64;
            o1 = act ? t1 : o1;
            o0 = N0[T - 1];
            diag = in0;
            if (!last && lane == 63 && act) {
                if (HBM) gout[i - 1] = P::edge(o0, o1);
                else edge_l[i - 1] = P::edge(o0, o1);
            }
        }
        // lane 63's edge rows are read by lane 0 of this wave in the next stripe: one wave's memory operations to an
        // address stay in order, and this wave-scope fence says so to the compiler and the memory model
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (last) {
            const int ke_l = (n - 1 - j0) / T, ke_k = (n - 1 - j0) % T;
            Num v = N0[0];
#pragma unroll
            for (int k = 1; k < T; k++)
                if (k == ke_k) v = N0[k];
            total = P::join(__builtin_amdgcn_readlane(P::hi(v), ke_l), __builtin_amdgcn_readlane(P::lo(v), ke_l));
        }
    }
    return total;
}

}  // namespace ga
