// ga_batch_count.hip -- batch_count_kernel: the number of co-optimal alignments of every pair of a batch, one wave
// per pair (gfx950; ga_batch_count).
//
// The reference's traceback (dp_array_backward, globaligner.py:395-593) is a walk on the DAG of states (i, j, L), L
// the level the walk entered cell (i, j) with; at a tie random.choice picks among the argmin set S_L(i, j).  The
// alignments it can return are the paths of that DAG from (m, n, 0) to row 0 or column 0, where the tail is forced:
//   T0 = N(i-1, j-1, 0)   T1 = N(i, j-1, 1)   T2 = N(i-1, j, 2)
//   N(i, j, L) = sum of T_k over k in S_L(i, j),   N = 1 in row 0 and column 0,   count = N(m, n, 0).
// The sets come from the pair's stored traceback words (sets_from_code, ga_walk.h), which an earlier launch on the
// same stream wrote (batch_words_kernel, or the single-pair fill for a large pair) and this kernel only reads, with
// vector loads.  Stream order is the only ordering: no wave waits for another.
//
// Persistent waves take pairs off a ticket word of their own.  A wave counts a pair in stripes of 64 * T columns,
// left to right, lane-skewed: lane l owns T adjacent columns and works on row t - l + 1 at step t, so T1 (and the
// first column's T0) arrive from the left neighbour one step after it made them, two 32-bit DPP wave_shr:1 moves per
// double; T2 and the other T0s are the lane's own previous row.  A stripe hands its right edge, N(i, edge, 0) and
// N(i, edge, 1), to the next through the wave's LDS share while m fits, else through two HBM slices of its own, as
// batch_pair does.  A stripe takes m + 63 steps.
//
// The arithmetic is IEEE double additions only, the selected terms in the order T0, T1, T2 (an unselected one adds
// 0.0, which is exact): the result is bit for bit what the recurrence gives in double anywhere, exact below 2^53,
// +inf past the double range and never NaN.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ga_batch.h"
#include "ga_batch_layout.h"
#include "ga_device.h"
#include "ga_walk.h"

namespace ga {

// written instead of a count when a work item does not fit the launch's buffers (the planner never emits one)
constexpr double COUNT_BAD_ITEM = -1.0;

// x of the lane to the left (lane 0: `edge`)
__device__ __forceinline__ double shr1_f64(double edge, double x) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(edge), __double2loint(x), 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(edge), __double2hiint(x), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// the terms of one rank set (bit 0: T0, bit 1: T1, bit 2: T2), added in that order
__device__ __forceinline__ double count_terms(int set, double t0, double t1, double t2) {
    return (((set & 1) ? t0 : 0.0) + ((set & 2) ? t1 : 0.0)) + ((set & 4) ? t2 : 0.0);
}

// One pair by one wave -> N(m, n, 0), the same in every lane.  tbw: the pair's words in LAYOUT (ga_batch_layout.h);
// HBM: the edge column lies in the wave's HBM slices (batch_pair's rule), else in LDS.
template <int T, int CB, int LAYOUT, bool HBM>
__device__ double count_pair(const CountArgs& q, const ga_batch_item& it, const uint32_t* tbw, double2* edge_l,
                             double2* edge_g, int lane) {
    using Addr = gabatch::TbAddr<CB, LAYOUT>;
    constexpr int RPW = 4 / CB;
    constexpr unsigned MASK = CB == 4 ? 0xffffffffu : (1u << (8 * CB)) - 1u;
    const int m = it.m, n = it.n, o = q.o;
    const int geom = LAYOUT == gabatch::LAYOUT_BATCH ? 64 * it.T * it.nstripes : q.tc;
    const long long srows = q.scratch_rows;
    double total = 0.0;
    for (int s = 0; s < it.nstripes; s++) {
        const int j0 = s * 64 * T;
        const bool last = s == it.nstripes - 1;
        // the edge column: in LDS one column read and rewritten in place (lane 0 reads a row 64 steps before lane 63
        // rewrites it), in HBM the two slices by stripe parity
        const double2* gin = edge_g + (long long)(s & 1) * srows;
        double2* gout = edge_g + (long long)((s + 1) & 1) * srows;
        // this lane's columns; one past n (the last stripe's) reads column n's words and counts garbage nobody
        // reads: a cell takes nothing from its right
        int jc[T];
#pragma unroll
        for (int k = 0; k < T; k++) jc[k] = min(j0 + lane * T + k + 1, n);
        double N0[T], N2[T];  // N(i - 1, column, 0) and N(i - 1, column, 2): row 0 holds 1
#pragma unroll
        for (int k = 0; k < T; k++) N0[k] = N2[k] = 1.0;
        double o0 = 1.0, o1 = 1.0;  // N(i, the lane's last column, 0 and 1): what the lane to the right takes
        double diag = 1.0;          // N(i - 1, the column left of the lane's first, 0)
        // a u32 holds RPW rows of a column: `cur` the rows being counted, `nxt` the next ones, on their way
        uint32_t cur[T], nxt[T];
#pragma unroll
        for (int k = 0; k < T; k++) {
            cur[k] = 0;
            nxt[k] = tbw[Addr::word(1, jc[k], geom)];
        }
        // lane 0: the left edge of its row, (N(i, edge, 0), N(i, edge, 1)), one row ahead; stripe 0: column 0's 1
        double2 en = make_double2(1.0, 1.0);
        if (s > 0 && lane == 0) en = HBM ? gin[0] : edge_l[0];
        for (int t = 0; t < m + 63; t++) {
            const int i = t - lane + 1;
            const bool act = i >= 1 && i <= m;
            const double2 e = en;
            if (s > 0 && lane == 0 && t + 1 < m) en = HBM ? gin[t + 1] : edge_l[t + 1];
            // (the DPPs run in every lane)
            const double in1 = shr1_f64(e.y, o1);  // N(i, left, 1)
            const double in0 = shr1_f64(e.x, o0);  // N(i, left, 0): the next step's diagonal
            if (act && ((i - 1) & (RPW - 1)) == 0) {
#pragma unroll
                for (int k = 0; k < T; k++) cur[k] = nxt[k];
                if (i + RPW <= m) {
#pragma unroll
                    for (int k = 0; k < T; k++) nxt[k] = tbw[Addr::word(i + RPW, jc[k], geom)];
                }
            }
            const int sh = Addr::shift(i);
            double t0 = diag, t1 = in1;
#pragma unroll
            for (int k = 0; k < T; k++) {
                const int sets = sets_from_code((cur[k] >> sh) & MASK, CB, o);
                const double t2 = N2[k];
                const double n0 = count_terms(sets, t0, t1, t2);
                const double n1 = count_terms(sets >> 3, t0, t1, t2);
                const double n2 = count_terms(sets >> 6, t0, t1, t2);
                t0 = N0[k];  // N(i - 1, this column, 0): the next column's diagonal
                t1 = n1;
                // a lane above row 1 keeps row 0's values, one past row m keeps row m's
                N0[k] = act ? n0 : N0[k];
                N2[k] = act ? n2 : N2[k];
            }
            o1 = act ? t1 : o1;
            o0 = N0[T - 1];
            diag = in0;
            if (!last && lane == 63 && act) {
                if (HBM) gout[i - 1] = make_double2(o0, o1);
                else edge_l[i - 1] = make_double2(o0, o1);
            }
        }
        // lane 63's edge rows are read by lane 0 of this wave in the next stripe: one wave's memory operations to an
        // address stay in order, and this wave-scope fence says so to the compiler and the memory model
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (last) {
            const int ke_l = (n - 1 - j0) / T, ke_k = (n - 1 - j0) % T;
            double v = N0[0];
#pragma unroll
            for (int k = 1; k < T; k++)
                if (k == ke_k) v = N0[k];
            total = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), ke_l),
                                     __builtin_amdgcn_readlane(__double2loint(v), ke_l));
        }
    }
    return total;
}

template <int T, int CB, int LAYOUT>
__device__ __forceinline__ double count_either(const CountArgs& q, const ga_batch_item& it, bool hbm, const uint32_t* tbw,
                                               double2* edge_l, double2* edge_g, int lane) {
    if (hbm) return count_pair<T, CB, LAYOUT, true>(q, it, tbw, edge_l, edge_g, lane);
    return count_pair<T, CB, LAYOUT, false>(q, it, tbw, edge_l, edge_g, lane);
}

template <int CB, int LAYOUT>
__global__ void __launch_bounds__(64 * gabatch::kWavesPerGroup) batch_count_kernel(CountArgs q) {
    __shared__ double2 edge_s[gabatch::kWavesPerGroup][gabatch::kLdsEdgeRows];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long gw = (long long)blockIdx.x * gabatch::kWavesPerGroup + w;
    double2* edge_g = q.scratch ? q.scratch + gw * 2 * q.scratch_rows : nullptr;
    for (;;) {
        // the only lane-divergent branch of the loop; the wave is whole again at the readfirstlane
        unsigned t = 0;
        if (lane == 0) t = __hip_atomic_fetch_add(q.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
        if (t >= (unsigned)q.nitems) break;
        const ga_batch_item it = q.items[t];
        const ga_batch_words_item ws = q.words[t];
        const bool hbm = it.nstripes > 1 && it.m > gabatch::kLdsEdgeRows;
        // the pair's words must lie inside the launch's, its stripes must cover its columns with only the last one
        // partial, and an edge column in HBM must fit this wave's slices (ga_batch.h plans it so); a count needs two
        // letters a side
        bool fits = it.m >= 2 && it.n >= 2 && it.T >= 1 && it.T <= gabatch::kMaxT && it.nstripes >= 1 &&
                    (long long)64 * it.T * it.nstripes >= it.n && (long long)64 * it.T * (it.nstripes - 1) < it.n &&
                    ws.tb_off >= 0 && ws.tb_off <= q.tb_words &&
                    !(hbm && (edge_g == nullptr || it.m > q.scratch_rows));
        if (LAYOUT == gabatch::LAYOUT_BATCH) {
            fits = fits && (long long)((it.m + 4 / CB - 1) / (4 / CB)) * 64 * it.T * it.nstripes <= ws.tb_words &&
                   ws.tb_words <= q.tb_words - ws.tb_off;
        } else {
            fits = fits && q.tc >= 1 && (long long)q.tc * (16 / CB) >= it.m &&
                   (long long)((it.n + 63) / 64) * q.tc * 256 <= q.tb_words - ws.tb_off;
        }
        const uint32_t* tbw = q.tb + (fits ? ws.tb_off : 0);
        double r = COUNT_BAD_ITEM;
        switch (fits ? it.T : 0) {
            case 1: r = count_either<1, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane); break;
            case 2: r = count_either<2, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane); break;
            case 3: r = count_either<3, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane); break;
            case 4: r = count_either<4, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane); break;
            case 5: r = count_either<5, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane); break;
            case 6: r = count_either<6, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane); break;
            case 7: r = count_either<7, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane); break;
            case 8: r = count_either<8, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane); break;
            default: break;
        }
        // every lane stores the same value (no lane-divergent branch at an item's end, see batch_pair); an item
        // whose slot lies outside the output has nowhere to report to
        if (it.out >= 0 && it.out < q.npairs) q.count_out[it.out] = r;
    }
}

template <int LAYOUT>
static void launch_batch_count_l(hipStream_t s, const CountArgs& q, int CB, int groups) {
    const int threads = 64 * gabatch::kWavesPerGroup;
    if (CB == 1) batch_count_kernel<1, LAYOUT><<<groups, threads, 0, s>>>(q);
    else if (CB == 2) batch_count_kernel<2, LAYOUT><<<groups, threads, 0, s>>>(q);
    else batch_count_kernel<4, LAYOUT><<<groups, threads, 0, s>>>(q);
}

// waves: resident waves the host sized the grid (and the scratch) for; a multiple of kWavesPerGroup
void launch_batch_count(hipStream_t s, const CountArgs& q, int CB, int layout, int waves) {
    const int groups = waves / gabatch::kWavesPerGroup;
    if (layout == gabatch::LAYOUT_STRIPE) launch_batch_count_l<gabatch::LAYOUT_STRIPE>(s, q, CB, groups);
    else launch_batch_count_l<gabatch::LAYOUT_BATCH>(s, q, CB, groups);
}

}  // namespace ga
