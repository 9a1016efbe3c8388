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
// Persistent waves take pairs off a ticket word of their own; a wave counts a pair with the stripe loop of
// ga_count_stripe.h (count_pair) in its double policy, CountF64: IEEE double additions only, the selected terms in the
// order T0, T1, T2, so the result is bit for bit what the recurrence gives in double anywhere, exact below 2^53, +inf
// past the double range and never NaN.  batch_rank_table_kernel (ga_batch_rank.hip) runs the same loop in u64.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ga_batch.h"
#include "ga_batch_layout.h"
#include "ga_count_stripe.h"
#include "ga_device.h"
#include "ga_walk.h"

namespace ga {

// written instead of a count when a work item does not fit the launch's buffers (the planner never emits one)
constexpr double COUNT_BAD_ITEM = -1.0;

template <int T, int CB, int LAYOUT>
__device__ __forceinline__ double count_either(const CountArgs& q, const ga_batch_item& it, bool hbm, const uint32_t* tbw,
                                               double2* edge_l, double2* edge_g, int lane) {
    if (hbm) return count_pair<CountF64, T, CB, LAYOUT, true>(q.o, q.tc, q.scratch_rows, it, tbw, edge_l, edge_g, lane);
    return count_pair<CountF64, T, CB, LAYOUT, false>(q.o, q.tc, q.scratch_rows, it, tbw, edge_l, edge_g, lane);
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
