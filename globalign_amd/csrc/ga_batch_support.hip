// ga_batch_support.hip -- batch_support_table_kernel, batch_flow_kernel and batch_support_gather_kernel: how many of a
// pair's co-optimal alignments pair letter i of seq_1 with letter j of seq_2 (gfx950; ga_batch_support).
//
// The alignments a pair's traceback can return are the paths of the state DAG (i, j, L) from (m, n, 0) to row 0 or
// column 0 (ga_batch_count.hip).  N(i, j, L) counts the paths from a state on, F(i, j, L) the walk prefixes that reach
// it (ga_batch_support.h has the recurrence); the members that take the diagonal out of cell (i, j) are
//   support(i, j) = A_0(i, j) * N(i-1, j-1, 0),   A_0 the prefix flow leaving the cell by the diagonal.
// batch_support_table_kernel is the count kernel's stripe loop (ga_count_stripe.h) in its CountF64Keep policy: the same
// doubles in the same order, and N(i, j, 0) of every cell kept in plane 0 of the pair's step-major table
// (gabatch::rank_table_index).  batch_flow_kernel, the next launch on the stream, runs the same wavefront backwards:
// stripes right to left, rows downwards, lane 63 leading; it reads N from plane 0 and writes support to plane 1 of the
// cell's own entry, so every load and store of a step is 64 consecutive 8-byte entries and no entry is both read and
// written.  batch_support_gather_kernel then copies plane 1 to dense row-major (m, n) doubles per pair.  All three only
// read what launches before them wrote; stream order is the only ordering, and no wave waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ga_batch.h"
#include "ga_batch_layout.h"
#include "ga_batch_rank.h"
#include "ga_batch_support.h"
#include "ga_count_stripe.h"
#include "ga_device.h"
#include "ga_walk.h"

namespace ga {

// written instead of a count when a work item does not fit the launch's buffers (the planner never emits one)
constexpr double SUPPORT_BAD_ITEM = -1.0;

// What the three kernels check of a pair before they touch its words, its table or its output: the geometry covers its
// columns with only the last stripe partial, and words, table and output lie inside the launch's (ga_batch.h plans it
// so).
template <int CB, int LAYOUT>
__device__ __forceinline__ bool support_pair_fits(const SupportArgs& q, const ga_batch_item& it,
                                                  const ga_batch_words_item& ws, long long toff, long long ooff) {
    bool fits = it.m >= 2 && it.n >= 2 && it.T >= 1 && it.T <= gabatch::kMaxT && it.nstripes >= 1 &&
                (long long)64 * it.T * it.nstripes >= it.n && (long long)64 * it.T * (it.nstripes - 1) < it.n &&
                ws.tb_off >= 0 && ws.tb_off <= q.tb_words && toff >= 0 && toff <= q.table_entries && ooff >= 0 &&
                ooff <= q.support_entries;
    if (!fits) return false;
    fits = (long long)it.nstripes * ((long long)it.m + 63) * 3 * it.T * 64 <= q.table_entries - toff &&
           (long long)it.m * it.n <= q.support_entries - ooff;
    if (LAYOUT == gabatch::LAYOUT_BATCH) {
        fits = fits && (long long)((it.m + 4 / CB - 1) / (4 / CB)) * 64 * it.T * it.nstripes <= ws.tb_words &&
               ws.tb_words <= q.tb_words - ws.tb_off;
    } else {
        fits = fits && q.tc >= 1 && (long long)q.tc * (16 / CB) >= it.m &&
               (long long)((it.n + 63) / 64) * q.tc * 256 <= q.tb_words - ws.tb_off;
    }
    return fits;
}

// x of the lane to the right (lane 63: `edge`)
__device__ __forceinline__ double shl1_f64(double edge, double x) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(edge), __double2loint(x), 0x130, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(edge), __double2hiint(x), 0x130, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// One pair by one wave: support of every cell into plane 1 of the pair's table, whose plane 0 holds N(i, j, 0).
// count_pair's stripes of 64 * T columns and the same lane ownership of columns, run the other way: stripes right to
// left, and at step t = m + 62 .. 0 lane l is on row t - l + 1.  A_1(i, right) and A_0(i + 1, right) arrive from lane
// l + 1, which made that column's row one step earlier, as two 32-bit DPP wave_shl:1 moves a number; A_2 and the other
// A_0s are the lane's own previous step (gabatch::flow_lane_step).  A stripe hands its left edge, A_0(i, edge) and
// A_1(i, edge), to the next stripe's lane 63 as count_pair hands its right edge on: through LDS at edge_l while m
// fits, else (HBM) through the wave's two slices edge_g by stripe parity.
template <int T, int CB, int LAYOUT, bool HBM>
__device__ void flow_pair(int o, int tc, long long srows, const ga_batch_item& it, const uint32_t* tbw, double2* edge_l,
                          double2* edge_g, int lane, double* table) {
    using Addr = gabatch::TbAddr<CB, LAYOUT>;
    constexpr int RPW = 4 / CB;
    constexpr unsigned MASK = CB == 4 ? 0xffffffffu : (1u << (8 * CB)) - 1u;
    const int m = it.m, n = it.n;
    const int geom = LAYOUT == gabatch::LAYOUT_BATCH ? 64 * it.T * it.nstripes : tc;
    for (int s = it.nstripes - 1; s >= 0; s--) {
        const int j0 = s * 64 * T;
        const bool first = s == it.nstripes - 1;  // the rightmost stripe: nothing to its right
        // the edge column: in LDS one column read and rewritten in place (lane 63 reads a row 64 steps before lane 0
        // rewrites it), in HBM the two slices by stripe parity
        const double2* gin = edge_g + (long long)(s & 1) * srows;
        double2* gout = edge_g + (long long)((s + 1) & 1) * srows;
        // this lane's columns; one past n (the rightmost stripe's) reads column n's words, and its cell is not live:
        // it hands on zero
        int jc[T];
        unsigned cols = 0;
        int seedk = -1;
#pragma unroll
        for (int k = 0; k < T; k++) {
            const int j = j0 + lane * T + k + 1;
            jc[k] = min(j, n);
            cols |= j <= n ? 1u << k : 0u;
            seedk = j == n ? k : seedk;
        }
        gabatch::FlowLane<T> st;
        st.reset();
        // a u32 holds RPW rows of a column: `cur` the rows being worked on, `nxt` the ones below, on their way
        uint32_t cur[T], nxt[T];
#pragma unroll
        for (int k = 0; k < T; k++) {
            cur[k] = 0;
            nxt[k] = tbw[Addr::word(m, jc[k], geom)];
        }
        // lane 63: the right edge of its row, (A_0(i, edge), A_1(i, edge)), one row ahead; the rightmost stripe: zero
        double2 en = make_double2(0.0, 0.0);
        if (!first && lane == 63) en = HBM ? gin[m - 1] : edge_l[m - 1];
        for (int t = m + 62; t >= 0; t--) {
            const int i = t - lane + 1;
            const bool act = i >= 1 && i <= m;
            const double2 e = en;
            if (!first && lane == 63 && t >= 64) en = HBM ? gin[t - 64] : edge_l[t - 64];
            // (the DPPs run in every lane)
            const double in1 = shl1_f64(e.y, st.o1);  // A_1(i, right)
            const double in0 = shl1_f64(e.x, st.o0);  // A_0(i, right): the next step's diagonal
            // the first row of a group of RPW on the way down: row m, or the group's last row
            if (act && (i == m || (i & (RPW - 1)) == 0)) {
#pragma unroll
                for (int k = 0; k < T; k++) cur[k] = nxt[k];
                const int below = (i - 1) / RPW * RPW;  // the first row met of the group below
                if (below >= 1) {
#pragma unroll
                    for (int k = 0; k < T; k++) nxt[k] = tbw[Addr::word(below, jc[k], geom)];
                }
            }
            const unsigned live = act ? cols : 0u;
            // N(i - 1, j - 1, 0) of the live cells: 64 consecutive entries a column (the lane's own previous step for
            // its columns k >= 1, the left lane's last column two steps back for k = 0)
            double nv[T];
#pragma unroll
            for (int k = 0; k < T; k++)
                nv[k] = ((live >> k) & 1u) ? gabatch::support_n(table, m, T, i, j0 + lane * T + k + 1) : 0.0;
            const int sh = Addr::shift(i);
            unsigned sets[T];
#pragma unroll
            for (int k = 0; k < T; k++) sets[k] = (unsigned)sets_from_code((cur[k] >> sh) & MASK, CB, o);
            double a0[T];
            gabatch::flow_lane_step<T>(st, in0, in1, sets, live, (first && i == m) ? seedk : -1, a0);
#pragma unroll
            for (int k = 0; k < T; k++) {
                // one multiply, rounded once, with nothing to contract into
                if ((live >> k) & 1u)
                    table[gabatch::support_index(m, T, i, j0 + lane * T + k + 1)] = __dmul_rn(a0[k], nv[k]);
            }
            if (s > 0 && lane == 0 && act) {
                if (HBM) gout[i - 1] = make_double2(st.o0, st.o1);
                else edge_l[i - 1] = make_double2(st.o0, st.o1);
            }
        }
        // lane 0's edge rows are read by lane 63 of this wave in the next stripe: one wave's memory operations to an
        // address stay in order, and this wave-scope fence says so to the compiler and the memory model
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
}

template <int T, int CB, int LAYOUT>
__device__ __forceinline__ double keep_either(const SupportArgs& q, const ga_batch_item& it, bool hbm, const uint32_t* tbw,
                                              double2* edge_l, double2* edge_g, int lane, unsigned long long* table) {
    if (hbm)
        return count_pair<CountF64Keep, T, CB, LAYOUT, true>(q.o, q.tc, q.scratch_rows, it, tbw, edge_l, edge_g, lane, table);
    return count_pair<CountF64Keep, T, CB, LAYOUT, false>(q.o, q.tc, q.scratch_rows, it, tbw, edge_l, edge_g, lane, table);
}

template <int T, int CB, int LAYOUT>
__device__ __forceinline__ void flow_either(const SupportArgs& q, const ga_batch_item& it, bool hbm, const uint32_t* tbw,
                                            double2* edge_l, double2* edge_g, int lane, double* table) {
    if (hbm) flow_pair<T, CB, LAYOUT, true>(q.o, q.tc, q.scratch_rows, it, tbw, edge_l, edge_g, lane, table);
    else flow_pair<T, CB, LAYOUT, false>(q.o, q.tc, q.scratch_rows, it, tbw, edge_l, edge_g, lane, table);
}

// batch_count_kernel's ticket loop: persistent waves, one wave per pair.  FLOW: the flow pass, else the N table.
template <int CB, int LAYOUT, bool FLOW>
__device__ __forceinline__ void support_wave_loop(const SupportArgs& q, double2 (*edge_s)[gabatch::kLdsEdgeRows]) {
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
        const long long toff = q.table_off[t], ooff = q.support_off[t];
        const bool hbm = it.nstripes > 1 && it.m > gabatch::kLdsEdgeRows;
        // also: an edge column in HBM must fit this wave's slices
        const bool fits = support_pair_fits<CB, LAYOUT>(q, it, ws, toff, ooff) &&
                          !(hbm && (edge_g == nullptr || it.m > q.scratch_rows));
        const uint32_t* tbw = q.tb + (fits ? ws.tb_off : 0);
        unsigned long long* table = q.table + (fits ? toff : 0);
        if constexpr (FLOW) {
            switch (fits ? it.T : 0) {
                case 1: flow_either<1, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, (double*)table); break;
                case 2: flow_either<2, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, (double*)table); break;
                case 3: flow_either<3, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, (double*)table); break;
                case 4: flow_either<4, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, (double*)table); break;
                case 5: flow_either<5, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, (double*)table); break;
                case 6: flow_either<6, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, (double*)table); break;
                case 7: flow_either<7, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, (double*)table); break;
                case 8: flow_either<8, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, (double*)table); break;
                default: break;
            }
        } else {
            double r = SUPPORT_BAD_ITEM;
            switch (fits ? it.T : 0) {
                case 1: r = keep_either<1, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, table); break;
                case 2: r = keep_either<2, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, table); break;
                case 3: r = keep_either<3, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, table); break;
                case 4: r = keep_either<4, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, table); break;
                case 5: r = keep_either<5, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, table); break;
                case 6: r = keep_either<6, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, table); break;
                case 7: r = keep_either<7, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, table); break;
                case 8: r = keep_either<8, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, table); break;
                default: break;
            }
            // every lane stores the same value (no lane-divergent branch at an item's end, see batch_pair); an item
            // whose slot lies outside the output has nowhere to report to
            if (it.out >= 0 && it.out < q.npairs) q.count_out[it.out] = r;
        }
    }
}

template <int CB, int LAYOUT>
__global__ void __launch_bounds__(64 * gabatch::kWavesPerGroup) batch_support_table_kernel(SupportArgs q) {
    __shared__ double2 edge_s[gabatch::kWavesPerGroup][gabatch::kLdsEdgeRows];
    support_wave_loop<CB, LAYOUT, false>(q, edge_s);
}

template <int CB, int LAYOUT>
__global__ void __launch_bounds__(64 * gabatch::kWavesPerGroup) batch_flow_kernel(SupportArgs q) {
    __shared__ double2 edge_s[gabatch::kWavesPerGroup][gabatch::kLdsEdgeRows];
    support_wave_loop<CB, LAYOUT, true>(q, edge_s);
}

// Plane 1 of every pair's table to the pair's dense row-major (m, n) doubles at support_off.  blockIdx.y strides over
// the items, blockIdx.x over an item's cells; an item that does not fit is skipped (its count says so already).
template <int CB, int LAYOUT>
__global__ void __launch_bounds__(256) batch_support_gather_kernel(SupportArgs q) {
    for (int t = blockIdx.y; t < q.nitems; t += gridDim.y) {
        const ga_batch_item it = q.items[t];
        const long long toff = q.table_off[t], ooff = q.support_off[t];
        if (!support_pair_fits<CB, LAYOUT>(q, it, q.words[t], toff, ooff)) continue;
        const double* table = (const double*)(q.table + toff);
        double* out = q.support + ooff;
        const long long cells = (long long)it.m * it.n;
        for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (long long)gridDim.x * blockDim.x) {
            const int i = (int)(c / it.n) + 1, j = (int)(c % it.n) + 1;
            out[c] = table[gabatch::rank_table_index(it.m, it.T, i, j, 1)];
        }
    }
}

template <int LAYOUT>
static void launch_support_l(hipStream_t s, const SupportArgs& q, int CB, int groups, int pass, dim3 gather) {
    const int threads = 64 * gabatch::kWavesPerGroup;
    if (pass == 0) {
        if (CB == 1) batch_support_table_kernel<1, LAYOUT><<<groups, threads, 0, s>>>(q);
        else if (CB == 2) batch_support_table_kernel<2, LAYOUT><<<groups, threads, 0, s>>>(q);
        else batch_support_table_kernel<4, LAYOUT><<<groups, threads, 0, s>>>(q);
    } else if (pass == 1) {
        if (CB == 1) batch_flow_kernel<1, LAYOUT><<<groups, threads, 0, s>>>(q);
        else if (CB == 2) batch_flow_kernel<2, LAYOUT><<<groups, threads, 0, s>>>(q);
        else batch_flow_kernel<4, LAYOUT><<<groups, threads, 0, s>>>(q);
    } else {
        if (CB == 1) batch_support_gather_kernel<1, LAYOUT><<<gather, 256, 0, s>>>(q);
        else if (CB == 2) batch_support_gather_kernel<2, LAYOUT><<<gather, 256, 0, s>>>(q);
        else batch_support_gather_kernel<4, LAYOUT><<<gather, 256, 0, s>>>(q);
    }
}

static void launch_support(hipStream_t s, const SupportArgs& q, int CB, int layout, int waves, int pass, dim3 gather) {
    const int groups = waves / gabatch::kWavesPerGroup;
    if (layout == gabatch::LAYOUT_STRIPE) launch_support_l<gabatch::LAYOUT_STRIPE>(s, q, CB, groups, pass, gather);
    else launch_support_l<gabatch::LAYOUT_BATCH>(s, q, CB, groups, pass, gather);
}

// waves: resident waves the host sized the grid (and the scratch) for; a multiple of kWavesPerGroup
void launch_batch_support_table(hipStream_t s, const SupportArgs& q, int CB, int layout, int waves) {
    launch_support(s, q, CB, layout, waves, 0, dim3(1));
}

void launch_batch_flow(hipStream_t s, const SupportArgs& q, int CB, int layout, int waves) {
    launch_support(s, q, CB, layout, waves, 1, dim3(1));
}

// max_cells: the cells of the launch's largest pair
void launch_batch_support_gather(hipStream_t s, const SupportArgs& q, int CB, int layout, long long max_cells) {
    // at most 4096 blocks across the largest pair, and about 2^16 blocks in all: both grid dimensions stride
    long long bx = (max_cells + 255) / 256;
    bx = bx < 1 ? 1 : bx > 4096 ? 4096 : bx;
    long long by = 65536 / bx;
    by = by > q.nitems ? q.nitems : by;
    by = by < 1 ? 1 : by;
    launch_support(s, q, CB, layout, gabatch::kWavesPerGroup, 2, dim3((unsigned)bx, (unsigned)by));
}

}  // namespace ga
