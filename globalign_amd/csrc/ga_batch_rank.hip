// ga_batch_rank.hip -- batch_rank_table_kernel and batch_rank_walk_kernel: co-optimal alignments by rank (gfx950;
// ga_batch_rank).
//
// The alignments a pair's traceback can return are the paths of the state DAG (i, j, L) from (m, n, 0) to row 0 or
// column 0 (ga_batch_count.hip).  Numbered in the order of their level sequences (ga_batch_rank.h), path r is found by
// unranking: at every tie the walk enters the branch whose path count contains r.  batch_rank_table_kernel keeps the
// per-state counts that batch_count_kernel computes and drops: the same stripe loop (ga_count_stripe.h) in u64 that
// saturates at 2^64 - 1, every interior cell's N(i, j, 0 .. 2) stored to the pair's table.  batch_rank_walk_kernel
// then walks a pair once per requested rank, one LANE per walk: a work item is up to 64 consecutive slots of one
// pair, all starting at (m, n) and sharing the path until their ranks part, so their early loads coalesce by
// themselves.  Both kernels are later launches on the stream that filled the words (batch_words_kernel, or the
// single-pair fill for a large pair) and only read what the launches before them wrote, with vector loads.  Stream
// order is the only ordering: no wave waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ga_batch.h"
#include "ga_batch_layout.h"
#include "ga_batch_rank.h"
#include "ga_count_stripe.h"
#include "ga_device.h"
#include "ga_walk.h"

namespace ga {

// written instead of a count when a work item does not fit the launch's buffers (the planner never emits one; a count
// is at least 1)
constexpr unsigned long long RANK_BAD_ITEM = 0ull;

// What both kernels check of a pair before they touch its words or its table: the geometry covers its columns with
// only the last stripe partial, and the words and the table lie inside the launch's (ga_batch.h plans it so).
template <int CB, int LAYOUT>
__device__ __forceinline__ bool rank_pair_fits(const ga_batch_item& it, const ga_batch_words_item& ws, long long toff,
                                               long long tb_words, int tc, long long table_entries) {
    bool fits = it.m >= 2 && it.n >= 2 && it.T >= 1 && it.T <= gabatch::kMaxT && it.nstripes >= 1 &&
                (long long)64 * it.T * it.nstripes >= it.n && (long long)64 * it.T * (it.nstripes - 1) < it.n &&
                ws.tb_off >= 0 && ws.tb_off <= tb_words && toff >= 0 && toff <= table_entries;
    if (!fits) return false;
    fits = (long long)it.nstripes * ((long long)it.m + 63) * 3 * it.T * 64 <= table_entries - toff;
    if (LAYOUT == gabatch::LAYOUT_BATCH) {
        fits = fits && (long long)((it.m + 4 / CB - 1) / (4 / CB)) * 64 * it.T * it.nstripes <= ws.tb_words &&
               ws.tb_words <= tb_words - ws.tb_off;
    } else {
        fits = fits && tc >= 1 && (long long)tc * (16 / CB) >= it.m &&
               (long long)((it.n + 63) / 64) * tc * 256 <= tb_words - ws.tb_off;
    }
    return fits;
}

template <int T, int CB, int LAYOUT>
__device__ __forceinline__ unsigned long long table_either(const RankTableArgs& q, const ga_batch_item& it, bool hbm,
                                                           const uint32_t* tbw, ulonglong2* edge_l, ulonglong2* edge_g,
                                                           int lane, unsigned long long* table) {
    if (hbm)
        return count_pair<CountU64Sat, T, CB, LAYOUT, true>(q.o, q.tc, q.scratch_rows, it, tbw, edge_l, edge_g, lane, table);
    return count_pair<CountU64Sat, T, CB, LAYOUT, false>(q.o, q.tc, q.scratch_rows, it, tbw, edge_l, edge_g, lane, table);
}

// batch_count_kernel's ticket loop: persistent waves, one wave per pair.
template <int CB, int LAYOUT>
__global__ void __launch_bounds__(64 * gabatch::kWavesPerGroup) batch_rank_table_kernel(RankTableArgs q) {
    __shared__ ulonglong2 edge_s[gabatch::kWavesPerGroup][gabatch::kLdsEdgeRows];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long gw = (long long)blockIdx.x * gabatch::kWavesPerGroup + w;
    ulonglong2* edge_g = q.scratch ? q.scratch + gw * 2 * q.scratch_rows : nullptr;
    for (;;) {
        // the only lane-divergent branch of the loop; the wave is whole again at the readfirstlane
        unsigned t = 0;
        if (lane == 0) t = __hip_atomic_fetch_add(q.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
        if (t >= (unsigned)q.nitems) break;
        const ga_batch_item it = q.items[t];
        const ga_batch_words_item ws = q.words[t];
        const long long toff = q.table_off[t];
        const bool hbm = it.nstripes > 1 && it.m > gabatch::kLdsEdgeRows;
        // also: an edge column in HBM must fit this wave's slices
        const bool fits = rank_pair_fits<CB, LAYOUT>(it, ws, toff, q.tb_words, q.tc, q.table_entries) &&
                          !(hbm && (edge_g == nullptr || it.m > q.scratch_rows));
        const uint32_t* tbw = q.tb + (fits ? ws.tb_off : 0);
        unsigned long long* table = q.table + (fits ? toff : 0);
        unsigned long long r = RANK_BAD_ITEM;
        switch (fits ? it.T : 0) {
            case 1: r = table_either<1, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, table); break;
            case 2: r = table_either<2, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, table); break;
            case 3: r = table_either<3, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, table); break;
            case 4: r = table_either<4, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, table); break;
            case 5: r = table_either<5, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, table); break;
            case 6: r = table_either<6, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, table); break;
            case 7: r = table_either<7, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, table); break;
            case 8: r = table_either<8, CB, LAYOUT>(q, it, hbm, tbw, edge_s[w], edge_g, lane, table); break;
            default: break;
        }
        // every lane stores the same value (no lane-divergent branch at an item's end, see batch_pair); an item
        // whose slot lies outside the output has nowhere to report to
        if (it.out >= 0 && it.out < q.npairs) q.count_out[it.out] = r;
    }
}

// One lane per walk.  A lane's walk for rank r starts at (m, n, 0); at a state it loads its cell's word, decodes S_L,
// and only when more than one move is selected loads the counts it needs from the pair's table (rank_choose,
// ga_batch_rank.h).  The level goes into the lane's own level word, batch_walk's format, stored every 16 steps to the
// lane's own slice of the item's level words.  A walk ends at i == 0, j == 0 or after m + n dispatches: every step
// lowers i + j, so a lane makes at most m + n - 1 steps whatever the words and the table hold, and every load is of a
// cell with 1 <= i <= m and 1 <= j <= n, inside the pair's words and table.  The wave's loop runs while any lane walks.
template <int CB, int LAYOUT>
__global__ void __launch_bounds__(64 * gabatch::kWavesPerGroup) batch_rank_walk_kernel(RankWalkArgs q) {
    using Addr = gabatch::TbAddr<CB, LAYOUT>;
    constexpr unsigned MASK = CB == 4 ? 0xffffffffu : (1u << (8 * CB)) - 1u;
    const int lane = threadIdx.x & 63;
    for (;;) {
        unsigned t = 0;
        if (lane == 0) t = __hip_atomic_fetch_add(q.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
        if (t >= (unsigned)q.nwalk) break;
        const ga_batch_rank_item wi = q.witems[t];
        const bool known = wi.fill >= 0 && wi.fill < q.nfill;
        const ga_batch_item it = q.items[known ? wi.fill : 0];
        const ga_batch_words_item ws = q.words[known ? wi.fill : 0];
        const long long toff = q.table_off[known ? wi.fill : 0];
        const int m = it.m, n = it.n, T = it.T;
        const long long wps = ((long long)m + n + 15) / 16;
        // the item's slots must have their ranks, results and level words inside the launch's
        const bool placed = wi.nslots >= 1 && wi.nslots <= 64 && wi.res >= 0 && (long long)wi.res + wi.nslots <= q.nslots;
        const bool fits = known && placed && rank_pair_fits<CB, LAYOUT>(it, ws, toff, q.tb_words, q.tc, q.table_entries) &&
                          wi.out >= 0 && (long long)wi.out + wi.nslots <= q.nranks && wi.ops_off >= 0 &&
                          wi.ops_off <= q.ops_words && wps * wi.nslots <= q.ops_words - wi.ops_off;
        const bool mine = placed && lane < wi.nslots;
        const int geom = LAYOUT == gabatch::LAYOUT_BATCH ? 64 * T * it.nstripes : q.tc;
        const uint32_t* tbw = q.tb + (fits ? ws.tb_off : 0);
        const unsigned long long* tab = q.table + (fits ? toff : 0);
        uint32_t* ops = q.ops + (fits ? wi.ops_off + lane * wps : 0);
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        int i = m, j = n, D = 0, L = 0, status = fits ? gabatch::kRankOk : gabatch::kRankBadItem;
        unsigned opsw = 0;
        unsigned long long r = 0;
        bool walking = fits && mine;
        if (walking) {
            r = q.ranks[wi.out + lane];
            // a rank at or above the pair's count draws no walk: N(m, n, 0) is the first state's count
            if (r >= tab[gabatch::rank_table_index(m, T, m, n, 0)]) {
                status = gabatch::kRankOutOfRange;
                walking = false;
            }
        }
        while (walking) {
            const unsigned code = (tbw[Addr::word(i, j, geom)] >> Addr::shift(i)) & MASK;
            const unsigned S = ((unsigned)sets_from_code(code, CB, q.o) >> (3 * L)) & 7u;
            const int lvl = gabatch::rank_choose(S, r, [&](int k) -> unsigned long long {
                const int pi = i - (k != 1), pj = j - (k != 2);
                return (pi == 0 || pj == 0) ? 1ull : tab[gabatch::rank_table_index(m, T, pi, pj, k)];
            });
            opsw |= (unsigned)lvl << (30 - 2 * (D & 15));
            if ((D & 15) == 15) {
                ops[D >> 4] = opsw;
                opsw = 0;
            }
            D++;
            i -= lvl != 1;
            j -= lvl != 2;
            L = lvl;
            walking = i > 0 && j > 0 && D < m + n;
        }
        if (fits && mine && status == gabatch::kRankOk && (D & 15)) ops[D >> 4] = opsw;
        const int ticks = (int)(__builtin_amdgcn_s_memrealtime() - t0);
        if (mine) {
            // reason as batch_walk's: 1 the walk ended in row 0, 2 in column 0 (0: in the corner)
            q.walk_out[2 * ((long long)wi.res + lane)] = make_int4(D, i, j, i == 0 ? (j == 0 ? 0 : 1) : 2);
            q.walk_out[2 * ((long long)wi.res + lane) + 1] = make_int4(status, lane == 0 ? ticks : 0, 0, 0);
        }
    }
}

template <int LAYOUT>
static void launch_rank_table_l(hipStream_t s, const RankTableArgs& q, int CB, int groups) {
    const int threads = 64 * gabatch::kWavesPerGroup;
    if (CB == 1) batch_rank_table_kernel<1, LAYOUT><<<groups, threads, 0, s>>>(q);
    else if (CB == 2) batch_rank_table_kernel<2, LAYOUT><<<groups, threads, 0, s>>>(q);
    else batch_rank_table_kernel<4, LAYOUT><<<groups, threads, 0, s>>>(q);
}

template <int LAYOUT>
static void launch_rank_walk_l(hipStream_t s, const RankWalkArgs& q, int CB, int groups) {
    const int threads = 64 * gabatch::kWavesPerGroup;
    if (CB == 1) batch_rank_walk_kernel<1, LAYOUT><<<groups, threads, 0, s>>>(q);
    else if (CB == 2) batch_rank_walk_kernel<2, LAYOUT><<<groups, threads, 0, s>>>(q);
    else batch_rank_walk_kernel<4, LAYOUT><<<groups, threads, 0, s>>>(q);
}

// waves: resident waves the host sized the grid (and the scratch) for; a multiple of kWavesPerGroup
void launch_batch_rank_table(hipStream_t s, const RankTableArgs& q, int CB, int layout, int waves) {
    const int groups = waves / gabatch::kWavesPerGroup;
    if (layout == gabatch::LAYOUT_STRIPE) launch_rank_table_l<gabatch::LAYOUT_STRIPE>(s, q, CB, groups);
    else launch_rank_table_l<gabatch::LAYOUT_BATCH>(s, q, CB, groups);
}

void launch_batch_rank_walk(hipStream_t s, const RankWalkArgs& q, int CB, int layout, int waves) {
    const int groups = waves / gabatch::kWavesPerGroup;
    if (layout == gabatch::LAYOUT_STRIPE) launch_rank_walk_l<gabatch::LAYOUT_STRIPE>(s, q, CB, groups);
    else launch_rank_walk_l<gabatch::LAYOUT_BATCH>(s, q, CB, groups);
}

}  // namespace ga
