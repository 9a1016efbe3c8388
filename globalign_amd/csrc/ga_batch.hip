// ga_batch.hip -- batch_fill_kernel: many score-only alignments in one launch, one wave per pair (gfx950), and
// batch_align_kernel (further down): the same with traceback words and the traceback walk, for alignment strings;
// batch_words_kernel and batch_walks_kernel (after it): that fill and that walk as two launches, many walks per fill.
//
// For each pair this replaces make_dp_array (globaligner.py:756-821), dp_array_forward (:366-392) and the min of
// the last cell (:425) -- what the single-pair path spreads over the boundary launches and a fill -- in the shifted
// int32 arithmetic of DESIGN.md 3, bit-identical to bnd_edges_kernel + the fills (ga_kernels.hip).
//
// Persistent waves: each wave takes the next pair of the host's work list (ga_batch.h, longest first) through an
// agent-scope ticket and walks it alone.  A pair is cut into stripes of 64 * T columns (T chosen per pair from n);
// lane l owns T adjacent columns and the wave steps down the rows with the row scan's recurrence (ga_row.h
// blocked_row: U = min(M', Y'), one DPP prefix-min across the lanes, X' = V~(j-1) + o).  Row 0 comes from a wave
// prefix sum of the stripe's horizontal gap costs, column 0 from a prefix sum of each 64-row chunk's vertical ones.
// Stripes run left to right in the same wave: row i's right edge (H'(i-1), V~(i)) goes to the wave's edge column
// (LDS while m fits, else a ping-pong slice of HBM scratch only this wave touches) and the next stripe reads it
// back a 64-row chunk at a time.  Waves never wait for each other: the only workgroup-wide step is the table load.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ga_batch.h"
#include "ga_batch_layout.h"
#include "ga_device.h"
#include "ga_row.h"
#include "ga_walk.h"

namespace ga {

// what a masked column contributes to the prefix-min: above every value the range guard admits (|v| < 2^29), and
// INF + o still clear of overflow
constexpr int BATCH_INF = 0x3f000000;
// written instead of a cost when a work item does not fit the launch's buffers (the planner never emits one)
constexpr long long BATCH_BAD_ITEM = INT64_MIN;

template <int CTRL, int ROWMASK>
__device__ __forceinline__ int dpp_add(int x) {
    return x + __builtin_amdgcn_update_dpp(0, x, CTRL, ROWMASK, 0xf, false);
}
// inclusive prefix sum over the wave (the steps of wave_scan_min)
__device__ __forceinline__ int wave_scan_add(int x) {
    x = dpp_add<0x111, 0xf>(x);
    x = dpp_add<0x112, 0xf>(x);
    x = dpp_add<0x114, 0xf>(x);
    x = dpp_add<0x118, 0xf>(x);
    x = dpp_add<0x142, 0xa>(x);
    x = dpp_add<0x143, 0xc>(x);
    return x;
}

// blocked_row for the stripe that holds column n: columns past n stay in the DPP (an exec-masked DPP would read
// stale lanes) and contribute BATCH_INF to the prefix-min instead.
template <int T>
__device__ __forceinline__ void masked_row(int (&Hprev)[T], int (&Yc)[T], int eh, int ev, const int (&sub)[T], int o,
                                           const bool (&ok)[T], int& oH, int& oV) {
    int U[T], P[T];
    const int M0 = shr1(eh, Hprev[T - 1]) + sub[0];  // the DPP itself runs in every lane
    U[0] = ok[0] ? min(M0, Yc[0]) : BATCH_INF;
#pragma unroll
    for (int k = 1; k < T; k++) U[k] = ok[k] ? min(Hprev[k - 1] + sub[k], Yc[k]) : BATCH_INF;
    P[0] = U[0];
#pragma unroll
    for (int k = 1; k < T; k++) P[k] = min(P[k - 1], U[k]);
    const int Wv = min(wave_scan_min(P[T - 1]), ev);
    const int C = shr1(ev, Wv);
    oH = Hprev[T - 1];
    oV = Wv;
    int Vl = C;
#pragma unroll
    for (int k = 0; k < T; k++) {
        const int H = min(U[k], Vl + o);
        if (k + 1 < T) Vl = min(C, P[k]);
        Yc[k] = min(Yc[k], H + o);
        Hprev[k] = H;
    }
}

// masked_row with the cells' traceback codes (blocked_row's, W-bit fields): the twin batch_align_kernel uses
template <int T, int CB>
__device__ __forceinline__ void masked_row_tb(int (&Hprev)[T], int (&Yc)[T], int eh, int ev, const int (&sub)[T], int o,
                                              unsigned op1, const bool (&ok)[T], unsigned (&code)[T], int& oH, int& oV) {
    constexpr int W = (8 * CB - 1) / 2;
    int M[T], U[T], P[T];
    M[0] = shr1(eh, Hprev[T - 1]) + sub[0];  // the DPP itself runs in every lane
#pragma unroll
    for (int k = 1; k < T; k++) M[k] = Hprev[k - 1] + sub[k];
#pragma unroll
    for (int k = 0; k < T; k++) U[k] = ok[k] ? min(M[k], Yc[k]) : BATCH_INF;
    P[0] = U[0];
#pragma unroll
    for (int k = 1; k < T; k++) P[k] = min(P[k - 1], U[k]);
    const int Wv = min(wave_scan_min(P[T - 1]), ev);
    const int C = shr1(ev, Wv);
    oH = Hprev[T - 1];
    oV = Wv;
    int Vl = C;
#pragma unroll
    for (int k = 0; k < T; k++) {
        const int X = Vl + o;
        const int H = min(U[k], X);
        // (a column past n: garbage nobody reads)
        code[k] = min((unsigned)(X - H), op1) | (min((unsigned)(Yc[k] - H), op1) << W) |
                  (min((unsigned)(M[k] - H), 1u) << (2 * W));
        if (k + 1 < T) Vl = min(C, P[k]);
        Yc[k] = min(Yc[k], H + o);
        Hprev[k] = H;
    }
}

// HBM: the pair's edge column lies in the wave's HBM slices (m above the LDS share and more than one stripe), else
// in LDS; a template parameter, so that every edge access has one address space (a run-time choice let the compiler
// merge the two stores into one flat store through a selected pointer).
// CB > 0 (batch_align_kernel): every cell's CB-byte traceback word also goes to tbw, the wave's slice of traceback
// scratch, 4 / CB rows of a column to a u32 and rows of u32s npitch = 64 * T * nstripes apart (ga_batch.h).  Columns
// past n are stored too (garbage nobody reads): the pitch covers them.
template <typename QT, int T, bool HBM, int CB = 0>
__device__ void batch_pair(const BatchArgs& p, const ga_batch_item& it, const QT* tab, const int* gh_s, const int* gv_s,
                           int2* edge_l, int2* edge_g, int lane, uint32_t* tbw = nullptr) {
    const int m = it.m, n = it.n, o = p.o, K = p.K, big = it.big;
    const uint8_t* a = p.codes + it.a_off;
    const uint8_t* b = p.codes + it.b_off;
    const long long srows = p.scratch_rows;
    int ghc = 0;     // GH(j0): the horizontal gap costs left of the stripe
    int gvm = 0;     // GV(m), from the first stripe
    int Hlast = 0;   // H'(m, n)
    for (int s = 0; s < it.nstripes; s++) {
        const int j0 = s * 64 * T;
        const bool last = s == it.nstripes - 1;
        const bool partial = j0 + 64 * T > n;
        // the edge column: in LDS one column read and rewritten in place (a chunk's rows are read before the first
        // of them is rewritten), in HBM the two slices by stripe parity
        const int2* gin = edge_g + (long long)(s & 1) * srows;
        int2* gout = edge_g + (long long)((s + 1) & 1) * srows;
        // this lane's columns j0 + lane * T + 1 .. + T, and row 0 of them as bnd_edges_kernel derives it from
        // (M, X, Y) = (big, o + GH(j), big)
        int bc[T], Hprev[T], Yc[T];
        bool ok[T];
        int run = 0;
#pragma unroll
        for (int k = 0; k < T; k++) {
            const int jc = j0 + lane * T + k + 1;
            ok[k] = jc <= n;
            bc[k] = ok[k] ? (int)b[jc - 1] : 0;
            run += ok[k] ? gh_s[bc[k]] : 0;
            Yc[k] = run;  // the lane's own prefix, for now
        }
        const int incl = wave_scan_add(run);
        const int base = ghc + incl - run;
#pragma unroll
        for (int k = 0; k < T; k++) {
            const int GH = base + Yc[k];
            const int X = o + GH;
            const int H = min(min(big, X), big);
            const int h2 = min(big, H + o);
            Hprev[k] = H - GH;
            Yc[k] = h2 - GH;
        }
        ghc += __builtin_amdgcn_readlane(incl, 63);  // columns past n add 0: GH(n) after the last stripe
        int gvc = 0;     // GV(i0)
        int lxp = 0;     // left[i0].x = H'(i0, 0) (row 0: the corner, 0)
        // CB > 0: the u32s of this lane's columns being packed, and where the next ones go
        constexpr int RPW = CB > 0 ? 4 / CB : 1;
        [[maybe_unused]] uint32_t cur[T];
        [[maybe_unused]] uint32_t* tbrow = nullptr;
        if constexpr (CB > 0) {
#pragma unroll
            for (int k = 0; k < T; k++) cur[k] = 0;
            tbrow = tbw + j0 + lane * T;
        }
        for (int i0 = 0; i0 < m; i0 += 64) {
            const int rows = min(64, m - i0);
            const int i = i0 + lane + 1;
            const bool rv = i <= m;
            const int ac = rv ? (int)a[i - 1] : 0;
            // lane r: what row i0 + r + 1 needs from the stripe's left edge, (H'(i-1, edge), V~(i, edge))
            int eH, eV;
            if (s == 0) {
                // column 0, from (M, X, Y) = (big, big, o + GV(i)); V~ = h1' - o
                const int GV = gvc + wave_scan_add(rv ? gv_s[ac] : 0);
                const int Y = o + GV;
                const int H = min(min(big, big), Y);
                const int h1 = min(big, H + o);
                const int Lx = H - GV;
                eH = shr1(lxp, Lx);
                eV = h1 - GV - o;
                gvc = __builtin_amdgcn_readlane(GV, 63);  // rows past m add 0: GV(m) after the last chunk
                lxp = __builtin_amdgcn_readlane(Lx, 63);
            } else {
                int2 e = make_int2(0, 0);
                if (rv) e = HBM ? gin[i - 1] : edge_l[i - 1];
                eH = e.x;
                eV = e.y;
            }
            int sub[T];
            {
                const QT* trow = tab + __builtin_amdgcn_readlane(ac, 0) * K;
#pragma unroll
                for (int k = 0; k < T; k++) sub[k] = (int)trow[bc[k]];
            }
            for (int r = 0; r < rows; r++) {
                // the next row's sub' first: its LDS latency runs beside this row's chain
                int subn[T];
                const QT* trow = tab + __builtin_amdgcn_readlane(ac, min(r + 1, 63)) * K;
#pragma unroll
                for (int k = 0; k < T; k++) subn[k] = (int)trow[bc[k]];
                const int eh = __builtin_amdgcn_readlane(eH, r), ev = __builtin_amdgcn_readlane(eV, r);
                int oH, oV;
                if constexpr (CB > 0) {
                    const unsigned op1 = (unsigned)o + 1u;
                    unsigned code[T];
                    if (partial) {
                        masked_row_tb<T, CB>(Hprev, Yc, eh, ev, sub, o, op1, ok, code, oH, oV);
                    } else {
                        uint32_t acc[T][4 * CB];
#pragma unroll
                        for (int k = 0; k < T; k++) acc[k][0] = 0;
                        blocked_row<T, true, CB>(Hprev, Yc, eh, ev, sub, o, op1, 0, acc, oH, oV);
#pragma unroll
                        for (int k = 0; k < T; k++) code[k] = acc[k][0];
                    }
                    // (i0 is a multiple of 64, so r alone gives the row's place in its u32)
                    const int q = r & (RPW - 1);
#pragma unroll
                    for (int k = 0; k < T; k++) cur[k] |= code[k] << (q * 8 * CB);
                    if (q == RPW - 1 || r == rows - 1) {
#pragma unroll
                        for (int k = 0; k < T; k++) {
                            tbrow[k] = cur[k];
                            cur[k] = 0;
                        }
                        tbrow += 64 * T * it.nstripes;
                    }
                } else if (partial) {
                    masked_row<T>(Hprev, Yc, eh, ev, sub, o, ok, oH, oV);
                } else {
                    uint32_t acc[T][4];
                    blocked_row<T, false, 1>(Hprev, Yc, eh, ev, sub, o, 0u, 0, acc, oH, oV);
                }
                if (!last && lane == 63) {
                    if (HBM) gout[i0 + r] = make_int2(oH, oV);
                    else edge_l[i0 + r] = make_int2(oH, oV);
                }
#pragma unroll
                for (int k = 0; k < T; k++) sub[k] = subn[k];
            }
        }
        if (s == 0) gvm = gvc;
        // lane 63's edge rows are read by every lane of this wave in the next stripe: one wave's memory operations
        // to an address stay in order, and this wave-scope fence says so to the compiler and the memory model
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (last) {
            const int ke_l = (n - 1 - j0) / T, ke_k = (n - 1 - j0) % T;
            int v = Hprev[0];
#pragma unroll
            for (int k = 1; k < T; k++)
                if (k == ke_k) v = Hprev[k];
            Hlast = __builtin_amdgcn_readlane(v, ke_l);
        }
    }
    // un-shift: cost = H'(m, n) + GV(m) + GH(n).  Every lane stores the same value to the same word (one write).
    // A store under `lane == 0` here was threaded into the ticket's `lane == 0` at the loop head (jump threading,
    // seen with AMD clang 22.0.0git of ROCm 7.2.0), which made the persistent loop's back edge divergent: lanes
    // 1..63 went round on their own with ticket 0.  With no lane-divergent branch at the end of a pair there is
    // nothing to thread, whatever the optimiser does.
    p.cost_out[it.out] = (long long)Hlast + gvm + ghc;
}

template <typename QT, int T>
__device__ __forceinline__ void pair_either(const BatchArgs& p, const ga_batch_item& it, bool hbm, const QT* tab,
                                            const int* gh_s, const int* gv_s, int2* edge_l, int2* edge_g, int lane) {
    if (hbm) batch_pair<QT, T, true>(p, it, tab, gh_s, gv_s, edge_l, edge_g, lane);
    else batch_pair<QT, T, false>(p, it, tab, gh_s, gv_s, edge_l, edge_g, lane);
}

template <typename QT>
__global__ void __launch_bounds__(64 * gabatch::kWavesPerGroup) batch_fill_kernel(BatchArgs p) {
    __shared__ QT tab[gabatch::kLdsTableBytes / sizeof(QT)];
    __shared__ int gh_s[256], gv_s[256];
    __shared__ int2 edge_s[gabatch::kWavesPerGroup][gabatch::kLdsEdgeRows];
    const int K = p.K;
    for (int q = threadIdx.x; q < K * K; q += blockDim.x) tab[q] = (QT)p.subp[q];
    for (int q = threadIdx.x; q < K; q += blockDim.x) {
        gh_s[q] = p.gh[q];
        gv_s[q] = p.gv[q];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long gw = (long long)blockIdx.x * gabatch::kWavesPerGroup + w;
    int2* edge_g = p.scratch ? p.scratch + gw * 2 * p.scratch_rows : nullptr;
    for (;;) {
        // the only lane-divergent branch of the loop; the wave is whole again at the readfirstlane
        unsigned t = 0;
        if (lane == 0) t = __hip_atomic_fetch_add(p.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
        if (t >= (unsigned)p.nitems) break;
        const ga_batch_item it = p.items[t];
        // an edge column in HBM must fit this wave's slices (ga_batch.h plans it so)
        const bool fits =
            !(it.nstripes > 1 && it.m > gabatch::kLdsEdgeRows && (edge_g == nullptr || it.m > p.scratch_rows));
        const bool hbm = it.nstripes > 1 && it.m > gabatch::kLdsEdgeRows;
        switch (fits ? it.T : 0) {
            case 1: pair_either<QT, 1>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane); break;
            case 2: pair_either<QT, 2>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane); break;
            case 3: pair_either<QT, 3>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane); break;
            case 4: pair_either<QT, 4>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane); break;
            case 5: pair_either<QT, 5>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane); break;
            case 6: pair_either<QT, 6>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane); break;
            case 7: pair_either<QT, 7>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane); break;
            case 8: pair_either<QT, 8>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane); break;
            default: p.cost_out[it.out] = BATCH_BAD_ITEM;  // (every lane, as batch_pair's cost)
        }
    }
}

// ------------------------------------------------------------------ batch_align_kernel
// Alignments with strings: the same persistent ticket loop, and per pair the fill above with its
// traceback words kept, then the traceback walk (dp_array_backward, globaligner.py:395-593) by the same wave, from
// (m, n) to row 0 or column 0, under the pair's own tie-break table.  The work list holds only pairs with
// min(m, n) >= 2: their walks stay inside the matrix (no first-step quirk, no IndexError).

// The walk of one pair by one wave.  Groups of up to 7 steps: one vector load per lane fetches the 8 x 8 window
// anchored at the current cell (lane r * 8 + c: cell (i - r, j - c), clamped at row / column 1 -- a clamped cell is
// never walked, the walk ends where it would be needed) and every lane decodes its cell into the three 5-bit table
// shifts of walk_body's cached cells; the steps then run on scalars, each reading its cell with a uniform-index
// v_readlane.  Every step lowers i + j and the walk ends at i == 0 or j == 0, so it makes at most m + n - 1 steps
// whatever the words and the table hold.  The words are read with vector loads only (the scalar cache could hold a
// previous pair's lines of this slice), after the fence that follows the fill's stores.
// LAYOUT (ga_batch_layout.h): where a cell's word lies in tbw -- LAYOUT_BATCH, batch_pair's words, or LAYOUT_STRIPE,
// a single-pair fill's at `tc` 16-byte words per lane (batch_walks_kernel's large route).
template <int CB, int LAYOUT = gabatch::LAYOUT_BATCH>
__device__ int4 batch_walk(const AlignArgs& q, const ga_batch_item& it, const ga_batch_walk_item& wi,
                           const uint32_t* tbw, int lane, int tc = 0) {
    using Addr = gabatch::TbAddr<CB, LAYOUT>;
    constexpr unsigned MASK = CB == 4 ? 0xffffffffu : (1u << (8 * CB)) - 1u;
    const int m = it.m, n = it.n, o = q.b.o;
    const int geom = LAYOUT == gabatch::LAYOUT_BATCH ? 64 * it.T * it.nstripes : tc, total = m + n;
    const uint8_t* a = q.b.codes + it.a_off;
    const uint8_t* b = q.b.codes + it.b_off;
    const uint32_t* tab = q.rng + wi.tab_off;
    uint32_t* ops = q.ops + wi.ops_off;
    const int lr = lane >> 3, lc = lane & 7;
    int i = m, j = n, D = 0;
    unsigned L5 = 0, opsw = 0;  // 5 * the level the walk entered the cell with; the level word being packed
    while (i > 0 && j > 0 && D < total) {
        const int ci = max(i - lr, 1), cj = max(j - lc, 1);
        const uint32_t wd = tbw[Addr::word(ci, cj, geom)];
        const unsigned code = (wd >> Addr::shift(ci)) & MASK;
        const int shf = (int)cell_shifts(sets_from_code(code, CB, o), a[ci - 1] == b[cj - 1]);
        const int tv = (int)tab[min(D + (lane & 7), total - 1)];  // lane s: the entry of the group's step s
        int di = 0, dj = 0;
#pragma unroll
        for (int s = 0; s < 7; s++) {
            const unsigned v = (unsigned)__builtin_amdgcn_readlane(shf, di * 8 + dj);
            const unsigned t = (unsigned)__builtin_amdgcn_readlane(tv, s);
            const unsigned lvl = (t >> (((v >> L5) & 31u) + 3u)) & 3u;
            opsw |= lvl << (30 - 2 * (D & 15));
            // every lane stores the same word (no lane-divergent branch in the persistent loop, see batch_pair)
            if ((D & 15) == 15) {
                ops[D >> 4] = opsw;
                opsw = 0;
            }
            D++;
            di += lvl != 1u;
            dj += lvl != 2u;
            L5 = 5u * lvl;
            if (di == i || dj == j || D >= total) break;
        }
        i -= di;
        j -= dj;
    }
    if (D & 15) ops[D >> 4] = opsw;
    // reason as walk_body's: 1 the walk ended in row 0, 2 in column 0 (0: in the corner, no tail either way)
    return make_int4(D, i, j, i == 0 ? (j == 0 ? 0 : 1) : 2);
}

template <typename QT, int T, int CB>
__device__ __forceinline__ void align_pair_either(const BatchArgs& p, const ga_batch_item& it, bool hbm, const QT* tab,
                                                  const int* gh_s, const int* gv_s, int2* edge_l, int2* edge_g, int lane,
                                                  uint32_t* tbw) {
    if (hbm) batch_pair<QT, T, true, CB>(p, it, tab, gh_s, gv_s, edge_l, edge_g, lane, tbw);
    else batch_pair<QT, T, false, CB>(p, it, tab, gh_s, gv_s, edge_l, edge_g, lane, tbw);
}

template <typename QT, int CB>
__global__ void __launch_bounds__(64 * gabatch::kWavesPerGroup) batch_align_kernel(AlignArgs q) {
    __shared__ QT tab[gabatch::kLdsTableBytes / sizeof(QT)];
    __shared__ int gh_s[256], gv_s[256];
    __shared__ int2 edge_s[gabatch::kWavesPerGroup][gabatch::kLdsEdgeRows];
    const BatchArgs& p = q.b;
    const int K = p.K;
    for (int x = threadIdx.x; x < K * K; x += blockDim.x) tab[x] = (QT)p.subp[x];
    for (int x = threadIdx.x; x < K; x += blockDim.x) {
        gh_s[x] = p.gh[x];
        gv_s[x] = p.gv[x];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long gw = (long long)blockIdx.x * gabatch::kWavesPerGroup + w;
    int2* edge_g = p.scratch ? p.scratch + gw * 2 * p.scratch_rows : nullptr;
    uint32_t* tbw = q.tb + gw * q.tb_words;
    for (;;) {
        unsigned t = 0;
        if (lane == 0) t = __hip_atomic_fetch_add(p.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
        if (t >= (unsigned)p.nitems) break;
        const ga_batch_item it = p.items[t];
        const ga_batch_walk_item wi = q.witems[t];
        const bool hbm = it.nstripes > 1 && it.m > gabatch::kLdsEdgeRows;
        // the edge column and the traceback words must fit this wave's slices, and the walk needs two letters a side
        // (ga_batch.h plans it so)
        const bool fits = !(hbm && (edge_g == nullptr || it.m > p.scratch_rows)) && it.m >= 2 && it.n >= 2 &&
                          it.T >= 1 && it.T <= gabatch::kMaxT &&
                          (long long)((it.m + 4 / CB - 1) / (4 / CB)) * 64 * it.T * it.nstripes <= q.tb_words &&
                          (long long)64 * it.T * it.nstripes >= it.n;
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        switch (fits ? it.T : 0) {
            case 1: align_pair_either<QT, 1, CB>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane, tbw); break;
            case 2: align_pair_either<QT, 2, CB>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane, tbw); break;
            case 3: align_pair_either<QT, 3, CB>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane, tbw); break;
            case 4: align_pair_either<QT, 4, CB>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane, tbw); break;
            case 5: align_pair_either<QT, 5, CB>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane, tbw); break;
            case 6: align_pair_either<QT, 6, CB>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane, tbw); break;
            case 7: align_pair_either<QT, 7, CB>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane, tbw); break;
            case 8: align_pair_either<QT, 8, CB>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane, tbw); break;
            default: p.cost_out[it.out] = BATCH_BAD_ITEM;  // (every lane, as batch_pair's cost)
        }
        // the fill's words, stored by this wave's lanes, are read by other lanes of the wave: one wave's memory
        // operations to an address stay in order (the edge column's fence, batch_pair)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (fits) {
            const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
            const int4 end = batch_walk<CB>(q, it, wi, tbw, lane);
            const unsigned long long t2 = __builtin_amdgcn_s_memrealtime();
            // every lane stores the same words (no lane-divergent branch in the loop, see batch_pair)
            q.walk_out[2 * (long long)it.out] = end;
            q.walk_out[2 * (long long)it.out + 1] = make_int4((int)(t1 - t0), (int)(t2 - t1), 0, 0);
        }
    }
}

// ------------------------------------------------------------------ batch_words_kernel, batch_walks_kernel
// Many seeded walks of a pair from one fill (ga_batch_sample).  batch_words_kernel is
// batch_align_kernel's ticket loop with the fill only: every pair's words go to the pair's own slice of the chunk's
// scratch and stay there.  batch_walks_kernel, a later launch on the same stream, has one work item per sample: a wave
// takes an item, finds its pair and walks the pair's words under the sample's table.  The order between the two is
// stream order and nothing else: no wave waits for another, the words are read-only in the walks kernel.

template <typename QT, int CB>
__global__ void __launch_bounds__(64 * gabatch::kWavesPerGroup) batch_words_kernel(WordsArgs q) {
    __shared__ QT tab[gabatch::kLdsTableBytes / sizeof(QT)];
    __shared__ int gh_s[256], gv_s[256];
    __shared__ int2 edge_s[gabatch::kWavesPerGroup][gabatch::kLdsEdgeRows];
    const BatchArgs& p = q.b;
    const int K = p.K;
    for (int x = threadIdx.x; x < K * K; x += blockDim.x) tab[x] = (QT)p.subp[x];
    for (int x = threadIdx.x; x < K; x += blockDim.x) {
        gh_s[x] = p.gh[x];
        gv_s[x] = p.gv[x];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long gw = (long long)blockIdx.x * gabatch::kWavesPerGroup + w;
    int2* edge_g = p.scratch ? p.scratch + gw * 2 * p.scratch_rows : nullptr;
    for (;;) {
        unsigned t = 0;
        if (lane == 0) t = __hip_atomic_fetch_add(p.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
        if (t >= (unsigned)p.nitems) break;
        const ga_batch_item it = p.items[t];
        const ga_batch_words_item ws = q.words[t];
        const bool hbm = it.nstripes > 1 && it.m > gabatch::kLdsEdgeRows;
        // the edge column must fit this wave's slices and the traceback words the pair's own slice, which must lie
        // inside the chunk's words; the walks need two letters a side (ga_batch.h plans it so)
        const bool fits = !(hbm && (edge_g == nullptr || it.m > p.scratch_rows)) && it.m >= 2 && it.n >= 2 &&
                          it.T >= 1 && it.T <= gabatch::kMaxT && it.nstripes >= 1 &&
                          (long long)((it.m + 4 / CB - 1) / (4 / CB)) * 64 * it.T * it.nstripes <= ws.tb_words &&
                          (long long)64 * it.T * it.nstripes >= it.n && ws.tb_off >= 0 &&
                          ws.tb_off <= q.tb_words && ws.tb_words <= q.tb_words - ws.tb_off;
        uint32_t* tbw = q.tb + (fits ? ws.tb_off : 0);
        switch (fits ? it.T : 0) {
            case 1: align_pair_either<QT, 1, CB>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane, tbw); break;
            case 2: align_pair_either<QT, 2, CB>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane, tbw); break;
            case 3: align_pair_either<QT, 3, CB>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane, tbw); break;
            case 4: align_pair_either<QT, 4, CB>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane, tbw); break;
            case 5: align_pair_either<QT, 5, CB>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane, tbw); break;
            case 6: align_pair_either<QT, 6, CB>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane, tbw); break;
            case 7: align_pair_either<QT, 7, CB>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane, tbw); break;
            case 8: align_pair_either<QT, 8, CB>(p, it, hbm, tab, gh_s, gv_s, edge_s[w], edge_g, lane, tbw); break;
            default: p.cost_out[it.out] = BATCH_BAD_ITEM;  // (every lane, as batch_pair's cost)
        }
    }
}

template <int CB, int LAYOUT>
__global__ void __launch_bounds__(64 * gabatch::kWavesPerGroup) batch_walks_kernel(WalksArgs q) {
    const int lane = threadIdx.x & 63;
    // batch_walk reads the codes, the gap-open cost, the tables and the level words out of an AlignArgs
    AlignArgs aq{};
    aq.b.codes = q.codes;
    aq.b.o = q.o;
    aq.rng = q.rng;
    aq.ops = q.ops;
    for (;;) {
        // the only lane-divergent branch of the loop; the wave is whole again at the readfirstlane
        unsigned t = 0;
        if (lane == 0) t = __hip_atomic_fetch_add(q.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
        if (t >= (unsigned)q.nwalk) break;
        const ga_batch_sample_item wi = q.witems[t];
        const bool known = wi.fill >= 0 && wi.fill < q.nfill;
        const ga_batch_item it = q.items[known ? wi.fill : 0];
        const ga_batch_words_item ws = q.words[known ? wi.fill : 0];
        const long long steps = (long long)it.m + it.n;
        // the pair's codes, the walk's table entries and level words, and the pair's words must lie inside the
        // launch's buffers (ga_batch.h plans it so); a walk needs two letters a side
        bool fits = known && it.m >= 2 && it.n >= 2 && it.a_off >= 0 && it.b_off >= 0 &&
                    (long long)it.a_off + it.m <= q.ncodes && (long long)it.b_off + it.n <= q.ncodes &&
                    wi.tab_off >= 0 && wi.tab_off <= q.rng_entries && steps <= q.rng_entries - wi.tab_off &&
                    wi.ops_off >= 0 && wi.ops_off <= q.ops_words && (steps + 15) / 16 <= q.ops_words - wi.ops_off &&
                    ws.tb_off >= 0 && ws.tb_off <= q.tb_words;
        if (LAYOUT == gabatch::LAYOUT_BATCH) {
            fits = fits && it.T >= 1 && it.T <= gabatch::kMaxT && it.nstripes >= 1 &&
                   (long long)64 * it.T * it.nstripes >= it.n &&
                   (long long)((it.m + 4 / CB - 1) / (4 / CB)) * 64 * it.T * it.nstripes <= ws.tb_words &&
                   ws.tb_words <= q.tb_words - ws.tb_off;
        } else {
            fits = fits && q.tc >= 1 && (long long)q.tc * (16 / CB) >= it.m &&
                   (long long)((it.n + 63) / 64) * q.tc * 256 <= q.tb_words - ws.tb_off;
        }
        int4 end = make_int4(-1, 0, 0, 0);
        int ticks = 0;
        if (fits) {
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
            end = batch_walk<CB, LAYOUT>(aq, it, ga_batch_walk_item{wi.tab_off, wi.ops_off}, q.tb + ws.tb_off, lane, q.tc);
            ticks = (int)(__builtin_amdgcn_s_memrealtime() - t0);
        }
        // every lane stores the same words (no lane-divergent branch at an item's end, see batch_pair)
        q.walk_out[2 * (long long)t] = end;
        q.walk_out[2 * (long long)t + 1] = make_int4(0, ticks, 0, 0);
    }
}

template <typename QT>
static void launch_batch_words_q(hipStream_t s, const WordsArgs& q, int CB, int groups) {
    const int threads = 64 * gabatch::kWavesPerGroup;
    if (CB == 1) batch_words_kernel<QT, 1><<<groups, threads, 0, s>>>(q);
    else if (CB == 2) batch_words_kernel<QT, 2><<<groups, threads, 0, s>>>(q);
    else batch_words_kernel<QT, 4><<<groups, threads, 0, s>>>(q);
}

void launch_batch_words(hipStream_t s, const WordsArgs& q, int qbytes, int CB, int waves) {
    const int groups = waves / gabatch::kWavesPerGroup;
    if (qbytes == 1) launch_batch_words_q<int8_t>(s, q, CB, groups);
    else if (qbytes == 2) launch_batch_words_q<int16_t>(s, q, CB, groups);
    else launch_batch_words_q<int32_t>(s, q, CB, groups);
}

template <int LAYOUT>
static void launch_batch_walks_l(hipStream_t s, const WalksArgs& q, int CB, int groups) {
    const int threads = 64 * gabatch::kWavesPerGroup;
    if (CB == 1) batch_walks_kernel<1, LAYOUT><<<groups, threads, 0, s>>>(q);
    else if (CB == 2) batch_walks_kernel<2, LAYOUT><<<groups, threads, 0, s>>>(q);
    else batch_walks_kernel<4, LAYOUT><<<groups, threads, 0, s>>>(q);
}

void launch_batch_walks(hipStream_t s, const WalksArgs& q, int CB, int layout, int waves) {
    const int groups = waves / gabatch::kWavesPerGroup;
    if (layout == gabatch::LAYOUT_STRIPE) launch_batch_walks_l<gabatch::LAYOUT_STRIPE>(s, q, CB, groups);
    else launch_batch_walks_l<gabatch::LAYOUT_BATCH>(s, q, CB, groups);
}

template <typename QT>
static void launch_batch_align_q(hipStream_t s, const AlignArgs& q, int CB, int groups) {
    const int threads = 64 * gabatch::kWavesPerGroup;
    if (CB == 1) batch_align_kernel<QT, 1><<<groups, threads, 0, s>>>(q);
    else if (CB == 2) batch_align_kernel<QT, 2><<<groups, threads, 0, s>>>(q);
    else batch_align_kernel<QT, 4><<<groups, threads, 0, s>>>(q);
}

void launch_batch_align(hipStream_t s, const AlignArgs& q, int qbytes, int CB, int waves) {
    const int groups = waves / gabatch::kWavesPerGroup;
    if (qbytes == 1) launch_batch_align_q<int8_t>(s, q, CB, groups);
    else if (qbytes == 2) launch_batch_align_q<int16_t>(s, q, CB, groups);
    else launch_batch_align_q<int32_t>(s, q, CB, groups);
}

// waves: resident waves the host sized the grid (and the scratch) for; a multiple of kWavesPerGroup
void launch_batch_fill(hipStream_t s, const BatchArgs& p, int qbytes, int waves) {
    const int groups = waves / gabatch::kWavesPerGroup;
    if (qbytes == 1)
        batch_fill_kernel<int8_t><<<groups, 64 * gabatch::kWavesPerGroup, 0, s>>>(p);
    else if (qbytes == 2)
        batch_fill_kernel<int16_t><<<groups, 64 * gabatch::kWavesPerGroup, 0, s>>>(p);
    else
        batch_fill_kernel<int32_t><<<groups, 64 * gabatch::kWavesPerGroup, 0, s>>>(p);
}

}  // namespace ga
