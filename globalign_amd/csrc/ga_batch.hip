// ga_batch.hip -- batch_fill_kernel: many score-only alignments in one launch, one wave per pair (gfx950).
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
#include "ga_device.h"
#include "ga_row.h"

namespace ga {

struct BatchArgs {
    const uint8_t* codes;        // every sequence's codes, concatenated
    const ga_batch_item* items;  // the work list
    int nitems;
    const int* subp;             // K x K: sub' = sub - gV - gH
    const int* gh;               // K: horizontal gap costs
    const int* gv;               // K: vertical gap costs
    int K, o;
    unsigned* ticket;            // zeroed by the host ahead of every launch
    long long* cost_out;         // [npairs], indexed by ga_batch_item::out
    int2* scratch;               // [waves][2][scratch_rows] edge columns (nullptr: no pair needs them)
    long long scratch_rows;
};

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

// HBM: the pair's edge column lies in the wave's HBM slices (m above the LDS share and more than one stripe), else
// in LDS; a template parameter, so that every edge access has one address space (a run-time choice let the compiler
// merge the two stores into one flat store through a selected pointer).
template <typename QT, int T, bool HBM>
__device__ void batch_pair(const BatchArgs& p, const ga_batch_item& it, const QT* tab, const int* gh_s, const int* gv_s,
                           int2* edge_l, int2* edge_g, int lane) {
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
                if (partial) {
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

// waves: resident waves the host sized the grid (and the scratch) for; a multiple of kWavesPerGroup
void launch_batch_fill(hipStream_t s, const uint8_t* codes, const ga_batch_item* items, int nitems, const int* subp,
                       const int* gh, const int* gv, int K, int o, int qbytes, unsigned* ticket, long long* cost_out,
                       int2* scratch, long long scratch_rows, int waves) {
    BatchArgs p{codes, items, nitems, subp, gh, gv, K, o, ticket, cost_out, scratch, scratch_rows};
    const int groups = waves / gabatch::kWavesPerGroup;
    if (qbytes == 1)
        batch_fill_kernel<int8_t><<<groups, 64 * gabatch::kWavesPerGroup, 0, s>>>(p);
    else if (qbytes == 2)
        batch_fill_kernel<int16_t><<<groups, 64 * gabatch::kWavesPerGroup, 0, s>>>(p);
    else
        batch_fill_kernel<int32_t><<<groups, 64 * gabatch::kWavesPerGroup, 0, s>>>(p);
}

}  // namespace ga
