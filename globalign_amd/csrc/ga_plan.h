// ga_plan.h -- the plan of one fill: which kernel (row scan, anti-diagonal, lane-skewed), its geometry (columns per
// lane, compute waves per workgroup, stripes, workgroups, profile rows) and, for the recompute walk's checkpointing
// fill, the checkpoint spacing that fits the memory budget and the recompute worker's LDS.  Pure integer arithmetic
// over the problem's shape, the request and a handful of knobs; no HIP, no context, no globals: built into the engine
// (enqueue_fill, ga_host.cpp) and into the host self-test, ga_host_selftest.cpp, under AddressSanitizer / UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../include/globalign_amd.h"

namespace gaplan {

constexpr int kFillRows = 16;  // ga::FROWS: rows per fill chunk (ga_host.cpp asserts the two agree)

// The problem as the planner sees it (ga_ctx's loaded problem or slab).
struct Problem {
    int64_t m = 0, n = 0;  // n: this context's columns (a slab's local ones)
    int64_t n_global = 0, col0 = 0;
    int K = 0, CB = 1, qbytes = 1, o = 0;
    int num_cu = 256;
    int qrows = 1024;  // the row scan's query-profile ring (load_problem: as many rows as fit 64 KB)
    bool slab = false;
    bool in_linked = false, out_linked = false;  // a slab's left / right edge is linked (ga_slab_link / _import)
    bool custom = false;
};

// One fill's request: a band of rows (banded traceback), the checkpointing pass, the recompute
// walk's score fill (5.8), or a pipeline slot's fill at a forced lane geometry (6).
struct Request {
    bool tb = false, full = false;  // GA_FILL_TRACEBACK | GA_FILL_FULL; GA_FILL_FULL
    bool band = false;              // fill rows r0+1 .. r0+mb only
    int64_t mb = 0;
    int64_t nc = 0;                 // a band's columns 1..nc only (0: all): the walk enters the band at column nc
    // the recompute walk's score fill: the lane kernel with its checkpoints (every stripe's right edge, the
    // staircase lane states every rc_every steps)
    bool rc = false;
    int rc_every = 0;               // 0: chosen with the stripes' geometry
    bool has_ckpt = false;          // the banded traceback's checkpointing pass (a checkpoint row buffer is present)
    // a traceback fill through the lane-skewed kernel at this geometry (TD columns per lane, NWC compute waves;
    // 0: the usual choice): the pipeline's narrow fills (align_many)
    int lane_td = 0, lane_nwc = 0;
};

constexpr bool kRcJumpDefault = false;  // the tie-to-tie walk unless GA_RC_JUMP says otherwise

// The knobs the choice reads, as numbers: parsed here and nowhere else, once per context (ga_ctx::pk), as
// gawalk::Knobs is: `get` looks a shipped knob up, `xget` one of a path that was measured and dropped.
struct Knobs {
    int T_req = 0, nwc_req = 0;  // GA_COLS_PER_LANE, GA_FILL_NWC (0: automatic)
    int diag_req = 0;            // GA_FILL_MODE: 0 automatic, 1 row scan, 2 anti-diagonal, 3 lane-skewed
    int lane_T_req = 0;          // GA_LANE_COLS_PER_LANE (0: automatic)
    int diag_T_req = 0;          // GA_DIAG_COLS_PER_LANE (0: automatic)
    // workgroups per CU the residency check may count on (GA_LANE_WG_PER_CU, tuning: 2 needs an LDS floor
    // below 80 KB, GA_FILL_LDS_FLOOR)
    int lane_wg_per_cu = 1;
    int lane_qrows = 4096;       // GA_LANE_QROWS caps the profile table (tuning: a smaller table lets two workgroups share a CU)
    bool rc_narrow = true;       // GA_RC_NARROW: unset and 1 both mean 2 columns per lane where the rule allows
    int64_t rc_budget = (int64_t)96 << 30;  // GA_RC_BUDGET_MB, in bytes
    bool rc_jump = false;        // the tie-to-tie walk is requested (experiments build): its cache is budgeted
    int64_t dev_avail = INT64_MAX / 4;  // device memory the recompute fill's checkpoints may take (dev_avail_bytes)
    template <typename Get, typename XGet>
    static Knobs parse(Get&& get, XGet&& xget) {
        Knobs kn;
        if (const char* e = get("GA_COLS_PER_LANE")) kn.T_req = atoi(e);  // tuning overrides
        if (const char* e = get("GA_FILL_NWC")) kn.nwc_req = atoi(e);
        if (const char* e = get("GA_FILL_MODE"))
            kn.diag_req = !strcmp(e, "diag") ? 2 : !strcmp(e, "row") ? 1 : !strcmp(e, "lane") ? 3 : 0;
        if (const char* e = get("GA_LANE_COLS_PER_LANE")) kn.lane_T_req = atoi(e);
        if (const char* e = get("GA_DIAG_COLS_PER_LANE")) kn.diag_T_req = atoi(e);
        if (const char* e = get("GA_LANE_WG_PER_CU")) kn.lane_wg_per_cu = std::max(1, std::min(2, atoi(e)));
        if (const char* e = get("GA_LANE_QROWS")) kn.lane_qrows = atoi(e);
        if (const char* e = get("GA_RC_NARROW")) kn.rc_narrow = atoi(e) != 0;
        if (const char* e = get("GA_RC_BUDGET_MB")) kn.rc_budget = atoll(e) << 20;
        // whether the tie-to-tie walk may run (GA_RC_JUMP): the checkpoint sizing then budgets its cache
        const char* e = xget("GA_RC_JUMP");
        kn.rc_jump = e ? atoi(e) != 0 : kRcJumpDefault;
        return kn;
    }
};

// The kernels' LDS formulas and the walk's cache size: defined beside the kernels (ga_lane.hip, ga_rcwalk.hip) and
// in ga_host.cpp, handed in so that this header stays free of HIP.
struct LdsSizes {
    size_t (*fill_lane_lds_bytes)(int nwc, int K, int qrows) = nullptr;
    int (*rc_worker_bytes)(int TD, int CB, int every) = nullptr;
    size_t (*rc_cache_bytes)(bool jump, int TD, int CB) = nullptr;
};

enum Kind { kRow = 0, kDiag = 1, kLane = 2 };

struct FillPlan {
    int kind = kRow;
    int T = 1;         // columns per lane (a stripe = one compute wave = 64*T columns)
    int nwc = 4;       // compute waves per workgroup
    int nstripes = 0;
    int nslabs = 0;    // workgroups
    int TC = 0;        // 16-byte traceback words per lane per 64-column stripe: 16-row chunks x CB
    int qrows = 1024;  // rows of the LDS query profile
    int rc_every = 64; // the recompute fill's checkpoint spacing
    int err = GA_OK;   // GA_E_*: no fill at this plan
    const char* msg = nullptr;
};

// Stripe geometry: T columns per lane (a stripe = one compute wave = 64*T columns).
// Blocked stripes pay the wave scan, the edge traffic and the control once per 64*T cells, but
// leave fewer stripes (waves) to fill the chip and lengthen each row's dependent chain.  A
// workgroup chains 4 waves (one per SIMD) when every stripe gets a wave that way, else 8.
inline void set_stripes(const Problem& pb, const Knobs& kn, FillPlan& pl, int T_req, bool tb, bool full,
                        int64_t ncols = -1) {
    const int64_t ncol = ncols < 0 ? pb.n : ncols;  // a traceback band may cover a prefix of the columns
    const int64_t simds = 4 * (int64_t)pb.num_cu;
    // register budget (no spills, see the code objects' vgpr_spill_count): the FULL debug output is
    // T == 1 only; traceback words T <= 2; score only T <= 8 with an int8 profile, 4 with int16
    const int cap = full ? 1 : tb ? 2 : (pb.qbytes == 2 ? 4 : 8);
    int T = 1;
    if (T_req == 1 || T_req == 2 || T_req == 4 || T_req == 8) {
        T = std::min(T_req, cap);
    } else {
        // the widest stripes that still leave >= 1.5 waves per SIMD (measured: 1M columns score
        // only T = 8 > 4 > 2 > 1; 100k columns with traceback T = 1 > 2 > 4)
        for (int t = cap; t > 1; t /= 2)
            if ((ncol + 64 * t - 1) / (64 * t) * 2 >= 3 * simds) {
                T = t;
                break;
            }
    }
    // a slab with a right neighbour hands column n on: its last stripe must be whole (T == 1
    // takes the edge from any lane)
    while (T > 1 && pb.col0 + pb.n < pb.n_global && pb.n % (64 * T) != 0) T /= 2;
    pl.T = T;
    pl.nstripes = (int)((ncol + 64 * T - 1) / (64 * T));
    pl.nwc = kn.nwc_req == 4 || kn.nwc_req == 8 ? kn.nwc_req : pl.nstripes <= 4 * pb.num_cu ? 4 : 8;
    pl.nslabs = (pl.nstripes + pl.nwc - 1) / pl.nwc;
}

// The row-scan geometry of a loaded problem: a context's plan before its first fill.
inline FillPlan row_plan(const Problem& pb, const Knobs& kn) {
    FillPlan pl;
    pl.qrows = pb.qrows;
    set_stripes(pb, kn, pl, kn.T_req, false, false);
    return pl;
}

// Lane-skewed fill geometry: TD columns per lane, NWC compute waves per workgroup,
// every stripe resident at once (a stripe waits on its left neighbour only, so the whole chain must
// run concurrently).  The cost model is the measured step of tools/micro/lane_bench.hip (cycles per
// step per wave at one / two waves per SIMD, with the kernel's per-step LDS traffic and the DPP
// shift-register output) times the chain's length, m steps plus ~74 steps of skew per stripe.
// Returns false (row scan), leaving the plan as it was, when no geometry is allowed or the profile table
// does not fit beside the rings.
inline bool lane_geometry(const Problem& pb, const Knobs& kn, const LdsSizes& lds, FillPlan& pl, int64_t ncol, bool tb,
                          int force_T = 0, int force_N = 0, int qrows_cap = 0) {
    if (pb.qbytes != 1 || pb.K > 32) return false;
    // Cycles per step per wave measured in the kernel (score only, 16-step sub-chunks; tools/lane_stamps.py,
    // tools/exp/lane_sub.sh, tools/exp/c4_pack.sh): one wave per SIMD (4-wave workgroups) 84 / 115 / 154 /
    // 239 at TD = 1 / 2 / 4 / 8; two waves per SIMD (8-wave workgroups) about 2.1x that per wave, the
    // partner's issue plus the chain coupling (C4: 243 ms against 207 for 1-wave rounds).
    static const double cyc1[4] = {84, 115, 154, 239};
    int64_t cus = pb.num_cu * kn.lane_wg_per_cu;
    // A slab whose edge another kernel (an RCCL receive or send) must move WHILE the fill runs: keep one CU
    // of every shader engine (8 CUs) free and every workgroup resident.  A kernel launched beside the fill
    // places each of its workgroups on a CU of one shader engine, round robin, and waits there: measured
    // (tools/exp/r3_cores.py), an RCCL-shaped kernel starts beside 224 fill workgroups on 256 CUs, not
    // beside 228.  Linked edges (ga_slab_link / _import: the fill stores them itself) need no room.
    const bool coresident = pb.slab && ((pb.col0 > 0 && !pb.in_linked) ||
                                        (pb.col0 + pb.n < pb.n_global && !pb.out_linked));
    if (coresident) cus = pb.num_cu - pb.num_cu / 8;
    // Rounds: with 4-wave workgroups, one per CU, more stripes than 4 per CU run in rounds of workgroups.
    // A later round starts as the first finish, on left edges long written, so it runs uncoupled; the
    // chain then takes R*m + skew steps at the 1-wave step cost.  Not for a slab with a right neighbour
    // (its last stripe, in the last round, would hold the next GPU back by the earlier rounds).
    const bool right_nb = pb.col0 + pb.n < pb.n_global;
    int bestT = 0, bestN = 0;
    double best = 0;
    for (int ti = 0; ti < 4; ti++) {
        const int T = 1 << ti;
        if (force_T ? force_T != T : kn.lane_T_req && kn.lane_T_req != T) continue;
        // traceback windows (register budget, ga_lane.hip lane_variant_ok): TD <= 4 with one-byte
        // words, <= 2 with two- and four-byte words (four-byte: 4 waves per workgroup)
        if (tb && T > (pb.CB == 1 ? 4 : 2)) continue;
        // a slab with a right neighbour hands column n on: its last stripe must be whole
        if (right_nb && ncol % (64 * T) != 0) continue;
        const int64_t ns = (ncol + 64 * T - 1) / (64 * T);
        for (int nwc : {4, 8}) {
            if (force_N ? force_N != nwc : (kn.nwc_req == 4 || kn.nwc_req == 8) && nwc != kn.nwc_req) continue;
            if (tb && pb.CB == 4 && nwc == 8) continue;
            const int64_t rounds = (ns + nwc * cus - 1) / (nwc * cus);
            if (rounds > 1 && (nwc == 8 || right_nb || tb || coresident)) continue;  // 8-wave workgroups: all resident
            const double step = nwc == 4 ? cyc1[ti] : 2.1 * cyc1[ti];
            const double t = ((double)rounds * (double)pb.m + 74.0 * (double)ns) * step;
            if (!bestT || t < best) {
                best = t;
                bestT = T;
                bestN = nwc;
            }
        }
    }
    if (!bestT) return false;
    const size_t budget = 150 * 1024;
    int qr = std::max(256, std::min(4096, qrows_cap > 0 ? qrows_cap : kn.lane_qrows));
    while (qr > 256 && lds.fill_lane_lds_bytes(bestN, pb.K, qr) > budget) qr >>= 1;
    if (lds.fill_lane_lds_bytes(bestN, pb.K, qr) > budget || qr < bestN * 64 + 192) return false;
    pl.T = bestT;
    pl.nwc = bestN;
    pl.nstripes = (int)((ncol + 64 * bestT - 1) / (64 * bestT));
    pl.nslabs = (pl.nstripes + pl.nwc - 1) / pl.nwc;
    pl.qrows = qr;
    return true;
}

inline FillPlan plan_error(FillPlan pl, int code, const char* msg) {
    pl.err = code;
    pl.msg = msg;
    return pl;
}

// The recompute walk's score fill: the lane kernel's geometry, then the checkpoint spacing.
inline FillPlan plan_rc_fill(const Problem& pb, const Request& rq, const Knobs& kn, const LdsSizes& lds, FillPlan pl,
                             int64_t m, int64_t n) {
    if (rq.tb || rq.full || !lane_geometry(pb, kn, lds, pl, n, false))
        return plan_error(pl, GA_E_STATE, "recompute fill needs the lane kernel");
    // the checkpointing variant runs 16-step sub-chunks (8 waves at TD = 8 would take 8-step ones)
    if (pl.nwc == 8 && pl.T == 8 && !lane_geometry(pb, kn, lds, pl, n, false, 8, 4))
        return plan_error(pl, GA_E_STATE, "recompute fill geometry");
    // the recompute workers stage a block's codes in LDS (64*TD columns x the checkpoint spacing): at
    // wide stripes and wide spacings (C4: TD 8, every 256 steps, 219 KB) that exceeds the CU's LDS, so
    // the stripes narrow until a worker fits beside the walk's 128 KB torus budget
    constexpr int kRcLds = 256 * 256 * 2;  // the walk's torus (ga_walk.h TP x TP u16): the launch's dynamic LDS
    // Stripes of at most 4 columns per lane (unless GA_LANE_COLS_PER_LANE asks): a block is 64 rows of one stripe, and the walk reads ~1-2 of
    // its TD tiles, so wider blocks starve the walk (C4 on one GPU at TD 8: fill 226 ms, walk 160 ms;
    // at TD 4: 284 + 90 ms, tools/exp/r3b_c4tb3.sh, r3b_c4rc.py)
    // and 4 where the geometry model chose fewer (round 4, the lean sub-chunk): fewer, wider stripes shorten
    // the ramp as much as their slower step lengthens the rows, and the walk's blocks come cheaper (C3: fill
    // 9.69 -> 9.81 ms, walk 5.72 -> 5.42; C5 3.92 against 6.3 ms at TD = 1; tools/r4_td.sh).
    // Round 6: with the lean ramp (the first 64 steps no longer masked) and the cone-shaped recompute window
    // below, 2 columns per lane win for small alphabets whose stripes all run at once (one workgroup of four per
    // CU): C3 fill 7.61 -> 6.83 ms, walk 5.18 -> 5.03 (cone 2; 5.65 with the round-5 window), call 12.98 ->
    // 12.09; C2 1.42 -> 1.30.  The protein fill does not (C5 at TD 2: fill 1.73 -> 1.91 ms), so K > 8 keeps 4
    // (tools/exp/r6/check5.sh, check6.sh, rc_diag.py).  The default under those conditions:
    // GA_RC_NARROW=0 restores 4 columns per lane for an A/B run, =1 and unset both mean 2; slabs, K > 8 and
    // problems with more 128-column stripes than SIMDs (C4) keep 4; GA_LANE_COLS_PER_LANE overrides both.
    if (!kn.lane_T_req) {
        const bool td2 = kn.rc_narrow && !pb.slab && pb.K <= 8 && (n + 127) / 128 <= 4 * (int64_t)pb.num_cu;
        if (td2 && lane_geometry(pb, kn, lds, pl, n, false, 2, 4)) {
        } else if (pl.T > 4) {
            if (!lane_geometry(pb, kn, lds, pl, n, false, 4, 4)) return plan_error(pl, GA_E_STATE, "recompute fill geometry");
        } else if (pl.T < 4) {
            (void)lane_geometry(pb, kn, lds, pl, n, false, 4, 4);
        }
    }
    // The checkpoint spacing, with the stripes' geometry known: the smallest (<= 4096 steps) whose states
    // fit the memory budget (default 96 GB of the 288: C4 on one GPU, TD 4, takes 128 steps, 78 GB; 64
    // would take 156 GB and walks no faster) and whose worker fits LDS; GA_RC_EVERY fixes it (the stripes
    // narrow if it must)
    // The budget is also capped by the device memory free for it: what hipMemGetInfo reports plus
    // what this context's checkpoint buffers already hold, less the right-edge columns (8 B per row per
    // stripe), the walk's tile cache and a 2 GB margin.  A problem whose checkpoints still do not fit returns
    // GA_E_NOMEM, and ga_problem_align takes the banded traceback instead.
    const int64_t budget = kn.rc_budget;
    auto ck_bytes = [&](int e) {
        const int64_t nck = std::max<int64_t>((m - 1) / e, 1);
        return nck * pl.nstripes * (pl.T + 1) * 512;
    };
    // (the walk's block cache as the walk that will run sizes it: ADVICE r5, the jump cache is ~6x the word one)
    auto other_bytes = [&]() {
        return (int64_t)pl.nstripes * (m + 1) * 8 + (int64_t)lds.rc_cache_bytes(kn.rc_jump && pl.T <= 4, pl.T, pb.CB) +
               ((int64_t)64 << 20);
    };
    auto fits = [&](int e) {
        return ck_bytes(e) <= std::min(budget, kn.dev_avail - other_bytes()) &&
               1024 + lds.rc_worker_bytes(pl.T, pb.CB, e) <= kRcLds;
    };
    int every = pl.rc_every;
    for (;;) {
        if (rq.rc_every > 0) every = rq.rc_every;
        else
            for (every = 64; every < 4096 && !fits(every); every *= 2) {}
        if (1024 + lds.rc_worker_bytes(pl.T, pb.CB, every) <= kRcLds) break;
        if (pl.T == 1) {
            // no spacing fits both: memory if the densest one fits LDS, else LDS
            if (1024 + lds.rc_worker_bytes(1, pb.CB, 64) <= kRcLds)
                return plan_error(pl, GA_E_NOMEM, "recompute walk: the checkpoints do not fit the budget / free device memory");
            return plan_error(pl, GA_E_RANGE, "recompute walk: a block's codes do not fit LDS");
        }
        if (!lane_geometry(pb, kn, lds, pl, n, false, pl.T / 2, 4)) return plan_error(pl, GA_E_STATE, "recompute fill geometry");
    }
    if (ck_bytes(every) > std::min(budget, kn.dev_avail - other_bytes()))
        return plan_error(pl, GA_E_NOMEM, "recompute walk: the checkpoints do not fit the budget / free device memory");
    pl.rc_every = every;
    pl.kind = kLane;
    return pl;
}

// The plan of one fill, or its error (FillPlan::err, ::msg): nothing is enqueued for a plan that failed.
inline FillPlan plan_fill(const Problem& pb, const Request& rq, const Knobs& kn, const LdsSizes& lds) {
    FillPlan pl;
    pl.rc_every = rq.rc_every > 0 ? rq.rc_every : 64;  // (chosen by plan_rc_fill for a recompute fill)
    const bool tb = rq.tb, full = rq.full;
    const int64_t m = rq.band ? rq.mb : pb.m, n = rq.band && rq.nc > 0 ? rq.nc : pb.n;
    if (full && (m + 1) * (n + 1) > (int64_t)64 << 20) return plan_error(pl, GA_E_RANGE, "GA_FILL_FULL is for small problems");
    // 16-row chunks; CB 16-byte words per lane per chunk (ga_device.h)
    pl.TC = (int)((m + kFillRows - 1) / kFillRows) * pb.CB;
    pl.qrows = pb.qrows;
    if (rq.rc) return plan_rc_fill(pb, rq, kn, lds, pl, m, n);
    // score only: the lane-skewed kernel when its chain's skew (~74 steps per stripe)
    // is short against the m rows every stripe walks (measured: 1M x 125k 60 ms against 107 for the row
    // scan, C4 244 against 312; 100k x 100k, whose 782 stripes add 58k steps of skew, 13.5 against 12.6)
    bool lane = false, diag = false;
    if (rq.lane_td > 0 && tb && !full && !rq.has_ckpt)
        lane = lane_geometry(pb, kn, lds, pl, n, tb, rq.lane_td, rq.lane_nwc, 2048);
    else if (!full && (!rq.has_ckpt || !tb) && (kn.diag_req == 3 || (kn.diag_req == 0 && !tb)) &&
             lane_geometry(pb, kn, lds, pl, n, tb) && (kn.diag_req == 3 || 4 * 74 * (int64_t)pl.nstripes <= m))
        lane = true;
    // score only: the anti-diagonal kernel (64-column stripes) when asked for and its profile
    // ring is deep enough for a workgroup's skew (NWC stripes x 64*TD steps).
    // automatic: score-only fills of tall problems on one GPU (m >= 4 n, <= 8 stripes per CU).
    // Measured (profiles/r01/diag_sweep.txt): 1M x 125k 80 ms (TD = 1) against 107 ms for the row
    // scan, 1M x 250k 126 ms (TD = 2) against 141 ms; the row scan wins on square shapes (C4 313 ms
    // against 400 ms), where the anti-diagonal skew of 64 steps per stripe costs more.  Not for a
    // slab of a multi-GPU fill: there the next rank starts when this one's last stripe does, and
    // that start (the ramp) is ~15 ms for the anti-diagonal fill against ~3 ms for the row scan.
    const int auto_td = (n + 63) / 64 <= 8 * (int64_t)pb.num_cu ? 1 : 2;
    const bool auto_diag = kn.diag_req == 0 && !tb && !rq.band && !pb.slab && m >= 4 * n &&
                           (n + 64 * auto_td - 1) / (64 * auto_td) <= 8 * (int64_t)pb.num_cu;
    if (!lane && (!tb || (full && pb.qbytes == 1)) && (kn.diag_req == 2 || auto_diag) && !rq.has_ckpt) {
        int td = full ? std::min(std::max(kn.diag_T_req, 1), 2)
                      : kn.diag_T_req == 1 || kn.diag_T_req == 2 || kn.diag_T_req == 4 ? kn.diag_T_req
                      : auto_diag ? auto_td : 1;
        if (pb.qbytes == 2) td = std::min(td, 2);  // int16 profiles at TD = 4 spill
        set_stripes(pb, kn, pl, td, false, false, n);
        if (full) {  // the debug FULL variant is built for 4 compute waves
            pl.nwc = 4;
            pl.nslabs = (pl.nstripes + 3) / 4;
        }
        pl.qrows = 8192;
        while (pl.qrows > 128 && (size_t)pb.K * (pl.qrows + 16) * pb.qbytes > 64 * 1024) pl.qrows >>= 1;
        diag = pl.qrows >= pl.nwc * (64 * pl.T + 16) + 64 * pl.T + 64;
    }
    if (!diag && !lane) {
        pl.qrows = pb.qrows;
        set_stripes(pb, kn, pl, kn.T_req, tb, full, n);
    }
    pl.kind = lane ? kLane : diag ? kDiag : kRow;
    return pl;
}

// The kernels' two LDS formulas written out with their constants, for the self-test, which has no kernels to ask.
// ga_ctx_create_opts checks them against the kernels' own functions, so a change there cannot pass unnoticed.
// ga_lane.hip:104 fill_lane_lds_bytes: LK_HEAD_BYTES (256 counters + 16 zero rows + 64 scratch slots of 8 B = 896)
// + (nwc + 1) rings of RING = 256 int2 rows + K x (qrows + LK_QMIRROR = 16) dwords of profile + K x 32 B of sub'
inline size_t restated_fill_lane_lds_bytes(int nwc, int K, int qrows) {
    return (size_t)896 + (size_t)(nwc + 1) * 256 * 8 + (size_t)K * (qrows + 16) * 4 + (size_t)K * 32;
}
// ga_rcwalk.hip:35-39 rc_sp, rc_aw, rc_worker_bytes: 64*TD columns of stage bytes, the a-window and the edge window
inline int restated_rc_worker_bytes(int TD, int CB, int every) {
    const int sp = (((every + 136) * CB + 16) + 15) & ~15, aw = every + 256;
    return 64 * TD * sp + aw * 4 + aw * 8;
}

}  // namespace gaplan
