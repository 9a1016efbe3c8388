// ga_walk_plan.h -- the pure part of one alignment's traceback (ga_problem_align): its knobs as
// numbers, which path the call takes (the recompute walk, banded traceback, the streamed or the plain walk of stored
// words) and the recompute walk's launch figures (the ranked window of candidate blocks, workers, workgroups).  No HIP,
// no context, no globals: built into the engine (ga_align_host.cpp) and into ga_host_selftest.cpp under ASan / UBSan.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <cstdlib>
#include <optional>
#include <utility>
#include <vector>

#include "ga_check.h"
#include "ga_plan.h"

namespace gawalk {

// ga_device.h's RC_SPAN_I / RC_SPAN_S and RcArgs::off's length (ga_align_host.cpp asserts they agree)
constexpr int kSpanI = 32, kSpanS = 8, kWindow = 64;

// The knobs of the traceback call, parsed here and nowhere else, once per context (ga_ctx::wk): `get` looks a shipped
// knob up, `xget` one of a path that was measured and dropped (ga_ctx_create_opts' two look-ups: the shipped build's xget sees
// nothing); nullptr for an unset name.
struct Knobs {
    int rc = -1;                            // GA_RC: 0 never, 1 whenever the shape allows (tests), else large problems
    std::optional<int64_t> rc_min_cells;    // GA_RC_MIN_CELLS (unset: rc_eligible's default per call)
    int rc_every = 0;                       // GA_RC_EVERY (checked in ga_ctx_create_opts; 0: chosen with the geometry)
    int rc_loaders = 14;                    // (experiments) GA_RC_LOADERS, 12..14
    int rc_tag_fault = 0;                   // GA_RC_TAG_FAULT (tests), >= 0
    std::optional<int> rc_wpw;              // GA_RC_WPW: workers per recompute workgroup (workers())
    int rc_span = kSpanI;                   // GA_RC_SPAN, 2..kSpanI
    int rc_cone = 3;                        // GA_RC_CONE, 1..8
    std::optional<int> rc_win;              // GA_RC_WIN, >= 4: caps the window
    int rc_servers = 64;                    // GA_RC_SERVERS, 1..255
    int64_t rc_decode_lag = 0;              // (diagnostics) GA_RC_DECODE_LAG blocks of 512 dispatches held back
    bool rc_decode_check = false;           // (diagnostics) GA_RC_DECODE_CHECK is set
    int walk_skip_corners = 1;              // (experiments) GA_WALK_SKIP_CORNERS
    int walk_loaders = 14;                  // (experiments) GA_WALK_LOADERS
    bool walk_nostream = false;             // GA_WALK_NOSTREAM is set
    std::optional<int64_t> tb_band_rows;    // GA_TB_BAND_ROWS (tests: force small bands)
    int64_t tb_budget = (int64_t)64 << 30;  // GA_TB_BUDGET_MB, in bytes
    std::optional<int64_t> dev_avail;       // GA_DEV_AVAIL_MB, in bytes (tests: forces the fallbacks)
    template <typename Get, typename XGet>
    static Knobs parse(Get&& get, XGet&& xget) {
        Knobs kn;
        auto clamp = [](int lo, int hi, const char* e) { return std::max(lo, std::min(hi, atoi(e))); };
        if (const char* e = get("GA_RC")) kn.rc = atoi(e);
        if (const char* e = get("GA_RC_MIN_CELLS")) kn.rc_min_cells = atoll(e);
        if (const char* e = get("GA_RC_EVERY")) kn.rc_every = atoi(e);
        if (const char* e = xget("GA_RC_LOADERS")) kn.rc_loaders = clamp(12, 14, e);
        if (const char* e = get("GA_RC_TAG_FAULT")) kn.rc_tag_fault = std::max(0, atoi(e));
        if (const char* e = get("GA_RC_WPW")) kn.rc_wpw = atoi(e);
        if (const char* e = get("GA_RC_SPAN")) kn.rc_span = clamp(2, kSpanI, e);
        if (const char* e = get("GA_RC_CONE")) kn.rc_cone = clamp(1, 8, e);
        if (const char* e = get("GA_RC_WIN")) kn.rc_win = std::max(4, atoi(e));
        if (const char* e = get("GA_RC_SERVERS")) kn.rc_servers = clamp(1, 255, e);
        if (const char* e = get("GA_RC_DECODE_LAG")) kn.rc_decode_lag = (int64_t)atoi(e) * 512;
        kn.rc_decode_check = get("GA_RC_DECODE_CHECK") != nullptr;
        if (const char* e = xget("GA_WALK_SKIP_CORNERS")) kn.walk_skip_corners = atoi(e);
        if (const char* e = xget("GA_WALK_LOADERS")) kn.walk_loaders = atoi(e);
        kn.walk_nostream = get("GA_WALK_NOSTREAM") != nullptr;
        if (const char* e = get("GA_TB_BAND_ROWS")) kn.tb_band_rows = atoll(e);
        if (const char* e = get("GA_TB_BUDGET_MB")) kn.tb_budget = atoll(e) << 20;
        if (const char* e = get("GA_DEV_AVAIL_MB")) kn.dev_avail = atoll(e) << 20;
        return kn;
    }
};

// Whether the recompute walk takes the traceback: of ga_problem_align's loaded problem, or
// (slab_call) of a slab's traceback fill, ga_slab_fill_launch, by the same rule on the slab's own columns.
inline bool rc_eligible(const gaplan::Problem& pb, const Knobs& kn, bool slab_call) {
    if (kn.rc == 0 || (pb.slab && !slab_call) || pb.qbytes != 1 || pb.K > 32) return false;
    if (pb.m < 256 || pb.n < 256) return false;  // (degenerate walks read cells no block ever recomputes)
    if (!rc_rows_fit(pb.m)) return false;        // the lean checkpoint store's 32-bit buffer (ga_check.h)
    if (kn.rc == 1) return true;
    // One call, 2^26 cells and up (round 4): with the lean sub-chunk and 4-column stripes the recompute call beats the
    // stored-words one from C2 up (C2 2.00 -> 1.75-1.77 ms, C5 4.12 -> 3.92, C3 15.73 -> 15.57; tools/r4_td.sh,
    // profiles/r04/single_call_td.txt).  A slab, C3 (10^10 cells) and up: C5 (20k x 20k protein) kept the stored-words
    // path, its rc lane fill (313 stripes at TD = 1 for 20k rows) took 4.8 ms against the row scan's 1.8
    // (tools/exp/r3 bench_c5 logs)
    return pb.m * pb.n >= kn.rc_min_cells.value_or((int64_t)1 << (slab_call ? 32 : 26));
}

// The rows of a band of the banded traceback (0: one fill holds the m*n*CB bytes of words).  The budget
// is GA_TB_BUDGET_MB and no more than avail_bytes, what the device has free for the words (dev_avail_bytes; what the
// context's word buffer already holds counts): a stored-words fill past it failed with GA_E_HIP instead of banding.
inline int64_t band_rows(int64_t m, int64_t n, int CB, const Knobs& kn, int64_t avail_bytes) {
    constexpr int64_t FR = gaplan::kFillRows;
    if (kn.tb_band_rows) {
        const int64_t Bh = (*kn.tb_band_rows / FR) * FR;
        return Bh >= FR && m >= 2 * Bh ? Bh : 0;
    }
    const int64_t budget = std::min(kn.tb_budget, avail_bytes);
    const int64_t words = ((n + 63) / 64) * 64 * CB;  // traceback bytes per row
    if (m * words <= budget) return 0;
    const int64_t Bh = std::max<int64_t>(64, (budget / words / FR) * FR);
    return m >= 2 * Bh ? Bh : 0;
}

// The stored-words call writes its levels to pinned host memory and decodes them while the walk runs (as the
// recompute call); degenerate walks, which need a row or column of the matrix of length 1, keep the plain path.
inline bool streamed(int64_t m, int64_t n, const Knobs& kn) { return std::min(m, n) >= 256 && !kn.walk_nostream; }

// The recompute walk's window (RcArgs::off, nwin): the first nwin offsets are recomputed ahead of the walker.
struct Window {
    unsigned char off[kWindow];
    int nwin;
};

// The window: blocks up-left of the walker's (dbi block rows, dbs stripes), the path's likeliest first: it runs near
// the diagonal, so the key is the tile distance plus the distance off the diagonal, dbi + dbs*TD + cone*|dbi - dbs*TD|
// (GA_RC_CONE weighs the off-diagonal distance more, which reaches further along the diagonal with the same 64
// blocks).  Only the first nwin are recomputed ahead (the walker's own 2 x 2 tiles always rank first); speculative
// blocks cost the workers' time and the claims.  Candidates up to 31 block rows / 7 stripes away (offsets dbi*8 + dbs)
// in a cache 64 x 32 deep (the safety argument is at rc_block's cache store, ga_rcwalk.hip).  Deeper candidates keep
// the recompute ahead of a fast walker (C4, TD 4: a 28 us block against 27 us of walking across 8 block rows; round 3
// first searched 8 x 8, round 4 16 x 16: the default window is the same 64 blocks in all three).
// (cone 3 by default since round 6: the same 64 candidates reach further along the diagonal, so the walker waits less
// on its tiles (C3 tile waits 0.31 -> 0.15 ms at TD 4, 0.70 -> 0.14 at TD 2) with fewer blocks recomputed (TD 2: 16.7k
// -> 12.5k); cones 2 and 4 walk as fast, tools/exp/r6/check6.sh)
inline Window window(int TD, const Knobs& kn) {
    const int span = kn.rc_span, cone = kn.rc_cone;
    std::vector<std::pair<int, int>> off;
    for (int di = 0; di < span; di++)
        for (int dj = 0; dj < std::min(span, kSpanS); dj++)
            off.push_back({di * 8 + dj, di + dj * TD + cone * std::abs(di - dj * TD)});
    // Liveness whatever the window's width: the walker waits only on tiles of its block and of the blocks above it,
    // left of it and up-left (its verified 2 x 2 tiles), so those four rank first (key -1); ranked by the key alone, a
    // 4-block window at TD = 4 held the walker's own stripe only, and one worker never recomputed the stripe to its
    // left (test_rc_worker_pools_vs_oracle[env0] timed out, round 4)
    for (auto& o : off)
        if (o.first == 0 || o.first == 1 || o.first == 8 || o.first == 9) o.second = -1;
    std::stable_sort(off.begin(), off.end(),
                     [](const std::pair<int, int>& x, const std::pair<int, int>& y) { return x.second < y.second; });
    Window w;
    for (int k = 0; k < kWindow; k++) w.off[k] = k < (int)off.size() ? (unsigned char)off[k].first : 0;
    // 64 candidates (C3 walk 5.63 ms against 5.80 with 48 of 8 x 8, C4 with traceback 61 ms against 90:
    // tools/exp/r3b_span.sh)
    w.nwin = std::min(kWindow, (int)off.size());
    if (kn.rc_win) w.nwin = std::min(w.nwin, *kn.rc_win);  // (both >= 4)
    return w;
}

// Workers per recompute workgroup: one (one workgroup per CU) by default: C3 blocks 14.7 us against 16.5 at three per
// CU, the walker's tile waits 0.07 against 0.5 ms (tools/exp/r3_rc_diag.py); GA_RC_WPW asks for more, up to what the
// workgroup's LDS holds (the tie-to-tie walk's workers: always one).
inline int workers(bool jump, int worker_bytes, const Knobs& kn) {
    if (!kn.rc_wpw) return 1;
    const int cap = jump ? 1 : std::max(1, std::min(16, (256 * 256 * 2 - 1024) / worker_bytes));
    return std::max(1, std::min(cap, *kn.rc_wpw));
}

// Recompute workgroups: with a faster walker (scalar entry loads) fewer workers keep up, and more of them slow the
// walker's own tile loads (C3 walk 5.78 / 5.84 / 5.99 / 6.24 ms at 48 / 64 / 96 / 128 workers, 6.05 at 40, 6.72 at
// 32: tools/exp/r3b_servers.sh); 64 keeps a margin above the cliff
inline int servers(const Knobs& kn) { return kn.rc_servers; }

}  // namespace gawalk
