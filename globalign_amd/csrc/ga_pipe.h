// ga_pipe.h -- the pure part of the repeated-alignment pipeline (ga_problem_align_many): its knobs as
// numbers, the plan of one call, and the host thread that extends the tie-break stream ahead of the walks.  No HIP, no
// context, no globals: built into the engine (ga_pipe_host.cpp) and into ga_pipe_selftest.cpp under ASan / UBSan / TSan.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <optional>
#include <thread>

#include "ga_plan.h"
#include "ga_rng.h"

namespace gapipe {

constexpr int kMaxSlots = 6;    // ga_ctx's pipeline slots (GA_PIPE_SLOTS clamps to it)
constexpr int kChainSlots = 6;  // ga::WALK_CHAIN_SLOTS (ga_pipe_host.cpp asserts the two agree)

enum Mode { kAuto = 0, kRow = 1, kLane = 2 };

// The pipeline's knobs, parsed here and nowhere else, once per context (ga_ctx::pipek): `get` looks a shipped knob up,
// `xget` one of a path that was measured and dropped (ga_ctx_create_opts' two look-ups: the shipped build's xget sees
// nothing); nullptr for an unset name.
struct Knobs {
    int mode = kAuto;                // GA_PIPE_MODE=row|lane
    std::optional<int> fills;        // GA_PIPE_FILLS (2..4)
    std::optional<int> slots;        // GA_PIPE_SLOTS (fills + 1 .. 6)
    bool chain = false;              // GA_PIPE_CHAIN, non-zero
    bool fill_prio = false;          // GA_PIPE_FILL_PRIO is set ...
    bool fill_prio_normal = false;   // ... to "normal": the fills on default-priority streams
    bool fixed_order = false;        // GA_PIPE_SLOT_ORDER=fixed: walk k takes slot k % S
    bool pinned_io = true;           // GA_PIPE_PINNED_IO=0: walk results and levels in device memory
    const char* trace = nullptr;     // GA_PIPE_TRACE=<file> (the caller's string: ga_ctx::knobs keeps it alive)
    int walk_cus = 0;                // (experiments) GA_PIPE_WALK_CUS, 0..8
    std::optional<int> row_first;    // (experiments) GA_PIPE_ROW_FIRST
    int diag_req = 0;                // gaplan::Knobs::diag_req (GA_FILL_MODE), which the caller copies in
    template <typename Get, typename XGet>
    static Knobs parse(Get&& get, XGet&& xget) {
        Knobs kn;
        if (const char* e = get("GA_PIPE_MODE")) kn.mode = !strcmp(e, "row") ? kRow : !strcmp(e, "lane") ? kLane : kAuto;
        if (const char* e = get("GA_PIPE_FILLS")) kn.fills = atoi(e);
        if (const char* e = get("GA_PIPE_SLOTS")) kn.slots = atoi(e);
        if (const char* e = get("GA_PIPE_CHAIN")) kn.chain = atoi(e) != 0;
        if (const char* e = get("GA_PIPE_FILL_PRIO")) kn.fill_prio = true, kn.fill_prio_normal = !strcmp(e, "normal");
        if (const char* e = get("GA_PIPE_SLOT_ORDER")) kn.fixed_order = !strcmp(e, "fixed");
        if (const char* e = get("GA_PIPE_PINNED_IO")) kn.pinned_io = atoi(e) != 0;
        kn.trace = get("GA_PIPE_TRACE");
        if (const char* e = xget("GA_PIPE_WALK_CUS")) kn.walk_cus = std::max(0, std::min(8, atoi(e)));
        if (const char* e = xget("GA_PIPE_ROW_FIRST")) kn.row_first = atoi(e);
        return kn;
    }
};

struct Plan {
    bool serial = false;             // one ga_problem_align after another, no pipeline
    int lane_td = 0, lane_nwc = 0;   // the fills' lane-kernel geometry (0: the row scan)
    int fills = 3, slots = 4;        // fills in flight (one stream each) and slots (fills + the walked ones)
    bool chain = false;              // the walks chained in one launch (align_chain)
    bool chain_refused = false;      // a chain that was asked for and fits, but with more slots than it has: GA_E_ARG
};

// The plan of `count` alignments of the loaded pair; band_rows > 0: the single call would band its traceback.
inline Plan plan(const gaplan::Problem& pb, const Knobs& kn, int hw_queues, int64_t count, int64_t band_rows) {
    Plan pl;
    // up to five slots of traceback words (four lane fills in flight + the walked one; GA_PIPE_SLOTS may ask for
    // more): beyond 160 GB of them, as for one alignment or banded tracebacks (whose band fills hold every CU), serial
    const bool fits = (int64_t)5 * ((pb.n + 63) / 64) * 64 * pb.m * pb.CB <= ((int64_t)160 << 30);
    pl.serial = count == 1 || band_rows > 0 || !fits;
    // Fill kernel and fills in flight (the measured timelines: DESIGN.md 6).  A row-scan traceback fill of C3 holds
    // 196 CUs and is issue bound there, so co-resident fills gain nothing; the lane-skewed fill at 4 columns per lane
    // is narrow and latency bound (98 one-wave-per-SIMD workgroups), and three share the chip.  So one-byte words of
    // long rows (K <= 32, an int8 profile) take lane fills, the rest row-scan fills.
    bool lane = pb.CB == 1 && pb.qbytes == 1 && pb.K <= 32 && pb.m >= 32768 && pb.n >= 4 * 4 * 64 * 64 &&
                kn.diag_req != 1 && kn.diag_req != 2;
    if (kn.mode == kRow) lane = false;
    if (kn.mode == kLane) lane = pb.qbytes == 1 && pb.K <= 32;
    pl.lane_td = lane ? (pb.CB == 1 ? 4 : 2) : 0;
    pl.lane_nwc = lane ? 4 : 0;
    // Lane fills: four in flight when the process has the hardware queues for them (the fill streams and the walk
    // stream share a priority's pool of GPU_MAX_HW_QUEUES queues; two streams on one in-order queue serialise), three
    // with HIP's default of four queues.  Row-scan fills: three (four streams with the walk's: the default pool).
    pl.fills = lane ? (hw_queues >= 5 ? 4 : 3) : 3;
    if (kn.fills) pl.fills = std::max(2, std::min(4, *kn.fills));
    // slots: fill k + S reuses walk k's buffers, so the walk chain allows one alignment per (walk + fill) / S;
    // GA_PIPE_SLOTS raises S above F + 1 (up to 6)
    pl.slots = pl.fills + 1;
    if (kn.slots) pl.slots = std::max(pl.fills + 1, std::min(kMaxSlots, *kn.slots));
    // the walks chained in one launch (align_chain): faster behind row-scan fills (C2, C5), slower behind C3's lane
    // fills, beside a walk that never gives its CU back.  Opt-in (GA_PIPE_CHAIN=1): the persistent chain polls
    // host-written words, so a device-synchronising call another thread of the process makes while it runs (hipFree,
    // hipDeviceSynchronize, a torch allocator release) would wait on it until its 60 s bound.
    const bool fits_chain = count * (pb.m + pb.n + 1) <= ((int64_t)256 << 20);  // 1 GB of entries
    const bool asked = kn.chain && fits_chain && kn.walk_cus == 0 && !kn.fill_prio && !kn.row_first;
    pl.chain = asked && pl.slots <= kChainSlots;
    pl.chain_refused = asked && !pl.chain;
    return pl;
}

// The tie-break stream of `count` consecutive alignments of one pair (per = m + n + 1 entries each at the most): one
// continuous RngTable, extended by this object's thread ahead of the walks.  The consumer raises the target as walks end
// and waits for the entries the next walk reads.  Invariant: the table's vectors are reserved for all count * per
// dispatches before the thread starts, so tab() never moves and entries below a published bound stay readable while
// later ones are written.  With a sink (the walk chain's pinned table and its `entries written` word) the stream grows
// in pieces of max(per / 2, 4096) entries, each copied to the sink and published through the word with a release store
// (the first walk waits for per entries, not for the three alignments' worth the thread starts with); without one,
// one extension per wake-up.
struct FeederSink {
    uint32_t* dst = nullptr;
    long long* word = nullptr;
};
class TableFeeder {
public:
    TableFeeder(garng::RngTable& R, const uint32_t* state, int64_t per, int64_t count, FeederSink sink = FeederSink())
        : R_(R), per_(per), need_(count * per), sink_(sink) {
        R_.start(state);
        R_.tab.reserve((size_t)need_);
        R_.step_end.reserve((size_t)need_ + 4);
        R_.acc.reserve((size_t)18 * need_ + 8);
        tab_ = R_.tab.data();
        // the first three alignments' worth while the first fills run (each alignment takes about (m + n) / 1.6
        // dispatches), then kept ahead of the walks (raise_target)
        target_ = std::min<int64_t>(need_, 3 * per_);
        th_ = std::thread([this] { run(); });
    }
    ~TableFeeder() { stop(); }
    const uint32_t* tab() const { return tab_; }
    double rng_ms() const { return rng_ms_; }  // the thread's time in extensions (after stop())
    // entries to build up to (never lowered; beyond count * per: everything)
    void raise_target(int64_t t) { update([&] { target_ = std::max(target_, t); }); }
    // until entries [0, upto) are built (or the feeder is stopped); the target must cover them
    void wait_ready(int64_t upto) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return quit_ || ready_ >= std::min(upto, need_); });
    }
    // ends the thread after the extension it is in; idempotent.  The table is the caller's alone from here on.
    void stop() {
        update([&] { quit_ = true; });
        if (th_.joinable()) th_.join();
    }

private:
    template <typename F>
    void update(F&& change) {  // a change of the shared fields under the lock, then the wake-up outside it
        {
            std::lock_guard<std::mutex> lk(mu_);
            change();
        }
        cv_.notify_all();
    }
    void run() {
        using clock = std::chrono::steady_clock;
        const int64_t piece = sink_.dst ? std::max<int64_t>(per_ / 2, 4096) : need_;
        for (;;) {
            int64_t want, to;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return quit_ || target_ > ready_; });
                if (quit_) return;
                want = std::min(target_, need_);
                to = ready_;
                if (want <= ready_) {
                    target_ = ready_;  // nothing more can be built
                    continue;
                }
            }
            const auto t1 = clock::now();
            while (to < want) {
                to = std::min(want, to + piece);
                R_.extend(to);
                if (sink_.dst) {
                    memcpy(sink_.dst + ready_, tab_ + ready_, sizeof(uint32_t) * (size_t)(to - ready_));
                    __atomic_store_n(sink_.word, (long long)to, __ATOMIC_RELEASE);
                }
                update([&] { ready_ = to; });
            }
            rng_ms_ += std::chrono::duration<double, std::milli>(clock::now() - t1).count();
        }
    }

    garng::RngTable& R_;
    const int64_t per_, need_;
    const FeederSink sink_;
    const uint32_t* tab_ = nullptr;
    std::mutex mu_;
    std::condition_variable cv_;
    int64_t ready_ = 0, target_ = 0;  // entries built (written by the thread only), and to build up to (under mu_)
    bool quit_ = false;
    double rng_ms_ = 0.0;
    std::thread th_;
};

}  // namespace gapipe
