// ga_pipe_host.cpp -- pipelined repeated alignments (ga_problem_align_many): `count` alignments of the
// loaded pair, each from the random state the previous one left.  Up to six slots of boundary arrays / traceback
// words / hand-off edges / walk buffers (every alignment runs the whole path); fills go round the fill streams, so
// fill k+1 starts on the CUs fill k leaves idle (C3: one fill holds 196 of 256) and on those its tail frees, and walk
// k runs on a stream of its own beside them.  Walks are serial (alignment k's table slice starts where alignment
// k-1's dispatches ended); a host thread extends the one tie-break stream ahead of them.  The choices and that
// thread are ga_pipe.h's; here are the HIP calls, in the order the measured timelines depend on.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <thread>

#include "ga_host_internal.h"

using namespace gahost;
using namespace garng;

namespace gahost {

static_assert(gapipe::kChainSlots == ga::WALK_CHAIN_SLOTS, "the plan's chain slots (ga_pipe.h)");

namespace {

// One call beside the context: its arguments (alignment k's strings go to k * cap) and what its loop sums up.
struct Many {
    int count;
    uint32_t* mt_state;
    const char *a_chr, *b_chr;
    char *oa, *om, *ob;
    int64_t cap, *out_len;
    int32_t* tb_status;
    int64_t* cost_out;
    double t0 = now_ms();
    int64_t G = 0;  // global dispatches consumed by the alignments so far
    float fill_sum = 0.f, walk_sum = 0.f;
};

int pipe_setup(ga_ctx* c, const gapipe::Knobs& kn) {
    Pipeline& P = c->pipe;
    if (!P.wstream) HIPCHK(hipStreamCreateWithPriority(&P.wstream, hipStreamNonBlocking, c->priority));
    for (int f = 1; f < 4; f++)
        if (!P.fstream[f]) HIPCHK(hipStreamCreateWithPriority(&P.fstream[f], hipStreamNonBlocking, c->priority));
    if (P.walk_cus < 0) {
        // The walk's LDS tile torus (128 KB) needs a CU no fill workgroup occupies.  With the walk's CUs masked out of the
        // fill streams it never waits for one to drain, and two fills may share the others (default 0: unmasked streams)
        const int wc = P.walk_cus = kn.walk_cus;
        if (wc > 0) {
            const int nc = c->num_cu, words = (nc + 31) / 32;
            std::vector<uint32_t> fm(words, 0u), wm(words, 0u);
            for (int cu = 0; cu < nc; cu++) {
                auto& mk = cu >= nc - wc ? wm : fm;
                mk[cu >> 5] |= 1u << (cu & 31);
            }
            HIPCHK(hipExtStreamCreateWithCUMask(&P.mwstream, (uint32_t)words, wm.data()));
            for (int f = 0; f < 4; f++) HIPCHK(hipExtStreamCreateWithCUMask(&P.mfstream[f], (uint32_t)words, fm.data()));
        }
    }
    HIPCHK(P.pin.ensure(sizeof(int) * 8 * 6));
    const int64_t per = c->m + c->n + 1;
    for (int s = 0; s < P.plan.slots; s++) {
        auto& sl = P.slot[s];
        for (hipEvent_t* e : {&sl.fb.ev[0], &sl.fb.ev[1], &sl.w0, &sl.w1})
            if (!*e) HIPCHK(hipEventCreate(e));
        if (!sl.fdone) HIPCHK(hipEventCreateWithFlags(&sl.fdone, hipEventDisableTiming));
        HIPCHK(sl.tab_pin.ensure(sizeof(uint32_t) * per));
        HIPCHK(sl.rng.ensure(sizeof(uint32_t) * (per + 64)));  // + the walk's entry look-ahead (SLD)
        HIPCHK(sl.ops.ensure(c->m + c->n + 1024));
        HIPCHK(sl.result.ensure(sizeof(int) * 16));
        const int64_t m = c->m, na = c->n_global;
        HIPCHK(sl.fb.ensure_boundary(m, na));
        if (c->custom) {  // host-supplied boundary triples: the boundary pass reads them from the slot
            HIPCHK(hipMemcpyAsync(sl.fb.bnd_row.p, c->fb.bnd_row.p, sizeof(int) * 3 * (na + 1), hipMemcpyDeviceToDevice,
                                  c->stream));
            HIPCHK(hipMemcpyAsync(sl.fb.bnd_col.p, c->fb.bnd_col.p, sizeof(int) * 3 * (m + 1), hipMemcpyDeviceToDevice,
                                  c->stream));
        }
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return GA_OK;
}

// fill of an alignment into slot `slot` on stream `st`, then its cost inputs into pinned memory, then `fdone`
int pipe_fill(ga_ctx* c, int slot, hipStream_t st, bool row = false, gaplan::FillPlan* plan_out = nullptr) {
    auto& sl = c->pipe.slot[slot];
    Band bd;  // this slot's buffers, this stream, this lane geometry
    bd.bufs = &sl.fb;
    bd.stream = st;
    bd.lane_td = row ? 0 : c->pipe.plan.lane_td;
    bd.lane_nwc = row ? 0 : c->pipe.plan.lane_nwc;
    if (int r = enqueue_fill(c, GA_FILL_TRACEBACK, bd, plan_out)) return r;
    int* pin = c->pipe.pin.host<int>() + 8 * slot;
    HIPCHK(hipMemcpyAsync(pin, sl.fb.out_last.p, sizeof(int) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(pin + 4, sl.fb.meta.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(pin + 5, sl.fb.GHp.as<int>() + c->col0 + c->n, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(pin + 6, sl.fb.flags.as<unsigned>() + 1, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(sl.fdone, st));
    return GA_OK;
}

// Per slot, pinned and coherent host memory for a pipelined walk's result words (256 B) and levels: the walk writes
// them there, so the host reads them without a hipMemcpy (which would wait for a CU, and the fills hold them all).
struct PipeIo {
    size_t stride = 0;
    uint8_t *dev = nullptr, *host = nullptr;
    int* res(uint8_t* base, int s) const { return reinterpret_cast<int*>(base + stride * s); }
    uint32_t* ops(uint8_t* base, int s) const { return reinterpret_cast<uint32_t*>(base + stride * s + 256); }
};
int pipe_io(ga_ctx* c, int S, PipeIo& io) {
    io.stride = 256 + (((size_t)(c->m + c->n + 1024) + 255) / 256) * 256;  // the levels' bytes, in whole 256
    HIPCHK(c->pipe.chain_io.ensure(io.stride * S));
    io.dev = c->pipe.chain_io.dev<uint8_t>();
    io.host = c->pipe.chain_io.host<uint8_t>();
    return GA_OK;
}

// Slot s's walk on stream ws: its result words and levels to pinned memory (pipe_io) or, GA_PIPE_PINNED_IO=0, to the
// slot's device buffers, read back with hipMemcpy.  The chain's walks read the table from pinned memory: no slot copy.
WalkBufs slot_walk_bufs(ga_ctx* c, int s, hipStream_t ws, const PipeIo& io, bool pinned_io, bool chain) {
    auto& sl = c->pipe.slot[s];
    return WalkBufs{sl.fb.tb.as<uint8_t>(), chain ? nullptr : sl.rng.as<uint32_t>(),
                    pinned_io ? io.ops(io.dev, s) : sl.ops.as<uint32_t>(), pinned_io ? io.res(io.dev, s) : sl.result.as<int>(),
                    ws, chain ? nullptr : sl.w0, chain ? nullptr : sl.w1, sl.fb.bnd_row.as<int>(),
                    sl.fb.bnd_col.as<int>()};
}

// GA_PIPE_TRACE=<file>: a line per alignment (a diagnostic of what bounds the pipeline), closed on every return path.
// The per-launch loop's lines hold GPU times from `origin`, an event recorded on the first fill's stream.
struct PipeTrace {
    FILE* f = nullptr;
    hipEvent_t origin = nullptr;
    void open(const char* path, const hipStream_t* on) {
        if (path && (!on || (hipEventCreate(&origin) == hipSuccess && hipEventRecord(origin, *on) == hipSuccess)))
            f = fopen(path, "a");
    }
    ~PipeTrace() {
        if (f) fclose(f);
        if (origin) (void)hipEventDestroy(origin);
    }
};

// The end of alignment k, whose walk (result words `res`, levels in host_ops or, nullptr, in wb.ops) has left slot
// `slot`: the fill's abort word, the cost and the fill's time out of the slot's pinned words and events; then
// `refill(fill_ms)`, the loop's own step that hands the slot to the next fill (nothing of the slot's is read after
// it); then the strings, while the next walk and the fills run, and the dispatches the alignment consumed.
template <typename Refill>
int finish_alignment(ga_ctx* c, Many& run, int k, int slot, const int* res, const uint32_t* host_ops, const WalkBufs& wb,
                     Refill&& refill) {
    auto& sl = c->pipe.slot[slot];
    const int* pin = c->pipe.pin.host<int>() + 8 * slot;
    if (pin[6]) return fail(GA_E_TIMEOUT, "fill kernel hand-off wait timed out");
    run.cost_out[k] = (int64_t)pin[0] + pin[4] + pin[5];
    float fill_ms = 0.f;
    if (hipEventElapsedTime(&fill_ms, sl.fb.ev[0], sl.fb.ev[1]) != hipSuccess) fill_ms = 0.f;
    run.fill_sum += fill_ms;
    if (int r = refill(fill_ms)) return r;
    WalkStart st = walk_origin(c);
    int reason = 0;
    int64_t len = 0;
    char *a_k = run.oa + (size_t)k * run.cap, *m_k = run.om + (size_t)k * run.cap, *b_k = run.ob + (size_t)k * run.cap;
    if (int r = decode_segment(c, res, st, reason, run.a_chr, run.b_chr, a_k, m_k, b_k, run.cap, len, wb, true, host_ops))
        return r;
    if (int r = conclude_walk(c->pipe.rng, st, reason, nullptr, run.a_chr, run.b_chr, a_k, m_k, b_k, run.cap, len,
                              &run.out_len[k], &run.tb_status[k]))
        return r;
    run.G += st.D;
    return GA_OK;
}

// What both loops leave once every alignment is out: the final random state, the mean times.
void finish_many(ga_ctx* c, const Many& run, double rng_ms) {
    state_after(c->pipe.rng, run.G, run.mt_state);  // the state the last alignment leaves (random.getstate() layout)
    c->fill_ms = run.fill_sum / run.count;
    c->walk_ms = run.walk_sum / run.count;
    c->rng_ms = (float)(rng_ms / run.count);
    c->call_ms = (float)(now_ms() - run.t0);
    c->filled_tb = false;  // ctx->tb does not hold the last fill's words
}

// The walks chained in one walk_chain_kernel launch (no host round trip between walks, 45-55 us at
// C2 / C5, 0.1-0.2 ms at C3, and the walks keep their CU).  Walk k+1 starts when walk k ends, reading the tie-break
// stream from G_{k+1}, which the kernel sums itself, straight out of pinned host memory that the feeder thread
// fills; the host only says which fills have ended and decodes each alignment's strings.
int align_chain(ga_ctx* c, const gapipe::Knobs& kn, Many& run, const hipStream_t* fs) {
    Pipeline& P = c->pipe;
    const int count = run.count;
    const int64_t m = c->m, n = c->n, per = m + n + 1;
    const int F = P.plan.fills, S = P.plan.slots;
    if (!P.cwstream) {
        int lo = 0, hi = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(hipStreamCreateWithPriority(&P.cwstream, hipStreamNonBlocking, lo));
    }
    hipStream_t ws = P.cwstream;
    HIPCHK(P.chain_tab.ensure(sizeof(uint32_t) * (int64_t)count * per));
    HIPCHK(P.chain_ctl.ensure(64));
    PipeIo io;
    if (int r = pipe_io(c, S, io)) return r;
    unsigned* ctl = P.chain_ctl.host<unsigned>();
    std::memset(ctl, 0, 64);

    // the tie-break stream: started before the fills are enqueued (C2 / C5: the first walk waited 2.1 / 4.0 ms for
    // its entries).  Walk k+1 may start the moment walk k ends, anywhere in [G_k + max(m, n), G_k + m + n]: the
    // entries are kept two alignments' worth ahead of the last walk known to have ended
    gapipe::TableFeeder feeder(P.rng, run.mt_state, per, count,
                               {P.chain_tab.host<uint32_t>(), reinterpret_cast<long long*>(ctl + 4)});
    auto stop = [&](int rc) {
        feeder.stop();
        if (rc != GA_OK) __atomic_store_n(ctl + 2, 1u, __ATOMIC_RELEASE);  // the chain exits at its next wait
        (void)hipStreamSynchronize(ws);
        c->guard.in_chain = false;
        if (rc != GA_OK)
            for (int f = 0; f < F; f++) (void)hipStreamSynchronize(fs[f]);
        return rc;
    };
    int enqueued = 0, signalled = 0;
    auto launch_all = [&]() -> int {
        // fill 0 first (it fixes the fill geometry and so the size of every slot's traceback words), then
        // the walks' launch, so that its workgroup has a CU before the other fills take them all, then
        // fills 1 .. S-1; fill j goes into slot j % S on fill stream j % F (each computes its own boundary)
        gaplan::FillPlan pl;
        if (int r = pipe_fill(c, 0, fs[0], false, &pl)) return r;
        enqueued++;
        // every slot's fill buffers at their final size now: a reallocation's hipFree while the chain runs
        // would wait for the chain, which waits for the host
        const size_t tb_bytes = (size_t)pl.nstripes * pl.T * pl.TC * 1024;
        const size_t hand_bytes = sizeof(int2) * (size_t)pl.nslabs * (m + 1);
        for (int s = 1; s < S; s++) {
            auto& sl = P.slot[s];
            HIPCHK(sl.fb.tb.ensure(tb_bytes));
            HIPCHK(sl.fb.hand.ensure(hand_bytes));
            HIPCHK(sl.fb.flags.ensure(sizeof(unsigned) * 16));
            HIPCHK(sl.fb.out_last.ensure(sizeof(int) * 4));
        }
        ga::WalkChainArgs A{};
        for (int s = 0; s < S; s++)
            A.w[s] = walk_args(c, per, walk_origin(c), 0, -1, false, slot_walk_bufs(c, s, ws, io, true, true));
        A.tab = P.chain_tab.dev<uint32_t>();
        A.ctl = P.chain_ctl.dev<unsigned>();
        A.tab_ready = reinterpret_cast<const long long*>(A.ctl + 4);
        A.per = per;
        A.wait_limit = 100ull * 1000 * 1000 * 60;  // 60 s of s_memrealtime (100 MHz)
        A.count = count;
        A.S = S;
        HIPCHK(hipEventRecord(P.slot[0].w0, ws));
        c->guard.in_chain = true;  // until stop(): guard mode must not wait for the device from here on
        ga::launch_walk_chain(ws, A);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(P.slot[0].w1, ws));
        for (int k = 1; k < std::min(count, S); k++) {
            if (int r = pipe_fill(c, k, fs[k % F])) return r;
            enqueued++;
        }
        return GA_OK;
    };
    if (int r = launch_all()) return stop(r);
    PipeTrace tr;
    tr.open(kn.trace, nullptr);
    const double h0 = now_ms();
    int rc = GA_OK;
    for (int k = 0; k < count && rc == GA_OK; k++) {
        // wait for walk k; meanwhile tell the chain which fills have ended (in order, enqueued ones only:
        // a slot's event still holds the previous fill of that slot until the next is enqueued)
        for (;;) {
            while (signalled < enqueued && hipEventQuery(P.slot[signalled % S].fdone) == hipSuccess)
                __atomic_store_n(ctl, (unsigned)++signalled, __ATOMIC_RELEASE);
            if ((int)__atomic_load_n(ctl + 1, __ATOMIC_ACQUIRE) > k) break;
            if (__atomic_load_n(ctl + 3, __ATOMIC_ACQUIRE)) {
                rc = fail(GA_E_TIMEOUT, "chained walk waited too long for its fill or tie-break entries");
                break;
            }
            std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
        if (rc != GA_OK) break;
        int res[16];
        std::memcpy(res, io.res(io.host, k % S), sizeof(res));
        const int64_t Dk = res[0];
        feeder.raise_target(run.G + Dk + 2 * per + per / 8);
        rc = finish_alignment(
            c, run, k, k % S, res, io.ops(io.host, k % S), slot_walk_bufs(c, k % S, ws, io, true, true),
            [&](float f) -> int {
                run.walk_sum += res[8] / 1.0e5f;  // the walker's own time (s_memrealtime ticks, 100 MHz)
                if (tr.f)
                    fprintf(tr.f, "{\"k\": %d, \"chain\": 1, \"fill_ms\": %.3f, \"walk_ms\": %.3f, \"walk_done_host\": %.3f, "
                            "\"D\": %lld, \"tile_wait_us\": %.2f, \"tile_loads\": %d, \"chain_wait_us\": %.2f, "
                            "\"polls_fill\": %d, \"polls_tab\": %d}\n", k, f, res[8] / 1.0e5,
                            now_ms() - h0, (long long)Dk, res[6] / 100.0, res[11], res[12] / 100.0, res[13], res[14]);
                // fill k+S into slot k's buffers (walk k has read them)
                if (k + S < count) {
                    if (int r = pipe_fill(c, k % S, fs[(k + S) % F])) return r;
                    enqueued++;
                }
                return GA_OK;
            });
    }
    if (int r = stop(rc)) return r;
    finish_many(c, run, feeder.rng_ms());
    return GA_OK;
}

// One launch per walk (the default): walk k+1 is launched by the host when walk k has ended.
int align_many(ga_ctx* c, const gapipe::Knobs& kn, Many& run) {
    Pipeline& P = c->pipe;
    const int count = run.count;
    if (int r = pipe_setup(c, kn)) return r;
    if (P.plan.chain_refused) return fail(GA_E_ARG, "too many pipeline slots for the walk chain");
    hipStream_t fs[4] = {c->stream, P.fstream[1], P.fstream[2], P.fstream[3]};
    if (P.plan.chain) return align_chain(c, kn, run, fs);
    const int64_t m = c->m, n = c->n, per = m + n + 1;
    const int F = P.plan.fills, S = P.plan.slots;
    hipStream_t ws = P.wstream;
    if (P.walk_cus > 0) {
        for (int f = 0; f < 4; f++) fs[f] = P.mfstream[f];
        ws = P.mwstream;
    } else if (kn.fill_prio_normal) {
        for (int f = 0; f < 4; f++) {
            if (!P.nfstream[f]) HIPCHK(hipStreamCreateWithPriority(&P.nfstream[f], hipStreamNonBlocking, 0));
            fs[f] = P.nfstream[f];
        }
    }
    PipeTrace tr;  // per alignment, GPU times (ms from the first fill's enqueue) of fill and walk, host times of launches
    tr.open(kn.trace, &fs[0]);
    const double h0 = now_ms();
    PipeIo io;
    if (int r = pipe_io(c, S, io)) return r;
    const bool pinned_io = kn.pinned_io;
    std::vector<int> pending;  // slots holding an enqueued fill no walk has taken, in enqueue order
    std::vector<int> walk_slot((size_t)count, -1);
    int fills_enqueued = 0;
    // fill j into slot j % S on fill stream j % F; each computes its own boundary
    for (int k = 0; k < std::min(count, S); k++) {
        // (experiment, GA_PIPE_ROW_FIRST=r: the first r fills through the row scan, whose latency alone is shorter)
        if (int r = pipe_fill(c, k, fs[k % F], k < kn.row_first.value_or(0))) return r;
        pending.push_back(k);
        fills_enqueued++;
    }
    gapipe::TableFeeder feeder(P.rng, run.mt_state, per, count);
    // walk k over its table slice [G, G + per), after fill k, on the walk stream
    auto start_walk = [&](int k, int64_t G) -> int {
        // the slot: every fill computes the same arrays (the same pair, boundary and words), so the first pending one
        // whose fill has ended, not slot k % S (GA_PIPE_SLOT_ORDER=fixed keeps that); while all still run, the host
        // waits for the first to end (the oldest is not always first: in the ramp four fills share the chip, and the
        // third ends ~3 ms after the fourth)
        size_t pick = 0;
        for (bool found = kn.fixed_order; !found;) {
            for (size_t q = 0; q < pending.size() && !found; q++)
                if (hipEventQuery(P.slot[pending[q]].fdone) == hipSuccess) {
                    pick = q;
                    found = true;
                }
            if (!found) std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
        walk_slot[k] = pending[pick];
        pending.erase(pending.begin() + (long)pick);
        auto& sl = P.slot[walk_slot[k]];
        feeder.wait_ready(G + per);
        HIPCHK(hipStreamWaitEvent(ws, sl.fdone, 0));
        std::memcpy(sl.tab_pin.p, feeder.tab() + G, sizeof(uint32_t) * per);
        const WalkBufs wb = slot_walk_bufs(c, walk_slot[k], ws, io, pinned_io, false);
        return run_walk(c, sl.tab_pin.host<uint32_t>(), per, walk_origin(c), 0, -1, false, true, &wb);
    };
    int rc = start_walk(0, 0);
    double walk_launch_host = now_ms() - h0;
    int64_t Dmax = 0;
    for (int k = 0; k < count && rc == GA_OK; k++) {
        const int s = walk_slot[k];
        auto& sl = P.slot[s];
        auto step = [&]() -> int {
            // walk k done: its dispatch count fixes where walk k+1's table slice starts
            HIPCHK(hipEventSynchronize(sl.w1));
            int res[16];
            if (pinned_io) std::memcpy(res, io.res(io.host, s), sizeof(res));
            else HIPCHK(hipMemcpy(res, sl.result.p, sizeof(int) * 16, hipMemcpyDeviceToHost));
            const int64_t Dk = res[0];
            Dmax = std::max(Dmax, Dk);
            if (tr.f) {
                float t[4] = {0.f, 0.f, 0.f, 0.f};
                hipEvent_t evs[4] = {sl.fb.ev[0], sl.fb.ev[1], sl.w0, sl.w1};
                for (int q = 0; q < 4; q++) (void)hipEventElapsedTime(&t[q], tr.origin, evs[q]);
                // the walker's own accounting (walk_kernel result[4..11]; s_memrealtime ticks at 100 MHz)
                fprintf(tr.f, "{\"k\": %d, \"fill0\": %.3f, \"fill1\": %.3f, \"walk0\": %.3f, \"walk1\": %.3f, "
                        "\"walk_launch_host\": %.3f, \"walk_done_host\": %.3f, \"D\": %lld, \"tile_wait_us\": %.2f, "
                        "\"walker_us\": %.2f, \"tile_loads\": %d, \"load_us_per_tile\": %.3f}\n", k, t[0], t[1], t[2],
                        t[3], walk_launch_host, now_ms() - h0, (long long)Dk, res[6] / 100.0, res[8] / 100.0, res[11],
                        res[11] > 0 ? res[10] / 100.0 / res[11] : 0.0);
            }
            // keep the feeder an alignment's worth (and some) ahead of the next walk
            feeder.raise_target(run.G + Dk + per + Dmax + Dmax / 8);
            if (k + 1 < count) {
                if (int r = start_walk(k + 1, run.G + Dk)) return r;
                walk_launch_host = now_ms() - h0;
            }
            // alignment k's cost (fill k finished before walk k started) and times, before slot k's pinned words
            // and events are reused
            return finish_alignment(
                c, run, k, s, res, pinned_io ? io.ops(io.host, s) : nullptr, slot_walk_bufs(c, s, ws, io, pinned_io, false),
                [&](float) -> int {
                    float wms = 0.f;
                    if (hipEventElapsedTime(&wms, sl.w0, sl.w1) == hipSuccess) run.walk_sum += wms;
                    // the next fill into walk k's slot (walk k has read it), on its stream after the fill F before
                    if (fills_enqueued < count) {
                        if (int r = pipe_fill(c, s, fs[fills_enqueued % F])) return r;
                        pending.push_back(s);
                        fills_enqueued++;
                    }
                    return GA_OK;
                });
        };
        rc = step();
    }
    feeder.stop();
    if (rc != GA_OK) {
        for (int f = 0; f < F; f++) (void)hipStreamSynchronize(fs[f]);
        (void)hipStreamSynchronize(ws);
        return rc;
    }
    finish_many(c, run, feeder.rng_ms());
    return GA_OK;
}

}  // namespace

int problem_align_many(ga_ctx* c, int32_t count, uint32_t* mt_state, const char* a_chr, const char* b_chr, char* oa,
                       char* om, char* ob, int64_t cap, int64_t* out_len, int32_t* tb_status, int64_t* cost_out) {
    if (int r = check_ctx(c)) return r;
    if (c->slab) return fail(GA_E_STATE, "slab contexts use ga_slab_fill_launch");
    if (count < 1) return fail(GA_E_ARG, "count must be >= 1");
    if (!mt_state || !a_chr || !b_chr || !oa || !om || !ob || !out_len || !tb_status || !cost_out)
        return fail(GA_E_ARG, "null argument");
    if (!c->loaded) return fail(GA_E_STATE, "no problem loaded");
    const gapipe::Knobs& kn = c->pipek;
    c->pipe.plan = gapipe::plan(plan_problem(c), kn, c->hw_queues, count, count == 1 ? 0 : band_rows(c));
    if (c->pipe.plan.serial) {
        const double t0 = now_ms();
        float fs = 0.f, ws = 0.f, rs = 0.f;
        for (int k = 0; k < count; k++) {
            if (int r = ga_problem_align(c, mt_state, a_chr, b_chr, oa + (size_t)k * cap, om + (size_t)k * cap,
                                         ob + (size_t)k * cap, cap, &out_len[k], &tb_status[k], &cost_out[k]))
                return r;
            fs += c->fill_ms;
            ws += c->walk_ms;
            rs += c->rng_ms;
        }
        c->fill_ms = fs / count;
        c->walk_ms = ws / count;
        c->rng_ms = rs / count;
        c->call_ms = (float)(now_ms() - t0);
        return GA_OK;
    }
    Many run{count, mt_state, a_chr, b_chr, oa, om, ob, cap, out_len, tb_status, cost_out};
    return align_many(c, kn, run);
}

}  // namespace gahost
