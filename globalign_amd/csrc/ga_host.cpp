// ga_host.cpp -- host side of the C ABI declared in include/globalign_amd.h.
//
// Owns device memory and the HIP stream of one context, runs the kernels of
// ga_kernels.hip, and does the two pieces of the traceback that are
// inherently host-side in the reference's semantics:
//   * the tie-break table: the reference draws 18 random.choice values per
//     dispatched traceback step from CPython's global MT19937
//     (globaligner.py:598-672); we emulate genrand_uint32 and
//     _randbelow_with_getrandbits exactly, starting from random.getstate(),
//     while the device fill runs;
//   * string assembly from the walk's per-step levels (take_* :688-753,
//     the i==0 / j==0 tails :542-581 and the final reverse :584-586): ga_strings.h.
// Here: the context, guard mode, load_problem, the fill, slabs and the debug ABI.  One alignment's traceback
// (ga_problem_align, ga_problem_traceback) is ga_align_host.cpp's.  The context's options (the GA_* knobs) are
// collected, checked and parsed into typed sets by ga_opts.h and its siblings, once, in ga_ctx_create_opts: no other
// code of the engine sees an option's name or string.
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstring>

#include "ga_host_internal.h"
#include "ga_lane.h"
#include "ga_check.h"

using namespace gahost;
using namespace garng;

namespace gahost {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// One guard of a buffer against the pattern: `img` is the guard's G bytes as the host reads them.
void guard_scan(GuardCfg* g, const std::string& name, int side, const uint8_t* img, size_t size,
                std::vector<gaguard::Violation>& out) {
    gaguard::Violation v;
    if (gaguard::make_violation(name, side, gaguard::scan(img, g->G, g->fill), size, g->G, v)) out.push_back(v);
}

// A device buffer's two guards, copied back (the caller has made sure no kernel still writes near them).
hipError_t guard_scan_dev(const DevBuf& b, bool front, bool rear, std::vector<gaguard::Violation>& out) {
    if (!b.p || !b.g) return hipSuccess;
    const size_t G = b.g->G;
    std::vector<uint8_t> img(G);
    const uint8_t* pay = static_cast<const uint8_t*>(b.p);
    if (front) {
        if (hipError_t e = hipMemcpy(img.data(), pay - G, G, hipMemcpyDeviceToHost); e != hipSuccess) return e;
        guard_scan(b.g, b.name, gaguard::kFront, img.data(), b.size, out);
    }
    if (rear) {
        if (hipError_t e = hipMemcpy(img.data(), pay + b.size, G, hipMemcpyDeviceToHost); e != hipSuccess) return e;
        guard_scan(b.g, b.name, gaguard::kRear, img.data(), b.size, out);
    }
    return hipSuccess;
}
void guard_scan_pin(const PinBuf& b, bool front, bool rear, std::vector<gaguard::Violation>& out) {
    if (!b.p || !b.g) return;
    const uint8_t* pay = static_cast<const uint8_t*>(b.p);
    if (front) guard_scan(b.g, b.name, gaguard::kFront, pay - b.g->G, b.size, out);
    if (rear) guard_scan(b.g, b.name, gaguard::kRear, pay + b.size, b.size, out);
}

// A re-lay or a reallocation rewrites guard bytes that kernels of earlier launches may have hit, and it fills memory
// that launches still in flight may be writing (a band's fill behind the previous band's): so the device
// is idle first.  Under the chained pipeline that wait would never end (its persistent kernel waits for this thread,
// up to its 60 s limit), and so would the null-stream memset after it: every buffer has its final size before the
// chain starts, and a request for another size while it runs is an error, not a stall.
hipError_t guard_quiesce(GuardCfg* g) {
    if (g->in_chain) return hipErrorNotSupported;
    return hipDeviceSynchronize();
}

hipError_t DevBuf::ensure_guarded(size_t bytes) {
    const size_t G = g->G;
    if (bytes <= cap && p) {
        if (bytes == size) return hipSuccess;
        // the same allocation for another size: what the old rear guard caught is kept, then the pattern goes from
        // the smaller of the two ends to the new guard's end.  Bytes below both ends keep their contents.
        if (hipError_t e = guard_quiesce(g); e != hipSuccess) return e;
        if (hipError_t e = guard_scan_dev(*this, false, true, g->pending); e != hipSuccess) return e;
        const gaguard::Range r = gaguard::relay_range(size, bytes, G);
        if (hipError_t e = hipMemset(static_cast<uint8_t*>(p) + r.lo, g->fill, r.hi - r.lo); e != hipSuccess) return e;
        size = bytes;
        return hipStreamSynchronize(nullptr);  // the context's streams do not wait for the null stream
    }
    if (p) {
        if (hipError_t e = guard_quiesce(g); e != hipSuccess) return e;
        if (hipError_t e = guard_scan_dev(*this, true, true, g->pending); e != hipSuccess) return e;
    }
    release();
    const size_t want = std::max<size_t>(bytes, 256), total = gaguard::alloc_bytes(want, G);
    void* raw = nullptr;
    hipError_t e = uncached ? hipExtMallocWithFlags(&raw, total, hipDeviceMallocUncached) : hipMalloc(&raw, total);
    if (e != hipSuccess) return e;
    uint8_t* r8 = static_cast<uint8_t*>(raw);
    p = r8 + gaguard::payload_off(G);
    goff = G;
    cap = want;
    size = bytes;
    if (g->poison) {
        e = hipMemset(r8, g->fill, total);
    } else {
        e = hipMemset(r8, g->fill, G);
        if (e == hipSuccess) e = hipMemset(r8 + gaguard::rear_off(bytes, G), g->fill, total - gaguard::rear_off(bytes, G));
    }
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    return e;
}

void DevBuf::release_checked() {
    // best effort: the caller is on an error path of its own, and a scan that fails loses only this evidence
    if (g && p && guard_quiesce(g) == hipSuccess) (void)guard_scan_dev(*this, true, true, g->pending);
    release();
}

hipError_t PinBuf::ensure_guarded(size_t bytes) {
    const size_t G = g->G;
    if (bytes <= cap && p) {
        if (bytes == size) return hipSuccess;
        if (hipError_t e = guard_quiesce(g); e != hipSuccess) return e;
        guard_scan_pin(*this, false, true, g->pending);
        const gaguard::Range r = gaguard::relay_range(size, bytes, G);
        std::memset(static_cast<uint8_t*>(p) + r.lo, g->fill, r.hi - r.lo);
        size = bytes;
        return hipSuccess;
    }
    if (p) {
        if (hipError_t e = guard_quiesce(g); e != hipSuccess) return e;
        guard_scan_pin(*this, true, true, g->pending);
    }
    void* old = p ? static_cast<uint8_t*>(p) - goff : nullptr;
    p = dp = nullptr;
    cap = goff = size = 0;
    if (old)
        if (hipError_t e = hipHostFree(old); e != hipSuccess) return e;
    const unsigned flags = mapped ? hipHostMallocMapped | hipHostMallocCoherent : hipHostMallocDefault;
    const size_t total = gaguard::alloc_bytes(bytes, G);
    void* raw = nullptr;
    void* rawd = nullptr;
    hipError_t e = hipHostMalloc(&raw, total, flags);
    if (e != hipSuccess) return e;
    uint8_t* r8 = static_cast<uint8_t*>(raw);
    p = r8 + gaguard::payload_off(G);
    goff = G;
    cap = size = bytes;
    if (mapped) {
        e = hipHostGetDevicePointer(&rawd, raw, 0);
        if (e != hipSuccess) return e;
        dp = static_cast<uint8_t*>(rawd) + gaguard::payload_off(G);
    }
    if (g->poison) {
        std::memset(r8, g->fill, total);
    } else {
        std::memset(r8, g->fill, G);
        std::memset(r8 + gaguard::rear_off(bytes, G), g->fill, G);
    }
    return hipSuccess;
}

static_assert(gaplan::kFillRows == ga::FROWS, "the planner's chunk rows (ga_plan.h)");
static_assert(ga::COLCK_PAD == 64, "rc_rows_fit (ga_check.h) assumes a 64-row pad");

int check_ctx(ga_ctx* c) {
    if (!c) return fail(GA_E_ARG, "null context");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return fail(GA_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    return GA_OK;
}

// ---------------------------------------------------------------- guard mode
// Every buffer of the context and of its pipeline slots under its member name ("colck", "fb.tb", "pipe2.fb.tb").
// `link` stays outside: it is exported through an IPC handle, which names the allocation and not a pointer inside
// it, so an importer would land on the front guard; ga_debug_guard_report lists it as unguarded.
template <typename F, typename P>
void guard_each(ga_ctx* c, F&& dev, P&& pin) {
    auto fillbufs = [&](FillBufs& fb, const std::string& pre) {
#define GA_FB(x) dev(fb.x, pre + "fb." #x)
        GA_FB(tb), GA_FB(hand), GA_FB(flags), GA_FB(out_last), GA_FB(GVp), GA_FB(GHp), GA_FB(top), GA_FB(left);
        GA_FB(bnd_row), GA_FB(bnd_col), GA_FB(meta), GA_FB(bscr);
#undef GA_FB
    };
#define GA_D(x) dev(c->x, #x)
#define GA_P(x) pin(c->x, #x)
    GA_D(a), GA_D(b), GA_D(sub), GA_D(gh), GA_D(gv), GA_D(qp), GA_D(full), GA_D(rng), GA_D(ckpt), GA_D(ops), GA_D(result);
    fillbufs(c->fb, "");
    GA_D(halo_in), GA_D(dbg), GA_D(wdbg), GA_D(colck), GA_D(stck), GA_D(rc_tb), GA_D(rc_flags), GA_D(rc_pos), GA_D(rc_own);
    GA_D(qprof), GA_D(bt_codes), GA_D(bt_items), GA_D(bt_sub), GA_D(bt_gh), GA_D(bt_gv), GA_D(bt_ticket), GA_D(bt_out);
    GA_D(bt_scratch), GA_D(bt_witems), GA_D(bt_rng), GA_D(bt_ops), GA_D(bt_walk), GA_D(bt_tb), GA_D(bt_ritems);
    GA_D(bt_rstatus), GA_D(bt_rbase), GA_D(jlut), GA_D(bs_words), GA_D(bs_tb), GA_D(bs_witems), GA_D(bs_ticket);
    GA_D(bc_out), GA_D(bc_ticket), GA_D(bc_scratch);
    GA_D(br_table), GA_D(br_toff), GA_D(br_out), GA_D(br_ranks), GA_D(br_items), GA_D(br_ticket);
    GA_D(bm_table), GA_D(bm_toff), GA_D(bm_ooff), GA_D(bm_out), GA_D(bm_count), GA_D(bm_ticket);
#define GA_PP(x) pin(c->pipe.x, #x)
    GA_P(res_pin), GA_P(prog), pin(c->pipe.pin, "pipe_pin"), GA_PP(chain_tab), GA_PP(chain_ctl), GA_PP(chain_io);
    GA_P(rc_ops_pin), GA_P(rc_ops_prog), GA_P(up_pin);
#undef GA_D
#undef GA_P
#undef GA_PP
    for (int s = 0; s < 6; s++) {
        auto& sl = c->pipe.slot[s];
        const std::string pre = "pipe" + std::to_string(s) + ".";
        fillbufs(sl.fb, pre);
        dev(sl.rng, pre + "rng"), dev(sl.ops, pre + "ops"), dev(sl.result, pre + "result");
        pin(sl.tab_pin, pre + "tab_pin");
    }
}
static_assert(sizeof(Pipeline::slot) / sizeof(PipeSlot) == 6, "guard_each walks six pipeline slots");

void guard_attach(ga_ctx* c) {
    GuardCfg* g = &c->guard;
    guard_each(
        c,
        [&](DevBuf& b, const std::string& name) {
            b.g = g;
            b.name = name;
            g->dev.push_back(&b);
        },
        [&](PinBuf& b, const std::string& name) {
            b.g = g;
            b.name = name;
            g->pin.push_back(&b);
        });
}

// Every guard of the context against the pattern, with what earlier re-lays kept: the device is idle first (a
// synchronous entry has waited for its own work; this also covers a pipeline's other streams).  `relay` restores the
// pattern where it was found changed, so that one stray store is reported once and the context stays usable.
int guard_collect(ga_ctx* c, bool relay, std::vector<gaguard::Violation>& out) {
    GuardCfg* g = &c->guard;
    out = g->pending;
    if (relay) g->pending.clear();
    HIPCHK(hipDeviceSynchronize());
    for (DevBuf* b : g->dev) {
        const size_t n0 = out.size();
        HIPCHK(guard_scan_dev(*b, true, true, out));
        if (relay)
            for (size_t k = n0; k < out.size(); k++) {
                uint8_t* at = b->as<uint8_t>() + (out[k].side == gaguard::kFront ? -(ptrdiff_t)g->G : (ptrdiff_t)b->size);
                HIPCHK(hipMemset(at, g->fill, g->G));
            }
    }
    for (PinBuf* b : g->pin) {
        const size_t n0 = out.size();
        guard_scan_pin(*b, true, true, out);
        if (relay)
            for (size_t k = n0; k < out.size(); k++)
                std::memset(b->host<uint8_t>() + (out[k].side == gaguard::kFront ? -(ptrdiff_t)g->G : (ptrdiff_t)b->size),
                            g->fill, g->G);
    }
    if (relay) HIPCHK(hipStreamSynchronize(nullptr));
    return GA_OK;
}

// The end of a synchronous entry that may have run kernels: its own result, or GA_E_GUARD with the report.
int guard_end(ga_ctx* c, int rc) {
    if (!c || !c->guard.G) return rc;
    const std::string msg = rc == GA_OK ? std::string() : g_err;
    std::vector<gaguard::Violation> vs;
    if (guard_collect(c, true, vs) != GA_OK) return rc != GA_OK ? fail(rc, msg) : GA_E_HIP;
    if (vs.empty()) return rc != GA_OK ? fail(rc, msg) : GA_OK;
    return fail(GA_E_GUARD, "guard violated: " + gaguard::describe(vs) +
                                (rc == GA_OK ? std::string() : " (the call itself failed with " + std::to_string(rc) + ": " + msg + ")"));
}

// The loaded problem or slab as the fill planner sees it (ga_plan.h).
gaplan::Problem plan_problem(const ga_ctx* c) {
    gaplan::Problem pb;
    pb.m = c->m;
    pb.n = c->n;
    pb.n_global = c->n_global;
    pb.col0 = c->col0;
    pb.K = c->K;
    pb.CB = c->CB;
    pb.qbytes = c->qbytes;
    pb.o = c->o;
    pb.num_cu = c->num_cu;
    pb.qrows = c->qrows;
    pb.slab = c->slab;
    pb.in_linked = c->in_prog_ext != nullptr;
    pb.out_linked = c->out_prog_ext != nullptr;
    pb.custom = c->custom;
    return pb;
}

// sub' = sub - gV - gH, K x K: what every fill adds per cell in the shifted domain
std::vector<int> shifted_sub(const ga_costs* cs) {
    const int K = cs->K;
    std::vector<int> subp((size_t)K * K);
    for (int x = 0; x < K; x++)
        for (int y = 0; y < K; y++) subp[x * K + y] = cs->sub[x * K + y] - cs->gap_v[x] - cs->gap_h[y];
    return subp;
}

int load_problem(ga_ctx* c, const uint8_t* a, int64_t m, const uint8_t* b_all, int64_t n_all, const ga_costs* cs,
                 const int32_t* row0, const int32_t* col0, int64_t cb, int64_t ce) {
    ProblemShape ps;
    std::string why;
    if (int r = check_problem(a, m, b_all, n_all, cs, row0, col0, cb, ce, ps, why)) return fail(r, why);
    const int K = cs->K;
    const int o = cs->gap_open;
    const int64_t big = ps.big;
    c->qbytes = ps.qbytes;
    c->CB = ps.CB;
    c->m = m;
    c->n = ce - cb;
    c->n_global = n_all;
    c->col0 = cb;
    c->K = K;
    c->o = o;
    c->big = (int)big;
    c->custom = row0 != nullptr || col0 != nullptr;
    c->gh_total = 0;  // GH(n) of the whole problem (the cost's un-shift), and the largest GH(j) of any column: the
    c->gh_max = INT64_MIN;  // lean ramp's uniform-row-0 test (enqueue_fill)
    for (int64_t j = 0; j < n_all; j++) {
        c->gh_total += cs->gap_h[b_all[j]];
        c->gh_max = std::max(c->gh_max, c->gh_total);
    }
    c->gv_total = 0;  // GV(m): the cost's un-shift (cost = H'(m, n) + GV(m) + GH(n))
    for (int64_t i = 0; i < m; i++) c->gv_total += cs->gap_v[a[i]];
    c->h_a.assign(a, a + m);
    c->h_b.assign(b_all, b_all + n_all);
    HIPCHK(c->a.ensure(m));
    HIPCHK(c->b.ensure(n_all));
    HIPCHK(c->sub.ensure(sizeof(int) * K * K));
    HIPCHK(c->gh.ensure(sizeof(int) * K));
    HIPCHK(c->gv.ensure(sizeof(int) * K));
    HIPCHK(hipMemcpyAsync(c->a.p, a, m, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->b.p, b_all, n_all, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->sub.p, cs->sub, sizeof(int) * K * K, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->gh.p, cs->gap_h, sizeof(int) * K, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->gv.p, cs->gap_v, sizeof(int) * K, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c->fb.ensure_boundary(m, n_all));
    if (c->custom) {
        HIPCHK(hipMemcpyAsync(c->fb.bnd_row.p, row0, sizeof(int) * 3 * (n_all + 1), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->fb.bnd_col.p, col0, sizeof(int) * 3 * (m + 1), hipMemcpyHostToDevice, c->stream));
    }
    {
        // sub', read by the fill's IO wave into its LDS query profile
        const std::vector<int> subp = shifted_sub(cs);
        HIPCHK(c->qp.ensure(sizeof(int) * K * K));
        HIPCHK(hipMemcpy(c->qp.p, subp.data(), sizeof(int) * K * K, hipMemcpyHostToDevice));
        // query-profile ring: as many rows as fit 64 KB (at least 128)
        c->qrows = 1024;
        while (c->qrows > 128 && (size_t)K * c->qrows * c->qbytes > 64 * 1024) c->qrows >>= 1;
        if (std::max(ga::fill_lds_bytes(8, c->qbytes, K, c->qrows, 8192), ga::fill_diag_lds_bytes(8, c->qbytes, K, c->qrows)) >
            160 * 1024)
            return fail(GA_E_RANGE, "alphabet too large for the LDS query profile");
    }
    // the loaded problem's row-scan geometry, until a fill plans its own: one stripe (64 columns) per compute wave;
    // a workgroup (one per CU) chains 4 waves (one per SIMD: the fastest rows) when every stripe gets a wave that
    // way, else 8 (two per SIMD)
    c->plan = gaplan::row_plan(plan_problem(c), c->pk);
    HIPCHK(c->result.ensure(sizeof(int) * 16));
    HIPCHK(c->ops.ensure(m + n_all + 1024));  // 2-bit levels; the walk flushes whole 128-byte blocks
    HIPCHK(c->rng.ensure(sizeof(uint32_t) * (m + n_all + 2 + 64)));  // + the walk's entry look-ahead (SLD)
    HIPCHK(hipStreamSynchronize(c->stream));
    c->loaded = true;
    c->filled_tb = false;
    return GA_OK;
}

// Device memory a buffer may take: hipMemGetInfo's free bytes plus `held` (what the context's own buffers being
// resized already hold), less a 2 GB margin; GA_DEV_AVAIL_MB caps it (tests: forces the fallbacks).
int64_t dev_avail_bytes(ga_ctx* c, int64_t held) {
    int64_t avail = INT64_MAX / 4;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) avail = (int64_t)fr + held - ((int64_t)2 << 30);
    if (c->wk.dev_avail) avail = std::min(avail, *c->wk.dev_avail);
    return std::max<int64_t>(avail, 0);
}

// the recompute walk's block cache: the word walk's, and (experiments build) the tie-to-tie walk's entries
size_t rc_cache_bytes(bool jump, int TD, int CB) {
    // (+ one 64-column stripe of slack: a loader reads whole 1 KiB runs)
    return jump ? (size_t)ga::RC_CACHE_I * ga::RC_CACHE_S * 4 * TD * 6144 + 65536
                : (size_t)ga::RC_CACHE_I * ga::RC_CACHE_S * TD * 64 * 64 * CB + (size_t)64 * 64 * 4 * 4;
}

// ---------------------------------------------------------------- the planner's inputs (ga_plan.h)
const gaplan::LdsSizes kLdsSizes{ga::fill_lane_lds_bytes, ga::rc_worker_bytes, rc_cache_bytes};

// ---------------------------------------------------------------- one fill: plan, buffers, arguments, launch
// What the four stages of enqueue_fill share: the request, its plan, and where this fill reads and writes.
struct FillJob {
    const Band& bd;
    gaplan::FillPlan pl;
    FillBufs& fb;
    hipStream_t st;
    bool tb, full;
    int64_t m, n;  // the rows and columns this fill covers (a band's, else the problem's)
    bool lane() const { return pl.kind == gaplan::kLane; }
};

// 1. The plan (ga_plan.h).  An error returns before anything is enqueued.
int fill_plan(ga_ctx* c, const Band& bd, bool tb, bool full, gaplan::FillPlan& pl) {
    gaplan::Request rq = bd;
    rq.tb = tb;
    rq.full = full;
    rq.has_ckpt = bd.ckpt != nullptr;
    gaplan::Knobs kn = c->pk;
    // what the checkpoints may take: the free device memory plus what this context's checkpoint buffers already hold
    if (bd.rc) kn.dev_avail = dev_avail_bytes(c, (int64_t)c->stck.cap + (int64_t)c->colck.cap + (int64_t)c->rc_tb.cap);
    pl = gaplan::plan_fill(plan_problem(c), rq, kn, kLdsSizes);
    return pl.err ? fail(pl.err, pl.msg) : GA_OK;
}

// 2. The buffers at the plan's sizes, and their presets on the fill's stream.
int fill_buffers(ga_ctx* c, const FillJob& j) {
    const gaplan::FillPlan& pl = j.pl;
    const int64_t m = j.m, n = j.n;
    HIPCHK(j.fb.out_last.ensure(sizeof(int) * 4));
    // traceback words cover T 64-column stripes per fill stripe
    if (j.tb) HIPCHK(j.fb.tb.ensure((size_t)pl.nstripes * pl.T * pl.TC * 1024));
    HIPCHK(j.fb.hand.ensure(sizeof(int2) * (size_t)pl.nslabs * (m + 1)));
    // workgroup hand-off rows read by a successor start as ga::HAND_SENT (bytes 0x80)
    if (pl.nslabs > 1)
        HIPCHK(hipMemsetAsync(j.fb.hand.p, 0x80, sizeof(int2) * (size_t)(pl.nslabs - 1) * (m + 1), j.st));
    HIPCHK(j.fb.flags.ensure(sizeof(unsigned) * 16));
    if (j.full) HIPCHK(c->full.ensure(sizeof(int) * 3 * (m + 1) * (n + 1)));
    // flags layout: [0] ticket, [1] abort
    HIPCHK(hipMemsetAsync(j.fb.flags.p, 0, sizeof(unsigned) * 16, j.st));
    if (j.bd.rc) {
        const int64_t nck = std::max<int64_t>((m - 1) / pl.rc_every, 1);
        // An allocation that fails (the plan's size check passed, but the device's free memory moved) releases every
        // recompute buffer before GA_E_NOMEM, so the fallback (ga_problem_align: banded / stored words) sizes
        // itself with that memory free.  The memsets enqueued above are harmless: the fallback's own fill
        // enqueues them again behind them on the same stream.  GA_RC_FAIL_ALLOC=1 (tests) fails the second
        // allocation after the first succeeded.
        const bool fail_test = c->lk.rc_fail_alloc;
        int nb = 0;
        for (auto [buf, bytes] : {std::pair<DevBuf*, size_t>{&c->colck, sizeof(int2) * (size_t)pl.nstripes * (m + 1 + ga::COLCK_PAD)},
                                  {&c->stck, sizeof(int2) * (size_t)nck * pl.nstripes * (pl.T + 1) * 64}}) {
            hipError_t e = buf->ensure(bytes);
            if (e == hipSuccess && fail_test && nb == 1) e = hipErrorOutOfMemory;
            nb++;
            if (e != hipSuccess) {
                (void)hipGetLastError();
                c->colck.release_checked();
                c->stck.release_checked();
                c->rc_tb.release_checked();
                return fail(e == hipErrorOutOfMemory ? GA_E_NOMEM : GA_E_HIP,
                            std::string("recompute checkpoints: ") + hipGetErrorString(e));
            }
        }
    }
    if (c->dbg_on) {
        HIPCHK(c->dbg.ensure(sizeof(unsigned long long) * ga::LK_DBG_WORDS * pl.nstripes));
        HIPCHK(hipMemsetAsync(c->dbg.p, 0, sizeof(unsigned long long) * ga::LK_DBG_WORDS * pl.nstripes, j.st));
    }
    // the lane fill's query profile (K x (m + 4) dwords: C5 1.9 MB)
    if (j.lane() && !c->lk.qprof_wave)  // (experiments build: the profile wave builds it, for A/B)
        HIPCHK(c->qprof.ensure(sizeof(uint32_t) * (size_t)c->K * (size_t)(m + 4)));
    return GA_OK;
}

// The launch-time knobs of the lane kernel (gaopts::LaneKnobs; tuning, A/B runs and tests: none changes the plan).
void fill_launch_knobs(const ga_ctx* c, const FillJob& j, ga::FillArgs& p) {
    const gaopts::LaneKnobs& lk = c->lk;
    const bool one_round = j.lane() && j.pl.nslabs <= c->num_cu;
    // one round of lane workgroups (every stripe resident): the chain's lag counts, read edges late
    p.late = lk.late.value_or(one_round ? 1 : 0);
    // chain neighbours on one XCD (ga_lane.hip lane_slab; experiments build only): measured no faster, since ticket
    // order already keeps 165 of C3's 195 cross-workgroup links on one XCD (r5: 188 with the map; C3 fill 9.43 ->
    // 9.46 ms, tools/exp/r5/xcd.sh).  Only for one round of workgroups that runs alone (a pipeline's fills share
    // the device; a fill that finds its workgroups not all resident falls back to ticket order after ~40 us)
    p.xcd_map = one_round && j.bd.stream == nullptr ? lk.xcd : 0;
    // measured: C4 210 ms against 221 with the direct hand-off, 1M x 125k 52.5 against 56 (r3_c4.log)
    p.hand_direct = lk.hand_direct;
    p.lds_floor = lk.lds_floor;
    p.lane_sub = lk.lane_sub;
    p.lane_tb_sub = lk.lane_tb_sub;
    p.asm_step = lk.asm_step;
    p.io_prio = lk.io_prio;
    p.hand_scope = lk.hand_scope;
    p.poll_win = lk.poll_win;
    p.out_wave = lk.out_wave;
    p.spin_limit = 1u << 26;        // ~seconds: only a broken hand-off can reach it
    p.halo_spin_limit = lk.halo_spin_limit.value_or(1u << 30);  // waiting on another GPU may take long (~30 s)
    // a slab with a left neighbour: every wait of its fill is, in the end, a wait for that halo
    if (c->slab && c->col0 > 0) p.spin_limit = std::max(p.spin_limit, p.halo_spin_limit);
    // the lean ramp (ga_lane.hip lean0): row 0 is the reference's boundary and uniform in the shifted domain (H' = o,
    // h2' = 2o in every column: 2o + GH(j) <= big for every j, so for the largest prefix sum, which is GH(n) only
    // when no gap cost is negative); GA_LANE_LEAN0=0 keeps the masked ramp (A/B)
    p.lean0 = lk.lean0 && j.lane() && !c->custom && j.bd.top == nullptr && !j.bd.band &&
              2 * (int64_t)c->o + c->gh_max <= (int64_t)c->big;
}

// 3. The kernels' arguments.
ga::FillArgs fill_args(const ga_ctx* c, const FillJob& j) {
    const gaplan::FillPlan& pl = j.pl;
    const Band& bd = j.bd;
    ga::FillArgs p{};
    p.a = c->a.as<uint8_t>() + bd.r0;
    p.ckpt = bd.ckpt;
    p.ckpt_rows = bd.ckpt_rows;
    p.colck = bd.rc ? c->colck.as<int2>() : nullptr;
    p.stck = bd.rc ? c->stck.as<int2>() : nullptr;
    p.stck_every = pl.rc_every;
    p.stck_shift = 0;
    while ((1 << p.stck_shift) < pl.rc_every) p.stck_shift++;
    fill_launch_knobs(c, j, p);
    p.subp = c->qp.as<int>();
    p.K = c->K;
    p.b = c->b.as<uint8_t>() + c->col0;
    p.top = (bd.top ? bd.top : j.fb.top.as<int2>()) + c->col0;
    if (c->slab && c->col0 > 0) {
        p.left = c->halo_in_ext ? c->halo_in_ext : c->halo_in.as<int2>();
        p.left_prog = c->in_prog_ext ? c->in_prog_ext : c->prog.dev<uint32_t>();  // [0]: halo_in rows
    } else {
        p.left = j.fb.left.as<int2>() + bd.r0;
        p.left_prog = nullptr;
    }
    p.hand = j.fb.hand.as<int2>();
    p.ticket = j.fb.flags.as<unsigned>();
    p.abort_word = p.ticket + 1;
    p.tb = j.tb ? j.fb.tb.as<uint8_t>() : nullptr;
    p.out_last = j.fb.out_last.as<int>();
    p.edge_prog = c->slab ? (c->out_prog_ext ? c->out_prog_ext : c->prog.dev<uint32_t>() + 1) : nullptr;  // [1]: halo_out rows
    p.edge_out = c->slab ? c->halo_out_ext : nullptr;
    p.full = j.full ? c->full.as<int>() : nullptr;
    p.m = (int)j.m;
    p.n = (int)j.n;
    p.o = c->o;
    p.nstripes = pl.nstripes;
    p.nslabs = pl.nslabs;
    p.TC = pl.TC;
    p.nwc = pl.nwc;
    p.qrows = pl.qrows;
    p.cols_per_lane = pl.T;
    p.dbg = c->dbg_on ? c->dbg.as<unsigned long long>() : nullptr;
    p.qprof = j.lane() && !c->lk.qprof_wave ? c->qprof.as<uint32_t>() : nullptr;
    return p;
}

// 4. The launches: the boundary pass, the lane fill's query profile, the fill between its two timing events.
int fill_launch(ga_ctx* c, const FillJob& j, const ga::FillArgs& p) {
    FillBufs& fb = j.fb;
    if (!j.bd.band)
        ga::launch_boundary(j.st, c->a.as<uint8_t>(), (int)j.m, c->b.as<uint8_t>(), (int)c->n_global,
                            c->gh.as<int>(), c->gv.as<int>(), c->o, c->big, fb.GVp.as<int>(), fb.GHp.as<int>(),
                            fb.top.as<int2>(), fb.left.as<int2>(), fb.bnd_row.as<int>(), fb.bnd_col.as<int>(),
                            fb.meta.as<int>(), c->custom, fb.bscr.as<int>());
    // the query profile is built on the fill's stream just before it (a few us).  Fills of one problem in flight on
    // other streams (align_many) rewrite it with the same values.
    if (p.qprof) ga::launch_lane_qprof(j.st, p.a, (int)j.m, p.subp, c->K, c->qprof.as<uint32_t>());
    HIPCHK(hipEventRecord(fb.ev[0], j.st));
    if (j.lane()) ga::launch_fill_lane(j.st, p, c->CB);
    else if (j.pl.kind == gaplan::kDiag) ga::launch_fill_diag(j.st, p, c->qbytes, j.full);
    else ga::launch_fill(j.st, p, c->CB, c->qbytes, j.tb, j.full);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(fb.ev[1], j.st));
    return GA_OK;
}

// Enqueue boundary + query profile + fill.  Does not synchronise.  The plan it used becomes the context's
// (ga_ctx::plan) and goes to plan_out.
int enqueue_fill(ga_ctx* c, int32_t flags, const Band& bd, gaplan::FillPlan* plan_out) {
    if (!c->loaded) return fail(GA_E_STATE, "no problem loaded");
    const bool tb = (flags & (GA_FILL_TRACEBACK | GA_FILL_FULL)) != 0;
    const bool full = (flags & GA_FILL_FULL) != 0;
    gaplan::FillPlan pl;
    if (int r = fill_plan(c, bd, tb, full, pl)) return r;
    c->plan = pl;
    if (plan_out) *plan_out = pl;
    const FillJob j{bd, pl, bd.bufs ? *bd.bufs : c->fb, bd.stream ? bd.stream : c->stream, tb, full,
                    bd.band ? bd.mb : c->m, bd.band && bd.nc > 0 ? bd.nc : c->n};
    if (int r = fill_buffers(c, j)) return r;
    if (int r = fill_launch(c, j, fill_args(c, j))) return r;
    c->filled_tb = tb;
    return GA_OK;
}

int finish_fill(ga_ctx* c, int64_t* cost_out, int32_t* full_out) {
    int last[4] = {0, 0, 0, 0}, meta[2] = {0, 0};
    unsigned abort_word = 0;
    HIPCHK(hipMemcpyAsync(last, c->fb.out_last.p, sizeof(int) * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(meta, c->fb.meta.p, sizeof(int) * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&abort_word, c->fb.flags.as<unsigned>() + 1, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipEventElapsedTime(&c->fill_ms, c->fb.ev[0], c->fb.ev[1]));
    if (abort_word) return fail(GA_E_TIMEOUT, "fill kernel hand-off wait timed out");
    c->GV_m = meta[0];
    // un-shift: cost = H'(m, n) + GV(m) + GH(column)
    int64_t gh_end = 0;
    {
        int v = 0;
        HIPCHK(hipMemcpy(&v, c->fb.GHp.as<int>() + c->col0 + c->n, sizeof(int), hipMemcpyDeviceToHost));
        gh_end = v;
    }
    if (cost_out) *cost_out = (int64_t)last[0] + c->GV_m + gh_end;
    if (full_out) {
        const int64_t m = c->m, n = c->n, W = n + 1;
        std::vector<int> GV(m + 1), GH(n + 1);
        HIPCHK(hipMemcpy(GV.data(), c->fb.GVp.p, sizeof(int) * (m + 1), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(GH.data(), c->fb.GHp.p, sizeof(int) * (n + 1), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(full_out, c->full.p, sizeof(int) * 3 * (m + 1) * W, hipMemcpyDeviceToHost));
        std::vector<int> br(3 * (n + 1)), bc(3 * (m + 1));
        HIPCHK(hipMemcpy(br.data(), c->fb.bnd_row.p, sizeof(int) * br.size(), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(bc.data(), c->fb.bnd_col.p, sizeof(int) * bc.size(), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i <= m; i++)
            for (int64_t j = 0; j <= n; j++) {
                int* f = full_out + 3 * (i * W + j);
                if (i == 0) { f[0] = br[3 * j]; f[1] = br[3 * j + 1]; f[2] = br[3 * j + 2]; }
                else if (j == 0) { f[0] = bc[3 * i]; f[1] = bc[3 * i + 1]; f[2] = bc[3 * i + 2]; }
                else {
                    const int sh = GV[i] + GH[j];
                    f[0] += sh; f[1] += sh; f[2] += sh;
                }
            }
    }
    return GA_OK;
}

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace gahost

// ====================================================================== C ABI
extern "C" {

const char* ga_last_error(void) { return g_err.c_str(); }

int ga_device_count(int* count) {
    if (!count) return fail(GA_E_ARG, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(GA_E_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    *count = n;
    return GA_OK;
}

int ga_ctx_create(int device, ga_ctx** out) { return ga_ctx_create_opts(device, nullptr, out); }

int ga_ctx_create_opts(int device, const char* options, ga_ctx** out) {
    if (!out) return fail(GA_E_ARG, "null out");
    // the knobs, once (ga_opts.h): the environment's shipped ones, then the options, checked before any device work
    // (an experiments build, make EXPERIMENTS=1, takes every GA_* variable and reads the dropped paths' knobs: xget)
#ifdef GA_EXPERIMENTS
    constexpr bool experiments = true;
#else
    constexpr bool experiments = false;
#endif
    gaopts::Map knobs;
    gaopts::GuardOpts guard;
    std::string why;
    if (int r = gaopts::collect(environ, options, experiments, knobs, why)) return fail(r, why);
    if (int r = gaopts::check(knobs, guard, why)) return fail(r, why);
    // the planner's self-test plans with the kernels' LDS formulas as ga_plan.h restates them: they must be the kernels'
    for (int every : {64, 128, 4096})
        for (int w : {1, 2, 4, 8})
            if (gaplan::restated_fill_lane_lds_bytes(w, 4 * w, 4 * every) != ga::fill_lane_lds_bytes(w, 4 * w, 4 * every) ||
                gaplan::restated_rc_worker_bytes(w, w == 8 ? 1 : w, every) != ga::rc_worker_bytes(w, w == 8 ? 1 : w, every))
                return fail(GA_E_STATE, "ga_plan.h restates the kernels' LDS formulas wrongly");
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(GA_E_ARG, "no such HIP device");
    HIPCHK(hipSetDevice(device));
    ga_ctx* c = new ga_ctx();
    c->device = device;
    c->knobs = std::move(knobs);
    // every typed knob set, parsed here and nowhere else: `get` looks a name up, `xget` one of a path that was measured
    // and dropped, which only an experiments build (make EXPERIMENTS=1) reads
    const auto get = [c](const char* name) -> const char* {
        const auto it = c->knobs.find(name);
        return it == c->knobs.end() ? nullptr : it->second.c_str();
    };
    const auto xget = [&get](const char* name) -> const char* { return experiments ? get(name) : nullptr; };
    c->pk = gaplan::Knobs::parse(get, xget);
    c->wk = gawalk::Knobs::parse(get, xget);
    c->lk = gaopts::LaneKnobs::parse(get, xget);
    c->bk = gaopts::BatchKnobs::parse(get, xget);
    c->pipek = gapipe::Knobs::parse(get, xget);
    c->pipek.diag_req = c->pk.diag_req;
    if (guard.bytes) {
        c->guard.G = guard.bytes;
        c->guard.fill = (uint8_t)guard.fill;
        c->guard.poison = guard.poison;
        guard_attach(c);
    }
    {
        // hardware queues per priority pool: what the HIP runtime read when it started, i.e. the variable
        // as the process first saw it here (a later change, e.g. a module setting it after HIP started,
        // does not change the runtime's queues)
        static const int hwq = [] {
            const char* e = getenv("GPU_MAX_HW_QUEUES");
            return e && atoi(e) > 0 ? atoi(e) : 4;
        }();
        c->hw_queues = hwq;
    }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
            c->num_cu = cus;
    }
    // The fill runs on a stream of the greatest priority.  HIP keeps a separate pool of hardware
    // queues per priority (GPU_MAX_HW_QUEUES = 4 per pool and process), so no normal-priority
    // stream -- torch's, RCCL's -- is ever put behind a running fill in the same in-order queue;
    // a slab fill that waits on its halo needs the RCCL kernel that delivers it to run beside it
    // (DESIGN.md 7).  GA_STREAM_PRIORITY=normal restores a default-priority stream (experiments).
    {
        int lo = 0, hi = 0;
        const bool normal = gaopts::stream_priority_normal(get);
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = hi = 0;
        c->priority = normal ? 0 : hi;  // 0: the default priority (lo is the LEAST, another pool)
        if (hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, c->priority) != hipSuccess) {
            delete c;
            return fail(GA_E_HIP, "hipStreamCreateWithPriority failed");
        }
    }
    if (hipEventCreateWithFlags(&c->ev_dep, hipEventDisableTiming) != hipSuccess) {
        delete c;
        return fail(GA_E_HIP, "hipEventCreate failed");
    }
    for (hipEvent_t* e : {&c->fb.ev[0], &c->fb.ev[1], &c->wev[0], &c->wev[1]}) {
        if (hipEventCreate(e) != hipSuccess) {
            delete c;
            return fail(GA_E_HIP, "hipEventCreate failed");
        }
    }
    *out = c;
    return GA_OK;
}

void ga_ctx_destroy(ga_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->guard.G) {
        // the last look at the guards: nobody is left to take an error code
        std::vector<gaguard::Violation> vs;
        if (guard_collect(c, false, vs) == GA_OK && !vs.empty())
            std::fprintf(stderr, "globalign_amd: guard violated at ga_ctx_destroy: %s\n", gaguard::describe(vs).c_str());
    }
    if (c->peer_link) (void)hipIpcCloseMemHandle(c->peer_link);
    if (c->ev_up) (void)hipEventDestroy(c->ev_up);
    if (c->ev_fill) (void)hipEventDestroy(c->ev_fill);
    if (c->ev_res) (void)hipEventDestroy(c->ev_res);
    if (c->ustream) (void)hipStreamDestroy(c->ustream);
    for (hipEvent_t e : {c->fb.ev[0], c->fb.ev[1], c->wev[0], c->wev[1], c->rev[0], c->rev[1]})
        if (e) (void)hipEventDestroy(e);
    if (c->ev_dep) (void)hipEventDestroy(c->ev_dep);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;  // the device and pinned buffers free themselves (DevBuf, PinBuf), the pipeline its streams and events
}

// ga_problem_set and the other entries that run kernels and wait for them: the exported definitions, which end each
// with guard mode's check, stand together at the end of the file (guard mode); the bodies are the *_impl.
static int problem_set_impl(ga_ctx* c, const uint8_t* a, int64_t m, const uint8_t* b, int64_t n, const ga_costs* cs,
                            const int32_t* row0, const int32_t* col0) {
    if (int r = check_ctx(c)) return r;
    c->slab = false;
    return load_problem(c, a, m, b, n, cs, row0, col0, 0, n);
}

static int problem_fill_impl(ga_ctx* c, int32_t flags, int64_t* cost_out, int32_t* full_out) {
    if (c) c->rc_used = false;
    if (int r = check_ctx(c)) return r;
    if (c->slab) return fail(GA_E_STATE, "slab contexts use ga_slab_fill_launch");
    if ((flags & GA_FILL_FULL) && !full_out) return fail(GA_E_ARG, "GA_FILL_FULL needs full_out");
    if (int r = enqueue_fill(c, flags)) return r;
    return finish_fill(c, cost_out, (flags & GA_FILL_FULL) ? full_out : nullptr);
}

int ga_debug_seed_state(uint64_t seed, uint32_t* state_out) {
    if (!state_out) return fail(GA_E_ARG, "null argument");
    seed_state(seed, state_out);
    return GA_OK;
}

static int problem_set_cells_impl(ga_ctx* c, const int32_t* cells, int64_t* cost_out) {
    if (int r = check_ctx(c)) return r;
    if (!c->loaded) return fail(GA_E_STATE, "no problem loaded");
    if (c->slab) return fail(GA_E_STATE, "slab contexts fill their own cells");
    if (!cells || !cost_out) return fail(GA_E_ARG, "null argument");
    const int64_t m = c->m, n = c->n;
    if ((m + 1) * (n + 1) > (int64_t)64 << 20) return fail(GA_E_RANGE, "ga_problem_set_cells is for small problems");
    // words in a fill's layout, 16-row chunks of CB 16-byte words per lane: the walk reads them at the plan's TC
    const int TC = (int)((m + ga::FROWS - 1) / ga::FROWS) * c->CB;
    gaplan::FillPlan pl = c->plan;
    pl.TC = TC;
    c->plan = pl;
    HIPCHK(c->fb.tb.ensure((size_t)((n + 63) / 64) * TC * 1024));
    HIPCHK(c->full.ensure(sizeof(int) * 3 * (m + 1) * (n + 1)));
    HIPCHK(hipMemcpyAsync(c->full.p, cells, sizeof(int) * 3 * (m + 1) * (n + 1), hipMemcpyHostToDevice, c->stream));
    ga::launch_tb_from_cells(c->stream, c->full.as<int>(), (int)m, (int)n, c->o, c->CB, TC, c->fb.tb.as<uint8_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    const int32_t* last = cells + 3 * (m * (n + 1) + n);
    *cost_out = std::min(std::min(last[0], last[1]), last[2]);  // min(dp_array[m][n]) (globaligner.py:425)
    c->filled_tb = true;
    return GA_OK;
}

// ---------------------------------------------------------------- slabs
static int problem_set_slab_impl(ga_ctx* c, const uint8_t* a, int64_t m, const uint8_t* b, int64_t n,
                                 const ga_costs* cs, int64_t col_begin, int64_t col_end) {
    if (int r = check_ctx(c)) return r;
    c->slab = true;
    c->halo_in_ext = c->halo_out_ext = nullptr;
    c->in_prog_ext = c->out_prog_ext = nullptr;
    c->walk_rng_ready = false;
    if (int r = load_problem(c, a, m, b, n, cs, nullptr, nullptr, col_begin, col_end)) return r;
    HIPCHK(c->halo_in.ensure(sizeof(int2) * (m + 1)));
    HIPCHK(c->prog.ensure(256));
    std::memset(c->prog.p, 0, 256);
    return GA_OK;
}

int ga_slab_bind_halos(ga_ctx* c, void* halo_in, void* halo_out) {
    if (int r = check_ctx(c)) return r;
    if (!c->slab) return fail(GA_E_STATE, "not a slab context");
    c->halo_in_ext = static_cast<int2*>(halo_in);
    c->halo_out_ext = static_cast<int2*>(halo_out);
    // bound halos go with the context's own (host-relayed) progress words, not a link's
    c->in_prog_ext = c->out_prog_ext = nullptr;
    return GA_OK;
}

// the right slab's side of a link: its left edge (m + 1 int2 rows) + progress word in uncached memory on
// its own GPU, bound as its halo_in / in_prog; the word zeroed (before any writer is launched)
static int link_alloc(ga_ctx* right, uint8_t** base_out) {
    HIPCHK(hipSetDevice(right->device));
    const size_t hbytes = sizeof(int2) * (size_t)(right->m + 1);
    right->link.uncached = true;
    HIPCHK(right->link.ensure(hbytes + 256));
    uint8_t* base = right->link.as<uint8_t>();
    auto* prog = reinterpret_cast<uint32_t*>(base + hbytes);
    HIPCHK(hipMemset(prog, 0, 256));
    right->halo_in_ext = reinterpret_cast<int2*>(base);
    right->in_prog_ext = prog;
    *base_out = base;
    return GA_OK;
}

int ga_slab_link(ga_ctx* left, ga_ctx* right) {
    if (int r = check_ctx(left)) return r;
    if (int r = check_ctx(right)) return r;
    if (left == right || !left->slab || !right->slab) return fail(GA_E_STATE, "ga_slab_link needs two slab contexts");
    if (left->m != right->m || left->col0 + left->n != right->col0)
        return fail(GA_E_ARG, "ga_slab_link: the slabs are not neighbours of one problem");
    if (left->device != right->device) {
        // left's fill stores into right's memory
        if (int r = ga_enable_peer_access(left->device, right->device)) return r;
    }
    uint8_t* base = nullptr;
    if (int r = link_alloc(right, &base)) return r;
    left->halo_out_ext = reinterpret_cast<int2*>(base);
    left->out_prog_ext = reinterpret_cast<uint32_t*>(base + sizeof(int2) * (size_t)(right->m + 1));
    return GA_OK;
}

int ga_slab_link_export(ga_ctx* right, void* handle_out) {
    if (int r = check_ctx(right)) return r;
    if (!handle_out) return fail(GA_E_ARG, "null argument");
    if (!right->slab || right->col0 == 0) return fail(GA_E_STATE, "ga_slab_link_export needs a slab with a left neighbour");
    uint8_t* base = nullptr;
    if (int r = link_alloc(right, &base)) return r;
    hipIpcMemHandle_t h;
    HIPCHK(hipIpcGetMemHandle(&h, base));
    std::memcpy(handle_out, &h, sizeof(h));
    return GA_OK;
}

int ga_slab_link_import(ga_ctx* left, const void* handle) {
    if (int r = check_ctx(left)) return r;
    if (!handle) return fail(GA_E_ARG, "null argument");
    if (!left->slab || left->col0 + left->n >= left->n_global)
        return fail(GA_E_STATE, "ga_slab_link_import needs a slab with a right neighbour");
    if (!left->peer_link || std::memcmp(left->peer_handle, handle, sizeof(left->peer_handle)) != 0) {
        if (left->peer_link) (void)hipIpcCloseMemHandle(left->peer_link);
        left->peer_link = nullptr;
        hipIpcMemHandle_t h;
        std::memcpy(&h, handle, sizeof(h));
        void* p = nullptr;
        HIPCHK(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
        left->peer_link = p;
        std::memcpy(left->peer_handle, handle, sizeof(left->peer_handle));
    }
    auto* base = static_cast<uint8_t*>(left->peer_link);
    left->halo_out_ext = reinterpret_cast<int2*>(base);
    left->out_prog_ext = reinterpret_cast<uint32_t*>(base + sizeof(int2) * (size_t)(left->m + 1));
    return GA_OK;
}

int ga_enable_peer_access(int device, int peer) {
    if (device == peer) return GA_OK;
    int can = 0;
    HIPCHK(hipDeviceCanAccessPeer(&can, device, peer));
    if (!can) return fail(GA_E_HIP, "device " + std::to_string(device) + " cannot access device " + std::to_string(peer));
    HIPCHK(hipSetDevice(device));
    const hipError_t e = hipDeviceEnablePeerAccess(peer, 0);
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
        return fail(GA_E_HIP, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
    (void)hipGetLastError();  // clear a sticky "already enabled"
    return GA_OK;
}

int ga_slab_buffers(ga_ctx* c, void** halo_in, uint32_t** halo_in_prog, void** halo_out, uint32_t** halo_out_prog) {
    if (int r = check_ctx(c)) return r;
    if (!c->slab) return fail(GA_E_STATE, "not a slab context");
    if (halo_in) *halo_in = c->halo_in_ext ? (void*)c->halo_in_ext : c->halo_in.p;
    if (halo_in_prog) *halo_in_prog = c->prog.host<uint32_t>();
    if (halo_out)
        *halo_out = c->halo_out_ext ? (void*)c->halo_out_ext
                                    : (void*)(c->fb.hand.as<int2>() + (size_t)(c->plan.nslabs - 1) * (c->m + 1));
    if (halo_out_prog) *halo_out_prog = c->prog.host<uint32_t>() + 1;
    return GA_OK;
}

int ga_slab_fill_launch(ga_ctx* c, int32_t flags) {
    if (int r = check_ctx(c)) return r;
    if (!c->slab) return fail(GA_E_STATE, "not a slab context");
    __atomic_store_n(c->prog.host<uint32_t>(), 0u, __ATOMIC_SEQ_CST);
    __atomic_store_n(c->prog.host<uint32_t>() + 1, 0u, __ATOMIC_SEQ_CST);
    c->rc_used = false;
    if ((flags & GA_FILL_TRACEBACK) && gawalk::rc_eligible(plan_problem(c), c->wk, true)) {
        // the slab's traceback by recompute: checkpoints instead of m * n words
        if (int r = rc_fill(c)) return r;
        c->filled_tb = true;
        return GA_OK;
    }
    return enqueue_fill(c, flags & GA_FILL_TRACEBACK);
}

static int slab_fill_finish_impl(ga_ctx* c, int64_t* cost_out) {
    if (int r = check_ctx(c)) return r;
    return finish_fill(c, cost_out, nullptr);
}

int ga_slab_walk_prepare(ga_ctx* c, const uint32_t* mt_state) {
    if (int r = check_ctx(c)) return r;
    if (!mt_state) return fail(GA_E_ARG, "null argument");
    const double t0 = now_ms();
    build_rng(mt_state, c->m + c->n_global + 1, c->walk_rng);
    c->rng_ms = (float)(now_ms() - t0);
    c->walk_rng_ready = true;
    return GA_OK;
}

static int slab_walk_impl(ga_ctx* c, ga_walk_state* st, const char* a_chr, const char* b_chr, char* oa, char* om,
                          char* ob, int64_t cap, int64_t* out_len) {
    if (int r = check_ctx(c)) return r;
    if (!st || !a_chr || !b_chr || !oa || !om || !ob || !out_len) return fail(GA_E_ARG, "null argument");
    if (!c->filled_tb) return fail(GA_E_STATE, "slab walk needs a GA_FILL_TRACEBACK fill first");
    if (!c->walk_rng_ready) return fail(GA_E_STATE, "call ga_slab_walk_prepare first");
    *out_len = 0;
    if (st->reason >= 0 && st->reason != 5) return GA_OK;  // the walk already ended to the right
    if (st->j != c->col0 + c->n) return fail(GA_E_ARG, "walk state is not at this slab's right edge");
    if (st->i < 1 || st->i > c->m) return fail(GA_E_ARG, "walk row out of range");
    WalkStart ws{st->i, st->j, st->D, st->h, st->L, st->first};
    int reason = 0;
    int64_t len = 0;
    if (c->rc_used) {
        WalkBufs wb = ctx_walk_bufs(c);
        const int64_t ntab = (int64_t)c->walk_rng.tab.size();
        HIPCHK(hipMemcpyAsync(wb.rng, c->walk_rng.tab.data(), sizeof(uint32_t) * ntab, hipMemcpyHostToDevice, wb.stream));
        if (int r = rc_walk_launch(c, ntab, ws, wb)) return r;
        if (int r = walk_segment(c, ws, reason, a_chr, b_chr, oa, om, ob, cap, len, &wb)) return r;
        if (reason == 7) return fail(GA_E_TIMEOUT, "recompute walk: a tile was never recomputed");
    } else {
        if (int r = run_walk(c, c->walk_rng.tab.data(), (int64_t)c->walk_rng.tab.size(), ws)) return r;
        if (int r = walk_segment(c, ws, reason, a_chr, b_chr, oa, om, ob, cap, len)) return r;
    }
    st->i = ws.i;
    st->j = ws.j;
    st->D = ws.D;
    st->h = ws.h;
    st->L = ws.L;
    st->first = ws.first;
    st->reason = reason;
    *out_len = len;
    return GA_OK;
}

int ga_slab_mt_state(ga_ctx* c, int64_t D, uint32_t* mt_out) {
    if (int r = check_ctx(c)) return r;
    if (!mt_out) return fail(GA_E_ARG, "null argument");
    if (!c->walk_rng_ready) return fail(GA_E_STATE, "call ga_slab_walk_prepare first");
    state_after(c->walk_rng, D, mt_out);
    return GA_OK;
}

int ga_stream_wait_ge(void* stream, uint32_t* prog, uint32_t value) {
    HIPCHK(hipStreamWaitValue32((hipStream_t)stream, prog, value, hipStreamWaitValueGte, 0xffffffffu));
    return GA_OK;
}

int ga_stream_write(void* stream, uint32_t* prog, uint32_t value) {
    HIPCHK(hipStreamWriteValue32((hipStream_t)stream, prog, value, 0));
    return GA_OK;
}

void* ga_ctx_stream(ga_ctx* c) { return c ? (void*)c->stream : nullptr; }

int ga_ctx_wait_stream(ga_ctx* c, void* stream) {
    if (int r = check_ctx(c)) return r;
    HIPCHK(hipEventRecord(c->ev_dep, (hipStream_t)stream));
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_dep, 0));
    return GA_OK;
}

int ga_ctx_stream_priority(ga_ctx* c, int* priority) {
    if (!c || !priority) return fail(GA_E_ARG, "null argument");
    *priority = c->priority;
    return GA_OK;
}

int ga_last_kernel_ms(ga_ctx* c, float* fill_ms, float* walk_ms) {
    if (!c) return fail(GA_E_ARG, "null context");
    if (fill_ms) *fill_ms = c->fill_ms;
    if (walk_ms) *walk_ms = c->walk_ms;
    return GA_OK;
}

// Diagnostics (not in the public header): the walk's tile-need records (ti, tj, D, wait ticks) x 8192.
int ga_debug_walk_tiles(ga_ctx* c, unsigned* out) {
    if (!c || !out) return fail(GA_E_ARG, "null argument");
    if (!c->wdbg.p) return fail(GA_E_STATE, "no diagnostic walk ran");
    HIPCHK(hipMemcpy(out, c->wdbg.p, sizeof(unsigned) * 4 * 8192, hipMemcpyDeviceToHost));
    return GA_OK;
}

// Diagnostics (not in the public header): per-stripe s_memrealtime stamps of the next fills.
int ga_debug_stamps(ga_ctx* c, int enable, unsigned long long* out, int64_t cap) {
    if (!c) return fail(GA_E_ARG, "null context");
    c->dbg_on = enable != 0;
    if (out && c->dbg.p) {
        const int64_t nb = std::min<int64_t>(cap, ga::LK_DBG_WORDS * (int64_t)c->plan.nstripes);
        HIPCHK(hipMemcpy(out, c->dbg.p, sizeof(unsigned long long) * nb, hipMemcpyDeviceToHost));
    }
    return GA_OK;
}

// Diagnostics: the fill geometry of the loaded problem {T, nstripes, nwc, nslabs}.
int ga_debug_geometry(ga_ctx* c, int32_t* out4) {
    if (!c || !out4) return fail(GA_E_ARG, "null argument");
    out4[0] = c->plan.T;
    out4[1] = c->plan.nstripes;
    out4[2] = c->plan.nwc;
    out4[3] = c->plan.nslabs;
    return GA_OK;
}

// Diagnostics: the kernel of the last enqueued fill (0 row scan, 1 per-column anti-diagonal, 2 lane-skewed)
// and its geometry {T, nstripes, nwc, nslabs}.
int ga_debug_fill_kind(ga_ctx* c, int32_t* out5) {
    if (!c || !out5) return fail(GA_E_ARG, "null argument");
    out5[0] = c->rc_used ? 3 : c->plan.kind == gaplan::kLane ? 2 : c->plan.kind == gaplan::kDiag ? 1 : 0;  // 3: the recompute walk's lane fill
    out5[1] = c->plan.T;
    out5[2] = c->plan.nstripes;
    out5[3] = c->plan.nwc;
    out5[4] = c->plan.nslabs;
    return GA_OK;
}

// CPU-only check of the tie-break table (tests): entries for `steps` dispatches from
// the 625-word state, and the state after the first D of them.
int ga_debug_rng(const uint32_t* state, int64_t steps, uint32_t* tab_out, int64_t D, uint32_t* state_out,
                 double* ms_out) {
    if (!state || !tab_out || !state_out || D < 0 || D > steps) return fail(GA_E_ARG, "bad argument");
    RngTable R;
    const double t0 = now_ms();
    build_rng(state, steps, R);
    if (ms_out) *ms_out = now_ms() - t0;
    std::memcpy(tab_out, R.tab.data(), sizeof(uint32_t) * steps);
    state_after(R, D, state_out);
    return GA_OK;
}

// CPU-only check of the resumable table stream (tests): entries for `steps` dispatches built in
// `chunk`-sized extensions, and the state after the first D of them.
int ga_debug_rng_chunked(const uint32_t* state, int64_t steps, int64_t chunk, uint32_t* tab_out, int64_t D,
                         uint32_t* state_out) {
    if (!state || !tab_out || !state_out || D < 0 || D > steps || chunk < 1) return fail(GA_E_ARG, "bad argument");
    RngTable R;
    R.start(state);
    for (int64_t b = chunk; b < steps + chunk; b += chunk) R.extend(std::min(b, steps));
    std::memcpy(tab_out, R.tab.data(), sizeof(uint32_t) * steps);
    state_after(R, D, state_out);
    return GA_OK;
}

// out6 = {tile wait spins, tiles entered, tile-wait ticks, ring-wait ticks, walker ticks (100 MHz),
//         walker shader clocks / 16, loader busy ticks, tiles loaded}
// Diagnostics of the last recompute walk: {blocks recomputed, their summed time in 100 MHz ticks,
// recompute workers, checkpoint spacing}.
int ga_debug_rc(ga_ctx* c, unsigned* out4) {
    if (!c || !out4) return fail(GA_E_ARG, "null argument");
    if (!c->rc_pos.p) return fail(GA_E_STATE, "no recompute walk ran");
    HIPCHK(hipMemcpy(out4, c->rc_pos.p, sizeof(unsigned) * 4, hipMemcpyDeviceToHost));
    return GA_OK;
}

// How the library was built: bit 0 set in an experiments build (make EXPERIMENTS=1: the measured-and-dropped paths,
// e.g. the tie-to-tie walk, and every GA_* variable read from the environment).
int ga_build_flags(int32_t* flags) {
    if (!flags) return fail(GA_E_ARG, "null argument");
#ifdef GA_EXPERIMENTS
    flags[0] = 1;
#else
    flags[0] = 0;
#endif
    return GA_OK;
}

// diagnostics / CPU tests: the jump workers' LUT for gap open o (4096 words)
int ga_debug_jump_lut(int32_t o, uint32_t* out4096) {
    if (!out4096 || o < 0 || o > 14) return fail(GA_E_ARG, "bad argument");
    ga::jump_lut_build(o, out4096);
    return GA_OK;
}

// diagnostics: the recompute walk's tile / entry cache (rc_tb) as the last walk left it
int ga_debug_rc_cache(ga_ctx* c, void* out, int64_t bytes) {
    if (!c || !out) return fail(GA_E_ARG, "null argument");
    if (!c->rc_tb.p) return fail(GA_E_STATE, "no recompute walk ran");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, c->rc_tb.p, std::min<size_t>((size_t)bytes, c->rc_tb.cap), hipMemcpyDeviceToHost));
    return GA_OK;
}

// which walk the last traceback ran: 0 the walk of stored words, 1 the recompute walk of traceback words, 2 the
// tie-to-tie recompute walk (jump entries)
int ga_debug_walk_kind(ga_ctx* c, int32_t* out) {
    if (!c || !out) return fail(GA_E_ARG, "null argument");
    out[0] = c->rc_used ? (c->rc_jump ? 2 : 1) : 0;
    return GA_OK;
}

int ga_debug_walk_jump(ga_ctx* c, int* out3) {
    if (!c || !out3) return fail(GA_E_ARG, "null argument");
    for (int q = 0; q < 3; q++) out3[q] = c->walk_jump_diag[q];
    return GA_OK;
}

int ga_debug_walk(ga_ctx* c, int* out5) {
    if (!c || !out5) return fail(GA_E_ARG, "null argument");
    out5[0] = c->walk_waits;
    out5[1] = c->walk_tiles;
    out5[2] = c->walk_t_tile;
    out5[3] = c->walk_t_ring;
    out5[4] = c->walk_t_total;
    out5[5] = c->walk_c_total;
    out5[6] = c->walk_load_ticks;
    out5[7] = c->walk_load_count;
    return GA_OK;
}

int ga_last_timings(ga_ctx* c, float* out4) {
    if (!c || !out4) return fail(GA_E_ARG, "null argument");
    out4[0] = c->fill_ms;
    out4[1] = c->walk_ms;
    out4[2] = c->rng_ms;
    out4[3] = c->call_ms;
    return GA_OK;
}

// ---- guard mode ----
// the entries that run kernels and wait for them end with the guards' check (guard mode off: one branch)
int ga_problem_set(ga_ctx* c, const uint8_t* a, int64_t m, const uint8_t* b, int64_t n, const ga_costs* cs,
                   const int32_t* row0, const int32_t* col0) {
    return guard_end(c, problem_set_impl(c, a, m, b, n, cs, row0, col0));
}

int ga_problem_fill(ga_ctx* c, int32_t flags, int64_t* cost_out, int32_t* full_out) {
    return guard_end(c, problem_fill_impl(c, flags, cost_out, full_out));
}

int ga_problem_set_cells(ga_ctx* c, const int32_t* cells, int64_t* cost_out) {
    return guard_end(c, problem_set_cells_impl(c, cells, cost_out));
}

int ga_problem_traceback(ga_ctx* c, uint32_t* mt_state, const char* a_chr, const char* b_chr, char* oa, char* om,
                         char* ob, int64_t cap, int64_t* out_len, int32_t* tb_status) {
    return guard_end(c, problem_traceback_impl(c, mt_state, a_chr, b_chr, oa, om, ob, cap, out_len, tb_status));
}

int ga_problem_align(ga_ctx* c, uint32_t* mt_state, const char* a_chr, const char* b_chr, char* oa, char* om,
                     char* ob, int64_t cap, int64_t* out_len, int32_t* tb_status, int64_t* cost_out) {
    return guard_end(c, problem_align_impl(c, mt_state, a_chr, b_chr, oa, om, ob, cap, out_len, tb_status, cost_out));
}

int ga_problem_align_many(ga_ctx* c, int32_t count, uint32_t* mt_state, const char* a_chr, const char* b_chr,
                          char* oa, char* om, char* ob, int64_t cap, int64_t* out_len, int32_t* tb_status,
                          int64_t* cost_out) {
    return guard_end(c, problem_align_many(c, count, mt_state, a_chr, b_chr, oa, om, ob, cap, out_len, tb_status,
                                                cost_out));
}

int ga_problem_set_slab(ga_ctx* c, const uint8_t* a, int64_t m, const uint8_t* b, int64_t n, const ga_costs* cs,
                        int64_t col_begin, int64_t col_end) {
    return guard_end(c, problem_set_slab_impl(c, a, m, b, n, cs, col_begin, col_end));
}

int ga_slab_fill_finish(ga_ctx* c, int64_t* cost_out) {
    return guard_end(c, slab_fill_finish_impl(c, cost_out));
}

int ga_slab_walk(ga_ctx* c, ga_walk_state* st, const char* a_chr, const char* b_chr, char* oa, char* om, char* ob,
                 int64_t cap, int64_t* out_len) {
    return guard_end(c, slab_walk_impl(c, st, a_chr, b_chr, oa, om, ob, cap, out_len));
}

int ga_debug_guard_report(ga_ctx* c, char* out, int64_t cap, int64_t* needed) {
    if (int r = check_ctx(c)) return r;
    if (!needed || (cap > 0 && !out) || cap < 0) return fail(GA_E_ARG, "null argument");
    if (!c->guard.G) return fail(GA_E_STATE, "guard mode is off (option GA_GUARD_BYTES)");
    std::vector<gaguard::Violation> vs;
    if (int r = guard_collect(c, false, vs)) return r;
    std::string js = "{\"guard_bytes\": " + std::to_string(c->guard.G) + ", \"fill\": " + std::to_string((int)c->guard.fill) +
                     ", \"poison\": " + (c->guard.poison ? "true" : "false") + ", \"violations\": [";
    for (size_t k = 0; k < vs.size(); k++)
        js += std::string(k ? ", " : "") + "{\"name\": \"" + vs[k].name + "\", \"side\": \"" +
              (vs[k].side == gaguard::kFront ? "front" : "rear") + "\", \"offset\": " + std::to_string(vs[k].offset) +
              ", \"last\": " + std::to_string(vs[k].last) + ", \"changed\": " + std::to_string(vs[k].changed) +
              ", \"payload\": " + std::to_string(vs[k].payload) + "}";
    js += "], \"buffers\": [";
    bool first = true;
    auto item = [&](const std::string& name, size_t payload, bool guarded) {
        js += std::string(first ? "" : ", ") + "{\"name\": \"" + name + "\", \"payload\": " + std::to_string(payload) +
              ", \"guarded\": " + (guarded ? "true" : "false") + "}";
        first = false;
    };
    for (const DevBuf* b : c->guard.dev)
        if (b->p) item(b->name, b->size, true);
    for (const PinBuf* b : c->guard.pin)
        if (b->p) item(b->name, b->size, true);
    if (c->link.p) item("link", c->link.cap, false);  // exported by IPC handle: outside guard mode (guard_each)
    js += "]}";
    *needed = (int64_t)js.size() + 1;
    if (cap >= *needed) std::memcpy(out, js.c_str(), js.size() + 1);
    return GA_OK;
}

int ga_debug_guard_poke(ga_ctx* c, const char* name, int32_t side, int64_t offset, int64_t nbytes) {
    if (int r = check_ctx(c)) return r;
    if (!name) return fail(GA_E_ARG, "null argument");
    const GuardCfg& g = c->guard;
    if (!g.G) return fail(GA_E_STATE, "guard mode is off (option GA_GUARD_BYTES)");
    // inside one guard of an allocation of ours, whatever the caller asks
    if ((side != gaguard::kFront && side != gaguard::kRear) || offset < 0 || nbytes < 1 || offset >= (int64_t)g.G ||
        nbytes > (int64_t)g.G - offset)
        return fail(GA_E_ARG, "ga_debug_guard_poke: side 0 or 1, and [offset, offset + nbytes) inside [0, GA_GUARD_BYTES)");
    const std::vector<uint8_t> other((size_t)nbytes, (uint8_t)~g.fill);
    for (DevBuf* b : g.dev)
        if (b->p && b->name == name) {
            HIPCHK(hipDeviceSynchronize());
            uint8_t* at = b->as<uint8_t>() + (side == gaguard::kFront ? -(ptrdiff_t)g.G : (ptrdiff_t)b->size) + offset;
            HIPCHK(hipMemcpy(at, other.data(), (size_t)nbytes, hipMemcpyHostToDevice));
            return GA_OK;
        }
    for (PinBuf* b : g.pin)
        if (b->p && b->name == name) {
            std::memcpy(b->host<uint8_t>() + (side == gaguard::kFront ? -(ptrdiff_t)g.G : (ptrdiff_t)b->size) + offset,
                        other.data(), (size_t)nbytes);
            return GA_OK;
        }
    return fail(GA_E_ARG, std::string("ga_debug_guard_poke: no allocated guarded buffer named '") + name + "'");
}

}  // extern "C"


namespace ga {
// The rank sets of a cell from its saturated differences (as ga_walk.h sets_from_code): per level the v_perm
// selector of the candidate its singleton move takes (bytes 4,5 of {src0, Pu} = Pd (diag), 6,7 = Pl (left), 0,1 = Pu
// (up)) or 0x0c0c (a zero half) for a tie, and the tie word ((2S - 2 + 14*(a != b)) << 2) the walker reads at a tie
void jump_lut_build(int o, uint32_t* out) {
    const unsigned uo = (unsigned)o;
    for (unsigned idx = 0; idx < 1024; idx++) {
        const unsigned fx = idx & 15u, fy = (idx >> 4) & 15u, zM = ((idx >> 8) & 1u) ^ 1u, mm = (idx >> 9) & 1u;
        const unsigned zX = fx == 0, zY = fy == 0, leX = fx <= uo, geX = fx >= uo, leY = fy <= uo, geY = fy >= uo;
        const unsigned S[3] = {zM | (zX << 1) | (zY << 2), (zM & geX) | (leX << 1) | ((zY & geX) << 2),
                               (zM & geY) | ((zX & geY) << 1) | (leY << 2)};
        unsigned sel[3], tw[3];
        for (int L = 0; L < 3; L++) {
            const unsigned x = S[L];
            sel[L] = x == 1u ? 0x0504u : x == 2u ? 0x0706u : x == 4u ? 0x0100u : 0x0c0cu;
            tw[L] = (x == 1u || x == 2u || x == 4u) ? 0u : x ? ((2u * x - 2u + 14u * mm) << 2) : 0x7cu;  // (empty: never walked)
        }
        out[4 * idx] = sel[0] | (sel[1] << 16);
        out[4 * idx + 1] = sel[2] | (0x0c0cu << 16);
        out[4 * idx + 2] = tw[0] | (tw[1] << 16);
        out[4 * idx + 3] = tw[2];
    }
}
}  // namespace ga
