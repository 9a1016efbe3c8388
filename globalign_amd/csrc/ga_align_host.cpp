// ga_align_host.cpp -- the HIP side of one alignment's traceback (ga_problem_align, ga_problem_traceback; DESIGN.md
// 5.4, 5.5, 5.8): the walk launches and the decode of their levels into strings (ga_strings.h: take_* :688-753, the
// i==0 / j==0 tails :542-581 and the final reverse :584-586), banded traceback, the recompute walk, and the call that
// chooses among them.  The choices, the knobs and the recompute walk's window are ga_walk_plan.h's; here are the HIP
// calls, in the order the measured timings depend on.  Slabs (ga_host.cpp) and the pipeline (ga_pipe_host.cpp) launch
// their walks through the same functions (ga_host_internal.h).
#include <cstring>
#include <thread>

#include "ga_host_internal.h"
#include "ga_strings.h"

using namespace gahost;
using namespace garng;

namespace gahost {

static_assert(gawalk::kSpanI == ga::RC_SPAN_I && gawalk::kSpanS == ga::RC_SPAN_S, "the window's spans (ga_walk_plan.h)");
static_assert(sizeof(ga::RcArgs::off) == sizeof(gawalk::Window::off), "the window's candidates (ga_walk_plan.h)");

WalkBufs ctx_walk_bufs(ga_ctx* c) {
    return WalkBufs{c->fb.tb.as<uint8_t>(), c->rng.as<uint32_t>(), c->ops.as<uint32_t>(), c->result.as<int>(), c->stream,
                    c->wev[0], c->wev[1]};
}

ga::WalkArgs walk_args(ga_ctx* c, int64_t ntab, const WalkStart& st, int64_t r0, int64_t mb, bool vhandoff,
                       const WalkBufs& wb) {
    ga::WalkArgs w{};
    w.tb = wb.tb;
    w.CB = c->CB;
    w.TC = c->plan.TC;
    w.a = c->a.as<uint8_t>() + r0;
    w.b = c->b.as<uint8_t>() + c->col0;
    w.bnd_row = (wb.bnd_row ? wb.bnd_row : c->fb.bnd_row.as<int>()) + 3 * c->col0;
    w.bnd_col = (wb.bnd_col ? wb.bnd_col : c->fb.bnd_col.as<int>()) + 3 * r0;
    w.rng = wb.rng;
    w.nrng = (long long)ntab;
    w.m = (int)(mb >= 0 ? mb : c->m);
    w.n = (int)c->n;
    w.o = c->o;
    w.i0 = (int)(st.i - r0);
    w.vhandoff = vhandoff ? 1 : 0;
    w.j0 = (int)(st.j - c->col0);
    w.L0 = st.L;
    w.first0 = st.first;
    w.D0 = (int)st.D;
    w.h0 = (int)st.h;
    w.handoff = c->col0 > 0;
    w.maxh = (int)(c->m + c->n_global);
    // the loaders leave the 4x4 tile block's far off-diagonal corners: 28 % fewer
    // speculative tile loads, C3 walk 6.87 -> 6.71 ms alone and 7.74 -> 7.4 ms in the pipeline, C5
    // 1.45 -> 1.27 ms (tools/exp/walk_skip.sh); GA_WALK_SKIP_CORNERS = 0 / 2 / 3 for none / more
    w.skip_corners = c->wk.walk_skip_corners;
    // 14 loader waves (the L2 prefetcher's and the idle wave's too): tile waits at C3 469 -> 186 us
    // alone, 921 -> 413 us in the pipeline, walk 6.81 -> 6.52 ms alone, C5 1.28 -> 1.15 ms
    // (tools/exp/walk_loaders.sh); GA_WALK_LOADERS = 12 / 13 for the former roles
    w.nloaders = c->wk.walk_loaders;
    w.ops = wb.ops;
    w.ops_prog = wb.ops_prog;
    w.result = wb.result;
    w.dbg = nullptr;
    return w;
}

int run_walk(ga_ctx* c, const uint32_t* tab, int64_t ntab, const WalkStart& st, int64_t r0, int64_t mb, bool vhandoff,
             bool upload_tab, const WalkBufs* wbp) {
    const WalkBufs wb = wbp ? *wbp : ctx_walk_bufs(c);
    if (upload_tab) HIPCHK(hipMemcpyAsync(wb.rng, tab, sizeof(uint32_t) * ntab, hipMemcpyHostToDevice, wb.stream));
    ga::WalkArgs w = walk_args(c, ntab, st, r0, mb, vhandoff, wb);
    if (c->dbg_on) {
        HIPCHK(c->wdbg.ensure(sizeof(unsigned) * 4 * 8192));
        HIPCHK(hipMemsetAsync(c->wdbg.p, 0xff, sizeof(unsigned) * 4 * 8192, wb.stream));
    }
    w.dbg = c->dbg_on ? c->wdbg.as<unsigned>() : nullptr;
    HIPCHK(hipEventRecord(wb.ev0, wb.stream));
    ga::launch_walk(wb.stream, w);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(wb.ev1, wb.stream));
    return GA_OK;
}

// The walk's result words [4, 15) into the context's diagnostic fields (ga_debug_walk, ga_debug_walk_jump).
void take_walk_diag(ga_ctx* c, const int* res) {
    c->walk_waits = res[4];
    c->walk_tiles = res[5];
    c->walk_t_tile = res[6];
    c->walk_t_ring = res[7];
    c->walk_t_total = res[8];
    c->walk_c_total = res[9];
    c->walk_load_ticks = res[10];
    c->walk_load_count = res[11];
    for (int q = 0; q < 3; q++) c->walk_jump_diag[q] = res[12 + q];
}

// The walk state after the dispatches up to D1, whose columns `col` holds (ga_strings.h).
void advance_walk(WalkStart& st, const gastr::Columns& col, int64_t D1) {
    if (D1 > st.D) {
        st.h += (D1 - st.D) - (st.first ? 1 : 0);
        st.first = 0;
    }
    st.i = col.i;
    st.j = col.j;
    st.L = col.L;
    st.D = D1;
}

int walk_segment(ga_ctx* c, WalkStart& st, int& reason, const char* a_chr, const char* b_chr, char* oa, char* om,
                 char* ob, int64_t cap, int64_t& len, const WalkBufs* wbp) {
    const WalkBufs wb = wbp ? *wbp : ctx_walk_bufs(c);
    int res[16];
    HIPCHK(hipMemcpyAsync(res, wb.result, sizeof(int) * 16, hipMemcpyDeviceToHost, wb.stream));
    HIPCHK(hipStreamSynchronize(wb.stream));
    return decode_segment(c, res, st, reason, a_chr, b_chr, oa, om, ob, cap, len, wb, false);
}

// The alignment columns of a finished walk (its result words already read): levels of dispatches
// [st.D, res[0]) decoded in walk order starting at (st.i, st.j).  synced: the walk is known to be
// complete, so its levels are read with a plain copy instead of on its stream (which may already
// hold the next walk).
int decode_segment(ga_ctx* c, const int* res, WalkStart& st, int& reason, const char* a_chr, const char* b_chr,
                   char* oa, char* om, char* ob, int64_t cap, int64_t& len, const WalkBufs& wb, bool synced,
                   const uint32_t* host_ops) {
    take_walk_diag(c, res);
    if (!synced) HIPCHK(hipEventElapsedTime(&c->walk_ms, wb.ev0, wb.ev1));
    const int64_t D0 = st.D, D1 = res[0];
    reason = res[3];
    // the level words that hold dispatches [D0, D1): 16 dispatches to a u32
    const int64_t w0 = D0 >> 4, w1 = (D1 + 15) >> 4;
    std::vector<uint32_t> ops((size_t)std::max<int64_t>(w1 - w0, 0));
    if (host_ops) {  // the levels in pinned host memory (the walk chain writes them there)
        if (D1 > D0) std::memcpy(ops.data(), host_ops + w0, ops.size() * sizeof(uint32_t));
    } else if (synced) {
        if (D1 > D0) HIPCHK(hipMemcpy(ops.data(), wb.ops + w0, ops.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    } else {
        if (D1 > D0)
            HIPCHK(hipMemcpyAsync(ops.data(), wb.ops + w0, ops.size() * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                  wb.stream));
        HIPCHK(hipStreamSynchronize(wb.stream));
    }
    gastr::Columns col{a_chr, c->m, b_chr, c->n_global, oa, om, ob, cap, st.i, st.j, st.L};
    if (reason != 4) col.decode<false>(ops.data(), w0, D0, D1);  // (4: the reference's IndexError, no columns)
    advance_walk(st, col, D1);
    len = col.len;
    if (len > cap) return fail(GA_E_ARG, "output capacity too small");
    return GA_OK;
}

// Whole-problem traceback: one walk from (m, n), tails, reversal (dp_array_backward's output).
int finish_walk(ga_ctx* c, const RngTable& snaps, uint32_t* mt_state, const char* a_chr, const char* b_chr,
                char* oa, char* om, char* ob, int64_t cap, int64_t* out_len, int32_t* tb_status) {
    WalkStart st = walk_origin(c);
    int reason = 0;
    int64_t len = 0;
    if (int r = walk_segment(c, st, reason, a_chr, b_chr, oa, om, ob, cap, len)) return r;
    return conclude_walk(snaps, st, reason, mt_state, a_chr, b_chr, oa, om, ob, cap, len, out_len, tb_status);
}

int conclude_walk(const RngTable& snaps, const WalkStart& st, int reason, uint32_t* mt_state, const char* a_chr,
                  const char* b_chr, char* oa, char* om, char* ob, int64_t cap, int64_t len, int64_t* out_len,
                  int32_t* tb_status) {
    if (mt_state) state_after(snaps, st.D, mt_state);
    if (reason == 4) {  // IndexError in the reference
        *tb_status = GA_TB_INDEX_ERROR;
        *out_len = 0;
        return GA_OK;
    }
    len = gastr::finish_strings(reason, st.i, st.j, a_chr, b_chr, oa, om, ob, cap, len);
    if (len > cap) return fail(GA_E_ARG, "output capacity too small");
    *out_len = len;
    *tb_status = GA_TB_OK;
    return GA_OK;
}

// ---------------------------------------------------------------- banded traceback
// Traceback words take m*n*CB bytes.  Past a budget (GA_TB_BUDGET_MB, default 64 GB of the 288 GB),
// the traceback runs in bands of Bh rows: one score-only fill that also saves the
// (H', h2') row every Bh rows, then, from the bottom band up, a fill of the band's rows with
// traceback words (its top row from the checkpoint) and the walk through it, handed on at the
// band's top row (walk reason 6).  Fill work doubles; memory is one band of words.
int64_t band_rows(ga_ctx* c) {
    // (forced rows, tests, do not ask the device what it has free)
    const int64_t avail = c->wk.tb_band_rows ? 0 : dev_avail_bytes(c, (int64_t)c->fb.tb.cap);
    return gawalk::band_rows(c->m, c->n, c->CB, c->wk, avail);
}

int check_fill_abort(ga_ctx* c) {
    unsigned abort_word = 0;
    HIPCHK(hipMemcpy(&abort_word, c->fb.flags.as<unsigned>() + 1, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (abort_word) return fail(GA_E_TIMEOUT, "fill kernel hand-off wait timed out");
    return GA_OK;
}

int banded_align(ga_ctx* c, int64_t Bh, uint32_t* mt_state, const char* a_chr, const char* b_chr, char* oa, char* om,
                 char* ob, int64_t cap, int64_t* out_len, int32_t* tb_status, int64_t* cost_out) {
    const double t0 = now_ms();
    const int64_t m = c->m, n = c->n;
    // bands [b*Bh, b*Bh + Bh) of rows, the last one absorbing a remainder of < 16 rows
    int64_t nb = (m + Bh - 1) / Bh;
    if (nb > 1 && m - (nb - 1) * Bh < ga::FROWS) nb--;
    const int64_t nck = (m - 1) / Bh;  // checkpoint rows the fill writes (every multiple of Bh below m)
    HIPCHK(c->ckpt.ensure(sizeof(int2) * (size_t)std::max<int64_t>(nck, 1) * (n + 1)));
    int2* ck = c->ckpt.as<int2>();
    Band pass1;
    pass1.ckpt = ck;
    pass1.ckpt_rows = (int)Bh;
    if (int r = enqueue_fill(c, 0, pass1)) return r;
    RngTable R;
    const double t1 = now_ms();
    build_rng(mt_state, m + n + 1, R);
    c->rng_ms = (float)(now_ms() - t1);
    if (int r = finish_fill(c, cost_out, nullptr)) return r;
    WalkStart st = walk_origin(c);
    int reason = 6;
    int64_t len = 0;
    float walk_ms = 0.f, fill_ms = c->fill_ms;
    for (int64_t b = nb - 1; b >= 0 && reason == 6; b--) {
        Band bd;
        bd.band = true;
        bd.r0 = b * Bh;
        bd.mb = b == nb - 1 ? m - bd.r0 : Bh;
        // the path only moves up and left: this band's cells right of the column where the walk
        // enters it are never read, so the band fills columns 1..j only (on a diagonal-ish path
        // about half the refill work of full-width bands)
        bd.nc = st.j;
        if (b > 0) {
            int2* row = ck + (size_t)(b - 1) * (n + 1);
            // column 0 of the checkpoint row: the left edge's corner H'(r0, 0)
            HIPCHK(hipMemcpyAsync(row, c->fb.left.as<int2>() + bd.r0, sizeof(int2), hipMemcpyDeviceToDevice, c->stream));
            bd.top = row;
        }
        if (int r = enqueue_fill(c, GA_FILL_TRACEBACK, bd)) return r;
        if (int r = run_walk(c, R.tab.data(), (int64_t)R.tab.size(), st, bd.r0, bd.mb, b > 0, b == nb - 1)) return r;
        int64_t seg = 0;
        if (int r = walk_segment(c, st, reason, a_chr, b_chr, oa + len, om + len, ob + len, cap - len, seg)) return r;
        if (int r = check_fill_abort(c)) return r;
        // the walk tests local row 0 first: a move that lands on a band's top row AND on local column 0 comes back
        // as a hand-over (6), but the walk has reached the left edge -- what it reports anywhere else in a band
        // (jend).  Handing it on would start the next band's walk at column 0, on the degenerate path.  (Only the
        // whole-problem call bands its traceback, col0 == 0: column 0 is the matrix edge, reason 2.)
        if (reason == 6 && st.j == 0) reason = 2;
        len += seg;
        walk_ms += c->walk_ms;
        float f = 0.f;
        if (hipEventElapsedTime(&f, c->fb.ev[0], c->fb.ev[1]) == hipSuccess) fill_ms += f;
    }
    c->walk_ms = walk_ms;
    c->fill_ms = fill_ms;
    const int rc = conclude_walk(R, st, reason, mt_state, a_chr, b_chr, oa, om, ob, cap, len, out_len, tb_status);
    c->call_ms = (float)(now_ms() - t0);
    return rc;
}

// ---------------------------------------------------------------- the recompute walk
// One find_global_alignment without stored traceback words: a score-only lane fill that leaves
// checkpoints, then one launch in which a workgroup walks while recompute workgroups write the
// traceback words of the 64-row blocks ahead of it into a small tile cache.  The fill runs at score-only
// speed and memory is O(checkpoints), not m*n words.  Which problems take it: gawalk::rc_eligible.

// The score-only checkpointing fill of the loaded problem or slab.  The checkpoint spacing (steps, a
// power of two >= 64: 64 keeps a block's recompute at <= 127 + 63 steps) trades recompute steps for checkpoint memory,
// (TD + 1) * 512 B per stripe per spacing: chosen with the geometry by the fill's plan (ga_plan.h) unless GA_RC_EVERY
// (a power of two in [64, 2^20], checked in ga_ctx_create_opts) fixes it.
int rc_fill(ga_ctx* c) {
    Band bd;
    bd.rc = true;
    bd.rc_every = c->wk.rc_every;
    if (int r = enqueue_fill(c, 0, bd, &c->rc_plan)) return r;
    c->rc_used = true;
    return GA_OK;
}

// The tie-to-tie walk (experiments build only: it measured slower than the word walk, 7.15-7.72
// against 5.2 ms at C3) when GA_RC_JUMP asks for it and its workers fit: at most 4 columns per lane (a worker stages
// its block's 3 x 64 x 64*TD entries in LDS) and o <= 14 (X'-H', Y'-H' saturated at o+1 index a 1024-entry LUT).
bool rc_jump_wanted(ga_ctx* c, int TD) {
#ifdef GA_EXPERIMENTS
    return c->pk.rc_jump && TD <= 4 && c->o <= 14 &&
           ga::rc_jump_lds_bytes(TD, c->rc_plan.rc_every) + 12 * 1024 <= 160 * 1024;
#else
    (void)c;
    (void)TD;
    return false;
#endif
}

// What a recompute walk of nbi x nbs blocks finds ready: the block cache, the blocks' flags and the cache slots' owner
// tags under a fresh epoch, the position words cleared, (experiments build) the jump workers' LUT.
static int rc_walk_upkeep(ga_ctx* c, hipStream_t stream, int TD, int nbi, int nbs) {
    HIPCHK(c->rc_tb.ensure(rc_cache_bytes(c->rc_jump, TD, c->CB)));
    const size_t nflags = (size_t)nbi * nbs;
    // the cache slots' owner tags (ga::rc_slot_tag) carry the epoch's ready value: cleared with the flags
    const size_t nown = (size_t)ga::RC_CACHE_I * ga::RC_CACHE_S * sizeof(unsigned long long);
    if (c->rc_flags.cap < nflags * sizeof(unsigned) || c->rc_own.cap < nown || c->rc_epoch >= 0x7ffffff0u) {
        // the flags are cleared here and then reused, by any later problem that fits, at the buffer's whole capacity:
        // the request names all of it
        HIPCHK(c->rc_flags.ensure(std::max<size_t>({nflags * sizeof(unsigned), c->rc_flags.cap, 256})));
        HIPCHK(hipMemsetAsync(c->rc_flags.p, 0, c->rc_flags.cap, stream));
        HIPCHK(c->rc_own.ensure(nown));
        HIPCHK(hipMemsetAsync(c->rc_own.p, 0, nown, stream));
        c->rc_epoch = 0;
    }
    c->rc_epoch++;
    HIPCHK(c->rc_pos.ensure(16));
    if (!c->rc_pos_zeroed) HIPCHK(hipMemsetAsync(c->rc_pos.p, 0, 16, stream));
    c->rc_pos_zeroed = false;
    // rc_windows reads the edge rows t0 + RC_EDGE_FIRST and up with t0 = (R0 / stck_every) * stck_every >= 0: never
    // row 0 of a colck stripe, which the fill's lean ramp leaves with a ramp value (ga_lane.hip).  A spacing that is
    // not positive would make t0 meaningless.
    static_assert(ga::RC_EDGE_FIRST >= 1, "the recompute blocks must not read colck row 0 (lean ramp, ga_lane.hip)");
    const int every = c->rc_plan.rc_every;
    if (every < 64 || (every & (every - 1)))
        return fail(GA_E_STATE, "recompute walk: checkpoint spacing " + std::to_string(every) +
                                    " is not a power of two >= 64 (the edge window's rows >= t0 + 1 rest on it)");
    if (c->rc_jump && c->jlut_o != c->o) {
        std::vector<uint32_t> lut(4096);
        ga::jump_lut_build(c->o, lut.data());
        HIPCHK(c->jlut.ensure(sizeof(uint32_t) * lut.size()));
        HIPCHK(hipMemcpy(c->jlut.p, lut.data(), sizeof(uint32_t) * lut.size(), hipMemcpyHostToDevice));
        c->jlut_o = c->o;
    }
    return GA_OK;
}

// Launch the walk + recompute workgroups from walk state `st` on the walk buffers `wb` (its table already uploaded),
// after rc_fill: the buffers' upkeep, the launch figures (ga_walk_plan.h), the two kernels' arguments.
int rc_walk_launch(ga_ctx* c, int64_t ntab, const WalkStart& st, WalkBufs& wb) {
    const int TD = c->rc_plan.T, CB = c->CB;
    const int nbi = (int)((c->m + 63) / 64), nbs = c->rc_plan.nstripes;
    c->rc_jump = rc_jump_wanted(c, TD);
    if (int rr = rc_walk_upkeep(c, wb.stream, TD, nbi, nbs)) return rr;
    const gawalk::Window win = gawalk::window(TD, c->wk);
    wb.tb = c->rc_tb.as<uint8_t>();
    ga::WalkArgs w = walk_args(c, ntab, st, 0, -1, false, wb);
    w.TC = ga::RC_CACHE_I * 4 * CB;  // 16-byte words per lane per 64-column stripe of the cache
    // 14 loaders, no L2 prefetcher (it would read blocks not yet recomputed); GA_RC_LOADERS = 12 / 13 leave
    // waves 8 and 12 / wave 8 (the walker's SIMD) idle instead
    w.nloaders = c->wk.rc_loaders;
    w.rc_flags = c->rc_flags.as<unsigned>();
    w.rc_ready = 2u * c->rc_epoch + 1u;
    w.rc_own = c->rc_own.as<unsigned long long>();
    w.rc_nbs = nbs;
    w.rc_td = TD;
    w.rc_pos = c->rc_pos.as<unsigned>();
    ga::RcArgs r{};
    r.a = c->a.as<uint8_t>();
    r.b = c->b.as<uint8_t>() + c->col0;
    r.subp = c->qp.as<int>();
    r.K = c->K;
    r.top = c->fb.top.as<int2>() + c->col0;
    // the slab's left edge (another GPU's right edge, landed in full by now) or column 0
    r.left = c->slab && c->col0 > 0 ? (c->halo_in_ext ? c->halo_in_ext : c->halo_in.as<int2>()) : c->fb.left.as<int2>();
    r.colck = c->colck.as<int2>();
    r.stck = c->stck.as<int2>();
    r.stck_every = c->rc_plan.rc_every;
    r.tb = c->rc_tb.as<uint8_t>();
    r.TC = w.TC;
    r.m = (int)c->m;
    r.n = (int)c->n;
    r.o = c->o;
    r.TD = TD;
    r.nstripes = r.nbs = nbs;
    r.nbi = nbi;
    r.flags = c->rc_flags.as<unsigned>();
    r.epoch = c->rc_epoch;
    r.own = w.rc_own;
    r.tag_fault = c->wk.rc_tag_fault;
    r.pos = c->rc_pos.as<unsigned>();
    r.tile0 = (int)((((st.i - 1) / 64) << 16) | ((st.j - c->col0 - 1) / 64));  // the walk's first tile
#ifdef GA_EXPERIMENTS
    r.worker_bytes = c->rc_jump ? ga::rc_jump_worker_bytes_host(TD, r.stck_every) : ga::rc_worker_bytes(TD, CB, r.stck_every);
#else
    r.worker_bytes = ga::rc_worker_bytes(TD, CB, r.stck_every);
#endif
    r.workers = gawalk::workers(c->rc_jump, r.worker_bytes, c->wk);
    r.spin_limit = 1u << 20;
    r.jlut = c->rc_jump ? c->jlut.as<uint4>() : nullptr;
    std::memcpy(r.off, win.off, sizeof(r.off));
    r.nwin = win.nwin;
    const int nserv = gawalk::servers(c->wk);
    HIPCHK(hipEventRecord(wb.ev0, wb.stream));
#ifdef GA_EXPERIMENTS
    if (c->rc_jump) ga::launch_walk_rc_jump(wb.stream, w, r, nserv);
    else
#endif
        ga::launch_walk_rc(wb.stream, w, r, nserv);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(wb.ev1, wb.stream));
    return GA_OK;
}

// One alignment's walk writing its levels to pinned host memory with a progress word (WalkArgs::ops_prog),
// so that the calling thread decodes them while the walk runs (rc_align, and the stored-words call)
int pinned_walk_levels(ga_ctx* c, WalkBufs& wb) {
    const int64_t m = c->m, n = c->n;
    const int64_t nwords = (m + n + 1 + 15) / 16 + 64;
    HIPCHK(c->rc_ops_pin.ensure(sizeof(uint32_t) * nwords));
    HIPCHK(c->rc_ops_prog.ensure(256));
    __atomic_store_n(c->rc_ops_prog.host<unsigned>(), 0u, __ATOMIC_SEQ_CST);
    wb.ops = c->rc_ops_pin.dev<uint32_t>();
    wb.ops_prog = c->rc_ops_prog.dev<unsigned>();
    // the walk's result words to pinned memory too: no hipMemcpy after the walk (round 6: the call's tail after the
    // walk held five small copies, ~0.1 ms)
    HIPCHK(c->res_pin.ensure(64 * sizeof(int)));
    std::memset(c->res_pin.p, 0, 64 * sizeof(int));
    wb.result = c->res_pin.dev<int>();
    return GA_OK;
}

// The context's side stream (the table's upload, the fill's result words), created by the first call that needs it.
static int side_stream(ga_ctx* c) {
    if (!c->ustream) HIPCHK(hipStreamCreateWithPriority(&c->ustream, hipStreamNonBlocking, c->priority));
    return GA_OK;
}

// The fill's result words (H'(m, n), the abort word) copied to pinned memory on the upload stream as soon as the
// fill ends, beside the walk (not on the fill's stream, where the copies would delay the walk's start), and read
// after the walk with no further copy; the cost's un-shift GV(m) + GH(n) comes from the host's own sums.
int fill_results_async(ga_ctx* c) {
    if (int r = side_stream(c)) return r;
    if (!c->ev_fill) HIPCHK(hipEventCreateWithFlags(&c->ev_fill, hipEventDisableTiming));
    if (!c->ev_res) HIPCHK(hipEventCreateWithFlags(&c->ev_res, hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->ev_fill, c->stream));
    HIPCHK(hipStreamWaitEvent(c->ustream, c->ev_fill, 0));
    int* res = c->res_pin.host<int>();
    HIPCHK(hipMemcpyAsync(res + 16, c->fb.out_last.p, sizeof(int) * 4, hipMemcpyDeviceToHost, c->ustream));
    HIPCHK(hipMemcpyAsync(res + 20, c->fb.flags.as<unsigned>() + 1, sizeof(unsigned), hipMemcpyDeviceToHost, c->ustream));
    HIPCHK(hipEventRecord(c->ev_res, c->ustream));
    return GA_OK;
}

int fill_results_finish(ga_ctx* c, int64_t* cost_out) {
    HIPCHK(hipEventSynchronize(c->ev_res));
    HIPCHK(hipEventElapsedTime(&c->fill_ms, c->fb.ev[0], c->fb.ev[1]));
    const int* res = c->res_pin.host<int>();
    if (res[20]) return fail(GA_E_TIMEOUT, "fill kernel hand-off wait timed out");
    c->GV_m = (int)c->gv_total;
    if (cost_out) *cost_out = (int64_t)res[16] + c->gv_total + c->gh_total;
    return GA_OK;
}

// The calling thread's side of such a walk (launched on wb.stream after the fill): decode the levels as
// the progress word covers them, then the fill's cost, the walk's result words, the last levels, the
// tails and the final random state
int streamed_walk_finish(ga_ctx* c, const RngTable& R, const WalkBufs& wb, const WalkStart& st0, double t0,
                         uint32_t* mt_state, const char* a_chr, const char* b_chr, char* oa, char* om, char* ob,
                         int64_t cap, int64_t* out_len, int32_t* tb_status, int64_t* cost_out) {
    const int64_t m = c->m, n = c->n;
    const int64_t nwords = (m + n + 1 + 15) / 16 + 64;
    WalkStart st = st0;
    int reason = 0;
    int64_t len = 0;
    {
        // decode dispatches [D, D1) of the levels (dp_array_backward's column output, in walk order)
        const uint32_t* ops = c->rc_ops_pin.host<uint32_t>();
        const unsigned* prog = c->rc_ops_prog.host<unsigned>();
        gastr::Columns col{a_chr, m, b_chr, n, oa, om, ob, cap, st.i, st.j, st.L};
        int64_t D = st.D;
        auto decode_to = [&](int64_t D1) {
            col.decode<false>(ops, 0, D, D1);
            D = std::max(D, D1);
        };
        const int64_t lag = c->wk.rc_decode_lag;  // (diagnostics) dispatches held back
        std::vector<uint32_t> seen;  // (diagnostics) GA_RC_DECODE_CHECK: the words as decoded
        const bool check = c->wk.rc_decode_check;
        if (check) seen.assign((size_t)nwords, 0u);
        for (;;) {
            const unsigned pr = __atomic_load_n(prog, __ATOMIC_ACQUIRE);
            if ((int64_t)pr - lag > D) {
                if (check)
                    for (int64_t q = D >> 4; q < (((int64_t)pr - lag + 15) >> 4); q++) seen[q] = ops[q];
                decode_to((int64_t)pr - lag);
                continue;
            }
            const hipError_t q = hipStreamQuery(wb.stream);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) return fail(GA_E_HIP, std::string("walk: ") + hipGetErrorString(q));
            std::this_thread::yield();
        }
        // the fill's cost and abort word (copied to pinned memory while the walk ran) and the walk's result words
        // (written to pinned memory by the walk): no copy here
        if (int rr = fill_results_finish(c, cost_out)) return rr;
        int res[16];
        std::memcpy(res, c->res_pin.p, sizeof(res));
        HIPCHK(hipEventElapsedTime(&c->walk_ms, wb.ev0, wb.ev1));
        take_walk_diag(c, res);
        reason = res[3];
        if (reason == 7) return fail(GA_E_TIMEOUT, "recompute walk: a tile was never recomputed");
        const int64_t D1 = res[0];
        if (D > D1) return fail(GA_E_STATE, "walk levels published past the walk's end");
        if (check) {
            int64_t bad = 0, first_bad = -1;
            for (int64_t q = 0; q < (D >> 4); q++)
                if (seen[q] != ops[q]) {
                    bad++;
                    if (first_bad < 0) first_bad = q;
                }
            if (bad)
                return fail(GA_E_STATE, "decode check: " + std::to_string(bad) + " level words changed after decode, first " +
                                            std::to_string(first_bad) + " of " + std::to_string(D >> 4) + " (D1 " +
                                            std::to_string(D1) + ")");
        }
        decode_to(D1);
        if (reason == 4) {  // (never here: such walks are degenerate, reason 7) the reference's IndexError
            col.len = 0;
            col.i = st.i;
            col.j = st.j;
        }
        advance_walk(st, col, D1);
        len = col.len;
        if (len > cap) return fail(GA_E_ARG, "output capacity too small");
    }
    const int rc = conclude_walk(R, st, reason, mt_state, a_chr, b_chr, oa, om, ob, cap, len, out_len, tb_status);
    c->call_ms = (float)(now_ms() - t0);
    return rc;
}

int rc_align(ga_ctx* c, uint32_t* mt_state, const char* a_chr, const char* b_chr, char* oa, char* om, char* ob,
             int64_t cap, int64_t* out_len, int32_t* tb_status, int64_t* cost_out) {
    const double t0 = now_ms();
    const int64_t m = c->m, n = c->n;
    // the walk's position words cleared before the fill (a memset between the fill and the walk delayed the walk)
    HIPCHK(c->rc_pos.ensure(16));
    HIPCHK(hipMemsetAsync(c->rc_pos.p, 0, 16, c->stream));
    if (int r = rc_fill(c)) {
        c->rc_pos_zeroed = false;
        return r;
    }
    c->rc_pos_zeroed = true;
    // the tie-break table on the host while the device fills
    RngTable R;
    const double t1 = now_ms();
    build_rng(mt_state, m + n + 1, R);
    c->rng_ms = (float)(now_ms() - t1);
    WalkBufs wb = ctx_walk_bufs(c);
    const int64_t ntab = (int64_t)R.tab.size();
    // the table goes up on a stream of its own while the fill still runs (pinned staging: the copy is asynchronous),
    // and the walk's stream waits for it: the walk launch below is then queued behind the fill at once
    HIPCHK(c->up_pin.ensure(sizeof(uint32_t) * ntab));
    if (int r = side_stream(c)) return r;
    if (!c->ev_up) HIPCHK(hipEventCreateWithFlags(&c->ev_up, hipEventDisableTiming));
    // (the last call's copy out of the staging buffer has ended: its walk waited for it, and the call for its walk)
    std::memcpy(c->up_pin.p, R.tab.data(), sizeof(uint32_t) * ntab);
    HIPCHK(hipMemcpyAsync(wb.rng, c->up_pin.p, sizeof(uint32_t) * ntab, hipMemcpyHostToDevice, c->ustream));
    HIPCHK(hipEventRecord(c->ev_up, c->ustream));
    HIPCHK(hipStreamWaitEvent(wb.stream, c->ev_up, 0));
    // the walk's levels go to pinned host memory, and this thread decodes them while the walk runs
    if (int r = pinned_walk_levels(c, wb)) return r;
    // (after the table's upload on the same side stream: the copies there wait for the fill's end)
    if (int r = fill_results_async(c)) return r;
    const WalkStart st0 = walk_origin(c);
    if (int r = rc_walk_launch(c, ntab, st0, wb)) return r;
    return streamed_walk_finish(c, R, wb, st0, t0, mt_state, a_chr, b_chr, oa, om, ob, cap, out_len, tb_status, cost_out);
}

// ---------------------------------------------------------------- the calls (their exported wrappers: ga_host.cpp)
int problem_traceback_impl(ga_ctx* c, uint32_t* mt_state, const char* a_chr, const char* b_chr, char* oa, char* om,
                           char* ob, int64_t cap, int64_t* out_len, int32_t* tb_status) {
    if (int r = check_ctx(c)) return r;
    if (!c->filled_tb) return fail(GA_E_STATE, "traceback needs a GA_FILL_TRACEBACK fill first");
    if (!mt_state || !a_chr || !b_chr || !oa || !om || !ob || !out_len || !tb_status) return fail(GA_E_ARG, "null argument");
    RngTable R;
    build_rng(mt_state, c->m + c->n + 1, R);
    if (int r = run_walk(c, R.tab.data(), (int64_t)R.tab.size(), walk_origin(c))) return r;
    return finish_walk(c, R, mt_state, a_chr, b_chr, oa, om, ob, cap, out_len, tb_status);
}

int problem_align_impl(ga_ctx* c, uint32_t* mt_state, const char* a_chr, const char* b_chr, char* oa, char* om,
                       char* ob, int64_t cap, int64_t* out_len, int32_t* tb_status, int64_t* cost_out) {
    if (int r = check_ctx(c)) return r;
    if (c->slab) return fail(GA_E_STATE, "slab contexts use ga_slab_fill_launch");
    if (!mt_state || !a_chr || !b_chr || !oa || !om || !ob || !out_len || !tb_status) return fail(GA_E_ARG, "null argument");
    c->rc_used = false;
    if (gawalk::rc_eligible(plan_problem(c), c->wk, false)) {
        const int r = rc_align(c, mt_state, a_chr, b_chr, oa, om, ob, cap, out_len, tb_status, cost_out);
        // checkpoints that do not fit this device (refused before anything was enqueued, or an allocation that
        // failed, after which the recompute buffers are released): the banded / stored-words paths below
        if (r != GA_E_NOMEM) return r;
        c->rc_used = false;
    }
    if (const int64_t Bh = band_rows(c)) return banded_align(c, Bh, mt_state, a_chr, b_chr, oa, om, ob, cap, out_len,
                                                             tb_status, cost_out);
    const double t0 = now_ms();
    if (int r = enqueue_fill(c, GA_FILL_TRACEBACK)) return r;
    // the tie-break table is built on the host while the device fills
    RngTable R;
    const double t1 = now_ms();
    build_rng(mt_state, c->m + c->n + 1, R);
    c->rng_ms = (float)(now_ms() - t1);
    if (gawalk::streamed(c->m, c->n, c->wk)) {
        // levels to pinned host memory, decoded while the walk runs (as rc_align)
        WalkBufs wb = ctx_walk_bufs(c);
        if (int r = pinned_walk_levels(c, wb)) return r;
        if (int r = fill_results_async(c)) return r;
        const WalkStart st0 = walk_origin(c);
        if (int r = run_walk(c, R.tab.data(), (int64_t)R.tab.size(), st0, 0, -1, false, true, &wb)) return r;
        return streamed_walk_finish(c, R, wb, st0, t0, mt_state, a_chr, b_chr, oa, om, ob, cap, out_len, tb_status,
                                    cost_out);
    }
    if (int r = run_walk(c, R.tab.data(), (int64_t)R.tab.size(), walk_origin(c))) return r;
    if (int r = finish_fill(c, cost_out, nullptr)) return r;
    const int rc = finish_walk(c, R, mt_state, a_chr, b_chr, oa, om, ob, cap, out_len, tb_status);
    c->call_ms = (float)(now_ms() - t0);
    return rc;
}

}  // namespace gahost
