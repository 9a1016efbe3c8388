// ga_batch_host.cpp -- the batch engine behind ga_batch_costs, ga_batch_align, ga_batch_sample, ga_batch_count,
// ga_batch_rank, ga_batch_support and ga_debug_pair_tables: staging and launches of the batch
// kernels, the one table stage and the one decode of the calls with strings, and the one stored-words fill of the last
// four calls: enqueue_chunk_fill / finish_chunk_fill for the kernel pairs, chunk by chunk, large_route for a pair that
// left the kernel route for its size, check_single_pairs for what is refused before anything is launched.  Each of the
// four adds its own kernels behind a fill, over the `Filled` either route yields.  It reaches the rest of the engine
// through ga_host_internal.h.
#include <cmath>
#include <cstring>

#include "ga_host_internal.h"
#include "ga_batch.h"
#include "ga_batch_align.h"
#include "ga_batch_layout.h"
#include "ga_batch_rng.h"

using namespace gahost;
using namespace garng;

namespace gahost {

// resident waves of a batch launch: two per SIMD on every CU
int64_t batch_max_waves(const ga_ctx* c) { return (int64_t)c->num_cu * 4 * 2; }
// the waves of a launch over n work items: never more waves than items; whole workgroups
int launch_waves(const ga_ctx* c, int64_t n) {
    const int W = gabatch::kWavesPerGroup;
    return (int)((std::min<int64_t>(batch_max_waves(c), n) + W - 1) / W * W);
}
// how every message about pair k of a batch starts (k < 0: nothing, where batch_single_pair names the pair itself)
std::string pair_prefix(int64_t k) { return k >= 0 ? "pair " + std::to_string(k) + ": " : std::string(); }
// c->rev, created with the first launch that records them
int ensure_rev(ga_ctx* c) {
    for (hipEvent_t& e : c->rev)
        if (!e) HIPCHK(hipEventCreate(&e));
    return GA_OK;
}

// A batch as every entry point takes it.
struct BatchIn {
    const uint8_t* codes;
    const int64_t* seq_off;
    int64_t nseq;
    const int32_t *pair_a, *pair_b, *pair_max_cost;
    int64_t npairs;
    const ga_costs* cs;
    int64_t m(int64_t k) const { return seq_off[pair_a[k] + 1] - seq_off[pair_a[k]]; }
    int64_t n(int64_t k) const { return seq_off[pair_b[k] + 1] - seq_off[pair_b[k]]; }
};

// What ga_batch_costs_ex and ga_batch_align stage alike for the planner's work list, on the context's stream: the
// launch's waves, and the codes, work list, sub' / gap tables, zeroed ticket, cost and edge-scratch buffers behind
// `args`.  subp is the upload's source: it lives until the caller has synchronised the stream.
struct BatchStage {
    std::vector<int> subp;
    ga::BatchArgs args{};
    int waves = 0;
};
int stage_batch(ga_ctx* c, const uint8_t* codes, const int64_t* seq_off, int64_t nseq, int64_t npairs, const ga_costs* cs,
                const std::vector<ga_batch_item>& items, int64_t scratch_rows, BatchStage& bs) {
    const int K = cs->K, nitems = (int)items.size();
    const int waves = bs.waves = launch_waves(c, nitems);
    bs.subp = shifted_sub(cs);
    const size_t ncodes = (size_t)seq_off[nseq];
    HIPCHK(c->bt_codes.ensure(ncodes));
    HIPCHK(c->bt_items.ensure(sizeof(ga_batch_item) * nitems));
    HIPCHK(c->bt_sub.ensure(sizeof(int) * K * K));
    HIPCHK(c->bt_gh.ensure(sizeof(int) * K));
    HIPCHK(c->bt_gv.ensure(sizeof(int) * K));
    HIPCHK(c->bt_ticket.ensure(sizeof(unsigned)));
    HIPCHK(c->bt_out.ensure(sizeof(long long) * npairs));
    if (scratch_rows > 0) HIPCHK(c->bt_scratch.ensure(sizeof(int2) * 2 * scratch_rows * waves));
    HIPCHK(hipMemcpyAsync(c->bt_codes.p, codes, ncodes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->bt_items.p, items.data(), sizeof(ga_batch_item) * nitems, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->bt_sub.p, bs.subp.data(), sizeof(int) * K * K, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->bt_gh.p, cs->gap_h, sizeof(int) * K, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->bt_gv.p, cs->gap_v, sizeof(int) * K, hipMemcpyHostToDevice, c->stream));
    // the ticket starts at zero for every launch (no last-arriver reset to rely on)
    HIPCHK(hipMemsetAsync(c->bt_ticket.p, 0, sizeof(unsigned), c->stream));
    bs.args = ga::BatchArgs{c->bt_codes.as<uint8_t>(), c->bt_items.as<ga_batch_item>(), nitems, c->bt_sub.as<int>(),
                            c->bt_gh.as<int>(), c->bt_gv.as<int>(), K, cs->gap_open, c->bt_ticket.as<unsigned>(),
                            c->bt_out.as<long long>(), scratch_rows > 0 ? c->bt_scratch.as<int2>() : nullptr,
                            scratch_rows};
    return GA_OK;
}

// Pair k of a batch through the single-pair path: loaded into the context's problem slot under the pair's own
// max_cost (its sentinel), then run(sa, sb) on its two sequences' indices.  No problem is loaded afterwards.
template <typename Run>
int batch_single_pair(ga_ctx* c, const uint8_t* codes, const int64_t* seq_off, const int32_t* pair_a,
                      const int32_t* pair_b, const int32_t* pair_max_cost, const ga_costs* cs, int64_t k, Run run) {
    const int64_t sa = pair_a[k], sb = pair_b[k];
    const int64_t m = seq_off[sa + 1] - seq_off[sa], n = seq_off[sb + 1] - seq_off[sb];
    ga_costs own = *cs;
    if (pair_max_cost) own.max_cost = pair_max_cost[k];
    int r = load_problem(c, codes + seq_off[sa], m, codes + seq_off[sb], n, &own, nullptr, nullptr, 0, n);
    if (!r) r = run(sa, sb);
    c->loaded = false;
    if (r) return fail(r, pair_prefix(k) + g_err);
    return GA_OK;
}

// How a call's tie-break tables are made: on the device for the items the route rule admits
// (gabrng::route_device) when the call's flags or the context (GA_BATCH_RNG=device) ask for it, with the item limit
// GA_BATCH_RNG_DEVICE_MAX_STEPS and the cap's words per dispatch GA_BATCH_RNG_WORD_CAP (both checked at creation).
struct RngRoute {
    bool want_device = false;
    int64_t max_steps = gabrng::kDeviceMaxSteps;
    int cap_words = gabrng::kCapWordsPerDispatch;
};
RngRoute rng_route(const ga_ctx* c, uint32_t flags) {
    RngRoute r;
    const uint32_t which = flags & GA_BATCH_TABLES_MASK;
    r.want_device = which == GA_BATCH_TABLES_DEVICE || (which == GA_BATCH_TABLES_DEFAULT && c->bk.rng_device_default);
    r.max_steps = c->bk.rng_max_steps;
    r.cap_words = c->bk.rng_cap_words;
    return r;
}

// batch_rng_kernel for `items` on the context's stream, between the events c->rev[0] and c->rev[1]: item t's entries
// go to tab_dev[items[t].tab_off ..), its status word to c->bt_rstatus[t].  `items` is an upload's source: it lives
// until the caller has synchronised the stream.  groups_out: the workgroups launched.
int enqueue_batch_rng(ga_ctx* c, const std::vector<gabrng::Item>& items, uint32_t* tab_dev, int cap_words,
                      int* groups_out) {
    if (!c->rbase_ready) {
        // init_genrand(19650218)'s array, the same for every seed: once per context
        uint32_t base[gabrng::kN];
        gabrng::base_array(base);
        HIPCHK(c->bt_rbase.ensure(sizeof(base)));
        HIPCHK(hipMemcpy(c->bt_rbase.p, base, sizeof(base), hipMemcpyHostToDevice));
        c->rbase_ready = true;
    }
    if (int r = ensure_rev(c)) return r;
    HIPCHK(c->bt_ritems.ensure(sizeof(gabrng::Item) * items.size()));
    HIPCHK(c->bt_rstatus.ensure(sizeof(int32_t) * items.size()));
    HIPCHK(hipMemcpyAsync(c->bt_ritems.p, items.data(), sizeof(gabrng::Item) * items.size(), hipMemcpyHostToDevice,
                          c->stream));
    HIPCHK(hipEventRecord(c->rev[0], c->stream));
    const ga::RngArgs a{c->bt_ritems.as<gabrng::Item>(), (long long)items.size(), c->bt_rbase.as<uint32_t>(), tab_dev,
                        c->bt_rstatus.as<int32_t>(), cap_words};
    *groups_out = ga::launch_batch_rng(c->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->rev[1], c->stream));
    return GA_OK;
}

// The tie-break tables of one launch's walks, in c->bt_rng: the one table stage of ga_batch_align,
// ga_batch_sample (ga_debug_pair_tables uses its pieces).  tables_enqueue splits the jobs by `route`, enqueues
// batch_rng_kernel for the device jobs and builds the host jobs' tables on a few threads meanwhile (sized by the host
// jobs), their ranges uploaded behind the generator; tables_read_back enqueues the copy of the generator's status words,
// behind the caller's launch; after the caller's one hipStreamSynchronize (the stage lives until then: it holds its
// uploads' sources) tables_finish has the figures.
struct TableStage {
    gabatch::TableSplit split;    // split.dev.size() / split.host.size(): the device and host item counts
    std::vector<uint32_t> tab;    // the host jobs' entries, at their places in the launch's table
    std::vector<int32_t> rstatus;
    int groups = 0;       // the generator's workgroups
    float host_ms = 0.f;  // the host's build and upload calls
    float ms = 0.f;       // "tables": the generator's time and whatever of the host's share it did not hide
    // an item stopped at its word cap: the walks read unwritten entries (harmlessly: a walk makes at most m + n - 1
    // steps whatever the table holds), and nothing of the launch is decoded
    bool capped = false;
};
int tables_enqueue(ga_ctx* c, const std::vector<gabrng::Item>& jobs, int64_t tab_entries, const RngRoute& route,
                   TableStage& ts) {
    ts.split = gabatch::split_tables(jobs.data(), (int64_t)jobs.size(), route.want_device, route.max_steps);
    const std::vector<gabrng::Item>& host = ts.split.host;
    uint32_t* tab_dev = c->bt_rng.as<uint32_t>();
    if (!ts.split.dev.empty())
        if (int r = enqueue_batch_rng(c, ts.split.dev, tab_dev, route.cap_words, &ts.groups)) return r;
    const double t_tab = now_ms();
    ts.tab = std::vector<uint32_t>(host.empty() ? 0 : (size_t)tab_entries);
    if (!host.empty()) {
        const int nthreads = gabatch::rng_threads(c->bk.rng_threads, (int64_t)host.size());
        gabatch::build_tables(host.data(), (int64_t)host.size(), nthreads, ts.tab.data());
        // (the work list's table ranges follow each other: neighbouring host items go up in one copy)
        for (const gabatch::TableRange& rg : ts.split.ranges)
            HIPCHK(hipMemcpyAsync(tab_dev + rg.first, ts.tab.data() + rg.first,
                                  sizeof(uint32_t) * (size_t)(rg.last - rg.first), hipMemcpyHostToDevice, c->stream));
    }
    ts.host_ms = (float)(now_ms() - t_tab);
    return GA_OK;
}
// the status words of a generator launch over n items, behind it on the context's stream
int read_back_status(ga_ctx* c, size_t n, std::vector<int32_t>& rstatus) {
    rstatus.assign(n, 0);
    if (n > 0)
        HIPCHK(hipMemcpyAsync(rstatus.data(), c->bt_rstatus.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
    return GA_OK;
}
int tables_read_back(ga_ctx* c, TableStage& ts) { return read_back_status(c, ts.split.dev.size(), ts.rstatus); }
int tables_finish(ga_ctx* c, TableStage& ts) {
    float gen_ms = 0.f;
    if (!ts.split.dev.empty()) HIPCHK(hipEventElapsedTime(&gen_ms, c->rev[0], c->rev[1]));
    ts.ms = gen_ms + std::max(0.f, ts.host_ms - gen_ms);
    for (const int32_t st : ts.rstatus) ts.capped |= st != gabrng::kComplete;
    return GA_OK;
}

int check_table_flags(uint32_t flags) {
    if ((flags & ~GA_BATCH_TABLES_MASK) || (flags & GA_BATCH_TABLES_MASK) > GA_BATCH_TABLES_DEVICE)
        return fail(GA_E_ARG, "bad flags: bits 0-1 choose the tables (0 default, 1 host, 2 device)");
    return GA_OK;
}
// the output slots [first, last) of pair k each hold the pair's longest alignment, m + n characters
int check_out_capacity(const int64_t* seq_off, const int32_t* pair_a, const int32_t* pair_b, int64_t k,
                       const int64_t* out_off, int64_t first, int64_t last) {
    const int64_t need = seq_off[pair_a[k] + 1] - seq_off[pair_a[k]] + seq_off[pair_b[k] + 1] - seq_off[pair_b[k]];
    for (int64_t f = first; f < last; f++)
        if (out_off[f] < 0 || out_off[f + 1] - out_off[f] < need)
            return fail(GA_E_ARG, pair_prefix(k) + "output capacity too small");
    return GA_OK;
}
// A slab context keeps its slab: the pairs in `single` cannot go through its problem slot (what: "fill" or "path").
int refuse_slab_single(const ga_ctx* c, const std::vector<int64_t>& single, const char* what) {
    if (single.empty() || !c->slab) return GA_OK;
    return fail(GA_E_STATE, pair_prefix(single[0]) + "needs the single-pair " + what + ", which a slab context cannot run");
}

// A batch launch's costs into cost_out, for the pairs of its work list.
int take_batch_costs(const std::vector<long long>& got, const ga_batch_item* items, size_t nitems, int64_t* cost_out) {
    for (size_t t = 0; t < nitems; t++) {
        const size_t k = (size_t)items[t].out;
        if (got[k] == INT64_MIN)
            return fail(GA_E_STATE, pair_prefix((int64_t)k) + "work item does not fit the batch launch");
        cost_out[k] = got[k];
    }
    return GA_OK;
}

// gabatch::decode_walk's codes in the serial pass after the threaded decode.  pair: the pair the message names, or -1
// where batch_single_pair names it itself (a large-route walk); no_fit: the launch's wording of -3.
int check_decoded(int64_t len, int64_t pair, const char* no_fit) {
    if (len >= 0) return GA_OK;
    return fail(GA_E_STATE, pair_prefix(pair) + (len == -3 ? no_fit : "the walk's levels do not decode"));
}

// Output slot f of pair k through the single-pair path, from the state seeds[f] starts (what it leaves is dropped).
int batch_single_align(ga_ctx* c, const uint8_t* codes, const int64_t* seq_off, const int32_t* pair_a,
                       const int32_t* pair_b, const int32_t* pair_max_cost, const ga_costs* cs, int64_t k, int64_t f,
                       const uint64_t* seeds, const gabatch::WalkOut& o, int64_t* cost_out) {
    uint32_t state[MTN + 1];
    auto align = [&](int64_t sa, int64_t sb) {
        seed_state(seeds[f], state);
        const int64_t at = o.out_off[f];
        return ga_problem_align(c, state, o.chars + seq_off[sa], o.chars + seq_off[sb], o.out_a + at, o.out_mid + at,
                                o.out_b + at, o.out_off[f + 1] - at, &o.out_len[f], &o.tb_status[f], &cost_out[k]);
    };
    return batch_single_pair(c, codes, seq_off, pair_a, pair_b, pair_max_cost, cs, k, align);
}

// a context's figures of its last batched call (the info and timings getters)
template <typename T, size_t N>
int copy_figures(const ga_ctx* c, T (ga_ctx::*figures)[N], T* out) {
    if (!c || !out) return fail(GA_E_ARG, "null argument");
    std::copy(c->*figures, c->*figures + N, out);
    return GA_OK;
}

// ---- the stored-words fill of ga_batch_sample, ga_batch_count, ga_batch_rank and ga_batch_support

// The planners' limits from the context's knobs and the launch's waves (each planner reads the ones it names).
gabatch::WordsLimits words_limits(const ga_ctx* c) {
    gabatch::WordsLimits lim;
    if (c->bk.align_max_cells) lim.max_cells = *c->bk.align_max_cells;
    if (c->bk.sample_chunk_words) lim.chunk_tb_words = *c->bk.sample_chunk_words;
    if (c->bk.sample_walk_entries) lim.walk_entries = *c->bk.sample_walk_entries;
    if (c->bk.rank_table_bytes) lim.chunk_table_bytes = *c->bk.rank_table_bytes;
    if (c->bk.support_bytes) lim.chunk_support_bytes = *c->bk.support_bytes;
    lim.scratch_rows_cap = gabatch::scratch_rows_cap(batch_max_waves(c));
    lim.count_rows_cap = gabatch::count_rows_cap(batch_max_waves(c));
    return lim;
}

// The pairs of one fill as the kernels behind it take them: their work list, here and on the device, their slices on
// the device, their words in tb (tb_words u32s, `layout`, `tc`).
struct Filled {
    std::vector<ga_batch_item> items;
    const ga_batch_item* items_dev;
    const ga_batch_words_item* words_dev;
    const uint32_t* tb;
    int64_t tb_words;
    int CB, layout, tc;
};
// What a call adds to a chunk's fill: an array with an entry per pair, uploaded beside the slices, and a large buffer
// that is allocated with the chunk's words and shares their out-of-memory verdict.
struct ChunkUpload {
    DevBuf* buf;
    const void* src;
    size_t bytes;
};
struct ChunkAlloc {
    DevBuf* buf;
    size_t bytes;
};
struct ChunkFill {
    BatchStage bs;  // the launch's waves (and an upload's source)
    Filled f;
    std::vector<long long> got;
};

// Chunk ch of `plan` on the context's stream: stage_batch for its pairs, its slices and the call's uploads, then
// batch_words_kernel between the events c->fb.ev, its words into c->bs_tb.  nomem: the call's wording of no memory for
// the words and its allocs.  The caller enqueues its own kernels behind it, then finish_chunk_fill.
int enqueue_chunk_fill(ga_ctx* c, const BatchIn& in, const gabatch::WordsPlan& plan, const gabatch::FillChunk& ch,
                       std::initializer_list<ChunkUpload> uploads, std::initializer_list<ChunkAlloc> allocs,
                       const char* nomem, ChunkFill& cf) {
    // (the device pointers follow once the buffers are ensured)
    cf.f = Filled{{plan.kernel.begin() + ch.first, plan.kernel.begin() + ch.first + ch.count}, nullptr, nullptr, nullptr,
                  ch.tb_words, plan.CB, gabatch::LAYOUT_BATCH, 0};
    Filled& f = cf.f;
    if (int r = stage_batch(c, in.codes, in.seq_off, in.nseq, in.npairs, in.cs, f.items, plan.scratch_rows, cf.bs)) return r;
    HIPCHK(c->bs_words.ensure(sizeof(ga_batch_words_item) * f.items.size()));
    for (const ChunkUpload& u : uploads) HIPCHK(u.buf->ensure(u.bytes));
    bool fits = c->bs_tb.ensure(sizeof(uint32_t) * (size_t)ch.tb_words) == hipSuccess;
    for (const ChunkAlloc& a : allocs) fits = fits && a.buf->ensure(a.bytes) == hipSuccess;
    if (!fits) {
        (void)hipStreamSynchronize(c->stream);  // the staged uploads read this call's buffers
        return fail(GA_E_NOMEM, nomem);
    }
    HIPCHK(hipMemcpyAsync(c->bs_words.p, plan.words.data() + ch.first, sizeof(ga_batch_words_item) * f.items.size(),
                          hipMemcpyHostToDevice, c->stream));
    for (const ChunkUpload& u : uploads) HIPCHK(hipMemcpyAsync(u.buf->p, u.src, u.bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->fb.ev[0], c->stream));
    const ga::WordsArgs q{cf.bs.args, c->bs_words.as<ga_batch_words_item>(), c->bs_tb.as<uint32_t>(), (long long)ch.tb_words};
    ga::launch_batch_words(c->stream, q, plan.qbytes, plan.CB, cf.bs.waves);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->fb.ev[1], c->stream));
    f.items_dev = q.b.items;
    f.words_dev = q.words;
    f.tb = q.tb;
    cf.got.resize((size_t)in.npairs);  // (while the fill runs)
    return GA_OK;
}
// The chunk's one wait, behind the costs' copy back and whatever copies the caller enqueued: the fill's time added to
// fill_ms, the costs into cost_out.
int finish_chunk_fill(ga_ctx* c, const BatchIn& in, ChunkFill& cf, float& fill_ms, int64_t* cost_out) {
    HIPCHK(hipMemcpyAsync(cf.got.data(), c->bt_out.p, sizeof(long long) * in.npairs, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipEventElapsedTime(&c->fill_ms, c->fb.ev[0], c->fb.ev[1]));
    fill_ms += c->fill_ms;
    return take_batch_costs(cf.got, cf.f.items.data(), cf.f.items.size(), cost_out);
}

// The large route: pair k left the kernel route for its size and is filled once by the single-pair engine with stored
// words, as ga_problem_align's stored-words route up to the walk (its time added to fill_ms, its cost to cost_out[k]);
// then(f) runs the call's kernels over c->fb.tb in that fill's layout, with gabatch::large_route_work's one-pair work
// list and slice on the device (with_codes: the batch's codes too, for a walk that reads them) and waits for them:
// the uploads' sources live until it returns.  Where the words do not fit band_rows' budget, a call without a banded
// route (activity: its name for gabatch::no_band_reason) fails; with activity == nullptr nothing is launched and
// `filled` stays false.  It goes through the context's problem slot, so no problem is loaded afterwards.
template <typename Then>
int large_route(ga_ctx* c, const BatchIn& in, int64_t k, const char* activity, bool with_codes, float& fill_ms,
                int64_t* cost_out, bool& filled, Then then) {
    filled = false;
    c->rc_used = false;
    auto run = [&](int64_t sa, int64_t sb) -> int {
        if (band_rows(c) != 0) return activity ? fail(GA_E_ARG, gabatch::no_band_reason(activity)) : GA_OK;
        if (int r = enqueue_fill(c, GA_FILL_TRACEBACK)) return r;
        if (int r = finish_fill(c, &cost_out[k], nullptr)) return r;
        fill_ms += c->fill_ms;
        const gaplan::FillPlan& pl = c->plan;
        gabatch::LargeWork w;
        if (const char* why = gabatch::large_route_work(in.m(k), in.n(k), k, in.seq_off[sa], in.seq_off[sb], pl.nstripes,
                                                        pl.T, pl.TC, c->CB, w))
            return fail(GA_E_STATE, why);
        const size_t ncodes = (size_t)in.seq_off[in.nseq];
        if (with_codes) HIPCHK(c->bt_codes.ensure(ncodes));
        HIPCHK(c->bt_items.ensure(sizeof(ga_batch_item)));
        HIPCHK(c->bs_words.ensure(sizeof(ga_batch_words_item)));
        if (with_codes) HIPCHK(hipMemcpyAsync(c->bt_codes.p, in.codes, ncodes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->bt_items.p, &w.item, sizeof(w.item), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->bs_words.p, &w.words, sizeof(w.words), hipMemcpyHostToDevice, c->stream));
        filled = true;
        return then(Filled{{w.item}, c->bt_items.as<ga_batch_item>(), c->bs_words.as<ga_batch_words_item>(),
                           c->fb.tb.as<uint32_t>(), w.words.tb_words, c->CB, gabatch::LAYOUT_STRIPE, pl.TC});
    };
    if (int r = batch_single_pair(c, in.codes, in.seq_off, in.pair_a, in.pair_b, in.pair_max_cost, in.cs, k, run)) return r;
    c->filled_tb = false;
    return GA_OK;
}

// What left the kernel route of ga_batch_count, ga_batch_rank or ga_batch_support is handled from a single-pair fill
// with stored words or not at all: the lowest pair that cannot be is refused before anything is launched, with
// gabatch::single_pair_verdict's reason in the call's words.
int check_single_pairs(ga_ctx* c, const BatchIn& in, const gabatch::WordsPlan& plan, const char* subject,
                       const char* activity) {
    int64_t bad = -1, avail = -1;
    std::string reason;
    for (const int64_t k : plan.single) {
        if (bad >= 0 && k > bad) continue;
        const int64_t m = in.m(k), n = in.n(k);
        int64_t band = 0;
        if (std::min(m, n) >= 2) {
            // (forced rows, tests, do not ask the device what it has free: band_rows, ga_align_host.cpp)
            if (avail < 0) avail = c->wk.tb_band_rows ? 0 : dev_avail_bytes(c, (int64_t)c->fb.tb.cap);
            band = gawalk::band_rows(m, n, plan.CB, c->wk, avail);
        }
        const std::string why = gabatch::single_pair_verdict(m, n, band, gabatch::count_rows_cap(gabatch::kWavesPerGroup),
                                                             subject, activity);
        if (!why.empty()) bad = k, reason = why;
    }
    if (bad >= 0) return fail(GA_E_ARG, pair_prefix(bad) + reason);
    return GA_OK;
}

}  // namespace gahost

extern "C" {

int ga_batch_costs(ga_ctx* c, const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                   const int32_t* pair_b, int64_t npairs, const ga_costs* cs, int64_t* cost_out) {
    return ga_batch_costs_ex(c, codes, seq_off, nseq, pair_a, pair_b, nullptr, npairs, cs, cost_out);
}

static int batch_costs_ex_impl(ga_ctx* c, const uint8_t* codes, const int64_t* seq_off, int64_t nseq,
                               const int32_t* pair_a, const int32_t* pair_b, const int32_t* pair_max_cost,
                               int64_t npairs, const ga_costs* cs, int64_t* cost_out) {
    if (int r = check_ctx(c)) return r;
    if (npairs == 0) return GA_OK;  // an empty batch: no launch
    if (!cost_out) return fail(GA_E_ARG, "null argument");
    // the planner's routing limits
    gabatch::Limits lim;
    if (c->bk.max_cells) lim.max_cells = *c->bk.max_cells;
    lim.scratch_rows_cap = gabatch::scratch_rows_cap(batch_max_waves(c));
    gabatch::Plan plan;
    std::string why;
    if (int r = gabatch::plan_batch(codes, seq_off, nseq, pair_a, pair_b, pair_max_cost, npairs, cs, lim, plan, why))
        return fail(r, why);
    if (!plan.kernel.empty()) {
        BatchStage bs;
        if (int r = stage_batch(c, codes, seq_off, nseq, npairs, cs, plan.kernel, plan.scratch_rows, bs)) return r;
        HIPCHK(hipEventRecord(c->fb.ev[0], c->stream));
        ga::launch_batch_fill(c->stream, bs.args, plan.qbytes, bs.waves);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->fb.ev[1], c->stream));
        std::vector<long long> got((size_t)npairs);
        HIPCHK(hipMemcpyAsync(got.data(), c->bt_out.p, sizeof(long long) * npairs, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipEventElapsedTime(&c->fill_ms, c->fb.ev[0], c->fb.ev[1]));
        if (int r = take_batch_costs(got, plan.kernel.data(), plan.kernel.size(), cost_out)) return r;
    }
    if (!plan.single.empty()) {
        // the existing score fill, one pair at a time (as ga_problem_set + ga_problem_fill): it goes through the
        // context's problem slot, so no problem is loaded afterwards.  A slab context keeps its slab: refused.
        if (int r = refuse_slab_single(c, plan.single, "fill")) return r;
        c->rc_used = false;
        for (const int64_t k : plan.single) {
            auto fill = [&](int64_t, int64_t) {
                const int e = enqueue_fill(c, 0);
                return e ? e : finish_fill(c, &cost_out[k], nullptr);
            };
            if (int r = batch_single_pair(c, codes, seq_off, pair_a, pair_b, pair_max_cost, cs, k, fill)) return r;
        }
    }
    return GA_OK;
}

int ga_batch_align(ga_ctx* c, const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                   const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* cs,
                   const uint64_t* seeds, const char* chars, char* out_a, char* out_mid, char* out_b,
                   const int64_t* out_off, int64_t* out_len, int32_t* tb_status, int64_t* cost_out) {
    return ga_batch_align_ex(c, codes, seq_off, nseq, pair_a, pair_b, pair_max_cost, npairs, cs, seeds, chars, out_a,
                             out_mid, out_b, out_off, out_len, tb_status, cost_out, GA_BATCH_TABLES_DEFAULT);
}

static int batch_align_ex_impl(ga_ctx* c, const uint8_t* codes, const int64_t* seq_off, int64_t nseq,
                               const int32_t* pair_a, const int32_t* pair_b, const int32_t* pair_max_cost,
                               int64_t npairs, const ga_costs* cs, const uint64_t* seeds, const char* chars,
                               char* out_a, char* out_mid, char* out_b, const int64_t* out_off, int64_t* out_len,
                               int32_t* tb_status, int64_t* cost_out, uint32_t flags) {
    if (int r = check_ctx(c)) return r;
    if (int r = check_table_flags(flags)) return r;
    for (int32_t& x : c->batch_rng_info) x = 0;
    if (npairs == 0) return GA_OK;  // an empty batch: no launch
    if (!seeds || !chars || !out_a || !out_mid || !out_b || !out_off || !out_len || !tb_status || !cost_out)
        return fail(GA_E_ARG, "null argument");
    const double t_call = now_ms();
    for (float& x : c->batch_align_ms) x = 0.f;
    const int64_t max_waves = batch_max_waves(c);
    gabatch::AlignLimits lim;
    if (c->bk.align_max_cells) lim.max_cells = *c->bk.align_max_cells;
    lim.scratch_rows_cap = gabatch::scratch_rows_cap(max_waves);
    lim.tb_words_cap = gabatch::tb_slice_words_cap(max_waves);
    gabatch::AlignPlan plan;
    std::string why;
    if (int r = gabatch::plan_batch_align(codes, seq_off, nseq, pair_a, pair_b, pair_max_cost, npairs, cs, lim, plan,
                                          why))
        return fail(r, why);
    for (int64_t k = 0; k < npairs; k++)
        if (int r = check_out_capacity(seq_off, pair_a, pair_b, k, out_off, k, k + 1)) return r;
    if (int r = refuse_slab_single(c, plan.single, "path")) return r;
    const gabatch::WalkOut out{chars, out_a, out_mid, out_b, out_off, out_len, tb_status};
    // every kernel pair's table from its own seed
    const int nitems = (int)plan.kernel.size();
    std::vector<gabrng::Item> jobs;
    jobs.reserve((size_t)nitems);
    for (int t = 0; t < nitems; t++) {
        const ga_batch_item& it = plan.kernel[(size_t)t];
        jobs.push_back(gabrng::Item{seeds[it.out], plan.walk[(size_t)t].tab_off, it.m + it.n, 0});
    }
    // The kernel pairs with their tables by `route`; fell_back: the generator reached an item's word cap, nothing of
    // the launch was decoded and the caller runs the pairs again with host tables.
    auto kernel_pairs = [&](const RngRoute& route, bool& fell_back) -> int {
        BatchStage bs;
        if (int r = stage_batch(c, codes, seq_off, nseq, npairs, cs, plan.kernel, plan.scratch_rows, bs)) return r;
        // its own: the walk items, the pairs' tables, their level words and walk results, the waves' traceback words
        HIPCHK(c->bt_witems.ensure(sizeof(ga_batch_walk_item) * nitems));
        HIPCHK(c->bt_walk.ensure(sizeof(int4) * 2 * npairs));
        HIPCHK(c->bt_rng.ensure(sizeof(uint32_t) * plan.tab_entries));
        HIPCHK(c->bt_ops.ensure(sizeof(uint32_t) * plan.ops_words));
        if (c->bt_tb.ensure(sizeof(uint32_t) * (size_t)plan.tb_words * bs.waves) != hipSuccess) {
            (void)hipStreamSynchronize(c->stream);  // the staged uploads read this call's buffers
            return fail(GA_E_NOMEM, "no device memory for the batch's traceback words");
        }
        HIPCHK(hipMemcpyAsync(c->bt_witems.p, plan.walk.data(), sizeof(ga_batch_walk_item) * nitems,
                              hipMemcpyHostToDevice, c->stream));
        // the tables ahead of the walks, on the same stream
        TableStage ts;
        if (int r = tables_enqueue(c, jobs, plan.tab_entries, route, ts)) return r;
        c->batch_align_ms[1] = ts.host_ms;
        c->batch_rng_info[0] = (int32_t)ts.split.dev.size();
        c->batch_rng_info[1] = (int32_t)ts.split.host.size();
        c->batch_rng_info[3] = ts.groups;
        HIPCHK(hipEventRecord(c->fb.ev[0], c->stream));
        const ga::AlignArgs q{bs.args, c->bt_witems.as<ga_batch_walk_item>(), c->bt_rng.as<uint32_t>(),
                              c->bt_ops.as<uint32_t>(), c->bt_walk.as<int4>(), c->bt_tb.as<uint32_t>(), plan.tb_words};
        ga::launch_batch_align(c->stream, q, plan.qbytes, plan.CB, bs.waves);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->fb.ev[1], c->stream));
        std::vector<long long> got((size_t)npairs);
        std::vector<int4> walked((size_t)npairs * 2);
        std::vector<uint32_t> ops((size_t)plan.ops_words);
        HIPCHK(hipMemcpyAsync(got.data(), c->bt_out.p, sizeof(long long) * npairs, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(walked.data(), c->bt_walk.p, sizeof(int4) * 2 * npairs, hipMemcpyDeviceToHost,
                              c->stream));
        HIPCHK(hipMemcpyAsync(ops.data(), c->bt_ops.p, sizeof(uint32_t) * ops.size(), hipMemcpyDeviceToHost, c->stream));
        // the generator's status words come back with the walks' results, in the same synchronisation
        if (int r = tables_read_back(c, ts)) return r;
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipEventElapsedTime(&c->fill_ms, c->fb.ev[0], c->fb.ev[1]));
        c->batch_align_ms[0] = c->fill_ms;
        if (int r = tables_finish(c, ts)) return r;
        c->batch_align_ms[1] = ts.ms;
        fell_back = ts.capped;
        if (fell_back) return GA_OK;
        // the strings, on threads sized by the kernel pairs (every pair writes its own outputs); out_len < 0: see below
        const double t_dec = now_ms();
        gabatch::run_shares(nitems, gabatch::rng_threads(c->bk.rng_threads, nitems),[&](int64_t first, int64_t stride) {
            for (int64_t t = first; t < nitems; t += stride) {
                const ga_batch_item& it = plan.kernel[(size_t)t];
                const size_t k = (size_t)it.out;
                const int32_t* wr = reinterpret_cast<const int32_t*>(&walked[2 * k]);
                cost_out[k] = got[k];
                gabatch::decode_walk(it, wr, ops.data() + plan.walk[(size_t)t].ops_off, it.out, got[k] == INT64_MIN, out);
            }
        });
        c->batch_align_ms[2] = (float)(now_ms() - t_dec);
        double fill_ticks = 0, walk_ticks = 0, steps = 0, cells = 0;
        for (const ga_batch_item& it : plan.kernel) {
            const size_t k = (size_t)it.out;
            if (int r = check_decoded(out_len[k], (int64_t)k, "work item does not fit the batch launch")) return r;
            fill_ticks += walked[2 * k + 1].x;
            walk_ticks += walked[2 * k + 1].y;
            steps += walked[2 * k].x;
            cells += (double)it.m * it.n;
        }
        c->batch_align_ms[4] = (float)(10.0 * walk_ticks / std::max(steps, 1.0));  // (a tick is 10 ns)
        c->batch_align_ms[5] = (float)(10.0 * fill_ticks / std::max(cells, 1.0));
        return GA_OK;
    };
    if (!plan.kernel.empty()) {
        bool fell_back = false;
        if (int r = kernel_pairs(rng_route(c, flags), fell_back)) return r;
        if (fell_back) {
            // through the host route; the figures of the device attempt stay in ga_batch_align_info
            const float tables_ms = c->batch_align_ms[1];
            const int32_t first_try[4] = {c->batch_rng_info[0], c->batch_rng_info[1], 1, c->batch_rng_info[3]};
            if (int r = kernel_pairs(rng_route(c, GA_BATCH_TABLES_HOST), fell_back)) return r;
            c->batch_align_ms[1] += tables_ms;
            for (int q = 0; q < 4; q++) c->batch_rng_info[q] = first_try[q];
        }
    }
    if (!plan.single.empty()) {
        // the single-pair path, one pair at a time, from that pair's seeded state (the state it leaves is dropped).
        // It goes through the context's problem slot, so no problem is loaded afterwards.
        c->rc_used = false;
        for (const int64_t k : plan.single)
            if (int r = batch_single_align(c, codes, seq_off, pair_a, pair_b, pair_max_cost, cs, k, k, seeds, out,
                                           cost_out))
                return r;
    }
    c->batch_align_ms[3] = (float)(now_ms() - t_call);
    return GA_OK;
}

// ga_batch_sample: every pair filled once, then walked once per sample.  Kernel pairs go chunk by
// chunk through the stored-words fill and, walk launch by walk launch, through batch_walks_kernel; a pair on the large
// route is walked by the same kernel in the fill's layout; what remains is looped sample by sample through
// ga_problem_align.
static int batch_sample_impl(ga_ctx* c, const BatchIn& in, const int64_t* sample_off, const uint64_t* seeds,
                             const char* chars, char* out_a, char* out_mid, char* out_b, const int64_t* out_off,
                             int64_t* out_len, int32_t* tb_status, int64_t* cost_out, uint32_t flags) {
    if (int r = check_ctx(c)) return r;
    if (int r = check_table_flags(flags)) return r;
    for (int64_t& x : c->batch_sample_info) x = 0;
    for (float& x : c->batch_sample_ms) x = 0.f;
    if (in.npairs == 0) return GA_OK;  // an empty batch: no launch
    if (!sample_off || !seeds || !chars || !out_a || !out_mid || !out_b || !out_off || !out_len || !tb_status || !cost_out)
        return fail(GA_E_ARG, "null argument");
    const double t_call = now_ms();
    const gabatch::WordsLimits lim = words_limits(c);
    gabatch::SamplePlan plan;
    std::string why;
    if (int r = gabatch::plan_batch_sample(in.codes, in.seq_off, in.nseq, in.pair_a, in.pair_b, in.pair_max_cost, in.npairs,
                                           in.cs, sample_off, lim, plan, why))
        return fail(r, why);
    for (int64_t k = 0; k < in.npairs; k++)
        if (int r = check_out_capacity(in.seq_off, in.pair_a, in.pair_b, k, out_off, sample_off[k], sample_off[k + 1]))
            return r;
    if (int r = refuse_slab_single(c, plan.single, "path")) return r;
    const gabatch::WalkOut out{chars, out_a, out_mid, out_b, out_off, out_len, tb_status};
    const size_t ncodes = (size_t)in.seq_off[in.nseq];
    double walk_ticks = 0, walk_steps = 0;

    // The walk launches `launches` over `witems` (both counted from 0 here) of the filled pairs; bt_codes holds the
    // batch's codes.  Tables by the call's route; a walk launch whose generator reached a word cap runs again with host
    // tables (the fill stays).  Then the copies back and the strings.
    auto run_walks = [&](const Filled& f, const ga_batch_sample_item* witems, const gabatch::WalkLaunch* launches,
                         int64_t nlaunch) -> int {
        for (int64_t L = 0; L < nlaunch; L++) {
            const gabatch::WalkLaunch& wl = launches[L];
            const ga_batch_sample_item* wi = witems + wl.first;
            const int64_t nw = wl.count;
            HIPCHK(c->bs_witems.ensure(sizeof(ga_batch_sample_item) * nw));
            HIPCHK(c->bs_ticket.ensure(sizeof(unsigned)));
            HIPCHK(c->bt_walk.ensure(sizeof(int4) * 2 * nw));
            HIPCHK(c->bt_rng.ensure(sizeof(uint32_t) * wl.tab_entries));
            HIPCHK(c->bt_ops.ensure(sizeof(uint32_t) * wl.ops_words));
            HIPCHK(hipMemcpyAsync(c->bs_witems.p, wi, sizeof(ga_batch_sample_item) * nw, hipMemcpyHostToDevice, c->stream));
            const int waves = launch_waves(c, nw);
            std::vector<int4> walked((size_t)nw * 2);
            std::vector<uint32_t> ops((size_t)wl.ops_words);
            // every walk's table from its own seed
            std::vector<gabrng::Item> jobs;
            jobs.reserve((size_t)nw);
            for (int64_t t = 0; t < nw; t++) {
                const ga_batch_item& it = f.items[(size_t)wi[t].fill];
                jobs.push_back(gabrng::Item{seeds[wi[t].out], wi[t].tab_off, it.m + it.n, 0});
            }
            RngRoute route = rng_route(c, flags);
            for (int attempt = 0;; attempt++) {
                TableStage ts;
                if (int r = tables_enqueue(c, jobs, wl.tab_entries, route, ts)) return r;
                c->batch_sample_info[6] += (int64_t)ts.split.dev.size();
                c->batch_sample_info[7] += (int64_t)ts.split.host.size();
                // the walks' ticket starts at zero for every launch
                HIPCHK(hipMemsetAsync(c->bs_ticket.p, 0, sizeof(unsigned), c->stream));
                HIPCHK(hipEventRecord(c->wev[0], c->stream));
                const ga::WalksArgs q{c->bt_codes.as<uint8_t>(), (long long)ncodes, in.cs->gap_open, f.items_dev,
                                      f.words_dev, (int)f.items.size(), c->bs_witems.as<ga_batch_sample_item>(), (int)nw,
                                      c->bs_ticket.as<unsigned>(), c->bt_rng.as<uint32_t>(), (long long)wl.tab_entries,
                                      c->bt_ops.as<uint32_t>(), (long long)wl.ops_words, c->bt_walk.as<int4>(), f.tb,
                                      (long long)f.tb_words, f.tc};
                ga::launch_batch_walks(c->stream, q, f.CB, f.layout, waves);
                HIPCHK(hipGetLastError());
                HIPCHK(hipEventRecord(c->wev[1], c->stream));
                c->batch_sample_info[5]++;
                HIPCHK(hipMemcpyAsync(walked.data(), c->bt_walk.p, sizeof(int4) * 2 * nw, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(hipMemcpyAsync(ops.data(), c->bt_ops.p, sizeof(uint32_t) * ops.size(), hipMemcpyDeviceToHost,
                                      c->stream));
                if (int r = tables_read_back(c, ts)) return r;
                HIPCHK(hipStreamSynchronize(c->stream));
                float walk_ms = 0.f;
                HIPCHK(hipEventElapsedTime(&walk_ms, c->wev[0], c->wev[1]));
                c->batch_sample_ms[1] += walk_ms;
                if (int r = tables_finish(c, ts)) return r;
                c->batch_sample_ms[2] += ts.ms;
                if (!ts.capped) break;  // (else it runs again with host tables)
                if (attempt > 0) return fail(GA_E_STATE, "the host tables' walk launch reports a generator status");
                route = rng_route(c, GA_BATCH_TABLES_HOST);
            }
            const double t_dec = now_ms();
            gabatch::run_shares(nw, gabatch::rng_threads(c->bk.rng_threads, nw), [&](int64_t first, int64_t stride) {
                for (int64_t t = first; t < nw; t += stride) {
                    const int32_t* wr = reinterpret_cast<const int32_t*>(&walked[2 * (size_t)t]);
                    gabatch::decode_walk(f.items[(size_t)wi[t].fill], wr, ops.data() + wi[t].ops_off, wi[t].out, wr[0] < 0,
                                         out);
                }
            });
            c->batch_sample_ms[3] += (float)(now_ms() - t_dec);
            for (int64_t t = 0; t < nw; t++) {
                // (batch_single_pair names the pair of a large-route walk itself)
                const int64_t k = f.layout == gabatch::LAYOUT_BATCH ? f.items[(size_t)wi[t].fill].out : -1;
                if (int r = check_decoded(out_len[wi[t].out], k, "walk item does not fit the batch launch")) return r;
                walk_ticks += walked[2 * (size_t)t + 1].y;
                walk_steps += walked[2 * (size_t)t].x;
            }
            c->batch_sample_info[3] += nw;
        }
        return GA_OK;
    };

    // the kernel pairs, fill chunk by fill chunk
    for (const gabatch::FillChunk& ch : plan.chunks) {
        ChunkFill cf;
        if (int r = enqueue_chunk_fill(c, in, plan, ch, {}, {}, "no device memory for the batch's traceback words", cf))
            return r;
        c->batch_sample_info[4]++;
        if (int r = finish_chunk_fill(c, in, cf, c->batch_sample_ms[0], cost_out)) return r;
        c->batch_sample_info[0] += ch.count;
        if (int r = run_walks(cf.f, plan.walk.data(), plan.launches.data() + ch.launch_first, ch.launch_count)) return r;
    }

    for (const int64_t k : plan.single) {
        bool filled = false;
        if (std::min(in.m(k), in.n(k)) >= 2) {
            // the large route where the words fit band_rows' budget: the pair's samples walk c->fb.tb
            auto walk_it = [&](const Filled& f) -> int {
                std::vector<ga_batch_sample_item> walk;
                std::vector<gabatch::WalkLaunch> launches;
                gabatch::plan_walk_launches(f.items.data(), 1, sample_off, lim.walk_entries, walk, launches);
                c->batch_sample_info[1]++;
                c->batch_sample_info[4]++;
                return run_walks(f, walk.data(), launches.data(), (int64_t)launches.size());
            };
            if (int r = large_route(c, in, k, nullptr, true, c->batch_sample_ms[6], cost_out, filled, walk_it)) return r;
        }
        if (filled) continue;
        // a one-letter sequence (only such a pair can raise the reference's IndexError or take its first-step
        // quirk), or words beyond the budget: sample by sample through the single-pair path, each from its seeded
        // state (the state it leaves is dropped)
        c->rc_used = false;
        for (int64_t f = sample_off[k]; f < sample_off[k + 1]; f++)
            if (int r = batch_single_align(c, in.codes, in.seq_off, in.pair_a, in.pair_b, in.pair_max_cost, in.cs, k, f, seeds,
                                           out, cost_out))
                return r;
        c->batch_sample_info[2]++;
    }
    c->batch_sample_ms[4] = (float)(now_ms() - t_call);
    c->batch_sample_ms[5] = (float)(10.0 * walk_ticks / std::max(walk_steps, 1.0));  // (a tick is 10 ns)
    return GA_OK;
}

// ga_batch_count: every pair filled by the stored-words fill, then counted by batch_count_kernel from
// the words the fill left, one wave per pair.  No table stage, no RNG and no decode.
static int batch_count_impl(ga_ctx* c, const BatchIn& in, int64_t* cost_out, double* count_out) {
    if (int r = check_ctx(c)) return r;
    for (int64_t& x : c->batch_count_info) x = 0;
    for (float& x : c->batch_count_ms) x = 0.f;
    if (in.npairs == 0) return GA_OK;  // an empty batch: no launch
    if (!cost_out || !count_out) return fail(GA_E_ARG, "null argument");
    const double t_call = now_ms();
    const int64_t npairs = in.npairs;
    const int W = gabatch::kWavesPerGroup;
    const gabatch::WordsLimits lim = words_limits(c);
    gabatch::CountPlan plan;
    std::string why;
    if (int r = gabatch::plan_batch_count(in.codes, in.seq_off, in.nseq, in.pair_a, in.pair_b, in.pair_max_cost, npairs,
                                          in.cs, lim, plan, why))
        return fail(r, why);
    if (int r = check_single_pairs(c, in, plan, "count needs", "counting")) return r;
    if (int r = refuse_slab_single(c, plan.single, "fill")) return r;
    HIPCHK(c->bc_out.ensure(sizeof(double) * npairs));
    HIPCHK(c->bc_ticket.ensure(sizeof(unsigned)));

    // The count launch over the filled pairs, behind the fill on the context's stream and between the events c->wev;
    // edge_rows: the HBM edge rows a wave needs (0: none).
    auto enqueue_count = [&](const Filled& f, int waves, int64_t edge_rows) -> int {
        if (edge_rows > 0) HIPCHK(c->bc_scratch.ensure(sizeof(double2) * 2 * (size_t)edge_rows * waves));
        // the count's ticket starts at zero for every launch
        HIPCHK(hipMemsetAsync(c->bc_ticket.p, 0, sizeof(unsigned), c->stream));
        HIPCHK(hipEventRecord(c->wev[0], c->stream));
        const ga::CountArgs q{in.cs->gap_open, f.items_dev, f.words_dev, (int)f.items.size(), c->bc_ticket.as<unsigned>(),
                              c->bc_out.as<double>(), (long long)npairs, f.tb, (long long)f.tb_words, f.tc,
                              edge_rows > 0 ? c->bc_scratch.as<double2>() : nullptr, (long long)edge_rows};
        ga::launch_batch_count(c->stream, q, f.CB, f.layout, waves);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->wev[1], c->stream));
        c->batch_count_info[4]++;
        return GA_OK;
    };
    // a launch's count of pair k and the launch's time (pair: the pair the message names, pair_prefix)
    auto take_count = [&](double got, int64_t k, int64_t pair) -> int {
        if (!(got >= 1.0)) return fail(GA_E_STATE, pair_prefix(pair) + "work item does not fit the count launch");
        count_out[k] = got;
        return GA_OK;
    };

    // the kernel pairs, fill chunk by fill chunk
    for (const gabatch::FillChunk& ch : plan.chunks) {
        ChunkFill cf;
        if (int r = enqueue_chunk_fill(c, in, plan, ch, {}, {}, "no device memory for the batch's traceback words", cf))
            return r;
        c->batch_count_info[3]++;
        if (int r = enqueue_count(cf.f, cf.bs.waves, plan.count_rows)) return r;
        std::vector<double> cnt((size_t)npairs);
        HIPCHK(hipMemcpyAsync(cnt.data(), c->bc_out.p, sizeof(double) * npairs, hipMemcpyDeviceToHost, c->stream));
        if (int r = finish_chunk_fill(c, in, cf, c->batch_count_ms[0], cost_out)) return r;
        float count_ms = 0.f;
        HIPCHK(hipEventElapsedTime(&count_ms, c->wev[0], c->wev[1]));
        c->batch_count_ms[1] += count_ms;
        for (const ga_batch_item& it : cf.f.items) {
            if (int r = take_count(cnt[(size_t)it.out], it.out, it.out)) return r;
            c->batch_count_info[5] += gabatch::needs_scratch(it.m, it.n);
        }
        c->batch_count_info[0] += ch.count;
        c->batch_count_info[2]++;
    }

    // the large route: one wave counts c->fb.tb
    for (const int64_t k : plan.single) {
        auto count_it = [&](const Filled& f) -> int {
            const int64_t m = f.items[0].m;
            const bool hbm = gabatch::needs_scratch(m, f.items[0].n);
            c->batch_count_info[3]++;
            if (int r = enqueue_count(f, W, hbm ? m : 0)) return r;
            double got = 0.0;
            HIPCHK(hipMemcpyAsync(&got, c->bc_out.as<double>() + k, sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            float count_ms = 0.f;
            HIPCHK(hipEventElapsedTime(&count_ms, c->wev[0], c->wev[1]));
            c->batch_count_ms[3] += count_ms;
            c->batch_count_info[1]++;
            c->batch_count_info[5] += hbm;
            return take_count(got, k, -1);
        };
        bool filled;
        if (int r = large_route(c, in, k, "counting", false, c->batch_count_ms[2], cost_out, filled, count_it)) return r;
    }
    c->batch_count_ms[4] = (float)(now_ms() - t_call);
    return GA_OK;
}

// ga_batch_rank: every pair filled by the stored-words fill; batch_rank_table_kernel then keeps the
// saturating u64 path counts of every cell in the pair's table, and batch_rank_walk_kernel walks the pair once per
// requested rank, one lane per walk, reading the counts only at ties.  No table stage and no RNG; the strings come
// from the walks' levels through decode_walk, as ga_batch_sample's.
static int batch_rank_impl(ga_ctx* c, const BatchIn& in, const int64_t* rank_off, const uint64_t* ranks, const char* chars,
                           char* out_a, char* out_mid, char* out_b, const int64_t* out_off, int64_t* out_len,
                           int32_t* rank_status, int64_t* cost_out, uint64_t* count_out) {
    if (int r = check_ctx(c)) return r;
    for (int64_t& x : c->batch_rank_info) x = 0;
    for (float& x : c->batch_rank_ms) x = 0.f;
    if (in.npairs == 0) return GA_OK;  // an empty batch: no launch
    if (!rank_off || !cost_out || !count_out) return fail(GA_E_ARG, "null argument");
    const double t_call = now_ms();
    const int64_t npairs = in.npairs;
    const int W = gabatch::kWavesPerGroup;
    const gabatch::WordsLimits lim = words_limits(c);
    gabatch::RankPlan plan;
    std::string why;
    if (int r = gabatch::plan_batch_rank(in.codes, in.seq_off, in.nseq, in.pair_a, in.pair_b, in.pair_max_cost, npairs,
                                         in.cs, rank_off, lim, plan, why))
        return fail(r, why);
    const int64_t nslots = rank_off[npairs];
    if (nslots > 0 && (!ranks || !chars || !out_a || !out_mid || !out_b || !out_off || !out_len || !rank_status))
        return fail(GA_E_ARG, "null argument");
    if (int r = check_single_pairs(c, in, plan, "ranks need", "ranking")) return r;
    for (int64_t k = 0; k < npairs; k++)
        if (int r = check_out_capacity(in.seq_off, in.pair_a, in.pair_b, k, out_off, rank_off[k], rank_off[k + 1])) return r;
    if (int r = refuse_slab_single(c, plan.single, "fill")) return r;
    const gabatch::WalkOut out{chars, out_a, out_mid, out_b, out_off, out_len, rank_status};
    HIPCHK(c->br_out.ensure(sizeof(uint64_t) * npairs));
    HIPCHK(c->br_ticket.ensure(sizeof(unsigned)));
    HIPCHK(c->br_ranks.ensure(sizeof(uint64_t) * std::max<int64_t>(nslots, 1)));
    if (nslots > 0)
        HIPCHK(hipMemcpyAsync(c->br_ranks.p, ranks, sizeof(uint64_t) * nslots, hipMemcpyHostToDevice, c->stream));
    double walk_ticks = 0, walk_steps = 0;

    // The table launch over the filled pairs, their tables' places in br_toff and their tables in br_table
    // (table_entries u64s), behind the fill on the context's stream and between the events c->wev; edge_rows: the HBM
    // edge rows a wave needs (0: none).
    auto enqueue_table = [&](const Filled& f, int64_t table_entries, int waves, int64_t edge_rows) -> int {
        if (edge_rows > 0) HIPCHK(c->bc_scratch.ensure(sizeof(ulonglong2) * 2 * (size_t)edge_rows * waves));
        // the ticket starts at zero for every launch
        HIPCHK(hipMemsetAsync(c->br_ticket.p, 0, sizeof(unsigned), c->stream));
        HIPCHK(hipEventRecord(c->wev[0], c->stream));
        const ga::RankTableArgs q{in.cs->gap_open, f.items_dev, f.words_dev, c->br_toff.as<int64_t>(), (int)f.items.size(),
                                  c->br_ticket.as<unsigned>(), c->br_out.as<unsigned long long>(), (long long)npairs, f.tb,
                                  (long long)f.tb_words, f.tc, c->br_table.as<unsigned long long>(),
                                  (long long)table_entries, edge_rows > 0 ? c->bc_scratch.as<ulonglong2>() : nullptr,
                                  (long long)edge_rows};
        ga::launch_batch_rank_table(c->stream, q, f.CB, f.layout, waves);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->wev[1], c->stream));
        c->batch_rank_info[4]++;
        return GA_OK;
    };
    // pair: the pair the message names (pair_prefix)
    auto take_count = [&](uint64_t got, int64_t k, int64_t pair) -> int {
        if (got == 0) return fail(GA_E_STATE, pair_prefix(pair) + "work item does not fit the table launch");
        count_out[k] = got;
        c->batch_rank_info[7] += got == gabatch::kRankCap;
        return GA_OK;
    };
    // The walk launches `launches` over `witems` (both counted from 0 here) of the filled pairs, each behind what is on
    // the stream; then the copies back and the strings.
    auto run_walks = [&](const Filled& f, int64_t table_entries, const ga_batch_rank_item* witems,
                         const gabatch::RankLaunch* launches, int64_t nlaunch) -> int {
        for (int64_t L = 0; L < nlaunch; L++) {
            const gabatch::RankLaunch& wl = launches[L];
            const ga_batch_rank_item* wi = witems + wl.first;
            const int64_t nw = wl.count;
            HIPCHK(c->br_items.ensure(sizeof(ga_batch_rank_item) * nw));
            HIPCHK(c->bt_walk.ensure(sizeof(int4) * 2 * wl.slots));
            HIPCHK(c->bt_ops.ensure(sizeof(uint32_t) * wl.ops_words));
            HIPCHK(hipMemcpyAsync(c->br_items.p, wi, sizeof(ga_batch_rank_item) * nw, hipMemcpyHostToDevice, c->stream));
            // a slot no item reports to keeps status -1; the ticket starts at zero for every launch
            HIPCHK(hipMemsetAsync(c->bt_walk.p, 0xff, sizeof(int4) * 2 * wl.slots, c->stream));
            HIPCHK(hipMemsetAsync(c->br_ticket.p, 0, sizeof(unsigned), c->stream));
            const int waves = launch_waves(c, nw);
            std::vector<int4> walked((size_t)wl.slots * 2);
            std::vector<uint32_t> ops((size_t)wl.ops_words);
            HIPCHK(hipEventRecord(c->rev[0], c->stream));
            const ga::RankWalkArgs q{in.cs->gap_open, f.items_dev, f.words_dev, c->br_toff.as<int64_t>(), (int)f.items.size(),
                                     c->br_items.as<ga_batch_rank_item>(), (int)nw, c->br_ticket.as<unsigned>(),
                                     c->br_ranks.as<unsigned long long>(), (long long)nslots, c->bt_ops.as<uint32_t>(),
                                     (long long)wl.ops_words, c->bt_walk.as<int4>(), (long long)wl.slots, f.tb,
                                     (long long)f.tb_words, f.tc, c->br_table.as<unsigned long long>(),
                                     (long long)table_entries};
            ga::launch_batch_rank_walk(c->stream, q, f.CB, f.layout, waves);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(c->rev[1], c->stream));
            c->batch_rank_info[5]++;
            HIPCHK(hipMemcpyAsync(walked.data(), c->bt_walk.p, sizeof(int4) * 2 * wl.slots, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(ops.data(), c->bt_ops.p, sizeof(uint32_t) * ops.size(), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            float walk_ms = 0.f;
            HIPCHK(hipEventElapsedTime(&walk_ms, c->rev[0], c->rev[1]));
            c->batch_rank_ms[2] += walk_ms;
            const double t_dec = now_ms();
            gabatch::run_shares(nw, gabatch::rng_threads(c->bk.rng_threads, nw), [&](int64_t first, int64_t stride) {
                for (int64_t t = first; t < nw; t += stride) {
                    const ga_batch_item& it = f.items[(size_t)wi[t].fill];
                    const int64_t wps = ((int64_t)it.m + it.n + 15) / 16;
                    for (int64_t l = 0; l < wi[t].nslots; l++) {
                        const int32_t* wr = reinterpret_cast<const int32_t*>(&walked[2 * (size_t)(wi[t].res + l)]);
                        const int64_t slot = wi[t].out + l;
                        if (wr[4] == gabatch::kRankOutOfRange) {
                            rank_status[slot] = 1;
                            out_len[slot] = 0;
                        } else {
                            gabatch::decode_walk(it, wr, ops.data() + wi[t].ops_off + l * wps, slot,
                                                 wr[4] != gabatch::kRankOk, out);
                        }
                    }
                }
            });
            c->batch_rank_ms[3] += (float)(now_ms() - t_dec);
            for (int64_t t = 0; t < nw; t++) {
                // (batch_single_pair names the pair of a large-route walk itself)
                const int64_t k = f.layout == gabatch::LAYOUT_BATCH ? f.items[(size_t)wi[t].fill].out : -1;
                for (int64_t l = 0; l < wi[t].nslots; l++) {
                    if (int r = check_decoded(out_len[wi[t].out + l], k, "walk item does not fit the walk launch")) return r;
                    walk_steps += walked[2 * (size_t)(wi[t].res + l)].x;
                }
                walk_ticks += walked[2 * (size_t)wi[t].res + 1].y;
            }
            c->batch_rank_info[6] += wl.slots;
        }
        return GA_OK;
    };
    if (int r = ensure_rev(c)) return r;

    // the kernel pairs, fill chunk by fill chunk
    for (size_t ci = 0; ci < plan.chunks.size(); ci++) {
        const gabatch::FillChunk& ch = plan.chunks[ci];
        const int64_t entries = plan.chunk_table[ci];
        ChunkFill cf;
        if (int r = enqueue_chunk_fill(c, in, plan, ch,
                                       {{&c->br_toff, plan.table_off.data() + ch.first, sizeof(int64_t) * (size_t)ch.count}},
                                       {{&c->br_table, sizeof(uint64_t) * (size_t)entries}},
                                       "no device memory for the batch's traceback words and count tables", cf))
            return r;
        c->batch_rank_info[3]++;
        if (int r = enqueue_table(cf.f, entries, cf.bs.waves, plan.count_rows)) return r;
        std::vector<uint64_t> cnt((size_t)npairs);
        HIPCHK(hipMemcpyAsync(cnt.data(), c->br_out.p, sizeof(uint64_t) * npairs, hipMemcpyDeviceToHost, c->stream));
        if (int r = finish_chunk_fill(c, in, cf, c->batch_rank_ms[0], cost_out)) return r;
        float table_ms = 0.f;
        HIPCHK(hipEventElapsedTime(&table_ms, c->wev[0], c->wev[1]));
        c->batch_rank_ms[1] += table_ms;
        for (const ga_batch_item& it : cf.f.items)
            if (int r = take_count(cnt[(size_t)it.out], it.out, it.out)) return r;
        c->batch_rank_info[0] += ch.count;
        c->batch_rank_info[2]++;
        if (int r = run_walks(cf.f, entries, plan.walk.data(), plan.launches.data() + ch.launch_first, ch.launch_count))
            return r;
    }

    // the large route: one wave makes the pair's table from c->fb.tb and its slots walk it
    for (const int64_t k : plan.single) {
        auto rank_it = [&](const Filled& f) -> int {
            const ga_batch_item& it = f.items[0];
            const int64_t toff = 0, entries = gabatch::rank_table_entries(it.m, it.T, it.nstripes);
            c->batch_rank_info[3]++;
            std::vector<ga_batch_rank_item> walk;
            std::vector<gabatch::RankLaunch> launches;
            gabatch::plan_rank_launches(&it, 1, rank_off, lim.walk_entries, walk, launches);
            HIPCHK(c->br_toff.ensure(sizeof(int64_t)));
            if (c->br_table.ensure(sizeof(uint64_t) * (size_t)entries) != hipSuccess) {
                (void)hipStreamSynchronize(c->stream);  // the staged uploads read this pair's work list
                return fail(GA_E_NOMEM, "no device memory for the pair's count table");
            }
            HIPCHK(hipMemcpyAsync(c->br_toff.p, &toff, sizeof(toff), hipMemcpyHostToDevice, c->stream));
            if (int r = enqueue_table(f, entries, W, gabatch::needs_scratch(it.m, it.n) ? it.m : 0)) return r;
            uint64_t got = 0;
            HIPCHK(hipMemcpyAsync(&got, c->br_out.as<uint64_t>() + k, sizeof(got), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            float table_ms = 0.f;
            HIPCHK(hipEventElapsedTime(&table_ms, c->wev[0], c->wev[1]));
            c->batch_rank_ms[7] += table_ms;
            c->batch_rank_info[1]++;
            if (int r = take_count(got, k, -1)) return r;
            return run_walks(f, entries, walk.data(), launches.data(), (int64_t)launches.size());
        };
        bool filled;
        if (int r = large_route(c, in, k, "ranking", false, c->batch_rank_ms[6], cost_out, filled, rank_it)) return r;
    }
    c->batch_rank_ms[4] = (float)(now_ms() - t_call);
    c->batch_rank_ms[5] = (float)(10.0 * walk_ticks / std::max(walk_steps, 1.0));  // (a tick is 10 ns)
    return GA_OK;
}

// ga_batch_support: every pair filled by the stored-words fill; batch_support_table_kernel keeps the
// doubles N(i, j, 0) in the pair's table, batch_flow_kernel runs the wavefront backwards and leaves support(i, j)
// there, batch_support_gather_kernel makes the pair's dense rows, and one copy a chunk brings costs, counts and
// supports back.  No table stage, no RNG and no decode.
static int batch_support_impl(ga_ctx* c, const BatchIn& in, const int64_t* support_off, double* support_out,
                              int64_t* cost_out, double* count_out) {
    if (int r = check_ctx(c)) return r;
    for (int64_t& x : c->batch_support_info) x = 0;
    for (float& x : c->batch_support_ms) x = 0.f;
    if (in.npairs == 0) return GA_OK;  // an empty batch: no launch
    if (!support_off || !support_out || !cost_out || !count_out) return fail(GA_E_ARG, "null argument");
    const int64_t npairs = in.npairs;
    const int W = gabatch::kWavesPerGroup;
    const gabatch::WordsLimits lim = words_limits(c);
    gabatch::SupportPlan plan;
    std::string why;
    if (int r = gabatch::plan_batch_support(in.codes, in.seq_off, in.nseq, in.pair_a, in.pair_b, in.pair_max_cost, npairs,
                                            in.cs, lim, plan, why))
        return fail(r, why);
    if (int r = check_single_pairs(c, in, plan, "support needs", "support")) return r;
    if (support_off[0] != 0) return fail(GA_E_ARG, "support_off must start at 0");
    for (int64_t k = 0; k < npairs; k++)
        if (support_off[k + 1] - support_off[k] < in.m(k) * in.n(k))
            return fail(GA_E_ARG, pair_prefix(k) + "support_off leaves fewer than m * n doubles");
    if (int r = refuse_slab_single(c, plan.single, "fill")) return r;
    HIPCHK(c->bm_count.ensure(sizeof(double) * npairs));
    HIPCHK(c->bm_ticket.ensure(sizeof(unsigned) * 2));

    // The N-table, flow and gather launches over the filled pairs, their places in bm_toff and bm_ooff, their tables in
    // bm_table (table_entries), their dense rows in bm_out (support_entries; max_cells: the largest pair's), behind the
    // fill on the context's stream, with the events c->wev[0], c->wev[1], c->rev[0] and c->rev[1] around them;
    // edge_rows: the HBM edge rows a wave needs (0: none).
    auto enqueue_support = [&](const Filled& f, int64_t table_entries, int64_t support_entries, int64_t max_cells, int waves,
                               int64_t edge_rows) -> int {
        if (edge_rows > 0) HIPCHK(c->bc_scratch.ensure(sizeof(double2) * 2 * (size_t)edge_rows * waves));
        // both tickets start at zero for every chunk
        HIPCHK(hipMemsetAsync(c->bm_ticket.p, 0, sizeof(unsigned) * 2, c->stream));
        ga::SupportArgs q{in.cs->gap_open, f.items_dev, f.words_dev, c->bm_toff.as<int64_t>(), c->bm_ooff.as<int64_t>(),
                          (int)f.items.size(), c->bm_ticket.as<unsigned>(), c->bm_count.as<double>(), (long long)npairs, f.tb,
                          (long long)f.tb_words, f.tc, c->bm_table.as<unsigned long long>(), (long long)table_entries,
                          c->bm_out.as<double>(), (long long)support_entries,
                          edge_rows > 0 ? c->bc_scratch.as<double2>() : nullptr, (long long)edge_rows};
        HIPCHK(hipEventRecord(c->wev[0], c->stream));
        ga::launch_batch_support_table(c->stream, q, f.CB, f.layout, waves);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->wev[1], c->stream));
        q.ticket = c->bm_ticket.as<unsigned>() + 1;
        ga::launch_batch_flow(c->stream, q, f.CB, f.layout, waves);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->rev[0], c->stream));
        ga::launch_batch_support_gather(c->stream, q, f.CB, f.layout, max_cells);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->rev[1], c->stream));
        c->batch_support_info[4]++;
        return GA_OK;
    };
    // the three launches' times of the chunk just waited for, into slots `at` .. `at` + 2
    auto take_times = [&](int at) -> int {
        float ms[3] = {0.f, 0.f, 0.f};
        HIPCHK(hipEventElapsedTime(&ms[0], c->wev[0], c->wev[1]));
        HIPCHK(hipEventElapsedTime(&ms[1], c->wev[1], c->rev[0]));
        HIPCHK(hipEventElapsedTime(&ms[2], c->rev[0], c->rev[1]));
        for (int x = 0; x < 3; x++) c->batch_support_ms[at + x] += ms[x];
        return GA_OK;
    };
    // the lowest pair whose count is not finite: its supports would be 0 * inf
    int64_t not_finite = -1;
    // pair: the pair the message names (pair_prefix)
    auto take_count = [&](double got, int64_t k, int64_t pair) -> int {
        if (!(got >= 1.0)) return fail(GA_E_STATE, pair_prefix(pair) + "work item does not fit the support launches");
        count_out[k] = got;
        if (!std::isfinite(got) && (not_finite < 0 || k < not_finite)) not_finite = k;
        return GA_OK;
    };
    if (int r = ensure_rev(c)) return r;

    // the kernel pairs, fill chunk by fill chunk
    for (size_t ci = 0; ci < plan.chunks.size(); ci++) {
        const gabatch::FillChunk& ch = plan.chunks[ci];
        const size_t each = sizeof(int64_t) * (size_t)ch.count;
        ChunkFill cf;
        if (int r = enqueue_chunk_fill(c, in, plan, ch,
                                       {{&c->bm_toff, plan.table_off.data() + ch.first, each},
                                        {&c->bm_ooff, plan.support_off.data() + ch.first, each}},
                                       {{&c->bm_table, sizeof(uint64_t) * (size_t)plan.chunk_table[ci]},
                                        {&c->bm_out, sizeof(double) * (size_t)plan.chunk_support[ci]}},
                                       "no device memory for the batch's traceback words, tables and supports", cf))
            return r;
        c->batch_support_info[3]++;
        const std::vector<ga_batch_item>& items = cf.f.items;
        // (the work list is sorted by cells, largest first)
        if (int r = enqueue_support(cf.f, plan.chunk_table[ci], plan.chunk_support[ci], (int64_t)items[0].m * items[0].n,
                                    cf.bs.waves, plan.count_rows))
            return r;
        std::vector<double> cnt((size_t)npairs), dense((size_t)plan.chunk_support[ci]);
        HIPCHK(hipMemcpyAsync(cnt.data(), c->bm_count.p, sizeof(double) * npairs, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(dense.data(), c->bm_out.p, sizeof(double) * dense.size(), hipMemcpyDeviceToHost, c->stream));
        if (int r = finish_chunk_fill(c, in, cf, c->batch_support_ms[0], cost_out)) return r;
        if (int r = take_times(1)) return r;
        for (size_t t = 0; t < items.size(); t++) {
            const ga_batch_item& it = items[t];
            if (int r = take_count(cnt[(size_t)it.out], it.out, it.out)) return r;
            std::copy_n(dense.data() + plan.support_off[(size_t)ch.first + t], (size_t)it.m * (size_t)it.n,
                        support_out + support_off[it.out]);
            c->batch_support_info[5] += gabatch::needs_scratch(it.m, it.n);
        }
        c->batch_support_info[0] += ch.count;
        c->batch_support_info[2]++;
    }

    // the large route: one wave makes the pair's table and its flow from c->fb.tb
    for (const int64_t k : plan.single) {
        auto support_it = [&](const Filled& f) -> int {
            const ga_batch_item& it = f.items[0];
            const int64_t m = it.m, n = it.n, zero = 0, entries = gabatch::rank_table_entries(m, it.T, it.nstripes);
            c->batch_support_info[3]++;
            HIPCHK(c->bm_toff.ensure(sizeof(int64_t)));
            HIPCHK(c->bm_ooff.ensure(sizeof(int64_t)));
            if (c->bm_table.ensure(sizeof(uint64_t) * (size_t)entries) != hipSuccess ||
                c->bm_out.ensure(sizeof(double) * (size_t)(m * n)) != hipSuccess) {
                (void)hipStreamSynchronize(c->stream);  // the staged uploads read this pair's work list
                return fail(GA_E_NOMEM, "no device memory for the pair's table and supports");
            }
            HIPCHK(hipMemcpyAsync(c->bm_toff.p, &zero, sizeof(zero), hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(c->bm_ooff.p, &zero, sizeof(zero), hipMemcpyHostToDevice, c->stream));
            const bool hbm = gabatch::needs_scratch(m, n);
            if (int r = enqueue_support(f, entries, m * n, m * n, W, hbm ? m : 0)) return r;
            double got = 0.0;
            HIPCHK(hipMemcpyAsync(&got, c->bm_count.as<double>() + k, sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(support_out + support_off[k], c->bm_out.p, sizeof(double) * (size_t)(m * n),
                                  hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            if (int r = take_times(5)) return r;
            c->batch_support_info[1]++;
            c->batch_support_info[5] += hbm;
            return take_count(got, k, -1);
        };
        bool filled;
        if (int r = large_route(c, in, k, "support", false, c->batch_support_ms[4], cost_out, filled, support_it)) return r;
    }
    if (not_finite >= 0)
        return fail(GA_E_COUNT, pair_prefix(not_finite) + "the count of co-optimal alignments is not finite");
    return GA_OK;
}

int ga_batch_support_info(ga_ctx* c, int64_t* out8) { return copy_figures(c, &ga_ctx::batch_support_info, out8); }
int ga_batch_support_timings(ga_ctx* c, float* out8) { return copy_figures(c, &ga_ctx::batch_support_ms, out8); }
int ga_batch_rank_info(ga_ctx* c, int64_t* out8) { return copy_figures(c, &ga_ctx::batch_rank_info, out8); }
int ga_batch_rank_timings(ga_ctx* c, float* out8) { return copy_figures(c, &ga_ctx::batch_rank_ms, out8); }
int ga_batch_count_info(ga_ctx* c, int64_t* out8) { return copy_figures(c, &ga_ctx::batch_count_info, out8); }
int ga_batch_count_timings(ga_ctx* c, float* out8) { return copy_figures(c, &ga_ctx::batch_count_ms, out8); }
int ga_batch_sample_info(ga_ctx* c, int64_t* out8) { return copy_figures(c, &ga_ctx::batch_sample_info, out8); }
int ga_batch_sample_timings(ga_ctx* c, float* out8) { return copy_figures(c, &ga_ctx::batch_sample_ms, out8); }
int ga_batch_align_timings(ga_ctx* c, float* out6) { return copy_figures(c, &ga_ctx::batch_align_ms, out6); }
int ga_batch_align_info(ga_ctx* c, int32_t* out4) { return copy_figures(c, &ga_ctx::batch_rng_info, out4); }

static int debug_pair_tables_impl(ga_ctx* c, const uint64_t* seeds, const int32_t* steps, int64_t nitems, int32_t route,
                                  uint32_t* tab_out, int32_t* status_out) {
    if (int r = check_ctx(c)) return r;
    if (route != GA_BATCH_TABLES_HOST && route != GA_BATCH_TABLES_DEVICE)
        return fail(GA_E_ARG, "route must be 1 (host) or 2 (device)");
    if (nitems < 0 || (nitems > 0 && (!seeds || !steps || !tab_out || !status_out))) return fail(GA_E_ARG, "null argument");
    for (int32_t& x : c->batch_rng_info) x = 0;
    c->batch_align_ms[1] = 0.f;
    // On the device the items lie kGuard words apart, between guard words no entry equals (bits 0 and 31 are never
    // set in one): a write outside an item's range shows as status 2.
    constexpr int64_t kGuard = 4;
    constexpr uint32_t kGuardWord = 0xA5A5A5A5u;
    const RngRoute rt = rng_route(c, (uint32_t)route);
    // item t's entries go to tab_out at the sum of the steps before it: the jobs as the host builds them
    std::vector<gabrng::Item> jobs;
    jobs.reserve((size_t)nitems);
    int64_t entries = 0;
    for (int64_t t = 0; t < nitems; t++) {
        if (steps[t] < 0) return fail(GA_E_ARG, "item " + std::to_string(t) + ": negative steps");
        jobs.push_back(gabrng::Item{seeds[t], entries, steps[t], 0});
        entries += steps[t];
        status_out[t] = gabrng::kComplete;
    }
    const gabatch::TableSplit sp = gabatch::split_tables(jobs.data(), nitems, rt.want_device, rt.max_steps);
    std::vector<gabrng::Item> dev = sp.dev;  // the device jobs, moved to the guard-word layout
    std::vector<int32_t> rstatus;
    int groups = 0;
    int64_t dev_words = kGuard;
    for (gabrng::Item& d : dev) {
        d.tab_off = dev_words;
        dev_words += d.steps + kGuard;
    }
    std::vector<uint32_t> got;
    if (!dev.empty()) {
        got.resize((size_t)dev_words);
        HIPCHK(c->bt_rng.ensure(sizeof(uint32_t) * (size_t)dev_words));
        HIPCHK(hipMemsetAsync(c->bt_rng.p, 0xA5, sizeof(uint32_t) * (size_t)dev_words, c->stream));
        if (int r = enqueue_batch_rng(c, dev, c->bt_rng.as<uint32_t>(), rt.cap_words, &groups)) return r;
        HIPCHK(hipMemcpyAsync(got.data(), c->bt_rng.p, sizeof(uint32_t) * got.size(), hipMemcpyDeviceToHost, c->stream));
        if (int r = read_back_status(c, dev.size(), rstatus)) return r;
    }
    // the host's items meanwhile, one after the other
    gabatch::build_tables(sp.host.data(), (int64_t)sp.host.size(), 1, tab_out);
    if (!dev.empty()) {
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipEventElapsedTime(&c->batch_align_ms[1], c->rev[0], c->rev[1]));
        for (size_t q = 0; q < dev.size(); q++) {
            const int64_t t = sp.dev_at[q], off = dev[q].tab_off;
            std::copy(got.begin() + off, got.begin() + off + steps[t], tab_out + jobs[(size_t)t].tab_off);
            bool intact = true;
            for (int64_t g = 1; g <= kGuard; g++)
                intact &= got[(size_t)(off - g)] == kGuardWord && got[(size_t)(off + steps[t] + g - 1)] == kGuardWord;
            status_out[t] = intact ? rstatus[q] : 2;
        }
    }
    c->batch_rng_info[0] = (int32_t)dev.size();
    c->batch_rng_info[1] = (int32_t)sp.host.size();
    c->batch_rng_info[3] = groups;
    return GA_OK;
}

// the entries that run kernels and wait for them end with the guards' check (guard mode)
int ga_batch_costs_ex(ga_ctx* c, const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                      const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* cs,
                      int64_t* cost_out) {
    return guard_end(c, batch_costs_ex_impl(c, codes, seq_off, nseq, pair_a, pair_b, pair_max_cost, npairs, cs,
                                            cost_out));
}

int ga_batch_align_ex(ga_ctx* c, const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                      const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* cs,
                      const uint64_t* seeds, const char* chars, char* out_a, char* out_mid, char* out_b,
                      const int64_t* out_off, int64_t* out_len, int32_t* tb_status, int64_t* cost_out, uint32_t flags) {
    return guard_end(c, batch_align_ex_impl(c, codes, seq_off, nseq, pair_a, pair_b, pair_max_cost, npairs, cs, seeds,
                                            chars, out_a, out_mid, out_b, out_off, out_len, tb_status, cost_out,
                                            flags));
}

int ga_batch_sample(ga_ctx* c, const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                    const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* cs,
                    const int64_t* sample_off, const uint64_t* seeds, const char* chars, char* out_a, char* out_mid,
                    char* out_b, const int64_t* out_off, int64_t* out_len, int32_t* tb_status, int64_t* cost_out,
                    uint32_t flags) {
    const BatchIn in{codes, seq_off, nseq, pair_a, pair_b, pair_max_cost, npairs, cs};
    return guard_end(c, batch_sample_impl(c, in, sample_off, seeds, chars, out_a, out_mid, out_b, out_off, out_len, tb_status,
                                          cost_out, flags));
}

int ga_batch_count(ga_ctx* c, const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                   const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* cs,
                   int64_t* cost_out, double* count_out) {
    const BatchIn in{codes, seq_off, nseq, pair_a, pair_b, pair_max_cost, npairs, cs};
    return guard_end(c, batch_count_impl(c, in, cost_out, count_out));
}

int ga_batch_support(ga_ctx* c, const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                     const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* cs,
                     const int64_t* support_off, double* support_out, int64_t* cost_out, double* count_out) {
    const BatchIn in{codes, seq_off, nseq, pair_a, pair_b, pair_max_cost, npairs, cs};
    return guard_end(c, batch_support_impl(c, in, support_off, support_out, cost_out, count_out));
}

int ga_batch_rank(ga_ctx* c, const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                  const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* cs,
                  const int64_t* rank_off, const uint64_t* ranks, const char* chars, char* out_a, char* out_mid,
                  char* out_b, const int64_t* out_off, int64_t* out_len, int32_t* rank_status, int64_t* cost_out,
                  uint64_t* count_out) {
    const BatchIn in{codes, seq_off, nseq, pair_a, pair_b, pair_max_cost, npairs, cs};
    return guard_end(c, batch_rank_impl(c, in, rank_off, ranks, chars, out_a, out_mid, out_b, out_off, out_len, rank_status,
                                        cost_out, count_out));
}

int ga_debug_pair_tables(ga_ctx* c, const uint64_t* seeds, const int32_t* steps, int64_t nitems, int32_t route,
                         uint32_t* tab_out, int32_t* status_out) {
    return guard_end(c, debug_pair_tables_impl(c, seeds, steps, nitems, route, tab_out, status_out));
}

}  // extern "C"
