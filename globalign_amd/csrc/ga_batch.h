// ga_batch.h -- host-side planning of a batch of score-only alignments (ga_batch_costs) and of a batch of alignments
// with strings (ga_batch_align, at the end); no HIP: built into the engine, into the kernels' translation unit for the
// work-item layout, and into the planner self-tests, ga_batch_selftest.cpp, ga_batch_align_selftest.cpp,
// ga_batch_sample_selftest.cpp (ga_batch_sample's planner, after ga_batch_align's), ga_batch_count_selftest.cpp
// (ga_batch_count's, after that, and what the four stored-words calls share), ga_batch_rank_selftest.cpp
// (ga_batch_rank's, after that) and ga_batch_support_selftest.cpp (ga_batch_support's, at the end), under
// AddressSanitizer / UBSan.
//
// A batch is a list of sequences (codes concatenated, seq_off[s] .. seq_off[s + 1]) and a list of pairs of sequence
// indices.  The planner checks every pair as check_problem (ga_check.h) checks a single problem -- with that pair's
// own sentinel big = (max_cost + 1) * max(m, n) -- and turns the pairs into a work list for batch_fill_kernel
// (ga_batch.hip, one wave per pair), longest first, plus the pairs that go to the single-pair score fill instead.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ga_batch_layout.h"
#include "ga_batch_rank.h"
#include "ga_check.h"

// One pair as the kernel takes it (a wave reads it with one uniform 32-byte load).
struct ga_batch_item {
    int32_t a_off, m;    // seq_1: codes[a_off .. a_off + m)
    int32_t b_off, n;    // seq_2: codes[b_off .. b_off + n)
    int32_t big;         // this pair's sentinel (globaligner.py:777)
    int32_t out;         // index into the caller's pair list (the cost goes to cost_out[out])
    int32_t T, nstripes; // columns per lane; stripes of 64 * T columns, left to right in the same wave
};

// What batch_align_kernel needs per pair beyond its ga_batch_item (same index in the work list).
struct ga_batch_walk_item {
    int64_t tab_off;  // the pair's m + n tie-break entries in the launch's table
    int64_t ops_off;  // its ceil((m + n) / 16) u32 words of packed levels
};

namespace gabatch {

constexpr int kMaxT = 8;                    // widest stripe: 512 columns
constexpr int kLdsEdgeRows = 1024;          // rows of a wave's edge column kept in LDS
constexpr int kLdsTableBytes = 16 * 1024;   // LDS budget of the sub' table (K * K entries of qbytes)
constexpr int kWavesPerGroup = 4;
// Pairs above this many cells take the single-pair fill (GA_BATCH_MAX_CELLS overrides).  Not the measured crossover
// of a lone pair (about 2.7e5 cells) but a value reasoned from that measurement: single-pair fills run one after the
// other while the kernel's pairs run side by side.
constexpr int64_t kDefaultMaxCells = 1 << 20;
constexpr int64_t kScratchBytesCap = 256ll << 20;  // HBM edge scratch of one launch, all waves

// Stripe geometry of a pair with n columns: the fewest stripes of at most 64 * kMaxT columns, then the narrowest T
// that covers n with them (a 300-column pair is one stripe at T = 5).
inline void stripe_geometry(int64_t n, int& T, int& nstripes) {
    nstripes = (int)((n + 64 * kMaxT - 1) / (64 * kMaxT));
    T = (int)((n + 64ll * nstripes - 1) / (64ll * nstripes));
}

// A pair's edge column lives in HBM scratch when it has a second stripe to hand an edge to and more rows than the
// wave's LDS share holds.
inline bool needs_scratch(int64_t m, int64_t n) { return n > 64 * kMaxT && m > kLdsEdgeRows; }

inline bool table_fits_lds(int K, int qbytes) { return (int64_t)K * K * qbytes <= kLdsTableBytes; }

struct Limits {
    int64_t max_cells = kDefaultMaxCells;  // 0: every pair to the single-pair fill
    int64_t scratch_rows_cap = 0;          // most rows of HBM edge column a wave may be given
};

struct Plan {
    std::vector<ga_batch_item> kernel;  // batch_fill_kernel's work list: cells descending, ties in input order
    std::vector<int64_t> single;        // pair indices for the single-pair fill, in the same order
    int64_t scratch_rows = 0;           // rows per wave and ping-pong slice of the HBM edge scratch (0: none)
    int qbytes = 1;                     // bytes per entry of the kernel's sub' table: 1, 2 or 4
};

// The most rows a wave's scratch slice may have with `waves` resident waves (two ping-pong slices of int2 rows each).
inline int64_t scratch_rows_cap(int64_t waves) { return kScratchBytesCap / (std::max<int64_t>(waves, 1) * 2 * 8); }

// One pair's range check: check_problem's guard with the pair's own big, from the pair's own max_cost (the largest
// entry of the costing matrix the single call would build for this pair).  GA_OK or GA_E_RANGE.
inline int check_pair_range(int64_t m, int64_t n, const ga_costs* cs, int64_t max_cost, int64_t maxabs,
                            int64_t& big_out) {
    const int64_t big = (max_cost + 1) * std::max(m, n);
    big_out = big;
    return range_fits(range_bound(std::llabs(big), m, n, maxabs, cs->gap_open)) ? GA_OK : GA_E_RANGE;
}

// GA_OK and the plan, or the code the single-pair path gives for the first failing pair (input order) with
// "pair <index>: <reason>" in err.  pair_max_cost: per pair, the max_cost of that pair's own costing matrix (a
// match / mismatch matrix over one letter has no mismatch entry, so its maximum -- and with it big -- is smaller);
// nullptr: cs->max_cost for every pair.
// also_single(m, n, T, nstripes): a further reason to give a pair to the single-pair path (plan_batch has none;
// plan_batch_align, below, adds its own).
template <typename AlsoSingle>
inline int plan_batch_routed(const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                             const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* cs,
                             const Limits& lim, AlsoSingle also_single, Plan& out, std::string& err) {
    auto fail = [&](int code, const std::string& msg) {
        err = msg;
        return code;
    };
    out = Plan();
    if (npairs < 0 || nseq < 0) return fail(GA_E_ARG, "negative count");
    if (npairs == 0) return GA_OK;
    if (npairs > (int64_t)INT32_MAX) return fail(GA_E_RANGE, "a batch holds at most 2^31 - 1 pairs");
    if (!codes || !seq_off || !pair_a || !pair_b || !cs || !cs->sub || !cs->gap_h || !cs->gap_v)
        return fail(GA_E_ARG, "null argument");
    const int K = cs->K;
    if (K < 1 || K > 255) return fail(GA_E_ARG, "alphabet size K must be in [1,255]");
    if (cs->gap_open < 0) return fail(GA_E_ARG, "gap_open cost must be >= 0");
    if (seq_off[0] != 0) return fail(GA_E_ARG, "seq_off must start at 0");
    for (int64_t s = 0; s < nseq; s++)
        if (seq_off[s + 1] < seq_off[s]) return fail(GA_E_ARG, "seq_off must not decrease");
    if (seq_off[nseq] > (int64_t)INT32_MAX) return fail(GA_E_RANGE, "a batch holds at most 2^31 - 1 codes");
    // a sequence's codes are checked once, however many pairs use it
    std::vector<uint8_t> bad(nseq, 0);
    for (int64_t s = 0; s < nseq; s++)
        for (int64_t q = seq_off[s]; q < seq_off[s + 1]; q++)
            if (codes[q] >= K) {
                bad[s] = 1;
                break;
            }
    const int64_t maxabs = costs_maxabs(cs);
    // sub' beyond the single-pair fill's int16 query profile: the batch kernel then reads 4-byte table entries (a
    // pair routed to the single-pair fill fails there, as a single call does)
    const int qbytes = profile_bytes(cs) ? profile_bytes(cs) : 4;
    const int o = cs->gap_open;
    const bool o_fits = (o + 1) < 32768;  // the single path's traceback-word limit holds for a score too
    struct Cand {
        int64_t cells, idx, big;
    };
    std::vector<Cand> cand((size_t)npairs);
    for (int64_t k = 0; k < npairs; k++) {
        auto at = [k](const char* why) { return "pair " + std::to_string(k) + ": " + why; };
        const int64_t sa = pair_a[k], sb = pair_b[k];
        if (sa < 0 || sa >= nseq || sb < 0 || sb >= nseq) return fail(GA_E_ARG, at("sequence index out of range"));
        const int64_t m = seq_off[sa + 1] - seq_off[sa], n = seq_off[sb + 1] - seq_off[sb];
        if (m < 1 || n < 1) return fail(GA_E_ARG, at("sequences must be non-empty"));
        if (bad[sa]) return fail(GA_E_ARG, at("seq_1 code out of range"));
        if (bad[sb]) return fail(GA_E_ARG, at("seq_2 code out of range"));
        int64_t big = 0;
        if (check_pair_range(m, n, cs, pair_max_cost ? pair_max_cost[k] : cs->max_cost, maxabs, big))
            return fail(GA_E_RANGE, at("problem exceeds the int32 score range of the device path"));
        if (!o_fits) return fail(GA_E_RANGE, at("gap_open cost too large for the traceback word"));
        cand[(size_t)k] = Cand{m * n, k, big};
    }
    out.qbytes = qbytes;
    std::stable_sort(cand.begin(), cand.end(), [](const Cand& x, const Cand& y) { return x.cells > y.cells; });
    const bool tab_ok = table_fits_lds(K, qbytes);
    for (const Cand& cd : cand) {
        const int64_t sa = pair_a[cd.idx], sb = pair_b[cd.idx];
        const int64_t m = seq_off[sa + 1] - seq_off[sa], n = seq_off[sb + 1] - seq_off[sb];
        const bool scr = needs_scratch(m, n);
        ga_batch_item it;
        stripe_geometry(n, it.T, it.nstripes);
        if (cd.cells > lim.max_cells || !tab_ok || (scr && m > lim.scratch_rows_cap) ||
            also_single(m, n, it.T, it.nstripes)) {
            out.single.push_back(cd.idx);
            continue;
        }
        it.a_off = (int32_t)seq_off[sa];
        it.m = (int32_t)m;
        it.b_off = (int32_t)seq_off[sb];
        it.n = (int32_t)n;
        it.big = (int32_t)cd.big;  // range_fits: |big| < 2^29
        it.out = (int32_t)cd.idx;
        out.kernel.push_back(it);
        if (scr) out.scratch_rows = std::max(out.scratch_rows, m);
    }
    return GA_OK;
}

inline int plan_batch(const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                      const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* cs,
                      const Limits& lim, Plan& out, std::string& err) {
    return plan_batch_routed(codes, seq_off, nseq, pair_a, pair_b, pair_max_cost, npairs, cs, lim,
                             [](int64_t, int64_t, int, int) { return false; }, out, err);
}

// ------------------------------------------------------------------ batches with alignment strings (ga_batch_align)
// batch_align_kernel (ga_batch.hip) fills a pair as batch_fill_kernel does, writes every cell's traceback word to a
// slice of HBM scratch that only the pair's wave touches, and walks the pair from (m, n) with the pair's own
// tie-break table.  The words are packed into u32s down the rows, 4 / CB rows of a column to a u32, rows of u32s with
// a pitch of the pair's padded columns: cell (i, j) is bits ((i - 1) % (4 / CB)) * 8 * CB .. of u32
// ((i - 1) / (4 / CB)) * 64 * T * nstripes + (j - 1).
constexpr int64_t kDefaultAlignMaxCells = 1 << 20;
// The traceback scratch of one launch, all waves.  8 GiB of the device's 288: with two waves per SIMD on 256 CUs a
// wave's share is 4 MiB, which holds a pair of kDefaultAlignMaxCells cells even at four bytes a word (its column
// padding aside), so the cells limit and not this cap decides the routing at the default settings.  The engine
// allocates only what the launch's largest pair needs.
constexpr int64_t kTbScratchBytesCap = 8ll << 30;

// u32 words of a pair's traceback slice
inline int64_t tb_slice_words(int64_t m, int T, int nstripes, int CB) {
    const int64_t rpw = 4 / CB;
    return (m + rpw - 1) / rpw * 64 * T * nstripes;
}
inline int64_t tb_slice_words_cap(int64_t waves) { return kTbScratchBytesCap / (std::max<int64_t>(waves, 1) * 4); }

struct AlignLimits : Limits {
    AlignLimits() { max_cells = kDefaultAlignMaxCells; }
    int64_t tb_words_cap = 0;  // most u32 words of traceback scratch a wave may be given
};

struct AlignPlan : Plan {
    int CB = 1;                            // traceback word bytes (ga_check.h tb_word_bytes)
    std::vector<ga_batch_walk_item> walk;  // parallel to `kernel`
    int64_t tab_entries = 0;               // tie-break entries of all kernel pairs (m + n each)
    int64_t ops_words = 0;                 // level words of all kernel pairs (ceil((m + n) / 16) each)
    int64_t tb_words = 0;                  // u32 words per wave of the traceback scratch
};

// plan_batch's checks, order and stripe geometry; to the single-pair path also go pairs with a sequence of one letter
// (only they can raise the reference's IndexError or take its first-step quirk) and pairs whose
// traceback words exceed a wave's share of the scratch.
inline int plan_batch_align(const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                            const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* cs,
                            const AlignLimits& lim, AlignPlan& out, std::string& err) {
    out = AlignPlan();
    const int CB = cs ? tb_word_bytes(cs->gap_open) : 0;  // (0: plan_batch_routed refuses every pair)
    Plan base;
    const int r = plan_batch_routed(
        codes, seq_off, nseq, pair_a, pair_b, pair_max_cost, npairs, cs, lim,
        [&](int64_t m, int64_t n, int T, int nstripes) {
            return std::min(m, n) < 2 || CB == 0 || tb_slice_words(m, T, nstripes, CB) > lim.tb_words_cap;
        },
        base, err);
    if (r) return r;
    static_cast<Plan&>(out) = std::move(base);
    out.CB = std::max(CB, 1);
    out.walk.reserve(out.kernel.size());
    for (const ga_batch_item& it : out.kernel) {
        const int64_t steps = (int64_t)it.m + it.n;
        out.walk.push_back(ga_batch_walk_item{out.tab_entries, out.ops_words});
        out.tab_entries += steps;
        out.ops_words += (steps + 15) / 16;
        out.tb_words = std::max(out.tb_words, tb_slice_words(it.m, it.T, it.nstripes, out.CB));
    }
    return GA_OK;
}

}  // namespace gabatch

// ------------------------------------------------------------------ the stored-words calls
// ga_batch_sample, ga_batch_count, ga_batch_rank and ga_batch_support fill alike: the fill of a pair
// does not depend on what is asked of it, so batch_words_kernel fills every kernel pair once, chunk by chunk, and keeps
// its traceback words in a slice of the pair's own; the call's kernels, later launches on the same stream, read them:
//   sample   batch_walks_kernel walks a pair once per sample, one wave per walk (ga_batch.hip);
//   count    batch_count_kernel counts a pair's co-optimal alignments, one wave per pair (ga_batch_count.hip, 5.13).  A
//            stripe hands the next one two doubles a row, N(i, edge, 0) and N(i, edge, 1): through the wave's LDS
//            share while m fits (kLdsEdgeRows rows), else through a ping-pong pair of HBM slices of the wave's own;
//   rank     batch_rank_table_kernel runs the count recurrence in saturating u64 and keeps every interior cell's three
//            counts in the pair's slice of the chunk's tables (ga_batch_rank.h has the layout); batch_rank_walk_kernel
//            walks a pair once per requested rank, one lane per walk (ga_batch_rank.hip, 5.14);
//   support  batch_support_table_kernel keeps N(i, j, 0) in the same tables, batch_flow_kernel runs the wavefront
//            backwards over the same words and leaves support(i, j) there, batch_support_gather_kernel copies it to
//            the pair's m * n dense doubles in the chunk's output (ga_batch_support.hip, 5.15).
// So they share their limits, the fill side of their plans, one chunker and what the engine asks about the pairs that
// leave the kernel route.

// What batch_words_kernel needs per pair beyond its ga_batch_item (same index in the chunk's work list).
struct ga_batch_words_item {
    int64_t tb_off;    // the pair's slice of the chunk's traceback words (u32 words)
    int64_t tb_words;  // its length: tb_slice_words of the pair
};

// One walk of ga_batch_sample: a sample of a pair.
struct ga_batch_sample_item {
    int64_t tab_off;  // the sample's m + n tie-break entries in the walk launch's table
    int64_t ops_off;  // its ceil((m + n) / 16) u32 words of packed levels
    int32_t fill;     // the pair's index in its chunk's work list
    int32_t out;      // the sample's flat index (pair order, then sample order): walk results and strings go there
};

// One walk item of ga_batch_rank: up to 64 consecutive slots of one pair, lane l walking slot `out` + l.
struct ga_batch_rank_item {
    int64_t ops_off;  // the item's level words in the walk launch's: slot l at ops_off + l * ceil((m + n) / 16)
    int32_t fill;     // the pair's index in its chunk's work list
    int32_t out;      // the first slot's flat index (pair order, then rank order): its rank, and where its strings go
    int32_t nslots;   // 1 .. 64
    int32_t res;      // the first slot's place among the walk launch's results
};

namespace gabatch {

constexpr int64_t kWalkTableEntriesCap = 1ll << 28;  // tie-break entries of one walk launch (1 GiB of u32)
constexpr int64_t kCountEdgeBytes = 16;              // two doubles a row
// The tables of one fill chunk, all its pairs: the words' cap.
constexpr int64_t kRankTableBytesCap = kTbScratchBytesCap;
// The dense output of one fill chunk, all its pairs: 2 GiB, a quarter of the tables' cap -- a pair's table is at
// least three times its output.
constexpr int64_t kSupportBytesCap = 2ll << 30;

// The most rows a wave's count scratch slice may have with `waves` resident waves (two ping-pong slices each).
inline int64_t count_rows_cap(int64_t waves) {
    return kScratchBytesCap / (std::max<int64_t>(waves, 1) * 2 * kCountEdgeBytes);
}

// The limits of the four calls; each reads the ones its planner names.
struct WordsLimits : AlignLimits {
    // u32 words of traceback scratch of one fill chunk, all its pairs (GA_BATCH_SAMPLE_CHUNK_WORDS overrides)
    int64_t chunk_tb_words = kTbScratchBytesCap / 4;
    // of one walk launch: tie-break entries (sample) or steps, m + n a slot (rank); GA_BATCH_SAMPLE_WALK_ENTRIES
    int64_t walk_entries = kWalkTableEntriesCap;
    int64_t count_rows_cap = 0;                       // most rows of HBM count edge a wave may be given (not sample)
    int64_t chunk_table_bytes = kRankTableBytesCap;   // rank, support (GA_BATCH_RANK_TABLE_BYTES overrides)
    int64_t chunk_support_bytes = kSupportBytesCap;   // support (GA_BATCH_SUPPORT_BYTES overrides)
};
using SampleLimits = WordsLimits;
using CountLimits = WordsLimits;
using RankLimits = WordsLimits;
using SupportLimits = WordsLimits;

// Kernel pairs [first, first + count) of the plan's `kernel` are filled by one launch, their slices side by side in
// tb_words u32 words; walk launches [launch_first, launch_first + launch_count) walk them (sample, rank).
struct FillChunk {
    int64_t first = 0, count = 0;
    int64_t tb_words = 0;
    int64_t launch_first = 0, launch_count = 0;
};

// The fill side of the four plans.
struct WordsPlan : Plan {
    int CB = 1;
    std::vector<ga_batch_words_item> words;  // parallel to `kernel`; tb_off counts from the chunk's start
    std::vector<FillChunk> chunks;
    int64_t count_rows = 0;  // rows per wave and ping-pong slice of the count's HBM edge (0: none; not sample)
    // rank, support: the pair's table in its chunk's (parallel to `kernel`) and the chunk's tables (parallel to
    // `chunks`), in 8-byte entries; support: the same for the pair's m * n doubles in its chunk's dense output
    std::vector<int64_t> table_off, chunk_table;
    std::vector<int64_t> support_off, chunk_support;
};
using CountPlan = WordsPlan;
using SupportPlan = WordsPlan;

// Walk items [first, first + count) of SamplePlan::walk share one launch; tab_off / ops_off count from its start.
struct WalkLaunch {
    int64_t first = 0, count = 0;
    int64_t tab_entries = 0, ops_words = 0;
};
struct SamplePlan : WordsPlan {
    std::vector<ga_batch_sample_item> walk;  // chunk by chunk, pair by pair in work-list order, sample by sample
    std::vector<WalkLaunch> launches;
};

// Walk items [first, first + count) of RankPlan::walk share one launch: `slots` results, ops_words level words.
struct RankLaunch {
    int64_t first = 0, count = 0;
    int64_t slots = 0, steps = 0, ops_words = 0;
};
struct RankPlan : WordsPlan {
    std::vector<ga_batch_rank_item> walk;  // chunk by chunk, pair by pair in work-list order, 64 slots at a time
    std::vector<RankLaunch> launches;
};

// plan_batch_align's checks, error order, stripe geometry and routing, a pair's traceback words measured against a
// fill chunk's cap instead of a wave's share.  count_edge (all but sample): also to `single` goes a pair whose count
// edge needs HBM rows beyond lim.count_rows_cap, and count_rows is set.  No chunks yet.
inline int plan_words_routed(const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                             const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* cs,
                             const WordsLimits& lim, bool count_edge, WordsPlan& out, std::string& err) {
    out = WordsPlan();
    const int CB = cs ? tb_word_bytes(cs->gap_open) : 0;  // (0: plan_batch_routed refuses every pair)
    const int64_t cap = std::max<int64_t>(lim.chunk_tb_words, 0);
    Plan base;
    const int r = plan_batch_routed(
        codes, seq_off, nseq, pair_a, pair_b, pair_max_cost, npairs, cs, lim,
        [&](int64_t m, int64_t n, int T, int nstripes) {
            return std::min(m, n) < 2 || CB == 0 || tb_slice_words(m, T, nstripes, CB) > cap ||
                   (count_edge && needs_scratch(m, n) && m > lim.count_rows_cap);
        },
        base, err);
    if (r) return r;
    static_cast<Plan&>(out) = std::move(base);
    out.CB = std::max(CB, 1);
    for (const ga_batch_item& it : out.kernel)
        if (count_edge && needs_scratch(it.m, it.n)) out.count_rows = std::max<int64_t>(out.count_rows, it.m);
    return GA_OK;
}

// A further meter of a fill chunk beside its words: what a pair adds to it and the most a chunk may hold (one unit),
// and where the chunker puts every pair's place in its chunk (parallel to the work list) and every chunk's total.
struct ChunkMeter {
    int64_t (*size)(const ga_batch_item&);
    int64_t cap;
    std::vector<int64_t>*off, *chunk;
};
inline int64_t pair_table_entries(const ga_batch_item& it) { return rank_table_entries(it.m, it.T, it.nstripes); }
inline int64_t pair_cells(const ga_batch_item& it) { return (int64_t)it.m * it.n; }

// The kernel pairs cut into fill chunks, in work-list order, the one chunk loop of the four planners: a chunk takes
// pairs while their traceback words stay within `cap` u32 words and every meter within its own cap (a pair's own share
// of each is within it: the planners' rule; a pair never appears in two chunks); pair t's slice is appended to `words`,
// and close(chunk) is called for every chunk as it ends.
template <typename Close>
inline void plan_fill_chunks(const std::vector<ga_batch_item>& kernel, int CB, int64_t cap,
                             std::vector<ga_batch_words_item>& words, const std::vector<ChunkMeter>& meters, Close close) {
    FillChunk ch;
    words.reserve(words.size() + kernel.size());
    std::vector<int64_t> sum(meters.size(), 0), add(meters.size(), 0);
    auto end_chunk = [&]() {
        for (size_t q = 0; q < meters.size(); q++) meters[q].chunk->push_back(sum[q]);
        close(ch);
    };
    for (int64_t t = 0; t < (int64_t)kernel.size(); t++) {
        const ga_batch_item& it = kernel[(size_t)t];
        const int64_t w = tb_slice_words(it.m, it.T, it.nstripes, CB);
        bool over = ch.tb_words + w > cap;
        for (size_t q = 0; q < meters.size(); q++) {
            add[q] = meters[q].size(it);
            over = over || sum[q] + add[q] > meters[q].cap;
        }
        if (ch.count > 0 && over) {
            end_chunk();
            ch = FillChunk();
            ch.first = t;
            std::fill(sum.begin(), sum.end(), 0);
        }
        words.push_back(ga_batch_words_item{ch.tb_words, w});
        ch.tb_words += w;
        ch.count++;
        for (size_t q = 0; q < meters.size(); q++) {
            meters[q].off->push_back(sum[q]);
            sum[q] += add[q];
        }
    }
    if (ch.count > 0) end_chunk();
}

// The slots of the pairs (sample_off, rank_off): pair k has off[k] .. off[k + 1].  name: the array's, nouns: what a
// slot holds.
inline int check_slot_offsets(const int64_t* off, int64_t npairs, const char* name, const char* nouns, std::string& err) {
    auto fail = [&](int code, const std::string& msg) {
        err = msg;
        return code;
    };
    if (!off) return fail(GA_E_ARG, "null argument");
    if (off[0] != 0) return fail(GA_E_ARG, std::string(name) + " must start at 0");
    for (int64_t k = 0; k < npairs; k++)
        if (off[k + 1] < off[k]) return fail(GA_E_ARG, std::string(name) + " must not decrease");
    if (off[npairs] > (int64_t)INT32_MAX) return fail(GA_E_RANGE, std::string("a batch holds at most 2^31 - 1 ") + nouns);
    return GA_OK;
}

// bytes of the count table of a pair of n columns (its stripe geometry is the fill's)
inline int64_t rank_table_bytes(int64_t m, int64_t n) {
    int T = 1, nstripes = 1;
    stripe_geometry(n, T, nstripes);
    return rank_table_entries(m, T, nstripes) * 8;
}

// A pair of two letters a side whose own table exceeds table_cap bytes, or whose own m * n doubles exceed support_cap
// bytes (rank: no such cap, INT64_MAX), is refused on whatever route, the lowest such pair first.
inline int check_pair_budgets(const int64_t* seq_off, const int32_t* pair_a, const int32_t* pair_b, int64_t npairs,
                              int64_t table_cap, int64_t support_cap, std::string& err) {
    for (int64_t k = 0; k < npairs; k++) {
        const int64_t m = seq_off[pair_a[k] + 1] - seq_off[pair_a[k]], n = seq_off[pair_b[k] + 1] - seq_off[pair_b[k]];
        if (std::min(m, n) < 2) continue;
        const char* why = rank_table_bytes(m, n) > table_cap ? "count table exceeds the rank table budget"
                          : m * n > support_cap / 8        ? "support matrix exceeds the support output budget"
                                                           : nullptr;
        if (why) {
            err = "pair " + std::to_string(k) + ": " + why;
            return GA_E_ARG;
        }
    }
    return GA_OK;
}

// ------------------------------------------------------------------ many seeded walks of a pair (ga_batch_sample)
// The walk items of one fill's pairs items[0 .. count) -- pair items[t] has the samples sample_off[items[t].out] ..
// sample_off[items[t].out + 1] and is walk item field `fill` = t -- appended to `walk`, cut into launches of at most
// walk_entries table entries (a single item above that gets a launch of its own), appended to `launches`.
inline void plan_walk_launches(const ga_batch_item* items, int64_t count, const int64_t* sample_off, int64_t walk_entries,
                               std::vector<ga_batch_sample_item>& walk, std::vector<WalkLaunch>& launches) {
    const int64_t walk_cap = std::max<int64_t>(walk_entries, 1);
    WalkLaunch wl;
    wl.first = (int64_t)walk.size();
    for (int64_t t = 0; t < count; t++) {
        const int64_t steps = (int64_t)items[t].m + items[t].n;
        for (int64_t f = sample_off[items[t].out]; f < sample_off[items[t].out + 1]; f++) {
            if (wl.count > 0 && wl.tab_entries + steps > walk_cap) {
                launches.push_back(wl);
                wl = WalkLaunch();
                wl.first = (int64_t)walk.size();
            }
            walk.push_back(ga_batch_sample_item{wl.tab_entries, wl.ops_words, (int32_t)t, (int32_t)f});
            wl.count++;
            wl.tab_entries += steps;
            wl.ops_words += (steps + 15) / 16;
        }
    }
    if (wl.count > 0) launches.push_back(wl);
}

// plan_words_routed without the count edge.  Pair k has the samples sample_off[k] .. sample_off[k + 1].  A walk launch
// takes items while their table entries stay within lim.walk_entries (a single item above it gets a launch of its
// own); a pair's samples may span several walk launches of its chunk.
inline int plan_batch_sample(const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                             const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* cs,
                             const int64_t* sample_off, const SampleLimits& lim, SamplePlan& out, std::string& err) {
    out = SamplePlan();
    WordsPlan base;
    if (int r = plan_words_routed(codes, seq_off, nseq, pair_a, pair_b, pair_max_cost, npairs, cs, lim, false, base, err))
        return r;
    if (npairs == 0) return GA_OK;
    if (int r = check_slot_offsets(sample_off, npairs, "sample_off", "samples", err)) return r;
    static_cast<WordsPlan&>(out) = std::move(base);
    auto close_chunk = [&](FillChunk& ch) {
        ch.launch_first = (int64_t)out.launches.size();
        plan_walk_launches(out.kernel.data() + ch.first, ch.count, sample_off, lim.walk_entries, out.walk, out.launches);
        ch.launch_count = (int64_t)out.launches.size() - ch.launch_first;
        out.chunks.push_back(ch);
    };
    plan_fill_chunks(out.kernel, out.CB, std::max<int64_t>(lim.chunk_tb_words, 0), out.words, {}, close_chunk);
    return GA_OK;
}

// ------------------------------------------------------------------ co-optimal alignment counts (ga_batch_count)
// plan_words_routed with the count edge, and plan_batch_sample's chunks.  The caller decides what becomes of `single`
// (a pair with a one-letter sequence has no count; the others are filled by the single-pair fill).
inline int plan_batch_count(const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                            const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* cs,
                            const CountLimits& lim, CountPlan& out, std::string& err) {
    if (int r = plan_words_routed(codes, seq_off, nseq, pair_a, pair_b, pair_max_cost, npairs, cs, lim, true, out, err))
        return r;
    plan_fill_chunks(out.kernel, out.CB, std::max<int64_t>(lim.chunk_tb_words, 0), out.words, {},
                     [&](const FillChunk& ch) { out.chunks.push_back(ch); });
    return GA_OK;
}

// ------------------------------------------------------------------ co-optimal alignments by rank (ga_batch_rank)
// plan_walk_launches' shape for rank items: the slots rank_off[items[t].out] .. rank_off[items[t].out + 1] of pair
// items[t] in groups of 64, appended to `walk`, cut into launches of at most walk_entries steps (m + n a slot; a
// single item above that gets a launch of its own), appended to `launches`.
inline void plan_rank_launches(const ga_batch_item* items, int64_t count, const int64_t* rank_off, int64_t walk_entries,
                               std::vector<ga_batch_rank_item>& walk, std::vector<RankLaunch>& launches) {
    const int64_t walk_cap = std::max<int64_t>(walk_entries, 1);
    RankLaunch wl;
    wl.first = (int64_t)walk.size();
    for (int64_t t = 0; t < count; t++) {
        const int64_t steps = (int64_t)items[t].m + items[t].n, wps = (steps + 15) / 16;
        const int64_t last = rank_off[items[t].out + 1];
        for (int64_t f = rank_off[items[t].out]; f < last; f += 64) {
            const int64_t ns = std::min<int64_t>(64, last - f);
            if (wl.count > 0 && wl.steps + ns * steps > walk_cap) {
                launches.push_back(wl);
                wl = RankLaunch();
                wl.first = (int64_t)walk.size();
            }
            walk.push_back(ga_batch_rank_item{wl.ops_words, (int32_t)t, (int32_t)f, (int32_t)ns, (int32_t)wl.slots});
            wl.count++;
            wl.slots += ns;
            wl.steps += ns * steps;
            wl.ops_words += ns * wps;
        }
    }
    if (wl.count > 0) launches.push_back(wl);
}

// plan_batch_count's checks, error order, stripe geometry and routing.  Pair k has the ranks rank_off[k] ..
// rank_off[k + 1] (none is legal: the pair is filled and counted).  check_pair_budgets' refusal for the tables.  A
// chunk closes when either its words would exceed lim.chunk_tb_words or its tables lim.chunk_table_bytes; a chunk's
// walk items follow plan_rank_launches.
inline int plan_batch_rank(const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                           const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* cs,
                           const int64_t* rank_off, const RankLimits& lim, RankPlan& out, std::string& err) {
    out = RankPlan();
    WordsPlan base;
    if (int r = plan_words_routed(codes, seq_off, nseq, pair_a, pair_b, pair_max_cost, npairs, cs, lim, true, base, err))
        return r;
    if (npairs == 0) return GA_OK;
    if (int r = check_slot_offsets(rank_off, npairs, "rank_off", "ranks", err)) return r;
    const int64_t table_cap = std::max<int64_t>(lim.chunk_table_bytes, 0);
    if (int r = check_pair_budgets(seq_off, pair_a, pair_b, npairs, table_cap, INT64_MAX, err)) return r;
    static_cast<WordsPlan&>(out) = std::move(base);
    auto close_chunk = [&](FillChunk& ch) {
        ch.launch_first = (int64_t)out.launches.size();
        plan_rank_launches(out.kernel.data() + ch.first, ch.count, rank_off, lim.walk_entries, out.walk, out.launches);
        ch.launch_count = (int64_t)out.launches.size() - ch.launch_first;
        out.chunks.push_back(ch);
    };
    plan_fill_chunks(out.kernel, out.CB, std::max<int64_t>(lim.chunk_tb_words, 0), out.words,
                     {{pair_table_entries, table_cap / 8, &out.table_off, &out.chunk_table}}, close_chunk);
    return GA_OK;
}

// ------------------------------------------------------------------ match support (ga_batch_support)
// plan_batch_count's checks, error order, stripe geometry and routing.  check_pair_budgets' refusals for the tables
// and the output.  A chunk closes when its words would exceed lim.chunk_tb_words, its tables lim.chunk_table_bytes or
// its output lim.chunk_support_bytes.
inline int plan_batch_support(const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                              const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* cs,
                              const SupportLimits& lim, SupportPlan& out, std::string& err) {
    out = SupportPlan();
    WordsPlan base;
    if (int r = plan_words_routed(codes, seq_off, nseq, pair_a, pair_b, pair_max_cost, npairs, cs, lim, true, base, err))
        return r;
    if (npairs == 0) return GA_OK;
    const int64_t table_cap = std::max<int64_t>(lim.chunk_table_bytes, 0);
    const int64_t support_cap = std::max<int64_t>(lim.chunk_support_bytes, 0);
    if (int r = check_pair_budgets(seq_off, pair_a, pair_b, npairs, table_cap, support_cap, err)) return r;
    out = std::move(base);
    plan_fill_chunks(out.kernel, out.CB, std::max<int64_t>(lim.chunk_tb_words, 0), out.words,
                     {{pair_table_entries, table_cap / 8, &out.table_off, &out.chunk_table},
                      {pair_cells, support_cap / 8, &out.support_off, &out.chunk_support}},
                     [&](const FillChunk& ch) { out.chunks.push_back(ch); });
    return GA_OK;
}

// ------------------------------------------------------------------ the pairs that left the kernel route
// What the engine decides about a pair of plan.single of ga_batch_count, _rank and _support before anything is
// launched: empty, or why the pair cannot be handled.  band: gawalk::band_rows of the pair on this device (0: its
// stored words fit the budget); rows_cap: count_rows_cap of the one workgroup that handles such a pair; subject and
// activity word the call ("count needs" / "counting", "ranks need" / "ranking", "support needs" / "support").
inline std::string no_band_reason(const char* activity) {
    return std::string("traceback words exceed the budget, and ") + activity + " has no banded route";
}
inline std::string single_pair_verdict(int64_t m, int64_t n, int64_t band, int64_t rows_cap, const char* subject,
                                       const char* activity) {
    if (std::min(m, n) < 2) return std::string(subject) + " sequences of at least two letters";
    if (band != 0) return no_band_reason(activity);
    if (needs_scratch(m, n) && m > rows_cap) return "edge column exceeds the count scratch";
    return std::string();
}

// The one-pair work list of the large route: pair k (m x n, codes at a_off / b_off) filled by the single-pair engine
// with stored words at TC 16-byte words per lane, nstripes * T stripes of 64 columns and CB bytes a word, as the four
// calls' kernels take it under LAYOUT_STRIPE: the pair's own stripe geometry (the count, table and support kernels
// read it; where a word lies comes from TC), its codes' places (batch_walks_kernel reads them) and one slice, the
// fill's words.  nullptr, or the refusal.
struct LargeWork {
    ga_batch_item item;
    ga_batch_words_item words;  // {0, tb_words}
};
inline const char* large_route_work(int64_t m, int64_t n, int64_t k, int64_t a_off, int64_t b_off, int nstripes, int T,
                                    int TC, int CB, LargeWork& out) {
    const int64_t tb_words = (int64_t)nstripes * T * TC * 256;
    if ((int64_t)TC * (16 / CB) < m || tb_words < stripe_words(n, TC)) return "the fill's words do not cover the pair";
    out.item = ga_batch_item{(int32_t)a_off, (int32_t)m, (int32_t)b_off, (int32_t)n, 0, (int32_t)k, 0, 0};
    stripe_geometry(n, out.item.T, out.item.nstripes);
    out.words = ga_batch_words_item{0, tb_words};
    return nullptr;
}

}  // namespace gabatch
