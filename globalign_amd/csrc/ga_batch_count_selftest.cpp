// ga_batch_count_selftest.cpp -- CPU self-test of the host's share of ga_batch_count: the count planner (ga_batch.h
// plan_batch_count: plan_batch_sample's fill side plus the count launch's edge scratch), what the four stored-words
// calls share (the chunker's meters, the large route's work list, the verdict on a pair of `single`) and the CPU model
// of the count recurrence (ga_batch_count.h), in double against 128-bit integers and against a walk of every path, plain and under
// AddressSanitizer + UndefinedBehaviorSanitizer (make -C globalign_amd/csrc batch_count_selftest batch_count_asan; run
// by tests/test_batch_count_host.py).  No HIP: the kernel is tested on the GPU.
#include <cmath>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "ga_batch.h"
#include "ga_batch_count.h"
#include "ga_batch_layout.h"

using namespace gabatch;

namespace {

int failures = 0;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            failures++;                                    \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);             \
            std::fprintf(stderr, "\n");                    \
        }                                                  \
    } while (0)

// match 0 / mismatch `mis` / gap extension `ext` over K - 1 letters and the gap code K - 1
struct Tables {
    int K;
    std::vector<int32_t> sub, gh, gv;
    ga_costs cs;
    Tables(int K_, int mis, int ext, int open) : K(K_), sub((size_t)K_ * K_), gh((size_t)K_, ext), gv((size_t)K_, ext) {
        for (int x = 0; x < K; x++)
            for (int y = 0; y < K; y++) sub[(size_t)x * K + y] = x == y ? 0 : (x == K - 1 || y == K - 1) ? ext : mis;
        cs = ga_costs{K, sub.data(), gh.data(), gv.data(), open, std::max(mis, ext)};
    }
};

struct Batch {
    std::vector<uint8_t> codes;
    std::vector<int64_t> off{0};
    std::vector<int32_t> pa, pb;
    int64_t npairs() const { return (int64_t)pa.size(); }
    int64_t nseq() const { return (int64_t)off.size() - 1; }
    void add(int64_t m, int64_t n, std::mt19937& rng) {
        for (const int64_t len : {m, n}) {
            for (int64_t q = 0; q < len; q++) codes.push_back((uint8_t)(rng() % 4));
            off.push_back((int64_t)codes.size());
        }
        pa.push_back((int32_t)nseq() - 2);
        pb.push_back((int32_t)nseq() - 1);
    }
};

int plan(const Batch& b, const Tables& t, const CountLimits& lim, CountPlan& p, std::string& err) {
    return plan_batch_count(b.codes.data(), b.off.data(), b.nseq(), b.pa.data(), b.pb.data(), nullptr, b.npairs(), &t.cs,
                            lim, p, err);
}

CountLimits wide_limits() {
    CountLimits lim;
    lim.max_cells = 1 << 30;
    lim.scratch_rows_cap = 1 << 20;
    lim.count_rows_cap = 1 << 20;
    return lim;
}

bool same_item(const ga_batch_item& x, const ga_batch_item& y) {
    return x.a_off == y.a_off && x.m == y.m && x.b_off == y.b_off && x.n == y.n && x.big == y.big && x.out == y.out &&
           x.T == y.T && x.nstripes == y.nstripes;
}

// every invariant of a count plan; with a count scratch wide enough for every pair its fill side is plan_batch_sample's
void check_plan(const Batch& b, const Tables& t, const CountLimits& lim, const CountPlan& p, const char* what) {
    CHECK(p.words.size() == p.kernel.size(), "%s: one slice per kernel pair", what);
    CHECK(p.kernel.size() + p.single.size() == (size_t)b.npairs(), "%s: every pair is routed once", what);
    std::vector<int> seen((size_t)b.npairs(), 0);
    for (const ga_batch_item& it : p.kernel) seen[(size_t)it.out]++;
    for (const int64_t k : p.single) seen[(size_t)k]++;
    for (size_t k = 0; k < seen.size(); k++) CHECK(seen[k] == 1, "%s: pair %zu is routed once", what, k);
    int64_t rows = 0, next_pair = 0;
    for (size_t q = 0; q < p.kernel.size(); q++) {
        const ga_batch_item& it = p.kernel[q];
        int T, ns;
        stripe_geometry(it.n, T, ns);
        CHECK(it.T == T && it.nstripes == ns && it.m >= 2 && it.n >= 2, "%s: work item %zu's geometry", what, q);
        CHECK((int64_t)it.m * it.n <= lim.max_cells, "%s: work item %zu within the cells limit", what, q);
        if (needs_scratch(it.m, it.n)) {
            CHECK(it.m <= lim.count_rows_cap && it.m <= lim.scratch_rows_cap, "%s: work item %zu's edge fits", what, q);
            rows = std::max<int64_t>(rows, it.m);
        }
        if (q > 0) CHECK((int64_t)p.kernel[q - 1].m * p.kernel[q - 1].n >= (int64_t)it.m * it.n, "%s: longest first", what);
    }
    CHECK(p.count_rows == rows, "%s: the count scratch holds the tallest pair that needs it", what);
    for (const int64_t k : p.single) {
        const int64_t m = b.off[(size_t)b.pa[(size_t)k] + 1] - b.off[(size_t)b.pa[(size_t)k]];
        const int64_t n = b.off[(size_t)b.pb[(size_t)k] + 1] - b.off[(size_t)b.pb[(size_t)k]];
        int T, ns;
        stripe_geometry(n, T, ns);
        const bool scr = needs_scratch(m, n);
        CHECK(std::min(m, n) < 2 || m * n > lim.max_cells || tb_slice_words(m, T, ns, p.CB) > lim.chunk_tb_words ||
                  (scr && (m > lim.count_rows_cap || m > lim.scratch_rows_cap)),
              "%s: pair %lld left the kernel route for a reason", what, (long long)k);
    }
    for (const FillChunk& ch : p.chunks) {
        CHECK(ch.first == next_pair && ch.count > 0, "%s: chunks follow each other", what);
        CHECK(ch.tb_words <= lim.chunk_tb_words, "%s: a chunk's slices stay within the cap", what);
        int64_t off = 0;
        for (int64_t q = ch.first; q < ch.first + ch.count && q < (int64_t)p.kernel.size(); q++) {
            const ga_batch_item& it = p.kernel[(size_t)q];
            const ga_batch_words_item& ws = p.words[(size_t)q];
            CHECK(ws.tb_off == off && ws.tb_words == tb_slice_words(it.m, it.T, it.nstripes, p.CB),
                  "%s: slice of work item %lld", what, (long long)q);
            CHECK(ws.tb_words * 4 >= (int64_t)it.m * it.n * p.CB, "%s: slice holds work item %lld", what, (long long)q);
            // the last cell's word lies inside the slice
            const int pitch = 64 * it.T * it.nstripes;
            const unsigned long long w = p.CB == 1   ? TbAddr<1, LAYOUT_BATCH>::word(it.m, it.n, pitch)
                                         : p.CB == 2 ? TbAddr<2, LAYOUT_BATCH>::word(it.m, it.n, pitch)
                                                     : TbAddr<4, LAYOUT_BATCH>::word(it.m, it.n, pitch);
            CHECK((int64_t)w < ws.tb_words, "%s: cell (m, n) of work item %lld inside its slice", what, (long long)q);
            off += ws.tb_words;
        }
        CHECK(off == ch.tb_words, "%s: a chunk's words are its slices", what);
        next_pair = ch.first + ch.count;
    }
    CHECK(next_pair == (int64_t)p.kernel.size(), "%s: every work item sits in a chunk", what);
    if (lim.count_rows_cap >= lim.scratch_rows_cap) {
        // the sample planner's fill side for the same inputs, every pair without samples
        SampleLimits sl;
        static_cast<Limits&>(sl) = lim;
        sl.chunk_tb_words = lim.chunk_tb_words;
        const std::vector<int64_t> sample_off((size_t)b.npairs() + 1, 0);
        SamplePlan sp;
        std::string err;
        CHECK(plan_batch_sample(b.codes.data(), b.off.data(), b.nseq(), b.pa.data(), b.pb.data(), nullptr, b.npairs(), &t.cs,
                                sample_off.data(), sl, sp, err) == GA_OK, "%s: sample plan failed: %s", what, err.c_str());
        CHECK(sp.single == p.single && sp.kernel.size() == p.kernel.size() && sp.CB == p.CB && sp.qbytes == p.qbytes &&
                  sp.scratch_rows == p.scratch_rows && sp.chunks.size() == p.chunks.size(),
              "%s: the fill side is plan_batch_sample's", what);
        for (size_t q = 0; q < p.kernel.size() && q < sp.kernel.size(); q++)
            CHECK(same_item(p.kernel[q], sp.kernel[q]) && p.words[q].tb_off == sp.words[q].tb_off &&
                      p.words[q].tb_words == sp.words[q].tb_words, "%s: work item %zu is plan_batch_sample's", what, q);
        for (size_t q = 0; q < p.chunks.size() && q < sp.chunks.size(); q++)
            CHECK(p.chunks[q].first == sp.chunks[q].first && p.chunks[q].count == sp.chunks[q].count &&
                      p.chunks[q].tb_words == sp.chunks[q].tb_words, "%s: chunk %zu is plan_batch_sample's", what, q);
    }
}

// Round `round` of the random batches: its gap open cost (one-, two- and four-byte words in turn), its pairs into b
// and its limits.
int round_gap_open(int round) { return round % 3 == 0 ? 4 : round % 3 == 1 ? 30 : 200; }
CountLimits random_round(std::mt19937& rng, int round, Batch& b) {
    const int npairs = 1 + (int)(rng() % 40);
    for (int k = 0; k < npairs; k++) {
        // one-letter sequences now and then, and pairs tall and wide enough for an HBM edge column
        auto len = [&](int max_len) { return rng() % 9 == 0 ? 1 : 2 + (int64_t)(rng() % (unsigned)(max_len - 1)); };
        if (rng() % 6 == 0) b.add(len(3000), len(1200), rng);
        else b.add(len(300), len(700), rng);
    }
    CountLimits lim = wide_limits();
    if (round % 2) {
        lim.max_cells = 1 + (int64_t)(rng() % 2000000);
        lim.chunk_tb_words = 64 + (int64_t)(rng() % 400000);
    }
    if (round % 4 == 3) lim.count_rows_cap = 1100 + (int64_t)(rng() % 1500);
    return lim;
}

void test_random_batches() {
    std::mt19937 rng(13);
    for (int round = 0; round < 200; round++) {
        Tables t(5, 5, 3, round_gap_open(round));
        Batch b;
        const CountLimits lim = random_round(rng, round, b);
        CountPlan p;
        std::string err;
        CHECK(plan(b, t, lim, p, err) == GA_OK, "round %d: plan failed: %s", round, err.c_str());
        check_plan(b, t, lim, p, ("round " + std::to_string(round)).c_str());
    }
}

void test_forced_routes() {
    Tables t(5, 5, 3, 4);
    std::mt19937 rng(5);
    Batch b;
    for (int k = 0; k < 5; k++) b.add(40 + 10 * k, 41 + 10 * k, rng);
    b.add(3000, 70, rng);    // tall and narrow: one stripe, no edge column
    b.add(3000, 600, rng);   // tall and wide: the edge column goes through HBM
    b.add(1024, 600, rng);   // the LDS share holds 1024 rows
    CountPlan p;
    std::string err;
    CountLimits lim = wide_limits();
    CHECK(plan(b, t, lim, p, err) == GA_OK, "plan failed: %s", err.c_str());
    CHECK(p.chunks.size() == 1 && p.single.empty() && p.kernel.size() == 8 && p.count_rows == 3000,
          "the defaults: one chunk, the count scratch of the one pair that needs it (%lld rows)", (long long)p.count_rows);
    check_plan(b, t, lim, p, "defaults");
    // a count scratch too small for the tall and wide pair sends it, and only it, to the single path
    lim.count_rows_cap = 2999;
    CHECK(plan(b, t, lim, p, err) == GA_OK, "plan failed: %s", err.c_str());
    CHECK(p.single == std::vector<int64_t>{6} && p.count_rows == 0, "an edge column over the cap goes to the single path");
    check_plan(b, t, lim, p, "edge over the cap");
    // tiny chunks
    lim = wide_limits();
    lim.chunk_tb_words = tb_slice_words(3000, 5, 2, 1);
    CHECK(plan(b, t, lim, p, err) == GA_OK, "plan failed: %s", err.c_str());
    CHECK(p.chunks.size() > 1 && p.kernel.size() == 8, "a small cap gives %zu chunks", p.chunks.size());
    check_plan(b, t, lim, p, "small chunks");
    lim.chunk_tb_words--;
    CHECK(plan(b, t, lim, p, err) == GA_OK, "plan failed: %s", err.c_str());
    CHECK(p.single == std::vector<int64_t>{6}, "a slice over the cap goes to the single path");
    check_plan(b, t, lim, p, "slice over the cap");
    // the cap formula: two ping-pong slices of 16-byte rows per wave within the launch's scratch
    CHECK(count_rows_cap(2048) * 2048 * 2 * 16 <= kScratchBytesCap && (count_rows_cap(2048) + 1) * 2048 * 2 * 16 > kScratchBytesCap,
          "count_rows_cap fills the scratch cap");
    CHECK(count_rows_cap(0) == count_rows_cap(1), "no waves count as one");
}

void test_errors() {
    Tables t(5, 5, 3, 4);
    Batch b;
    b.codes.assign(20, 0);
    b.off = {0, 10, 20};
    b.pa = {0};
    b.pb = {1};
    CountPlan p;
    std::string err;
    // the pairs' own errors, as plan_batch_align gives them
    b.codes[3] = 9;
    CHECK(plan(b, t, wide_limits(), p, err) == GA_E_ARG && err == "pair 0: seq_1 code out of range", "got: %s", err.c_str());
    b.codes[3] = 0;
    b.pb = {2};
    CHECK(plan(b, t, wide_limits(), p, err) == GA_E_ARG && err == "pair 0: sequence index out of range", "got: %s", err.c_str());
    b.pb = {1};
    CHECK(plan_batch_count(b.codes.data(), b.off.data(), 2, b.pa.data(), b.pb.data(), nullptr, 1, nullptr, wide_limits(), p,
                           err) == GA_E_ARG, "null costs");
    CHECK(plan_batch_count(nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, &t.cs, wide_limits(), p, err) == GA_OK &&
              p.chunks.empty() && p.kernel.empty(), "an empty batch plans to nothing");
    // a gap open cost beyond the traceback word is refused for the pair
    Tables big(5, 5, 3, 40000);
    CHECK(plan(b, big, wide_limits(), p, err) == GA_E_RANGE, "gap open cost too large: %s", err.c_str());
    // a one-letter sequence leaves the kernel route: the caller refuses it
    Batch one;
    one.codes.assign(5, 0);
    one.off = {0, 1, 5};
    one.pa = {0};
    one.pb = {1};
    CHECK(plan(one, t, wide_limits(), p, err) == GA_OK && p.single == std::vector<int64_t>{0} && p.kernel.empty(),
          "a one-letter sequence goes to the single list");
}

// ------------------------------------------------------------------ what the four stored-words calls share
// plan_fill_chunks with one and two meters beside the words, over test_random_batches' batches (its seed)
void test_chunker_meters() {
    std::mt19937 rng(13), caps(29);
    for (int round = 0; round < 200; round++) {
        Tables t(5, 5, 3, round_gap_open(round));
        Batch b;
        const CountLimits lim = random_round(rng, round, b);
        CountPlan p;
        std::string err;
        CHECK(plan(b, t, lim, p, err) == GA_OK, "round %d: plan failed: %s", round, err.c_str());
        for (int nmeters = 1; nmeters <= 2; nmeters++) {
            // caps that a lone pair may exceed, now and then
            const int64_t cap[3] = {lim.chunk_tb_words, 1000 + (int64_t)(caps() % 3000000), 100 + (int64_t)(caps() % 600000)};
            int64_t (*const size[3])(const ga_batch_item&) = {nullptr, pair_table_entries, pair_cells};
            std::vector<ga_batch_words_item> words;
            std::vector<int64_t> off[3], total[3];
            std::vector<FillChunk> chunks;
            std::vector<ChunkMeter> meters;
            for (int q = 1; q <= nmeters; q++) meters.push_back(ChunkMeter{size[q], cap[q], &off[q], &total[q]});
            plan_fill_chunks(p.kernel, p.CB, cap[0], words, meters, [&](const FillChunk& ch) { chunks.push_back(ch); });
            auto add = [&](int q, int64_t at) {
                const ga_batch_item& it = p.kernel[(size_t)at];
                return q == 0 ? tb_slice_words(it.m, it.T, it.nstripes, p.CB) : size[q](it);
            };
            CHECK(words.size() == p.kernel.size(), "round %d: one slice per pair", round);
            int64_t next_pair = 0;
            for (size_t c = 0; c < chunks.size(); c++) {
                const FillChunk& ch = chunks[c];
                CHECK(ch.first == next_pair && ch.count > 0, "round %d: chunks follow each other", round);
                next_pair = ch.first + ch.count;
                bool next_over = false;
                for (int q = 0; q <= nmeters; q++) {
                    CHECK(q == 0 || (off[q].size() == p.kernel.size() && total[q].size() == chunks.size()),
                          "round %d: meter %d has a place per pair and a total per chunk", round, q);
                    int64_t sum = 0;
                    for (int64_t at = ch.first; at < next_pair; at++) {
                        const int64_t place = q == 0 ? words[(size_t)at].tb_off : off[q][(size_t)at];
                        CHECK(place == sum, "round %d: meter %d, pair %lld sits at the running sum", round, q, (long long)at);
                        sum += add(q, at);
                    }
                    CHECK(sum == (q == 0 ? ch.tb_words : total[q][c]), "round %d: meter %d, chunk %zu's total", round, q, c);
                    CHECK(sum <= cap[q] || ch.count == 1, "round %d: meter %d, chunk %zu within the cap", round, q, c);
                    if (c + 1 < chunks.size()) next_over = next_over || sum + add(q, next_pair) > cap[q];
                }
                CHECK(c + 1 == chunks.size() || next_over, "round %d: chunk %zu closed for a cap", round, c);
            }
            CHECK(next_pair == (int64_t)p.kernel.size(), "round %d: every pair sits in a chunk", round);
        }
    }
}

// large_route_work: the one-pair work list over a single-pair fill's words
void test_large_route_work() {
    for (const int CB : {1, 2, 4}) {
        const int spc = 16 / CB, TC = 7;
        const int64_t m = (int64_t)TC * spc, n = 130, k = 5;  // three stripes of 64 columns
        LargeWork w;
        CHECK(large_route_work(m, n, k, 11, 22, 1, 3, TC, CB, w) == nullptr, "CB %d: TC * (16 / CB) == m is covered", CB);
        int T, ns;
        stripe_geometry(n, T, ns);
        CHECK(w.item.a_off == 11 && w.item.m == m && w.item.b_off == 22 && w.item.n == n && w.item.big == 0 && w.item.out == k &&
                  w.item.T == T && w.item.nstripes == ns, "CB %d: the item is the pair with its own geometry", CB);
        CHECK(w.words.tb_off == 0 && w.words.tb_words == 3 * TC * 256 && w.words.tb_words == stripe_words(n, TC),
              "CB %d: one slice, the fill's words, exactly stripe_words", CB);
        const std::string refusal = "the fill's words do not cover the pair";
        const char* why = large_route_work(m + 1, n, k, 11, 22, 1, 3, TC, CB, w);
        CHECK(why && why == refusal, "CB %d: TC * (16 / CB) == m - 1 is refused", CB);
        // (the words come in stripes of TC * 256: the nearest shortfall is one stripe)
        why = large_route_work(m, n, k, 11, 22, 1, 2, TC, CB, w);
        CHECK(why && why == refusal, "CB %d: a stripe fewer than stripe_words is refused", CB);
        CHECK(large_route_work(m, 128, k, 0, 0, 2, 1, TC, CB, w) == nullptr && w.words.tb_words == stripe_words(128, TC) &&
                  large_route_work(m, 129, k, 0, 0, 2, 1, TC, CB, w) != nullptr, "CB %d: the last covered column", CB);
        // a wide pair: the fill's stripes of 64 columns, the item's of 64 * T
        CHECK(large_route_work(m, 1000, k, 0, 0, 4, 4, TC, CB, w) == nullptr && w.item.T == 8 && w.item.nstripes == 2 &&
                  w.words.tb_words == 16 * TC * 256, "CB %d: a two-stripe item over sixteen fill stripes", CB);
    }
}

// single_pair_verdict: each reason, their precedence, and the calls' words
void test_single_pair_verdict() {
    const int64_t cap = count_rows_cap(kWavesPerGroup);
    const char* words[3][2] = {{"count needs", "counting"}, {"ranks need", "ranking"}, {"support needs", "support"}};
    const std::string short_seq[3] = {"count needs sequences of at least two letters", "ranks need sequences of at least two letters",
                                      "support needs sequences of at least two letters"};
    const std::string no_band[3] = {"traceback words exceed the budget, and counting has no banded route",
                                    "traceback words exceed the budget, and ranking has no banded route",
                                    "traceback words exceed the budget, and support has no banded route"};
    const std::string edge = "edge column exceeds the count scratch";
    for (int q = 0; q < 3; q++) {
        auto verdict = [&](int64_t m, int64_t n, int64_t band, int64_t rows_cap) {
            return single_pair_verdict(m, n, band, rows_cap, words[q][0], words[q][1]);
        };
        CHECK(verdict(50, 60, 0, cap).empty() && verdict(2, 2, 0, cap).empty(), "call %d: a pair that can be handled", q);
        CHECK(verdict(1, 60, 0, cap) == short_seq[q] && verdict(60, 1, 0, cap) == short_seq[q], "call %d: one letter", q);
        CHECK(verdict(50, 60, 256, cap) == no_band[q] && no_band_reason(words[q][1]) == no_band[q], "call %d: banded", q);
        // an edge column in HBM (more than 512 columns, more than 1024 rows) beyond the cap, and at it
        CHECK(verdict(2000, 600, 0, 1999) == edge && verdict(2000, 600, 0, 2000).empty(), "call %d: the edge's cap", q);
        CHECK(verdict(2000, 512, 0, 10).empty() && verdict(1024, 600, 0, 10).empty(), "call %d: no HBM edge, no cap", q);
        CHECK(verdict(1, 600, 256, 0) == short_seq[q], "call %d: one letter comes first", q);
        CHECK(verdict(2000, 600, 256, 10) == no_band[q], "call %d: the band comes before the edge", q);
    }
    CHECK(cap > 3000, "one workgroup's count scratch holds tall pairs (%lld rows)", (long long)cap);
}

// ------------------------------------------------------------------ the recurrence
typedef unsigned __int128 u128;

// every path of the walk's DAG from (i, j, L), one by one
uint64_t walk_paths(const std::vector<uint16_t>& sets, int64_t n, int64_t i, int64_t j, int L) {
    if (i == 0 || j == 0) return 1;
    const unsigned s = (sets[(size_t)((i - 1) * n + (j - 1))] >> (3 * L)) & 7u;
    uint64_t total = 0;
    if (s & 1u) total += walk_paths(sets, n, i - 1, j - 1, 0);
    if (s & 2u) total += walk_paths(sets, n, i, j - 1, 1);
    if (s & 4u) total += walk_paths(sets, n, i - 1, j, 2);
    return total;
}

std::vector<uint16_t> random_sets(std::mt19937& rng, int64_t m, int64_t n, int tie_in) {
    std::vector<uint16_t> sets((size_t)(m * n));
    for (uint16_t& s : sets) {
        s = 0;
        for (int L = 0; L < 3; L++) {
            // a non-empty set: one entry, or (one time in tie_in) any of the seven
            const unsigned set = rng() % (unsigned)tie_in == 0 ? 1u + rng() % 7u : 1u << (rng() % 3u);
            s = (uint16_t)(s | (set << (3 * L)));
        }
    }
    return sets;
}

void test_model() {
    std::mt19937 rng(77);
    // tiny grids: the recurrence against the paths themselves
    for (int round = 0; round < 300; round++) {
        const int64_t m = 1 + rng() % 6, n = 1 + rng() % 6;
        const std::vector<uint16_t> sets = random_sets(rng, m, n, 1 + (int)(rng() % 3));
        const uint64_t want = walk_paths(sets, n, m, n, 0);
        const u128 got = count_paths<u128>(sets.data(), m, n);
        const double gotd = count_paths<double>(sets.data(), m, n);
        CHECK(got == (u128)want && gotd == (double)want, "tiny grid %lld x %lld: %llu paths, the model has %llu / %.17g",
              (long long)m, (long long)n, (unsigned long long)want, (unsigned long long)got, gotd);
    }
    // small grids: double against 128-bit integers, exactly (the counts stay far below 2^53)
    for (int round = 0; round < 300; round++) {
        const int64_t m = 2 + rng() % 13, n = 2 + rng() % 13;
        const std::vector<uint16_t> sets = random_sets(rng, m, n, 1 + (int)(rng() % 4));
        const u128 got = count_paths<u128>(sets.data(), m, n);
        const double gotd = count_paths<double>(sets.data(), m, n);
        CHECK(got >= 1 && got < ((u128)1 << 53) && (u128)gotd == got && gotd == (double)(uint64_t)got,
              "small grid %lld x %lld: double %.17g against the integers", (long long)m, (long long)n, gotd);
    }
    // every decision tied: the fastest growth; 2 x 2 by hand, then the double stays within the chain's rounding
    // bound of the integers while they fit 128 bits, saturates past the double range and is never NaN
    {
        const std::vector<uint16_t> all(4, 0x1ff);
        // N(1, 1, .) = 3; N(1, 2, .) = N(2, 1, .) = 1 + 3 + 1 = 5; N(2, 2, 0) = 3 + 5 + 5
        CHECK(count_paths<u128>(all.data(), 2, 2) == 13 && count_paths<double>(all.data(), 2, 2) == 13.0, "2 x 2, all tied");
    }
    for (const int64_t side : {20, 45}) {
        const std::vector<uint16_t> all((size_t)(side * side), 0x1ff);
        const u128 got = count_paths<u128>(all.data(), side, side);
        const double gotd = count_paths<double>(all.data(), side, side);
        const double want = std::ldexp((double)(uint64_t)(got >> 64), 64) + (double)(uint64_t)got;
        CHECK(std::fabs(gotd - want) <= want * 2.0 * (2 * side) * std::ldexp(1.0, -53) * 1.01 + want * std::ldexp(1.0, -52),
              "all tied, side %lld: %.17g against %.17g", (long long)side, gotd, want);
    }
    {
        const int64_t side = 450;
        const std::vector<uint16_t> all((size_t)(side * side), 0x1ff);
        const double gotd = count_paths<double>(all.data(), side, side);
        CHECK(std::isinf(gotd) && gotd > 0, "all tied, side 450: +inf, got %.17g", gotd);
        const double mid = count_paths<double>(all.data(), 300, 300);
        CHECK(std::isfinite(mid) && mid > std::ldexp(1.0, 600), "all tied, side 300: finite and huge, got %.17g", mid);
    }
}

}  // namespace

int main() {
    test_random_batches();
    test_forced_routes();
    test_errors();
    test_chunker_meters();
    test_large_route_work();
    test_single_pair_verdict();
    test_model();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
