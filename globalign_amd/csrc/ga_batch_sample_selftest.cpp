// ga_batch_sample_selftest.cpp -- CPU self-test of the host's share of ga_batch_sample: the sample planner (ga_batch.h
// plan_batch_sample: fill chunks, per-pair slices, walk items and walk launches) and the walks' word address
// (ga_batch_layout.h), plain and under AddressSanitizer + UndefinedBehaviorSanitizer (make -C globalign_amd/csrc
// batch_sample_selftest batch_sample_asan; run by tests/test_batch_sample_host.py).  No HIP: the kernels are tested
// on the GPU.
#include <cstdio>
#include <random>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "ga_batch.h"
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
    std::vector<int64_t> off{0}, sample_off{0};
    std::vector<int32_t> pa, pb;
    int64_t npairs() const { return (int64_t)pa.size(); }
    int64_t nseq() const { return (int64_t)off.size() - 1; }
};

Batch random_batch(std::mt19937& rng, int npairs, int max_len, int max_samples) {
    Batch b;
    for (int k = 0; k < npairs; k++) {
        for (int side = 0; side < 2; side++) {
            // one-letter sequences now and then: they leave the kernel route
            const int64_t len = rng() % 9 == 0 ? 1 : 2 + (int64_t)(rng() % (unsigned)(max_len - 1));
            b.codes.insert(b.codes.end(), (size_t)len, (uint8_t)(rng() % 4));
            b.off.push_back((int64_t)b.codes.size());
        }
        b.pa.push_back(2 * k);
        b.pb.push_back(2 * k + 1);
        b.sample_off.push_back(b.sample_off.back() + (int64_t)(rng() % (unsigned)(max_samples + 1)));
    }
    return b;
}

// every invariant of a sample plan, and its routing against plan_batch_align's for the same inputs
void check_plan(const Batch& b, const Tables& t, const SampleLimits& lim, const SamplePlan& p, const char* what) {
    AlignLimits al = lim;
    al.tb_words_cap = lim.chunk_tb_words;
    AlignPlan ap;
    std::string err;
    CHECK(plan_batch_align(b.codes.data(), b.off.data(), b.nseq(), b.pa.data(), b.pb.data(), nullptr, b.npairs(), &t.cs, al,
                           ap, err) == GA_OK, "%s: align plan failed: %s", what, err.c_str());
    CHECK(ap.single == p.single, "%s: the single-path pairs are plan_batch_align's", what);
    CHECK(ap.kernel.size() == p.kernel.size() && ap.CB == p.CB && ap.qbytes == p.qbytes &&
              ap.scratch_rows == p.scratch_rows, "%s: the kernel pairs are plan_batch_align's", what);
    for (size_t q = 0; q < p.kernel.size() && q < ap.kernel.size(); q++) {
        const ga_batch_item &x = p.kernel[q], &y = ap.kernel[q];
        CHECK(x.a_off == y.a_off && x.m == y.m && x.b_off == y.b_off && x.n == y.n && x.big == y.big && x.out == y.out &&
                  x.T == y.T && x.nstripes == y.nstripes, "%s: work item %zu is plan_batch_align's", what, q);
    }
    CHECK(p.words.size() == p.kernel.size(), "%s: one slice per kernel pair", what);
    // every kernel pair in exactly one chunk; slices disjoint, side by side, inside the cap
    std::vector<int> seen(p.kernel.size(), 0);
    int64_t next_pair = 0, next_launch = 0, next_walk = 0;
    for (const FillChunk& ch : p.chunks) {
        CHECK(ch.first == next_pair && ch.count > 0, "%s: chunks follow each other", what);
        CHECK(ch.tb_words <= lim.chunk_tb_words, "%s: a chunk's slices stay within the cap", what);
        int64_t off = 0;
        for (int64_t q = ch.first; q < ch.first + ch.count && q < (int64_t)p.kernel.size(); q++) {
            seen[(size_t)q]++;
            const ga_batch_item& it = p.kernel[(size_t)q];
            const ga_batch_words_item& ws = p.words[(size_t)q];
            CHECK(ws.tb_off == off && ws.tb_words == tb_slice_words(it.m, it.T, it.nstripes, p.CB),
                  "%s: slice of work item %lld", what, (long long)q);
            CHECK(ws.tb_words * 4 >= (int64_t)it.m * it.n * p.CB, "%s: slice holds work item %lld", what, (long long)q);
            off += ws.tb_words;
        }
        CHECK(off == ch.tb_words, "%s: a chunk's words are its slices", what);
        next_pair = ch.first + ch.count;
        // its walk launches: items of this chunk's pairs only, in pair and sample order, ranges disjoint and in order
        CHECK(ch.launch_first == next_launch, "%s: walk launches follow each other", what);
        std::vector<std::pair<int64_t, int64_t>> want_seq;  // (fill item, flat sample): pair order, then sample order
        for (int64_t q = ch.first; q < ch.first + ch.count && q < (int64_t)p.kernel.size(); q++)
            for (int64_t f = b.sample_off[(size_t)p.kernel[(size_t)q].out]; f < b.sample_off[(size_t)p.kernel[(size_t)q].out + 1]; f++)
                want_seq.emplace_back(q - ch.first, f);
        size_t pos = 0;
        for (int64_t L = ch.launch_first; L < ch.launch_first + ch.launch_count && L < (int64_t)p.launches.size(); L++) {
            const WalkLaunch& wl = p.launches[(size_t)L];
            CHECK(wl.first == next_walk && wl.count > 0, "%s: walk items follow each other", what);
            CHECK(wl.tab_entries <= lim.walk_entries || wl.count == 1, "%s: a walk launch stays within its cap", what);
            int64_t tab = 0, ops = 0;
            for (int64_t w = wl.first; w < wl.first + wl.count && w < (int64_t)p.walk.size(); w++) {
                const ga_batch_sample_item& wi = p.walk[(size_t)w];
                CHECK(wi.fill >= 0 && wi.fill < ch.count, "%s: a walk item points at a fill item of its chunk", what);
                if (wi.fill < 0 || wi.fill >= ch.count) continue;
                const ga_batch_item& it = p.kernel[(size_t)(ch.first + wi.fill)];
                CHECK(wi.tab_off == tab && wi.ops_off == ops, "%s: table and level ranges of walk %lld", what, (long long)w);
                tab += (int64_t)it.m + it.n;
                ops += ((int64_t)it.m + it.n + 15) / 16;
                CHECK(pos < want_seq.size() && wi.fill == want_seq[pos].first && wi.out == want_seq[pos].second,
                      "%s: walk %lld in pair order, then sample order", what, (long long)w);
                pos++;
            }
            CHECK(tab == wl.tab_entries && ops == wl.ops_words, "%s: a walk launch's totals", what);
            next_walk = wl.first + wl.count;
        }
        CHECK(pos == want_seq.size(), "%s: every sample of the chunk's pairs is walked", what);
        next_launch = ch.launch_first + ch.launch_count;
    }
    for (size_t q = 0; q < seen.size(); q++) CHECK(seen[q] == 1, "%s: work item %zu sits in exactly one chunk", what, q);
    CHECK(next_launch == (int64_t)p.launches.size() && next_walk == (int64_t)p.walk.size(), "%s: nothing is left over", what);
    // every sample of every kernel pair is walked exactly once
    std::set<int32_t> outs;
    for (const ga_batch_sample_item& wi : p.walk) outs.insert(wi.out);
    int64_t want = 0;
    for (const ga_batch_item& it : p.kernel) want += b.sample_off[(size_t)it.out + 1] - b.sample_off[(size_t)it.out];
    CHECK((int64_t)outs.size() == want && (int64_t)p.walk.size() == want, "%s: one walk per sample", what);
}

int plan(const Batch& b, const Tables& t, const SampleLimits& lim, SamplePlan& p, std::string& err) {
    return plan_batch_sample(b.codes.data(), b.off.data(), b.nseq(), b.pa.data(), b.pb.data(), nullptr, b.npairs(), &t.cs,
                             b.sample_off.data(), lim, p, err);
}

SampleLimits wide_limits() {
    SampleLimits lim;
    lim.max_cells = 1 << 30;
    lim.scratch_rows_cap = 1 << 20;
    return lim;
}

void test_random_batches() {
    std::mt19937 rng(12);
    for (int round = 0; round < 200; round++) {
        const int open = round % 3 == 0 ? 4 : round % 3 == 1 ? 30 : 200;  // one-, two- and four-byte words
        Tables t(5, 5, 3, open);
        const Batch b = random_batch(rng, 1 + (int)(rng() % 40), 2 + (int)(rng() % 700), (int)(rng() % 6));
        SampleLimits lim = wide_limits();
        if (round % 2) {
            lim.max_cells = 1 + (int64_t)(rng() % 200000);
            lim.chunk_tb_words = 64 + (int64_t)(rng() % 100000);
            lim.walk_entries = 1 + (int64_t)(rng() % 3000);
        }
        SamplePlan p;
        std::string err;
        CHECK(plan(b, t, lim, p, err) == GA_OK, "round %d: plan failed: %s", round, err.c_str());
        check_plan(b, t, lim, p, ("round " + std::to_string(round)).c_str());
    }
}

void test_forced_caps() {
    Tables t(5, 5, 3, 4);
    Batch b;
    for (int k = 0; k < 5; k++) {
        for (int side = 0; side < 2; side++) {
            b.codes.insert(b.codes.end(), (size_t)(40 + 10 * k + side), 1);
            b.off.push_back((int64_t)b.codes.size());
        }
        b.pa.push_back(2 * k);
        b.pb.push_back(2 * k + 1);
        b.sample_off.push_back(b.sample_off.back() + 5);
    }
    SamplePlan p;
    std::string err;
    SampleLimits lim = wide_limits();
    CHECK(plan(b, t, lim, p, err) == GA_OK, "plan failed: %s", err.c_str());
    CHECK(p.chunks.size() == 1 && p.launches.size() == 1 && p.walk.size() == 25 && p.single.empty(),
          "the defaults: one chunk, one walk launch");
    check_plan(b, t, lim, p, "defaults");
    // tiny caps: a chunk holds two of the pairs at most, a walk launch a few walks
    lim.chunk_tb_words = 2 * tb_slice_words(80, 2, 1, 1);
    lim.walk_entries = 500;
    CHECK(plan(b, t, lim, p, err) == GA_OK, "plan failed: %s", err.c_str());
    CHECK(p.chunks.size() > 1 && p.launches.size() > p.chunks.size() && p.kernel.size() == 5 && p.walk.size() == 25,
          "tiny caps give %zu chunks and %zu walk launches", p.chunks.size(), p.launches.size());
    check_plan(b, t, lim, p, "tiny caps");
    // a pair whose own slice exceeds the chunk cap leaves the kernel route
    lim.chunk_tb_words = tb_slice_words(80, 2, 1, 1) - 1;
    CHECK(plan(b, t, lim, p, err) == GA_OK, "plan failed: %s", err.c_str());
    CHECK(p.single == std::vector<int64_t>{4} && p.kernel.size() == 4, "a slice over the cap goes to the single path");
    check_plan(b, t, lim, p, "slice over the cap");
    // a walk above the launch cap gets a launch of its own
    lim = wide_limits();
    lim.walk_entries = 10;
    CHECK(plan(b, t, lim, p, err) == GA_OK, "plan failed: %s", err.c_str());
    CHECK(p.launches.size() == 25, "one launch per walk, got %zu", p.launches.size());
    check_plan(b, t, lim, p, "walks over the cap");
}

void test_errors() {
    Tables t(5, 5, 3, 4);
    Batch b;
    b.codes.assign(20, 0);
    b.off = {0, 10, 20};
    b.pa = {0};
    b.pb = {1};
    SamplePlan p;
    std::string err;
    b.sample_off = {1, 2};
    CHECK(plan(b, t, wide_limits(), p, err) == GA_E_ARG, "sample_off must start at 0");
    b.sample_off = {0, -1};
    CHECK(plan(b, t, wide_limits(), p, err) == GA_E_ARG, "sample_off must not decrease");
    CHECK(plan_batch_sample(b.codes.data(), b.off.data(), 2, b.pa.data(), b.pb.data(), nullptr, 1, &t.cs, nullptr,
                            wide_limits(), p, err) == GA_E_ARG, "null sample_off");
    // the pairs' own errors come first, as plan_batch_align gives them
    b.codes[3] = 9;
    b.sample_off = {1, 2};
    CHECK(plan(b, t, wide_limits(), p, err) == GA_E_ARG && err == "pair 0: seq_1 code out of range", "got: %s", err.c_str());
    // no pairs, no samples
    CHECK(plan_batch_sample(nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, &t.cs, nullptr, wide_limits(), p, err) == GA_OK &&
              p.chunks.empty() && p.walk.empty(), "an empty batch plans to nothing");
    // a pair without samples is still filled
    b.codes[3] = 0;
    b.sample_off = {0, 0};
    CHECK(plan(b, t, wide_limits(), p, err) == GA_OK && p.kernel.size() == 1 && p.chunks.size() == 1 &&
              p.chunks[0].launch_count == 0 && p.walk.empty(), "a pair without samples");
}

// LAYOUT_STRIPE against the single-pair fills' formula (ga_device.h): byte
// ((s * TC + q) * 64 + l) * 16 + ((i - 1) % SPC) * CB; LAYOUT_BATCH against ga_batch.h's
template <int CB>
void test_layout() {
    const int SPC = 16 / CB, RPW = 4 / CB;
    for (const int m : {2, SPC - 1, SPC, SPC + 1, 4 * SPC, 4 * SPC + 1, 1000}) {
        const int TC = (m + SPC - 1) / SPC;
        std::set<long long> bytes;
        for (const int j : {1, 2, 63, 64, 65, 127, 128, 129, 640, 641}) {
            for (int i = 1; i <= m; i++) {
                const long long s = (j - 1) / 64, l = (j - 1) % 64, q = (i - 1) / SPC;
                const long long want = ((s * TC + q) * 64 + l) * 16 + ((i - 1) % SPC) * CB;
                const unsigned long long w = TbAddr<CB, LAYOUT_STRIPE>::word(i, j, TC);
                const int sh = TbAddr<CB, LAYOUT_STRIPE>::shift(i);
                CHECK((long long)w * 4 + sh / 8 == want, "stripe layout, CB %d: cell (%d, %d) at TC %d", CB, i, j, TC);
                CHECK(sh % (8 * CB) == 0 && sh + 8 * CB <= 32, "stripe layout, CB %d: a cell lies inside one dword", CB);
                CHECK((long long)w < stripe_words(641, TC), "stripe layout, CB %d: cell (%d, %d) inside the words", CB, i, j);
                CHECK(bytes.insert(want).second, "stripe layout, CB %d: no two cells share bytes", CB);
            }
        }
        for (const int n : {2, 64, 65, 300, 513}) {
            int T, nstripes;
            stripe_geometry(n, T, nstripes);
            const int pitch = 64 * T * nstripes;
            for (const int i : {1, std::min(RPW, m), std::min(RPW + 1, m), m})
                for (const int j : {1, n}) {
                    const unsigned long long w = TbAddr<CB, LAYOUT_BATCH>::word(i, j, pitch);
                    const int sh = TbAddr<CB, LAYOUT_BATCH>::shift(i);
                    CHECK((long long)w == (long long)((i - 1) / RPW) * pitch + (j - 1) && sh == ((i - 1) % RPW) * 8 * CB &&
                              (long long)w < tb_slice_words(m, T, nstripes, CB),
                          "batch layout, CB %d: cell (%d, %d)", CB, i, j);
                }
        }
    }
}

}  // namespace

int main() {
    test_random_batches();
    test_forced_caps();
    test_errors();
    test_layout<1>();
    test_layout<2>();
    test_layout<4>();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
