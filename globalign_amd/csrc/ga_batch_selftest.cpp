// ga_batch_selftest.cpp -- CPU self-test of the batch planner (ga_batch.h), plain and under AddressSanitizer +
// UndefinedBehaviorSanitizer (make -C globalign_amd/csrc batch_selftest batch_asan; run by tests/test_batch_host.py):
// the work list's order, the routing rule at its edges, the scratch sizing, the per-pair range guard, the first
// failing pair, empty and one-pair batches, the largest sequence indices.
// No HIP: the kernel is tested on the GPU; this binary covers the host logic under the sanitizers.
#include <cstdio>
#include <string>
#include <vector>

#include "ga_batch.h"

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

// sequences of the given lengths (code 0 everywhere) and their offsets
struct Seqs {
    std::vector<uint8_t> codes;
    std::vector<int64_t> off{0};
    explicit Seqs(const std::vector<int64_t>& lens) {
        for (int64_t L : lens) {
            codes.insert(codes.end(), (size_t)L, 0);
            off.push_back((int64_t)codes.size());
        }
        if (codes.empty()) codes.push_back(0);  // a non-null pointer for an all-empty list
    }
    int64_t n() const { return (int64_t)off.size() - 1; }
};

int plan(const Seqs& sq, const std::vector<int32_t>& pa, const std::vector<int32_t>& pb, const Tables& t,
         const Limits& lim, Plan& out, std::string& err) {
    return plan_batch(sq.codes.data(), sq.off.data(), sq.n(), pa.data(), pb.data(), nullptr, (int64_t)pa.size(), &t.cs, lim,
                      out, err);
}

void test_order_and_geometry() {
    Tables t(5, 5, 3, 4);
    // lengths 10, 20, 20, 10, 300, 513: cells of pairs (s, s)
    Seqs sq({10, 20, 20, 10, 300, 513});
    std::vector<int32_t> pa{0, 1, 2, 3, 4, 5, 0}, pb{0, 1, 2, 3, 4, 5, 3};
    Limits lim;
    lim.max_cells = 1 << 30;
    lim.scratch_rows_cap = 1 << 20;
    Plan p;
    std::string err;
    CHECK(plan(sq, pa, pb, t, lim, p, err) == GA_OK, "plan failed: %s", err.c_str());
    CHECK(p.single.empty(), "nothing routes to the single-pair fill");
    const std::vector<int> want{5, 4, 1, 2, 0, 3, 6};  // cells descending, ties in input order
    CHECK(p.kernel.size() == want.size(), "work list size %zu", p.kernel.size());
    for (size_t k = 0; k < want.size() && k < p.kernel.size(); k++)
        CHECK(p.kernel[k].out == want[k], "work item %zu is pair %d, want %d", k, p.kernel[k].out, want[k]);
    for (const ga_batch_item& it : p.kernel) {
        CHECK(it.m == sq.off[pa[it.out] + 1] - sq.off[pa[it.out]] && it.a_off == sq.off[pa[it.out]], "seq_1 of %d", it.out);
        CHECK(it.n == sq.off[pb[it.out] + 1] - sq.off[pb[it.out]] && it.b_off == sq.off[pb[it.out]], "seq_2 of %d", it.out);
        CHECK(it.big == (5 + 1) * std::max(it.m, it.n), "big of %d", it.out);
        CHECK(it.T >= 1 && it.T <= kMaxT && (int64_t)64 * it.T * it.nstripes >= it.n, "stripes cover n of %d", it.out);
        CHECK(it.nstripes == 1 || (int64_t)64 * kMaxT * (it.nstripes - 1) < it.n, "fewest stripes of %d", it.out);
    }
    CHECK(p.kernel[1].T == 5 && p.kernel[1].nstripes == 1, "300 columns are one pass at T = 5");
    CHECK(p.kernel[0].T == 5 && p.kernel[0].nstripes == 2, "513 columns: two stripes, T = %d", p.kernel[0].T);
    CHECK(p.scratch_rows == 0, "every m fits LDS: no scratch, got %lld", (long long)p.scratch_rows);
    int T, ns;
    stripe_geometry(1, T, ns);
    CHECK(T == 1 && ns == 1, "1 column");
    stripe_geometry(64, T, ns);
    CHECK(T == 1 && ns == 1, "64 columns");
    stripe_geometry(65, T, ns);
    CHECK(T == 2 && ns == 1, "65 columns");
    stripe_geometry(512, T, ns);
    CHECK(T == 8 && ns == 1, "512 columns");
    stripe_geometry(5000, T, ns);
    CHECK(T == 8 && ns == 10, "5000 columns: T %d x %d", T, ns);
}

void test_routing() {
    Tables t(5, 5, 3, 4);
    Seqs sq({100, 200, 201, 2000, 600, 1024, 1025});
    Plan p;
    std::string err;
    Limits lim;
    lim.scratch_rows_cap = 1500;
    // the threshold's edges: cells == max_cells stays in the kernel, one more leaves it
    lim.max_cells = 100 * 200;
    std::vector<int32_t> pa{0, 0, 1}, pb{1, 2, 0};
    CHECK(plan(sq, pa, pb, t, lim, p, err) == GA_OK, "plan failed: %s", err.c_str());
    CHECK(p.kernel.size() == 2 && p.single.size() == 1 && p.single[0] == 1, "100 x 201 alone exceeds 20000 cells");
    CHECK(p.kernel[0].out == 0 && p.kernel[1].out == 2, "ties keep input order");
    // 0: everything to the single-pair fill, longest first
    lim.max_cells = 0;
    CHECK(plan(sq, pa, pb, t, lim, p, err) == GA_OK, "plan failed: %s", err.c_str());
    CHECK(p.kernel.empty() && p.single.size() == 3 && p.single[0] == 1, "max_cells 0 sends all to the single-pair fill");
    // edge scratch: needed only with a second stripe and more rows than LDS holds; refused above the cap
    lim.max_cells = 1ll << 40;
    pa = {5, 6, 6, 3, 3};
    pb = {4, 4, 0, 4, 0};
    CHECK(plan(sq, pa, pb, t, lim, p, err) == GA_OK, "plan failed: %s", err.c_str());
    // 1024 x 600: LDS.  1025 x 600: scratch, 1025 rows.  1025 x 100: one stripe, none.  2000 x 600: above the cap
    // of 1500 rows -> single.  2000 x 100: one stripe, kernel.
    CHECK(p.single.size() == 1 && p.single[0] == 3, "2000 x 600 needs more scratch than planned");
    CHECK(p.kernel.size() == 4, "four pairs stay, got %zu", p.kernel.size());
    CHECK(p.scratch_rows == 1025, "scratch rows %lld", (long long)p.scratch_rows);
    CHECK(needs_scratch(1025, 513) && !needs_scratch(1024, 513) && !needs_scratch(1025, 512), "needs_scratch edges");
    lim.scratch_rows_cap = 2000;
    CHECK(plan(sq, pa, pb, t, lim, p, err) == GA_OK && p.single.empty() && p.scratch_rows == 2000, "cap 2000 admits it");
    CHECK(scratch_rows_cap(2048) * 2048 * 16 <= kScratchBytesCap && scratch_rows_cap(2048) >= 4096, "scratch cap");
    // a table too large for LDS sends every pair to the single-pair fill
    Tables wide(200, 5, 3, 4);
    CHECK(!table_fits_lds(200, 1) && table_fits_lds(128, 1) && table_fits_lds(90, 2) && !table_fits_lds(91, 2),
          "table budget");
    pa = {0};
    pb = {1};
    CHECK(plan(sq, pa, pb, wide, lim, p, err) == GA_OK && p.kernel.empty() && p.single.size() == 1, "K = 200 routes out");
    // an int16 profile is reported
    Tables w16(5, 300, 3, 4);
    CHECK(plan(sq, pa, pb, w16, lim, p, err) == GA_OK && p.qbytes == 2, "int16 profile");
    CHECK(plan(sq, pa, pb, t, lim, p, err) == GA_OK && p.qbytes == 1, "int8 profile");
    // beyond int16 the kernel's table has 4-byte entries, and fits LDS up to K = 64
    Tables w32(5, 1000000, 3, 4);
    Seqs tiny({3, 4});
    CHECK(plan(tiny, pa, pb, w32, lim, p, err) == GA_OK && p.qbytes == 4 && p.kernel.size() == 1, "int32 table");
    CHECK(table_fits_lds(64, 4) && !table_fits_lds(65, 4), "int32 table budget");
}

void test_range_and_errors() {
    // mismatch 10^6, open 1, extension 1: 3 x 3 is in range, 100 x 100 is not (big = 10^8 and 202 * 3 * 10^6 give a
    // bound of 7 * 10^8; four times that exceeds 2^31), each judged with its own big
    Tables t(5, 1000000, 1, 1);
    Seqs sq({3, 100, 0});
    Limits lim;
    lim.scratch_rows_cap = 4096;
    Plan p;
    std::string err;
    std::vector<int32_t> pa{0, 1}, pb{0, 1};
    CHECK(plan(sq, pa, pb, t, lim, p, err) == GA_E_RANGE, "100 x 100 is out of range");
    CHECK(err.rfind("pair 1: ", 0) == 0, "message names pair 1: %s", err.c_str());
    CHECK(p.kernel.empty() && p.single.empty(), "a failed plan is empty");
    pa = {0};
    pb = {0};
    CHECK(plan(sq, pa, pb, t, lim, p, err) == GA_OK && p.kernel.size() == 1, "3 x 3 alone is in range: %s", err.c_str());
    CHECK(!p.kernel.empty() && p.kernel[0].big == 1000001 * 3, "its own big");
    CHECK(p.qbytes == 4, "sub' of 10^6 takes 4-byte entries");
    // agreement with check_problem on both
    ProblemShape ps;
    std::string why;
    std::vector<uint8_t> z(100, 0);
    int64_t big = 0;
    CHECK(check_pair_range(3, 3, &t.cs, t.cs.max_cost, costs_maxabs(&t.cs), big) == GA_OK && big == 3000003, "range of 3 x 3");
    CHECK(check_pair_range(100, 100, &t.cs, t.cs.max_cost, costs_maxabs(&t.cs), big) == GA_E_RANGE, "range of 100 x 100");
    CHECK(check_problem(z.data(), 100, z.data(), 100, &t.cs, nullptr, nullptr, 0, 100, ps, why) == GA_E_RANGE &&
              why == "problem exceeds the int32 score range of the device path",
          "single 100 x 100: %s", why.c_str());
    Tables mild(5, 10000, 1, 1);  // within the int16 profile: both checks agree at the guard's edge
    for (int64_t L : {100, 1000, 5000, 10000, 20000, 50000}) {
        const int single = check_problem(z.data(), 1, z.data(), 1, &mild.cs, nullptr, nullptr, 0, 1, ps, why);
        CHECK(single == GA_OK, "1 x 1");
        std::vector<uint8_t> zz((size_t)L, 0);
        const int want = check_problem(zz.data(), L, zz.data(), L, &mild.cs, nullptr, nullptr, 0, L, ps, why);
        CHECK(check_pair_range(L, L, &mild.cs, mild.cs.max_cost, costs_maxabs(&mild.cs), big) == want, "guard agrees at %lld", (long long)L);
    }
    // the first failing pair in input order, whatever fails later
    pa = {0, 0, 1, 0};
    pb = {0, 2, 1, 7};
    CHECK(plan(sq, pa, pb, t, lim, p, err) == GA_E_ARG && err.rfind("pair 1: ", 0) == 0, "empty sequence first: %s",
          err.c_str());
    pa = {0, 0};
    pb = {0, 3};
    CHECK(plan(sq, pa, pb, t, lim, p, err) == GA_E_ARG && err.rfind("pair 1: ", 0) == 0, "index past the last: %s",
          err.c_str());
    pb = {0, -1};
    CHECK(plan(sq, pa, pb, t, lim, p, err) == GA_E_ARG, "negative index");
    // a code outside the alphabet fails the first pair that uses its sequence
    Tables d(5, 5, 3, 4);
    Seqs bad({4, 4, 4});
    bad.codes[9] = 5;
    pa = {0, 1, 2};
    pb = {1, 0, 0};
    CHECK(plan(bad, pa, pb, d, lim, p, err) == GA_E_ARG && err == "pair 2: seq_1 code out of range", "bad code: %s",
          err.c_str());
    pb = {1, 2, 0};
    CHECK(plan(bad, pa, pb, d, lim, p, err) == GA_E_ARG && err == "pair 1: seq_2 code out of range", "bad code: %s",
          err.c_str());
    // null tables, bad alphabet, negative gap open
    ga_costs cs = d.cs;
    cs.sub = nullptr;
    CHECK(plan_batch(bad.codes.data(), bad.off.data(), 3, pa.data(), pb.data(), nullptr, 3, &cs, lim, p, err) == GA_E_ARG, "null sub");
    cs = d.cs;
    cs.gap_open = -1;
    CHECK(plan_batch(bad.codes.data(), bad.off.data(), 3, pa.data(), pb.data(), nullptr, 3, &cs, lim, p, err) == GA_E_ARG, "open < 0");
    cs = d.cs;
    cs.K = 0;
    CHECK(plan_batch(bad.codes.data(), bad.off.data(), 3, pa.data(), pb.data(), nullptr, 3, &cs, lim, p, err) == GA_E_ARG, "K = 0");
}

void test_pair_max_cost() {
    // a max_cost per pair: the pair's own big, in the work list and in the range guard
    Tables t(5, 5, 3, 4);
    Seqs sq({3, 2, 4});
    Limits lim;
    lim.scratch_rows_cap = 4096;
    Plan p;
    std::string err;
    std::vector<int32_t> pa{0, 0, 2}, pb{1, 1, 2}, mc{5, 3, 3};
    CHECK(plan_batch(sq.codes.data(), sq.off.data(), sq.n(), pa.data(), pb.data(), mc.data(), 3, &t.cs, lim, p, err) ==
              GA_OK && p.kernel.size() == 3,
          "plan with per-pair max_cost: %s", err.c_str());
    for (const ga_batch_item& it : p.kernel)
        CHECK(it.big == (mc[(size_t)it.out] + 1) * std::max(it.m, it.n), "pair %d: big %d", it.out, it.big);
    // the guard uses the pair's max_cost: at mismatch 10^6 an 80 x 80 pair has a bound of 4.86e8 + big, in range
    // (below 2^31 / 4 = 5.37e8) with a one-letter matrix's big of 160 and out of it with big = 8e7
    Tables wide(5, 1000000, 1, 1);
    Seqs sq2({80});
    pa = {0, 0};
    pb = {0, 0};
    mc = {1, 1000000};
    CHECK(plan_batch(sq2.codes.data(), sq2.off.data(), 1, pa.data(), pb.data(), mc.data(), 2, &wide.cs, lim, p, err) ==
              GA_E_RANGE && err.rfind("pair 1: ", 0) == 0,
          "pair 1 alone is out of range: %s", err.c_str());
}

void test_small_and_large() {
    Tables t(5, 5, 3, 4);
    Limits lim;
    lim.scratch_rows_cap = 4096;
    Plan p;
    std::string err;
    // no pairs: an empty plan, whatever else is passed
    CHECK(plan_batch(nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, lim, p, err) == GA_OK && p.kernel.empty() &&
              p.single.empty(),
          "0 pairs");
    Seqs one({7});
    std::vector<int32_t> pa{0}, pb{0};
    CHECK(plan(one, pa, pb, t, lim, p, err) == GA_OK && p.kernel.size() == 1 && p.kernel[0].out == 0 &&
              p.kernel[0].m == 7 && p.kernel[0].n == 7 && p.kernel[0].a_off == 0,
          "1 pair");
    // many sequences, the last ones used: offsets and indices at the top of the list
    std::vector<int64_t> lens(5000);
    for (size_t s = 0; s < lens.size(); s++) lens[s] = 1 + (int64_t)(s % 37);
    Seqs many(lens);
    pa.clear();
    pb.clear();
    for (int k = 0; k < 5000; k++) {
        pa.push_back(4999 - k);
        pb.push_back(k == 0 ? 4999 : 4999 - k / 2);
    }
    CHECK(plan(many, pa, pb, t, lim, p, err) == GA_OK && p.kernel.size() == 5000, "5000 pairs: %s", err.c_str());
    std::vector<char> seen(5000, 0);
    int64_t prev = INT64_MAX;
    for (const ga_batch_item& it : p.kernel) {
        CHECK(it.out >= 0 && it.out < 5000 && !seen[(size_t)it.out], "each pair once");
        seen[(size_t)it.out] = 1;
        CHECK((int64_t)it.a_off + it.m <= many.off.back() && (int64_t)it.b_off + it.n <= many.off.back(), "in bounds");
        CHECK(it.a_off == many.off[pa[it.out]] && it.b_off == many.off[pb[it.out]], "offsets of pair %d", it.out);
        const int64_t cells = (int64_t)it.m * it.n;
        CHECK(cells <= prev, "descending");
        prev = cells;
    }
}

}  // namespace

int main() {
    test_order_and_geometry();
    test_routing();
    test_range_and_errors();
    test_pair_max_cost();
    test_small_and_large();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
