// ga_batch_align_selftest.cpp -- CPU self-test of the host's share of ga_batch_align: the align planner (ga_batch.h
// plan_batch_align), the table jobs' split and build and the levels-to-strings decode (ga_batch_align.h's decode_walk /
// decode_levels and, under them and under every single-pair walk, ga_strings.h's resumable decoder), plain, under
// AddressSanitizer + UndefinedBehaviorSanitizer and -- for the threaded table build -- under ThreadSanitizer
// (make -C globalign_amd/csrc batch_align_selftest batch_align_asan batch_align_tsan; run by
// tests/test_batch_align_host.py).  No HIP: the kernel is tested on the GPU.
#include <cstdio>
#include <string>
#include <vector>

#include "ga_batch_align.h"

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
    }
    int64_t n() const { return (int64_t)off.size() - 1; }
};

AlignLimits wide_limits() {
    AlignLimits lim;
    lim.max_cells = 1 << 30;
    lim.scratch_rows_cap = 1 << 20;
    lim.tb_words_cap = (int64_t)1 << 40;
    return lim;
}

int plan(const Seqs& sq, const std::vector<int32_t>& pa, const std::vector<int32_t>& pb, const Tables& t,
         const AlignLimits& lim, AlignPlan& out, std::string& err) {
    return plan_batch_align(sq.codes.data(), sq.off.data(), sq.n(), pa.data(), pb.data(), nullptr, (int64_t)pa.size(),
                            &t.cs, lim, out, err);
}

void test_routing_and_order() {
    Tables t(5, 5, 3, 4);
    Seqs sq({1, 2, 40, 300, 513, 1, 90});
    //                        1x2   2x1   2x2   40x300 513x513 1x1   90x40  300x2
    std::vector<int32_t> pa{0, 1, 1, 2, 4, 5, 6, 3}, pb{1, 0, 1, 3, 4, 5, 2, 1};
    AlignPlan p;
    std::string err;
    CHECK(plan(sq, pa, pb, t, wide_limits(), p, err) == GA_OK, "plan failed: %s", err.c_str());
    // a sequence of one letter: the single-pair path, whatever the other side
    const std::vector<int64_t> want_single{0, 1, 5};
    CHECK(p.single == want_single, "one-letter pairs route to the single path (%zu do)", p.single.size());
    // the rest in plan_batch's order: the score planner's list without the pairs routed away
    Plan score;
    Limits lim;
    lim.max_cells = 1 << 30;
    lim.scratch_rows_cap = 1 << 20;
    CHECK(plan_batch(sq.codes.data(), sq.off.data(), sq.n(), pa.data(), pb.data(), nullptr, (int64_t)pa.size(), &t.cs, lim,
                     score, err) == GA_OK, "score plan failed");
    size_t q = 0;
    for (const ga_batch_item& it : score.kernel) {
        if (it.m < 2 || it.n < 2) continue;
        CHECK(q < p.kernel.size() && p.kernel[q].out == it.out && p.kernel[q].T == it.T &&
                  p.kernel[q].nstripes == it.nstripes && p.kernel[q].big == it.big, "work item %zu follows plan_batch", q);
        q++;
    }
    CHECK(q == p.kernel.size() && q == 5, "five kernel pairs, got %zu", p.kernel.size());
    CHECK(p.walk.size() == p.kernel.size(), "one walk item per work item");
    // tables and level words: disjoint, in list order, large enough
    int64_t tab = 0, ops = 0, tbw = 0;
    for (size_t k = 0; k < p.kernel.size() && k < p.walk.size(); k++) {
        const ga_batch_item& it = p.kernel[k];
        CHECK(p.walk[k].tab_off == tab && p.walk[k].ops_off == ops, "offsets of work item %zu", k);
        tab += it.m + it.n;
        ops += (it.m + it.n + 15) / 16;
        tbw = std::max(tbw, tb_slice_words(it.m, it.T, it.nstripes, p.CB));
        CHECK(tb_slice_words(it.m, it.T, it.nstripes, p.CB) * 4 >= (int64_t)it.m * it.n * p.CB, "slice holds item %zu", k);
    }
    CHECK(p.tab_entries == tab && p.ops_words == ops && p.tb_words == tbw, "totals");
    CHECK(p.CB == 1, "gap open 4: one-byte words");
    // plan_batch itself still takes one-letter pairs
    CHECK(score.kernel.size() == pa.size() && score.single.empty(), "plan_batch is unchanged");
}

void test_limits() {
    Tables t(5, 5, 3, 4);
    Seqs sq({100, 101});
    std::vector<int32_t> pa{0, 1, 0}, pb{0, 1, 1};  // 10000, 10201, 10100 cells
    AlignPlan p;
    std::string err;
    AlignLimits lim = wide_limits();
    lim.max_cells = 10100;
    CHECK(plan(sq, pa, pb, t, lim, p, err) == GA_OK, "plan failed: %s", err.c_str());
    CHECK(p.single == std::vector<int64_t>{1} && p.kernel.size() == 2, "the cells limit is inclusive");
    lim.max_cells = 0;
    CHECK(plan(sq, pa, pb, t, lim, p, err) == GA_OK && p.kernel.empty() && p.single.size() == 3, "limit 0: all single");
    CHECK(p.tab_entries == 0 && p.ops_words == 0 && p.tb_words == 0, "no kernel pair: no buffers");
    // the traceback scratch cap: 100 rows of 128 padded columns, 4 rows to a u32 = 25 * 128 words
    lim = wide_limits();
    CHECK(tb_slice_words(100, 2, 1, 1) == 25 * 128 && tb_slice_words(101, 2, 1, 1) == 26 * 128, "slice words");
    CHECK(tb_slice_words(101, 2, 1, 2) == 51 * 128 && tb_slice_words(101, 2, 1, 4) == 101 * 128, "slice words by CB");
    lim.tb_words_cap = 25 * 128;
    CHECK(plan(sq, pa, pb, t, lim, p, err) == GA_OK, "plan failed: %s", err.c_str());
    CHECK(p.kernel.size() == 2 && p.single == std::vector<int64_t>{1}, "101 rows exceed a 25-row-word share");
    CHECK(p.tb_words == 25 * 128, "the scratch is sized by the largest kernel pair");
    lim.tb_words_cap = 25 * 128 - 1;
    CHECK(plan(sq, pa, pb, t, lim, p, err) == GA_OK && p.kernel.empty(), "one word short: none fits");
    CHECK(tb_slice_words_cap(2048) * 4 * 2048 == kTbScratchBytesCap, "a wave's share of the cap");
}

void test_word_widths() {
    Seqs sq({10});
    std::vector<int32_t> pa{0}, pb{0};
    const int opens[] = {0, 6, 7, 126, 127, 300, 32766};
    const int want[] = {1, 1, 2, 2, 4, 4, 4};
    for (int q = 0; q < 7; q++) {
        Tables t(5, 5, 3, opens[q]);
        AlignPlan p;
        std::string err;
        CHECK(plan(sq, pa, pb, t, wide_limits(), p, err) == GA_OK, "plan failed: %s", err.c_str());
        CHECK(p.CB == want[q] && p.CB == tb_word_bytes(opens[q]), "gap open %d: CB %d", opens[q], p.CB);
    }
    Tables t(5, 5, 3, 32767);
    AlignPlan p;
    std::string err;
    CHECK(plan(sq, pa, pb, t, wide_limits(), p, err) == GA_E_RANGE && err.find("pair 0") == 0, "gap open 32767: %s",
          err.c_str());
    // errors are plan_batch's: the first failing pair in input order
    Seqs two({3, 0});
    Tables ok(5, 5, 3, 4);
    std::vector<int32_t> a2{0, 1}, b2{0, 0};
    CHECK(plan(two, a2, b2, ok, wide_limits(), p, err) == GA_E_ARG && err == "pair 1: sequences must be non-empty", "%s",
          err.c_str());
}

// decode_levels against a character-by-character restatement of the reference's loop and tails
void reference_strings(const std::vector<int>& lv, const std::string& a, const std::string& b, int reason,
                       std::string& oa, std::string& om, std::string& ob, int64_t& i, int64_t& j) {
    i = (int64_t)a.size();
    j = (int64_t)b.size();
    for (int l : lv) {
        if (l == 0) {
            oa += a[i - 1]; ob += b[j - 1]; om += a[i - 1] == b[j - 1] ? '|' : '*';
            i--; j--;
        } else if (l == 1) {
            oa += '-'; om += ' '; ob += b[j - 1];
            j--;
        } else {
            oa += a[i - 1]; om += ' '; ob += '-';
            i--;
        }
    }
    if (reason == 1) for (int64_t jj = j; jj > 0; jj--) { oa += '-'; om += ' '; ob += b[jj - 1]; }
    if (reason == 2) for (int64_t ii = i; ii > 0; ii--) { oa += a[ii - 1]; om += ' '; ob += '-'; }
    oa = std::string(oa.rbegin(), oa.rend());
    om = std::string(om.rbegin(), om.rend());
    ob = std::string(ob.rbegin(), ob.rend());
}

void test_decode() {
    uint64_t x = 0x9e3779b97f4a7c15ull;
    auto next = [&]() {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        return x;
    };
    int tails[3] = {0, 0, 0};
    for (int rep = 0; rep < 400; rep++) {
        const int m = 2 + (int)(next() % 40), n = 2 + (int)(next() % 40);
        std::string a, b;
        for (int k = 0; k < m; k++) a += "ACGT"[next() % 4];
        for (int k = 0; k < n; k++) b += "ACGT"[next() % 4];
        // a random walk from (m, n) to row 0 or column 0, biased so that both tails and the corner occur
        std::vector<int> lv;
        int i = m, j = n;
        const int bias = rep % 3;
        while (i > 0 && j > 0) {
            const int r = (int)(next() % 4);
            const int l = r < 2 ? 0 : bias == 0 ? r - 1 : bias;
            lv.push_back(l);
            i -= l != 1;
            j -= l != 2;
        }
        const int reason = i == 0 ? (j == 0 ? 0 : 1) : 2;
        tails[reason]++;
        std::vector<uint32_t> ops((lv.size() + 15) / 16 + 1, 0xffffffffu);  // (bits past D are never read)
        for (size_t k = 0; k < lv.size(); k++) {
            ops[k >> 4] &= ~(3u << (30 - 2 * (k & 15)));
            ops[k >> 4] |= (uint32_t)lv[k] << (30 - 2 * (k & 15));
        }
        std::string wa, wm, wb;
        int64_t wi, wj;
        reference_strings(lv, a, b, reason, wa, wm, wb, wi, wj);
        const int64_t cap = m + n;
        std::vector<char> oa((size_t)cap), om((size_t)cap), ob((size_t)cap);
        const int64_t len = decode_levels(ops.data(), (int64_t)lv.size(), m, n, i, j, reason, a.data(), b.data(), oa.data(),
                                          om.data(), ob.data(), cap);
        CHECK(len == (int64_t)wa.size(), "length %lld, want %zu", (long long)len, wa.size());
        if (len == (int64_t)wa.size())
            CHECK(std::string(oa.data(), (size_t)len) == wa && std::string(om.data(), (size_t)len) == wm &&
                      std::string(ob.data(), (size_t)len) == wb, "strings of walk %d", rep);
        // too small a buffer, and an end cell the levels do not lead to
        CHECK(decode_levels(ops.data(), (int64_t)lv.size(), m, n, i, j, reason, a.data(), b.data(), oa.data(), om.data(),
                            ob.data(), len - 1) == -1, "capacity");
        CHECK(decode_levels(ops.data(), (int64_t)lv.size(), m, n, i + 1, j, reason, a.data(), b.data(), oa.data(),
                            om.data(), ob.data(), cap) == -2, "end cell");
        // the same walk through decode_walk: sequences side by side in one chars buffer, output slot 1 of two
        const std::string chars = "xyz" + a + b;
        ga_batch_item it{};
        it.a_off = 3;
        it.m = m;
        it.b_off = 3 + m;
        it.n = n;
        const int64_t off[3] = {0, 5, 5 + cap};
        std::vector<char> wa2((size_t)(5 + cap), '?'), wm2(wa2), wb2(wa2);
        int64_t lens[2] = {77, 77};
        int32_t status[2] = {77, 77};
        const WalkOut o{chars.data(), wa2.data(), wm2.data(), wb2.data(), off, lens, status};
        const int32_t wr[4] = {(int32_t)lv.size(), i, j, reason};
        CHECK(decode_walk(it, wr, ops.data(), 1, false, o) == len && lens[1] == len && status[1] == GA_TB_OK,
              "decode_walk's length");
        CHECK(lens[0] == 77 && status[0] == 77 && wa2[4] == '?' && std::string(wa2.data() + 5, (size_t)len) == wa &&
                  std::string(wm2.data() + 5, (size_t)len) == wm && std::string(wb2.data() + 5, (size_t)len) == wb,
              "decode_walk's strings, in its slot only (walk %d)", rep);
        const int32_t end_off[4] = {wr[0], i + 1, j, reason}, neg[4] = {-1, i, j, reason}, past[4] = {m + n + 1, i, j, reason};
        CHECK(decode_walk(it, end_off, ops.data(), 1, false, o) == -2 && lens[1] == -2, "decode_walk: end cell");
        CHECK(decode_walk(it, neg, ops.data(), 1, false, o) == -2 && decode_walk(it, past, ops.data(), 1, false, o) == -2,
              "decode_walk: dispatches outside [0, m + n]");
        CHECK(decode_walk(it, wr, ops.data(), 1, true, o) == -3 && lens[1] == -3 && status[1] == GA_TB_OK,
              "decode_walk: an item that did not fit");
        CHECK(decode_walk(it, neg, ops.data(), 1, true, o) == -3, "decode_walk: did not fit comes first");
    }
    CHECK(tails[0] > 0 && tails[1] > 0 && tails[2] > 0, "corner %d, row-0 %d and column-0 %d endings all occur", tails[0],
          tails[1], tails[2]);
    // a level 3, and levels that run past the matrix edge
    const uint32_t bad = 0xc0000000u, diag[1] = {0};
    char o1[8], o2[8], o3[8];
    CHECK(decode_levels(&bad, 1, 2, 2, 1, 1, 0, "AC", "AC", o1, o2, o3, 8) == -2, "level 3");
    CHECK(decode_levels(diag, 3, 2, 2, 0, 0, 0, "AC", "AC", o1, o2, o3, 8) == -2, "three diagonal steps in a 2 x 2 matrix");
    CHECK(decode_levels(diag, 2, 2, 2, 0, 0, 0, "AC", "AG", o1, o2, o3, 8) == 2 && std::string(o2, 2) == "|*", "2 x 2");
}

// gastr::Columns (ga_strings.h), the decoder every walk of the engine goes through: a piece [D0, D1) out of a word array
// that starts at word D0 >> 4, any chunking, and the lenient mode's Python-style indexing at i == 0 / j == 0.  Letters,
// words and outputs live in heap buffers of exactly the size in use, so AddressSanitizer sees any index outside them.
struct Decoded {
    std::vector<char> oa, om, ob;
    int64_t i, j, len;
    int L;
    bool ok;
    bool operator==(const Decoded& o) const {
        return oa == o.oa && om == o.om && ob == o.ob && i == o.i && j == o.j && len == o.len && L == o.L && ok == o.ok;
    }
};

// dispatches [0, D) of `ops` from (m, n), in the given chunks (chunk <= 0: one call)
template <bool STRICT>
Decoded decode_chunked(const std::vector<uint32_t>& ops, int64_t D, const std::vector<char>& a, const std::vector<char>& b,
                       int64_t cap, int64_t chunk) {
    Decoded d{std::vector<char>((size_t)cap, '?'), std::vector<char>((size_t)cap, '?'), std::vector<char>((size_t)cap, '?'),
              0, 0, 0, 0, true};
    gastr::Columns col{a.data(), (int64_t)a.size(), b.data(), (int64_t)b.size(), d.oa.data(), d.om.data(), d.ob.data(),
                       cap, (int64_t)a.size(), (int64_t)b.size()};
    if (chunk <= 0) chunk = std::max<int64_t>(D, 1);
    for (int64_t k = 0; k < D && d.ok; k += chunk) d.ok = col.decode<STRICT>(ops.data(), 0, k, std::min(D, k + chunk));
    d.i = col.i;
    d.j = col.j;
    d.len = col.len;
    d.L = col.L;
    return d;
}

std::vector<uint32_t> pack_levels(const std::vector<int>& lv) {
    std::vector<uint32_t> ops((lv.size() + 15) / 16, 0xffffffffu);  // (bits past the last dispatch are never read)
    for (size_t k = 0; k < lv.size(); k++) ops[k >> 4] ^= (uint32_t)(3 - lv[k]) << (30 - 2 * (k & 15));
    return ops;
}

void test_columns() {
    uint64_t x = 0x2545f4914f6cdd1dull;
    auto next = [&]() {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        return x;
    };
    int segments = 0;
    for (int rep = 0; rep < 300; rep++) {
        const int m = 2 + (int)(next() % 39), n = 2 + (int)(next() % 39);
        std::vector<char> a((size_t)m), b((size_t)n);
        for (char& ch : a) ch = "ACGT"[next() % 4];
        for (char& ch : b) ch = "ACGT"[next() % 4];
        std::vector<int> lv;
        for (int i = m, j = n; i > 0 && j > 0;) {
            const int r = (int)(next() % 4);
            const int l = r < 2 ? 0 : r - 1;
            lv.push_back(l);
            i -= l != 1;
            j -= l != 2;
        }
        const int64_t D = (int64_t)lv.size();
        const std::vector<uint32_t> ops = pack_levels(lv);
        const Decoded one = decode_chunked<false>(ops, D, a, b, D, 0);
        CHECK(one.ok && one.len == D && one.L == lv.back() && (one.i == 0 || one.j == 0), "one-shot decode of walk %d", rep);
        // a walk inside the matrix decodes alike in both modes
        CHECK(decode_chunked<true>(ops, D, a, b, D, 0) == one, "strict = lenient inside the matrix (walk %d)", rep);
        // chunks of 1, 7, 16 and 17 dispatches: the same strings and end state
        for (int64_t chunk : {1, 7, 16, 17}) {
            CHECK(decode_chunked<false>(ops, D, a, b, D, chunk) == one, "chunks of %lld (walk %d)", (long long)chunk, rep);
            CHECK(decode_chunked<true>(ops, D, a, b, D, chunk) == one, "strict chunks of %lld (walk %d)", (long long)chunk, rep);
        }
        // too small a buffer: len counts on, nothing is written past cap
        const Decoded small = decode_chunked<false>(ops, D, a, b, D - 1, 7);
        CHECK(small.len == D && small.i == one.i && small.j == one.j &&
                  std::equal(small.oa.begin(), small.oa.end(), one.oa.begin()), "capacity (walk %d)", rep);
        // a segment [D0, D1), D0 not a multiple of 16, out of the words from D0 >> 4 on, started at the state the
        // dispatches before D0 leave: the matching slice of the one-shot columns
        if (D < 3) continue;
        int64_t D0 = 1 + (int64_t)(next() % (uint64_t)(D - 1));
        if ((D0 & 15) == 0) D0--;
        const int64_t D1 = D0 + 1 + (int64_t)(next() % (uint64_t)(D - D0));
        int64_t i0 = m, j0 = n;
        for (int64_t k = 0; k < D0; k++) {
            i0 -= lv[(size_t)k] != 1;
            j0 -= lv[(size_t)k] != 2;
        }
        const int64_t w0 = D0 >> 4, w1 = (D1 + 15) >> 4;
        const std::vector<uint32_t> part(ops.begin() + w0, ops.begin() + w1);
        const int64_t cap = D1 - D0;
        std::vector<char> oa((size_t)cap), om((size_t)cap), ob((size_t)cap);
        gastr::Columns col{a.data(), m, b.data(), n, oa.data(), om.data(), ob.data(), cap, i0, j0, lv[(size_t)D0 - 1]};
        CHECK(col.decode<false>(part.data(), w0, D0, D1) && col.len == cap, "segment decode (walk %d)", rep);
        CHECK(std::equal(oa.begin(), oa.end(), one.oa.begin() + D0) && std::equal(om.begin(), om.end(), one.om.begin() + D0) &&
                  std::equal(ob.begin(), ob.end(), one.ob.begin() + D0), "segment [%lld, %lld) of walk %d", (long long)D0,
              (long long)D1, rep);
        segments++;
    }
    CHECK(segments > 250, "segments decoded: %d", segments);
    // Python's seq[-1]: a step taken from i == 0 (j == 0) reads the last letter of seq_1 (seq_2) in lenient mode, as the
    // reference's first step at m == 1 / n == 1 does; strict mode stops there, having read nothing for that step
    for (int side = 0; side < 2; side++)
        for (int m = 1; m <= 5; m++)
            for (int n = 1; n <= 5; n++) {
                std::vector<char> a((size_t)m), b((size_t)n);
                for (int k = 0; k < m; k++) a[(size_t)k] = (char)('a' + k);
                for (int k = 0; k < n; k++) b[(size_t)k] = (char)('p' + k);
                // down column n to row 0 (side 1: along row m to column 0), then one more diagonal step
                std::vector<int> lv((size_t)(side == 0 ? m : n), side == 0 ? 2 : 1);
                lv.push_back(0);
                const int64_t D = (int64_t)lv.size(), edge = D - 1;
                const std::vector<uint32_t> ops = pack_levels(lv);
                // that step, from (0, n) [(m, 0)], pairs the last letters of both sequences: one of them is seq[-1]
                const Decoded py = decode_chunked<false>(ops, D, a, b, D, 0);
                CHECK(py.ok && py.len == D && py.oa[(size_t)edge] == a[(size_t)m - 1] && py.om[(size_t)edge] == '*' &&
                          py.ob[(size_t)edge] == b[(size_t)n - 1], "wrapped step, side %d, %d x %d", side, m, n);
                CHECK(side == 0 ? (py.i == -1 && py.j == n - 1) : (py.i == m - 1 && py.j == -1), "end cell past the edge");
                const Decoded st = decode_chunked<true>(ops, D, a, b, D, 0);
                CHECK(!st.ok && st.len == edge && (side == 0 ? st.i == 0 && st.j == n : st.i == m && st.j == 0),
                      "strict mode stops at the edge, side %d, %d x %d", side, m, n);
                CHECK(std::equal(st.oa.begin(), st.oa.begin() + edge, py.oa.begin()) && st.oa[(size_t)edge] == '?',
                      "strict mode wrote the steps before the edge only");
            }
    // a level 3: level 2 in lenient mode, refused in strict mode
    const std::vector<char> a{'A', 'C'}, b{'G', 'T'};
    const std::vector<uint32_t> three{0xc0000000u};
    const Decoded l3 = decode_chunked<false>(three, 1, a, b, 1, 0);
    CHECK(l3.ok && l3.oa[0] == 'C' && l3.om[0] == ' ' && l3.ob[0] == '-' && l3.i == 1 && l3.j == 2 && l3.L == 3, "lenient level 3");
    CHECK(!decode_chunked<true>(three, 1, a, b, 1, 0).ok, "strict level 3");
}

void test_seed_and_tables() {
    uint32_t st[garng::MTN + 1];
    garng::seed_state(0, st);
    CHECK(st[garng::MTN] == 624, "state index");
    CHECK(st[0] == 2147483648u, "word 0 of every seeded state");
    uint32_t st2[garng::MTN + 1];
    garng::seed_state((uint64_t)1 << 32, st2);
    bool differ = false;
    for (int k = 1; k < garng::MTN; k++) differ |= st[k] != st2[k];
    CHECK(differ, "seed 2^32 (key {0, 1}) differs from seed 0 (key {0})");
    // the threaded build gives the sequential build's tables
    Tables t(5, 5, 3, 4);
    std::vector<int64_t> lens;
    for (int k = 0; k < 300; k++) lens.push_back(2 + (k * 37) % 200);
    Seqs sq(lens);
    std::vector<int32_t> pa, pb;
    std::vector<uint64_t> seeds;
    for (int k = 0; k < 299; k++) {
        pa.push_back(k);
        pb.push_back(k + 1);
        seeds.push_back(k % 7 == 0 ? 0 : ((uint64_t)k << 30) + (uint64_t)k);
    }
    AlignPlan p;
    std::string err;
    CHECK(plan(sq, pa, pb, t, wide_limits(), p, err) == GA_OK, "plan failed: %s", err.c_str());
    std::vector<uint32_t> one((size_t)p.tab_entries, 0xdeadbeefu), many((size_t)p.tab_entries, 0xdeadbeefu);
    std::vector<gabrng::Item> jobs;
    for (size_t k = 0; k < p.kernel.size(); k++)
        jobs.push_back(gabrng::Item{seeds[(size_t)p.kernel[k].out], p.walk[k].tab_off, p.kernel[k].m + p.kernel[k].n, 0});
    build_tables(jobs.data(), (int64_t)jobs.size(), 1, one.data());
    for (int nt : {2, 3, 8, 64}) {
        std::fill(many.begin(), many.end(), 0xdeadbeefu);
        build_tables(jobs.data(), (int64_t)jobs.size(), nt, many.data());
        CHECK(one == many, "%d threads give the sequential tables", nt);
    }
    // every job's table is the one garng::RngTable makes from its seed, and no entry outside the jobs is written
    std::vector<uint32_t> direct((size_t)p.tab_entries, 0xdeadbeefu);
    for (const gabrng::Item& jb : jobs) {
        garng::RngTable R;
        garng::seed_state(jb.seed, st);
        R.start(st);
        R.extend(jb.steps);
        std::copy(R.tab.begin(), R.tab.begin() + jb.steps, direct.begin() + jb.tab_off);
    }
    CHECK(one == direct, "a table per job, made directly");
    // a pair's table is build_rng's from its seeded state, whatever else the batch holds
    for (size_t k = 0; k < p.kernel.size(); k += 50) {
        garng::RngTable R;
        garng::seed_state(seeds[(size_t)p.kernel[k].out], st);
        const int64_t steps = p.kernel[k].m + p.kernel[k].n;
        garng::build_rng(st, steps, R);
        bool same = true;
        for (int64_t d = 0; d < steps; d++) same &= R.tab[(size_t)d] == one[(size_t)(p.walk[k].tab_off + d)];
        CHECK(same, "table of work item %zu", k);
    }
    CHECK(rng_threads(0, 1) == 1 && rng_threads(0, 64) == 1 && rng_threads(0, 1 << 20) <= kMaxRngThreads, "automatic");
    CHECK(rng_threads(1, 1 << 20) == 1 && rng_threads(5, 10) == 5 && rng_threads(99, 10) == kMaxRngThreads, "requested");
}

// split_tables on `jobs` (entries: the table's size): the two lists partition the jobs in order, by the route rule;
// the ranges cover the host jobs' entries once and nothing else; no range is empty or begins where another ends
// (the route per job is restated here as the rule's own expression, so the counts want_dev and want_ranges, worked out
// by hand at every call, are the independent reference for the rule)
void check_split(const std::vector<gabrng::Item>& jobs, int64_t entries, bool want_device, int64_t limit, size_t want_dev,
                 size_t want_ranges) {
    const TableSplit sp = split_tables(jobs.data(), (int64_t)jobs.size(), want_device, limit);
    auto same = [](const gabrng::Item& x, const gabrng::Item& y) {
        return x.seed == y.seed && x.tab_off == y.tab_off && x.steps == y.steps && x.pad == y.pad;
    };
    CHECK(sp.dev.size() == want_dev && sp.dev.size() + sp.host.size() == jobs.size() && sp.dev_at.size() == sp.dev.size(),
          "limit %lld: %zu device and %zu host jobs of %zu", (long long)limit, sp.dev.size(), sp.host.size(), jobs.size());
    std::vector<int> want((size_t)entries, 0), cover((size_t)entries, 0);
    size_t q = 0, h = 0;
    for (size_t t = 0; t < jobs.size(); t++) {
        const bool dev = want_device && jobs[t].steps <= limit;
        if (dev) {
            CHECK(q < sp.dev.size() && sp.dev_at[q] == (int64_t)t && same(sp.dev[q], jobs[t]), "job %zu is device job %zu", t, q);
            q++;
        } else {
            CHECK(h < sp.host.size() && same(sp.host[h], jobs[t]), "job %zu is host job %zu", t, h);
            h++;
            for (int64_t d = 0; d < jobs[t].steps; d++) want[(size_t)(jobs[t].tab_off + d)]++;
        }
    }
    for (const TableRange& rg : sp.ranges) {
        CHECK(0 <= rg.first && rg.first < rg.last && rg.last <= entries, "range [%lld, %lld)", (long long)rg.first,
              (long long)rg.last);
        for (int64_t d = std::max<int64_t>(rg.first, 0); d < std::min(rg.last, entries); d++) cover[(size_t)d]++;
        for (const TableRange& other : sp.ranges) CHECK(rg.last != other.first, "ranges touch at %lld", (long long)rg.last);
    }
    CHECK(want == cover, "limit %lld: the ranges cover the host jobs' entries, once", (long long)limit);
    CHECK(sp.ranges.size() == want_ranges, "limit %lld: %zu ranges, want %zu", (long long)limit, sp.ranges.size(), want_ranges);
}

void test_split() {
    // steps at entry offsets: two host neighbours, a device job, a host job behind it, jobs at the limit 10 and one
    // under it, a jump to 100 with a neighbour, a last device job
    const int32_t steps[] = {12, 15, 8, 11, 10, 9, 20, 11, 3};
    const int64_t offs[] = {0, 12, 27, 35, 46, 56, 100, 120, 131};
    std::vector<gabrng::Item> jobs;
    for (int k = 0; k < 9; k++) jobs.push_back(gabrng::Item{0x1234567800ull + (uint64_t)k, offs[k], steps[k], 0});
    const int64_t entries = 134;
    check_split(jobs, entries, true, 9, 3, 3);    // host: [0, 27) [35, 56) [100, 131)
    check_split(jobs, entries, true, 10, 4, 3);   // host: [0, 27) [35, 46) [100, 131)
    check_split(jobs, entries, true, 11, 6, 2);   // host: [0, 27) [100, 120)
    check_split(jobs, entries, true, 1 << 20, 9, 0);
    check_split(jobs, entries, false, 1 << 20, 0, 2);  // all host: [0, 65) [100, 134)
    check_split(jobs, entries, true, 0, 0, 2);
    check_split(std::vector<gabrng::Item>(), 0, true, 10, 0, 0);
    check_split(std::vector<gabrng::Item>(), 0, false, 10, 0, 0);
}

}  // namespace

int main() {
    test_split();
    test_routing_and_order();
    test_limits();
    test_word_widths();
    test_decode();
    test_columns();
    test_seed_and_tables();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
