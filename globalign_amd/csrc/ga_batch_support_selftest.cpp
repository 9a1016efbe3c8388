// ga_batch_support_selftest.cpp -- CPU self-test of the host's share of ga_batch_support: the pure model of match
// support (ga_batch_support.h: the recurrence, a lane's step, and the wave's loop run lane by lane as batch_flow_kernel
// runs it) and the support planner (ga_batch.h plan_batch_support: plan_batch_count's fill side plus the tables' and
// the output's chunk caps), plain and under AddressSanitizer + UndefinedBehaviorSanitizer (make -C globalign_amd/csrc
// batch_support_selftest batch_support_asan; run by tests/test_batch_support_host.py).  No HIP: the kernels are tested
// on the GPU.
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "ga_batch.h"
#include "ga_batch_count.h"
#include "ga_batch_layout.h"
#include "ga_batch_rank.h"
#include "ga_batch_support.h"

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

typedef unsigned __int128 u128;

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

// ------------------------------------------------------------------ the recurrence against 128-bit integers
void test_model() {
    std::mt19937 rng(515);
    for (int round = 0; round < 400; round++) {
        const int64_t m = 1 + rng() % 14, n = 1 + rng() % 14;
        const std::vector<uint16_t> sets = random_sets(rng, m, n, 1 + (int)(rng() % 3));
        std::vector<u128> want;
        std::vector<double> got;
        const u128 count = support_matrix<u128>(sets.data(), m, n, want);
        const double countf = support_matrix<double>(sets.data(), m, n, got);
        CHECK(count == count_paths<u128>(sets.data(), m, n) && (u128)countf == count, "round %d: the count is count_paths's", round);
        bool same = got.size() == want.size(), below = true;
        for (size_t q = 0; same && q < got.size(); q++) {
            same = (u128)got[q] == want[q] && got[q] == (double)want[q];
            below = below && want[q] <= count;
        }
        CHECK(same, "round %d (%lld x %lld): the doubles are the integers", round, (long long)m, (long long)n);
        CHECK(below, "round %d: a support above the count", round);
        // a row's and a column's supports are disjoint sets of members: their sums are at most the count
        for (int64_t i = 0; i < m; i++) {
            u128 sum = 0;
            for (int64_t j = 0; j < n; j++) sum += want[(size_t)(i * n + j)];
            CHECK(sum <= count, "round %d: row %lld sums past the count", round, (long long)i);
        }
        for (int64_t j = 0; j < n; j++) {
            u128 sum = 0;
            for (int64_t i = 0; i < m; i++) sum += want[(size_t)(i * n + j)];
            CHECK(sum <= count, "round %d: column %lld sums past the count", round, (long long)j);
        }
    }
    // every decision tied, 40 x 40: past 2^53, the doubles stay within the chain's rounding bound of the integers
    {
        const std::vector<uint16_t> all(1600, 0x1ff);
        std::vector<u128> want;
        std::vector<double> got;
        const u128 count = support_matrix<u128>(all.data(), 40, 40, want);
        support_matrix<double>(all.data(), 40, 40, got);
        CHECK(count > ((u128)1 << 53), "all tied, side 40 is past 2^53");
        bool close = true;
        for (size_t q = 0; q < got.size(); q++) {
            const double w = (double)want[q];
            close = close && got[q] >= w * (1 - 400 * 0x1p-53) && got[q] <= w * (1 + 400 * 0x1p-53);
        }
        CHECK(close, "all tied, side 40: within 400 ulp of the integers");
    }
    // by hand: two letters a side, every decision tied: 13 members (ga_batch_count's), the four supports
    {
        const std::vector<uint16_t> all(4, 0x1ff);
        std::vector<u128> s;
        CHECK(support_matrix<u128>(all.data(), 2, 2, s) == 13, "2 x 2 all tied: 13 members");
        // (2, 2) by the diagonal then any of N(1, 1, 0) = 3; (1, 1): prefixes reaching it with the diagonal open
        CHECK(s[3] == 3 && s[0] == 3 && s[1] == 1 && s[2] == 1, "2 x 2 all tied: supports %d %d %d %d", (int)s[0], (int)s[1],
              (int)s[2], (int)s[3]);
    }
}

// ------------------------------------------------------------------ the recurrence against a walk of every path
void tally_paths(const std::vector<uint16_t>& sets, int64_t n, int64_t i, int64_t j, int L, std::vector<int64_t>& cur,
                 std::vector<u128>& tally, u128& paths) {
    if (i == 0 || j == 0) {
        paths++;
        for (const int64_t cell : cur) tally[(size_t)cell]++;
        return;
    }
    const unsigned s = (sets[(size_t)((i - 1) * n + (j - 1))] >> (3 * L)) & 7u;
    for (int k = 0; k < 3; k++)
        if (s & (1u << k)) {
            if (k == 0) cur.push_back((i - 1) * n + (j - 1));
            tally_paths(sets, n, i - (k != 1), j - (k != 2), k, cur, tally, paths);
            if (k == 0) cur.pop_back();
        }
}

void test_paths() {
    std::mt19937 rng(77);
    u128 most = 0;
    for (int round = 0; round < 400; round++) {
        const int64_t m = 1 + rng() % 7, n = 1 + rng() % 7;
        const std::vector<uint16_t> sets = random_sets(rng, m, n, 1 + (int)(rng() % 3));
        std::vector<u128> tally((size_t)(m * n), 0), want;
        std::vector<int64_t> cur;
        u128 paths = 0;
        tally_paths(sets, n, m, n, 0, cur, tally, paths);
        CHECK(support_matrix<u128>(sets.data(), m, n, want) == paths, "round %d: the count is the number of paths", round);
        CHECK(tally == want, "round %d (%lld x %lld): forward x backward is the tally over every path", round, (long long)m,
              (long long)n);
        most = std::max(most, paths);
    }
    CHECK(most >= 20, "the random grids have ties");
}

// ------------------------------------------------------------------ the wave's loop
// a lane whose cells do not exist hands on zero whatever it holds and is handed
void test_zero_handover() {
    FlowLane<3> st;
    for (int k = 0; k < 3; k++) st.A0[k] = 5.0 + k, st.A2[k] = 7.0 + k;
    st.o0 = 9.0, st.o1 = 11.0, st.diag = 13.0;
    const unsigned sets[3] = {0x1ffu, 0x1ffu, 0x1ffu};
    double a0[3];
    flow_lane_step<3>(st, 17.0, 19.0, sets, 0u, -1, a0);
    CHECK(st.o0 == 0.0 && st.o1 == 0.0 && st.diag == 17.0, "a dead lane hands on zero");
    for (int k = 0; k < 3; k++) CHECK(st.A0[k] == 0.0 && st.A2[k] == 0.0 && a0[k] == 0.0, "a dead lane keeps zero");
    // only its last column past n: the live columns take nothing from it
    for (int k = 0; k < 3; k++) st.A0[k] = 0.0, st.A2[k] = 0.0;
    st.diag = 0.0;
    flow_lane_step<3>(st, 0.0, 0.0, sets, 3u, 1, a0);
    CHECK(a0[2] == 0.0 && a0[1] == 1.0 && a0[0] == 1.0, "the seed in column 1, column 2 dead: %g %g %g", a0[0], a0[1], a0[2]);
}

template <int T>
void wave_case(const std::vector<uint16_t>& sets, int m, int n, int nstripes, const char* what) {
    std::vector<double> want, N0;
    support_matrix<double>(sets.data(), m, n, want);
    count_plane0<double>(sets.data(), m, n, N0);
    // the pair's table as the N-table launch leaves it: plane 0 filled, everything else poisoned
    std::vector<double> table((size_t)rank_table_entries(m, T, nstripes), -12345.0);
    for (int i = 1; i <= m; i++)
        for (int j = 1; j <= n; j++)
            table[(size_t)rank_table_index(m, T, i, j, 0)] = N0[(size_t)i * ((size_t)n + 1) + (size_t)j];
    bool inside = true;
    support_wave<T>(
        [&](int i, int j) {
            inside = inside && i >= 1 && i <= m && j >= 1 && j <= n;
            return sets[(size_t)(i - 1) * (size_t)n + (size_t)(j - 1)];
        },
        m, n, nstripes, table);
    CHECK(inside, "%s (%d x %d): a word outside the matrix was asked for", what, m, n);
    bool same = true, kept = true;
    for (int i = 1; i <= m; i++)
        for (int j = 1; j <= n; j++) {
            same = same && table[(size_t)support_index(m, T, i, j)] == want[(size_t)(i - 1) * (size_t)n + (size_t)(j - 1)];
            kept = kept && table[(size_t)rank_table_index(m, T, i, j, 0)] == N0[(size_t)i * ((size_t)n + 1) + (size_t)j] &&
                   table[(size_t)rank_table_index(m, T, i, j, 2)] == -12345.0;
        }
    CHECK(same, "%s (%d x %d, T %d, %d stripes): the wave's supports are the recurrence's", what, m, n, T, nstripes);
    CHECK(kept, "%s (%d x %d): planes 0 and 2 are left alone", what, m, n);
}

void wave_any(const std::vector<uint16_t>& sets, int m, int n, const char* what) {
    int T = 1, ns = 1;
    stripe_geometry(n, T, ns);
    switch (T) {
        case 1: wave_case<1>(sets, m, n, ns, what); break;
        case 2: wave_case<2>(sets, m, n, ns, what); break;
        case 3: wave_case<3>(sets, m, n, ns, what); break;
        case 4: wave_case<4>(sets, m, n, ns, what); break;
        case 5: wave_case<5>(sets, m, n, ns, what); break;
        case 6: wave_case<6>(sets, m, n, ns, what); break;
        case 7: wave_case<7>(sets, m, n, ns, what); break;
        case 8: wave_case<8>(sets, m, n, ns, what); break;
        default: CHECK(false, "T %d", T);
    }
}

void test_wave() {
    std::mt19937 rng(2026);
    // every n up to three stripes at two rows: cell (m, n) in every lane and every column of a lane, of one, two and
    // three stripes, with every number of dead columns and lanes to its right
    for (int n = 1; n <= 1100; n++) wave_any(random_sets(rng, 2, n, 2), 2, n, "placement");
    // more rows than lanes, fewer, and the sizes around 64
    for (const int m : {1, 3, 63, 64, 65, 130})
        for (const int n : {1, 2, 5, 63, 64, 65, 127, 128, 129, 320, 512, 513, 1024, 1025})
            wave_any(random_sets(rng, m, n, 1 + (int)(rng() % 3)), m, n, "shape");
    // every decision tied: the largest flows
    wave_any(std::vector<uint16_t>(70 * 530, 0x1ff), 70, 530, "tied");
}

// ------------------------------------------------------------------ the planner
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

int plan(const Batch& b, const Tables& t, const SupportLimits& lim, SupportPlan& p, std::string& err) {
    return plan_batch_support(b.codes.data(), b.off.data(), b.nseq(), b.pa.data(), b.pb.data(), nullptr, b.npairs(), &t.cs, lim,
                              p, err);
}

SupportLimits wide_limits() {
    SupportLimits lim;
    lim.max_cells = 1 << 30;
    lim.scratch_rows_cap = 1 << 20;
    lim.count_rows_cap = 1 << 20;
    return lim;
}

void check_plan(const Batch& b, const Tables& t, const SupportLimits& lim, const SupportPlan& p, const char* what) {
    CountPlan cp;
    std::string err;
    CHECK(plan_batch_count(b.codes.data(), b.off.data(), b.nseq(), b.pa.data(), b.pb.data(), nullptr, b.npairs(), &t.cs, lim,
                           cp, err) == GA_OK, "%s: count plan failed: %s", what, err.c_str());
    CHECK(cp.single == p.single && cp.kernel.size() == p.kernel.size() && cp.CB == p.CB && cp.qbytes == p.qbytes &&
              cp.scratch_rows == p.scratch_rows && cp.count_rows == p.count_rows, "%s: the fill side is plan_batch_count's", what);
    for (size_t q = 0; q < p.kernel.size() && q < cp.kernel.size(); q++)
        CHECK(p.kernel[q].out == cp.kernel[q].out && p.kernel[q].m == cp.kernel[q].m && p.kernel[q].n == cp.kernel[q].n &&
                  p.kernel[q].T == cp.kernel[q].T && p.kernel[q].nstripes == cp.kernel[q].nstripes &&
                  p.kernel[q].a_off == cp.kernel[q].a_off && p.kernel[q].b_off == cp.kernel[q].b_off &&
                  p.kernel[q].big == cp.kernel[q].big, "%s: work item %zu is plan_batch_count's", what, q);
    CHECK(p.words.size() == p.kernel.size() && p.table_off.size() == p.kernel.size() && p.support_off.size() == p.kernel.size() &&
              p.chunk_table.size() == p.chunks.size() && p.chunk_support.size() == p.chunks.size(),
          "%s: one slice, one table and one output per kernel pair", what);
    int64_t next_pair = 0;
    for (size_t c = 0; c < p.chunks.size(); c++) {
        const FillChunk& ch = p.chunks[c];
        CHECK(ch.first == next_pair && ch.count > 0, "%s: chunks follow each other", what);
        CHECK(ch.tb_words <= lim.chunk_tb_words && p.chunk_table[c] * 8 <= lim.chunk_table_bytes &&
                  p.chunk_support[c] * 8 <= lim.chunk_support_bytes, "%s: chunk %zu respects the three caps", what, c);
        int64_t woff = 0, toff = 0, ooff = 0;
        for (int64_t q = ch.first; q < ch.first + ch.count && q < (int64_t)p.kernel.size(); q++) {
            const ga_batch_item& it = p.kernel[(size_t)q];
            CHECK(p.words[(size_t)q].tb_off == woff && p.words[(size_t)q].tb_words == tb_slice_words(it.m, it.T, it.nstripes, p.CB),
                  "%s: slice of work item %lld", what, (long long)q);
            CHECK(p.table_off[(size_t)q] == toff && p.support_off[(size_t)q] == ooff, "%s: table and output of work item %lld",
                  what, (long long)q);
            CHECK(support_index(it.m, it.T, it.m, it.n) < (unsigned long long)rank_table_entries(it.m, it.T, it.nstripes),
                  "%s: cell (m, n) of work item %lld inside its table", what, (long long)q);
            woff += p.words[(size_t)q].tb_words;
            toff += rank_table_entries(it.m, it.T, it.nstripes);
            ooff += (int64_t)it.m * it.n;
        }
        CHECK(woff == ch.tb_words && toff == p.chunk_table[c] && ooff == p.chunk_support[c],
              "%s: a chunk's words, tables and output are its pairs'", what);
        if (c + 1 < p.chunks.size()) {
            const ga_batch_item& nx = p.kernel[(size_t)(ch.first + ch.count)];
            CHECK(ch.tb_words + tb_slice_words(nx.m, nx.T, nx.nstripes, p.CB) > lim.chunk_tb_words ||
                      (p.chunk_table[c] + rank_table_entries(nx.m, nx.T, nx.nstripes)) * 8 > lim.chunk_table_bytes ||
                      (p.chunk_support[c] + (int64_t)nx.m * nx.n) * 8 > lim.chunk_support_bytes,
                  "%s: chunk %zu closed for a reason", what, c);
        }
        next_pair = ch.first + ch.count;
    }
    CHECK(next_pair == (int64_t)p.kernel.size(), "%s: every work item sits in a chunk", what);
}

void test_planner() {
    std::mt19937 rng(31);
    for (int round = 0; round < 200; round++) {
        const int open = round % 3 == 0 ? 4 : round % 3 == 1 ? 30 : 200;  // one-, two- and four-byte words
        Tables t(5, 5, 3, open);
        Batch b;
        const int npairs = 1 + (int)(rng() % 30);
        int64_t most_table = 0, most_out = 0;
        for (int k = 0; k < npairs; k++) {
            auto len = [&](int max_len) { return rng() % 9 == 0 ? 1 : 2 + (int64_t)(rng() % (unsigned)(max_len - 1)); };
            const int64_t m = rng() % 8 == 0 ? len(2000) : len(200), n = rng() % 8 == 0 ? len(1200) : len(600);
            b.add(m, n, rng);
            if (std::min(m, n) >= 2) most_table = std::max(most_table, rank_table_bytes(m, n)), most_out = std::max(most_out, m * n * 8);
        }
        SupportLimits lim = wide_limits();
        if (round % 2) {
            lim.max_cells = 1 + (int64_t)(rng() % 2000000);
            lim.chunk_tb_words = 64 + (int64_t)(rng() % 400000);
        }
        // caps no pair exceeds, small enough to cut chunks
        if (round % 4 >= 2) lim.chunk_table_bytes = most_table + (int64_t)(rng() % (unsigned)(most_table + 1));
        if (round % 8 >= 4) lim.chunk_support_bytes = most_out + (int64_t)(rng() % (unsigned)(most_out + 1));
        SupportPlan p;
        std::string err;
        CHECK(plan(b, t, lim, p, err) == GA_OK, "round %d: plan failed: %s", round, err.c_str());
        check_plan(b, t, lim, p, ("round " + std::to_string(round)).c_str());
    }
    // the caps by hand: five pairs of one size
    {
        Tables t(5, 5, 3, 4);
        Batch b;
        for (int k = 0; k < 5; k++) b.add(50, 70, rng);
        SupportLimits lim = wide_limits();
        SupportPlan p;
        std::string err;
        CHECK(plan(b, t, lim, p, err) == GA_OK && p.chunks.size() == 1 && p.chunk_support[0] == 5 * 3500, "the defaults: one chunk");
        check_plan(b, t, lim, p, "defaults");
        lim.chunk_support_bytes = 2 * 3500 * 8;
        CHECK(plan(b, t, lim, p, err) == GA_OK && p.chunks.size() == 3, "two outputs a chunk: three chunks, got %zu", p.chunks.size());
        check_plan(b, t, lim, p, "output cap");
        lim.chunk_support_bytes = 3500 * 8 - 1;
        CHECK(plan(b, t, lim, p, err) == GA_E_ARG && err == "pair 0: support matrix exceeds the support output budget", "got: %s",
              err.c_str());
        lim = wide_limits();
        lim.chunk_table_bytes = 2 * rank_table_bytes(50, 70);
        CHECK(plan(b, t, lim, p, err) == GA_OK && p.chunks.size() == 3, "two tables a chunk: three chunks");
        check_plan(b, t, lim, p, "table cap");
        lim.chunk_table_bytes = rank_table_bytes(50, 70) - 1;
        CHECK(plan(b, t, lim, p, err) == GA_E_ARG && err == "pair 0: count table exceeds the rank table budget", "got: %s", err.c_str());
        lim = wide_limits();
        lim.chunk_tb_words = 2 * tb_slice_words(50, 2, 1, 1);
        CHECK(plan(b, t, lim, p, err) == GA_OK && p.chunks.size() == 3, "two slices a chunk: three chunks");
        check_plan(b, t, lim, p, "words cap");
        // a pair with a one-letter sequence ahead of one over the output cap: only the second is the planner's to refuse
        Batch c;
        c.add(1, 9, rng);
        c.add(50, 70, rng);
        c.add(60, 70, rng);
        lim = wide_limits();
        lim.chunk_support_bytes = 3500 * 8;
        CHECK(plan(c, t, lim, p, err) == GA_E_ARG && err == "pair 2: support matrix exceeds the support output budget", "got: %s",
              err.c_str());
    }
    // the checks and their order are plan_batch_count's
    {
        Tables t(5, 5, 3, 4);
        Batch b;
        b.codes.assign(20, 0);
        b.off = {0, 10, 20};
        b.pa = {0};
        b.pb = {1};
        SupportPlan p;
        CountPlan cp;
        std::string err, cerr;
        auto both = [&](const Tables& tt, const char* what) {
            const int r = plan(b, tt, wide_limits(), p, err);
            const int rc = plan_batch_count(b.codes.data(), b.off.data(), b.nseq(), b.pa.data(), b.pb.data(), nullptr, b.npairs(),
                                            &tt.cs, wide_limits(), cp, cerr);
            CHECK(r == rc && err == cerr && r != GA_OK, "%s: %d '%s' against %d '%s'", what, r, err.c_str(), rc, cerr.c_str());
        };
        b.codes[3] = 9;
        both(t, "a code out of range");
        b.codes[3] = 0;
        b.pb = {2};
        both(t, "a sequence index out of range");
        b.pb = {1};
        both(Tables(5, 5, 3, 40000), "gap open cost too large");
        CHECK(plan_batch_support(nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, &t.cs, wide_limits(), p, err) == GA_OK &&
                  p.chunks.empty() && p.kernel.empty(), "an empty batch plans to nothing");
    }
    CHECK(kSupportBytesCap == (2ll << 30), "the output's default cap");
}

}  // namespace

int main() {
    test_model();
    test_paths();
    test_zero_handover();
    test_wave();
    test_planner();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
