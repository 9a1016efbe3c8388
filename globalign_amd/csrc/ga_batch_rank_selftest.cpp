// ga_batch_rank_selftest.cpp -- CPU self-test of the host's share of ga_batch_rank: the CPU model of the saturating
// count table and of the unranking walk, and the table's address function (ga_batch_rank.h), and the rank planner
// (ga_batch.h plan_batch_rank: plan_batch_count's fill side plus the tables' chunk cap and the walk items), plain and
// under AddressSanitizer + UndefinedBehaviorSanitizer (make -C globalign_amd/csrc batch_rank_selftest batch_rank_asan;
// run by tests/test_batch_rank_host.py).  No HIP: the kernels are tested on the GPU.
#include <cstdio>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "ga_batch.h"
#include "ga_batch_count.h"
#include "ga_batch_layout.h"
#include "ga_batch_rank.h"

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

// N(i, j, L) of every interior cell in 128-bit integers, as rank_table lays its own out
std::vector<u128> exact_table(const std::vector<uint16_t>& sets, int64_t m, int64_t n) {
    std::vector<u128> N((size_t)(m * n * 3), 0);
    auto at = [&](int64_t i, int64_t j, int L) -> u128 {
        return (i == 0 || j == 0) ? 1 : N[(size_t)(((i - 1) * n + (j - 1)) * 3 + L)];
    };
    for (int64_t i = 1; i <= m; i++)
        for (int64_t j = 1; j <= n; j++)
            for (int L = 0; L < 3; L++) {
                const unsigned set = sets[(size_t)((i - 1) * n + (j - 1))] >> (3 * L);
                N[(size_t)(((i - 1) * n + (j - 1)) * 3 + L)] = ((set & 1u) ? at(i - 1, j - 1, 0) : 0) +
                                                                 ((set & 2u) ? at(i, j - 1, 1) : 0) +
                                                                 ((set & 4u) ? at(i - 1, j, 2) : 0);
            }
    return N;
}

// ------------------------------------------------------------------ the table
void test_table() {
    std::mt19937 rng(41);
    for (int round = 0; round < 400; round++) {
        const int64_t m = 1 + rng() % 12, n = 1 + rng() % 12;
        const std::vector<uint16_t> sets = random_sets(rng, m, n, 1 + (int)(rng() % 3));
        const std::vector<u128> want = exact_table(sets, m, n);
        // nothing saturates at the real cap on grids this small; a small artificial cap is reached on them
        for (const uint64_t cap : {kRankCap, (uint64_t)5, (uint64_t)(1 + rng() % 200)}) {
            std::vector<uint64_t> N;
            const uint64_t total = rank_table(sets.data(), m, n, cap, N);
            bool same = N.size() == want.size();
            for (size_t q = 0; same && q < N.size(); q++) same = (u128)N[q] == std::min<u128>(want[q], cap);
            CHECK(same, "round %d cap %llu: the u64 table is min(exact, cap)", round, (unsigned long long)cap);
            CHECK((u128)total == std::min<u128>(want[(size_t)(((m - 1) * n + (n - 1)) * 3)], cap), "round %d: the total", round);
            if (cap == kRankCap)
                CHECK((u128)total == count_paths<u128>(sets.data(), m, n), "round %d: the total is count_paths's", round);
        }
    }
    // every decision tied, 60 x 60: far past 2^64, and the table says so
    {
        const std::vector<uint16_t> all(3600, 0x1ff);
        std::vector<uint64_t> N;
        CHECK(rank_table(all.data(), 60, 60, kRankCap, N) == kRankCap, "all tied, side 60: saturated");
        CHECK(count_paths<u128>(all.data(), 30, 30) > ((u128)1 << 64), "all tied, side 30 is past 2^64 already");
        const std::vector<u128> want = exact_table(std::vector<uint16_t>(400, 0x1ff), 20, 20);
        std::vector<uint64_t> N20;
        rank_table(all.data() /* any 400 tied cells */, 20, 20, kRankCap, N20);
        bool same = true;
        for (size_t q = 0; q < N20.size(); q++) same = same && (u128)N20[q] == std::min<u128>(want[q], kRankCap);
        CHECK(same, "all tied, side 20: min(exact, 2^64 - 1)");
    }
    CHECK(sat_add(kRankCap, 1, kRankCap) == kRankCap && sat_add(kRankCap - 1, 1, kRankCap) == kRankCap &&
              sat_add(1ull << 63, 1ull << 63, kRankCap) == kRankCap && sat_add(3, 4, kRankCap) == 7 && sat_add(3, 4, 5) == 5,
          "sat_add");
}

// ------------------------------------------------------------------ the walk
// every path of the DAG from (i, j, L) in depth-first order, moves tried in the order 0, 1, 2: its level sequence
void dfs_paths(const std::vector<uint16_t>& sets, int64_t n, int64_t i, int64_t j, int L, std::vector<int>& cur,
               std::vector<std::vector<int>>& out) {
    if (i == 0 || j == 0) {
        out.push_back(cur);
        return;
    }
    const unsigned s = (sets[(size_t)((i - 1) * n + (j - 1))] >> (3 * L)) & 7u;
    for (int k = 0; k < 3; k++)
        if (s & (1u << k)) {
            cur.push_back(k);
            dfs_paths(sets, n, i - (k != 1), j - (k != 2), k, cur, out);
            cur.pop_back();
        }
}

std::vector<int> levels_of(const std::vector<uint32_t>& ops, int D) {
    std::vector<int> lv;
    for (int d = 0; d < D; d++) lv.push_back((int)((ops[(size_t)(d >> 4)] >> (30 - 2 * (d & 15))) & 3u));
    return lv;
}

void test_walk() {
    std::mt19937 rng(99);
    int64_t most = 0;
    for (int round = 0; round < 400; round++) {
        const int32_t m = 2 + (int32_t)(rng() % 7), n = 2 + (int32_t)(rng() % 7);
        const std::vector<uint16_t> sets = random_sets(rng, m, n, 1 + (int)(rng() % 3));
        std::vector<std::vector<int>> paths;
        std::vector<int> cur;
        dfs_paths(sets, n, m, n, 0, cur, paths);
        // the real cap, and a small one: ranks below min(count, cap) unrank exactly under saturated counts too
        for (const uint64_t cap : {kRankCap, (uint64_t)(2 + rng() % 6)}) {
            std::vector<uint64_t> N;
            const uint64_t total = rank_table(sets.data(), m, n, cap, N);
            CHECK(total == std::min<uint64_t>(paths.size(), cap), "round %d: %zu paths, the table has %llu", round,
                  paths.size(), (unsigned long long)total);
            auto set_at = [&](int32_t i, int32_t j) { return sets[(size_t)((i - 1) * n + (j - 1))]; };
            auto cnt_at = [&](int32_t i, int32_t j, int L) { return N[(size_t)(((i - 1) * n + (j - 1)) * 3 + L)]; };
            std::set<std::vector<int>> seen;
            std::vector<uint32_t> ops((size_t)((m + n + 15) / 16) + 1, 0xdeadbeefu);
            for (uint64_t r = 0; r < total; r++) {
                const RankWalk w = rank_walk(set_at, cnt_at, m, n, r, ops.data());
                const std::vector<int> lv = levels_of(ops, w.D);
                CHECK(w.status == kRankOk && lv == paths[(size_t)r], "round %d rank %llu: the DFS's path", round,
                      (unsigned long long)r);
                CHECK((w.i_end == 0 || w.j_end == 0) && w.D >= 1 && w.D <= m + n - 1 &&
                          w.reason == (w.i_end == 0 ? (w.j_end == 0 ? 0 : 1) : 2), "round %d rank %llu: the end", round,
                      (unsigned long long)r);
                seen.insert(lv);
            }
            CHECK(seen.size() == (size_t)total, "round %d: the ranks' paths all differ", round);
            CHECK(ops.back() == 0xdeadbeefu, "round %d: the level words stay within ceil((m + n) / 16)", round);
            // a rank at or above the count is reported and draws no walk
            for (const uint64_t r : {total, total + 1, kRankCap - 1}) {
                if (r < total) continue;
                const RankWalk w = rank_walk(set_at, cnt_at, m, n, r, ops.data());
                CHECK(w.status == kRankOutOfRange && w.D == 0, "round %d: rank %llu is out of range", round,
                      (unsigned long long)r);
            }
        }
        most = std::max<int64_t>(most, (int64_t)paths.size());
    }
    CHECK(most >= 20, "the random grids have ties (most paths: %lld)", (long long)most);
    // garbage sets and counts: at most m + n - 1 dispatches, never outside rows / columns >= 1 before the end, and the
    // loads it asks for are all of interior cells
    for (int round = 0; round < 2000; round++) {
        const int32_t m = 2 + (int32_t)(rng() % 9), n = 2 + (int32_t)(rng() % 9);
        bool inside = true;
        auto set_at = [&](int32_t i, int32_t j) {
            inside = inside && i >= 1 && i <= m && j >= 1 && j <= n;
            return (uint16_t)(rng() & (round % 2 ? 0xffffu : 0x1ffu));  // (also empty sets and bits above the nine)
        };
        auto cnt_at = [&](int32_t i, int32_t j, int L) -> uint64_t {
            inside = inside && i >= 1 && i <= m && j >= 1 && j <= n && L >= 0 && L <= 2;
            const uint64_t v = ((uint64_t)rng() << 32) | rng();
            return rng() % 3 == 0 ? 0 : rng() % 3 == 0 ? kRankCap : v >> (rng() % 64);
        };
        std::vector<uint32_t> ops((size_t)((m + n + 15) / 16) + 1, 0xdeadbeefu);
        const RankWalk w = rank_walk(set_at, cnt_at, m, n, ((uint64_t)rng() << 32 | rng()) >> (rng() % 64), ops.data());
        CHECK(inside, "garbage round %d: a load outside the matrix", round);
        CHECK(ops.back() == 0xdeadbeefu, "garbage round %d: level words past the slice", round);
        if (w.status == kRankOk) {
            CHECK(w.D >= 1 && w.D <= m + n - 1 && (w.i_end == 0 || w.j_end == 0) && w.i_end >= 0 && w.j_end >= 0,
                  "garbage round %d: %d dispatches to (%d, %d)", round, w.D, w.i_end, w.j_end);
            // the levels lead from (m, n) to the end it reports, inside the matrix all the way
            int32_t i = m, j = n;
            bool ok = true;
            for (const int lv : levels_of(ops, w.D)) {
                ok = ok && i >= 1 && j >= 1 && lv <= 2;
                i -= lv != 1;
                j -= lv != 2;
            }
            CHECK(ok && i == w.i_end && j == w.j_end, "garbage round %d: the levels lead to the end", round);
        } else {
            CHECK(w.status == kRankOutOfRange && w.D == 0, "garbage round %d: status %d", round, w.status);
        }
    }
}

// ------------------------------------------------------------------ the table's address function
void test_address() {
    for (int T = 1; T <= kMaxT; T++)
        for (int ns = 1; ns <= 3; ns++)
            for (const int m : {1, 2, 3, 63, 64, 65, 130}) {
                // the widest pair of the geometry, and one whose last stripe is partial (its last lane too)
                for (const int n : {64 * T * ns, 64 * T * (ns - 1) + std::max(1, 64 * T - T - 1)}) {
                    const int64_t entries = rank_table_entries(m, T, ns);
                    std::vector<uint8_t> hit((size_t)entries, 0);
                    bool in = true, once = true;
                    for (int i = 1; i <= m; i++)
                        for (int j = 1; j <= n; j++)
                            for (int plane = 0; plane < 3; plane++) {
                                const unsigned long long x = rank_table_index(m, T, i, j, plane);
                                if (x >= (unsigned long long)entries) {
                                    in = false;
                                    continue;
                                }
                                once = once && !hit[(size_t)x];
                                hit[(size_t)x] = 1;
                            }
                    CHECK(in, "T %d, %d stripes, m %d, n %d: an entry outside the pair's table", T, ns, m, n);
                    CHECK(once, "T %d, %d stripes, m %d, n %d: two cells share an entry", T, ns, m, n);
                    // a step's store of one plane of one column is 64 consecutive entries, lane by lane
                    const int j = std::min(n, 64 * T * (ns - 1) + 1);
                    if (m >= 64 && j + 63 * T <= n) {
                        bool run = true;
                        for (int l = 1; l < 64; l++)
                            run = run && rank_table_index(m, T, 64 - l, j + l * T, 1) == rank_table_index(m, T, 64, j, 1) + (unsigned)l;
                        CHECK(run, "T %d, %d stripes, m %d: a step's lanes store side by side", T, ns, m);
                    }
                }
            }
    CHECK(rank_table_step(5, 2, 0, 0) == 0 && rank_table_step(5, 2, 1, 0) == 68ull * 6 * 64 &&
              rank_table_index(5, 2, 1, 1, 0) == 0 && rank_table_index(5, 2, 1, 2, 2) == 5 * 64 &&
              rank_table_index(5, 2, 2, 3, 1) == (2ull * 6 + 1) * 64 + 1,
          "the formula by hand");
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
    std::vector<int64_t> rank_off{0};
    int64_t npairs() const { return (int64_t)pa.size(); }
    int64_t nseq() const { return (int64_t)off.size() - 1; }
    void add(int64_t m, int64_t n, int64_t nranks, std::mt19937& rng) {
        for (const int64_t len : {m, n}) {
            for (int64_t q = 0; q < len; q++) codes.push_back((uint8_t)(rng() % 4));
            off.push_back((int64_t)codes.size());
        }
        pa.push_back((int32_t)nseq() - 2);
        pb.push_back((int32_t)nseq() - 1);
        rank_off.push_back(rank_off.back() + nranks);
    }
};

int plan(const Batch& b, const Tables& t, const RankLimits& lim, RankPlan& p, std::string& err) {
    return plan_batch_rank(b.codes.data(), b.off.data(), b.nseq(), b.pa.data(), b.pb.data(), nullptr, b.npairs(), &t.cs,
                           b.rank_off.data(), lim, p, err);
}

RankLimits wide_limits() {
    RankLimits lim;
    lim.max_cells = 1 << 30;
    lim.scratch_rows_cap = 1 << 20;
    lim.count_rows_cap = 1 << 20;
    return lim;
}

void check_plan(const Batch& b, const Tables& t, const RankLimits& lim, const RankPlan& p, const char* what) {
    // the fill side: plan_batch_count's routing and work list for the same inputs
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
    CHECK(p.words.size() == p.kernel.size() && p.table_off.size() == p.kernel.size() && p.chunk_table.size() == p.chunks.size(),
          "%s: one slice and one table per kernel pair", what);
    std::vector<int> in_chunk(p.kernel.size(), 0);
    std::vector<int> walked((size_t)b.rank_off.back(), 0);
    int64_t next_pair = 0, next_launch = 0, next_item = 0;
    for (size_t c = 0; c < p.chunks.size(); c++) {
        const FillChunk& ch = p.chunks[c];
        CHECK(ch.first == next_pair && ch.count > 0, "%s: chunks follow each other", what);
        CHECK(ch.tb_words <= lim.chunk_tb_words && p.chunk_table[c] * 8 <= lim.chunk_table_bytes,
              "%s: chunk %zu respects both caps", what, c);
        int64_t woff = 0, toff = 0;
        for (int64_t q = ch.first; q < ch.first + ch.count && q < (int64_t)p.kernel.size(); q++) {
            const ga_batch_item& it = p.kernel[(size_t)q];
            in_chunk[(size_t)q]++;
            CHECK(p.words[(size_t)q].tb_off == woff && p.words[(size_t)q].tb_words == tb_slice_words(it.m, it.T, it.nstripes, p.CB),
                  "%s: slice of work item %lld", what, (long long)q);
            CHECK(p.table_off[(size_t)q] == toff, "%s: table of work item %lld", what, (long long)q);
            CHECK(rank_table_entries(it.m, it.T, it.nstripes) * 8 == rank_table_bytes(it.m, it.n), "%s: table bytes", what);
            CHECK(rank_table_index(it.m, it.T, it.m, it.n, 2) < (unsigned long long)rank_table_entries(it.m, it.T, it.nstripes),
                  "%s: cell (m, n) of work item %lld inside its table", what, (long long)q);
            woff += p.words[(size_t)q].tb_words;
            toff += rank_table_entries(it.m, it.T, it.nstripes);
        }
        CHECK(woff == ch.tb_words && toff == p.chunk_table[c], "%s: a chunk's words and tables are its pairs'", what);
        // a chunk closed because the next pair would not fit one of the caps
        if (c + 1 < p.chunks.size()) {
            const ga_batch_item& nx = p.kernel[(size_t)(ch.first + ch.count)];
            CHECK(ch.tb_words + tb_slice_words(nx.m, nx.T, nx.nstripes, p.CB) > lim.chunk_tb_words ||
                      (p.chunk_table[c] + rank_table_entries(nx.m, nx.T, nx.nstripes)) * 8 > lim.chunk_table_bytes,
                  "%s: chunk %zu closed for a reason", what, c);
        }
        // the chunk's walk launches and items: its pairs in work-list order, every slot once and in order
        CHECK(ch.launch_first == next_launch, "%s: launches follow each other", what);
        int64_t pair = ch.first, slot = pair < (int64_t)p.kernel.size() ? b.rank_off[(size_t)p.kernel[(size_t)pair].out] : 0;
        for (int64_t L = ch.launch_first; L < ch.launch_first + ch.launch_count; L++) {
            const RankLaunch& wl = p.launches[(size_t)L];
            CHECK(wl.first == next_item && wl.count > 0, "%s: launch %lld's items follow", what, (long long)L);
            int64_t slots = 0, steps = 0, words = 0;
            for (int64_t x = wl.first; x < wl.first + wl.count; x++) {
                const ga_batch_rank_item& wi = p.walk[(size_t)x];
                CHECK(wi.fill >= 0 && wi.fill < ch.count && wi.nslots >= 1 && wi.nslots <= 64, "%s: walk item %lld", what, (long long)x);
                const ga_batch_item& it = p.kernel[(size_t)(ch.first + wi.fill)];
                // on to the pair of this item, past pairs without ranks
                while (pair < ch.first + ch.count &&
                       (pair < ch.first + wi.fill || slot == b.rank_off[(size_t)p.kernel[(size_t)pair].out + 1])) {
                    CHECK(slot == b.rank_off[(size_t)p.kernel[(size_t)pair].out + 1], "%s: a pair's slots are all walked", what);
                    pair++;
                    if (pair < ch.first + ch.count) slot = b.rank_off[(size_t)p.kernel[(size_t)pair].out];
                }
                CHECK(pair == ch.first + wi.fill && wi.out == slot, "%s: walk item %lld takes the next slots", what, (long long)x);
                CHECK(wi.out + wi.nslots <= b.rank_off[(size_t)it.out + 1] &&
                          (wi.nslots == 64 || wi.out + wi.nslots == b.rank_off[(size_t)it.out + 1]),
                      "%s: walk item %lld is 64 slots or the pair's last", what, (long long)x);
                CHECK(wi.res == slots && wi.ops_off == words, "%s: walk item %lld's results and level words", what, (long long)x);
                for (int l = 0; l < wi.nslots; l++) walked[(size_t)(wi.out + l)]++;
                slot = wi.out + wi.nslots;
                slots += wi.nslots;
                steps += (int64_t)wi.nslots * (it.m + it.n);
                words += (int64_t)wi.nslots * ((it.m + it.n + 15) / 16);
            }
            CHECK(slots == wl.slots && steps == wl.steps && words == wl.ops_words, "%s: launch %lld's sums", what, (long long)L);
            CHECK(wl.steps <= std::max<int64_t>(lim.walk_entries, 1) || wl.count == 1, "%s: launch %lld within the cap", what, (long long)L);
            next_item = wl.first + wl.count;
        }
        next_launch = ch.launch_first + ch.launch_count;
        next_pair = ch.first + ch.count;
    }
    CHECK(next_pair == (int64_t)p.kernel.size() && next_launch == (int64_t)p.launches.size() && next_item == (int64_t)p.walk.size(),
          "%s: every work item, launch and walk item sits in a chunk", what);
    for (size_t q = 0; q < in_chunk.size(); q++) CHECK(in_chunk[q] == 1, "%s: work item %zu in exactly one chunk", what, q);
    for (const ga_batch_item& it : p.kernel)
        for (int64_t f = b.rank_off[(size_t)it.out]; f < b.rank_off[(size_t)it.out + 1]; f++)
            CHECK(walked[(size_t)f] == 1, "%s: slot %lld is walked once", what, (long long)f);
    for (const int64_t k : p.single)
        for (int64_t f = b.rank_off[(size_t)k]; f < b.rank_off[(size_t)k + 1]; f++)
            CHECK(walked[(size_t)f] == 0, "%s: a single pair's slot %lld is not the kernel route's", what, (long long)f);
}

void test_planner() {
    std::mt19937 rng(23);
    for (int round = 0; round < 200; round++) {
        const int open = round % 3 == 0 ? 4 : round % 3 == 1 ? 30 : 200;  // one-, two- and four-byte words
        Tables t(5, 5, 3, open);
        Batch b;
        const int npairs = 1 + (int)(rng() % 30);
        for (int k = 0; k < npairs; k++) {
            auto len = [&](int max_len) { return rng() % 9 == 0 ? 1 : 2 + (int64_t)(rng() % (unsigned)(max_len - 1)); };
            const int64_t nranks = rng() % 4 == 0 ? 0 : rng() % 4 == 0 ? 60 + rng() % 150 : 1 + rng() % 20;
            if (rng() % 8 == 0) b.add(len(2000), len(1200), nranks, rng);
            else b.add(len(200), len(600), nranks, rng);
        }
        RankLimits lim = wide_limits();
        if (round % 2) {
            lim.max_cells = 1 + (int64_t)(rng() % 2000000);
            lim.chunk_tb_words = 64 + (int64_t)(rng() % 400000);
            lim.walk_entries = 1 + (int64_t)(rng() % 20000);
        }
        if (round % 4 >= 2) {
            // a table cap no pair exceeds, small enough to cut chunks
            int64_t most = 0;
            for (int k = 0; k < npairs; k++) {
                const int64_t m = b.off[(size_t)b.pa[(size_t)k] + 1] - b.off[(size_t)b.pa[(size_t)k]];
                const int64_t n = b.off[(size_t)b.pb[(size_t)k] + 1] - b.off[(size_t)b.pb[(size_t)k]];
                if (std::min(m, n) >= 2) most = std::max(most, rank_table_bytes(m, n));
            }
            lim.chunk_table_bytes = most + (int64_t)(rng() % (unsigned)(most + 1));
        }
        RankPlan p;
        std::string err;
        CHECK(plan(b, t, lim, p, err) == GA_OK, "round %d: plan failed: %s", round, err.c_str());
        check_plan(b, t, lim, p, ("round " + std::to_string(round)).c_str());
    }
    // the two caps by hand: five pairs of one size
    {
        Tables t(5, 5, 3, 4);
        Batch b;
        for (int k = 0; k < 5; k++) b.add(50, 70, 130, rng);
        RankLimits lim = wide_limits();
        RankPlan p;
        std::string err;
        CHECK(plan(b, t, lim, p, err) == GA_OK && p.chunks.size() == 1 && p.launches.size() == 1 && p.walk.size() == 15 &&
                  p.launches[0].slots == 650, "the defaults: one chunk, one walk launch, three items a pair");
        check_plan(b, t, lim, p, "defaults");
        CHECK(rank_table_bytes(50, 70) == (50 + 63) * 3 * 2 * 64 * 8, "a 50 x 70 pair's table: one stripe at T = 2");
        lim.chunk_table_bytes = 2 * rank_table_bytes(50, 70);
        CHECK(plan(b, t, lim, p, err) == GA_OK && p.chunks.size() == 3, "two tables a chunk: three chunks, got %zu", p.chunks.size());
        check_plan(b, t, lim, p, "table cap");
        lim.chunk_table_bytes = rank_table_bytes(50, 70) - 1;
        CHECK(plan(b, t, lim, p, err) == GA_E_ARG && err == "pair 0: count table exceeds the rank table budget", "got: %s", err.c_str());
        lim = wide_limits();
        lim.chunk_tb_words = 2 * tb_slice_words(50, 2, 1, 1);
        CHECK(plan(b, t, lim, p, err) == GA_OK && p.chunks.size() == 3, "two slices a chunk: three chunks");
        check_plan(b, t, lim, p, "words cap");
        lim = wide_limits();
        lim.walk_entries = 64 * 120;
        CHECK(plan(b, t, lim, p, err) == GA_OK && p.launches.size() == 15, "one item a launch: %zu launches", p.launches.size());
        check_plan(b, t, lim, p, "walk cap");
        // a pair with a one-letter sequence ahead of one over the table cap: only the second is the planner's to refuse
        Batch c;
        c.add(1, 9, 3, rng);
        c.add(50, 70, 3, rng);
        c.add(60, 70, 3, rng);
        lim = wide_limits();
        lim.chunk_table_bytes = rank_table_bytes(50, 70);
        CHECK(plan(c, t, lim, p, err) == GA_E_ARG && err == "pair 2: count table exceeds the rank table budget", "got: %s", err.c_str());
    }
    // the checks and their order are plan_batch_count's, then the ranks'
    {
        Tables t(5, 5, 3, 4);
        Batch b;
        b.codes.assign(20, 0);
        b.off = {0, 10, 20};
        b.pa = {0};
        b.pb = {1};
        b.rank_off = {0, 2};
        RankPlan p;
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
        // (both faults: the index comes first, as in plan_batch_count)
        b.codes[3] = 9;
        both(t, "index, then code");
        b.codes[3] = 0;
        b.pb = {1};
        both(Tables(5, 5, 3, 40000), "gap open cost too large");
        CHECK(plan_batch_rank(b.codes.data(), b.off.data(), 2, b.pa.data(), b.pb.data(), nullptr, 1, nullptr, b.rank_off.data(),
                              wide_limits(), p, err) == GA_E_ARG, "null costs");
        CHECK(plan_batch_rank(b.codes.data(), b.off.data(), 2, b.pa.data(), b.pb.data(), nullptr, 1, &t.cs, nullptr,
                              wide_limits(), p, err) == GA_E_ARG && err == "null argument", "null rank_off");
        b.rank_off = {1, 2};
        CHECK(plan(b, t, wide_limits(), p, err) == GA_E_ARG && err == "rank_off must start at 0", "got: %s", err.c_str());
        b.rank_off = {0, -1};
        CHECK(plan(b, t, wide_limits(), p, err) == GA_E_ARG && err == "rank_off must not decrease", "got: %s", err.c_str());
        b.rank_off = {0, (int64_t)1 << 31};
        CHECK(plan(b, t, wide_limits(), p, err) == GA_E_RANGE, "too many ranks: %s", err.c_str());
        b.rank_off = {0, 0};
        CHECK(plan(b, t, wide_limits(), p, err) == GA_OK && p.chunks.size() == 1 && p.walk.empty() && p.launches.empty() &&
                  p.chunks[0].launch_count == 0, "no ranks: filled and counted, nothing walked");
        CHECK(plan_batch_rank(nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, &t.cs, nullptr, wide_limits(), p, err) == GA_OK &&
                  p.chunks.empty() && p.kernel.empty(), "an empty batch plans to nothing");
    }
    CHECK(kRankTableBytesCap == (8ll << 30), "the tables' default cap is the words'");
}

}  // namespace

int main() {
    test_table();
    test_walk();
    test_address();
    test_planner();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
