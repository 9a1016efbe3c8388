// ga_pipe_selftest.cpp -- CPU self-test of the repeated-alignment pipeline's pure part (ga_pipe.h): the knob parse,
// the plan of a call against a table worked out from its rules, and the tie-break table's feeder thread against a
// one-shot table, plain, under AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer (make -C
// globalign_amd/csrc pipe_selftest pipe_asan pipe_tsan; run by tests/test_pipe_host.py).  No HIP: the pipeline's
// device side is tested on the GPU.
#include <atomic>
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "ga_pipe.h"

using namespace gapipe;

namespace {

std::atomic<int> failures{0};  // (checks run on several threads)

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            failures++;                                    \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);             \
            std::fprintf(stderr, "\n");                    \
        }                                                  \
    } while (0)

using KnobMap = std::map<std::string, std::string>;

// the shipped build's view (experiments = false: the dropped paths' knobs are not seen) or an experiments build's
Knobs parse(const KnobMap& kv, bool experiments = false) {
    auto get = [&kv](const char* name) -> const char* {
        const auto it = kv.find(name);
        return it == kv.end() ? nullptr : it->second.c_str();
    };
    auto none = [](const char*) -> const char* { return nullptr; };
    return experiments ? Knobs::parse(get, get) : Knobs::parse(get, none);
}

gaplan::Problem problem(int64_t m, int64_t n, int CB = 1, int qbytes = 1, int K = 4) {
    gaplan::Problem pb;
    pb.m = pb.n_global = m, pb.n = n, pb.CB = CB, pb.qbytes = qbytes, pb.K = K;
    return pb;
}

// GA_FILL_MODE as the fill planner parsed it (gaplan::Knobs::diag_req), beside the pipeline's own knobs
Knobs with_fill_mode(Knobs kn, int diag_req) {
    kn.diag_req = diag_req;
    return kn;
}

void test_knobs() {
    const Knobs d = parse({});
    CHECK(d.mode == kAuto && !d.fills && !d.slots && !d.chain && !d.fill_prio && !d.fill_prio_normal && !d.fixed_order &&
              d.pinned_io && !d.trace && d.walk_cus == 0 && !d.row_first, "defaults");
    const KnobMap all{{"GA_PIPE_MODE", "lane"}, {"GA_PIPE_FILLS", "9"}, {"GA_PIPE_SLOTS", "5"}, {"GA_PIPE_CHAIN", "1"},
                      {"GA_PIPE_FILL_PRIO", "normal"}, {"GA_PIPE_SLOT_ORDER", "fixed"}, {"GA_PIPE_PINNED_IO", "0"},
                      {"GA_PIPE_TRACE", "t.jsonl"}, {"GA_PIPE_WALK_CUS", "11"}, {"GA_PIPE_ROW_FIRST", "2"}};
    const Knobs k = parse(all);
    CHECK(k.mode == kLane && k.fills == 9 && k.slots == 5 && k.chain && k.fill_prio && k.fill_prio_normal &&
              k.fixed_order && !k.pinned_io && k.trace && std::string(k.trace) == "t.jsonl", "every shipped knob");
    CHECK(k.walk_cus == 0 && !k.row_first, "the shipped build ignores the experiments-only knobs");
    const Knobs x = parse(all, true);
    CHECK(x.walk_cus == 8 && x.row_first == 2, "an experiments build sees them (walk CUs clamped to 8)");
    CHECK(parse({{"GA_PIPE_MODE", "row"}}).mode == kRow && parse({{"GA_PIPE_MODE", "other"}}).mode == kAuto, "mode");
    CHECK(!parse({{"GA_PIPE_CHAIN", "0"}}).chain, "chain 0");
    const Knobs p = parse({{"GA_PIPE_FILL_PRIO", "high"}, {"GA_PIPE_SLOT_ORDER", "any"}, {"GA_PIPE_PINNED_IO", "1"}});
    CHECK(p.fill_prio && !p.fill_prio_normal && !p.fixed_order && p.pinned_io, "set, but not to the special values");
}

// Every expectation follows from the rules (the issue's table), not from a run of plan().
void test_plan() {
    const Knobs none = parse({});
    const int64_t C3 = 100000;
    {
        const Plan p = plan(problem(C3, C3), none, 4, 7, 0);
        CHECK(!p.serial && p.lane_td == 4 && p.lane_nwc == 4 && p.fills == 3 && p.slots == 4 && !p.chain &&
                  !p.chain_refused, "C3, 4 queues");
        const Plan q = plan(problem(C3, C3), none, 8, 7, 0);
        CHECK(q.lane_td == 4 && q.lane_nwc == 4 && q.fills == 4 && q.slots == 5, "C3, 8 queues");
        CHECK(plan(problem(C3, C3), none, 5, 7, 0).fills == 4, "five queues are enough");
    }
    // each lane condition alone sends the fills to the row scan (8 queues: the lane rule would give F = 4)
    const gaplan::Problem rows[] = {problem(32767, C3), problem(C3, 65535), problem(C3, C3, 1, 1, 33),
                                    problem(C3, C3, 1, 2), problem(C3, C3, 2)};
    for (const gaplan::Problem& pb : rows) {
        const Plan p = plan(pb, none, 8, 7, 0);
        CHECK(p.lane_td == 0 && p.lane_nwc == 0 && p.fills == 3 && p.slots == 4,
              "row: m %lld n %lld K %d qbytes %d CB %d", (long long)pb.m, (long long)pb.n, pb.K, pb.qbytes, pb.CB);
    }
    for (int fill_mode : {1, 2}) {  // GA_FILL_MODE=row|diag
        const Plan p = plan(problem(C3, C3), with_fill_mode(none, fill_mode), 8, 7, 0);
        CHECK(p.lane_td == 0 && p.lane_nwc == 0 && p.fills == 3 && p.slots == 4, "row: GA_FILL_MODE %d", fill_mode);
    }
    CHECK(plan(problem(32768, 65536), none, 4, 7, 0).lane_td == 4, "the smallest lane shape");
    CHECK(plan(problem(C3, C3, 1, 1, 32), with_fill_mode(none, 3), 4, 7, 0).lane_td == 4, "K = 32, GA_FILL_MODE=lane");
    CHECK(plan(problem(C3, C3), parse({{"GA_PIPE_MODE", "row"}}), 8, 7, 0).lane_td == 0, "MODE=row clears it");
    {
        const Knobs lane = parse({{"GA_PIPE_MODE", "lane"}});
        const Plan p = plan(problem(900, 1000), lane, 4, 7, 0);
        CHECK(p.lane_td == 4 && p.lane_nwc == 4 && p.fills == 3 && p.slots == 4, "MODE=lane at 900 x 1000");
        CHECK(plan(problem(900, 1000, 2), lane, 4, 7, 0).lane_td == 2, "MODE=lane with two-byte words");
        CHECK(plan(problem(900, 1000), with_fill_mode(lane, 1), 4, 7, 0).lane_td == 4, "MODE=lane over GA_FILL_MODE=row");
        CHECK(plan(problem(900, 1000, 1, 2), lane, 4, 7, 0).lane_td == 0, "MODE=lane needs an int8 profile");
        CHECK(plan(problem(900, 1000, 1, 1, 33), lane, 4, 7, 0).lane_td == 0, "MODE=lane needs K <= 32");
    }
    CHECK(plan(problem(900, 1000), parse({{"GA_PIPE_FILLS", "1"}}), 4, 7, 0).fills == 2, "FILLS=1");
    {
        const Plan p = plan(problem(900, 1000), parse({{"GA_PIPE_FILLS", "9"}}), 4, 7, 0);
        CHECK(p.fills == 4 && p.slots == 5, "FILLS=9");
    }
    CHECK(plan(problem(900, 1000), parse({{"GA_PIPE_SLOTS", "1"}}), 4, 7, 0).slots == 4, "SLOTS=1 with F = 3");
    CHECK(plan(problem(900, 1000), parse({{"GA_PIPE_SLOTS", "9"}}), 4, 7, 0).slots == 6, "SLOTS=9 with F = 3");
    CHECK(plan(problem(900, 1000), parse({{"GA_PIPE_SLOTS", "5"}}), 4, 7, 0).slots == 5, "SLOTS=5 with F = 3");
    CHECK(plan(problem(900, 1000), parse({{"GA_PIPE_SLOTS", "4"}, {"GA_PIPE_FILLS", "4"}}), 4, 7, 0).slots == 5,
          "SLOTS below F + 1");
    {
        // the chain: count * (m + n + 1) <= 256 Mi entries.  16 * 2^24 = 2^28; 2^28 + 1 = 17 * 15790321
        const Knobs ch = parse({{"GA_PIPE_CHAIN", "1"}});
        const Plan at = plan(problem(8388607, 8388608), ch, 4, 16, 0);
        CHECK(at.chain && !at.chain_refused, "chain at 256 Mi entries");
        CHECK(!plan(problem(7895160, 7895160), ch, 4, 17, 0).chain, "chain one entry above 256 Mi");
        CHECK(plan(problem(700, 650), ch, 4, 11, 0).chain, "chain asked");
        CHECK(!plan(problem(700, 650), none, 4, 11, 0).chain, "chain not asked");
        CHECK(!plan(problem(700, 650), parse({{"GA_PIPE_CHAIN", "0"}}), 4, 11, 0).chain, "chain = 0");
        for (const char* prio : {"normal", "high"})
            CHECK(!plan(problem(700, 650), parse({{"GA_PIPE_CHAIN", "1"}, {"GA_PIPE_FILL_PRIO", prio}}), 4, 11, 0).chain,
                  "chain with FILL_PRIO=%s", prio);
        const Plan s6 = plan(problem(700, 650), parse({{"GA_PIPE_CHAIN", "1"}, {"GA_PIPE_SLOTS", "6"}}), 4, 11, 0);
        CHECK(s6.slots == 6 && s6.chain == (6 <= kChainSlots) && s6.chain_refused == (6 > kChainSlots), "chain, six slots");
        CHECK(!plan(problem(700, 650), parse({{"GA_PIPE_CHAIN", "1"}, {"GA_PIPE_WALK_CUS", "1"}}, true), 4, 11, 0).chain,
              "chain with masked streams (experiments)");
        CHECK(!plan(problem(700, 650), parse({{"GA_PIPE_CHAIN", "1"}, {"GA_PIPE_ROW_FIRST", "0"}}, true), 4, 11, 0).chain,
              "chain with ROW_FIRST (experiments)");
        CHECK(plan(problem(700, 650), parse({{"GA_PIPE_CHAIN", "1"}, {"GA_PIPE_WALK_CUS", "1"}, {"GA_PIPE_ROW_FIRST", "1"}}),
                   4, 11, 0).chain, "the shipped build ignores both");
    }
    CHECK(plan(problem(900, 1000), none, 4, 1, 0).serial, "count 1");
    CHECK(plan(problem(2500, 3100), none, 4, 3, 512).serial, "banded tracebacks");
    CHECK(!plan(problem(900, 1000), none, 4, 2, 0).serial, "count 2");
    // 160 GiB of words in five slots: 5 * roundup(n, 64) * m * CB <= 160 * 2^30 = 171798691840.
    // n = 65536: m <= 171798691840 / 327680 = 524288 exactly
    CHECK(!plan(problem(524288, 65536), none, 4, 2, 0).serial, "160 GiB exactly");
    CHECK(plan(problem(524289, 65536), none, 4, 2, 0).serial, "one row past 160 GiB");
    // n = 100000 rounds up to 100032: 500160 * 343487 = 171798457920 fits, 233920 bytes below the bound
    CHECK(!plan(problem(343487, 100000), none, 4, 2, 0).serial, "the last m that fits at n = 100000");
    CHECK(plan(problem(343488, 100000), none, 4, 2, 0).serial, "the next m at n = 100000");
    CHECK(plan(problem(262145, 65536, 2), none, 4, 2, 0).serial && !plan(problem(262144, 65536, 2), none, 4, 2, 0).serial,
          "two-byte words halve it");
}

// ---------------------------------------------------------------- the feeder
constexpr int64_t kM = 700, kN = 799, kPer = kM + kN + 1;  // per = 1500
// dispatch counts of the played walks, each in [max(m, n), m + n]
const int64_t kWalks[] = {799, 1499, 1000, 1234, 900, 1499, 1111, 805};

// A consumer plays `count` walks as the pipeline's loops do (chain: the chain's look-ahead and a sink) and checks
// every slice it is given against the one-shot table.
void play(uint64_t seed, int count, bool chain) {
    uint32_t state[garng::MTN + 1];
    garng::seed_state(seed, state);
    const int64_t need = (int64_t)count * kPer;
    garng::RngTable ref;
    garng::build_rng(state, need, ref);
    garng::RngTable R;
    // never a table entry (its three low bits are clear): what the sink holds where nothing was published
    const uint32_t kStale = 0xffffffffu;
    std::vector<uint32_t> sink((size_t)need, kStale);
    long long word = 0;
    FeederSink sk;
    if (chain) sk = FeederSink{sink.data(), &word};
    TableFeeder feeder(R, state, kPer, count, sk);
    // the chain's reader: whatever the word publishes is in the sink, and the word only grows
    std::atomic<bool> done{false};
    std::thread watcher([&] {
        long long last = 0;
        while (chain && !done.load()) {
            const long long w = __atomic_load_n(&word, __ATOMIC_ACQUIRE);
            CHECK(w >= last && w <= need, "published word %lld after %lld (need %lld)", w, last, (long long)need);
            for (long long q = last; q < w; q++)
                if (sink[(size_t)q] != ref.tab[(size_t)q] || feeder.tab()[q] != ref.tab[(size_t)q]) {
                    CHECK(false, "sink entry %lld of %lld published", q, w);
                    break;
                }
            last = w;
            std::this_thread::yield();
        }
    });
    std::thread consumer([&] {
        int64_t G = 0, Dmax = 0;
        for (int k = 0; k < count; k++) {
            feeder.wait_ready(G + kPer);
            const uint32_t* tab = feeder.tab();
            int64_t bad = -1;
            for (int64_t q = G; q < G + kPer && bad < 0; q++)
                if (tab[q] != ref.tab[(size_t)q]) bad = q;
            CHECK(bad < 0, "seed %llu walk %d: entry %lld differs", (unsigned long long)seed, k, (long long)bad);
            const int64_t Dk = kWalks[k % 8];
            Dmax = std::max(Dmax, Dk);
            feeder.raise_target(chain ? G + Dk + 2 * kPer + kPer / 8 : G + Dk + kPer + Dmax + Dmax / 8);
            G += Dk;
        }
        feeder.stop();
        uint32_t got[garng::MTN + 1], want[garng::MTN + 1];
        garng::state_after(R, G, got);
        garng::state_after(ref, G, want);
        CHECK(!memcmp(got, want, sizeof(got)), "seed %llu: the state after %lld dispatches", (unsigned long long)seed,
              (long long)G);
    });
    consumer.join();
    done.store(true);
    watcher.join();
    feeder.stop();  // idempotent
    CHECK(feeder.tab() == R.tab.data(), "the table moved");
    CHECK(feeder.rng_ms() >= 0.0, "rng_ms");
    if (chain) {
        CHECK(word <= need && word == (long long)R.built, "the word at the end: %lld of %lld built", word, (long long)R.built);
        for (int64_t q = word; q < need; q++)
            if (sink[(size_t)q] != kStale) {
                CHECK(false, "sink entry %lld written past the published %lld", (long long)q, word);
                break;
            }
    }
}

void test_feeder_shutdown() {
    uint32_t state[garng::MTN + 1];
    garng::seed_state(12345, state);
    const int count = 100;
    const int64_t need = count * kPer;
    for (int pass = 0; pass < 4; pass++) {
        garng::RngTable R;
        std::vector<uint32_t> sink((size_t)need);
        long long word = 0;
        {
            TableFeeder feeder(R, state, kPer, count, pass & 1 ? FeederSink{sink.data(), &word} : FeederSink());
            feeder.raise_target(need);  // far ahead of what is built
            if (pass & 2) feeder.stop();  // (else the destructor's)
        }
        CHECK(R.built <= need && (!(pass & 1) || word == (long long)R.built), "pass %d: built %lld", pass, (long long)R.built);
    }
    // a feeder nobody ever asks for more, stopped at once
    garng::RngTable R;
    { TableFeeder feeder(R, state, kPer, count); }
    CHECK(R.built <= 3 * kPer, "the initial target is three alignments' worth");
}

void test_feeder_clamps() {
    uint32_t state[garng::MTN + 1];
    garng::seed_state(0, state);
    for (int count : {1, 2, 3}) {  // need <= 3 * per: the initial target covers everything
        const int64_t need = count * kPer;
        garng::RngTable ref, R;
        garng::build_rng(state, need, ref);
        TableFeeder feeder(R, state, kPer, count);
        feeder.wait_ready(need);
        CHECK(!memcmp(feeder.tab(), ref.tab.data(), sizeof(uint32_t) * (size_t)need), "count %d without a raise", count);
        feeder.raise_target(need + 12345);
        feeder.wait_ready(need + 12345);  // clamps: returns
    }
    const int count = 8;
    const int64_t need = count * kPer;
    garng::RngTable ref, R;
    garng::build_rng(state, need, ref);
    TableFeeder feeder(R, state, kPer, count);
    feeder.raise_target(10 * need);
    feeder.wait_ready(need);
    feeder.raise_target(INT64_MAX / 2);
    feeder.wait_ready(need + 1);
    feeder.stop();
    CHECK(R.built == need && !memcmp(feeder.tab(), ref.tab.data(), sizeof(uint32_t) * (size_t)need),
          "a target beyond the need builds everything and no more");
}

}  // namespace

int main() {
    test_knobs();
    test_plan();
    for (uint64_t seed : {(uint64_t)0, (uint64_t)12345})
        for (bool chain : {false, true}) {
            play(seed, 6, chain);
            play(seed, 2, chain);
        }
    test_feeder_shutdown();
    test_feeder_clamps();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures.load());
        return 1;
    }
    std::printf("ga_pipe_selftest: all checks passed\n");
    return 0;
}
