// ga_batch_rng_selftest.cpp -- CPU self-test of the device table generator's block-level pieces (ga_batch_rng.h),
// plain and under AddressSanitizer + UndefinedBehaviorSanitizer (make -C globalign_amd/csrc batch_rng_selftest
// batch_rng_asan; run by tests/test_batch_rng_host.py).  The model below drives the header's functions exactly as
// batch_rng_kernel does -- lane 0..63 in turn where the kernel's lanes run side by side, a loop's end where the kernel
// has a fence, chunks of 64 with all reads before the writes -- and must equal ga_rng.h's RngTable entry for entry.
// No HIP: the kernel is tested on the GPU; this binary covers the arithmetic it shares with the model.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ga_batch_rng.h"
#include "ga_rng.h"

using namespace gabrng;

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

struct Tables {
    uint16_t quad[kQuadEntries];
    uint32_t base[kN];
    Tables() {
        for (int x = 0; x < kQuadEntries; x++) quad[x] = quad_entry(x >> 8, x & 255);
        base_array(base);
    }
};
const Tables T;

// One wave's work on one item, as batch_rng_kernel does it.  Returns the status; blocks_out: blocks generated.
int32_t model_item(const Item& it, int words_per_dispatch, uint32_t* tab_all, int64_t* blocks_out = nullptr) {
    uint32_t mt[kN];
    uint8_t sym[kSymBytes], acc[kAccBytes];
    const int steps = it.steps;
    const int64_t blocks = max_blocks(steps, words_per_dispatch);
    uint32_t* tab = tab_all + it.tab_off;
    std::memcpy(mt, T.base, sizeof(mt));
    seed_array(mt, it.seed);
    int64_t done = 0, b = 0;
    uint32_t carry = 0;
    for (; b < blocks && done < steps; b++) {
        for (int c = 0; c < kTwistChunks; c++) {
            uint32_t v[kLanes];
            for (int lane = 0; lane < kLanes; lane++) v[lane] = twist_read(mt, c, lane);
            for (int lane = 0; lane < kLanes; lane++) twist_write(mt, c, lane, v[lane]);
        }
        uint32_t B[kLanes][kPasses], mine[kLanes][kPasses], total = 0;
        for (int lane = 0; lane < kLanes; lane++)
            for (int p = 0; p < kPasses; p++) B[lane][p] = symbols_lane(mt, p, lane, sym);
        for (int lane = 0; lane < kLanes; lane++) {
            const uint32_t t = run_automaton(T.quad, sym, carry, lane, mine[lane]);
            CHECK(lane == 0 || t == total, "the automaton's end differs between lanes");
            total = t;
        }
        for (int lane = 0; lane < kLanes; lane++)
            for (int p = 0; p < kPasses; p++) scatter_lane(T.quad, B[lane][p], mine[lane][p], p, lane, acc);
        uint8_t v[kLanes];
        for (int lane = 0; lane < kLanes; lane++) {
            entries_lane(acc, total, lane, done, steps, tab);
            v[lane] = carry_read(acc, total, lane);
        }
        for (int lane = 0; lane < kLanes; lane++) carry_write(acc, total, lane, v[lane]);
        CHECK(total / kDraws <= (uint32_t)kMaxBlockDispatches, "a block completed %u dispatches", total / kDraws);
        done += total / kDraws;
        carry = total % kDraws;
    }
    if (blocks_out) *blocks_out = b;
    return done >= steps ? kComplete : kCapReached;
}

std::vector<uint64_t> seeds_under_test() {
    std::vector<uint64_t> s = {0, 1, 0xffffffffull, 1ull << 32, (1ull << 32) + 1, 1ull << 63, ~0ull};
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (int k = 0; k < 200; k++) {  // half below 2^32 (one key word), half above
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        s.push_back(k & 1 ? x : x >> 33);
    }
    return s;
}
const int kSteps[] = {1, 4, 19, 20, 21, 39, 40, 700, 3000};

void test_seeding() {
    for (uint64_t seed : seeds_under_test()) {
        uint32_t want[garng::MTN + 1], mt[kN];
        garng::seed_state(seed, want);
        std::memcpy(mt, T.base, sizeof(mt));
        seed_array(mt, seed);
        CHECK(!std::memcmp(mt, want, sizeof(mt)), "seed_array(%llu)", (unsigned long long)seed);
    }
}

void test_twist_and_quartets() {
    // the chunked twist leaves CPython's array, three twists in a row; the packed quartet entry is Quad2's
    for (uint64_t seed : {0ull, 5ull, 1ull << 40}) {
        uint32_t st[garng::MTN + 1];
        garng::seed_state(seed, st);
        garng::PyMT g;
        std::memcpy(g.mt, st, sizeof(g.mt));
        uint32_t mt[kN];
        std::memcpy(mt, st, sizeof(mt));
        for (int round = 0; round < 3; round++) {
            g.twist();
            for (int c = 0; c < kTwistChunks; c++) {
                uint32_t v[kLanes];
                for (int lane = 0; lane < kLanes; lane++) v[lane] = twist_read(mt, c, lane);
                for (int lane = 0; lane < kLanes; lane++) twist_write(mt, c, lane, v[lane]);
            }
            CHECK(!std::memcmp(mt, g.mt, sizeof(mt)), "twist %d of seed %llu", round, (unsigned long long)seed);
        }
    }
    static const garng::Quad2 Q;
    for (int d = 0; d < kDraws; d++)
        for (int B = 0; B < 256; B++) {
            const garng::QuadEntry2& q = Q.e[d][B];
            const uint32_t e = quad_entry(d, B);
            bool same = entry_nacc(e) == q.nacc && entry_next(e) == q.nd;
            for (uint32_t x = 0; x < q.nacc; x++) same &= ((e >> (2 * x)) & 3u) == ((q.bytes >> (8 * x)) & 0xffu);
            CHECK(same, "quad_entry(%d, %d)", d, B);
        }
}

constexpr uint32_t kGuard = 0xA5A5A5A5u;  // no entry: bits 0 and 31 are never set

void test_tables() {
    int capped_24_long = 0, long_items = 0;
    for (uint64_t seed : seeds_under_test()) {
        garng::RngTable R;
        uint32_t st[garng::MTN + 1];
        garng::seed_state(seed, st);
        R.start(st);
        for (int steps : kSteps) {
            R.extend(steps);
            const int64_t words = R.step_end[(size_t)steps - 1];
            // guard words on both sides of the item's range
            std::vector<uint32_t> tab((size_t)steps + 8, kGuard);
            const Item it{seed, 4, steps, 0};
            int64_t blocks = 0;
            const int32_t st48 = model_item(it, kCapWordsPerDispatch, tab.data(), &blocks);
            CHECK(st48 == kComplete, "seed %llu steps %d: the default cap was reached", (unsigned long long)seed, steps);
            CHECK(words <= word_cap(steps, kCapWordsPerDispatch), "seed %llu steps %d: %lld words over the cap",
                  (unsigned long long)seed, steps, (long long)words);
            CHECK(blocks == (words + kN - 1) / kN, "seed %llu steps %d: %lld blocks for %lld words",
                  (unsigned long long)seed, steps, (long long)blocks, (long long)words);
            bool same = true, guards = true;
            for (int d = 0; d < steps; d++) same &= tab[(size_t)d + 4] == R.tab[(size_t)d];
            for (int g = 0; g < 4; g++) guards &= tab[(size_t)g] == kGuard && tab[(size_t)steps + 4 + g] == kGuard;
            CHECK(same, "seed %llu steps %d: entries differ from RngTable", (unsigned long long)seed, steps);
            CHECK(guards, "seed %llu steps %d: a write outside the item's range", (unsigned long long)seed, steps);

            // 24 words per dispatch are fewer than the 32 a dispatch takes on average: the item stops at the cap's
            // blocks, with status 1 exactly when it needed more words than they hold, the entries before the stop
            // right and nothing written past its range.  (A short item's cap is mostly its 624-word allowance, so
            // it may complete; from 700 dispatches on, 8 words per dispatch short, every item must stop.)
            std::fill(tab.begin(), tab.end(), kGuard);
            const int32_t st24 = model_item(it, 24, tab.data(), &blocks);
            const int64_t held = max_blocks(steps, 24) * kN;
            CHECK(st24 == (words > held ? kCapReached : kComplete), "seed %llu steps %d: status %d, %lld words, %lld held",
                  (unsigned long long)seed, steps, st24, (long long)words, (long long)held);
            CHECK(blocks <= max_blocks(steps, 24), "seed %llu steps %d: past the block bound", (unsigned long long)seed,
                  steps);
            same = guards = true;
            for (int d = 0; d < steps; d++) same &= tab[(size_t)d + 4] == R.tab[(size_t)d] || tab[(size_t)d + 4] == kGuard;
            for (int g = 0; g < 4; g++) guards &= tab[(size_t)g] == kGuard && tab[(size_t)steps + 4 + g] == kGuard;
            CHECK(same && guards, "seed %llu steps %d under cap 24: wrong entry or a write outside the range",
                  (unsigned long long)seed, steps);
            if (steps >= 700) {
                long_items++;
                capped_24_long += st24 == kCapReached;
            }
        }
    }
    CHECK(capped_24_long == long_items, "cap 24: %d of %d long items stopped", capped_24_long, long_items);
}

void test_cap_and_route() {
    CHECK(word_cap(0, 48) == 624 && word_cap(100, 48) == 5424 && word_cap(100, 24) == 3024, "word_cap");
    CHECK(max_blocks(0, 48) == 1 && max_blocks(1, 48) == 2 && max_blocks(13, 48) == 2 && max_blocks(14, 48) == 3, "max_blocks");
    CHECK(max_blocks(kDeviceMaxSteps, 48) == (48ll * kDeviceMaxSteps + 624 + 623) / 624, "max_blocks at the limit");
    const int64_t L = kDeviceMaxSteps;
    CHECK(route_device(true, L - 1, L) && route_device(true, L, L) && !route_device(true, L + 1, L), "route at the limit");
    CHECK(!route_device(false, L - 1, L) && !route_device(false, L, L) && !route_device(false, 1, L), "host asked for");
    CHECK(route_device(true, 300, 300) && !route_device(true, 301, 300) && !route_device(true, 1, 0), "other limits");
    CHECK(kDeviceMaxSteps > 0 && (kDeviceMaxSteps & (kDeviceMaxSteps - 1)) == 0, "the limit is a power of two");
}

}  // namespace

int main() {
    test_seeding();
    test_twist_and_quartets();
    test_tables();
    test_cap_and_route();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
