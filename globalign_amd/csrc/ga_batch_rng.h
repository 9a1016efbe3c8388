// ga_batch_rng.h -- the block-level pieces of the device's tie-break table generator (batch_rng_kernel,
// ga_batch_rng.hip).  No HIP: the kernel includes it, and so does its CPU model in
// ga_batch_rng_selftest.cpp, which runs the same functions lane by lane against ga_rng.h's RngTable.
//
// One wave makes one work item's table: tab[tab_off .. tab_off + steps) of the stream random.seed(seed) starts.
// random.seed(int) leaves the state index at 624, so the stream is whole 624-word blocks.  Per block the wave
//   1. twists the MT array in LDS in chunks of 64 words, all of a chunk's reads before its writes (the update
//      m[k] = tw(m[k], m[k+1], m[k+397]) reads new values only at distance 227 > 64);
//   2. tempers every word, keeps its top two bits (every draw is getrandbits(2)) and packs four words' symbols
//      into a quartet byte;
//   3. steps the acceptance automaton -- the draw index 0..17 -- over the 156 quartets, the same in every lane,
//      each lane keeping the (accepted so far, draw index) at the quartets it packed;
//   4. scatters its quartets' accepted draws to their places, builds the entries of the dispatches that completed
//      (draws 0-3 and 9-12, ga_rng.h fill_entries) and stores them; the draws of the unfinished dispatch (< 18)
//      move to the front for the next block.
// Every function takes the lane as an argument: the kernel calls it with its own, the model for lane 0..63 in turn,
// with the kernel's fences where the model's loops end.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GA_RNG_FN __host__ __device__ __forceinline__
#define GA_RNG_PRAGMA(x) _Pragma(#x)
#else
#define GA_RNG_FN inline
#define GA_RNG_PRAGMA(x)
#endif

namespace gabrng {

constexpr int kN = 624, kM = 397;           // MT19937
constexpr int kLanes = 64;
constexpr int kTwistChunks = (kN + kLanes - 1) / kLanes;        // 10, the last of 48 words
constexpr int kQuartets = kN / 4;                               // 156
constexpr int kPasses = (kQuartets + kLanes - 1) / kLanes;      // 3 quartets per lane, the last pass of 28
constexpr int kDraws = 18;                                      // accepted draws per dispatch
constexpr int kSymBytes = 160;                                  // the block's quartet bytes, rounded to words
constexpr int kAccBytes = 648;                                  // carried draws (<= 17) + at most 624 accepted
constexpr int kMaxBlockDispatches = (kDraws - 1 + kN) / kDraws; // 35: one entry per lane is enough
static_assert(kMaxBlockDispatches <= kLanes, "a block's dispatches fit one pass of the wave");
static_assert(kDraws - 1 + kN <= kAccBytes && kQuartets <= kSymBytes, "LDS rows");
constexpr int kWavesPerGroup = 4;           // work item = workgroup * kWavesPerGroup + wave

// A work item may consume word_cap(steps) words before it gives up (status kCapReached).  A dispatch takes 32.0
// words on average (6 draws of 3 at 4/3 words, 12 draws of 2 at 2 words); over 204 seeds x 1500 dispatches the
// words after D dispatches stayed below 0.67 * (48 D + 624).
constexpr int kCapWordsPerDispatch = 48;
// Items of more dispatches than this are built on the host (GA_BATCH_RNG_DEVICE_MAX_STEPS): a lone wave is slower
// per dispatch than a host thread (about 380 ns against 27 ns), and one long item would be the launch's tail.  The
// largest power of two at which a lone item's generator time (0.46 ms at 1024, 0.84 ms at 2048, 3.1 ms at 8192) stays
// below batch_align_kernel's time for 1024 BLOSUM62 pairs of 100-600 letters (0.55 ms) on an MI355X.
constexpr int kDeviceMaxSteps = 1024;
constexpr int32_t kComplete = 0, kCapReached = 1;

struct Item {
    uint64_t seed;
    int64_t tab_off;  // its entries go to tab[tab_off .. tab_off + steps)
    int32_t steps;    // dispatches: m + n
    int32_t pad;
};

GA_RNG_FN int64_t word_cap(int64_t steps, int64_t words_per_dispatch) {
    return words_per_dispatch * steps + kN;
}
// the block loop's bound: whole blocks that hold the cap
GA_RNG_FN int64_t max_blocks(int64_t steps, int64_t words_per_dispatch) {
    return (word_cap(steps, words_per_dispatch) + kN - 1) / kN;
}
// the route of one kernel item: the device when the call asks for it and the item is not too long
GA_RNG_FN bool route_device(bool want_device, int64_t steps, int64_t device_max_steps) {
    return want_device && steps <= device_max_steps;
}

// ------------------------------------------------------------------ seeding
// init_genrand(19650218): the array init_by_array starts from, the same for every seed (uploaded once per context)
inline void base_array(uint32_t* mt) {
    mt[0] = 19650218u;
    for (int k = 1; k < kN; k++) mt[k] = 1812433253u * (mt[k - 1] ^ (mt[k - 1] >> 30)) + (uint32_t)k;
}
// init_by_array over the seed's one or two 32-bit chunks, on mt = base_array (ga_rng.h seed_state; serial)
GA_RNG_FN void seed_array(uint32_t* mt, uint64_t seed) {
    const uint32_t key0 = (uint32_t)seed, key1 = (uint32_t)(seed >> 32);
    const bool two = key1 != 0;
    int i = 1;
    uint32_t j = 0, prev = mt[0];
    for (int k = kN; k; k--) {
        prev = (mt[i] ^ ((prev ^ (prev >> 30)) * 1664525u)) + (j ? key1 : key0) + j;
        mt[i] = prev;
        j = two ? j ^ 1u : 0u;
        if (++i >= kN) {
            mt[0] = prev;
            i = 1;
        }
    }
    for (int k = kN - 1; k; k--) {
        prev = (mt[i] ^ ((prev ^ (prev >> 30)) * 1566083941u)) - (uint32_t)i;
        mt[i] = prev;
        if (++i >= kN) {
            mt[0] = prev;
            i = 1;
        }
    }
    mt[0] = 0x80000000u;
}

// ------------------------------------------------------------------ twist, temper, symbols
GA_RNG_FN uint32_t tw(uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
    return c ^ (y >> 1) ^ ((0u - (y & 1u)) & 0x9908b0dfu);
}
// word 64 * chunk + lane of the next block, from the array as the earlier chunks left it (0 past the array)
GA_RNG_FN uint32_t twist_read(const uint32_t* mt, int chunk, int lane) {
    const int k = kLanes * chunk + lane;
    if (k >= kN) return 0;
    const int k1 = k + 1 < kN ? k + 1 : 0, km = k + kM < kN ? k + kM : k + kM - kN;
    return tw(mt[k], mt[k1], mt[km]);
}
GA_RNG_FN void twist_write(uint32_t* mt, int chunk, int lane, uint32_t v) {
    const int k = kLanes * chunk + lane;
    if (k < kN) mt[k] = v;
}
// getrandbits(2) of a word: the top two bits of its tempering
GA_RNG_FN uint32_t symbol(uint32_t y) {
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y >> 30;
}
// the quartet byte of words 4q .. 4q + 3 for q = 64 * pass + lane, also stored to sym[q] (0, unstored, past 155)
GA_RNG_FN uint32_t symbols_lane(const uint32_t* mt, int pass, int lane, uint8_t* sym) {
    const int q = kLanes * pass + lane;
    if (q >= kQuartets) return 0;
    const uint32_t B = symbol(mt[4 * q]) | (symbol(mt[4 * q + 1]) << 2) | (symbol(mt[4 * q + 2]) << 4) |
                       (symbol(mt[4 * q + 3]) << 6);
    sym[q] = (uint8_t)B;
    return B;
}

// ------------------------------------------------------------------ the acceptance automaton
// random.choice's sequence length at draw d of a dispatch: 3 at d = 0, 4, 8, 9, 13, 17, else 2
GA_RNG_FN uint32_t draw_size(uint32_t d) { return 2u + ((0x22311u >> d) & 1u); }
// The quartet table's entry for draw index d and quartet byte B (ga_rng.h Quad2, packed): the accepted values two
// bits each in order (bits 0-7), how many were accepted (bits 8-10), the draw index afterwards (bits 11-15).
GA_RNG_FN uint16_t quad_entry(uint32_t d, uint32_t B) {
    uint32_t vals = 0, nacc = 0;
    GA_RNG_PRAGMA(unroll)
    for (int w = 0; w < 4; w++) {
        const uint32_t r = (B >> (2 * w)) & 3u;
        if (r < draw_size(d)) {
            vals |= r << (2 * nacc);
            nacc++;
            d = d == kDraws - 1 ? 0 : d + 1;
        }
    }
    return (uint16_t)(vals | (nacc << 8) | (d << 11));
}
GA_RNG_FN uint32_t entry_nacc(uint32_t e) { return (e >> 8) & 7u; }
GA_RNG_FN uint32_t entry_next(uint32_t e) { return e >> 11; }
constexpr int kQuadEntries = kDraws * 256;

// The automaton over the block's quartets from `carry` accepted draws of the unfinished dispatch (its draw index):
// the same steps in every lane, no lane-dependent branch.  mine[pass] = accepted before | draw index << 16 at the
// lane's own quartet of each pass.  Returns the accepted draws at the block's end, the carried ones included.
GA_RNG_FN uint32_t run_automaton(const uint16_t* Q, const uint8_t* sym, uint32_t carry, int lane,
                                 uint32_t (&mine)[kPasses]) {
    uint32_t p = carry, d = carry;
    for (int pass = 0; pass < kPasses; pass++) {
        const int nq = kQuartets - kLanes * pass < kLanes ? kQuartets - kLanes * pass : kLanes;
        uint32_t keep = 0;
        GA_RNG_PRAGMA(unroll 4)
        for (int x = 0; x < nq; x++) {
            keep = x == lane ? (p | (d << 16)) : keep;
            const uint32_t e = Q[d * 256 + sym[kLanes * pass + x]];
            p += entry_nacc(e);
            d = entry_next(e);
        }
        mine[pass] = keep;
    }
    return p;
}
// the accepted draws of the lane's quartet of `pass` to their places in acc
GA_RNG_FN void scatter_lane(const uint16_t* Q, uint32_t B, uint32_t mine, int pass, int lane, uint8_t* acc) {
    if (kLanes * pass + lane >= kQuartets) return;
    const uint32_t p = mine & 0xffffu, e = Q[(mine >> 16) * 256 + B], n = entry_nacc(e);
    GA_RNG_PRAGMA(unroll)
    for (uint32_t x = 0; x < 4; x++)
        if (x < n) acc[p + x] = (uint8_t)((e >> (2 * x)) & 3u);
}

// ------------------------------------------------------------------ entries
// A dispatch's entry from its 18 accepted draws (ga_rng.h fill_entries): per half, the levels of the rank sets
// S = 1..7 are 0, 1, q[1], 2, 2 q[2], 1 + q[3], q[0] with q = draws 9 * half .., at bits 2S + 1 + 14 * half.
GA_RNG_FN uint32_t pack_entry(const uint8_t* r) {
    uint32_t e = 0;
    for (int half = 0; half < 2; half++) {
        const uint8_t* q = r + 9 * half;
        const uint32_t h = (1u << 5) | ((uint32_t)q[1] << 7) | (2u << 9) | (2u * q[2] << 11) | ((1u + q[3]) << 13) |
                           ((uint32_t)q[0] << 15);
        e |= h << (14 * half);
    }
    return e;
}
// Lane `lane` stores the entry of the block's lane-th completed dispatch, item dispatch done + lane, when the block
// completed that many and the item has that many.  total: run_automaton's result.
GA_RNG_FN void entries_lane(const uint8_t* acc, uint32_t total, int lane, int64_t done, int64_t steps, uint32_t* tab) {
    if ((uint32_t)lane < total / kDraws && done + lane < steps) tab[done + lane] = pack_entry(acc + kDraws * lane);
}
// the unfinished dispatch's draws move to the front: read, (fence,) write
GA_RNG_FN uint8_t carry_read(const uint8_t* acc, uint32_t total, int lane) {
    return (uint32_t)lane < total % kDraws ? acc[total / kDraws * kDraws + lane] : 0;
}
GA_RNG_FN void carry_write(uint8_t* acc, uint32_t total, int lane, uint8_t v) {
    if ((uint32_t)lane < total % kDraws) acc[lane] = v;
}

}  // namespace gabrng
