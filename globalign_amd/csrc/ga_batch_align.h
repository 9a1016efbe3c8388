// ga_batch_align.h -- the host's share of a batch of alignments with strings (ga_batch_align; no HIP: built into
// the engine and into ga_batch_align_selftest.cpp under AddressSanitizer / UBSan / ThreadSanitizer).
//
// Every pair of the batch walks with a tie-break stream of its own, the one `random.seed(seed)` starts, so the walks
// do not depend on each other: build_pair_tables makes the kernel pairs' tables (ga_rng.h) on a few threads, and
// decode_levels turns a finished walk's packed levels into the three alignment strings with the engine's one decoder
// (ga_strings.h) in its strict mode, checking that the levels lead to the end cell the walk reported.  Under the
// device route (ga_batch_align_ex, ga_batch_rng.h) build_pair_tables makes only the tables of the items that stay
// on the host.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "ga_batch.h"
#include "ga_rng.h"
#include "ga_strings.h"

namespace gabatch {

constexpr int kMaxRngThreads = 8;

// Threads for the tables of nitems pairs.  requested > 0 (GA_BATCH_RNG_THREADS): that many, 1 meaning sequential;
// else one per 64 pairs, never more than the machine reports.  At most kMaxRngThreads either way.
inline int rng_threads(int requested, int64_t nitems) {
    int64_t nt = requested > 0 ? requested : (nitems + 63) / 64;
    if (requested <= 0) {
        const unsigned hc = std::thread::hardware_concurrency();
        if (hc > 0) nt = std::min<int64_t>(nt, hc);
    }
    return (int)std::max<int64_t>(1, std::min<int64_t>(nt, kMaxRngThreads));
}

// share(first, stride) on nthreads threads (the caller's among them): thread q gets (q, nthreads) and takes the
// work items q, q + nthreads, ... -- the list is sorted longest first, so the shares are even.
template <typename Share>
inline void run_shares(int64_t nitems, int nthreads, Share share) {
    nthreads = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(nthreads, kMaxRngThreads), nitems));
    if (nthreads == 1) return share(0, 1);
    std::vector<std::thread> pool;
    for (int q = 1; q < nthreads; q++) pool.emplace_back(share, q, nthreads);
    share(0, nthreads);
    for (std::thread& th : pool) th.join();
}

// tab[walk[t].tab_off .. + m + n): the entries of work item t under seeds[items[t].out]; no two items share entries.
inline void build_pair_tables(const ga_batch_item* items, const ga_batch_walk_item* walk, int64_t nitems,
                              const uint64_t* seeds, int nthreads, uint32_t* tab) {
    run_shares(nitems, nthreads, [=](int64_t first, int64_t stride) {
        garng::RngTable R;
        uint32_t state[garng::MTN + 1];
        for (int64_t t = first; t < nitems; t += stride) {
            const int64_t steps = (int64_t)items[t].m + items[t].n;
            garng::seed_state(seeds[items[t].out], state);
            R.start(state);
            R.extend(steps);
            std::copy(R.tab.begin(), R.tab.begin() + steps, tab + walk[t].tab_off);
        }
    });
}

// The strings of one walk from (m, n): the levels of dispatches [0, D) out of `ops` through ga_strings.h's strict
// decode, then its tail for `reason` and the reversal.  Returns the length, -1 when it exceeds cap, -2 when the levels
// do not lead to (i_end, j_end) inside the matrix.
inline int64_t decode_levels(const uint32_t* ops, int64_t D, int64_t m, int64_t n, int64_t i_end, int64_t j_end,
                             int reason, const char* a_chr, const char* b_chr, char* oa, char* om, char* ob,
                             int64_t cap) {
    gastr::Columns col{a_chr, m, b_chr, n, oa, om, ob, cap, m, n};
    if (!col.decode<true>(ops, 0, 0, D)) return -2;
    if (col.i != i_end || col.j != j_end || (col.i > 0 && col.j > 0)) return -2;
    const int64_t len = gastr::finish_strings(reason, col.i, col.j, a_chr, b_chr, oa, om, ob, cap, col.len);
    return len > cap ? -1 : len;
}

}  // namespace gabatch
