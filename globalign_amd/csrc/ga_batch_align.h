// ga_batch_align.h -- the host's share of a batch of alignments with strings (ga_batch_align; no HIP: built into
// the engine and into ga_batch_align_selftest.cpp under AddressSanitizer / UBSan / ThreadSanitizer).
//
// Every walk of a batch (a pair of ga_batch_align, a sample of ga_batch_sample) has a tie-break stream of its own,
// the one `random.seed(seed)` starts, so the walks do not depend on each other.  A walk's table is one gabrng::Item
// (seed, tab_off, steps): split_tables divides a launch's jobs between the device generator (ga_batch_rng.h) and the
// host and names the host jobs' upload ranges, build_tables makes the host jobs' tables (ga_rng.h) on a few threads,
// and decode_walk / decode_levels turn a finished walk's packed levels into the three alignment strings with the
// engine's one decoder (ga_strings.h) in its strict mode, checking that the levels lead to the end cell the walk
// reported.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "ga_batch.h"
#include "ga_batch_rng.h"
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

// tab[jobs[t].tab_off .. + jobs[t].steps): the entries of job t under jobs[t].seed; no two jobs share entries.
inline void build_tables(const gabrng::Item* jobs, int64_t njobs, int nthreads, uint32_t* tab) {
    run_shares(njobs, nthreads, [=](int64_t first, int64_t stride) {
        garng::RngTable R;
        uint32_t state[garng::MTN + 1];
        for (int64_t t = first; t < njobs; t += stride) {
            garng::seed_state(jobs[t].seed, state);
            R.start(state);
            R.extend(jobs[t].steps);
            std::copy(R.tab.begin(), R.tab.begin() + jobs[t].steps, tab + jobs[t].tab_off);
        }
    });
}

// A job list by gabrng::route_device: the generator's jobs and the host's, each in list order (dev_at: a device
// job's place in the list), and the host jobs' entries as the ranges [first, last) they are uploaded in -- in list
// order, a range grows only while the next host job's tab_off is its end.
struct TableRange {
    int64_t first, last;
};
struct TableSplit {
    std::vector<gabrng::Item> dev, host;
    std::vector<int64_t> dev_at;
    std::vector<TableRange> ranges;
};
inline TableSplit split_tables(const gabrng::Item* jobs, int64_t njobs, bool want_device, int64_t max_steps) {
    TableSplit sp;
    for (int64_t t = 0; t < njobs; t++) {
        const gabrng::Item& jb = jobs[t];
        if (gabrng::route_device(want_device, jb.steps, max_steps)) {
            sp.dev.push_back(jb);
            sp.dev_at.push_back(t);
            continue;
        }
        sp.host.push_back(jb);
        if (jb.steps <= 0) continue;
        if (sp.ranges.empty() || sp.ranges.back().last != jb.tab_off)
            sp.ranges.push_back(TableRange{jb.tab_off, jb.tab_off});
        sp.ranges.back().last += jb.steps;
    }
    return sp;
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

// Where a batch's strings go: walk or sample `slot` has out_off[slot + 1] - out_off[slot] characters at out_off[slot]
// of each of the three buffers, its length in out_len[slot] and its traceback status in tb_status[slot].
struct WalkOut {
    const char* chars;  // every sequence's characters, at its codes' offsets
    char *out_a, *out_mid, *out_b;
    const int64_t* out_off;
    int64_t* out_len;
    int32_t* tb_status;
};

// A finished walk of `it` to its slot: wr are the walk's result words {dispatches, i_end, j_end, reason}, ops its
// level words; no_fit: the launch reported that the item did not fit it.  Sets tb_status and out_len and returns
// out_len: the length, or -3 (no_fit), -2 (dispatches outside [0, m + n], or levels that do not decode) or -1
// (decode_levels).
inline int64_t decode_walk(const ga_batch_item& it, const int32_t* wr, const uint32_t* ops, int64_t slot, bool no_fit,
                           const WalkOut& o) {
    const int64_t at = o.out_off[slot];
    o.tb_status[slot] = GA_TB_OK;
    return o.out_len[slot] = no_fit ? -3
                             : wr[0] < 0 || wr[0] > (int64_t)it.m + it.n
                                 ? -2
                                 : decode_levels(ops, wr[0], it.m, it.n, wr[1], wr[2], wr[3], o.chars + it.a_off,
                                                 o.chars + it.b_off, o.out_a + at, o.out_mid + at, o.out_b + at,
                                                 o.out_off[slot + 1] - at);
}

}  // namespace gabatch
