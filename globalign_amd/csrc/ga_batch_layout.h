// ga_batch_layout.h -- where a cell's traceback word lies, for the walks of ga_batch.hip (no HIP: built into the
// kernels' translation unit and into ga_batch_sample_selftest.cpp).
//
// LAYOUT_BATCH: the words batch_pair writes (ga_batch.h): 4 / CB rows of a column to a u32, rows of u32s `geom` =
// 64 * T * nstripes apart.  LAYOUT_STRIPE: the single-pair fills' (ga_device.h, "Traceback word layout"): stripes of
// 64 columns, per stripe s and lane l 16-byte words of SPC = 16 / CB rows, `geom` = TC of them per lane:
//   byte ((s * TC + q) * 64 + l) * 16 + ((i - 1) % SPC) * CB,  q = (i - 1) / SPC.
// SPC * CB = 16 and CB divides 4, so a cell's CB bytes lie inside one aligned dword in either layout.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GA_LAYOUT_HD __host__ __device__ __forceinline__
#else
#define GA_LAYOUT_HD inline
#endif

namespace gabatch {

constexpr int LAYOUT_BATCH = 0;
constexpr int LAYOUT_STRIPE = 1;

// cell (i, j), 1-based: the index of its u32 in the pair's words, and the shift of its CB bytes inside that u32
template <int CB, int LAYOUT>
struct TbAddr {
    static constexpr int RPW = 4 / CB;
    static GA_LAYOUT_HD unsigned long long word(int i, int j, int geom) {
        if (LAYOUT == LAYOUT_BATCH) return (unsigned)((i - 1) / RPW) * (unsigned)geom + (unsigned)(j - 1);
        constexpr int SPC = 16 / CB;
        const unsigned long long s = (unsigned)(j - 1) >> 6, l = (unsigned)(j - 1) & 63u, q = (unsigned)(i - 1) / SPC;
        return ((s * (unsigned long long)geom + q) * 64 + l) * 4 + ((unsigned)(i - 1) % SPC) / RPW;
    }
    static GA_LAYOUT_HD int shift(int i) { return ((i - 1) & (RPW - 1)) * 8 * CB; }
};

// u32 words of a LAYOUT_STRIPE pair of n columns at TC 16-byte words per lane
inline long long stripe_words(long long n, long long TC) { return (n + 63) / 64 * TC * 64 * 4; }

}  // namespace gabatch
