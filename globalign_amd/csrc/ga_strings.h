// ga_strings.h -- a walk's packed levels to the three alignment strings (dp_array_backward's output,
// globaligner.py:514-586).  No HIP: built into the engine (every walk of ga_host.cpp and ga_batch_align.h's
// decode_levels go through it) and into ga_batch_align_selftest.cpp under AddressSanitizer / UBSan.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace gastr {

// seq[k] as Python indexes it: -1 is the last letter (the reference's first step at m == 1 / n == 1 reads seq[-1])
inline int64_t pywrap(int64_t k, int64_t L) { return k < 0 ? k + L : k; }

// The columns of one walk, in walk order, resumable: (i, j, L, len) carry from one decode() to the next, so a walk's
// dispatches may be decoded in any number of pieces, while it still runs (streamed_walk_finish) or a slab / band at a
// time.  len counts on past cap without writing; the caller reports the overflow.
struct Columns {
    const char* a_chr;  // seq_1's m letters
    int64_t m;
    const char* b_chr;  // seq_2's n letters
    int64_t n;
    char *oa, *om, *ob;  // out: seq_1's row, the middle row, seq_2's row
    int64_t cap;
    int64_t i, j;  // the cell the next dispatch leaves
    int L = 0;     // the last level taken
    int64_t len = 0;

    // Dispatches [D0, D1) of the walk out of `words`, whose first word is word `word0` of the walk's: levels are packed
    // 2 bits per dispatch, dispatch k at bits 30 - 2 * (k & 15) of word k >> 4.  Level 0 takes a column of both
    // sequences, 1 a gap above seq_2's letter, 2 seq_1's letter above a gap.
    // Lenient (the single-pair walks, whose kernel keeps the reference's quirks): letters are indexed as Python would
    // (pywrap), a level 3 is taken as level 2; always true.
    // STRICT (the batch walks, which stay inside the matrix): false ("does not decode") at a step from i < 1 or j < 1
    // or at a level 3, before anything is read for that step.
    template <bool STRICT>
    bool decode(const uint32_t* words, int64_t word0, int64_t D0, int64_t D1) {
        int64_t ci = i, cj = j, cl = len;
        int lv = L;
        bool ok = true;
        for (int64_t k = D0; k < D1; k++) {
            if (STRICT && (ci < 1 || cj < 1)) { ok = false; break; }
            const char ca = a_chr[STRICT ? ci - 1 : pywrap(ci - 1, m)], cb = b_chr[STRICT ? cj - 1 : pywrap(cj - 1, n)];
            lv = (int)((words[(k >> 4) - word0] >> (30 - 2 * (k & 15))) & 3u);
            if (STRICT && lv == 3) { ok = false; break; }
            if (cl < cap) {
                oa[cl] = lv == 1 ? '-' : ca;
                om[cl] = lv != 0 ? ' ' : ca == cb ? '|' : '*';
                ob[cl] = lv >= 2 ? '-' : cb;
            }
            cl++;
            ci -= lv != 1;
            cj -= lv < 2;
        }
        i = ci;
        j = cj;
        L = lv;
        len = cl;
        return ok;
    }
};

// The end of a walk that stopped at (i, j) with len columns decoded: the reference's tail for a walk that ended in
// row 0 (reason 1: the rest of seq_2 under gaps) or column 0 (reason 2: the rest of seq_1 over gaps), then the
// reversal of all three rows (:584-586).  Returns the length; past cap nothing is reversed.
inline int64_t finish_strings(int reason, int64_t i, int64_t j, const char* a_chr, const char* b_chr, char* oa, char* om,
                              char* ob, int64_t cap, int64_t len) {
    auto put = [&](char x, char y, char z) {
        if (len < cap) { oa[len] = x; om[len] = y; ob[len] = z; }
        len++;
    };
    if (reason == 1)
        for (int64_t jj = j; jj > 0; jj--) put('-', ' ', b_chr[jj - 1]);
    else if (reason == 2)
        for (int64_t ii = i; ii > 0; ii--) put(a_chr[ii - 1], ' ', '-');
    if (len <= cap) {
        std::reverse(oa, oa + len);
        std::reverse(om, om + len);
        std::reverse(ob, ob + len);
    }
    return len;
}

}  // namespace gastr
