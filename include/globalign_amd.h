/*
 * globalign_amd.h -- C ABI of the MI355X affine-gap global-alignment engine.
 *
 * The reference (iamgiddyaboutgit/globalign) is pure CPython with no FFI; each
 * entry point below replaces the Python function(s) cited next to it
 * (paths relative to the reference's src/globalign/).  The Python host layer
 * (globalign_amd/_native.py) binds these with ctypes; INTEGRATION.md shows
 * the binding a globalign maintainer would add.
 *
 * Conventions: every function returns 0 on success or a negative GA_E* code;
 * ga_last_error() then describes the failure (thread-local).  Host buffers
 * are caller-owned; device buffers are owned by the context.  A context is
 * bound to one GPU and is not thread-safe (one per host thread).
 */
#ifndef GLOBALIGN_AMD_H
#define GLOBALIGN_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GA_OK 0
#define GA_E_ARG -1      /* invalid argument (maps to ValueError)          */
#define GA_E_HIP -2      /* HIP runtime failure (maps to RuntimeError)     */
#define GA_E_RANGE -3    /* int32 range / size limit exceeded               */
#define GA_E_STATE -4    /* call order violated (e.g. traceback before fill) */
#define GA_E_TIMEOUT -5  /* a device-side wait exceeded its spin bound      */
#define GA_E_NOMEM -6    /* device memory too small for the chosen path      */
#define GA_E_GUARD -7    /* guard mode: bytes outside a buffer were changed   */
#define GA_E_COUNT -8    /* ga_batch_support: a pair's count is not finite (maps to ValueError) */

/* Python-visible outcome of a traceback (dp_array_backward semantics). */
#define GA_TB_OK 0
#define GA_TB_INDEX_ERROR 1 /* the reference raises IndexError */

typedef struct ga_ctx ga_ctx;

/* Integer tables derived from the costing matrix (start.py:500-557).  Codes
 * index the alphabet in any fixed order; the gap character has a code too. */
typedef struct {
    int32_t K;              /* alphabet size including the gap code           */
    const int32_t* sub;     /* K*K: costing_mat[x][y]                         */
    const int32_t* gap_h;   /* K:   costing_mat['-'][y] (globaligner.py:347) */
    const int32_t* gap_v;   /* K:   costing_mat[x]['-'] (globaligner.py:357) */
    int32_t gap_open;       /* gap_open_cost >= 0                             */
    int32_t max_cost;       /* get_max_val(costing_mat) (start.py:488-497)   */
} ga_costs;

/* Last error message of this thread ("" if none). */
const char* ga_last_error(void);

/* Number of visible HIP devices. */
int ga_device_count(int* count);

/* Create / destroy a context on HIP device `device`.  ga_ctx_create reads the shipped GA_* environment knobs
 *  once; ga_ctx_create_opts also takes explicit options, "GA_NAME=VALUE" entries separated by ';' or
 * newlines (kernel variants for tests and tuning, fault injection, diagnostics: never read from the environment).
 * No reference counterpart: the reference has no device context. */
int ga_ctx_create(int device, ga_ctx** out);
int ga_ctx_create_opts(int device, const char* options, ga_ctx** out);
void ga_ctx_destroy(ga_ctx* ctx);

/* How the library was built: flags[0] bit 0 = an experiments build (measured-and-dropped paths compiled in). */
int ga_build_flags(int32_t* flags);

/* Load a problem: sequence codes (host), tables, optional custom boundaries.
 * Replaces make_dp_array (globaligner.py:756-821): when row0/col0 are NULL the
 * boundary is the reference's (finite sentinel big=(max_cost+1)*max(m,n));
 * otherwise row0 = 3*(n+1) and col0 = 3*(m+1) triples (M, X, Y) as in the
 * reference's own test (tests/globaligner_test.py:8-33).  Uploads to HBM. */
int ga_problem_set(ga_ctx* ctx, const uint8_t* a, int64_t m, const uint8_t* b, int64_t n, const ga_costs* costs,
                   const int32_t* row0, const int32_t* col0);

#define GA_FILL_TRACEBACK 1 /* store per-cell traceback words (needed by ga_problem_traceback) */
#define GA_FILL_FULL 2      /* also return every cell's (M, X, Y) (small problems only)       */

/* Matrix fill (dp_array_forward, globaligner.py:366-392 with
 * get_next_best_costs :317-363) on the loaded problem.  *cost_out receives
 * min(dp[m][n]) (globaligner.py:425).  With GA_FILL_FULL, full_out receives
 * 3*(m+1)*(n+1) int32 (row-major, boundary included). */
int ga_problem_fill(ga_ctx* ctx, int32_t flags, int64_t* cost_out, int32_t* full_out);

/* Costs of many pairs in one call, scores only (no traceback, no random
 * state).  For every pair this replaces make_dp_array (globaligner.py:756-821)
 * + dp_array_forward (:366-392) and the min of the last cell (:425), each pair
 * with its own sentinel big=(max_cost+1)*max(m,n): cost_out[k] is what
 * ga_problem_set + ga_problem_fill give for pair k.
 * codes holds every sequence's codes concatenated, sequence s being
 * codes[seq_off[s] .. seq_off[s+1]) (seq_off has nseq+1 entries, seq_off[0]
 * = 0); it is uploaded once, however many pairs use a sequence.  Pair k aligns
 * sequence pair_a[k] (seq_1, the rows) with sequence pair_b[k] (seq_2).
 * Every pair is checked as ga_problem_set checks a problem; the first failing
 * pair fails the call with that code and "pair <k>: ..." as the message, and
 * nothing is launched.  Short pairs share one kernel launch, one wave per
 * pair; a pair above GA_BATCH_MAX_CELLS cells (a context option, see
 * INTEGRATION.md), or one that does not fit that kernel's LDS or edge scratch,
 * takes the single-pair score fill.  The call works in a fresh context and
 * keeps buffers of its own, so a loaded problem stays loaded -- unless a pair
 * took the single-pair fill, which uses the context's problem slot: then no
 * problem is loaded afterwards (GA_E_STATE until the next ga_problem_set); on
 * a slab context (ga_problem_set_slab) such a call fails with GA_E_STATE and
 * leaves the slab as it is.
 * npairs = 0 returns GA_OK without a launch. */
int ga_batch_costs(ga_ctx* ctx, const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                   const int32_t* pair_b, int64_t npairs, const ga_costs* costs, int64_t* cost_out);
/* The same with a max_cost per pair (NULL: costs->max_cost for all, which is
 * ga_batch_costs).  The reference builds a match / mismatch costing matrix
 * over the letters of the two sequences it is given (start.py:431-468), so a
 * pair made of one letter has no mismatch entry, a smaller get_max_val
 * (start.py:488-497) and a smaller sentinel big than a pair scored under the
 * same settings with two letters or more; where big leaks into the optimum
 *  the cost differs.  pair_max_cost[k] is the maximum of pair
 * k's own matrix; the tables in `costs` may then span the whole batch's
 * alphabet. */
int ga_batch_costs_ex(ga_ctx* ctx, const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                      const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* costs,
                      int64_t* cost_out);

/* Alignments of many pairs in one call, strings included, every pair with a
 * random seed of its own.  For pair k this replaces random.seed(seeds[k])
 * followed by find_global_alignment (globaligner.py:258-302: make_dp_array,
 * dp_array_forward, dp_array_backward with cost_ranks_dispatcher's
 * random.choice calls): the strings, the cost and the traceback status are
 * what ga_problem_set + ga_problem_align give from the 625-word state
 * ga_debug_seed_state(seeds[k]) makes.  No state is returned: the pairs do not
 * share a random stream, so the results do not depend on the batch's order or
 * composition.
 * codes .. costs: as ga_batch_costs_ex, with the same checks and errors.
 * chars: the upper-cased sequences' characters, concatenated as codes is (one
 * byte each).  Pair k's strings go to out_a / out_mid / out_b at offset
 * out_off[k] (npairs + 1 entries; out_off[k+1] - out_off[k] is the pair's
 * capacity: m + n suffices for a pair whose sequences have two letters or
 * more, m + n + 1 for any pair), unterminated, out_len[k] bytes each;
 * tb_status[k] receives GA_TB_OK or GA_TB_INDEX_ERROR (possible only when a
 * sequence has one letter; out_len[k] is then 0), cost_out[k] the cost.
 * Short pairs share one kernel launch, one wave per pair filling and then
 * walking it.  The single-pair path (ga_problem_align) takes a pair with a
 * one-letter sequence, one above GA_BATCH_ALIGN_MAX_CELLS cells (a context
 * option), or one that does not fit the kernel's LDS, edge
 * scratch or traceback scratch; what ga_batch_costs says about loaded
 * problems and slab contexts holds here too.  The pairs' tie-break tables are
 * built on up to 8 host threads (option GA_BATCH_RNG_THREADS; 1: none).
 * npairs = 0 returns GA_OK without a launch. */
int ga_batch_align(ga_ctx* ctx, const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                   const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* costs,
                   const uint64_t* seeds, const char* chars, char* out_a, char* out_mid, char* out_b,
                   const int64_t* out_off, int64_t* out_len, int32_t* tb_status, int64_t* cost_out);
/* out6 = {kernel ms, host tie-break tables ms, host string decode ms, whole call wall ms, the walks' ns per
 * dispatch, the fills' ns per cell} of the last ga_batch_align.  All but the call's cover the pairs that shared
 * the kernel launch; the last two are averages of what each wave timed for its own pairs. */
int ga_batch_align_timings(ga_ctx* ctx, float* out6);
/* ga_batch_align with a choice of where the kernel pairs' tie-break tables are made.  flags bits 0-1:
 * GA_BATCH_TABLES_DEFAULT (the context's: host, or the device under option GA_BATCH_RNG=device),
 * GA_BATCH_TABLES_HOST (ga_batch_align's threads) or GA_BATCH_TABLES_DEVICE: batch_rng_kernel generates each
 * pair's MT19937 stream and its table on the GPU, ahead of the walks on the same stream, so neither the table
 * build nor its upload remains.  The results are the same byte for byte.  Other bits must be zero.
 * Under the device route a kernel pair of more than GA_BATCH_RNG_DEVICE_MAX_STEPS dispatches (m + n; option,
 * default 1024, at most 2^20) still gets a host table, built while the generator runs.  A generator item may
 * consume GA_BATCH_RNG_WORD_CAP * (m + n) + 624 words (option, default 48; a dispatch takes 32 on average); if
 * one reaches that cap, nothing of the launch is decoded and the kernel pairs run again with host tables.
 * ga_batch_align is this call with flags 0.  Slot 1 of ga_batch_align_timings is then the generator's time plus
 * the host table time it did not hide. */
#define GA_BATCH_TABLES_DEFAULT 0u
#define GA_BATCH_TABLES_HOST 1u
#define GA_BATCH_TABLES_DEVICE 2u
#define GA_BATCH_TABLES_MASK 3u
int ga_batch_align_ex(ga_ctx* ctx, const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                      const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* costs,
                      const uint64_t* seeds, const char* chars, char* out_a, char* out_mid, char* out_b,
                      const int64_t* out_off, int64_t* out_len, int32_t* tb_status, int64_t* cost_out, uint32_t flags);
/* out4 = {kernel pairs whose table the device made, kernel pairs whose table the host made, 1 when the generator
 * reached a word cap and the pairs were redone with host tables (the first two then describe the device attempt),
 * workgroups of the generator's launch} of the last ga_batch_align(_ex) or ga_debug_pair_tables. */
int ga_batch_align_info(ga_ctx* ctx, int32_t* out4);
/* Many seeded alignments of every pair from one fill of the pair.  Pair k has
 * the samples sample_off[k] .. sample_off[k + 1] (npairs + 1 entries, starting
 * at 0, not decreasing); sample f is aligned under seeds[f] and is, byte for
 * byte, entry f of ga_batch_align_ex on the pair lists with pair k repeated
 * once per sample: its strings go to out_a / out_mid / out_b at out_off[f]
 * (nsamples + 1 entries), out_len[f] bytes each, tb_status[f] receives GA_TB_OK
 * or GA_TB_INDEX_ERROR; cost_out[k] receives pair k's cost, which does not
 * depend on the seed.  codes .. costs, chars and flags are ga_batch_align_ex's,
 * with the same checks, errors ("pair <k>: ...") and table routes; under the
 * device route a walk launch whose generator reaches a word cap runs again with
 * host tables.
 * A kernel pair is filled once by batch_words_kernel, which keeps its traceback
 * words in a slice of the pair's own, and walked once per sample by
 * batch_walks_kernel, one wave per walk, in a later launch on the same stream.
 * The pairs are cut into fill chunks whose slices stay within
 * GA_BATCH_SAMPLE_CHUNK_WORDS u32 words (option, default 2^31: 8 GiB) and a
 * chunk's walks into launches of at most GA_BATCH_SAMPLE_WALK_ENTRIES table
 * entries (option, default 2^28: 1 GiB).  A pair of two letters or more a side
 * that leaves the kernel route (above GA_BATCH_ALIGN_MAX_CELLS cells, LDS, edge
 * scratch, or a slice over the chunk cap) is filled once by the single-pair
 * fill with stored traceback words, if they fit the traceback budget
 * (GA_TB_BUDGET_MB), and its samples are walked by the same kernel; any other
 * pair is looped sample by sample through ga_problem_align. */
int ga_batch_sample(ga_ctx* ctx, const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                    const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* costs,
                    const int64_t* sample_off, const uint64_t* seeds, const char* chars, char* out_a, char* out_mid,
                    char* out_b, const int64_t* out_off, int64_t* out_len, int32_t* tb_status, int64_t* cost_out,
                    uint32_t flags);
/* out8 = {pairs filled by batch_words_kernel, pairs filled by the single-pair fill, pairs looped sample by sample,
 * walk items, fill launches (batch_words_kernel's and single-pair fills), walk launches (a repeated one counts
 * twice), walk items whose table the device made, walk items whose table the host made} of the last
 * ga_batch_sample. */
int ga_batch_sample_info(ga_ctx* ctx, int64_t* out8);
/* out8 = {batch_words_kernel ms, batch_walks_kernel ms, tables ms (the generator's time plus the host table time it
 * did not hide), host string decode ms, whole call wall ms, the walks' ns per dispatch (average of what each wave
 * timed), single-pair fills ms, 0} of the last ga_batch_sample, summed over its launches. */
int ga_batch_sample_timings(ga_ctx* ctx, float* out8);
/* The number of co-optimal alignments of every pair: how many different
 * alignments the traceback can return for pair k over all tie-breaks, the
 * paths from (m, n) of the DAG its walk moves on.
 * count_out[k] receives it as a double -- the exact integer below 2^53, the
 * recurrence's double sum above, +inf past the double range, never NaN -- and
 * cost_out[k] pair k's cost.  codes .. costs are ga_batch_sample's, with the
 * same checks and errors ("pair <k>: ..."); no seeds, no tables, no strings.
 * Kernel pairs are filled chunk by chunk by batch_words_kernel as for
 * ga_batch_sample (GA_BATCH_ALIGN_MAX_CELLS, GA_BATCH_SAMPLE_CHUNK_WORDS) and
 * counted by batch_count_kernel, one wave per pair, in a later launch on the
 * same stream.  A pair that leaves the kernel route for its size is filled by
 * the single-pair fill with stored traceback words and counted by one wave of
 * the same kernel.  Refused with GA_E_ARG, before any launch and for the lowest
 * such pair: a pair with a one-letter sequence (the reference's traceback is
 * no path walk there) and a pair whose words exceed the traceback budget
 * (GA_TB_BUDGET_MB): there is no banded or recompute route for counting. */
int ga_batch_count(ga_ctx* ctx, const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                   const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* costs,
                   int64_t* cost_out, double* count_out);
/* out8 = {pairs counted on the kernel route, pairs counted from a single-pair fill, fill chunks, fill launches
 * (batch_words_kernel's and single-pair fills), count launches, pairs whose edge column went through HBM, 0, 0} of
 * the last ga_batch_count. */
int ga_batch_count_info(ga_ctx* ctx, int64_t* out8);
/* out8 = {batch_words_kernel ms, batch_count_kernel ms over those pairs, single-pair fills ms, batch_count_kernel ms
 * over their pairs, whole call wall ms, 0, 0, 0} of the last ga_batch_count, summed over its launches. */
int ga_batch_count_timings(ga_ctx* ctx, float* out8);
/* Co-optimal alignments by rank.  The alignments the traceback
 * can return for pair k are ordered by their level sequence as the traceback
 * emits it, from the alignment's last column backwards, lexicographically with
 * diagonal < gap in seq_1 < gap in seq_2; rank r names the r-th of them, from 0.
 * Pair k has the slots rank_off[k] .. rank_off[k + 1] (npairs + 1 entries from
 * 0, at most 2^31 - 1 slots; a pair without slots is legal: it is filled and
 * counted, nothing is walked) and slot f asks for rank ranks[f].  Its strings go
 * to out_a / out_mid / out_b at out_off[f] (slots + 1 entries, m + n characters
 * a slot at least), out_len[f] bytes each; rank_status[f] receives 0, or 1 for
 * a rank that is not below the pair's count: such a slot draws no walk and has
 * out_len[f] = 0.  count_out[k] receives min(count, 2^64 - 1) -- the counts are
 * u64 that saturate; every rank below that value is exact, whatever the true
 * count -- and cost_out[k] pair k's cost.  codes .. costs and chars are
 * ga_batch_sample's, with ga_batch_count's checks, errors ("pair <k>: ...") and
 * refusals.  No seeds, no tables, no random numbers.
 * Kernel pairs are filled chunk by chunk by batch_words_kernel as for
 * ga_batch_count; batch_rank_table_kernel, one wave per pair, keeps the three
 * path counts of every cell in the pair's table, 24 (m + 63) 64 T bytes a stripe
 * of 64 T columns, and batch_rank_walk_kernel walks a pair once per slot, one
 * lane per walk, 64 slots of a pair to a wave; both are later launches on the
 * same stream.  A chunk closes when its words would exceed
 * GA_BATCH_SAMPLE_CHUNK_WORDS or its tables GA_BATCH_RANK_TABLE_BYTES (option,
 * default 2^33: 8 GiB); a pair whose own table exceeds that is refused with
 * GA_E_ARG before any launch, the lowest such pair first.  A chunk's walks are
 * cut into launches of at most GA_BATCH_SAMPLE_WALK_ENTRIES steps (m + n a
 * slot).  A pair that leaves the kernel route for its size is filled by the
 * single-pair fill with stored traceback words; one wave makes its table and
 * the same walk kernel walks it. */
int ga_batch_rank(ga_ctx* ctx, const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                  const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* costs,
                  const int64_t* rank_off, const uint64_t* ranks, const char* chars, char* out_a, char* out_mid,
                  char* out_b, const int64_t* out_off, int64_t* out_len, int32_t* rank_status, int64_t* cost_out,
                  uint64_t* count_out);
/* out8 = {pairs on the kernel route, pairs filled by the single-pair fill, fill chunks, fill launches
 * (batch_words_kernel's and single-pair fills), table launches, walk launches, slots walked, pairs with a saturated
 * count} of the last ga_batch_rank. */
int ga_batch_rank_info(ga_ctx* ctx, int64_t* out8);
/* out8 = {batch_words_kernel ms, batch_rank_table_kernel ms over those pairs, batch_rank_walk_kernel ms, host string
 * decode ms, whole call wall ms, the walks' ns per step (what each wave timed over the steps of its 64 lanes),
 * single-pair fills ms, batch_rank_table_kernel ms over their pairs} of the last ga_batch_rank, summed over its
 * launches. */
int ga_batch_rank_timings(ga_ctx* ctx, float* out8);
/* Match support: for every pair k and every cell (i, j), how
 * many of the pair's co-optimal alignments (ga_batch_count's family) align
 * letter i of seq_1 with letter j of seq_2:
 *   support(i, j) = A_0(i, j) * N(i-1, j-1, 0),
 * A_0 the number of walk prefixes from (m, n) that leave cell (i, j) by the
 * diagonal and N the number of paths from the cell they enter on, all in IEEE
 * double in a fixed order: the exact integer while count_out[k] < 2^53, the
 * recurrence's double above.  Pair k's m * n doubles go to support_out at
 * support_off[k], row-major (npairs + 1 entries from 0, at least m * n doubles
 * a pair); count_out[k] and cost_out[k] are ga_batch_count's.  codes .. costs,
 * checks, errors ("pair <k>: ...") and refusals are ga_batch_count's.
 * Kernel pairs are filled chunk by chunk by batch_words_kernel as for
 * ga_batch_count; batch_support_table_kernel, one wave per pair, keeps N(i, j, 0)
 * in the pair's table (ga_batch_rank's layout and size), batch_flow_kernel, one
 * wave per pair, runs the wavefront backwards over the same words and leaves
 * the supports in the same table, and batch_support_gather_kernel makes the
 * dense rows; all are later launches on the same stream.  A chunk closes when
 * its words would exceed GA_BATCH_SAMPLE_CHUNK_WORDS, its tables
 * GA_BATCH_RANK_TABLE_BYTES or its dense output GA_BATCH_SUPPORT_BYTES (option,
 * default 2^31: 2 GiB); a pair whose own table or output exceeds its cap is
 * refused with GA_E_ARG before any launch, the lowest such pair first.  A pair
 * that leaves the kernel route for its size is filled by the single-pair fill
 * with stored traceback words and handled by one wave of the same kernels.
 * After the counts are back, a pair whose count is not finite (+inf: its
 * supports would be 0 * inf) fails the call with GA_E_COUNT, the lowest such
 * pair named; the outputs are then unspecified. */
int ga_batch_support(ga_ctx* ctx, const uint8_t* codes, const int64_t* seq_off, int64_t nseq, const int32_t* pair_a,
                     const int32_t* pair_b, const int32_t* pair_max_cost, int64_t npairs, const ga_costs* costs,
                     const int64_t* support_off, double* support_out, int64_t* cost_out, double* count_out);
/* out8 = {pairs on the kernel route, pairs filled by the single-pair fill, fill chunks, fill launches
 * (batch_words_kernel's and single-pair fills), support launch sets (N table, flow, gather), pairs whose edge column
 * went through HBM, 0, 0} of the last ga_batch_support. */
int ga_batch_support_info(ga_ctx* ctx, int64_t* out8);
/* out8 = {batch_words_kernel ms, batch_support_table_kernel ms, batch_flow_kernel ms, batch_support_gather_kernel ms
 * over those pairs, single-pair fills ms, and the three kernels' ms over their pairs} of the last ga_batch_support,
 * summed over its launches. */
int ga_batch_support_timings(ga_ctx* ctx, float* out8);
/* The tie-break tables alone, with no alignment: item t's steps[t] entries under seeds[t], concatenated in
 * tab_out, by route 1 (host) or 2 (device; an item over GA_BATCH_RNG_DEVICE_MAX_STEPS is built on the host, as
 * in the real call).  status_out[t]: 0 complete, 1 the word cap was reached (entries past the stop are
 * 0xA5A5A5A5, which no entry equals), 2 a word outside the item's range was written.  Afterwards slot 1 of
 * ga_batch_align_timings holds the generator's time. */
int ga_debug_pair_tables(ga_ctx* ctx, const uint64_t* seeds, const int32_t* steps, int64_t nitems, int32_t route,
                         uint32_t* tab_out, int32_t* status_out);
/* random.seed(seed) for an int seed (Modules/_randommodule.c random_seed): the 625 words of
 * random.getstate()[1] it leaves.  CPU only. */
int ga_debug_seed_state(uint64_t seed, uint32_t* state_out);

/* Traceback walk (dp_array_backward :395-593, cost_ranks_dispatcher
 * :595-685, take_* :688-753) on the last GA_FILL_TRACEBACK fill.
 * mt_state: 625 words = random.getstate()[1] in, the state after the
 * reference's random.choice calls out.  a_chr/b_chr: the upper-cased
 * sequences.  out_* need cap >= m+n+1 bytes; strings are not terminated.
 * *tb_status receives GA_TB_OK or GA_TB_INDEX_ERROR. */
int ga_problem_traceback(ga_ctx* ctx, uint32_t* mt_state, const char* a_chr, const char* b_chr, char* out_a,
                         char* out_mid, char* out_b, int64_t cap, int64_t* out_len, int32_t* tb_status);

/* Use a caller-filled cell array for the next ga_problem_traceback instead of
 * a fill: cells = 3*(m+1)*(n+1) int32 (M, X, Y), row-major, boundary
 * included (the loaded problem's row0/col0 must be its row 0 / column 0).
 * Replaces the part of dp_array_backward (globaligner.py:425-514) that reads
 * the caller's dp_array: the walk then follows THOSE cells, whatever filled
 * them.  *cost_out = min(cells[m][n]).  Small problems only. */
int ga_problem_set_cells(ga_ctx* ctx, const int32_t* cells, int64_t* cost_out);

/* fill + traceback in one call, overlapping the host-side tie-break table
 * with the device fill (the whole find_global_alignment hot path,
 * globaligner.py:258-302). */
int ga_problem_align(ga_ctx* ctx, uint32_t* mt_state, const char* a_chr, const char* b_chr, char* out_a,
                     char* out_mid, char* out_b, int64_t cap, int64_t* out_len, int32_t* tb_status,
                     int64_t* cost_out);

/* `count` consecutive alignments of the loaded pair, exactly as `count`
 * consecutive find_global_alignment calls make them: alignment k starts from
 * the random state alignment k-1 left (repeated calls sample the co-optimal
 * alignments the reference's tie-breaks reach).  The walk of alignment k runs
 * on a second stream beside the fill of alignment k+1 (double-buffered
 * traceback words; the tie-break table is one continuous MT19937 stream), so
 * the throughput is one fill per alignment.  out_a/out_mid/out_b: count*cap
 * bytes, alignment k at offset k*cap; out_len, tb_status, cost_out: count
 * entries; mt_state: in the state before the first alignment, out the state
 * after the last. */
int ga_problem_align_many(ga_ctx* ctx, int32_t count, uint32_t* mt_state, const char* a_chr, const char* b_chr,
                          char* out_a, char* out_mid, char* out_b, int64_t cap, int64_t* out_len, int32_t* tb_status,
                          int64_t* cost_out);

/* ---- multi-GPU column slabs ----------------------------------
 * A context can own the column slab [col_begin, col_end) of a larger problem
 * (global m, n and boundary).  Its left edge arrives in `halo_in`
 * ((m+1) x int2 of (H', h1') in the shifted space of DESIGN.md) guarded by
 * the progress word `halo_in_prog` (rows available, written by the host when
 * a band has arrived); its right edge is produced into `halo_out` with the
 * progress word `halo_out_prog` (rows published by the fill).  Both words are
 * HOST pointers into pinned coherent memory that the running fill reads and
 * writes, so the host can stream bands with RCCL send/recv without blocking
 * a device queue. */
int ga_problem_set_slab(ga_ctx* ctx, const uint8_t* a, int64_t m, const uint8_t* b, int64_t n, const ga_costs* costs,
                        int64_t col_begin, int64_t col_end);
int ga_slab_buffers(ga_ctx* ctx, void** halo_in, uint32_t** halo_in_prog, void** halo_out, uint32_t** halo_out_prog);
/* Use caller-owned device buffers ((m+1) x int2 each) as the slab's left-edge
 * input and right-edge output (e.g. tensors that RCCL receives into / sends
 * from); NULL keeps the context's own buffer.  Their progress goes through the context's own
 * words (ga_slab_buffers): this undoes a ga_slab_link / _export / _import. */
int ga_slab_bind_halos(ga_ctx* ctx, void* halo_in, void* halo_out);
/* Join two neighbouring slab contexts of ONE process (GlobalAligner(devices=[...])) device to device: the
 * right context allocates its left edge (m + 1 int2 rows) and a progress word in uncached device memory
 * on its own GPU, and the left context's fill writes both directly -- system-scope stores, over xGMI
 * when the contexts sit on different GPUs (peer access is enabled here) -- while the right context's
 * fill polls the word.  No host thread relays anything.  Call after ga_problem_set_slab on both
 * contexts and before either fill is launched (it zeroes the word); launch left before right.
 * Replaces the pinned-host halos + host relay of round 2 (reference: none -- the reference is
 * single-threaded CPU code). */
int ga_slab_link(ga_ctx* left, ga_ctx* right);
/* The same link between two PROCESSES (one GPU each, bench.py --gpus N): the right slab's context allocates
 * its left edge + progress word (uncached, on its GPU; zeroing the word) and exports an IPC handle
 * (HIP_IPC_HANDLE_SIZE = 64 bytes); the left slab's context maps it (hipIpcOpenMemHandle, peer access
 * enabled lazily; kept while the handle stays the same) and its fill stores the edge there directly.
 * Per problem: export on the right, hand the bytes over (any channel), import on the left, and launch
 * the left fill only after the right side's export returned (the word is zero). */
int ga_slab_link_export(ga_ctx* right, void* handle_out);
int ga_slab_link_import(ga_ctx* left, const void* handle);
/* Let `device` read and write `peer`'s memory (hipDeviceEnablePeerAccess); GA_OK if already enabled. */
int ga_enable_peer_access(int device, int peer);
/* Launch the slab fill asynchronously on the context's compute stream. */
int ga_slab_fill_launch(ga_ctx* ctx, int32_t flags);
/* Wait for the slab fill; returns H'(m, col_end) un-shifted (only meaningful on the last slab). */
int ga_slab_fill_finish(ga_ctx* ctx, int64_t* cost_out);

/* Traceback across slabs (dp_array_backward :395-593 cut at slab edges): the
 * walk starts on the slab owning column n and moves right to left; each slab
 * continues the state its right neighbour handed over. */
typedef struct {
    int64_t i, j;   /* current cell (j: global column)                        */
    int64_t D, h;   /* dispatches so far; moves after the first one            */
    int32_t L;      /* level the walk entered the cell with (0 M, 1 X, 2 Y)    */
    int32_t first;  /* 1 before the first move                                 */
    int32_t reason; /* -1 running; 0..4 ended (as the whole-problem walk);
                       5 reached this slab's left edge (continue on the left)  */
    int32_t pad;
} ga_walk_state;
/* Build the host tie-break table of the global problem from the 625-word MT
 * state (call while the fill runs). */
int ga_slab_walk_prepare(ga_ctx* ctx, const uint32_t* mt_state);
/* Walk this slab from *st (j must be the slab's right edge); writes the
 * alignment columns it produced in walk order (not reversed, no tails) and
 * updates *st.  a_chr / b_chr: the whole upper-cased sequences. */
int ga_slab_walk(ga_ctx* ctx, ga_walk_state* st, const char* a_chr, const char* b_chr, char* out_a, char* out_mid,
                 char* out_b, int64_t cap, int64_t* out_len);
/* MT state after the first D dispatches (random.getstate()[1] layout). */
int ga_slab_mt_state(ga_ctx* ctx, int64_t D, uint32_t* mt_state_out);
/* Enqueue on `stream` (a hipStream_t): wait until *prog >= value / write value to *prog. */
int ga_stream_wait_ge(void* stream, uint32_t* prog, uint32_t value);
int ga_stream_write(void* stream, uint32_t* prog, uint32_t value);
/* The context's compute stream (hipStream_t).  It is created with the
 * device's greatest stream priority, so it owns a hardware queue that no
 * normal-priority stream (torch's, RCCL's) shares: a slab fill waiting on its
 * halo never holds up the RCCL kernel that delivers it. */
void* ga_ctx_stream(ga_ctx* ctx);
/* Order the context's stream after all work enqueued so far on `stream`
 * (a hipStream_t, e.g. torch.cuda.current_stream().cuda_stream): buffers that
 * stream allocated or initialised are then safe for the next fill. */
int ga_ctx_wait_stream(ga_ctx* ctx, void* stream);
/* The priority the context's stream was created with (hipDeviceGetStreamPriorityRange units). */
int ga_ctx_stream_priority(ga_ctx* ctx, int* priority);

/* ---- guard mode (tests) ------------------------
 * Under the context option GA_GUARD_BYTES=G every device and pinned buffer of
 * the context has G pattern bytes in front of and behind its payload, and every
 * entry that runs kernels and waits for them checks them before it returns:
 * GA_E_GUARD, with ga_last_error naming buffer, side, offset of the first
 * changed byte relative to the payload, count and payload size.  No reference
 * counterpart.
 * ga_debug_guard_report: the same check without an error, as JSON text
 * {"guard_bytes", "fill", "poison", "violations": [{"name", "side", "offset",
 * "last", "changed", "payload"}], "buffers": [{"name", "payload", "guarded"}]}
 * (buffers: the allocated ones).  *needed receives the text's size with its
 * terminator; it is written when cap suffices.  It repairs nothing.
 * ga_debug_guard_poke: a host-side copy of nbytes bytes that differ from the
 * pattern into a guard of buffer `name` (side 0 front, 1 rear; offset counts
 * from that guard's first byte), so that a test can see the check report it;
 * it cannot leave the guard.  Both need guard mode (GA_E_STATE without). */
int ga_debug_guard_report(ga_ctx* ctx, char* out, int64_t cap, int64_t* needed);
int ga_debug_guard_poke(ga_ctx* ctx, const char* name, int32_t side, int64_t offset, int64_t nbytes);

/* ---- measurement --------------------------------------------------------- */
/* Device time (ms, HIP events on the launch stream) of the last fill kernel
 * and of the last traceback walk kernel. */
int ga_last_kernel_ms(ga_ctx* ctx, float* fill_ms, float* walk_ms);
/* out4 = {fill kernel ms, walk kernel ms, host tie-break table ms, whole ga_problem_align wall ms}. */
int ga_last_timings(ga_ctx* ctx, float* out4);

#ifdef __cplusplus
}
#endif
#endif
