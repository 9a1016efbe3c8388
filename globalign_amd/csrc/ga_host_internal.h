// ga_host_internal.h -- what the host engine's four translation units share (ga_host.cpp: contexts, the fill, slabs;
// ga_align_host.cpp: one alignment's traceback; ga_batch_host.cpp: the batched calls; ga_pipe_host.cpp: the
// repeated-alignment pipeline).  Internal: not installed, and include/globalign_amd.h does not mention it.  The shared
// helpers live in namespace gahost and are defined in the file named above each group.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/globalign_amd.h"
#include "ga_device.h"
#include "ga_guard.h"
#include "ga_opts.h"
#include "ga_pipe.h"
#include "ga_plan.h"
#include "ga_rng.h"
#include "ga_walk_plan.h"

namespace gahost {

extern thread_local std::string g_err;
int fail(int code, const std::string& msg);

#define HIPCHK(expr)                                                                               \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(GA_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));              \
    } while (0)

// ------------------------------------------------------------------ buffers
struct DevBuf;
struct PinBuf;
// Guard mode (ga_guard.h; options GA_GUARD_BYTES / GA_GUARD_FILL / GA_GUARD_POISON, never the
// environment): one per context, shared by its buffers and its pipeline slots'.  Every buffer is allocated with G
// bytes of a pattern in front of and behind what its kernels may write, and guard_check reads them back.
struct GuardCfg {
    size_t G = 0;
    uint8_t fill = (uint8_t)gaguard::kDefaultFill;
    bool poison = false;   // the payload starts as the pattern too
    // the chained pipeline's persistent kernel runs (align_chain sets it around the launch): that kernel waits for
    // this thread, so nothing may wait for the device or free memory; a buffer that asks for another size then is refused
    bool in_chain = false;
    std::vector<DevBuf*> dev;
    std::vector<PinBuf*> pin;
    // what a re-lay or a reallocation found in the guard it was about to overwrite, kept for the next check
    std::vector<gaguard::Violation> pending;
};

// Device memory that grows on demand and is released with its owner (a context or a pipeline slot): nothing copies
// one, FillBufs, Band and the launches' argument structs hold pointers into it.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool uncached = false;
    // guard mode (nullptr: off): p and cap are what they are without it -- the kernels' pointer and budget -- inside
    // an allocation of goff + cap + goff bytes; size is the last request, where the rear guard begins
    GuardCfg* g = nullptr;
    size_t goff = 0, size = 0;
    std::string name;
    explicit DevBuf(bool uncached_ = false) : uncached(uncached_) {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t ensure(size_t bytes) {
        if (g) return ensure_guarded(bytes);
        if (bytes <= cap && p) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max<size_t>(bytes, 256);
        hipError_t e = uncached ? hipExtMallocWithFlags(&p, want, hipDeviceMallocUncached) : hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    hipError_t ensure_guarded(size_t bytes);
    void release() {
        if (p) (void)hipFree(static_cast<uint8_t*>(p) - goff);
        p = nullptr;
        cap = goff = size = 0;
    }
    // release() outside the destructor: in guard mode what the guards caught is kept for the next check first
    void release_checked();
    template <typename T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

// Its pinned-host counterpart: plain pinned memory (staging for asynchronous copies), or mapped and coherent, which the
// device reads and writes in place through dev().  It grows by free-then-allocate at the ensure() call, never later: a
// free while a persistent kernel polls host memory would wait for that kernel (align_chain).
struct PinBuf {
    void* p = nullptr;
    void* dp = nullptr;  // the same memory as the device sees it (mapped buffers), looked up once per allocation
    size_t cap = 0;
    bool mapped = false;
    GuardCfg* g = nullptr;  // guard mode, as DevBuf's
    size_t goff = 0, size = 0;
    std::string name;
    explicit PinBuf(bool mapped_ = false) : mapped(mapped_) {}
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() {
        if (p) (void)hipHostFree(static_cast<uint8_t*>(p) - goff);
    }
    hipError_t ensure(size_t bytes) {
        if (g) return ensure_guarded(bytes);
        if (bytes <= cap && p) return hipSuccess;
        void* old = p;
        p = dp = nullptr;
        cap = 0;
        if (old)
            if (hipError_t e = hipHostFree(old); e != hipSuccess) return e;
        const unsigned flags = mapped ? hipHostMallocMapped | hipHostMallocCoherent : hipHostMallocDefault;
        hipError_t e = hipHostMalloc(&p, bytes, flags);
        if (e == hipSuccess && mapped) e = hipHostGetDevicePointer(&dp, p, 0);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    hipError_t ensure_guarded(size_t bytes);
    template <typename T>
    T* host() const { return static_cast<T*>(p); }
    template <typename T>
    T* dev() const { return static_cast<T*>(dp); }
};

// The buffers one fill writes, and its two timing events (created and destroyed by their owner): the context has
// one set, every pipeline slot one of its own, so that fills can run side by side.
struct FillBufs {
    DevBuf tb;                 // traceback words
    DevBuf hand;               // workgroup hand-off edges
    DevBuf flags;              // [0] ticket, [1] abort
    DevBuf out_last;           // H'(m, n)
    DevBuf GVp, GHp, top, left, bnd_row, bnd_col, meta, bscr;  // the boundary pass's output (make_dp_array) and scratch
    hipEvent_t ev[2] = {nullptr, nullptr};
    // the boundary arrays of an m x n_all problem, and the fill's four result words
    hipError_t ensure_boundary(int64_t m, int64_t n_all) {
        const std::pair<DevBuf*, size_t> want[] = {
            {&bnd_row, sizeof(int) * 3 * (n_all + 1)}, {&bnd_col, sizeof(int) * 3 * (m + 1)},
            {&GVp, sizeof(int) * (m + 1)},             {&bscr, sizeof(int) * ga::boundary_scratch_ints((int)m, (int)n_all)},
            {&GHp, sizeof(int) * (n_all + 1)},         {&top, sizeof(int2) * (n_all + 1)},
            {&left, sizeof(int2) * (m + 1)},           {&meta, sizeof(int) * 8},
            {&out_last, sizeof(int) * 4}};
        for (const auto& [buf, bytes] : want)
            if (hipError_t e = buf->ensure(bytes); e != hipSuccess) return e;
        return hipSuccess;
    }
};


// Pipelined repeated alignments (ga_problem_align_many, ga_pipe_host.cpp): what the context keeps
// between calls.  A slot holds one alignment's boundary arrays, traceback words, walk buffers and events; fills run
// on streams of their own, the walk on another beside them.
struct PipeSlot {
    FillBufs fb;  // each pipelined alignment computes its own boundary (make_dp_array) into its slot
    DevBuf rng, ops, result;
    hipEvent_t fdone = nullptr, w0 = nullptr, w1 = nullptr;
    PinBuf tab_pin;  // pinned staging of the walk's table slice
};
struct Pipeline {
    PipeSlot slot[gapipe::kMaxSlots];
    hipStream_t wstream = nullptr, fstream[4] = {nullptr, nullptr, nullptr, nullptr};  // [0] unused: ctx->stream
    // CU-masked pipeline streams (GA_PIPE_WALK_CUS > 0): the walk keeps CUs of its own, the fills the rest
    hipStream_t mwstream = nullptr, mfstream[4] = {nullptr, nullptr, nullptr, nullptr};
    // default-priority pipeline fill streams (GA_PIPE_FILL_PRIO=normal): four fills on their own pool of
    // hardware queues, the walk stream keeping the greatest priority (it takes the next free CU)
    hipStream_t nfstream[4] = {nullptr, nullptr, nullptr, nullptr};
    int walk_cus = -1;  // CUs reserved for the walk (0: no masks; -1: not yet set up)
    PinBuf pin;         // ("pipe_pin") pinned: per slot {out_last[4], GV(m), GH(n), abort, pad}
    gapipe::Plan plan;  // the current call's (ga_pipe.h)
    garng::RngTable rng;  // the calls' one continuous tie-break stream (gapipe::TableFeeder extends it)
    // chained pipeline walks (walk_chain_kernel): the tie-break stream in pinned, coherent host memory
    // and the control words {fills done, walks done, abort, timed out, entries written (8 B at [4])}
    PinBuf chain_tab{true}, chain_ctl{true};
    // the chain's stream, at the LEAST priority: HIP gives each priority its own pool of hardware
    // queues, and no other stream of the process uses this pool, so no fill can ever be queued behind
    // the persistent chain on an in-order queue it shares (the chain waits for those fills)
    hipStream_t cwstream = nullptr;
    // per slot, pinned and coherent: the walk's result words and levels, written by the chain straight
    // into host memory (a hipMemcpy would wait for a CU, and the fills hold them all)
    PinBuf chain_io{true};
    ~Pipeline() {  // its streams and events (the context's device is current: ga_ctx_destroy)
        for (auto& sl : slot)
            for (hipEvent_t e : {sl.fb.ev[0], sl.fb.ev[1], sl.fdone, sl.w0, sl.w1})
                if (e) (void)hipEventDestroy(e);
        for (hipStream_t st : {wstream, cwstream, mwstream, mfstream[0], mfstream[1], mfstream[2], mfstream[3],
                               nfstream[0], nfstream[1], nfstream[2], nfstream[3], fstream[1], fstream[2], fstream[3]})
            if (st) (void)hipStreamDestroy(st);
    }
};

}  // namespace gahost
// (ga_ctx is the C ABI's type and stays global: it names these five; the .cpp files open gahost themselves)
using gahost::DevBuf;
using gahost::FillBufs;
using gahost::GuardCfg;
using gahost::PinBuf;
using garng::RngTable;

struct ga_ctx {
    // GA_* tuning / diagnostic overrides, snapshotted when the context is created (ga_ctx_create_opts): the
    // environment's shipped knobs (gaopts::kEnvKnobs) at that moment, then the caller's options.  A context's kernel choices
    // never change under it, whatever the process does to its environment later.  Read once, there, into the typed
    // sets below (pk, wk, lk, bk, pipek); kept because pipek.trace points into it.
    gaopts::Map knobs;
    int device = 0;
    int priority = 0;  // of `stream` (the greatest the device offers, see ga_ctx_create)
    hipStream_t stream = nullptr;
    hipEvent_t ev_dep = nullptr;  // ga_ctx_wait_stream
    hipEvent_t wev[2] = {nullptr, nullptr};  // the walk's timing events (the fill's: fb.ev)
    // problem
    bool loaded = false, custom = false, filled_tb = false;
    int64_t m = 0, n = 0;      // local problem (slab: n = local columns)
    int64_t n_global = 0, col0 = 0;
    int K = 0, o = 0, big = 0, CB = 1, qbytes = 1;
    int64_t gh_total = 0;      // GH(n_global): the sum of the horizontal gap costs of seq_2
    int64_t gh_max = 0;        // max over j = 1 .. n_global of GH(j): with gap costs of mixed sign GH is not monotone
    int64_t gv_total = 0;      // GV(m): the sum of the vertical gap costs of seq_1
    // a streamed single call's small results in pinned, coherent host memory (no copy after the walk): [0, 16) the
    // walk's result words (it writes them there), [16, 20) the fill's H'(m, n) words, [20] its abort word (copied on
    // the upload stream while the walk runs)
    PinBuf res_pin{true};
    hipEvent_t ev_fill = nullptr, ev_res = nullptr;
    bool rc_pos_zeroed = false;  // rc_pos was cleared on the fill's stream before the fill (rc_align)
    int qrows = 1024, num_cu = 256;  // the row scan's query-profile ring (load_problem)
    gaplan::Knobs pk;          // the planner's knobs, parsed once (ga_plan.h)
    gawalk::Knobs wk;          // the traceback call's, parsed once (ga_walk_plan.h)
    gaopts::LaneKnobs lk;      // the lane fill's launch knobs and the batched calls', parsed once (ga_opts.h)
    gaopts::BatchKnobs bk;
    gapipe::Knobs pipek;       // the pipeline's, parsed once (ga_pipe.h), diag_req copied in from pk
    // the last enqueued fill's plan (ga_plan.h): kernel, geometry, checkpoint spacing; before the first fill the
    // loaded problem's row-scan geometry
    gaplan::FillPlan plan;
    int64_t GV_m = 0, GH_n = 0;
    std::vector<uint8_t> h_a, h_b;
    // device buffers
    DevBuf a, b, sub, gh, gv, qp, full, rng, ckpt, ops, result;
    FillBufs fb;  // what a fill writes
    DevBuf halo_in{true};  // uncached
    bool slab = false;
    // slab progress words in pinned, coherent host memory: [0] halo_in rows (written by the host
    // when a band has arrived), [1] halo_out rows (written by the fill's IO wave)
    PinBuf prog{true};
    int2* halo_in_ext = nullptr;   // caller-bound halo buffers (e.g. tensors RCCL sends from / receives into)
    int2* halo_out_ext = nullptr;
    // caller-bound progress words (device-visible; e.g. on the reading GPU, written over xGMI by the
    // writing GPU's fill): nullptr keeps prog_dev[0] / prog_dev[1]
    uint32_t* in_prog_ext = nullptr;
    uint32_t* out_prog_ext = nullptr;
    RngTable walk_rng;             // tie-break table of the global problem (slab walks)
    int hw_queues = 4;             // GPU_MAX_HW_QUEUES as the process first saw it (ga_ctx_create)
    gahost::Pipeline pipe;         // pipelined repeated alignments (ga_problem_align_many)
    bool walk_rng_ready = false;
    float fill_ms = 0.f, walk_ms = 0.f, rng_ms = 0.f, call_ms = 0.f;
    bool dbg_on = false;
    int walk_waits = 0, walk_tiles = 0, walk_t_tile = 0, walk_t_ring = 0, walk_t_total = 0, walk_c_total = 0, walk_load_ticks = 0, walk_load_count = 0;
    DevBuf dbg, wdbg;
    // the recompute walk: the score fill's checkpoints, the tile cache, the blocks' flags
    DevBuf colck, stck, rc_tb, rc_flags, rc_pos, rc_own;
    DevBuf qprof;  // the lane fill's query profile (ga::launch_lane_qprof), rebuilt by every lane fill
    // ga_batch_costs: buffers of its own, so a loaded problem's stay as they are -- every sequence's
    // codes, the work list, sub' / gap tables, the ticket word, the costs, the waves' HBM edge columns
    DevBuf bt_codes, bt_items, bt_sub, bt_gh, bt_gv, bt_ticket, bt_out, bt_scratch;
    // ga_batch_align adds the walk items, the pairs' tie-break tables, their packed levels and walk
    // results, and the waves' traceback words; ga_batch_align_timings's figures of its last call
    DevBuf bt_witems, bt_rng, bt_ops, bt_walk, bt_tb;
    float batch_align_ms[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // [4], [5]: walk ns per dispatch, fill ns per cell
    // the device route of the pairs' tables (batch_rng_kernel): its work items, status words and the seeding's base
    // array (uploaded once), its own timing events, and ga_batch_align_info's figures of the last call
    DevBuf bt_ritems, bt_rstatus, bt_rbase;
    bool rbase_ready = false;
    hipEvent_t rev[2] = {nullptr, nullptr};  // (created with the first generator launch)
    int32_t batch_rng_info[4] = {0, 0, 0, 0};  // device-routed items, host-routed items, fell back, generator blocks
    // The stored-words fill (ga_batch_host.cpp enqueue_chunk_fill, large_route) adds the pairs' slices
    // (ga_batch_words_item) and the chunk's traceback words, for ga_batch_sample, _count, _rank and _support alike;
    // ga_batch_sample a walk launch's items and the walks' own ticket word, and ga_batch_sample_info's and _timings's
    // figures of its last call
    DevBuf bs_words, bs_tb, bs_witems, bs_ticket;
    int64_t batch_sample_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float batch_sample_ms[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // ga_batch_count adds, behind that fill, the counts, the count launch's own ticket
    // word and the waves' HBM edge columns of doubles; ga_batch_count_info's and _timings's figures of its last call
    DevBuf bc_out, bc_ticket, bc_scratch;
    int64_t batch_count_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float batch_count_ms[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // ga_batch_rank adds, behind that fill, the chunk's count tables and the pairs'
    // places in them, the u64 counts, the call's ranks, a walk launch's items and the two launches' ticket word (the
    // edge columns go through bc_scratch, the walks' results and level words through bt_walk and bt_ops);
    // ga_batch_rank_info's and _timings's figures of its last call
    DevBuf br_table, br_toff, br_out, br_ranks, br_items, br_ticket;
    int64_t batch_rank_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float batch_rank_ms[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // ga_batch_support adds, behind that fill, the chunk's N tables, the pairs' places in
    // them and in the dense output, that output, the double counts and the table and flow launches' ticket words (the
    // edge columns go through bc_scratch); ga_batch_support_info's and _timings's figures of its last call
    DevBuf bm_table, bm_toff, bm_ooff, bm_out, bm_count, bm_ticket;
    int64_t batch_support_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float batch_support_ms[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int walk_jump_diag[3] = {0, 0, 0};  // the tie-to-tie walk's trips, region re-checks, ties (result[12..14])
    DevBuf jlut;           // the jump workers' LUT for gap open jlut_o (ga::jump_lut_build)
    int jlut_o = -1;
    // ga_slab_link: this slab's left edge + its progress word, uncached device memory on this GPU that
    // the left neighbour's fill writes (over xGMI when it runs on another GPU)
    DevBuf link;
    // ga_slab_link_import: the right neighbour's link buffer, mapped from another process
    void* peer_link = nullptr;
    char peer_handle[64] = {};
    unsigned rc_epoch = 0;
    bool rc_used = false;  // the last fill was the recompute path's (ga_problem_align or a slab's)
    // rc_align's walk levels in pinned host memory and the helper's progress word: decoded while the walk runs
    PinBuf rc_ops_pin{true}, rc_ops_prog{true};
    // rc_align's tie-break table: pinned staging, uploaded on a stream of its own while the fill runs, so that the walk
    // is queued behind the fill at once (a pageable copy on the fill's stream held the calling thread to the fill's end)
    PinBuf up_pin;
    hipStream_t ustream = nullptr;
    hipEvent_t ev_up = nullptr;
    gaplan::FillPlan rc_plan;  // the plan of the fill the recompute walk reads (rc_fill): stripes, spacing
    bool rc_jump = false;  // the last recompute walk was the tie-to-tie walk (jump entries)
    GuardCfg guard;        // guard mode (G = 0: off; guard_attach names and registers every buffer above)
};

namespace gahost {

// A band of rows of the whole problem (banded traceback): rows r0+1 .. r0+mb, its
// top row from a checkpoint (nullptr: row 0), no boundary pass; or the checkpointing pass itself; or the recompute
// walk's score fill; or a pipeline slot's fill (align_many): the planner's request (ga_plan.h; tb, full and
// has_ckpt are enqueue_fill's to set) and where the fill reads and writes.
struct Band : gaplan::Request {
    int64_t r0 = 0;
    const int2* top = nullptr;  // (H', h2') of row r0, [n+1] (column 0 = the left edge's corner)
    int2* ckpt = nullptr;       // checkpointing pass: where rows ckpt_rows, 2*ckpt_rows, ... go
    int ckpt_rows = 0;
    // pipelined alignments (align_many): a fill with buffers and a stream of its own, so that several fills can
    // run at once (nullptr: the context's)
    FillBufs* bufs = nullptr;
    hipStream_t stream = nullptr;
};

// Walk state between slab walks (the C ABI's ga_walk_state without the padding rules).
struct WalkStart {
    int64_t i, j, D, h;  // j: global column
    int L, first;
};

// Where a walk reads its words and table and leaves its levels / result, on which stream.
struct WalkBufs {
    const uint8_t* tb;
    uint32_t* rng;
    uint32_t* ops;
    int* result;
    hipStream_t stream;
    hipEvent_t ev0, ev1;
    const int* bnd_row = nullptr;  // the boundary triples (nullptr: the context's)
    const int* bnd_col = nullptr;
    unsigned* ops_prog = nullptr;  // WalkArgs::ops_prog (ops then in pinned host memory)
};

// ---- ga_host.cpp
int check_ctx(ga_ctx* c);
gaplan::Problem plan_problem(const ga_ctx* c);
int guard_end(ga_ctx* c, int rc);
std::vector<int> shifted_sub(const ga_costs* cs);
int load_problem(ga_ctx* c, const uint8_t* a, int64_t m, const uint8_t* b_all, int64_t n_all, const ga_costs* cs,
                 const int32_t* row0, const int32_t* col0, int64_t cb, int64_t ce);
int64_t dev_avail_bytes(ga_ctx* c, int64_t held);
size_t rc_cache_bytes(bool jump, int TD, int CB);
int enqueue_fill(ga_ctx* c, int32_t flags, const Band& bd = Band(), gaplan::FillPlan* plan_out = nullptr);
int finish_fill(ga_ctx* c, int64_t* cost_out, int32_t* full_out);
double now_ms();

// ---- ga_align_host.cpp
// the start state of a whole problem's walk: at (m, n), no dispatch made yet
inline WalkStart walk_origin(const ga_ctx* c) { return WalkStart{c->m, c->n, 0, 0, 0, 1}; }
int64_t band_rows(ga_ctx* c);  // gawalk::band_rows of the loaded problem on this device
WalkBufs ctx_walk_bufs(ga_ctx* c);
ga::WalkArgs walk_args(ga_ctx* c, int64_t ntab, const WalkStart& st, int64_t r0, int64_t mb, bool vhandoff,
                       const WalkBufs& wb);
int run_walk(ga_ctx* c, const uint32_t* tab, int64_t ntab, const WalkStart& st, int64_t r0 = 0, int64_t mb = -1,
             bool vhandoff = false, bool upload_tab = true, const WalkBufs* wbp = nullptr);
// A launched walk's result words and levels, waited for on its stream and decoded (decode_segment).
int walk_segment(ga_ctx* c, WalkStart& st, int& reason, const char* a_chr, const char* b_chr, char* oa, char* om,
                 char* ob, int64_t cap, int64_t& len, const WalkBufs* wbp = nullptr);
// The recompute walk: its score-only checkpointing fill of the loaded problem or slab, and the launch
// of the walk + recompute workgroups from walk state `st` on the walk buffers `wb` (its table already uploaded).
int rc_fill(ga_ctx* c);
int rc_walk_launch(ga_ctx* c, int64_t ntab, const WalkStart& st, WalkBufs& wb);
// ga_problem_traceback and ga_problem_align without guard mode's ending
int problem_traceback_impl(ga_ctx* c, uint32_t* mt_state, const char* a_chr, const char* b_chr, char* oa, char* om,
                           char* ob, int64_t cap, int64_t* out_len, int32_t* tb_status);
int problem_align_impl(ga_ctx* c, uint32_t* mt_state, const char* a_chr, const char* b_chr, char* oa, char* om,
                       char* ob, int64_t cap, int64_t* out_len, int32_t* tb_status, int64_t* cost_out);
// The alignment columns of a finished walk (its result words already read): levels of dispatches
// [st.D, res[0]) decoded in walk order starting at (st.i, st.j) (global columns); the end state through `st` and
// `reason`.  synced: the walk is known to be complete, so its levels are read with a plain copy instead of on its
// stream (which may already hold the next walk); host_ops: they are in pinned host memory already.
int decode_segment(ga_ctx* c, const int* res, WalkStart& st, int& reason, const char* a_chr, const char* b_chr,
                   char* oa, char* om, char* ob, int64_t cap, int64_t& len, const WalkBufs& wb, bool synced,
                   const uint32_t* host_ops = nullptr);
// The end of a traceback: the MT state after its dispatches, the reference's tails, reversal.
int conclude_walk(const RngTable& snaps, const WalkStart& st, int reason, uint32_t* mt_state, const char* a_chr,
                  const char* b_chr, char* oa, char* om, char* ob, int64_t cap, int64_t len, int64_t* out_len,
                  int32_t* tb_status);
// ga_problem_align_many without guard mode's ending (ga_pipe_host.cpp)
int problem_align_many(ga_ctx* c, int32_t count, uint32_t* mt_state, const char* a_chr, const char* b_chr, char* oa,
                       char* om, char* ob, int64_t cap, int64_t* out_len, int32_t* tb_status, int64_t* cost_out);

}  // namespace gahost
