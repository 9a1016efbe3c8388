// ga_opts.h -- a context's options (the GA_* knobs), as far as they are strings: which of the environment's variables
// the library reads, how the option string is split, the range checks of ga_ctx_create_opts with their error texts,
// and the typed knob sets that have no home of their own (the planner's are gaplan::Knobs in ga_plan.h, the traceback
// call's gawalk::Knobs in ga_walk_plan.h, the pipeline's gapipe::Knobs in ga_pipe.h).  No HIP, no context, no globals
// beyond the name list: built into the engine (ga_ctx_create_opts, ga_host.cpp, the one place that parses) and into
// ga_host_selftest.cpp under ASan / UBSan.  Numbers parse as atoi / atoll do (junk is 0); unknown names are kept and
// read by nobody.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <optional>
#include <string>

#include "../../include/globalign_amd.h"
#include "ga_batch_rng.h"
#include "ga_guard.h"

namespace gaopts {

using Map = std::map<std::string, std::string>;

// The GA_* variables the shipped library reads from the environment (INTEGRATION.md lists them): the path choices
// and budgets an operator may want to set.  Every other option -- kernel variants for tests and tuning, fault
// injection, diagnostics -- reaches a context only through ga_ctx_create_opts, never from the environment, so a
// stray variable cannot change a production context's kernels or inject a fault.  An experiments build
// (make EXPERIMENTS=1) takes every GA_* variable.
constexpr const char* kEnvKnobs[] = {"GA_RC",           "GA_RC_MIN_CELLS", "GA_RC_BUDGET_MB",      "GA_RC_EVERY",
                                     "GA_RC_SERVERS",   "GA_TB_BUDGET_MB", "GA_FILL_MODE",         "GA_COLS_PER_LANE",
                                     "GA_LANE_COLS_PER_LANE", "GA_PIPE_FILLS", "GA_PIPE_CHAIN",    "GA_STREAM_PRIORITY",
                                     "GA_HALO_SPIN_LIMIT", "GA_PIPE_TRACE"};
inline bool env_knob(const std::string& name, bool experiments) {
    if (experiments) return name.compare(0, 3, "GA_") == 0;
    for (const char* k : kEnvKnobs)
        if (name == k) return true;
    return false;
}

// The knob map of a new context: the entries of `envp` (an environ-style array; nullptr: none) that env_knob admits,
// then the options ("NAME=VALUE" entries separated by ';' or newlines; nullptr: none), which override them.
inline int collect(const char* const* envp, const char* options, bool experiments, Map& out, std::string& why) {
    for (const char* const* e = envp; e && *e; e++)
        if (!strncmp(*e, "GA_", 3))
            if (const char* eq = strchr(*e, '=')) {
                std::string name(*e, (size_t)(eq - *e));
                if (env_knob(name, experiments)) out[name] = eq + 1;
            }
    if (options) {
        std::string s(options), item;
        for (size_t p = 0; p <= s.size(); p++) {
            if (p < s.size() && s[p] != ';' && s[p] != '\n') {
                item += s[p];
                continue;
            }
            if (!item.empty()) {
                const size_t eq = item.find('=');
                if (eq == std::string::npos || item.compare(0, 3, "GA_") != 0) {
                    why = "bad option '" + item + "' (expected GA_NAME=VALUE)";
                    return GA_E_ARG;
                }
                out[item.substr(0, eq)] = item.substr(eq + 1);
            }
            item.clear();
        }
    }
    return GA_OK;
}

// Guard mode's options: options only, none is in kEnvKnobs.
struct GuardOpts {
    size_t bytes = 0;                        // GA_GUARD_BYTES (0: off)
    long fill = (long)gaguard::kDefaultFill;  // GA_GUARD_FILL
    bool poison = false;                     // GA_GUARD_POISON
};

// The range checks of a context's options, before any device work: GA_E_ARG and the reason for the first that fails.
inline int check(const Map& knobs, GuardOpts& out, std::string& why) {
    auto refuse = [&why](const std::string& msg) {
        why = msg;
        return GA_E_ARG;
    };
    {
        // GA_RC_EVERY: the checkpoint spacing is a power of two (a mask and a shift per iteration)
        const auto it = knobs.find("GA_RC_EVERY");
        if (it != knobs.end()) {
            const long v = atol(it->second.c_str());
            if (v < 64 || (v & (v - 1)) != 0 || v > (1L << 20))
                return refuse("GA_RC_EVERY must be a power of two in [64, 2^20], not '" + it->second + "'");
        }
    }
    {
        // the tables' route: a name, an item limit the generator's int32 counters hold, a word cap
        auto it = knobs.find("GA_BATCH_RNG");
        if (it != knobs.end() && it->second != "host" && it->second != "device")
            return refuse("GA_BATCH_RNG must be host or device, not '" + it->second + "'");
        it = knobs.find("GA_BATCH_RNG_DEVICE_MAX_STEPS");
        if (it != knobs.end() && (atoll(it->second.c_str()) < 0 || atoll(it->second.c_str()) > (1 << 20)))
            return refuse("GA_BATCH_RNG_DEVICE_MAX_STEPS must be in [0, 2^20], not '" + it->second + "'");
        it = knobs.find("GA_BATCH_RNG_WORD_CAP");
        if (it != knobs.end() && (atoll(it->second.c_str()) < 1 || atoll(it->second.c_str()) > 1024))
            return refuse("GA_BATCH_RNG_WORD_CAP must be in [1, 1024], not '" + it->second + "'");
    }
    out = GuardOpts();
    auto whole = [](const std::string& v, long long& num) {
        char* end = nullptr;
        num = strtoll(v.c_str(), &end, 0);
        return !v.empty() && end && *end == 0;
    };
    long long v = 0;
    auto it = knobs.find("GA_GUARD_BYTES");
    if (it != knobs.end()) {
        if (!whole(it->second, v) || !gaguard::valid_guard_bytes(v))
            return refuse("GA_GUARD_BYTES must be 0 or a multiple of 256 up to 2^20, not '" + it->second + "'");
        out.bytes = (size_t)v;
    }
    it = knobs.find("GA_GUARD_FILL");
    if (it != knobs.end()) {
        if (!whole(it->second, v) || !gaguard::valid_fill(v))
            return refuse("GA_GUARD_FILL must be a byte value in [0, 255], not '" + it->second + "'");
        out.fill = (long)v;
    }
    it = knobs.find("GA_GUARD_POISON");
    if (it != knobs.end()) {
        if (it->second != "0" && it->second != "1")
            return refuse("GA_GUARD_POISON must be 0 or 1, not '" + it->second + "'");
        out.poison = it->second == "1";
        if (out.poison && !out.bytes) return refuse("GA_GUARD_POISON=1 needs GA_GUARD_BYTES");
    }
    return GA_OK;
}

// The typed knob sets below are parsed as gawalk::Knobs is: `get` looks a shipped knob up, `xget` one of a path that
// was measured and dropped (the shipped build's sees nothing); nullptr for an unset name.

// What a lane fill's buffers and launch read (fill_buffers, fill_launch_knobs in ga_host.cpp): tuning, A/B runs and
// tests, none changes the plan.
struct LaneKnobs {
    std::optional<int> late;     // GA_LANE_LATE (unset: the fill decides, 1 for one round of workgroups)
    int xcd = 0;                 // (experiments) GA_LANE_XCD
    int hand_direct = 0;         // GA_LANE_DIRECT
    int lds_floor = -1;          // GA_FILL_LDS_FLOOR
    int lane_sub = -1;           // GA_LANE_SUB
    int lane_tb_sub = -1;        // GA_LANE_TB_SUB
    int asm_step = 1;            // GA_LANE_ASM
    int io_prio = 0;             // (experiments) GA_LANE_IOPRIO
    int hand_scope = 0;          // (experiments) GA_LANE_HANDSCOPE
    int poll_win = 0;            // GA_LANE_POLLWIN, 0..192
    int out_wave = 1;            // GA_LANE_OUTWAVE
    std::optional<unsigned> halo_spin_limit;  // GA_HALO_SPIN_LIMIT, >= 1 (tests)
    int lean0 = 1;               // GA_LANE_LEAN0 (0 keeps the masked ramp, A/B)
    bool rc_fail_alloc = false;  // GA_RC_FAIL_ALLOC=1 (tests): the second checkpoint allocation fails
    bool qprof_wave = false;     // (experiments) GA_LANE_QPROF_WAVE is set: the profile wave builds the query profile
    template <typename Get, typename XGet>
    static LaneKnobs parse(Get&& get, XGet&& xget) {
        LaneKnobs kn;
        if (const char* e = get("GA_LANE_LATE")) kn.late = atoi(e);
        if (const char* e = xget("GA_LANE_XCD")) kn.xcd = atoi(e);
        if (const char* e = get("GA_LANE_DIRECT")) kn.hand_direct = atoi(e);
        if (const char* e = get("GA_FILL_LDS_FLOOR")) kn.lds_floor = atoi(e);
        if (const char* e = get("GA_LANE_SUB")) kn.lane_sub = atoi(e);
        if (const char* e = get("GA_LANE_TB_SUB")) kn.lane_tb_sub = atoi(e);
        if (const char* e = get("GA_LANE_ASM")) kn.asm_step = atoi(e);
        if (const char* e = xget("GA_LANE_IOPRIO")) kn.io_prio = atoi(e);
        if (const char* e = xget("GA_LANE_HANDSCOPE")) kn.hand_scope = atoi(e);
        if (const char* e = get("GA_LANE_POLLWIN")) kn.poll_win = std::min(std::max(atoi(e), 0), 192);
        if (const char* e = get("GA_LANE_OUTWAVE")) kn.out_wave = atoi(e);
        if (const char* e = get("GA_HALO_SPIN_LIMIT")) kn.halo_spin_limit = (unsigned)std::max(1L, atol(e));
        if (const char* e = get("GA_LANE_LEAN0")) kn.lean0 = atoi(e);
        if (const char* e = get("GA_RC_FAIL_ALLOC")) kn.rc_fail_alloc = atoi(e) == 1;
        kn.qprof_wave = xget("GA_LANE_QPROF_WAVE") != nullptr;
        return kn;
    }
};

// The batched calls' (ga_batch_host.cpp): the tables' route (its three knobs are checked by check()),
// the host threads, the planners' routing limits (unset: gabatch's own defaults).
struct BatchKnobs {
    bool rng_device_default = false;                   // GA_BATCH_RNG=device
    int64_t rng_max_steps = gabrng::kDeviceMaxSteps;   // GA_BATCH_RNG_DEVICE_MAX_STEPS
    int rng_cap_words = gabrng::kCapWordsPerDispatch;  // GA_BATCH_RNG_WORD_CAP
    int rng_threads = 0;                               // GA_BATCH_RNG_THREADS (0: gabatch::rng_threads chooses)
    std::optional<int64_t> max_cells;                  // GA_BATCH_MAX_CELLS, >= 0
    std::optional<int64_t> align_max_cells;            // GA_BATCH_ALIGN_MAX_CELLS, >= 0
    std::optional<int64_t> sample_chunk_words;         // GA_BATCH_SAMPLE_CHUNK_WORDS, >= 1
    std::optional<int64_t> sample_walk_entries;        // GA_BATCH_SAMPLE_WALK_ENTRIES, >= 1
    std::optional<int64_t> rank_table_bytes;           // GA_BATCH_RANK_TABLE_BYTES, >= 1
    std::optional<int64_t> support_bytes;              // GA_BATCH_SUPPORT_BYTES, >= 1
    template <typename Get, typename XGet>
    static BatchKnobs parse(Get&& get, XGet&&) {
        BatchKnobs kn;
        if (const char* e = get("GA_BATCH_RNG")) kn.rng_device_default = !strcmp(e, "device");
        if (const char* e = get("GA_BATCH_RNG_DEVICE_MAX_STEPS")) kn.rng_max_steps = atoll(e);
        if (const char* e = get("GA_BATCH_RNG_WORD_CAP")) kn.rng_cap_words = atoi(e);
        if (const char* e = get("GA_BATCH_RNG_THREADS")) kn.rng_threads = atoi(e);
        if (const char* e = get("GA_BATCH_MAX_CELLS")) kn.max_cells = std::max<int64_t>(0, atoll(e));
        if (const char* e = get("GA_BATCH_ALIGN_MAX_CELLS")) kn.align_max_cells = std::max<int64_t>(0, atoll(e));
        if (const char* e = get("GA_BATCH_SAMPLE_CHUNK_WORDS")) kn.sample_chunk_words = std::max<int64_t>(1, atoll(e));
        if (const char* e = get("GA_BATCH_SAMPLE_WALK_ENTRIES")) kn.sample_walk_entries = std::max<int64_t>(1, atoll(e));
        if (const char* e = get("GA_BATCH_RANK_TABLE_BYTES")) kn.rank_table_bytes = std::max<int64_t>(1, atoll(e));
        if (const char* e = get("GA_BATCH_SUPPORT_BYTES")) kn.support_bytes = std::max<int64_t>(1, atoll(e));
        return kn;
    }
};

// GA_STREAM_PRIORITY=normal: the context's stream at the default priority instead of the greatest (experiments)
template <typename Get>
bool stream_priority_normal(Get&& get) {
    const char* e = get("GA_STREAM_PRIORITY");
    return e && !strcmp(e, "normal");
}

}  // namespace gaopts
