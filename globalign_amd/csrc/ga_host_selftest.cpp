// ga_host_selftest.cpp -- CPU self-test of the engine's host-only pieces, built with AddressSanitizer and
// UndefinedBehaviorSanitizer (make -C globalign_amd/csrc asan; run by tests/test_host_asan.py):
//   * the tie-break table (ga_rng.h): RngTable's four-word scan, its resumable extend() and state_after(), against a draw-by-draw restatement of CPython's random.choice (_randbelow_with_getrandbits over
//     genrand_uint32) and the dispatcher's level rule (globaligner.py:595-685);
//   * the problem checks (ga_check.h): argument validation, the int32 range guard, the profile / word widths, and the
//     limit tables of tests/limit_costs.py at the last factor the guard accepts and the first it refuses;
//   * the fill planner (ga_plan.h): the kernel, geometry and checkpoint spacing of the shapes the project's records
//     pin (profiles/r06, DESIGN.md 5.2 / 5.6 / 5.8.1, tests/test_gpu_rc_default_width.py), and every error return;
//   * the traceback call's pure part (ga_walk_plan.h): its knobs' defaults and clamps, the recompute walk's eligibility,
//     the banded traceback's rows, the recompute window's invariants and its default tables, workers per workgroup;
//   * the guard bands' layout, scan and report (ga_guard.h) on a host model of a guarded buffer;
//   * a context's options (ga_opts.h): which of the environment's variables land in the knob map, the option string's
//     split, every range check with its text, and the typed knob sets' defaults and clamps (gaopts::LaneKnobs,
//     gaopts::BatchKnobs, gaplan::Knobs::parse).
// No HIP: the engine's library is tested on the GPU; this binary covers the host logic under the sanitizers.
//
//   ga_host_selftest            all checks; exit status 0 when every one passes
//   ga_host_selftest bench S    time the table for S dispatches
//   ga_host_selftest envknobs   the GA_* names the shipped library reads from the environment, one per line
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "ga_batch.h"
#include "ga_check.h"
#include "ga_guard.h"
#include "ga_opts.h"
#include "ga_plan.h"
#include "ga_rng.h"
#include "ga_walk_plan.h"

using namespace garng;

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

uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// a random 625-word state (624 words + index), as random.getstate()[1] could hold
std::vector<uint32_t> random_state(uint64_t seed) {
    std::vector<uint32_t> st(MTN + 1);
    uint64_t s = seed;
    for (int k = 0; k < MTN; k++) st[k] = (uint32_t)splitmix(s);
    st[0] |= 0x80000000u;  // never the all-zero array
    st[MTN] = (uint32_t)(splitmix(s) % (MTN + 1));
    return st;
}

// the dispatcher's level per rank set S = 1..7 from one step's 18 draws (ga_rng.h fill_entries' rule, written out
// from the dict literal, :599-671): S = 7 {0,1,2} -> draw 0; 3 {0,1} -> (0,1)[draw 1]; 5 {0,2} -> (0,2)[draw 2];
// 6 {1,2} -> (1,2)[draw 3]; singletons fixed; the mismatch half uses draws 9..12
uint32_t naive_entry(const unsigned* r) {
    uint32_t e = 0;
    for (int half = 0; half < 2; half++) {
        const unsigned* q = r + 9 * half;
        const unsigned lv[8] = {0, 0, 1, q[1] ? 1u : 0u, 2, q[2] ? 2u : 0u, q[3] ? 2u : 1u, q[0]};
        for (int S = 1; S <= 7; S++) e |= lv[S] << (2 * S + 1 + 14 * half);
    }
    return e;
}

struct Naive {
    std::vector<uint32_t> tab;
    std::map<int64_t, std::vector<uint32_t>> states;  // state after d dispatches (only where asked)
};

Naive naive_table(const std::vector<uint32_t>& st, int64_t steps, const std::vector<int64_t>& want_states) {
    static const unsigned sz[18] = {3, 2, 2, 2, 3, 2, 2, 2, 3, 3, 2, 2, 2, 3, 2, 2, 2, 3};
    PyMT g;
    std::memcpy(g.mt, st.data(), sizeof(uint32_t) * MTN);
    g.mti = (int)st[MTN];
    Naive out;
    out.tab.resize(steps);
    auto snap = [&](int64_t d) {
        for (int64_t w : want_states)
            if (w == d) {
                std::vector<uint32_t> s(MTN + 1);
                std::memcpy(s.data(), g.mt, sizeof(uint32_t) * MTN);
                s[MTN] = (uint32_t)g.mti;
                out.states[d] = s;
            }
    };
    snap(0);
    for (int64_t d = 0; d < steps; d++) {
        unsigned r[18];
        for (int k = 0; k < 18; k++) r[k] = g.below(sz[k]);
        out.tab[d] = naive_entry(r);
        snap(d + 1);
    }
    return out;
}

bool same_state(const uint32_t* a, const std::vector<uint32_t>& b) {
    // equal as CPython states: the same 624 words and index (a twisted-at-624 array equals its untwisted form only
    // through the index, so compare the next words instead when the indices differ)
    if (std::memcmp(a, b.data(), sizeof(uint32_t) * (MTN + 1)) == 0) return true;
    PyMT x, y;
    std::memcpy(x.mt, a, sizeof(uint32_t) * MTN);
    x.mti = (int)a[MTN];
    std::memcpy(y.mt, b.data(), sizeof(uint32_t) * MTN);
    y.mti = (int)b[MTN];
    for (int k = 0; k < 2 * MTN; k++)
        if (x.next() != y.next()) return false;
    return true;
}

void test_table(uint64_t seed, int64_t steps) {
    const auto st = random_state(seed);
    std::vector<int64_t> Ds = {0, 1, steps / 3, steps / 2, steps};
    for (auto& D : Ds) D = std::min(D, steps);
    const Naive nv = naive_table(st, steps, Ds);
    // sequential build
    RngTable R;
    build_rng(st.data(), steps, R);
    CHECK((int64_t)R.tab.size() == steps, "seed %llu: %zu entries for %lld steps", (unsigned long long)seed, R.tab.size(),
          (long long)steps);
    for (int64_t d = 0; d < steps && d < (int64_t)R.tab.size(); d++)
        if (R.tab[d] != nv.tab[d]) {
            CHECK(false, "seed %llu steps %lld: entry %lld %08x != %08x", (unsigned long long)seed, (long long)steps,
                  (long long)d, R.tab[d], nv.tab[d]);
            break;
        }
    for (size_t k = 0; k < Ds.size(); k++) {
        uint32_t out[MTN + 1];
        state_after(R, Ds[k], out);
        CHECK(same_state(out, nv.states.at(Ds[k])), "seed %llu: state after %lld dispatches", (unsigned long long)seed,
              (long long)Ds[k]);
    }
    // resumable: extend() in uneven chunks
    RngTable Q;
    Q.start(st.data());
    for (int64_t b = 7; b < steps + 7; b = b * 2 + 3) Q.extend(std::min(b, steps));
    Q.extend(steps);
    CHECK(Q.tab == R.tab, "seed %llu: chunked extend differs", (unsigned long long)seed);
}

void test_checks() {
    const int K = 5;
    int32_t sub[K * K], gh[K], gv[K];
    for (int x = 0; x < K; x++) {
        gh[x] = 2;
        gv[x] = 2;
        for (int y = 0; y < K; y++) sub[x * K + y] = x == y ? 0 : 5;
    }
    ga_costs cs{K, sub, gh, gv, 5, 5};
    std::vector<uint8_t> a(1000), b(800);
    uint64_t s = 99;
    for (auto& x : a) x = (uint8_t)(splitmix(s) % 4);
    for (auto& x : b) x = (uint8_t)(splitmix(s) % 4);
    ProblemShape ps;
    std::string err;
    CHECK(check_problem(a.data(), 1000, b.data(), 800, &cs, nullptr, nullptr, 0, 800, ps, err) == GA_OK, "valid: %s",
          err.c_str());
    CHECK(ps.big == 6 * 1000 && ps.CB == 1 && ps.qbytes == 1, "shape big %lld CB %d qbytes %d", (long long)ps.big, ps.CB,
          ps.qbytes);
    CHECK(check_problem(nullptr, 1000, b.data(), 800, &cs, nullptr, nullptr, 0, 800, ps, err) == GA_E_ARG, "null a");
    CHECK(check_problem(a.data(), 0, b.data(), 800, &cs, nullptr, nullptr, 0, 800, ps, err) == GA_E_ARG, "empty");
    CHECK(check_problem(a.data(), 1000, b.data(), 800, &cs, nullptr, nullptr, 10, 5, ps, err) == GA_E_ARG, "slab");
    a[17] = K;
    CHECK(check_problem(a.data(), 1000, b.data(), 800, &cs, nullptr, nullptr, 0, 800, ps, err) == GA_E_ARG, "code");
    a[17] = 0;
    ga_costs neg = cs;
    neg.gap_open = -1;
    CHECK(check_problem(a.data(), 1000, b.data(), 800, &neg, nullptr, nullptr, 0, 800, ps, err) == GA_E_ARG, "open < 0");
    ga_costs wide = cs;
    wide.gap_open = 200;  // o + 1 >= 128: 4-byte traceback words
    CHECK(check_problem(a.data(), 1000, b.data(), 800, &wide, nullptr, nullptr, 0, 800, ps, err) == GA_OK && ps.CB == 4,
          "open 200: CB %d", ps.CB);
    ga_costs huge = cs;
    huge.gap_open = 40000;
    CHECK(check_problem(a.data(), 1000, b.data(), 800, &huge, nullptr, nullptr, 0, 800, ps, err) == GA_E_RANGE,
          "open 40000 must not fit a traceback word");
    int32_t sub2[K * K];
    std::memcpy(sub2, sub, sizeof(sub));
    sub2[3] = 1 << 20;
    ga_costs big = cs;
    big.sub = sub2;
    big.max_cost = 1 << 20;
    CHECK(check_problem(a.data(), 1000, b.data(), 800, &big, nullptr, nullptr, 0, 800, ps, err) == GA_E_RANGE,
          "int32 range guard");
    // custom boundaries: both or neither
    std::vector<int32_t> row0(3 * 801, 0), col0(3 * 1001, 0);
    CHECK(check_problem(a.data(), 1000, b.data(), 800, &cs, row0.data(), nullptr, 0, 800, ps, err) == GA_E_ARG,
          "row0 without col0");
    CHECK(check_problem(a.data(), 1000, b.data(), 800, &cs, row0.data(), col0.data(), 0, 800, ps, err) == GA_OK,
          "custom boundaries: %s", err.c_str());
    row0[5] = 1 << 29;
    CHECK(check_problem(a.data(), 1000, b.data(), 800, &cs, row0.data(), col0.data(), 0, 800, ps, err) == GA_E_RANGE,
          "boundary values in the range guard");
    // the lean checkpoint store's 32-bit buffer: recompute checkpoints refused past it
    CHECK(rc_rows_fit(100000) && !rc_rows_fit((int64_t)1 << 28), "rc_rows_fit");
}

// A K = 5 table over A C G T and '-' as CostTables lays a costing dict out: sub[x][4] = gap_v[x], sub[4][y] = gap_h[y].
struct Table5 {
    int32_t sub[25] = {}, gh[5] = {}, gv[5] = {};
    ga_costs cs{5, sub, gh, gv, 0, 0};
    Table5() = default;
    Table5(const Table5&) = delete;
    // sub' = d under the gap costs gh4 / gv4
    void set(const int64_t (&d)[4][4], const int64_t (&gh4)[4], const int64_t (&gv4)[4], int o) {
        int64_t mx = 0;
        for (int x = 0; x < 4; x++) {
            gh[x] = (int32_t)gh4[x];
            gv[x] = (int32_t)gv4[x];
            sub[x * 5 + 4] = gv[x];
            sub[4 * 5 + x] = gh[x];
            mx = std::max<int64_t>(mx, std::max(gh4[x], gv4[x]));
            for (int y = 0; y < 4; y++) {
                sub[x * 5 + y] = (int32_t)(d[x][y] + gv4[x] + gh4[y]);
                mx = std::max<int64_t>(mx, sub[x * 5 + y]);
            }
        }
        cs.gap_open = o;
        cs.max_cost = (int32_t)mx;
    }
};

// The limit families of tests/limit_costs.py at the factors its restated guard gives (tests/test_limit_costs_cpu.py
// pins the same figures): check_problem accepts the factor and refuses factor + 1; the profile and word widths switch
// where the restatement says they do.
void test_limit_tables() {
    std::vector<uint8_t> a(4096, 0), b(4096, 1);
    ProblemShape ps;
    std::string err;
    auto check = [&](Table5& t, int64_t m, int64_t n) {
        return check_problem(a.data(), m, b.data(), n, &t.cs, nullptr, nullptr, 0, n, ps, err);
    };
    // V16: match 0 / mismatch 5 / gaps 2-3, times f
    auto v16 = [](Table5& t, int64_t f, int o) {
        const int64_t gv[4] = {2 * f, 3 * f, 2 * f, 3 * f}, gh[4] = {3 * f, 2 * f, 3 * f, 2 * f};
        int64_t d[4][4];
        for (int x = 0; x < 4; x++)
            for (int y = 0; y < 4; y++) d[x][y] = (x == y ? 0 : 5 * f) - gv[x] - gh[y];
        t.set(d, gh, gv, o);
    };
    // Vphi: gap costs G + small offsets, sub' fixed within int8
    auto vphi = [](Table5& t, int64_t G, int o) {
        const int64_t d[4][4] = {{-127, 127, 12, 6}, {12, -127, 5, 12}, {6, 12, -127, -3}, {127, 0, 12, -127}};
        const int64_t gv[4] = {G + 1, G + 4, G + 6, G + 9}, gh[4] = {G + 2, G + 3, G + 7, G + 8};
        t.set(d, gh, gv, o);
    };
    struct Lim { const char* what; bool phi; int sign; int64_t m, n; int o; int64_t f; int qbytes; const char* why; };
    const Lim lims[] = {
        {"V16 1100 x 600", false, 1, 1100, 600, 32766, 6553, 2, "substitution costs exceed the int16 query profile"},
        {"V16 4096 x 1024", false, 1, 4096, 1024, 5, 5516, 2, "problem exceeds the int32 score range of the device path"},
        {"Vphi 777 x 2049", true, 1, 777, 2049, 7, 25415, 1, "problem exceeds the int32 score range of the device path"},
        {"V- 2049 x 700", true, -1, 2049, 700, 5, 32462, 1, "problem exceeds the int32 score range of the device path"},
    };
    for (const Lim& L : lims)
        for (int excess = 0; excess < 2; excess++) {
            Table5 t;
            if (L.phi) vphi(t, L.sign * (L.f + excess), L.o);
            else v16(t, L.f + excess, L.o);
            const int r = check(t, L.m, L.n);
            if (!excess)
                CHECK(r == GA_OK && ps.qbytes == L.qbytes, "%s at factor %lld: %d (%s), qbytes %d", L.what, (long long)L.f, r,
                      err.c_str(), ps.qbytes);
            else
                CHECK(r == GA_E_RANGE && err == L.why, "%s at factor %lld: %d (%s)", L.what, (long long)L.f + 1, r, err.c_str());
        }
    {
        // V32: the batch planner's range check of a pair (4-byte table entries, no profile limit)
        for (int excess = 0; excess < 2; excess++) {
            Table5 t;
            v16(t, 221364 + excess, 32766);
            int64_t big = 0;
            const int r = gabatch::check_pair_range(65, 70, &t.cs, t.cs.max_cost, costs_maxabs(&t.cs), big);
            CHECK(r == (excess ? GA_E_RANGE : GA_OK) && profile_bytes(&t.cs) == 0, "V32 65 x 70 at factor %d: %d", 221364 + excess, r);
        }
    }
    {
        // the profile width by the largest |sub'|, on either sign: int8 to 127, int16 to 32767, refused beyond
        const int64_t gv[4] = {20, 25, 31, 40}, gh[4] = {23, 28, 35, 43};
        struct W { int64_t v; int qbytes; };
        for (const W& w : {W{127, 1}, W{128, 2}, W{32767, 2}, W{32768, 0}})
            for (int sign : {1, -1}) {
                int64_t d[4][4] = {};
                d[2][3] = sign * w.v;
                Table5 t;
                t.set(d, gh, gv, 6);
                CHECK(profile_bytes(&t.cs) == w.qbytes, "profile_bytes at sub' = %lld", (long long)(sign * w.v));
                const int r = check(t, 70, 130);
                if (w.qbytes)
                    CHECK(r == GA_OK && ps.qbytes == w.qbytes, "sub' = %lld: %d (%s)", (long long)(sign * w.v), r, err.c_str());
                else
                    CHECK(r == GA_E_RANGE && err == "substitution costs exceed the int16 query profile", "sub' = %lld: %d (%s)",
                          (long long)(sign * w.v), r, err.c_str());
            }
    }
    // the traceback word by o + 1: its fields hold values up to o + 1
    CHECK(tb_word_bytes(6) == 1 && tb_word_bytes(7) == 2 && tb_word_bytes(126) == 2 && tb_word_bytes(127) == 4 &&
              tb_word_bytes(32766) == 4 && tb_word_bytes(32767) == 0,
          "tb_word_bytes at the field widths");
    {
        Table5 t;
        v16(t, 1, 32766);
        CHECK(check(t, 70, 130) == GA_OK && ps.CB == 4, "o = 32766: %s", err.c_str());
        t.cs.gap_open = 32767;
        CHECK(check(t, 70, 130) == GA_E_RANGE && err == "gap_open cost too large for the traceback word", "o = 32767: %s", err.c_str());
        // caller-supplied boundary values: the largest B the guard admits at 130 x 321, and B + 1
        t.cs.gap_open = 6;
        const int64_t m = 130, n = 321, B = ((int64_t)INT32_MAX - 1) / 4 - (m + n + 2) * (3 * costs_maxabs(&t.cs) + 6);
        for (int sign : {1, -1})
            for (int excess = 0; excess < 2; excess++) {
                std::vector<int32_t> row0(3 * (n + 1), 0), col0(3 * (m + 1), 0);
                col0[3 * m + 1] = (int32_t)(sign * (B + excess));
                const int r = check_problem(a.data(), m, b.data(), n, &t.cs, row0.data(), col0.data(), 0, n, ps, err);
                CHECK(r == (excess ? GA_E_RANGE : GA_OK), "boundary value %lld: %d", (long long)(sign * (B + excess)), r);
            }
    }
}

// ---------------------------------------------------------------- the fill planner (ga_plan.h)
// The recompute walk's word cache as ga_host.cpp rc_cache_bytes sizes it: RC_CACHE_I x RC_CACHE_S = 64 x 32 blocks
// (ga_device.h) of TD 64 x 64 tiles of CB bytes, + one stripe of slack (the tie-to-tie walk's is not planned here)
size_t word_cache_bytes(bool, int TD, int CB) { return (size_t)64 * 32 * TD * 64 * 64 * CB + (size_t)64 * 64 * 4 * 4; }
const gaplan::LdsSizes kLds{gaplan::restated_fill_lane_lds_bytes, gaplan::restated_rc_worker_bytes, word_cache_bytes};

// an m x n problem on 256 CUs: DNA (K = 4) unless K says otherwise, one-byte words and profile
gaplan::Problem shape(int64_t m, int64_t n, int K = 4) {
    gaplan::Problem pb;
    pb.m = m;
    pb.n = pb.n_global = n;
    pb.K = K;
    pb.o = 5;
    return pb;  // CB 1, qbytes 1, 256 CUs, 1024 profile rows (load_problem's for K <= 64): the defaults
}

gaplan::Request rc_request() {
    gaplan::Request rq;
    rq.rc = true;
    return rq;
}

void expect_plan(const char* what, const gaplan::FillPlan& pl, int kind, int T, int nstripes = -1, int nwc = -1,
                 int nslabs = -1, int every = -1) {
    CHECK(pl.err == GA_OK, "%s: error %d (%s)", what, pl.err, pl.msg ? pl.msg : "");
    CHECK(pl.kind == kind && pl.T == T && (nstripes < 0 || pl.nstripes == nstripes) && (nwc < 0 || pl.nwc == nwc) &&
              (nslabs < 0 || pl.nslabs == nslabs) && (every < 0 || pl.rc_every == every),
          "%s: kind %d T %d stripes %d waves %d workgroups %d every %d, expected %d %d %d %d %d %d", what, pl.kind, pl.T,
          pl.nstripes, pl.nwc, pl.nslabs, pl.rc_every, kind, T, nstripes, nwc, nslabs, every);
}

void expect_error(const char* what, const gaplan::FillPlan& pl, int code, const char* msg) {
    CHECK(pl.err == code && pl.msg && std::strcmp(pl.msg, msg) == 0, "%s: error %d (%s), expected %d (%s)", what, pl.err,
          pl.msg ? pl.msg : "", code, msg);
}

void test_plan() {
    using namespace gaplan;
    const Knobs unset;
    Knobs wide = unset;  // GA_RC_NARROW=0
    wide.rc_narrow = false;
    const Request score, rc = rc_request();
    Request tb;
    tb.tb = true;
    const int64_t c2 = 10000, c3 = 100000, c5 = 20000, c4 = 1000000;
    const int kProtein = 25;  // BLOSUM62's letters and '-' (scoring.load_named_matrix: CostTables' K)
    // the recompute fill of the benchmark's workloads (profiles/r06/check5_bench_*.json, fill_kind)
    expect_plan("C3 rc", plan_fill(shape(c3, c3), rc, unset, kLds), kLane, 2, 782, 4, 196);
    expect_plan("C3 rc, GA_RC_NARROW=0", plan_fill(shape(c3, c3), rc, wide, kLds), kLane, 4, 391, 4, 98);
    expect_plan("C2 rc", plan_fill(shape(c2, c2), rc, unset, kLds), kLane, 2, 79, 4, 20);
    expect_plan("C2 rc, GA_RC_NARROW=0", plan_fill(shape(c2, c2), rc, wide, kLds), kLane, 4, 40, 4, 10);
    expect_plan("C5 rc", plan_fill(shape(c5, c5, kProtein), rc, unset, kLds), kLane, 4, 79, 4, 20);
    // score only: C4 in two rounds of 4-wave workgroups; the tall fills' widths
    expect_plan("C4 score", plan_fill(shape(c4, c4), score, unset, kLds), kLane, 8, 1954, 4, 489);
    expect_plan("1M x 125k score", plan_fill(shape(c4, 125000), score, unset, kLds), kLane, 2);
    expect_plan("1M x 250k score", plan_fill(shape(c4, 250000), score, unset, kLds), kLane, 4);
    expect_plan("1M x 500k score", plan_fill(shape(c4, 500000), score, unset, kLds), kLane, 8);
    // stored words: the row scan, 64-column stripes, two waves per SIMD
    expect_plan("C3 stored words", plan_fill(shape(c3, c3), tb, unset, kLds), kRow, 1, 1563, 8, 196);
    {
        // C4 with traceback on one GPU: 4 columns per lane, and the spacing whose checkpoints fit 96 GB (128 steps,
        // 78 GB; 64 would take 156 GB)
        Knobs kn = unset;
        kn.dev_avail = (int64_t)286 << 30;
        expect_plan("C4 rc", plan_fill(shape(c4, c4), rc, kn, kLds), kLane, 4, -1, -1, -1, 128);
    }
    {
        // the pipeline's narrow traceback fills at C3
        Request pipe = tb;
        pipe.lane_td = 4;
        pipe.lane_nwc = 4;
        const FillPlan pl = plan_fill(shape(c3, c3), pipe, unset, kLds);
        expect_plan("C3 pipeline fill", pl, kLane, 4, 391, 4, 98);
        CHECK(pl.qrows <= 2048, "C3 pipeline fill: %d profile rows", pl.qrows);
    }
    {
        // the guard tests' edge sweep (tests/test_gpu_guard.py): every shape of the recompute walk's cross plans the
        // lane kernel at the width asked for, and so does every shape of the lane fills' sweep, score only at 1 to 8
        // columns per lane and with traceback words at 1 to 4 -- none is declined
        for (int td : {1, 2, 4, 8}) {
            Knobs kn = unset;
            kn.lane_T_req = td;
            const int64_t w = 64 * td, k = (256 + 1 + w - 1) / w;
            for (int64_t r : {1, 17, 48, 63, 64, 65, 130})
                for (int64_t n : {(int64_t)256, k * w - 1, k * w, k * w + 1, (k + 2) * w + 17}) {
                    const FillPlan pl = plan_fill(shape(256 + r, n, 5), rc, kn, kLds);
                    CHECK(pl.err == GA_OK && pl.kind == kLane && pl.T == td && pl.nstripes == (n + w - 1) / w,
                          "guard sweep rc %lld x %lld at %d columns per lane: error %d kind %d T %d", (long long)(256 + r),
                          (long long)n, td, pl.err, pl.kind, pl.T);
                }
            kn.diag_req = 3;  // GA_FILL_MODE=lane
            kn.nwc_req = 4;
            for (int64_t m : {1, 17, 48, 63, 64, 65, 130})
                for (int64_t n : {(int64_t)1, w - 1, w, w + 1, 3 * w + 17})
                    for (const Request& rq : {score, tb}) {
                        if (rq.tb && td == 8) continue;  // no traceback-word variant at 8 columns per lane
                        const FillPlan pl = plan_fill(shape(m, n, 5), rq, kn, kLds);
                        CHECK(pl.err == GA_OK && pl.kind == kLane && pl.T == td && pl.nwc == 4,
                              "guard sweep lane %lld x %lld at %d columns per lane, tb %d: error %d kind %d T %d",
                              (long long)m, (long long)n, td, (int)rq.tb, pl.err, pl.kind, pl.T);
                    }
        }
    }
    // the recompute fill's width rules at tests/test_gpu_rc_default_width.py's shapes
    expect_plan("DNA default", plan_fill(shape(2500, 2600), rc, unset, kLds), kLane, 2);
    expect_plan("DNA, GA_RC_NARROW=0", plan_fill(shape(2500, 2600), rc, wide, kLds), kLane, 4);
    expect_plan("protein", plan_fill(shape(1200, 1400, kProtein), rc, unset, kLds), kLane, 4);
    expect_plan("more stripes than SIMDs", plan_fill(shape(256, 131300), rc, unset, kLds), kLane, 4);
    {
        Knobs kn = unset;  // GA_LANE_COLS_PER_LANE=4, GA_RC_NARROW=1
        kn.lane_T_req = 4;
        expect_plan("GA_LANE_COLS_PER_LANE=4", plan_fill(shape(2500, 2600), rc, kn, kLds), kLane, 4);
    }
    {
        // a slab with a right neighbour ends on a whole stripe: 1,000,192 columns are 3907 x 256, so
        // the 8 columns per lane a fill this wide would take fall to 4; too many stripes for the lane kernel, which
        // keeps every stripe of such a slab resident
        Problem pb = shape(c4, 1000192);
        pb.slab = true;
        pb.n_global = 2 * pb.n;
        expect_plan("slab with a right neighbour", plan_fill(pb, score, unset, kLds), kRow, 4, 3907);
        // the last slab hands nothing on and keeps 8 (its 1954 stripes are still more than the 8 x 224 that stay
        // resident beside the kernel that brings its left edge)
        pb.col0 = pb.n;
        expect_plan("last slab", plan_fill(pb, score, unset, kLds), kRow, 8, 1954);
        // the context's plan before any fill: the row scan's (ga_slab_buffers' default halo_out address)
        pb.col0 = 0;
        expect_plan("slab, loaded", row_plan(pb, unset), kRow, 4, 3907, 8, 489);
    }
    // every error return
    expect_error("K > 32", plan_fill(shape(c2, c2, 33), rc, unset, kLds), GA_E_STATE, "recompute fill needs the lane kernel");
    {
        Request both = rc;
        both.tb = true;
        expect_error("rc with words", plan_fill(shape(c2, c2), both, unset, kLds), GA_E_STATE,
                     "recompute fill needs the lane kernel");
    }
    {
        // a linked slab with a right neighbour, 1500 stripes of 512 columns: resident only as 8-wave workgroups, which
        // the checkpointing variant does not run, and rounds of 4-wave ones are not for such a slab
        Problem pb = shape(c4, 768000);
        pb.slab = pb.in_linked = pb.out_linked = true;
        pb.n_global = 2 * pb.n;
        expect_plan("linked slab, score", plan_fill(pb, score, unset, kLds), kLane, 8, 1500, 8, 188);
        expect_error("linked slab, rc", plan_fill(pb, rc, unset, kLds), GA_E_STATE, "recompute fill geometry");
    }
    {
        Knobs kn = unset;
        kn.dev_avail = 1 << 20;  // no spacing fits 1 MB: the stripes narrow to one column per lane, then give up
        expect_error("1 MB available", plan_fill(shape(c3, c3), rc, kn, kLds), GA_E_NOMEM,
                     "recompute walk: the checkpoints do not fit the budget / free device memory");
        Request fixed = rc;  // GA_RC_EVERY=64: its worker fits LDS, its checkpoints do not fit
        fixed.rc_every = 64;
        expect_error("1 MB available, GA_RC_EVERY=64", plan_fill(shape(c3, c3), fixed, kn, kLds), GA_E_NOMEM,
                     "recompute walk: the checkpoints do not fit the budget / free device memory");
        // (no real word width makes the densest worker miss LDS: a formula that does)
        LdsSizes big = kLds;
        big.rc_worker_bytes = [](int, int, int) { return 1 << 20; };
        expect_error("worker past LDS", plan_fill(shape(c3, c3), rc, unset, big), GA_E_RANGE,
                     "recompute walk: a block's codes do not fit LDS");
    }
    {
        Request full = tb;
        full.full = true;
        expect_error("FULL at C2", plan_fill(shape(c2, c2), full, unset, kLds), GA_E_RANGE, "GA_FILL_FULL is for small problems");
        // the FULL debug variant of the anti-diagonal kernel is built for 4 compute waves
        Knobs kn = unset;
        kn.diag_req = 2;
        kn.nwc_req = 8;
        expect_plan("FULL anti-diagonal", plan_fill(shape(300, 1000), full, kn, kLds), kDiag, 1, 16, 4, 4);
    }
}

// The guard bands' layout arithmetic (ga_guard.h), on a host model of one guarded buffer that follows DevBuf::ensure
// step by step: allocate G + cap + G, lay the pattern, re-lay the rear guard when the request changes.
struct GuardModel {
    size_t G;
    uint8_t fill;
    std::vector<uint8_t> raw;
    size_t cap = 0, size = 0;
    GuardModel(size_t G_, uint8_t fill_) : G(G_), fill(fill_) {}
    uint8_t* payload() { return raw.data() + gaguard::payload_off(G); }
    void ensure(size_t bytes) {
        if (bytes <= cap && !raw.empty()) {
            if (bytes == size) return;
            const gaguard::Range r = gaguard::relay_range(size, bytes, G);
            CHECK(r.hi <= cap + G, "re-lay %zu -> %zu leaves the allocation", size, bytes);
            std::memset(payload() + r.lo, fill, r.hi - r.lo);
            size = bytes;
            return;
        }
        cap = std::max<size_t>(bytes, 256);
        raw.assign(gaguard::alloc_bytes(cap, G), 0);  // (a vector of exactly the allocation: ASan sees an overrun)
        std::memset(raw.data(), fill, G);
        std::memset(raw.data() + gaguard::rear_off(bytes, G), fill, cap + G - bytes);
        size = bytes;
    }
    std::vector<gaguard::Violation> check() {
        std::vector<gaguard::Violation> out;
        gaguard::Violation v;
        if (gaguard::make_violation("buf", gaguard::kFront, gaguard::scan(raw.data(), G, fill), size, G, v)) out.push_back(v);
        if (gaguard::make_violation("buf", gaguard::kRear, gaguard::scan(raw.data() + gaguard::rear_off(size, G), G, fill), size, G, v))
            out.push_back(v);
        return out;
    }
};

void test_guard() {
    using namespace gaguard;
    for (long long g : {0LL, 256LL, 4096LL, 1LL << 20}) CHECK(valid_guard_bytes(g), "GA_GUARD_BYTES=%lld refused", g);
    for (long long g : {-256LL, 1LL, 255LL, 257LL, 4097LL, (1LL << 20) + 256}) CHECK(!valid_guard_bytes(g), "GA_GUARD_BYTES=%lld accepted", g);
    CHECK(valid_fill(0) && valid_fill(255) && !valid_fill(256) && !valid_fill(-1), "GA_GUARD_FILL range");
    for (size_t G : {(size_t)256, (size_t)4096})
        for (size_t bytes : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)33333}) {
            GuardModel b(G, 0xA5);
            b.ensure(bytes);
            CHECK(payload_off(G) % kAlign == 0, "payload alignment at G=%zu", G);
            CHECK(b.cap == std::max<size_t>(bytes, 256), "cap %zu for %zu bytes", b.cap, bytes);
            CHECK(b.raw.size() == G + b.cap + G, "allocation of %zu bytes", bytes);
            CHECK(rear_off(bytes, G) + G <= b.raw.size(), "rear guard of %zu bytes inside the allocation", bytes);
            CHECK(b.check().empty(), "fresh buffer of %zu bytes not clean", bytes);
            // the whole payload may be written: nothing is reported
            std::memset(b.payload(), 0x11, bytes);
            CHECK(b.check().empty(), "payload writes of %zu bytes reported", bytes);
            // the first and the last byte of each guard, alone and together
            struct Poke { int side; size_t idx, n; };
            for (const Poke& pk : {Poke{kFront, 0, 1}, Poke{kFront, G - 1, 1}, Poke{kRear, 0, 1}, Poke{kRear, G - 1, 1},
                                   Poke{kFront, 0, G}, Poke{kRear, 0, G}, Poke{kRear, 3, 5}}) {
                uint8_t* at = (pk.side == kFront ? b.raw.data() : b.raw.data() + rear_off(bytes, G)) + pk.idx;
                std::memset(at, 0x5A, pk.n);
                const auto vs = b.check();
                CHECK(vs.size() == 1, "%zu violations, expected one", vs.size());
                if (vs.size() == 1) {
                    const long long want = pk.side == kFront ? (long long)pk.idx - (long long)G : (long long)(bytes + pk.idx);
                    CHECK(vs[0].side == pk.side && vs[0].offset == want && vs[0].changed == pk.n &&
                              vs[0].last == want + (long long)pk.n - 1 && vs[0].payload == bytes && vs[0].name == "buf",
                          "report '%s' for side %d idx %zu n %zu of %zu bytes", describe(vs[0]).c_str(), pk.side, pk.idx, pk.n, bytes);
                }
                std::memset(at, 0xA5, pk.n);
                CHECK(b.check().empty(), "guard not clean after the pattern was restored");
            }
        }
    // two guards at once, and the text of a report
    {
        GuardModel b(256, 0xFF);
        b.ensure(1001);  // an unaligned end: the rear guard starts at payload byte 1001
        b.raw[256 - 8] = 0;
        b.payload()[1001 + 7] = 0;
        b.payload()[1001 + 9] = 0;
        const auto vs = b.check();
        CHECK(vs.size() == 2 && describe(vs) == "buf front -8 n=1 last=-8 payload=1001; buf rear +1008 n=2 last=+1010 payload=1001",
              "report '%s'", describe(vs).c_str());
    }
    // shrink, then grow, inside one allocation: the bytes both requests cover keep their contents, the rear guard
    // follows the request, and what the old guard covered is pattern again (no stale guard inside the payload is
    // mistaken for data, no stale payload inside the guard for a stray store)
    {
        const size_t G = 256;
        GuardModel b(G, 0xA5);
        b.ensure(5000);
        for (size_t k = 0; k < 5000; k++) b.payload()[k] = (uint8_t)(k * 7 + 1) | 1;
        const uint8_t* before = b.raw.data();
        b.ensure(129);
        CHECK(b.raw.data() == before && b.cap == 5000 && b.size == 129, "a smaller request reallocated");
        CHECK(b.check().empty(), "after the shrink: %s", describe(b.check()).c_str());
        bool kept = true;
        for (size_t k = 0; k < 129; k++) kept = kept && b.payload()[k] == ((uint8_t)(k * 7 + 1) | 1);
        CHECK(kept, "the shrink lost payload below the new end");
        b.payload()[129] = 0;  // one past the smaller request: the moved guard sees it
        auto vs = b.check();
        CHECK(vs.size() == 1 && vs[0].side == kRear && vs[0].offset == 129 && vs[0].payload == 129, "store past a shrunk request: %s",
              describe(vs).c_str());
        b.ensure(4097);
        CHECK(b.raw.data() == before && b.size == 4097, "growing inside cap reallocated");
        CHECK(b.check().empty(), "after the growth: %s", describe(b.check()).c_str());
        kept = true;
        for (size_t k = 0; k < 129; k++) kept = kept && b.payload()[k] == ((uint8_t)(k * 7 + 1) | 1);
        CHECK(kept, "the growth lost payload below the old end");
        b.ensure(5000);
        CHECK(b.check().empty() && rear_off(5000, G) + G == b.raw.size(), "back at the full size");
        b.ensure(5001);  // past cap: a new allocation
        CHECK(b.cap == 5001 && b.check().empty(), "growth past cap");
        const Range r = relay_range(700, 300, G);
        CHECK(r.lo == 300 && r.hi == 700 + G, "relay_range(700, 300) = [%zu, %zu)", r.lo, r.hi);
    }
}

// ---------------------------------------------------------------- the traceback call's pure part (ga_walk_plan.h)
using KnobMap = std::map<std::string, std::string>;

// the knobs of `kv` as a context would parse them: in an experiments build (xknobs) xget sees what get sees
template <typename K>
K parse_knobs(const KnobMap& kv, bool xknobs = false) {
    auto get = [&kv](const char* name) -> const char* {
        const auto it = kv.find(name);
        return it == kv.end() ? nullptr : it->second.c_str();
    };
    auto none = [](const char*) -> const char* { return nullptr; };
    return xknobs ? K::parse(get, get) : K::parse(get, none);
}
gawalk::Knobs walk_knobs(const KnobMap& kv, bool xknobs = false) { return parse_knobs<gawalk::Knobs>(kv, xknobs); }

void test_walk_knobs() {
    {
        const gawalk::Knobs kn = walk_knobs({});
        CHECK(kn.rc == -1 && !kn.rc_min_cells && kn.rc_every == 0 && kn.rc_loaders == 14 && kn.rc_tag_fault == 0 &&
                  !kn.rc_wpw && kn.rc_span == 32 && kn.rc_cone == 3 && !kn.rc_win && kn.rc_servers == 64 &&
                  kn.rc_decode_lag == 0 && !kn.rc_decode_check,
              "GA_RC_* defaults");
        CHECK(kn.walk_skip_corners == 1 && kn.walk_loaders == 14 && !kn.walk_nostream && !kn.tb_band_rows &&
                  kn.tb_budget == (int64_t)64 << 30 && !kn.dev_avail,
              "GA_WALK_* / GA_TB_* / GA_DEV_AVAIL_MB defaults");
        CHECK(gawalk::servers(kn) == 64, "64 recompute workgroups by default");
    }
    // every clamp: one step outside each end, both ends, inside
    struct Clamp { const char* name; int gawalk::Knobs::*field; bool x; int in[5], out[5]; };
    const Clamp clamps[] = {
        {"GA_RC_LOADERS", &gawalk::Knobs::rc_loaders, true, {11, 12, 13, 14, 15}, {12, 12, 13, 14, 14}},
        {"GA_RC_SPAN", &gawalk::Knobs::rc_span, false, {1, 2, 5, 32, 33}, {2, 2, 5, 32, 32}},
        {"GA_RC_CONE", &gawalk::Knobs::rc_cone, false, {0, 1, 4, 8, 9}, {1, 1, 4, 8, 8}},
        {"GA_RC_SERVERS", &gawalk::Knobs::rc_servers, false, {0, 1, 100, 255, 256}, {1, 1, 100, 255, 255}},
        {"GA_RC_TAG_FAULT", &gawalk::Knobs::rc_tag_fault, false, {-2, -1, 0, 1, 7}, {0, 0, 0, 1, 7}},
        // (no clamp: the experiments build's values as given)
        {"GA_WALK_SKIP_CORNERS", &gawalk::Knobs::walk_skip_corners, true, {-1, 0, 2, 3, 9}, {-1, 0, 2, 3, 9}},
        {"GA_WALK_LOADERS", &gawalk::Knobs::walk_loaders, true, {0, 12, 13, 14, 20}, {0, 12, 13, 14, 20}},
        {"GA_RC", &gawalk::Knobs::rc, false, {-1, 0, 1, 2, 7}, {-1, 0, 1, 2, 7}},
        {"GA_RC_EVERY", &gawalk::Knobs::rc_every, false, {64, 128, 256, 4096, 1 << 20}, {64, 128, 256, 4096, 1 << 20}},
    };
    for (const Clamp& cl : clamps)
        for (int k = 0; k < 5; k++) {
            const gawalk::Knobs kn = walk_knobs({{cl.name, std::to_string(cl.in[k])}}, cl.x);
            CHECK(kn.*cl.field == cl.out[k], "%s=%d parsed as %d, expected %d", cl.name, cl.in[k], kn.*cl.field, cl.out[k]);
        }
    for (const auto& [in, out] : {std::pair<int, int>{3, 4}, {4, 4}, {5, 5}, {1000, 1000}}) {
        const gawalk::Knobs kn = walk_knobs({{"GA_RC_WIN", std::to_string(in)}});
        CHECK(kn.rc_win && *kn.rc_win == out, "GA_RC_WIN=%d", in);
    }
    {
        const gawalk::Knobs kn = walk_knobs({{"GA_RC_DECODE_LAG", "3"}, {"GA_RC_DECODE_CHECK", "0"}, {"GA_WALK_NOSTREAM", "0"},
                                             {"GA_TB_BUDGET_MB", "100"}, {"GA_DEV_AVAIL_MB", "5"}, {"GA_TB_BAND_ROWS", "40"},
                                             {"GA_RC_MIN_CELLS", "5000000000"}, {"GA_RC_WPW", "0"}});
        CHECK(kn.rc_decode_lag == 1536 && kn.rc_decode_check && kn.walk_nostream, "lag in blocks of 512; flags set by presence");
        CHECK(kn.tb_budget == (int64_t)100 << 20 && kn.dev_avail && *kn.dev_avail == (int64_t)5 << 20, "megabytes to bytes");
        CHECK(kn.tb_band_rows && *kn.tb_band_rows == 40 && kn.rc_min_cells && *kn.rc_min_cells == 5000000000LL &&
                  kn.rc_wpw && *kn.rc_wpw == 0,
              "optional knobs as given");
    }
    {
        // the knobs of dropped paths: invisible to a shipped build, whose xget sees nothing
        const KnobMap kv = {{"GA_WALK_SKIP_CORNERS", "3"}, {"GA_WALK_LOADERS", "12"}, {"GA_RC_LOADERS", "12"}};
        const gawalk::Knobs ship = walk_knobs(kv), xb = walk_knobs(kv, true);
        CHECK(ship.walk_skip_corners == 1 && ship.walk_loaders == 14 && ship.rc_loaders == 14, "shipped build read an xknob");
        CHECK(xb.walk_skip_corners == 3 && xb.walk_loaders == 12 && xb.rc_loaders == 12, "experiments build's xknobs");
    }
}

void test_walk_paths() {
    using gawalk::rc_eligible;
    const gawalk::Knobs unset, never = walk_knobs({{"GA_RC", "0"}}), always = walk_knobs({{"GA_RC", "1"}});
    // the shape's floor (GA_RC=1: the shape alone decides)
    CHECK(rc_eligible(shape(256, 256), always, false) && !rc_eligible(shape(255, 256), always, false) &&
              !rc_eligible(shape(256, 255), always, false),
          "256 rows and columns at the least");
    CHECK(rc_eligible(shape(256, 256, 32), always, false) && !rc_eligible(shape(256, 256, 33), always, false), "K <= 32");
    {
        gaplan::Problem pb = shape(256, 256);
        pb.qbytes = 2;
        CHECK(!rc_eligible(pb, always, false) && !rc_eligible(pb, always, true), "an int16 profile");
    }
    CHECK(!rc_eligible(shape(100000, 100000), never, false) && !rc_eligible(shape(100000, 100000), never, true), "GA_RC=0");
    CHECK(!rc_eligible(shape(256, 256), unset, false), "a small problem by default");
    // the cell thresholds: 2^26 for the single call (8191 * 8193 = 2^26 - 1), 2^32 for a slab (65535 * 65537 = 2^32 - 1)
    CHECK(rc_eligible(shape(8192, 8192), unset, false) && !rc_eligible(shape(8191, 8193), unset, false), "2^26 cells");
    CHECK(!rc_eligible(shape(8192, 8192), unset, true), "2^26 cells are too few for a slab");
    CHECK(rc_eligible(shape(65536, 65536), unset, true) && !rc_eligible(shape(65535, 65537), unset, true), "2^32 cells");
    {
        const gawalk::Knobs kn = walk_knobs({{"GA_RC_MIN_CELLS", "1000000"}});
        for (bool slab_call : {false, true})
            CHECK(rc_eligible(shape(1000, 1000), kn, slab_call) && !rc_eligible(shape(1000, 999), kn, slab_call),
                  "GA_RC_MIN_CELLS=1000000, slab call %d", (int)slab_call);
    }
    // the lean checkpoint store's 32-bit buffer: (m + 1 + 64) * 8 < 0x7ffffff0 holds up to m = 268435388
    CHECK(rc_eligible(shape(268435388, 256), always, false) && !rc_eligible(shape(268435389, 256), always, false),
          "rc_rows_fit's last row count");
    {
        gaplan::Problem pb = shape(65536, 65536);
        pb.slab = true;
        CHECK(!rc_eligible(pb, unset, false) && !rc_eligible(pb, always, false) && rc_eligible(pb, unset, true),
              "a slab context qualifies on the slab call only");
    }

    using gawalk::band_rows;
    const int64_t plenty = INT64_MAX / 4;
    // forced rows round down to whole 16-row chunks, and band only where two bands fit
    for (const auto& [rows, Bh] : {std::pair<int, int>{15, 0}, {16, 16}, {40, 32}})
        CHECK(band_rows(1000, 1000, 1, walk_knobs({{"GA_TB_BAND_ROWS", std::to_string(rows)}}), plenty) == Bh,
              "GA_TB_BAND_ROWS=%d", rows);
    {
        const gawalk::Knobs kn = walk_knobs({{"GA_TB_BAND_ROWS", "32"}});
        CHECK(band_rows(63, 1000, 1, kn, plenty) == 0 && band_rows(64, 1000, 1, kn, 0) == 32, "forced rows: m >= 2 * Bh");
    }
    {
        // 4096 x 1000 at one-byte words: 1024 bytes a row, 4 MiB in all
        gawalk::Knobs kn;
        kn.tb_budget = (int64_t)4 << 20;
        CHECK(band_rows(4096, 1000, 1, kn, plenty) == 0, "words that fit the budget exactly");
        kn.tb_budget--;  // 4095 rows fit, 4080 in whole chunks: no two such bands in 4096 rows, so no banding either
        CHECK(band_rows(4096, 1000, 1, kn, plenty) == 0, "one byte less: a band of 4080 rows does not halve 4096");
        kn.tb_budget = (int64_t)2 << 20;
        CHECK(band_rows(4096, 1000, 1, kn, plenty) == 2048 && band_rows(4095, 1000, 1, kn, plenty) == 0, "half the words");
        kn.tb_budget--;
        CHECK(band_rows(4096, 1000, 1, kn, plenty) == 2032, "half the words less one byte: 2047 rows, 2032 in chunks");
        CHECK(band_rows(4096, 1000, 4, kn, plenty) == 496, "4-byte words: 511 rows fit, 496 in chunks");
        // the device's free memory below the budget (the default 64 GB here)
        CHECK(band_rows(4096, 1000, 1, gawalk::Knobs(), 1 << 20) == 1024, "1 MiB available");
        CHECK(band_rows(4096, 1000, 1, gawalk::Knobs(), plenty) == 0, "64 GB by default");
        // the 64-row floor: 10 rows' worth available
        CHECK(band_rows(4096, 1000, 1, gawalk::Knobs(), 10 * 1024) == 64 && band_rows(128, 1000, 1, gawalk::Knobs(), 10 * 1024) == 64 &&
                  band_rows(127, 1000, 1, gawalk::Knobs(), 10 * 1024) == 0,
              "the 64-row floor");
    }

    CHECK(gawalk::streamed(256, 256, unset) && !gawalk::streamed(255, 1000, unset) && !gawalk::streamed(1000, 255, unset) &&
              !gawalk::streamed(1000, 1000, walk_knobs({{"GA_WALK_NOSTREAM", "1"}})),
          "streamed levels from 256 x 256 up unless GA_WALK_NOSTREAM");

    // workers per recompute workgroup: 20000-byte workers, of which (2 * 65536 - 1024) / 20000 = 6 fit
    CHECK(gawalk::workers(false, 20000, unset) == 1, "one worker unless GA_RC_WPW");
    for (const auto& [wpw, n] : {std::pair<int, int>{0, 1}, {4, 4}, {99, 6}})
        CHECK(gawalk::workers(false, 20000, walk_knobs({{"GA_RC_WPW", std::to_string(wpw)}})) == n, "GA_RC_WPW=%d", wpw);
    CHECK(gawalk::workers(false, 1000, walk_knobs({{"GA_RC_WPW", "99"}})) == 16, "16 workers at the most");
    CHECK(gawalk::workers(true, 20000, walk_knobs({{"GA_RC_WPW", "99"}})) == 1 && gawalk::workers(true, 20000, unset) == 1,
          "the tie-to-tie walk's one worker");
}

// The default windows (cone 3, span 32) at 1, 2, 4 and 8 columns per lane, recorded from the candidate loop as it stood
// in ga_host.cpp's rc_walk_launch before it moved to ga_walk_plan.h (that loop compiled verbatim in a program of its own)
const unsigned char kWindows[4][64] = {
    {0, 1, 8, 9, 18, 10, 17, 27, 2, 16, 19, 26, 36, 11, 25, 28, 35, 45, 3, 20, 24, 34, 37, 44, 54, 12, 29, 33, 43, 46, 53, 63,
     4, 21, 32, 38, 42, 52, 55, 62, 13, 30, 41, 47, 51, 61, 71, 5, 22, 39, 40, 50, 60, 70, 14, 31, 49, 59, 69, 79, 6, 23, 48, 58},
    {0, 1, 8, 9, 17, 16, 25, 34, 26, 18, 24, 33, 42, 51, 10, 43, 2, 32, 35, 41, 50, 59, 68, 27, 60, 19, 40, 49, 52, 58, 67, 76,
     85, 11, 44, 77, 3, 36, 48, 57, 66, 69, 75, 84, 93, 102, 28, 61, 94, 20, 53, 56, 65, 74, 83, 86, 92, 101, 110, 119, 12, 45,
     78, 111},
    {0, 1, 8, 9, 16, 33, 25, 17, 24, 41, 32, 49, 66, 58, 40, 50, 57, 74, 42, 34, 48, 65, 82, 99, 26, 91, 18, 56, 73, 83, 90, 107,
     10, 75, 2, 64, 67, 81, 98, 115, 132, 59, 124, 51, 72, 89, 106, 116, 123, 140, 43, 108, 35, 80, 97, 100, 114, 131, 148, 165,
     27, 92, 157, 19},
    {0, 1, 8, 9, 16, 24, 32, 65, 57, 40, 49, 73, 41, 33, 48, 81, 25, 17, 56, 89, 64, 97, 130, 122, 72, 105, 114, 138, 106, 80, 98,
     113, 146, 90, 82, 88, 121, 154, 74, 66, 96, 129, 162, 195, 58, 187, 50, 104, 137, 170, 179, 203, 42, 171, 34, 112, 145, 163,
     178, 211, 26, 155, 18, 120}};

void test_walk_window() {
    for (int TD : {1, 2, 4, 8})
        for (int cone : {1, 3, 8})
            for (int span : {2, 3, 8, 32}) {
                const KnobMap kv = {{"GA_RC_CONE", std::to_string(cone)}, {"GA_RC_SPAN", std::to_string(span)}};
                const gawalk::Window w = gawalk::window(TD, walk_knobs(kv));
                const int cols = std::min(span, 8), want = std::min(64, span * cols);
                // the walker's own 2 x 2 blocks first: it waits on no others, so the walk always makes progress
                CHECK(w.off[0] == 0 && w.off[1] == 1 && w.off[2] == 8 && w.off[3] == 9, "TD %d cone %d span %d: first four %d %d %d %d",
                      TD, cone, span, w.off[0], w.off[1], w.off[2], w.off[3]);
                CHECK(w.nwin == want, "TD %d cone %d span %d: %d window blocks, expected %d", TD, cone, span, w.nwin, want);
                bool seen[256] = {};
                int last = -1;
                for (int k = 0; k < 64; k++) {
                    const int di = w.off[k] >> 3, dj = w.off[k] & 7, dist = di - dj * TD;
                    const int key = di + dj * TD + cone * (dist < 0 ? -dist : dist);
                    if (k >= w.nwin) {
                        CHECK(w.off[k] == 0, "TD %d cone %d span %d: entry %d past the window is %d", TD, cone, span, k, w.off[k]);
                        continue;
                    }
                    CHECK(!seen[w.off[k]] && di < span && dj < cols, "TD %d cone %d span %d: entry %d = %d repeats or is out of range",
                          TD, cone, span, k, w.off[k]);
                    seen[w.off[k]] = true;
                    if (k >= 4) {
                        CHECK(key >= last, "TD %d cone %d span %d: key %d at entry %d after %d", TD, cone, span, key, k, last);
                        last = key;
                    }
                }
                // GA_RC_WIN caps the window, never below the four
                KnobMap capped = kv;
                capped["GA_RC_WIN"] = "4";
                CHECK(gawalk::window(TD, walk_knobs(capped)).nwin == 4, "GA_RC_WIN=4");
                capped["GA_RC_WIN"] = "10";
                CHECK(gawalk::window(TD, walk_knobs(capped)).nwin == std::min(want, 10), "GA_RC_WIN=10");
                capped["GA_RC_WIN"] = "1";
                CHECK(gawalk::window(TD, walk_knobs(capped)).nwin == 4, "GA_RC_WIN=1");
                capped["GA_RC_WIN"] = "1000";
                CHECK(gawalk::window(TD, walk_knobs(capped)).nwin == want, "GA_RC_WIN=1000");
            }
    const int tds[4] = {1, 2, 4, 8};
    for (int t = 0; t < 4; t++) {
        const gawalk::Window w = gawalk::window(tds[t], gawalk::Knobs());
        CHECK(w.nwin == 64 && std::memcmp(w.off, kWindows[t], 64) == 0, "the default window at %d columns per lane changed", tds[t]);
    }
}

// ---------------------------------------------------------------- a context's options (ga_opts.h)
// collect() over an environ-style array of `env` and the option string `opts` (nullptr: none)
struct Collected {
    int rc;
    KnobMap kv;
    std::string why;
};
Collected collect(const std::vector<std::string>& env, const char* opts, bool experiments = false) {
    std::vector<const char*> envp;
    for (const std::string& e : env) envp.push_back(e.c_str());
    envp.push_back(nullptr);
    Collected c;
    c.rc = gaopts::collect(envp.data(), opts, experiments, c.kv, c.why);
    return c;
}

void test_opts_collect() {
    // what a process may have around a shipped knob: an option-only knob, a fault injector, a name without a value,
    // a variable of somebody else's
    const std::vector<std::string> strays = {"GA_GUARD_BYTES=100", "GA_RC_TAG_FAULT=3", "GA_NOVALUE", "PATH=/bin", "XGA_RC=1"};
    std::vector<std::string> all = strays;
    int nk = 0;
    for (const char* k : gaopts::kEnvKnobs) {
        std::vector<std::string> env = strays;
        const std::string val = "v" + std::to_string(nk++);
        env.insert(env.begin() + 2, std::string(k) + "=" + val);
        all.push_back(std::string(k) + "=" + val);
        const Collected ship = collect(env, nullptr), xb = collect(env, nullptr, true);
        CHECK(ship.rc == GA_OK && ship.kv == (KnobMap{{k, val}}), "%s from the environment: %zu knobs", k, ship.kv.size());
        CHECK(xb.rc == GA_OK && xb.kv == (KnobMap{{k, val}, {"GA_GUARD_BYTES", "100"}, {"GA_RC_TAG_FAULT", "3"}}),
              "%s from the environment of an experiments build: %zu knobs", k, xb.kv.size());
        CHECK(gaopts::env_knob(k, false) && gaopts::env_knob(k, true), "env_knob(%s)", k);
    }
    CHECK(nk == 14 && collect(all, nullptr).kv.size() == 14 && collect(all, nullptr, true).kv.size() == 16, "%d shipped knobs", nk);
    struct Rule { const char* name; bool ship, xb; };
    for (const Rule& r : {Rule{"GA_GUARD_BYTES", false, true}, Rule{"GA_RC_", false, true}, Rule{"GA_", false, true},
                          Rule{"PATH", false, false}, Rule{"ga_rc", false, false}, Rule{"", false, false}})
        CHECK(gaopts::env_knob(r.name, false) == r.ship && gaopts::env_knob(r.name, true) == r.xb, "env_knob's two rules on '%s'", r.name);
    {
        KnobMap kv;
        std::string why;
        CHECK(gaopts::collect(nullptr, nullptr, false, kv, why) == GA_OK && kv.empty() && why.empty(), "no environment, no options");
        CHECK(collect({}, nullptr).rc == GA_OK && collect({"GA_RC=1"}, nullptr).kv == (KnobMap{{"GA_RC", "1"}}), "options == nullptr");
    }
    {
        // options override the environment, a later option an earlier one; a value keeps its '=' and may be empty
        const Collected c = collect({"GA_RC=0", "GA_RC_SERVERS=48", "GA_PIPE_TRACE=/tmp/a=b"}, "GA_RC=1;GA_X=a=b;GA_Y=;GA_Z=1;GA_Z=2");
        CHECK(c.rc == GA_OK && c.kv == (KnobMap{{"GA_RC", "1"}, {"GA_RC_SERVERS", "48"}, {"GA_PIPE_TRACE", "/tmp/a=b"},
                                                {"GA_X", "a=b"}, {"GA_Y", ""}, {"GA_Z", "2"}}),
              "precedence and '=' in values: %zu knobs (%s)", c.kv.size(), c.why.c_str());
        // an option may name what the environment may not
        const Collected g = collect({"GA_GUARD_BYTES=100"}, "GA_GUARD_BYTES=0");
        CHECK(g.rc == GA_OK && g.kv == (KnobMap{{"GA_GUARD_BYTES", "0"}}), "an option-only knob");
    }
    {
        // both separators, empty items, trailing separators
        const KnobMap want = {{"GA_A", "1"}, {"GA_B", "2"}, {"GA_C", "3"}, {"GA_D", "4"}};
        for (const char* opts : {"GA_A=1;GA_B=2;GA_C=3;GA_D=4", "GA_A=1\nGA_B=2\nGA_C=3\nGA_D=4\n", ";;GA_A=1;\nGA_B=2\n\n;GA_C=3;;GA_D=4;\n;"}) {
            const Collected c = collect({}, opts);
            CHECK(c.rc == GA_OK && c.kv == want, "separators in '%s': %zu knobs (%s)", opts, c.kv.size(), c.why.c_str());
        }
        for (const char* opts : {"", ";", "\n", ";\n;;"}) CHECK(collect({}, opts).rc == GA_OK && collect({}, opts).kv.empty(), "empty options");
        // (a space is no separator: it belongs to the value)
        CHECK(collect({}, "GA_A=1 GA_B=2").kv == (KnobMap{{"GA_A", "1 GA_B=2"}}), "a space inside a value");
    }
    // the two malformed forms, wherever they stand
    struct Bad { const char* opts; const char* why; };
    for (const Bad& b : {Bad{"GA_RC", "bad option 'GA_RC' (expected GA_NAME=VALUE)"},
                         Bad{"RC=1", "bad option 'RC=1' (expected GA_NAME=VALUE)"},
                         Bad{"GA_RC=1;FOO=2;GA_RC_EVERY=64", "bad option 'FOO=2' (expected GA_NAME=VALUE)"},
                         Bad{"GA_RC=1\nGA_RC_EVERY\n", "bad option 'GA_RC_EVERY' (expected GA_NAME=VALUE)"},
                         Bad{" GA_RC=1", "bad option ' GA_RC=1' (expected GA_NAME=VALUE)"},
                         Bad{"ga_rc=1", "bad option 'ga_rc=1' (expected GA_NAME=VALUE)"}}) {
        const Collected c = collect({}, b.opts);
        CHECK(c.rc == GA_E_ARG && c.why == b.why, "options '%s': %d (%s)", b.opts, c.rc, c.why.c_str());
    }
}

void test_opts_check() {
    struct Case { KnobMap kv; const char* why; };  // why: nullptr when the options are accepted
    const std::string p20 = std::to_string(1 << 20), p21 = std::to_string(1 << 21);
    const Case cases[] = {
        {{}, nullptr},
        {{{"GA_RC_EVERY", "63"}}, "GA_RC_EVERY must be a power of two in [64, 2^20], not '63'"},
        {{{"GA_RC_EVERY", "64"}}, nullptr},
        {{{"GA_RC_EVERY", "96"}}, "GA_RC_EVERY must be a power of two in [64, 2^20], not '96'"},
        {{{"GA_RC_EVERY", p20}}, nullptr},
        {{{"GA_RC_EVERY", p21}}, "GA_RC_EVERY must be a power of two in [64, 2^20], not '2097152'"},
        {{{"GA_RC_EVERY", "many"}}, "GA_RC_EVERY must be a power of two in [64, 2^20], not 'many'"},
        {{{"GA_BATCH_RNG", "host"}}, nullptr},
        {{{"GA_BATCH_RNG", "device"}}, nullptr},
        {{{"GA_BATCH_RNG", "gpu"}}, "GA_BATCH_RNG must be host or device, not 'gpu'"},
        {{{"GA_BATCH_RNG_DEVICE_MAX_STEPS", "-1"}}, "GA_BATCH_RNG_DEVICE_MAX_STEPS must be in [0, 2^20], not '-1'"},
        {{{"GA_BATCH_RNG_DEVICE_MAX_STEPS", "0"}}, nullptr},
        {{{"GA_BATCH_RNG_DEVICE_MAX_STEPS", p20}}, nullptr},
        {{{"GA_BATCH_RNG_DEVICE_MAX_STEPS", "1048577"}}, "GA_BATCH_RNG_DEVICE_MAX_STEPS must be in [0, 2^20], not '1048577'"},
        {{{"GA_BATCH_RNG_WORD_CAP", "0"}}, "GA_BATCH_RNG_WORD_CAP must be in [1, 1024], not '0'"},
        {{{"GA_BATCH_RNG_WORD_CAP", "1"}}, nullptr},
        {{{"GA_BATCH_RNG_WORD_CAP", "1024"}}, nullptr},
        {{{"GA_BATCH_RNG_WORD_CAP", "1025"}}, "GA_BATCH_RNG_WORD_CAP must be in [1, 1024], not '1025'"},
        // tests/test_gpu_guard.py test_guard_options_are_checked's eight
        {{{"GA_GUARD_BYTES", "100"}}, "GA_GUARD_BYTES must be 0 or a multiple of 256 up to 2^20, not '100'"},
        {{{"GA_GUARD_BYTES", "4097"}}, "GA_GUARD_BYTES must be 0 or a multiple of 256 up to 2^20, not '4097'"},
        {{{"GA_GUARD_BYTES", "-256"}}, "GA_GUARD_BYTES must be 0 or a multiple of 256 up to 2^20, not '-256'"},
        {{{"GA_GUARD_BYTES", "1048832"}}, "GA_GUARD_BYTES must be 0 or a multiple of 256 up to 2^20, not '1048832'"},
        {{{"GA_GUARD_BYTES", "4k"}}, "GA_GUARD_BYTES must be 0 or a multiple of 256 up to 2^20, not '4k'"},
        {{{"GA_GUARD_BYTES", "256"}, {"GA_GUARD_FILL", "256"}}, "GA_GUARD_FILL must be a byte value in [0, 255], not '256'"},
        {{{"GA_GUARD_POISON", "1"}}, "GA_GUARD_POISON=1 needs GA_GUARD_BYTES"},
        {{{"GA_GUARD_BYTES", "256"}, {"GA_GUARD_POISON", "2"}}, "GA_GUARD_POISON must be 0 or 1, not '2'"},
        // whole(): a number and nothing else
        {{{"GA_GUARD_BYTES", ""}}, "GA_GUARD_BYTES must be 0 or a multiple of 256 up to 2^20, not ''"},
        {{{"GA_GUARD_BYTES", "256"}, {"GA_GUARD_FILL", ""}}, "GA_GUARD_FILL must be a byte value in [0, 255], not ''"},
        {{{"GA_GUARD_BYTES", "256"}, {"GA_GUARD_FILL", "-1"}}, "GA_GUARD_FILL must be a byte value in [0, 255], not '-1'"},
        {{{"GA_GUARD_BYTES", "256"}, {"GA_GUARD_FILL", "0x3c "}}, "GA_GUARD_FILL must be a byte value in [0, 255], not '0x3c '"},
        {{{"GA_GUARD_BYTES", "0"}, {"GA_GUARD_POISON", "1"}}, "GA_GUARD_POISON=1 needs GA_GUARD_BYTES"},
        {{{"GA_GUARD_POISON", "0"}}, nullptr},
        {{{"GA_GUARD_POISON", ""}}, "GA_GUARD_POISON must be 0 or 1, not ''"},
        // today's order: the spacing, the tables' route, the guards
        {{{"GA_GUARD_BYTES", "100"}, {"GA_BATCH_RNG", "gpu"}, {"GA_RC_EVERY", "96"}}, "GA_RC_EVERY must be a power of two in [64, 2^20], not '96'"},
        {{{"GA_GUARD_BYTES", "100"}, {"GA_BATCH_RNG_WORD_CAP", "0"}, {"GA_BATCH_RNG", "gpu"}}, "GA_BATCH_RNG must be host or device, not 'gpu'"},
        {{{"GA_GUARD_BYTES", "100"}, {"GA_BATCH_RNG_WORD_CAP", "0"}, {"GA_BATCH_RNG_DEVICE_MAX_STEPS", "-1"}},
         "GA_BATCH_RNG_DEVICE_MAX_STEPS must be in [0, 2^20], not '-1'"},
        {{{"GA_GUARD_BYTES", "100"}, {"GA_BATCH_RNG_WORD_CAP", "0"}}, "GA_BATCH_RNG_WORD_CAP must be in [1, 1024], not '0'"},
        {{{"GA_GUARD_BYTES", "100"}, {"GA_GUARD_FILL", "256"}, {"GA_GUARD_POISON", "2"}},
         "GA_GUARD_BYTES must be 0 or a multiple of 256 up to 2^20, not '100'"},
        // names nobody reads are nobody's to refuse
        {{{"GA_NO_SUCH_KNOB", "1"}, {"GA_RC", "many"}}, nullptr},
    };
    for (const Case& cs : cases) {
        std::string desc, why;
        for (const auto& [k, v] : cs.kv) desc += k + "=" + v + ";";
        gaopts::GuardOpts g;
        const int rc = gaopts::check(cs.kv, g, why);
        if (cs.why) CHECK(rc == GA_E_ARG && why == cs.why, "options %s: %d (%s)", desc.c_str(), rc, why.c_str());
        else CHECK(rc == GA_OK && why.empty(), "options %s refused: %d (%s)", desc.c_str(), rc, why.c_str());
    }
    {
        gaopts::GuardOpts g;
        std::string why;
        CHECK(gaopts::check({}, g, why) == GA_OK && g.bytes == 0 && g.fill == 0xA5 && !g.poison, "guard mode is off by default");
        CHECK(gaopts::check({{"GA_GUARD_BYTES", "1048576"}, {"GA_GUARD_FILL", "0x3c"}, {"GA_GUARD_POISON", "1"}}, g, why) == GA_OK &&
                  g.bytes == (size_t)1 << 20 && g.fill == 0x3c && g.poison,
              "the guard triple: %zu bytes, fill %ld, poison %d (%s)", g.bytes, g.fill, (int)g.poison, why.c_str());
        CHECK(gaopts::check({{"GA_GUARD_BYTES", "0x100"}, {"GA_GUARD_FILL", "255"}, {"GA_GUARD_POISON", "0"}}, g, why) == GA_OK &&
                  g.bytes == 256 && g.fill == 255 && !g.poison,
              "guard options in hex and decimal");
        CHECK(gaopts::check({{"GA_GUARD_BYTES", "0"}, {"GA_GUARD_FILL", "0"}}, g, why) == GA_OK && g.bytes == 0 && g.fill == 0, "guards off");
    }
}

// one knob's values as given, and what the field holds for each
template <typename K>
struct IntKnob { const char* name; int K::*field; bool x; int in[5], out[5]; };
template <typename K, size_t N>
void check_int_knobs(const IntKnob<K> (&knobs)[N]) {
    for (const IntKnob<K>& kb : knobs) {
        const K unset;
        for (int k = 0; k < 5; k++) {
            const K kn = parse_knobs<K>({{kb.name, std::to_string(kb.in[k])}}, kb.x);
            CHECK(kn.*kb.field == kb.out[k], "%s=%d parsed as %d, expected %d", kb.name, kb.in[k], kn.*kb.field, kb.out[k]);
            // a dropped path's knob: the shipped build does not see it
            if (kb.x) CHECK(parse_knobs<K>({{kb.name, std::to_string(kb.in[k])}}).*kb.field == unset.*kb.field, "shipped build read %s", kb.name);
        }
        CHECK(parse_knobs<K>({{kb.name, "junk"}}, kb.x).*kb.field == parse_knobs<K>({{kb.name, "0"}}, kb.x).*kb.field, "%s=junk is 0", kb.name);
    }
}

void test_lane_knobs() {
    using gaopts::LaneKnobs;
    for (bool x : {false, true}) {
        const LaneKnobs kn = parse_knobs<LaneKnobs>({}, x);
        CHECK(!kn.late && kn.xcd == 0 && kn.hand_direct == 0 && kn.lds_floor == -1 && kn.lane_sub == -1 && kn.lane_tb_sub == -1 &&
                  kn.asm_step == 1 && kn.io_prio == 0 && kn.hand_scope == 0 && kn.poll_win == 0 && kn.out_wave == 1 &&
                  !kn.halo_spin_limit && kn.lean0 == 1 && !kn.rc_fail_alloc && !kn.qprof_wave,
              "GA_LANE_* defaults");
    }
    const IntKnob<LaneKnobs> knobs[] = {
        {"GA_LANE_XCD", &LaneKnobs::xcd, true, {-1, 0, 1, 2, 9}, {-1, 0, 1, 2, 9}},
        {"GA_LANE_DIRECT", &LaneKnobs::hand_direct, false, {-1, 0, 1, 2, 9}, {-1, 0, 1, 2, 9}},
        {"GA_FILL_LDS_FLOOR", &LaneKnobs::lds_floor, false, {-1, 0, 1, 40000, 163840}, {-1, 0, 1, 40000, 163840}},
        {"GA_LANE_SUB", &LaneKnobs::lane_sub, false, {-1, 0, 1, 2, 9}, {-1, 0, 1, 2, 9}},
        {"GA_LANE_TB_SUB", &LaneKnobs::lane_tb_sub, false, {-1, 0, 1, 2, 9}, {-1, 0, 1, 2, 9}},
        {"GA_LANE_ASM", &LaneKnobs::asm_step, false, {-1, 0, 1, 2, 9}, {-1, 0, 1, 2, 9}},
        {"GA_LANE_IOPRIO", &LaneKnobs::io_prio, true, {-1, 0, 1, 2, 3}, {-1, 0, 1, 2, 3}},
        {"GA_LANE_HANDSCOPE", &LaneKnobs::hand_scope, true, {-1, 0, 1, 2, 3}, {-1, 0, 1, 2, 3}},
        {"GA_LANE_POLLWIN", &LaneKnobs::poll_win, false, {-1, 0, 64, 192, 193}, {0, 0, 64, 192, 192}},
        {"GA_LANE_OUTWAVE", &LaneKnobs::out_wave, false, {-1, 0, 1, 2, 9}, {-1, 0, 1, 2, 9}},
        {"GA_LANE_LEAN0", &LaneKnobs::lean0, false, {-1, 0, 1, 2, 9}, {-1, 0, 1, 2, 9}},
    };
    check_int_knobs(knobs);
    for (const auto& [in, out] : {std::pair<const char*, int>{"0", 0}, {"1", 1}, {"-3", -3}, {"junk", 0}}) {
        const LaneKnobs kn = parse_knobs<LaneKnobs>({{"GA_LANE_LATE", in}});
        CHECK(kn.late && *kn.late == out, "GA_LANE_LATE=%s", in);
    }
    for (const auto& [in, out] : {std::pair<const char*, unsigned>{"-5", 1u}, {"0", 1u}, {"1", 1u}, {"1000", 1000u}, {"1073741824", 1u << 30}}) {
        const LaneKnobs kn = parse_knobs<LaneKnobs>({{"GA_HALO_SPIN_LIMIT", in}});
        CHECK(kn.halo_spin_limit && *kn.halo_spin_limit == out, "GA_HALO_SPIN_LIMIT=%s", in);
    }
    for (const auto& [in, out] : {std::pair<const char*, bool>{"0", false}, {"1", true}, {"2", false}, {"-1", false}, {"yes", false}})
        CHECK(parse_knobs<LaneKnobs>({{"GA_RC_FAIL_ALLOC", in}}).rc_fail_alloc == out, "GA_RC_FAIL_ALLOC=%s", in);
    // set by presence, and an experiments build's alone
    CHECK(parse_knobs<LaneKnobs>({{"GA_LANE_QPROF_WAVE", "0"}}, true).qprof_wave && !parse_knobs<LaneKnobs>({{"GA_LANE_QPROF_WAVE", "1"}}).qprof_wave,
          "GA_LANE_QPROF_WAVE");
    auto get_of = [](const KnobMap& kv) {
        return [kv](const char* name) -> const char* {
            const auto it = kv.find(name);
            return it == kv.end() ? nullptr : it->second.c_str();
        };
    };
    CHECK(!gaopts::stream_priority_normal(get_of({})) && gaopts::stream_priority_normal(get_of({{"GA_STREAM_PRIORITY", "normal"}})) &&
              !gaopts::stream_priority_normal(get_of({{"GA_STREAM_PRIORITY", "high"}})) &&
              !gaopts::stream_priority_normal(get_of({{"GA_STREAM_PRIORITY", ""}})),
          "GA_STREAM_PRIORITY=normal and nothing else");
}

void test_batch_knobs() {
    using gaopts::BatchKnobs;
    for (bool x : {false, true}) {  // (no knob of a dropped path among them: both builds read the same)
        const BatchKnobs kn = parse_knobs<BatchKnobs>({}, x);
        CHECK(!kn.rng_device_default && kn.rng_max_steps == 1024 && kn.rng_cap_words == 48 && kn.rng_threads == 0 && !kn.max_cells &&
                  !kn.align_max_cells && !kn.sample_chunk_words && !kn.sample_walk_entries && !kn.rank_table_bytes && !kn.support_bytes,
              "GA_BATCH_* defaults");
    }
    const IntKnob<BatchKnobs> knobs[] = {
        {"GA_BATCH_RNG_WORD_CAP", &BatchKnobs::rng_cap_words, false, {1, 2, 48, 1000, 1024}, {1, 2, 48, 1000, 1024}},
        {"GA_BATCH_RNG_THREADS", &BatchKnobs::rng_threads, false, {-2, 0, 1, 8, 500}, {-2, 0, 1, 8, 500}},
    };
    check_int_knobs(knobs);
    CHECK(parse_knobs<BatchKnobs>({{"GA_BATCH_RNG", "device"}}).rng_device_default && !parse_knobs<BatchKnobs>({{"GA_BATCH_RNG", "host"}}).rng_device_default,
          "GA_BATCH_RNG");
    for (int64_t v : {(int64_t)0, (int64_t)1, (int64_t)1024, (int64_t)1 << 20})
        CHECK(parse_knobs<BatchKnobs>({{"GA_BATCH_RNG_DEVICE_MAX_STEPS", std::to_string(v)}}).rng_max_steps == v,
              "GA_BATCH_RNG_DEVICE_MAX_STEPS=%lld", (long long)v);
    struct Floor { const char* name; std::optional<int64_t> BatchKnobs::*field; int64_t floor; };
    for (const Floor& f : {Floor{"GA_BATCH_MAX_CELLS", &BatchKnobs::max_cells, 0}, Floor{"GA_BATCH_ALIGN_MAX_CELLS", &BatchKnobs::align_max_cells, 0},
                           Floor{"GA_BATCH_SAMPLE_CHUNK_WORDS", &BatchKnobs::sample_chunk_words, 1},
                           Floor{"GA_BATCH_SAMPLE_WALK_ENTRIES", &BatchKnobs::sample_walk_entries, 1},
                           Floor{"GA_BATCH_RANK_TABLE_BYTES", &BatchKnobs::rank_table_bytes, 1},
                           Floor{"GA_BATCH_SUPPORT_BYTES", &BatchKnobs::support_bytes, 1}})
        for (int64_t v : {(int64_t)-7, (int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)2, (int64_t)5000000000LL}) {
            const BatchKnobs kn = parse_knobs<BatchKnobs>({{f.name, std::to_string(v)}});
            const std::optional<int64_t>& got = kn.*f.field;
            CHECK(got && *got == std::max(v, f.floor), "%s=%lld", f.name, (long long)v);
            // each name fills its own field and no other
            int set = 0;
            for (const auto* o : {&kn.max_cells, &kn.align_max_cells, &kn.sample_chunk_words, &kn.sample_walk_entries, &kn.rank_table_bytes, &kn.support_bytes}) set += o->has_value();
            CHECK(set == 1, "%s set %d fields", f.name, set);
        }
}

void test_plan_knobs() {
    using gaplan::Knobs;
    for (bool x : {false, true}) {
        const Knobs kn = parse_knobs<Knobs>({}, x), unset;
        CHECK(kn.T_req == 0 && kn.nwc_req == 0 && kn.diag_req == 0 && kn.lane_T_req == 0 && kn.diag_T_req == 0 && kn.lane_wg_per_cu == 1 &&
                  kn.lane_qrows == 4096 && kn.rc_narrow && kn.rc_budget == (int64_t)96 << 30 && kn.rc_jump == gaplan::kRcJumpDefault &&
                  kn.dev_avail == unset.dev_avail,
              "the planner's defaults");
    }
    const IntKnob<Knobs> knobs[] = {
        {"GA_COLS_PER_LANE", &Knobs::T_req, false, {-1, 0, 1, 4, 8}, {-1, 0, 1, 4, 8}},
        {"GA_FILL_NWC", &Knobs::nwc_req, false, {-1, 0, 4, 8, 16}, {-1, 0, 4, 8, 16}},
        {"GA_LANE_COLS_PER_LANE", &Knobs::lane_T_req, false, {-1, 0, 1, 4, 8}, {-1, 0, 1, 4, 8}},
        {"GA_DIAG_COLS_PER_LANE", &Knobs::diag_T_req, false, {-1, 0, 1, 4, 8}, {-1, 0, 1, 4, 8}},
        {"GA_LANE_WG_PER_CU", &Knobs::lane_wg_per_cu, false, {-1, 0, 1, 2, 3}, {1, 1, 1, 2, 2}},
        {"GA_LANE_QROWS", &Knobs::lane_qrows, false, {0, 64, 1024, 4096, 8192}, {0, 64, 1024, 4096, 8192}},
    };
    check_int_knobs(knobs);
    for (const auto& [in, out] : {std::pair<const char*, int>{"row", 1}, {"diag", 2}, {"lane", 3}, {"auto", 0}, {"", 0}, {"Row", 0}})
        CHECK(parse_knobs<Knobs>({{"GA_FILL_MODE", in}}).diag_req == out, "GA_FILL_MODE=%s", in);
    for (const auto& [in, out] : {std::pair<const char*, bool>{"0", false}, {"1", true}, {"2", true}, {"junk", false}})
        CHECK(parse_knobs<Knobs>({{"GA_RC_NARROW", in}}).rc_narrow == out, "GA_RC_NARROW=%s", in);
    for (int64_t mb : {(int64_t)0, (int64_t)1, (int64_t)98304, (int64_t)300000})
        CHECK(parse_knobs<Knobs>({{"GA_RC_BUDGET_MB", std::to_string(mb)}}).rc_budget == mb << 20, "GA_RC_BUDGET_MB=%lld", (long long)mb);
    // the tie-to-tie walk is an experiments build's to ask for
    CHECK(!parse_knobs<Knobs>({{"GA_RC_JUMP", "1"}}).rc_jump && parse_knobs<Knobs>({{"GA_RC_JUMP", "1"}}, true).rc_jump &&
              !parse_knobs<Knobs>({{"GA_RC_JUMP", "0"}}, true).rc_jump,
          "GA_RC_JUMP");
}

double ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 3 && std::string(argv[1]) == "bench") {
        const int64_t steps = std::atoll(argv[2]);
        const auto st = random_state(1);
        for (int rep = 0; rep < 3; rep++) {
            RngTable R;
            auto t0 = std::chrono::steady_clock::now();
            build_rng(st.data(), steps, R);
            std::printf("table of %lld dispatches: %.3f ms\n", (long long)steps, ms_since(t0));
        }
        PyMT g;
        std::memcpy(g.mt, st.data(), sizeof(uint32_t) * MTN);
        auto t0 = std::chrono::steady_clock::now();
        const int64_t tw = steps * 32 / MTN + 1;
        for (int64_t t = 0; t < tw; t++) g.twist();
        std::printf("twists alone (%lld): %.3f ms (%u)\n", (long long)tw, ms_since(t0), g.mt[5]);
        return 0;
    }
    if (argc >= 2 && std::string(argv[1]) == "envknobs") {
        for (const char* k : gaopts::kEnvKnobs) std::printf("%s\n", k);
        return 0;
    }
    for (uint64_t seed = 1; seed <= 12; seed++) {
        const int64_t steps = seed <= 6 ? (int64_t)(seed * seed * 37) : (int64_t)(seed * 2111);
        test_table(seed, steps);
    }
    test_table(77, 0);
    test_table(78, 1);
    test_table(79, 50000);
    test_checks();
    test_limit_tables();
    test_plan();
    test_walk_knobs();
    test_walk_paths();
    test_walk_window();
    test_guard();
    test_opts_collect();
    test_opts_check();
    test_lane_knobs();
    test_batch_knobs();
    test_plan_knobs();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("ga_host_selftest: all checks passed\n");
    return 0;
}
