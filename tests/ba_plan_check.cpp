// Host-only check of the bundle-adjustment plan (stella_vslam_amd/csrc/ba_plan.h), built and run by tests/test_arena_layouts.py:
// ba_env_parse on tables (defaults, every switch, the clamps at their edges), every plan function against the expression the driver, the
// launchers and the envelope planner used to write out inline, over grids that hold the bench shapes and the neighbours of every
// threshold, and the key of the envelope plan cache.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "ba_plan.h"
#include "layout_check.h"  // CHECK, layout_check_result

using Table = std::map<std::string, std::string>;
static BaEnv parse(const Table& t) {
    return ba_env_parse([&](const char* name) -> const char* {
        const auto it = t.find(name);
        return it == t.end() ? nullptr : it->second.c_str();
    });
}

static bool same_process(const BaEnv::Process& a, const BaEnv::Process& b) {
    return a.dbg == b.dbg && a.share_pairs == b.share_pairs && a.no_fusion == b.no_fusion && a.lin_two_launches == b.lin_two_launches && a.chol_mfma == b.chol_mfma
           && a.dense_one_wg == b.dense_one_wg;
}
static bool same(const BaEnv& a, const BaEnv& b) {
    return same_process(a.proc, b.proc) && a.trace == b.trace && a.team_min_obs == b.team_min_obs && a.one_thread == b.one_thread && a.host_threads == b.host_threads
           && a.solver == b.solver && a.no_dense_tiled == b.no_dense_tiled && a.no_renumber == b.no_renumber && a.no_units == b.no_units && a.copy_on_main == b.copy_on_main
           && a.units_min == b.units_min && a.chunk_shift == b.chunk_shift && a.exchange_full == b.exchange_full && a.host_boundary == b.host_boundary
           && a.schur_order == b.schur_order && a.sky_no_band == b.sky_no_band && a.sky_segments == b.sky_segments && a.sky_one_sided == b.sky_one_sided;
}

static void check_parse() {
    const BaEnv d = parse({});
    CHECK(same(d, BaEnv()));
    CHECK(d.proc.dbg == BA_ENV_DBG_OFF && d.proc.share_pairs == 192 && !d.proc.no_fusion && !d.proc.lin_two_launches && !d.proc.chol_mfma && !d.proc.dense_one_wg);
    CHECK(d.trace == 0 && d.team_min_obs == 400000 && !d.one_thread && d.host_threads == 8 && d.solver == BA_ENV_NOT_SET && !d.no_dense_tiled && !d.no_renumber && !d.no_units);
    CHECK(!d.copy_on_main && d.units_min == 8192 && d.chunk_shift == BA_ENV_NOT_SET && !d.exchange_full && !d.host_boundary && d.schur_order == BA_ENV_NOT_SET);
    CHECK(!d.sky_no_band && d.sky_segments == BA_ENV_NOT_SET && !d.sky_one_sided);

    // every switch is recognised: set alone, it changes the parsed value, and no other name does
    const std::vector<std::pair<const char*, const char*>> all = {
        {"SVGPU_BA_TRACE", "1"}, {"SVGPU_BA_TEAM_MIN_OBS", "1000"}, {"SVGPU_BA_ONE_THREAD", "1"}, {"SVGPU_BA_HOST_THREADS", "3"}, {"SVGPU_BA_SOLVER", "pcg"},
        {"SVGPU_BA_NO_DENSE_TILED", "1"}, {"SVGPU_BA_NO_RENUMBER", "1"}, {"SVGPU_BA_DBG", "1"}, {"SVGPU_BA_NO_UNITS", "1"}, {"SVGPU_BA_COPY_ON_MAIN", "1"},
        {"SVGPU_BA_SHARE_PAIRS", "96"}, {"SVGPU_BA_UNITS_MIN", "1"}, {"SVGPU_BA_CHUNK_SHIFT", "6"}, {"SVGPU_BA_EXCHANGE", "full"}, {"SVGPU_BA_NO_FUSION", "1"},
        {"SVGPU_BA_HOST_BOUNDARY", "1"}, {"SVGPU_BA_LIN_TWO_LAUNCHES", "1"}, {"SVGPU_BA_SCHUR_ORDER", "0"}, {"SVGPU_BA_CHOL", "mfma"}, {"SVGPU_BA_DENSE_ONE_WG", "1"},
        {"SVGPU_SKY_NO_BAND", "1"}, {"SVGPU_SKY_SEGMENTS", "5"}, {"SVGPU_SKY_ONE_SIDED", "1"}};
    CHECK(all.size() == 23);
    std::vector<BaEnv> alone;
    for (const auto& kv : all) {
        alone.push_back(parse({{kv.first, kv.second}}));
        if (same(alone.back(), d)) std::printf("FAIL %s is not recognised\n", kv.first), ++failures;
    }
    for (size_t i = 0; i < alone.size(); ++i)
        for (size_t j = i + 1; j < alone.size(); ++j) CHECK(!same(alone[i], alone[j]));
    CHECK(same(parse({{"SVGPU_BA_UNKNOWN", "1"}, {"SVGPU_SKY_SEGMENT", "3"}}), d));
    // a switch that is "set" counts whatever its value, the empty one included
    CHECK(parse({{"SVGPU_BA_ONE_THREAD", ""}}).one_thread && parse({{"SVGPU_BA_NO_UNITS", "0"}}).no_units && parse({{"SVGPU_BA_TRACE", ""}}).trace == 1);
    CHECK(parse({{"SVGPU_BA_TRACE", "2"}}).trace == 2 && parse({{"SVGPU_BA_TRACE", "21"}}).trace == 2 && parse({{"SVGPU_BA_TRACE", "12"}}).trace == 1);

    // the clamps at their edges
    CHECK(parse({{"SVGPU_BA_TEAM_MIN_OBS", "63"}}).team_min_obs == 64 && parse({{"SVGPU_BA_TEAM_MIN_OBS", "-5"}}).team_min_obs == 64 && parse({{"SVGPU_BA_TEAM_MIN_OBS", "64"}}).team_min_obs == 64);
    CHECK(parse({{"SVGPU_BA_TEAM_MIN_OBS", "65"}}).team_min_obs == 65 && parse({{"SVGPU_BA_TEAM_MIN_OBS", "x"}}).team_min_obs == 64);
    CHECK(parse({{"SVGPU_BA_SHARE_PAIRS", "63"}}).proc.share_pairs == 192 && parse({{"SVGPU_BA_SHARE_PAIRS", "64"}}).proc.share_pairs == 64);
    CHECK(parse({{"SVGPU_BA_SHARE_PAIRS", "0"}}).proc.share_pairs == 192 && parse({{"SVGPU_BA_SHARE_PAIRS", "1536"}}).proc.share_pairs == 1536);
    CHECK(parse({{"SVGPU_BA_CHUNK_SHIFT", "-1"}}).chunk_shift == 0 && parse({{"SVGPU_BA_CHUNK_SHIFT", "31"}}).chunk_shift == 30);
    CHECK(parse({{"SVGPU_BA_CHUNK_SHIFT", "0"}}).chunk_shift == 0 && parse({{"SVGPU_BA_CHUNK_SHIFT", "30"}}).chunk_shift == 30 && parse({{"SVGPU_BA_CHUNK_SHIFT", "6"}}).chunk_shift == 6);
    CHECK(parse({{"SVGPU_BA_UNITS_MIN", "0"}}).units_min == 1 && parse({{"SVGPU_BA_UNITS_MIN", "1"}}).units_min == 1 && parse({{"SVGPU_BA_UNITS_MIN", "-7"}}).units_min == 1);
    CHECK(parse({{"SVGPU_BA_UNITS_MIN", "100000"}}).units_min == 100000);
    // SVGPU_BA_HOST_THREADS is kept as requested; the plan function clamps it to 1 .. min(16, CPUs)
    const BaEnv t0 = parse({{"SVGPU_BA_HOST_THREADS", "0"}}), t99 = parse({{"SVGPU_BA_HOST_THREADS", "99"}}), t3 = parse({{"SVGPU_BA_HOST_THREADS", "3"}});
    CHECK(t0.host_threads == 0 && t99.host_threads == 99 && t3.host_threads == 3);
    CHECK(ba_plan_host_threads(true, t0, 4) == 1 && ba_plan_host_threads(true, t99, 4) == 4 && ba_plan_host_threads(true, t3, 4) == 3 && ba_plan_host_threads(true, d, 4) == 4);
    CHECK(ba_plan_host_threads(true, t99, 64) == 16 && ba_plan_host_threads(true, t99, 0) == 16 && ba_plan_host_threads(true, d, 64) == 8 && ba_plan_host_threads(true, d, 0) == 8);
    CHECK(ba_plan_host_threads(false, t99, 64) == 1 && ba_plan_host_threads(false, d, 4) == 1);

    // SVGPU_BA_SOLVER: its six words, and an unknown one, which is ignored
    const std::vector<std::pair<const char*, int>> words = {{"cholesky", SVGPU_BA_SOLVER_CHOLESKY}, {"cholesky_mfma", SVGPU_BA_SOLVER_CHOLESKY_MFMA}, {"pcg", SVGPU_BA_SOLVER_PCG},
                                                            {"dense", SVGPU_BA_SOLVER_DENSE}, {"pcg_multi", SVGPU_BA_SOLVER_PCG_MULTI}, {"envelope", SVGPU_BA_SOLVER_ENVELOPE}};
    for (const auto& w : words) {
        const BaEnv e = parse({{"SVGPU_BA_SOLVER", w.first}});
        CHECK(e.solver == w.second);
        for (int ctx_solver : {0, 1, 2, 3, 4, 6, 7}) CHECK(ba_plan_solver_option(ctx_solver, e) == w.second);
    }
    for (const char* w : {"auto", "Cholesky", "pcg ", "", "6"}) {
        const BaEnv e = parse({{"SVGPU_BA_SOLVER", w}});
        CHECK(e.solver == BA_ENV_NOT_SET);
        for (int ctx_solver : {0, 1, 2, 3, 4, 6, 7}) CHECK(ba_plan_solver_option(ctx_solver, e) == ctx_solver);
    }
    CHECK(parse({{"SVGPU_BA_CHOL", "mfma"}}).proc.chol_mfma && !parse({{"SVGPU_BA_CHOL", "other"}}).proc.chol_mfma && !parse({{"SVGPU_BA_CHOL", ""}}).proc.chol_mfma);
    // SVGPU_BA_DBG plain, =schur, =chol: what ba_sizes is handed, and which kernel stamps
    const BaEnv g1 = parse({{"SVGPU_BA_DBG", "1"}}), gs = parse({{"SVGPU_BA_DBG", "schur"}}), gc = parse({{"SVGPU_BA_DBG", "chol"}});
    CHECK(g1.proc.dbg == BA_ENV_DBG_TAIL && gs.proc.dbg == BA_ENV_DBG_SCHUR && gc.proc.dbg == BA_ENV_DBG_CHOL && parse({{"SVGPU_BA_DBG", ""}}).proc.dbg == BA_ENV_DBG_TAIL);
    CHECK(ba_plan_dbg_mode(d) == BA_DBG_OFF && ba_plan_dbg_mode(g1) == BA_DBG_PER_LANDMARK && ba_plan_dbg_mode(gs) == BA_DBG_SCHUR && ba_plan_dbg_mode(gc) == BA_DBG_PER_LANDMARK);
    CHECK(ba_plan_dbg_kernel(d) == 0 && ba_plan_dbg_kernel(g1) == 0 && ba_plan_dbg_kernel(gs) == 1 && ba_plan_dbg_kernel(gc) == 2);
    CHECK(parse({{"SVGPU_BA_EXCHANGE", "full"}}).exchange_full && !parse({{"SVGPU_BA_EXCHANGE", "segments"}}).exchange_full && !parse({{"SVGPU_BA_EXCHANGE", ""}}).exchange_full);
    CHECK(parse({{"SVGPU_BA_SCHUR_ORDER", "0"}}).schur_order == 0 && parse({{"SVGPU_BA_SCHUR_ORDER", "1"}}).schur_order == 1 && parse({{"SVGPU_BA_SCHUR_ORDER", "7"}}).schur_order == 1);
    CHECK(parse({{"SVGPU_BA_SCHUR_ORDER", "x"}}).schur_order == 0);
    CHECK(parse({{"SVGPU_SKY_SEGMENTS", "0"}}).sky_segments == 0 && parse({{"SVGPU_SKY_SEGMENTS", "5"}}).sky_segments == 5 && parse({{"SVGPU_SKY_SEGMENTS", "-1"}}).sky_segments == -1);
    std::printf("ok parse: %zu switches\n", all.size());
}

// ---- the expressions as the driver, the launchers and the envelope planner held them before ba_plan.h, restated on a table
struct Old {
    const Table& t;
    const char* get(const char* name) const {
        const auto it = t.find(name);
        return it == t.end() ? nullptr : it->second.c_str();
    }
    bool team_sized(int E) const {
        const char* ev = get("SVGPU_BA_TEAM_MIN_OBS");
        const int team_min_obs = ev ? std::max(64, std::atoi(ev)) : 400000;
        return E >= team_min_obs && !get("SVGPU_BA_ONE_THREAD");
    }
    int nth(bool team_sized, unsigned hw) const {
        if (!team_sized) return 1;
        const char* ev = get("SVGPU_BA_HOST_THREADS");
        const int v = ev ? std::atoi(ev) : 8;
        const int cap = hw == 0 ? 16 : (int)std::min(16u, hw);
        return v < 1 ? 1 : (v > cap ? cap : v);
    }
    int solver_opt(int ctx_solver) const {
        int solver_opt = ctx_solver;
        if (const char* ev = get("SVGPU_BA_SOLVER")) {
            if (!strcmp(ev, "cholesky")) solver_opt = SV_BA_SOLVER_CHOLESKY;
            else if (!strcmp(ev, "cholesky_mfma")) solver_opt = SV_BA_SOLVER_CHOLESKY_MFMA;
            else if (!strcmp(ev, "pcg")) solver_opt = SV_BA_SOLVER_PCG;
            else if (!strcmp(ev, "dense")) solver_opt = SV_BA_SOLVER_DENSE;
            else if (!strcmp(ev, "pcg_multi")) solver_opt = SV_BA_SOLVER_PCG_MULTI;
            else if (!strcmp(ev, "envelope")) solver_opt = SV_BA_SOLVER_ENVELOPE;
        }
        return solver_opt;
    }
    bool want_dense(int solver_opt, bool sharded, int P) const {
        return solver_opt == SV_BA_SOLVER_DENSE || (solver_opt == SV_BA_SOLVER_AUTO && !sharded && P >= 24 && P <= 256 && !get("SVGPU_BA_NO_DENSE_TILED"));
    }
    bool renumber(bool team_running, bool single_stage) const { return team_running && single_stage && !get("SVGPU_BA_NO_RENUMBER"); }
    int nshare(size_t num_pairs, int NB) const {
        const char* e = get("SVGPU_BA_SHARE_PAIRS");
        const long v = e ? std::atol(e) : 0;
        const size_t share_pairs = (size_t)(v >= 64 ? v : 192);
        int nshare = NB > 0 ? (int)std::min<size_t>(16, std::max<size_t>(1, (num_pairs / (size_t)NB + share_pairs - 1) / share_pairs)) : 1;
        if (NB > 0) {
            const size_t avg = num_pairs / (size_t)NB, ns_max = std::min<size_t>(16, std::max<size_t>(1, (avg + 63) / 64));
            while ((size_t)nshare < ns_max && (size_t)NB * (nshare + 1) <= 2304) ++nshare;
        }
        return nshare;
    }
    bool units(bool chunk_units, int nP, int NB, int nshare, size_t num_pairs) const {
        const char* ev = get("SVGPU_BA_UNITS_MIN");
        const size_t units_min = ev ? (size_t)std::max(1, std::atoi(ev)) : (size_t)8192;
        return chunk_units && nP > 48 && (size_t)NB * nshare >= units_min && num_pairs > 0;
    }
    int chunk_shift(int E, int L) const {
        int shift = 4;
        while (((size_t)2 << shift) * 144 * ((size_t)E / (size_t)std::max(L, 1) + 1) <= ((size_t)1 << 19)) ++shift;
        if (const char* ev = get("SVGPU_BA_CHUNK_SHIFT")) shift = std::max(0, std::min(30, std::atoi(ev)));
        return shift;
    }
    int schur_large(int n_schur) const {
        int large = n_schur >= 8192;
        const char* const order_env = get("SVGPU_BA_SCHUR_ORDER");
        if (order_env) large = std::atoi(order_env) != 0;
        return large;
    }
    // the cascade of upload_structure; *asked: sv_sky_plan's verdict was consulted
    int solver(int solver_opt, bool chol_in_lds, bool S, int n, int NB, int nP, bool lds_ok, bool envelope_ok, bool* asked, int* chol_mfma) const {
        int solver = solver_opt;
        *chol_mfma = 0;
        *asked = false;
        if (solver == SV_BA_SOLVER_CHOLESKY_MFMA) {
            solver = SV_BA_SOLVER_CHOLESKY;
            *chol_mfma = 1;
        }
        if (solver == SV_BA_SOLVER_AUTO && chol_in_lds) solver = SV_BA_SOLVER_CHOLESKY;
        if (solver == SV_BA_SOLVER_CHOLESKY && !chol_in_lds) solver = SV_BA_SOLVER_AUTO;
        if (solver == SV_BA_SOLVER_AUTO && S && !chol_in_lds && n <= 1536 && (size_t)NB * 5 >= (size_t)nP * (nP + 1)) solver = SV_BA_SOLVER_DENSE;
        if ((solver == SV_BA_SOLVER_AUTO && !lds_ok) || solver == SV_BA_SOLVER_ENVELOPE) {
            *asked = true;
            solver = envelope_ok ? SV_BA_SOLVER_ENVELOPE : SV_BA_SOLVER_AUTO;
        }
        if (solver == SV_BA_SOLVER_AUTO || solver == SV_BA_SOLVER_PCG) solver = lds_ok ? SV_BA_SOLVER_PCG_LDS : SV_BA_SOLVER_PCG_MULTI;
        return solver;
    }
    bool sky_band(int wmax, int band_w, size_t n0, size_t n1) const { return wmax <= band_w && 3 * n1 <= 4 * n0 && !get("SVGPU_SKY_NO_BAND"); }
    bool sky_segments(bool band, int max_m, int nP, int* want) const {
        const char* ev = get("SVGPU_SKY_SEGMENTS");
        *want = ev ? std::atoi(ev) : -1;
        if (*want == 0 || get("SVGPU_SKY_ONE_SIDED") || !band || max_m < 1 || nP < 8 * (max_m + 1)) return false;
        return true;
    }
    bool sky_two_sided(int cus, bool band, int max_m, int nP) const { return cus >= 2 && band && max_m >= 1 && nP >= 8 * (max_m + 1) && !get("SVGPU_SKY_ONE_SIDED"); }
};

static void check_plan() {
    const std::vector<Table> tables = {{}, {{"SVGPU_BA_TEAM_MIN_OBS", "64"}, {"SVGPU_BA_UNITS_MIN", "1"}}, {{"SVGPU_BA_TEAM_MIN_OBS", "1000"}, {"SVGPU_BA_UNITS_MIN", "2300"}},
        {{"SVGPU_BA_ONE_THREAD", "1"}}, {{"SVGPU_BA_HOST_THREADS", "0"}}, {{"SVGPU_BA_HOST_THREADS", "3"}}, {{"SVGPU_BA_HOST_THREADS", "99"}},
        {{"SVGPU_BA_SOLVER", "cholesky"}}, {{"SVGPU_BA_SOLVER", "cholesky_mfma"}}, {{"SVGPU_BA_SOLVER", "pcg"}}, {{"SVGPU_BA_SOLVER", "dense"}}, {{"SVGPU_BA_SOLVER", "pcg_multi"}},
        {{"SVGPU_BA_SOLVER", "envelope"}}, {{"SVGPU_BA_SOLVER", "simplex"}}, {{"SVGPU_BA_NO_DENSE_TILED", "1"}}, {{"SVGPU_BA_NO_RENUMBER", "1"}}, {{"SVGPU_BA_NO_UNITS", "1"}},
        {{"SVGPU_BA_SHARE_PAIRS", "63"}}, {{"SVGPU_BA_SHARE_PAIRS", "64"}}, {{"SVGPU_BA_SHARE_PAIRS", "768"}}, {{"SVGPU_BA_UNITS_MIN", "0"}}, {{"SVGPU_BA_UNITS_MIN", "2304"}},
        {{"SVGPU_BA_CHUNK_SHIFT", "-1"}}, {{"SVGPU_BA_CHUNK_SHIFT", "6"}}, {{"SVGPU_BA_CHUNK_SHIFT", "31"}}, {{"SVGPU_BA_SCHUR_ORDER", "0"}}, {{"SVGPU_BA_SCHUR_ORDER", "1"}},
        {{"SVGPU_SKY_NO_BAND", "1"}}, {{"SVGPU_SKY_SEGMENTS", "0"}}, {{"SVGPU_SKY_SEGMENTS", "5"}}, {{"SVGPU_SKY_SEGMENTS", "-3"}}, {{"SVGPU_SKY_ONE_SIDED", "1"}},
        {{"SVGPU_SKY_ONE_SIDED", "1"}, {"SVGPU_SKY_NO_BAND", "1"}}, {{"SVGPU_SKY_SEGMENTS", "3"}, {"SVGPU_SKY_ONE_SIDED", "1"}}};
    const int solvers[] = {SV_BA_SOLVER_AUTO, SV_BA_SOLVER_CHOLESKY, SV_BA_SOLVER_PCG, SV_BA_SOLVER_DENSE, SV_BA_SOLVER_PCG_MULTI, SV_BA_SOLVER_ENVELOPE, SV_BA_SOLVER_CHOLESKY_MFMA};
    size_t compared = 0;
    for (const Table& t : tables) {
        const Old old{t};
        const BaEnv env = parse(t);
        // the host team
        for (int E : {0, 63, 64, 65, 999, 1000, 60000, 399999, 400000, 400001, 1200000, 9600000}) {
            CHECK(ba_plan_team_sized(E, env) == old.team_sized(E));
            for (unsigned hw : {0u, 1u, 2u, 4u, 8u, 15u, 16u, 17u, 256u})
                for (bool sized : {false, true}) { CHECK(ba_plan_host_threads(sized, env, hw) == old.nth(sized, hw)); ++compared; }
        }
        // what the arena is sized for
        for (int ctx_solver : solvers) {
            const int so = old.solver_opt(ctx_solver);
            CHECK(ba_plan_solver_option(ctx_solver, env) == so);
            for (int P : {1, 20, 23, 24, 25, 100, 255, 256, 257, 500})
                for (bool sharded : {false, true}) { CHECK(ba_plan_want_dense(so, sharded, P, env) == old.want_dense(so, sharded, P)); ++compared; }
        }
        for (int k = 0; k < 4; ++k) CHECK(ba_plan_renumber(k & 1, k & 2, env) == old.renumber(k & 1, k & 2));
        // shares per block and units.  NB * nshare around 2304 (the resident round) and around units_min (1, 2300, 2304, 8192 in the tables);
        // nP 48 / 49 (the local-BA sizes keep the arithmetic shares)
        for (int NB : {0, 1, 2, 135, 136, 137, 143, 144, 145, 153, 154, 164, 165, 176, 177, 192, 209, 210, 256, 287, 288, 289, 328, 329, 383, 384, 385, 511, 512, 513, 575, 576, 577, 767, 768,
                       769, 1151, 1152, 1153, 1175, 1176, 1177, 2299, 2300, 2301, 2303, 2304, 2305, 4095, 4096, 4097, 8191, 8192, 8193, 9949, 125250})
            for (size_t per_block : {0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 383, 384, 385, 448, 449, 1000, 2637, 3071, 3072, 3073, 100000})
                for (size_t extra : {(size_t)0, (size_t)NB / 2}) {
                    const size_t num_pairs = per_block * (size_t)NB + extra;
                    const int ns = old.nshare(num_pairs, NB);
                    CHECK(ba_plan_nshare(num_pairs, NB, env) == ns);
                    CHECK(ns >= 1 && ns <= 16);
                    ++compared;
                    for (int nP : {1, 48, 49, 500})
                        for (bool chunk_units : {false, true})
                            for (int nsh : {ns, 1, 16}) CHECK(ba_plan_units(chunk_units, nP, NB, nsh, num_pairs, env) == old.units(chunk_units, nP, NB, nsh, num_pairs));
                }
        // the chunk shift
        for (int L : {0, 1, 500, 10000, 200000, 1600000})
            for (int E : {0, 1, 2500, 59999, 60000, 399999, 400000, 1200000, 9600000, 29826160}) { CHECK(ba_plan_chunk_shift(E, L, env) == old.chunk_shift(E, L)); ++compared; }
        // the form of the Schur launch
        for (int n_schur : {0, 1, 952, 2304, 8191, 8192, 8193, 100000}) { CHECK((int)ba_plan_schur_large(n_schur, env) == old.schur_large(n_schur)); ++compared; }
        // the solver of a stage: n around 1536, the 40 % inequality 5 NB >= nP (nP + 1) on both sides of equality (nP = 4: 20 = 5 * 4;
        // nP = 24: 600 = 5 * 120; nP = 255 / 256 / 257: n = 1530 / 1536 / 1542)
        for (int ctx_solver : solvers)
            for (int nP : {1, 4, 22, 23, 24, 31, 48, 49, 86, 255, 256, 257, 500}) {
                const int full = nP * (nP + 1) / 2, eq = (nP * (nP + 1) + 4) / 5;
                for (int NB : {nP, eq - 1, eq, eq + 1, full})
                    for (int flags = 0; flags < 16; ++flags) {
                        const bool chol_in_lds = flags & 1, S = flags & 2, lds_ok = flags & 4, envelope_ok = flags & 8;
                        const int so = old.solver_opt(ctx_solver), n = 6 * nP;
                        bool asked = false;
                        int mfma = 0;
                        const int want = old.solver(so, chol_in_lds, S, n, NB, nP, lds_ok, envelope_ok, &asked, &mfma);
                        const BaSolverFront F = ba_plan_solver_front(so, chol_in_lds, S, n, NB, nP, lds_ok);
                        CHECK(F.ask_envelope == asked && ba_plan_solver_final(F, envelope_ok, lds_ok) == want);
                        CHECK(mfma == (so == SV_BA_SOLVER_CHOLESKY_MFMA));  // (the driver sets BaDev::chol_mfma from the option itself)
                        ++compared;
                    }
            }
        // the gates of the envelope planner: nP against 8 (max_m + 1) on both sides, the band's width and growth at their limits
        for (int max_m : {0, 1, 7, 11, 16, 200})
            for (int nP : {1, 15, 16, 17, 63, 64, 65, 95, 96, 97, 135, 136, 137, 500, 1607, 1608, 1609})
                for (bool band : {false, true}) {
                    int w0 = 12345, w1 = 54321;
                    const bool a = ba_plan_sky_segments(band, max_m, nP, env, &w0), b = old.sky_segments(band, max_m, nP, &w1);
                    CHECK(a == b && w0 == w1);
                    for (int cus : {0, 1, 2, 256}) { CHECK(ba_plan_sky_two_sided(cus, band, max_m, nP, env) == old.sky_two_sided(cus, band, max_m, nP)); ++compared; }
                }
        for (int wmax : {0, 15, 16, 17})
            for (size_t n0 : {1, 3, 299, 300, 301, 1000000})
                for (size_t n1 : {n0, n0 * 4 / 3 - 1, n0 * 4 / 3, n0 * 4 / 3 + 1, 2 * n0}) { CHECK(ba_plan_sky_band(wmax, 16, n0, n1, env) == old.sky_band(wmax, 16, n0, n1)); ++compared; }
    }
    std::printf("ok plan functions against their restatement: %zu environments, %zu comparisons\n", tables.size(), compared);
}

// The bench shapes.  Pairs and blocks are what the driver's trace (SVGPU_BA_TRACE=1, the "structure rebuilt" and "chunk-major units"
// lines) printed for bench.py's scenes on an MI355X at the commit before ba_plan.h existed; the shares follow from them by the expression
// of that commit, worked out by hand beside each literal.
static void check_bench_shapes() {
    const BaEnv d = parse({});
    // "structure rebuilt (360000 pairs, 136 blocks, n = 96, solver 1)"
    const size_t CONFIG3_PAIRS = 360000;
    const int CONFIG3_BLOCKS = 136;
    // "chunk-major units: 11252 (chunks of 512 landmarks)", "structure rebuilt (4185570 pairs, 2989 blocks, n = 2994, solver 6)"
    //   4 185 570 / 2 989 = 1 400 pairs per block -> ceil(1 400 / 192) = 8 shares, and 2 989 x 9 is beyond the 2 304 of a resident round: 8
    const size_t CONFIG5_PAIRS = 4185570;
    const int CONFIG5_BLOCKS = 2989, CONFIG5_FREE_POSES = 499, CONFIG5_NSHARE = 8;
    // config 3, synthetic.ba_scene(seed=1234): 20 keyframes (16 free) / 10 000 landmarks / 60 000 observations through svgpu_local_ba.
    // Every upper block is kept: 136 blocks, and the pair count is the capacity, 6^2 per landmark = 360 000.
    //   360 000 / 136 = 2 647 pairs per block -> ceil(2 647 / 192) = 14 shares; up to min(16, ceil(2 647 / 64)) = 16 while 136 (s + 1) <= 2 304: 16
    CHECK(ba_plan_nshare(CONFIG3_PAIRS, CONFIG3_BLOCKS, d) == 16);
    CHECK(!ba_plan_units(false, 16, CONFIG3_BLOCKS, 16, CONFIG3_PAIRS, d) && !ba_plan_units(true, 16, CONFIG3_BLOCKS, 16, CONFIG3_PAIRS, d));  // (16 free poses: never units)
    CHECK(!ba_plan_schur_large(CONFIG3_BLOCKS * 16, d));  // 2 176 units: the small-system form
    CHECK(!ba_plan_team_sized(60000, d) && ba_plan_host_threads(false, d, 16) == 1);
    CHECK(!ba_plan_want_dense(SV_BA_SOLVER_AUTO, false, 20, d));
    // config 5, synthetic.ba_scene_large(): 500 keyframes / 200 000 landmarks / 1 200 000 observations through svgpu_global_ba
    CHECK(ba_plan_team_sized(1200000, d) && ba_plan_host_threads(true, d, 16) == 8);
    CHECK(ba_plan_nshare(CONFIG5_PAIRS, CONFIG5_BLOCKS, d) == CONFIG5_NSHARE);
    CHECK(ba_plan_units(true, CONFIG5_FREE_POSES, CONFIG5_BLOCKS, CONFIG5_NSHARE, CONFIG5_PAIRS, d));  // 23 912 shares >= 8 192
    CHECK(ba_plan_schur_large(CONFIG5_BLOCKS * CONFIG5_NSHARE, d));                                    // (the form its arithmetic shares would take)
    {
        const BaSolverFront F = ba_plan_solver_front(SV_BA_SOLVER_AUTO, false, false, 6 * CONFIG5_FREE_POSES, CONFIG5_BLOCKS, CONFIG5_FREE_POSES, false);
        CHECK(F.ask_envelope && ba_plan_solver_final(F, true, false) == SV_BA_SOLVER_ENVELOPE);  // "solver 6"
        const BaSolverFront F3 = ba_plan_solver_front(SV_BA_SOLVER_AUTO, true, false, 96, CONFIG3_BLOCKS, 16, true);
        CHECK(!F3.ask_envelope && ba_plan_solver_final(F3, false, true) == SV_BA_SOLVER_CHOLESKY);  // "solver 1"
    }
    CHECK(ba_plan_chunk_shift(1200000, 200000, d) == 9);  // "chunks of 512 landmarks"
    CHECK(ba_plan_chunk_shift(60000, 10000, d) == 9);     // (config 3 has the same 6 observations per landmark)
    std::printf("ok bench shapes\n");
}

static void check_cache_key() {
    const std::vector<Table> planner = {{}, {{"SVGPU_SKY_SEGMENTS", "0"}}, {{"SVGPU_SKY_SEGMENTS", "5"}}, {{"SVGPU_SKY_ONE_SIDED", "1"}}, {{"SVGPU_SKY_NO_BAND", "1"}},
                                        {{"SVGPU_SKY_ONE_SIDED", "1"}, {"SVGPU_SKY_NO_BAND", "1"}}};
    for (size_t i = 0; i < planner.size(); ++i)
        for (size_t j = 0; j < planner.size(); ++j) CHECK((ba_plan_sky_env_key(parse(planner[i])) == ba_plan_sky_env_key(parse(planner[j]))) == (i == j));
    // what the planner does not read leaves the key alone
    const Table others = {{"SVGPU_BA_TRACE", "1"}, {"SVGPU_BA_HOST_THREADS", "3"}, {"SVGPU_BA_SOLVER", "envelope"}, {"SVGPU_BA_SCHUR_ORDER", "1"}, {"SVGPU_BA_DBG", "schur"},
                          {"SVGPU_BA_TEAM_MIN_OBS", "64"}, {"SVGPU_BA_UNITS_MIN", "1"}, {"SVGPU_BA_EXCHANGE", "full"}};
    for (const Table& t : planner) {
        Table with = t;
        with.insert(others.begin(), others.end());
        CHECK(ba_plan_sky_env_key(parse(with)) == ba_plan_sky_env_key(parse(t)));
    }
    std::printf("ok cache key: %zu planner environments\n", planner.size());
}

int main() {
    check_parse();
    check_plan();
    check_bench_shapes();
    check_cache_key();
    return layout_check_result("ba plan ok");
}
