// Host-side plan of bundle adjustment: the environment switches as values, and the decisions of local_ba_impl (svgpu_ba.hip), of the
// launchers at the end of ba_kernels.hip and of the envelope planner (ba_skyline.hip) that choose which kernels run and how their launches
// are sized.  Every decision is integer arithmetic on a handful of sizes.  Plain C++17 with no HIP include; nothing in this header reads
// the environment (svgpu_ba.hip ba_env() does, tests/ba_plan_check.cpp feeds ba_env_parse a table).
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdlib>
#include <cstring>

#include "ba_layout.h"  // BA_DBG_*
#include "svgpu.h"      // svgpu_ba_solver

// svgpu_ba_solver and the forms only the driver knows
enum {
    SV_BA_SOLVER_AUTO = SVGPU_BA_SOLVER_AUTO, SV_BA_SOLVER_CHOLESKY = SVGPU_BA_SOLVER_CHOLESKY, SV_BA_SOLVER_PCG = SVGPU_BA_SOLVER_PCG, SV_BA_SOLVER_DENSE = SVGPU_BA_SOLVER_DENSE,
    SV_BA_SOLVER_PCG_MULTI = SVGPU_BA_SOLVER_PCG_MULTI, SV_BA_SOLVER_PCG_LDS = 5 /* internal: the PCG inside one workgroup's LDS */,
    SV_BA_SOLVER_ENVELOPE = SVGPU_BA_SOLVER_ENVELOPE, SV_BA_SOLVER_CHOLESKY_MFMA = SVGPU_BA_SOLVER_CHOLESKY_MFMA
};

#define BA_ENV_NOT_SET INT_MIN  // an integer switch that is absent from the environment

enum { BA_ENV_DBG_OFF = 0, BA_ENV_DBG_TAIL = 1, BA_ENV_DBG_SCHUR = 2, BA_ENV_DBG_CHOL = 3 };  // SVGPU_BA_DBG: unset | set | "schur" | "chol"

// The switches of bundle adjustment, parsed.  Each comment is the switch's one definition.  "set" means present in the environment, whatever
// the value.
struct BaEnv {
    // ---- process: the first value read holds for the life of the process (ba_env() keeps it)
    struct Process {
        int dbg = BA_ENV_DBG_OFF;      // SVGPU_BA_DBG: device time stamps, printed after the first stage.  Set: 8 per landmark-side workgroup of the last
                                       // fused tail; "schur": 8 per unit of the last k_ba_schur_rhs; "chol": phase stamps of the last k_ba_chol_mfma.  Default off
        size_t share_pairs = 192;      // SVGPU_BA_SHARE_PAIRS: tuning aid, pairs per share of a block of the reduced system.  Default 192; a value below 64
                                       // is ignored (the partial-sum buffer is sized for shares of at least 64 pairs)
        bool no_fusion = false;        // SVGPU_BA_NO_FUSION set: A/B aid, update and chi2 as separate kernels instead of the fused tail
        bool lin_two_launches = false; // SVGPU_BA_LIN_TWO_LAUNCHES set: profiling aid, the two sides of the linearisation in a launch each
        bool chol_mfma = false;        // SVGPU_BA_CHOL=mfma: A/B aid, the on-chip dense solve takes the blocked MFMA factorisation; any other value: off
        bool dense_one_wg = false;     // SVGPU_BA_DENSE_ONE_WG set: A/B aid, solver = dense takes the one-workgroup column-by-column form
    } proc;
    // ---- call: read once at the entry of every call (the tests switch these between calls)
    int trace = 0;                     // SVGPU_BA_TRACE: 0 unset; 1 set: host phase times and the chosen plan to stderr; 2 (value begins with '2'):
                                       // also one step per read-back, printed
    int team_min_obs = 400000;         // SVGPU_BA_TEAM_MIN_OBS: observations from which the host team sets the call up.  Default 400 000; floored at 64
    bool one_thread = false;           // SVGPU_BA_ONE_THREAD set: never the host team
    int host_threads = 8;              // SVGPU_BA_HOST_THREADS: threads of the team, as requested.  Default 8; ba_plan_host_threads clamps to 1 .. min(16, CPUs)
    int solver = BA_ENV_NOT_SET;       // SVGPU_BA_SOLVER: cholesky | cholesky_mfma | pcg | dense | pcg_multi | envelope, as its svgpu_ba_solver value, overrides
                                       // svgpu_ba_set_solver; any other word is ignored
    bool no_dense_tiled = false;       // SVGPU_BA_NO_DENSE_TILED set: AUTO does not consider the tiled dense LL^T
    bool no_renumber = false;          // SVGPU_BA_NO_RENUMBER set: the solve keeps the caller's landmark numbering
    bool no_units = false;             // SVGPU_BA_NO_UNITS set: arithmetic shares only, no chunk-major units
    bool copy_on_main = false;         // SVGPU_BA_COPY_ON_MAIN set: the team uploads the measurements on the solve's own stream
    size_t units_min = 8192;           // SVGPU_BA_UNITS_MIN: arithmetic shares below this many (blocks x shares).  Default 8192; floored at 1
    int chunk_shift = BA_ENV_NOT_SET;  // SVGPU_BA_CHUNK_SHIFT: a chunk of units = 2^shift landmarks, clamped to 0 .. 30.  Default: ba_plan_chunk_shift's own
    bool exchange_full = false;        // SVGPU_BA_EXCHANGE=full: a sharded solve sums the whole reduced system even where keyframe segments apply
    bool host_boundary = false;        // SVGPU_BA_HOST_BOUNDARY set: A/B aid, the stage boundary always comes back to the host
    int schur_order = BA_ENV_NOT_SET;  // SVGPU_BA_SCHUR_ORDER: 0 = the small-system form of the Schur launch, any other number = the large-system form.
                                       // Default: by size (ba_plan_schur_large)
    bool sky_no_band = false;          // SVGPU_SKY_NO_BAND set: no envelope is widened to a band (the general kernel factors it)
    int sky_segments = BA_ENV_NOT_SET; // SVGPU_SKY_SEGMENTS: 0 = no segmented elimination, n > 0 = exactly n cuts.  Default (and n < 0): 2 .. 8 cuts by the cost model
    bool sky_one_sided = false;        // SVGPU_SKY_ONE_SIDED set: neither the segmented nor the two-sided elimination
};

// lookup: any callable const char*(const char*), null for a name that is not set.  Pure: the same table gives the same BaEnv.
template <class Lookup>
BaEnv ba_env_parse(Lookup&& lookup) {
    BaEnv e;
    const auto is_set = [&](const char* name) { return lookup(name) != nullptr; };
    const auto is_word = [&](const char* name, const char* word) {
        const char* v = lookup(name);
        return v && !strcmp(v, word);
    };
    e.proc.dbg = !is_set("SVGPU_BA_DBG") ? BA_ENV_DBG_OFF : is_word("SVGPU_BA_DBG", "schur") ? BA_ENV_DBG_SCHUR : is_word("SVGPU_BA_DBG", "chol") ? BA_ENV_DBG_CHOL : BA_ENV_DBG_TAIL;
    if (const char* v = lookup("SVGPU_BA_SHARE_PAIRS")) {
        const long n = std::atol(v);
        if (n >= 64) e.proc.share_pairs = (size_t)n;
    }
    e.proc.no_fusion = is_set("SVGPU_BA_NO_FUSION");
    e.proc.lin_two_launches = is_set("SVGPU_BA_LIN_TWO_LAUNCHES");
    e.proc.chol_mfma = is_word("SVGPU_BA_CHOL", "mfma");
    e.proc.dense_one_wg = is_set("SVGPU_BA_DENSE_ONE_WG");

    if (const char* v = lookup("SVGPU_BA_TRACE")) e.trace = v[0] == '2' ? 2 : 1;
    if (const char* v = lookup("SVGPU_BA_TEAM_MIN_OBS")) e.team_min_obs = std::max(64, std::atoi(v));
    e.one_thread = is_set("SVGPU_BA_ONE_THREAD");
    if (const char* v = lookup("SVGPU_BA_HOST_THREADS")) e.host_threads = std::atoi(v);
    if (const char* v = lookup("SVGPU_BA_SOLVER")) {
        if (!strcmp(v, "cholesky")) e.solver = SV_BA_SOLVER_CHOLESKY;
        else if (!strcmp(v, "cholesky_mfma")) e.solver = SV_BA_SOLVER_CHOLESKY_MFMA;
        else if (!strcmp(v, "pcg")) e.solver = SV_BA_SOLVER_PCG;
        else if (!strcmp(v, "dense")) e.solver = SV_BA_SOLVER_DENSE;
        else if (!strcmp(v, "pcg_multi")) e.solver = SV_BA_SOLVER_PCG_MULTI;
        else if (!strcmp(v, "envelope")) e.solver = SV_BA_SOLVER_ENVELOPE;
    }
    e.no_dense_tiled = is_set("SVGPU_BA_NO_DENSE_TILED");
    e.no_renumber = is_set("SVGPU_BA_NO_RENUMBER");
    e.no_units = is_set("SVGPU_BA_NO_UNITS");
    e.copy_on_main = is_set("SVGPU_BA_COPY_ON_MAIN");
    if (const char* v = lookup("SVGPU_BA_UNITS_MIN")) e.units_min = (size_t)std::max(1, std::atoi(v));
    if (const char* v = lookup("SVGPU_BA_CHUNK_SHIFT")) e.chunk_shift = std::max(0, std::min(30, std::atoi(v)));
    e.exchange_full = is_word("SVGPU_BA_EXCHANGE", "full");
    e.host_boundary = is_set("SVGPU_BA_HOST_BOUNDARY");
    if (const char* v = lookup("SVGPU_BA_SCHUR_ORDER")) e.schur_order = std::atoi(v) != 0;
    e.sky_no_band = is_set("SVGPU_SKY_NO_BAND");
    if (const char* v = lookup("SVGPU_SKY_SEGMENTS")) e.sky_segments = std::atoi(v);
    e.sky_one_sided = is_set("SVGPU_SKY_ONE_SIDED");
    return e;
}

// ---- the host team of a global-BA sized call
inline bool ba_plan_team_sized(int E, const BaEnv& env) { return E >= env.team_min_obs && !env.one_thread; }
// threads of the staging pass (config 5: 1.28 ms with 4 threads, 0.69 with 8, flat beyond).  The team spins at its barriers: never more
// threads than `cpus`, the CPUs this process may run on (0: not known)
inline int ba_plan_host_threads(bool team_sized, const BaEnv& env, unsigned cpus) {
    if (!team_sized) return 1;
    const int cap = cpus == 0 ? 16 : (int)std::min(16u, cpus);
    return env.host_threads < 1 ? 1 : (env.host_threads > cap ? cap : env.host_threads);
}

// ---- what the arena is sized for
inline int ba_plan_solver_option(int ctx_solver, const BaEnv& env) { return env.solver != BA_ENV_NOT_SET ? env.solver : ctx_solver; }
// the dense matrix of the tiled LL^T (ba_dense_tiled.hip): on request, and as a candidate of AUTO for windows of 24 - 256 keyframes on one rank
inline bool ba_plan_want_dense(int solver_opt, bool sharded, int P, const BaEnv& env) {
    return solver_opt == SV_BA_SOLVER_DENSE || (solver_opt == SV_BA_SOLVER_AUTO && !sharded && P >= 24 && P <= 256 && !env.no_dense_tiled);
}
// the solve's own landmark numbering (ba_pairs.hip): one stage, the host team's sizes, observations grouped by landmark
inline bool ba_plan_renumber(bool team_running, bool single_stage, const BaEnv& env) { return team_running && single_stage && !env.no_renumber; }
inline int ba_plan_dbg_mode(const BaEnv& env) {  // the BA_DBG_* handed to ba_sizes
    return env.proc.dbg == BA_ENV_DBG_SCHUR ? BA_DBG_SCHUR : (env.proc.dbg != BA_ENV_DBG_OFF ? BA_DBG_PER_LANDMARK : BA_DBG_OFF);
}
inline int ba_plan_dbg_kernel(const BaEnv& env) {  // BaDev::dbg_schur_on: which kernel writes the stamps (0: the fused tail)
    return env.proc.dbg == BA_ENV_DBG_SCHUR ? 1 : (env.proc.dbg == BA_ENV_DBG_CHOL ? 2 : 0);
}

// ---- the Schur launch
// shares per block: ~192 pairs per wave (3 per lane); fewer, longer walks are slower (a lane's pairs are a chain of dependent loads),
// measured 2.30 / 2.31 / 2.43 / 2.90 / 3.79 ms per config-3 call at 96 / 192 / 384 / 768 / 1536 pairs per wave.
// A small system does not fill the chip with ~192-pair shares (config 3: 136 blocks x 7 shares for 1 792 unit slots): its shares shrink
// down to one trip of a wave (64 pairs) while the units still fit one resident round -- 17.7 -> 13.4 us per launch there; a large
// system keeps the long shares (config 5 at 64 pairs per share: 314 us instead of 189)
inline int ba_plan_nshare(size_t num_pairs, int NB, const BaEnv& env) {
    if (NB <= 0) return 1;
    const size_t share_pairs = env.proc.share_pairs, avg = num_pairs / (size_t)NB;
    int nshare = (int)std::min<size_t>(16, std::max<size_t>(1, (avg + share_pairs - 1) / share_pairs));
    const size_t ns_max = std::min<size_t>(16, std::max<size_t>(1, (avg + 63) / 64));
    while ((size_t)nshare < ns_max && (size_t)NB * (nshare + 1) <= 2304) ++nshare;
    return nshare;
}
// chunk-major units instead of the arithmetic shares: where the layout holds them, beyond the local-BA sizes, from units_min shares on
inline bool ba_plan_units(bool chunk_units, int nP, int NB, int nshare, size_t num_pairs, const BaEnv& env) {
    return chunk_units && nP > 48 && (size_t)NB * nshare >= env.units_min && num_pairs > 0;
}
// ~0.5 MB of W records per chunk of consecutive landmark ranks (chunk = 2^shift landmarks).  Measured, Schur launch at config 5 / 9.6 M
// observations: 256 landmarks 125 / 930 us, 512: 122 / 880, 1 024: 132 / 882, 2 048: 158 / 973; arithmetic shares 144 / 1 537
inline int ba_plan_chunk_shift(int E, int L, const BaEnv& env) {
    if (env.chunk_shift != BA_ENV_NOT_SET) return env.chunk_shift;
    int shift = 4;
    while (((size_t)2 << shift) * 144 * ((size_t)E / (size_t)std::max(L, 1) + 1) <= ((size_t)1 << 19)) ++shift;
    return shift;
}
// A large system (more than one resident round of units, n_schur = blocks x shares): XCD-contiguous unit order, right-hand side summed by
// the shares of the diagonal blocks.  A small one (local BA) leaves the chip part-filled: the right-hand side runs beside the blocks as
// units of its own, which also leaves the observation arrays warm for the next linearisation (folded there: k_ba_schur_rhs 13.3 -> 13.6 us,
// k_ba_lin 11.8 -> 13.0 us).
inline bool ba_plan_schur_large(int n_schur, const BaEnv& env) { return env.schur_order != BA_ENV_NOT_SET ? env.schur_order != 0 : n_schur >= 8192; }

// ---- the solver of a stage, in two steps around the envelope plan (sv_sky_plan)
struct BaSolverFront {
    int solver;         // the choice so far (CHOLESKY_MFMA counts as CHOLESKY: the same dense on-chip solve, its MFMA form)
    bool ask_envelope;  // the envelope plan decides: ba_plan_solver_final needs envelope_ok
};
// solver_opt: ba_plan_solver_option; chol_in_lds: the register-tile LL^T fits LDS; dense_matrix: the arena holds the dense image
// (ba_plan_want_dense); n = 6 nP unknowns, NB kept upper blocks; lds_ok: the LDS-resident PCG fits.
// AUTO: dense LL^T in LDS while it fits (n <= ~135: 70 us per trial against 88 us for the LDS-resident PCG at n = 96), the LDS-resident PCG
// up to 512 unknowns / ~150 KB of blocks, the one-launch-per-iteration PCG beyond.
// Beyond one workgroup's LDS, a window whose block pattern is close to full (every keyframe of a local window shares landmarks with most
// others): the tiled dense LL^T -- 2 launches per 48 columns, MFMA updates.  Measured per damping trial, auto before / tiled: see DESIGN
// section 6 (windows of 40 - 100 keyframes).  (From where the register-tile solve no longer fits LDS -- n = 138: per trial 232 us at
// n = 156 against 386 for the LDS-resident PCG AUTO took there and 282 for the envelope factorisation; at n = 132, where the register-tile
// solve still fits, the two tie at ~200 us.)
// Beyond the on-chip solvers: the direct envelope factorisation while the envelope of the ordered block graph is small (keyframe graphs
// are banded up to a few loop-closure rows), else -- or on request -- the PCG with one launch per iteration.
inline BaSolverFront ba_plan_solver_front(int solver_opt, bool chol_in_lds, bool dense_matrix, int n, int NB, int nP, bool lds_ok) {
    BaSolverFront F{solver_opt == SV_BA_SOLVER_CHOLESKY_MFMA ? (int)SV_BA_SOLVER_CHOLESKY : solver_opt, false};
    if (F.solver == SV_BA_SOLVER_AUTO && chol_in_lds) F.solver = SV_BA_SOLVER_CHOLESKY;
    if (F.solver == SV_BA_SOLVER_CHOLESKY && !chol_in_lds) F.solver = SV_BA_SOLVER_AUTO;
    if (F.solver == SV_BA_SOLVER_AUTO && dense_matrix && !chol_in_lds && n <= 1536 && (size_t)NB * 5 >= (size_t)nP * (nP + 1)) F.solver = SV_BA_SOLVER_DENSE;  // >= 40 % of the upper blocks kept
    F.ask_envelope = (F.solver == SV_BA_SOLVER_AUTO && !lds_ok) || F.solver == SV_BA_SOLVER_ENVELOPE;
    return F;
}
inline int ba_plan_solver_final(const BaSolverFront& F, bool envelope_ok, bool lds_ok) {
    int solver = F.solver;
    if (F.ask_envelope) solver = envelope_ok ? SV_BA_SOLVER_ENVELOPE : SV_BA_SOLVER_AUTO;
    if (solver == SV_BA_SOLVER_AUTO || solver == SV_BA_SOLVER_PCG) solver = lds_ok ? SV_BA_SOLVER_PCG_LDS : SV_BA_SOLVER_PCG_MULTI;
    return solver;
}

// ---- the gates of the envelope planner (ba_skyline.hip)
// A non-decreasing first[] makes the rows of every column contiguous (the banded kernel, bands up to band_w wide); taking the suffix
// minimum only adds blocks, so it is kept when the envelope grows by less than a third (n0 -> n1 blocks) and stays narrow (wmax).
inline bool ba_plan_sky_band(int wmax, int band_w, size_t n0, size_t n1, const BaEnv& env) { return wmax <= band_w && 3 * n1 <= 4 * n0 && !env.sky_no_band; }
// segmented elimination of a banded one-piece plan (nP block rows, widest column max_m): attempted when the band is long enough and nothing
// switches it off; *want > 0 forces that many cuts
inline bool ba_plan_sky_segments(bool band, int max_m, int nP, const BaEnv& env, int* want) {
    *want = env.sky_segments != BA_ENV_NOT_SET ? env.sky_segments : -1;
    return !(*want == 0 || env.sky_one_sided || !band || max_m < 1 || nP < 8 * (max_m + 1));
}
// two-sided elimination, the fallback when the segmented plan does not apply.  Its two workgroups wait for each other on flags, so both
// must be resident at once: any device with at least two compute units -- a device restricted below that keeps the one-sided sweep.
inline bool ba_plan_sky_two_sided(int cus, bool band, int max_m, int nP, const BaEnv& env) {
    return cus >= 2 && band && max_m >= 1 && nP >= 8 * (max_m + 1) && !env.sky_one_sided;
}
// what of the environment a cached envelope plan depends on: two environments that plan differently have different keys (the key lives
// only inside a process)
inline unsigned long long ba_plan_sky_env_key(const BaEnv& env) {
    return ((unsigned long long)(unsigned)env.sky_segments << 2) | (env.sky_one_sided ? 2u : 0u) | (env.sky_no_band ? 1u : 0u);
}
