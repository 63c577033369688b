// Host side of local bundle adjustment: problem flattening, structure (CSR) construction, and the
// Levenberg-Marquardt control flow of g2o restated around the device kernels.
//   two-stage schedule                 optimize/local_bundle_adjuster_g2o.cc:306-348
//   OptimizationAlgorithmLevenberg     g2o (pinned 20230223_git): lambda init 1e-5 * max diag, rho test, 10 trials
//   terminate_action                   optimize/terminate_action.cc:36-76 (writes through the force-stop pointer)
#include <algorithm>
#include <cfloat>
#include <cmath>

#include <chrono>
#include <cstdlib>
#include <dlfcn.h>
#include <thread>

#include "svgpu_internal.h"
#include "ba_kernels.h"
#include "ba_layout.h"
#include "ba_stage.h"
#include "poseopt_batch_layout.h"
#include "sv_staged_call.h"
#include "sv_validate.h"

// The switches of bundle adjustment as this call sees them (ba_plan.h).  The only reader of the environment in the bundle-adjustment
// sources: every entry point calls it once, at its entry.  The process-wide switches keep the first value read.
BaEnv ba_env() {
    BaEnv env = ba_env_parse(std::getenv);
    static const BaEnv::Process first = env.proc;
    env.proc = first;
    return env;
}

namespace {

struct HostStructure {
    std::vector<int> pose_slot, slot_pose;
    std::vector<uint8_t> pt_free;
    std::vector<int> blk_off;
    std::vector<int2> blk_ab;
    bool envelope_ok = false;  // the envelope Cholesky has a plan for this block pattern
    size_t num_pairs = 0;  // the pairs themselves live on the device only
    int nP = 0, nL = 0;
};

// pose / landmark activity under the current edge levels (the cheap first half of build_structure)
// (no_levels: no edge is excluded yet -- the first stage of a call: the poses with an observation were marked by the staging pass and a
//  landmark is active when its edge range is not empty; saves a pass over all observations, ~0.5 ms of a config-5 call)
void activity_only(const svgpu_ba_problem& pr, const int* e_pose, const int* e_point,
                   const std::vector<uint8_t>& level, const std::vector<uint8_t>* pose_active_global, HostStructure& H,
                   const std::vector<uint8_t>* pose_seen_no_levels = nullptr, const int* lm_off = nullptr) {
    const int P = pr.num_poses, L = pr.num_points, E = pr.num_obs;
    std::vector<uint8_t> pa(P, 0), la(L, 0);
    if (pose_seen_no_levels && lm_off) {
        pa = *pose_seen_no_levels;
        for (int l = 0; l < L; ++l) la[l] = lm_off[l + 1] > lm_off[l];
    }
    else
        for (int e = 0; e < E; ++e)
            if (!level[e]) {
                pa[e_pose[e]] = 1;
                la[e_point[e]] = 1;
            }
    if (pose_active_global) pa = *pose_active_global;
    H.pose_slot.assign(P, -1);
    H.slot_pose.clear();
    for (int p = 0; p < P; ++p)
        if (pa[p] && !pr.pose_fixed[p]) {
            H.pose_slot[p] = (int)H.slot_pose.size();
            H.slot_pose.push_back(p);
        }
    H.nP = (int)H.slot_pose.size();
    H.pt_free.assign(L, 0);
    H.nL = 0;
    for (int l = 0; l < L; ++l)
        if (la[l] && !(pr.point_fixed && pr.point_fixed[l])) {
            H.pt_free[l] = 1;
            ++H.nL;
        }
}

// dense block offsets (from the device) -> kept blocks: every diagonal block (it carries Hpp + lambda I) and every non-empty
// off-diagonal block, in (a, b) order; the sorted pair array needs no compaction (empty blocks hold no pairs)
void compact_blocks(const std::vector<int>& dense_off, const std::vector<uint8_t>& present, HostStructure& H) {
    H.blk_ab.clear();
    H.blk_off.clear();
    size_t k = 0;
    for (int a = 0; a < H.nP; ++a)
        for (int b = a; b < H.nP; ++b, ++k)
            if (a == b || present[k]) {
                int2 ab;
                ab.x = a;
                ab.y = b;
                H.blk_ab.push_back(ab);
                H.blk_off.push_back(dense_off[k]);
            }
    H.blk_off.push_back(dense_off.empty() ? 0 : dense_off.back());
    H.num_pairs = (size_t)(dense_off.empty() ? 0 : dense_off.back());
}

}  // namespace

// ---- in-library collectives: RCCL resolved with dlopen on first use (no link-time dependency, nothing of Python in the data path)
namespace {
struct NcclId {
    char internal[128];  // ncclUniqueId (NCCL_UNIQUE_ID_BYTES)
};
struct Rccl {
    void* h = nullptr;
    int (*get_unique_id)(NcclId*) = nullptr;
    int (*comm_init_rank)(void**, int, NcclId, int) = nullptr;
    int (*comm_destroy)(void*) = nullptr;
    int (*all_reduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    const char* (*get_error_string)(int) = nullptr;
    bool tried = false, ok = false;
};
Rccl g_rccl;
bool rccl_ready() {
    if (g_rccl.tried) return g_rccl.ok;
    g_rccl.tried = true;
    // a process that already carries an RCCL (torch's) keeps using that copy
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
    for (const char* nm : names)
        if (!g_rccl.h) g_rccl.h = dlopen(nm, RTLD_NOW | RTLD_NOLOAD);
    for (const char* nm : names)
        if (!g_rccl.h) g_rccl.h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
    if (!g_rccl.h) return false;
    g_rccl.get_unique_id = (int (*)(NcclId*))dlsym(g_rccl.h, "ncclGetUniqueId");
    g_rccl.comm_init_rank = (int (*)(void**, int, NcclId, int))dlsym(g_rccl.h, "ncclCommInitRank");
    g_rccl.comm_destroy = (int (*)(void*))dlsym(g_rccl.h, "ncclCommDestroy");
    g_rccl.all_reduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(g_rccl.h, "ncclAllReduce");
    g_rccl.get_error_string = (const char* (*)(int))dlsym(g_rccl.h, "ncclGetErrorString");
    g_rccl.ok = g_rccl.get_unique_id && g_rccl.comm_init_rank && g_rccl.comm_destroy && g_rccl.all_reduce;
    return g_rccl.ok;
}
// svgpu_allreduce_fn bound to the context's communicator: sum of `count` doubles, in place, on `stream`
int rccl_allreduce_cb(void* user, double* dev_buf, size_t count, void* stream) {
    svgpu_ctx* ctx = (svgpu_ctx*)user;
    if (!ctx || !ctx->comm || !g_rccl.ok) return 1;
    return g_rccl.all_reduce(dev_buf, dev_buf, count, /*ncclFloat64*/ 8, /*ncclSum*/ 0, ctx->comm, (hipStream_t)stream);
}
}  // namespace

void sv_comm_release(svgpu_ctx* ctx) {
    if (ctx && ctx->comm && g_rccl.ok) g_rccl.comm_destroy(ctx->comm);
    if (ctx) ctx->comm = nullptr;
}

static_assert(sizeof(BaCtl) == BA_LAYOUT_CTL, "ba_layout.h and ba_kernels.h disagree on the control block");
static_assert(sizeof(BaInt2) == sizeof(int2) && alignof(BaInt2) == alignof(int2), "ba_layout.h: BaInt2 is not laid out like int2");
static_assert(sizeof(BaInt4) == sizeof(int4) && alignof(BaInt4) == alignof(int4), "ba_layout.h: BaInt4 is not laid out like int4");

namespace {

// The pointer fields of the kernels' argument struct, from the placed pieces (everything else starts as zero).  A renumbered solve reads
// the rn_* arrays where the others read the uploaded ones (the caller's order), which stay the sources of the permutation kernels.
void ba_bind(BaDev& D, const BaSizes& Z, const BaIn& in, const BaOut& out, const BaWork& w, bool sharded) {
    memset(&D, 0, sizeof(D));
    D.P = Z.P, D.L = Z.L, D.E = Z.E, D.world = Z.world;
    D.ctl = (BaCtl*)out.ctl.p;
    D.pose_buf[0] = in.pose, D.pose_buf[1] = w.pose1;
    D.pt_buf[0] = Z.renumber ? w.rn_pts : in.points, D.pt_buf[1] = w.pt1;
    D.e_pose = Z.renumber ? w.rn_e_pose : in.e_pose;
    D.e_point = Z.renumber ? w.rn_e_point : in.e_point;
    D.e_uvr = Z.renumber ? w.rn_uvr : in.e_uvr;
    D.e_w = Z.renumber ? w.rn_w : in.e_w;
    D.e_huber = Z.renumber ? w.rn_hub : in.e_hub;
    D.lm_off = Z.renumber ? w.rn_lm_off : in.lm_off;
    D.lm_order = w.rn_order;                               // (null unless renumbered)
    D.lm_off_caller = Z.renumber ? in.lm_off.p : nullptr;
    D.e_level = w.e_level, D.e_robust = in.e_robust, D.e_chi = w.e_chi;
    D.intr = in.intr;
    D.pose_slot = w.pose_slot, D.pt_free = w.pt_free, D.slot_pose = w.slot_pose;
    D.pe_off = in.pe_off, D.pe_idx = in.pe_idx;
    D.pm_point = w.pm_point, D.pm_uvr = w.pm_uvr, D.pm_w = w.pm_w, D.pm_hub = w.pm_hub;
    D.blk_off = w.blk_off, D.blk_pairs = (const int2*)w.blk_pairs.p, D.blk_ab = (const int2*)w.blk_ab.p, D.blk_pair_l = w.blk_pair_l;
    D.W = w.W, D.lp_part = w.lp_part, D.lm_max = w.lm_max, D.sc_part = w.sc_part, D.rhs_part = w.rhs_part;  // (lm_max: nb_lm == sv_ba_lm_blocks(L))
    D.Hll = w.Hll, D.bl = w.bl, D.Hpp = w.Hpp, D.bp = w.bp, D.Sblk = w.Sblk, D.S = w.S, D.dp = w.dp;
    D.red = w.red;  // chi2 parts | step-scale parts | flags
    D.red_chi_off = 0, D.red_chi_n = Z.nb_lm;
    D.red_scale_off = Z.nb_lm, D.red_scale_n = Z.nb_lm + Z.nb_pose;
    D.red_flag_off = Z.nb_lm + Z.nb_lm + Z.nb_pose;
    D.dbg = w.dbg;
    D.any_owner = w.any_owner;
    D.maxslots = w.sc + 8;
    D.xsum = sharded ? w.sc.p : nullptr;
    D.prow_off = w.prow_off, D.prow_ent = (const int2*)w.prow_ent.p, D.diag_blk = w.diag_blk;
    D.pcg_Minv = w.pcg_Minv, D.pcg_rws = w.pcg_rws, D.pcg_own = w.pcg_own, D.pcg_parts = w.pcg_parts, D.pcg_scal = w.pcg_scal;
}

// Copies between host memory and the pieces of the device arena, on the solve's stream.  A copy into or out of a piece moves the whole
// piece; one that is deliberately shorter names its count, in elements, and one longer than its piece fails the call instead of being
// copied (StagedCall's rule).
struct BaCopy {
    svgpu_ctx* ctx;
    hipStream_t s;
    bool fits(size_t count, size_t n) const {
        if (count > n) sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_local_ba: internal count mismatch (a transfer longer than its arena piece)");
        return count <= n;
    }
    template <class T>
    int h2d(Piece<T> dst, const T* src, size_t count) const {
        if (!fits(count, dst.n)) return SVGPU_ERR_INVALID;
        SV_HIP(ctx, hipMemcpyAsync(dst.p, src, count * sizeof(T), hipMemcpyHostToDevice, s));
        return SVGPU_OK;
    }
    template <class T>
    int h2d(Piece<T> dst, const T* src) const { return h2d(dst, src, dst.n); }
    template <class T>
    int h2d(Piece<T> dst, Piece<T> src) const { return h2d(dst, src.p, src.n); }  // (a host piece of another count than its device piece fails the call)
    template <class T>
    int h2d(Piece<T> dst, Piece<T> src, size_t count) const { return fits(count, src.n) ? h2d(dst, src.p, count) : SVGPU_ERR_INVALID; }
    // a run of adjacent pieces of the input block in one copy, padding included: from `first` up to where `behind` begins (both placements
    // come from one layout: the run is as long in the host image)
    template <class T, class U>
    int h2d_run(Piece<T> first, Piece<U> behind, Piece<T> src) const {
        SV_HIP(ctx, hipMemcpyAsync(first.p, src.p, (size_t)((const char*)behind.p - (const char*)first.p), hipMemcpyHostToDevice, s));
        return SVGPU_OK;
    }
    template <class T>
    int d2h(T* dst, Piece<T> src, size_t count) const {
        if (!fits(count, src.n)) return SVGPU_ERR_INVALID;
        SV_HIP(ctx, hipMemcpyAsync(dst, src.p, count * sizeof(T), hipMemcpyDeviceToHost, s));
        return SVGPU_OK;
    }
};

// The device side of the host team (ba_stage.h): its workers upload what they staged, on the copy stream or, under SVGPU_BA_COPY_ON_MAIN,
// on the solve's own (the caller has created the copy stream before it releases the team).
struct BaTeamUpload {
    svgpu_ctx* ctx;
    bool copy_on_main;
    int begin() const { return (int)hipSetDevice(ctx->device); }  // (the current device is a per-thread setting)
    template <class T>
    int operator()(Piece<T> dev, Piece<T> host, size_t first, size_t count) const {
        return (int)hipMemcpyAsync(dev.p + first, host.p + first, count * sizeof(T), hipMemcpyHostToDevice, copy_on_main ? ctx->stream : ctx->ba_copy_stream);
    }
};
static_assert(BA_STAGE_ERR_RANGE == (int)hipErrorInvalidValue, "ba_stage.h: a range error must read as hipErrorInvalidValue");

}  // namespace

static int local_ba_impl(svgpu_ctx* ctx, const svgpu_ba_problem* pr, bool single_stage, int rank, int world,
                         svgpu_allreduce_fn allreduce, void* ar_user, volatile uint8_t* stop, double* pose_out, double* points_out, uint8_t* outlier_out,
                         svgpu_ba_stats* stats) {
    if (!ctx || !pr || !pose_out || !points_out) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_local_ba: null argument");
    const int P = pr->num_poses, L = pr->num_points, E = pr->num_obs;
    if (P < 0 || L < 0 || E < 0 || (P > 0 && (!pr->pose_cw || !pr->pose_fixed || !pr->intrinsics)) || (L > 0 && !pr->points)
        || (E > 0 && (!pr->obs_pose || !pr->obs_point || !pr->obs_uvr || !pr->obs_inv_sigma_sq || (!outlier_out && !single_stage))))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_local_ba: inconsistent problem");
    // the record gathers of k_ba_schur_rhs address the W / Hll / bl arrays with 32-bit byte offsets (144 bytes per observation, 48 per landmark)
    if ((size_t)E * 144 >= ((size_t)1 << 32) || (size_t)L * 48 >= ((size_t)1 << 32))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_local_ba: more than 2^32 / 144 observations per rank (shard the landmarks over more ranks)");
    const bool sharded = allreduce != nullptr;
    if (sharded && (world < 1 || rank < 0 || rank >= world)) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_local_ba_sharded: bad rank/world");
    ctx->ba_ar_fn = allreduce;  // (the segmented envelope solve of ba_skyline.hip exchanges through the same all-reduce)
    ctx->ba_ar_user = ar_user;
    const BaEnv env = ctx->ba_env = ba_env();  // (the launchers of ba_kernels.hip and the envelope planner read the context's copy)
    if (!sharded) {
        world = 1;
        rank = 0;
    }
    svgpu_ba_stats st;
    memset(&st, 0, sizeof(st));
    const bool trace = env.trace > 0;
    auto t_start = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!trace) return;
        auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[ba] %-22s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_start).count());
        t_start = now;
    };
    // (the outputs start as the inputs: every early return leaves the estimate untouched.  At global-BA sizes the copy of the landmark
    //  positions -- 38 MB at 1.6 M landmarks -- is left to the host team below)
    const bool team_sized = ba_plan_team_sized(E, env);  // (the tests take small problems through the team's set-up)
    // host threads of the staging pass at global-BA sizes (SVGPU_BA_HOST_THREADS overrides, 1 .. 16)
    const int nth = ba_plan_host_threads(team_sized, env, team_sized ? ba_stage_usable_cpus() : 0);
    memcpy(pose_out, pr->pose_cw, sizeof(double) * 12 * (size_t)P);
    // (the flag is volatile and another thread raises it: ONE read decides both the copy and the return, so that no path leaves
    //  points_out unwritten -- ADVICE r5)
    const bool stopped_at_entry = !sharded && stop && *stop;  // local_bundle_adjuster_g2o.cc:308-310
    // complete: points_out holds a full copy of pr->points, or will once the team, whose workers make the copy in shares, is joined.
    // Every other copy is this one: here for a call without a team, on the way out for one that returns before its team has started
    struct PointsOut {
        double* out;
        const double* in;
        size_t bytes;
        bool complete;
        void restore() {
            if (!complete) memcpy(out, in, bytes);
            complete = true;
        }
        ~PointsOut() { restore(); }
    } points_guard{points_out, pr->points, sizeof(double) * 3 * (size_t)L, false};
    const bool team_copies_points = nth > 1 && !stopped_at_entry && E > 0 && P > 0 && L > 0;
    if (!team_copies_points) points_guard.restore();
    if (E > 0 && outlier_out) memset(outlier_out, 0, E);
    if (stats) *stats = st;
    if (!sharded) {
        if (stopped_at_entry) return SVGPU_STOPPED;
        if (E == 0 || P == 0 || L == 0) return SVGPU_OK;
    }
    else if (P == 0 || L == 0) return SVGPU_OK;  // same on every rank
    SV_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;

    // ---- page-locked staging (ba_layout.h): input block | output block | structure block, the input block laid out exactly like the one at
    //      the head of the device arena (one copy carries everything).  The observations are written sorted by landmark (stable; a plain
    //      copy when they arrive that way): landmark-major kernels then read contiguous runs.
    BaIn hin, din;    // h*: placed over the host image, d*: over the device arena (once its sizes are known, below)
    BaOut hout, dout;
    BaStructure hst;
    BaWork dw;
    {
        const BaSizes shape = ba_sizes(P, L, E, world, nullptr, false, false, false, BA_DBG_OFF);  // (the landmark offsets are written into this image)
        const auto image = [&](Arena& A) { ba_host_layout(A, shape, hin, hout, hst); };
        const int r = sv_ensure_stage(ctx, arena_measure(image));
        if (r) return r;
        Arena A(ctx->h_stage, ctx->stage_bytes);
        image(A);
        if (A.overflow) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_local_ba: internal staging overflow");
    }
    int* const lm_off = hin.lm_off;
    int* const e_pose = hin.e_pose;
    int* const e_point = hin.e_point;
    std::vector<uint8_t> level((sharded || !single_stage) ? E : 0, 0);  // (host image of the edge levels: the stage boundary and the sharded set-up read it)
    bool no_levels = true;  // until the first gate: every edge is at level 0
    // ---- the staging pass (ba_stage.h): scan and index arrays on nth threads; from here until it is joined, a team stages and uploads the
    //      measurements and copies points_out beside this thread's device work
    BaStageTeam<BaTeamUpload> team(*pr, hin, points_out, nth, BA_STAGE_TUNING, BaTeamUpload{ctx, env.copy_on_main});
    const BaStageResult staged = team.scan();
    if (staged.no_threads)
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_global_ba: could not start the host threads of the set-up (SVGPU_BA_ONE_THREAD=1 runs it on the caller's thread)");
    points_guard.complete |= nth > 1;  // (a team that has started copies points_out, whatever becomes of it)
    if (staged.bad_index) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_local_ba: observation index out of range");
    const std::vector<int>& perm = staged.perm;  // sorted position -> caller's observation index (empty = identity)
    const std::vector<uint8_t>& pose_seen = staged.pose_seen;
    // (the pose -> edge lists and the robust-kernel flags are built on the device once the observations are there: sv_ba_build_pose_lists)
    memcpy(hin.pose, pr->pose_cw, hin.pose.bytes());
    memcpy(hin.intr, pr->intrinsics, hin.intr.bytes());

    lap("sort observations");
    // ---- solver choice (svgpu_ba_set_solver; SVGPU_BA_SOLVER overrides for experiments)
    const int solver_opt = ba_plan_solver_option(ctx->ba_solver, env);
    // ---- device arena
    const bool want_dense = ba_plan_want_dense(solver_opt, sharded, P, env);
    // (a sharded solve renumbers the landmarks of ITS shard: the numbering is private to the rank's kernels, every landmark-sized exchange
    //  between ranks -- ownership marks, the final positions -- stays in the caller's numbering)
    const bool renumber = ba_plan_renumber(team.running(), single_stage, env);
    BaSizes Z = ba_sizes(P, L, E, world, lm_off, want_dense, renumber, /*units_wanted*/ !env.no_units, ba_plan_dbg_mode(env));
    Z.pair_scratch = std::max(std::max(std::max(sv_ba_pairs_scratch_bytes(Z.pair_cap, E, Z.nb_cap), sv_ba_pose_lists_scratch_bytes((size_t)E)), renumber ? sv_ba_renumber_scratch_bytes((size_t)L) : 0),
                              Z.chunk_units ? sv_ba_units_scratch_bytes(Z.pair_cap, Z.unit_cap()) : 0);
    const size_t pair_cap = Z.pair_cap, nb_cap = Z.nb_cap, xch_doubles = Z.xch_doubles;
    // ---- the device arena (ba_layout.h): measured for sv_ensure_scratch, then placed
    const auto arena = [&](Arena& A) { ba_device_layout(A, Z, din, dout, dw); };
    int rc = sv_ensure_scratch(ctx, arena_measure(arena));
    if (rc) return rc;
    Arena A(ctx->d_scratch, ctx->scratch_bytes);
    arena(A);
    if (A.overflow) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_local_ba: internal arena overflow");
    if (ba_in_bytes(din, dout) != ba_in_bytes(hin, hout)) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_local_ba: internal layout mismatch");
    BaDev D;
    ba_bind(D, Z, din, dout, dw, sharded);
    D.rank = rank;
    D.dbg_schur_on = ba_plan_dbg_kernel(env);
    for (int p = 0; p < P; ++p)
        if (pr->intrinsics[5 * (size_t)p] == 0.0 && pr->intrinsics[5 * (size_t)p + 1] == 0.0) D.any_equirect = 1;
    BaCopy cp{ctx, s};
    // page-locked block: the control block's read-back copy + the word the caller's stop flag is mirrored into for the device
    const size_t pinned_need = (sizeof(BaCtl) + 7) / 8 + 16;
    if (ctx->pinned_doubles < pinned_need) {
        if (ctx->h_pinned) SV_HIP(ctx, hipHostFree(ctx->h_pinned));
        ctx->h_pinned = nullptr;
        ctx->pinned_doubles = 0;
        SV_HIP(ctx, hipHostMalloc((void**)&ctx->h_pinned, sizeof(double) * pinned_need, hipHostMallocMapped));
        ctx->pinned_doubles = pinned_need;
    }
    if (!ctx->ev_ba) SV_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_ba, hipEventDisableTiming));
    BaCtl* const h_ctl = (BaCtl*)ctx->h_pinned;
    volatile int* const h_mirror = (volatile int*)(ctx->h_pinned + pinned_need - 8);
    *h_mirror = 0;
    {
        void* dptr = nullptr;
        SV_HIP(ctx, hipHostGetDevicePointer(&dptr, (void*)h_mirror, 0));
        D.stop_mirror = (const volatile int*)dptr;
    }

    uint8_t aux_flag = 0;  // g2o installs its own flag when the caller passes none (see svgpu.h)
    volatile uint8_t* flag = stop ? stop : &aux_flag;
    *h_mirror = *flag ? 1 : 0;
    // Wait for the stream.  While the device works, the caller's force_stop_flag (set asynchronously by the tracking thread,
    // mapping_module.h:232) is mirrored into the page-locked word k_ba_decide / k_ba_begin poll at every trial boundary.  The
    // host itself never branches on the caller's flag between two collectives of a sharded solve: every rank acts on the
    // all-reduced votes inside the control block only.
    auto wait_stream = [&]() -> int {
        SV_HIP(ctx, hipEventRecord(ctx->ev_ba, s));
        // (the mapping thread must not pin a host core the tracking thread needs: a short spin for the sub-100 us waits of a local
        //  window, then the poll yields / sleeps ~20 us between queries -- the stop flag is sampled every time)
        int polls = 0;
        for (;;) {
            if (*flag) *h_mirror = 1;
            const hipError_t q = hipEventQuery(ctx->ev_ba);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) return sv_set_error(ctx, SVGPU_ERR_HIP, "hipEventQuery", q);
            if (++polls > 2000) std::this_thread::sleep_for(std::chrono::microseconds(20));
            else if (polls > 200) std::this_thread::yield();
        }
        return SVGPU_OK;
    };
    auto read_ctl = [&]() -> int {
        SV_HIP(ctx, hipMemcpyAsync(h_ctl, D.ctl, sizeof(BaCtl), hipMemcpyDeviceToHost, s));
        return wait_stream();
    };

    const void* sorted_edges = nullptr;  // the (pose, edge) records of sv_ba_prepare_lists, kept in the W buffer until the measurements are there
    {
        const size_t want = sv_ba_pose_lists_scratch_bytes((size_t)E);
        const bool in_W = dw.W.bytes() >= want;  // (the pair lists are built in the pair scratch: the records survive them only in W)
        void* sc = in_W ? (void*)D.W : (void*)dw.pair_scratch.p;
        const size_t sc_bytes = in_W ? dw.W.bytes() : dw.pair_scratch.bytes();
        if (team.running() && !in_W) {  // (cannot happen at these sizes; the team's work is then uploaded in one piece)
            team.abandon();
            team.join();
            ba_stage_measurements(*pr, hin, 0, (size_t)E);
            memcpy(hin.points, pr->points, hin.points.bytes());
        }
        if (team.running()) {
            if (!ctx->ba_copy_stream) SV_HIP(ctx, hipStreamCreateWithFlags(&ctx->ba_copy_stream, hipStreamNonBlocking));
            if (!ctx->ev_ba_copy) SV_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_ba_copy, hipEventDisableTiming));
            if ((rc = cp.h2d_run(din.pose, din.points, hin.pose))) return rc;      // poses
            if ((rc = cp.h2d_run(din.intr, din.e_uvr, hin.intr))) return rc;       // intrinsics | e_pose | e_point
            if ((rc = cp.h2d_run(din.lm_off, din.pe_off, hin.lm_off))) return rc;  // landmark offsets
            // (the link is shared: the measurements queue behind the index arrays, which the structure kernels are waiting for)
            // SVGPU_BA_COPY_ON_MAIN: the measurements on the solve's own stream instead.  Measured over 150 config-5 calls: copy stream median
            // 7.50 ms, but 2 calls of 15 ms (the stream's first synchronisation arrives ~8 ms late: two DMA users of one process); own stream
            // 8.06 ms, no call above 8.9.  The default keeps the better mean (7.6 against 8.1); a caller that minds the tail sets the variable.
            if (!env.copy_on_main) {
                SV_HIP(ctx, hipEventRecord(ctx->ev_ba_copy, s));
                SV_HIP(ctx, hipStreamWaitEvent(ctx->ba_copy_stream, ctx->ev_ba_copy, 0));
            }
            team.release(din);  // (BaTeamUpload picks the stream)
        }
        else if ((rc = cp.h2d_run(din.pose, dout.ctl, hin.pose))) return rc;  // the whole input block
        if (renumber) {  // (ba_bind has pointed the kernels at the rn_* arrays)
            const int rr = sv_ba_renumber_landmarks(ctx, s, din.lm_off, din.e_pose, L, P, E, dw.pair_scratch, dw.pair_scratch.bytes(), dw.rn_order, dw.rn_lm_off, dw.rn_e_pose, dw.rn_e_point, dw.rn_src);
            if (rr) return rr;
        }
        // pose -> edge lists on the device (they need the pose indices only)
        const int rp = sv_ba_prepare_lists(ctx, s, D.e_pose, E, P, sc, sc_bytes, din.pe_off, D.e_level, D.e_chi, &sorted_edges);  // (also clears e_level / e_chi)
        if (rp) return rp;
    }
    // the measurements are on the device (pipelined: the stream waits for the copy stream) -> pose-major copies + robust flags
    auto finish_observations = [&]() -> int {
        if (team.running()) {
            const int he = team.join();
            if (he) return sv_set_error(ctx, SVGPU_ERR_HIP, "hipMemcpyAsync (measurements)", (hipError_t)he);
            SV_HIP(ctx, hipEventRecord(ctx->ev_ba_copy, ctx->ba_copy_stream));
            SV_HIP(ctx, hipStreamWaitEvent(s, ctx->ev_ba_copy, 0));
        }
        if (renumber) {  // measurements and positions into the solve's numbering
            sv_ba_permute_measurements(s, dw.rn_src, E, din.e_uvr, din.e_w, din.e_hub, dw.rn_uvr, dw.rn_w, dw.rn_hub);
            sv_ba_permute_points(s, dw.rn_order, L, din.points, dw.rn_pts);
        }
        const int rp = sv_ba_prepare_pose_major(ctx, s, sorted_edges, D.e_point, D.e_uvr, D.e_w, D.e_huber, E, din.pe_idx, D.e_robust, dw.pm_point, dw.pm_uvr, dw.pm_w, dw.pm_hub);
        sorted_edges = nullptr;
        return rp;
    };
    bool observations_finished = false;
    if (!team.running()) {
        const int rp = finish_observations();
        if (rp) return rp;
        observations_finished = true;
    }
    BaCtl ctl0;
    memset(&ctl0, 0, sizeof(ctl0));
    ctl0.gain_thr = pr->gain_threshold;
    ctl0.pcg_tol2 = ctx->pcg_tol * ctx->pcg_tol;
    ctl0.phase = 2;
    if ((rc = cp.h2d(dout.ctl, (const char*)&ctl0))) return rc;
    SV_HIP(ctx, hipMemsetAsync(dw.sc, 0, dw.sc.bytes(), s));

    // ---- exchange helpers (sharded solve; no-ops otherwise)
    enum { XC_SETUP = 1, XC_POSE_BLOCKS = 2, XC_SYSTEM = 3, XC_SUMS = 6 };  // (4, 5: the separator / solution exchanges of ba_skyline.hip)
    for (long long& v : ctx->ba_xch) v = 0;
    ctx->ba_xch[0] = sharded ? 1 : 0;
    auto allreduce_dev = [&](double* dev, size_t n, int cat) -> int {
        if (!sharded || n == 0) return SVGPU_OK;
        ctx->ba_xch[cat] += 8 * (long long)n;
        ++ctx->ba_xch[7];
        return allreduce(ar_user, dev, n, (void*)s) == 0 ? SVGPU_OK : sv_set_error(ctx, SVGPU_ERR_HIP, "all-reduce callback failed");
    };
    std::vector<double> xch_host(sharded ? std::max((size_t)P, nb_cap) + 8 : 8);  // (the landmark-sized exchanges stay on the device)
    auto allreduce_host = [&](size_t n) -> int {  // xch_host[0..n) summed over the ranks (set-up steps only)
        int r = cp.h2d(dw.xch, xch_host.data(), n);
        if (r || (r = allreduce_dev(dw.xch, n, XC_SETUP))) return r;
        if ((r = cp.d2h(xch_host.data(), dw.xch, n))) return r;
        SV_HIP(ctx, hipStreamSynchronize(s));
        return SVGPU_OK;
    };
    // Whether "the caller passed a stop pointer" must mean the same on every rank: the early return and the skipped second stage below
    // branch on it, and a rank that left while the others entered the next collective would hang them.  A sharded solve therefore acts as
    // if every rank had a pointer as soon as ANY rank has one (the flag rides along with the contract check).
    bool stop_ptr_any = stop != nullptr;
    if (sharded) {
        // contract check on the device: a landmark's observations must not be split over ranks.  Every rank marks the landmarks it holds
        // observations of (its landmark offsets are already there), the marks are summed, a landmark with two owners fails the call on
        // every rank; what comes back is two words.  The sum also says which landmarks have an owner at all (the final exchange of the
        // points leaves the others alone).
        sv_ba_owned_mark(s, din.lm_off, L, dw.xch, stop ? 1.0 : 0.0);
        int r = allreduce_dev(dw.xch, (size_t)L + 1, XC_SETUP);
        if (r) return r;
        sv_ba_owned_check(s, dw.xch, L, dw.any_owner, dw.sc + 32);
        double verdict[2] = {0.0, 0.0};
        SV_HIP(ctx, hipMemcpyAsync(verdict, dw.sc + 32, 16, hipMemcpyDeviceToHost, s));
        SV_HIP(ctx, hipStreamSynchronize(s));
        if (verdict[0] > 0.5) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_local_ba_sharded: observations must be sharded by landmark");
        stop_ptr_any = verdict[1] > 0.5;
    }

    lap("arena + uploads");
    HostStructure HS;
    bool xs_on = false;  // keyframe-segment exchange (decided with the plan, the same on every rank)
    int xs_nb = 0, xs_ns = 0;
    bool have_lists = false;
    std::vector<uint8_t> pose_active;
    int solver = SV_BA_SOLVER_CHOLESKY;
    auto upload_structure = [&]() -> int {
        int r = SVGPU_OK;
        const std::vector<uint8_t>* pa_override = nullptr;
        if (sharded) {  // a pose is active if ANY rank holds an active observation of it
            for (int p = 0; p < P; ++p) xch_host[p] = 0;
            for (int e = 0; e < E; ++e)
                if (!level[e]) xch_host[e_pose[e]] = 1;
            if ((r = allreduce_host(P))) return r;
            pose_active.assign(P, 0);
            for (int p = 0; p < P; ++p) pose_active[p] = xch_host[p] > 0.5;
            pa_override = &pose_active;
        }
        // Activity of poses / landmarks under the current levels (cheap), then the expensive part -- pose->edge lists
        // and (edge, edge) pair lists -- only when the free-pose numbering changed.  Lists built for an earlier stage
        // stay valid: edges excluded since then are skipped by level (lin_pose, rhs) or contribute W = Y = 0 (pairs).
        auto tb0 = std::chrono::steady_clock::now();
        auto sub = [&](const char* what) {
            if (trace) std::fprintf(stderr, "[ba]     %-20s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb0).count());
        };
        HostStructure probe;
        activity_only(*pr, e_pose, e_point, level, pa_override, probe, no_levels ? &pose_seen : nullptr, no_levels ? lm_off : nullptr);
        const bool reuse = have_lists && probe.pose_slot == HS.pose_slot;
        if (reuse) {
            HS.pt_free = probe.pt_free;
            HS.nL = probe.nL;
        }
        else {
            HS.pose_slot = probe.pose_slot;
            HS.slot_pose = probe.slot_pose;
            HS.pt_free = probe.pt_free;
            HS.nP = probe.nP;
            HS.nL = probe.nL;
        }
        D.nP = HS.nP;
        D.n = 6 * HS.nP;
        D.lin_split = sv_ba_lin_split(E, HS.nP);
        D.chol_in_lds = D.n <= 186 && sv_ba_chol_bytes(D.n) <= 160 * 1024 - 12 * 1024;
        D.chol_mfma = solver_opt == SV_BA_SOLVER_CHOLESKY_MFMA ? 1 : 0;  // the same dense on-chip solve, its MFMA form
        D.Hpp_full = sharded ? dw.HB_full.p : D.Hpp;
        D.bp_full = sharded ? dw.HB_full + 36 * (size_t)HS.nP : D.bp;
        D.scale_pose = (!sharded || rank == 0) ? 1 : 0;
        D.add_lambda = (!sharded || rank == 0) ? 1 : 0;
        memcpy(hst.pt_free, HS.pt_free.data(), hst.pt_free.bytes());
        if (renumber) {
            if ((r = cp.h2d(dw.rn_pt_free_in, hst.pt_free))) return r;
            sv_ba_permute_flags(s, dw.rn_order, L, dw.rn_pt_free_in, dw.pt_free);
        }
        else if ((r = cp.h2d(dw.pt_free, hst.pt_free))) return r;
        if (!reuse) {
            memcpy(hst.pose_slot, HS.pose_slot.data(), hst.pose_slot.bytes());
            if ((r = cp.h2d(dw.pose_slot, hst.pose_slot))) return r;
            // The pair lists are built on the device.  A local-BA sized problem (<= 48 free poses; the count is the same on every rank of
            // a sharded solve) keeps EVERY upper block -- blocks without a pair are zero blocks, the solvers of that size are dense
            // anyway, and no union of block patterns has to be agreed between ranks -- so nothing has to come back: the pair total stays
            // on the device (launches sized for the capacity) and the whole structure pipeline runs unattended.
            // Larger systems synchronise twice (pair total, block offsets) and keep only the blocks that hold a pair.
            const bool all_blocks = HS.nP <= 48;  // (the pair total stays on the device: the launches are sized for the capacity)
            std::vector<int> dense_off;
            if (all_blocks) {
                int rp = sv_ba_build_pairs_async(ctx, s, D, dw.pair_scratch, dw.pair_scratch.bytes(), pair_cap, -1, (int2*)dw.blk_pairs.p, dw.blk_pair_l, dw.blk_off);
                if (rp) return rp;
                sub("pairs enqueued");
            }
            have_lists = true;
            for (int sl = 0; sl < HS.nP; ++sl) hst.slot_pose[sl] = HS.slot_pose[sl];
            if (HS.nP > 0 && (r = cp.h2d(dw.slot_pose, hst.slot_pose, HS.nP))) return r;
            if (all_blocks) {
                HS.blk_ab.clear();
                for (int a = 0; a < HS.nP; ++a)
                    for (int b = a; b < HS.nP; ++b) {
                        int2 ab;
                        ab.x = a;
                        ab.y = b;
                        HS.blk_ab.push_back(ab);
                    }
                HS.blk_off.clear();  // lives on the device only
                HS.num_pairs = pair_cap;  // (an upper bound: sum over the landmarks of k^2; sizes the Schur shares)
            }
            else {
                int rp = sv_ba_build_pairs(ctx, s, D, dw.pair_scratch, dw.pair_scratch.bytes(), pair_cap, (int2*)dw.blk_pairs.p, dw.blk_pair_l, dense_off);
                if (rp) return rp;
                sub("device pairs");
                std::vector<uint8_t> present(dense_off.size() ? dense_off.size() - 1 : 0, 0);
                for (size_t k = 0; k < present.size(); ++k) present[k] = dense_off[k + 1] > dense_off[k];
                if (sharded && !present.empty()) {  // the kept-block list must be the same on every rank: union of the local patterns
                    for (size_t k = 0; k < present.size(); ++k) xch_host[k] = present[k];
                    if ((r = allreduce_host(present.size()))) return r;
                    for (size_t k = 0; k < present.size(); ++k) present[k] = xch_host[k] > 0.5;
                }
                compact_blocks(dense_off, present, HS);
                if ((r = cp.h2d(dw.blk_off, HS.blk_off.data(), HS.blk_off.size()))) return r;
            }
            // block rows for the PCG: row a lists its kept blocks (a, b) and, transposed, (b, a)
            const int NB = (int)HS.blk_ab.size();
            if ((size_t)NB > hst.blk_ab.n) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_local_ba: more kept blocks than the upper triangle holds");
            memcpy(hst.blk_ab, HS.blk_ab.data(), sizeof(int2) * (size_t)NB);
            ba_block_rows(hst.blk_ab, NB, HS.nP, hst.prow_off, hst.diag, hst.prow_ent);
            const int rows = hst.prow_off[HS.nP];
            if (NB > 0 && (r = cp.h2d(dw.blk_ab, hst.blk_ab, NB))) return r;
            if ((r = cp.h2d(dw.prow_off, hst.prow_off, HS.nP + 1))) return r;
            if (rows > 0 && (r = cp.h2d(dw.prow_ent, hst.prow_ent, rows))) return r;
            if (HS.nP > 0 && (r = cp.h2d(dw.diag_blk, hst.diag, HS.nP))) return r;
            sub("block rows");
        }
        else sv_ba_zero_inactive(s, D);
        D.NB = (int)HS.blk_ab.size();
        D.g = D.Sblk + 36 * (size_t)D.NB;
        D.pcg_nparts = (HS.nP + 3) / 4;
        D.nshare = ba_plan_nshare(HS.num_pairs, D.NB, env);  // shares per block
        if (!reuse) {
            D.unit_rec = nullptr;
            D.num_units = 0;
            if (ba_plan_units(Z.chunk_units, HS.nP, D.NB, D.nshare, HS.num_pairs, env)) {
                const int shift = ba_plan_chunk_shift(E, L, env);  // a chunk = 2^shift consecutive landmark ranks
                int U = 0;
                const int ru = sv_ba_build_units(ctx, s, dw.blk_off, D.NB, dw.blk_pair_l, (int)HS.num_pairs, L, shift, (int)Z.unit_cap(), dw.pair_scratch, dw.pair_scratch.bytes(), (int4*)dw.unit_rec.p, dw.blk_unit_off, &U);
                if (ru) return ru;
                if (U > 0) {
                    D.unit_rec = (const int4*)dw.unit_rec.p, D.blk_unit_off = dw.blk_unit_off, D.rhs_unit = dw.rhs_unit, D.num_units = U;
                }
                if (trace) std::fprintf(stderr, "[ba]     chunk-major units: %d (chunks of %d landmarks)\n", U, 1 << shift);
                sub("units");
            }
        }
        // solver of this stage: PCG inside one workgroup's LDS when the blocks fit, else one launch per PCG iteration
        const bool lds_ok = sv_ba_pcg_lds_bytes(D) > 0;
        // (the cascade AUTO -> CHOLESKY / DENSE / ENVELOPE / PCG_LDS / PCG_MULTI: ba_plan.h)
        const BaSolverFront front = ba_plan_solver_front(solver_opt, D.chol_in_lds != 0, D.S != nullptr, D.n, D.NB, HS.nP, lds_ok);
        if (front.ask_envelope && !reuse) {
            bool ok = false;
            const int rs = sv_sky_plan(ctx, s, HS.nP, HS.blk_ab, (size_t)256 << 20, &ok, rank, world);
            if (rs) return rs;
            HS.envelope_ok = ok;
        }
        solver = ba_plan_solver_final(front, HS.envelope_ok, lds_ok);
        ctx->ba_last_solver = solver;
        // Keyframe-segment exchange.  When the envelope solve is segmented and every observation this rank holds is of a keyframe in one of
        // ITS jobs' pieces (or of a separator keyframe) -- svgpu_ba_partition_keyframe_segments cuts shards that way -- the blocks and
        // right-hand side rows of a piece are complete on the rank that eliminates it and no other rank reads them: only the kept blocks
        // between two separator rows and the separator rows of g have to be summed.  One all-reduced flag makes the decision collective.
        if (!reuse) {
            xs_on = false;
            D.lam_slot = nullptr;
            const std::vector<int>*job_of = nullptr, *owner = nullptr, *sep_blocks = nullptr;
            const bool candidate = sharded && world > 1 && solver == SV_BA_SOLVER_ENVELOPE && !env.exchange_full && sv_sky_current_roles(ctx, &job_of, &owner, &sep_blocks);
            if (sharded && world > 1) {
                double misplaced = candidate ? 0.0 : 1.0;
                if (candidate)
                    for (int e = 0; e < E && misplaced == 0.0; ++e) {
                        if (level[e]) continue;
                        const int sl = HS.pose_slot[e_pose[e]];
                        if (sl >= 0 && (*job_of)[sl] >= 0 && (*owner)[(*job_of)[sl]] != rank) misplaced = 1.0;
                    }
                xch_host[0] = misplaced;
                if ((r = allreduce_host(1))) return r;
                std::vector<int> sep_slots;
                if (candidate)
                    for (int sl = 0; sl < HS.nP; ++sl)
                        if ((*job_of)[sl] < 0) sep_slots.push_back(sl);
                if (candidate && xch_host[0] < 0.5 && 36 * sep_blocks->size() + 6 * sep_slots.size() <= xch_doubles) {
                    xs_on = true;
                    xs_nb = (int)sep_blocks->size();
                    xs_ns = (int)sep_slots.size();
                    if ((size_t)xs_nb + xs_ns > hst.xs_idx.n) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_local_ba: more separator blocks and rows than their index list holds");
                    SV_HIP(ctx, hipStreamSynchronize(s));  // (an upload of an earlier structure may still be reading the lists' image)
                    for (int k = 0; k < xs_nb; ++k) hst.xs_idx[k] = (*sep_blocks)[k];
                    for (int k = 0; k < xs_ns; ++k) hst.xs_idx[xs_nb + k] = sep_slots[k];
                    for (int sl = 0; sl < HS.nP; ++sl) hst.lam[sl] = (*job_of)[sl] >= 0 ? (*owner)[(*job_of)[sl]] == rank : rank == 0;
                    if ((r = cp.h2d(dw.xs_idx, hst.xs_idx, xs_nb + xs_ns))) return r;
                    if ((r = cp.h2d(dw.lam_slot, hst.lam, HS.nP))) return r;
                    SV_HIP(ctx, hipStreamSynchronize(s));  // (the staging image is rewritten by the next structure)
                    D.lam_slot = dw.lam_slot;
                }
            }
            ctx->ba_xch[0] = !sharded ? 0 : (xs_on ? 2 : 1);
            if (trace && sharded) std::fprintf(stderr, "[ba]     exchange per trial: %s (%d separator blocks, %d separator rows of %d)\n", xs_on ? "keyframe segments" : "whole reduced system", xs_nb, xs_ns, HS.nP);
        }
        if (sv_ba_lin_split_max() > 16 || sv_ba_rhs_split() > 16) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_local_ba: partial-sum buffers too small for the kernel splits");
        if (trace) std::fprintf(stderr, "[ba]   structure %s     %8.3f ms (%zu pairs, %zu blocks, n = %d, solver %d)\n", reuse ? "reused " : "rebuilt", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb0).count(), HS.num_pairs, HS.blk_ab.size(), D.n, solver);
        return SVGPU_OK;
    };

    // activeRobustChi2 of the estimate -> partial sums on the device (a sharded solve folds them and sums over the ranks,
    // the stop votes ride along)
    auto chi2_begin = [&](int store_cache) -> int {
        sv_ba_chi2(ctx, s, D, 0, store_cache, 0);
        if (sharded) {
            sv_ba_fold(s, D, dw.sc, 0);
            return allreduce_dev(dw.sc, 4, XC_SUMS);
        }
        return SVGPU_OK;
    };

    // one damping trial (preceded by the linearisation when the control block asks for one); everything is guarded by the control
    // block on the device, so a step enqueued behind a finished optimisation costs a dozen empty launches
    const int pcg_max_it = ctx->pcg_max_it > 0 ? ctx->pcg_max_it : 0;
    auto enqueue_step = [&](bool* finished_seen) -> int {
        int r;
        const bool fused_tail = !env.proc.no_fusion &&!sharded && sv_ba_tail_ok(D);
        sv_ba_linearize(ctx, s, D, sharded ? 0 : 1);
        if (sharded) {  // pose blocks summed over the ranks before the damping is initialised from their diagonal
            // ONE collective (round 6; it was two): the rank's slot of the damping initialisation -- the largest diagonal entry of ITS landmarks,
            // which k_ba_lin has just left in the control block -- rides behind the pose blocks.  The pose part of the maximum is taken from the
            // SUMMED blocks afterwards, identically on every rank; k_ba_prepare takes the largest of that and the slots.
            if (HS.nP > 0) {
                SV_HIP(ctx, hipMemcpyAsync(dw.HB_full, D.Hpp, 8 * 36 * (size_t)HS.nP, hipMemcpyDeviceToDevice, s));
                SV_HIP(ctx, hipMemcpyAsync(dw.HB_full + 36 * (size_t)HS.nP, D.bp, 8 * 6 * (size_t)HS.nP, hipMemcpyDeviceToDevice, s));
            }
            D.maxslots = dw.HB_full + 42 * (size_t)HS.nP;
            sv_ba_maxslot(s, D);
            if ((r = allreduce_dev(dw.HB_full, 42 * (size_t)HS.nP + (size_t)world, XC_POSE_BLOCKS))) return r;
            sv_ba_maxdiag(s, D);
            sv_ba_prepare(s, D);
        }
        sv_ba_reduce(ctx, s, D);
        if (HS.nP > 0) {
            if (xs_on) {  // keyframe-segment shards: only what touches two separator rows is shared between ranks
                sv_ba_xs_move(s, D, dw.xs_idx, xs_nb, dw.xs_idx + xs_nb, xs_ns, dw.xch, 0);
                if ((r = allreduce_dev(dw.xch, 36 * (size_t)xs_nb + 6 * (size_t)xs_ns, XC_SYSTEM))) return r;
                sv_ba_xs_move(s, D, dw.xs_idx, xs_nb, dw.xs_idx + xs_nb, xs_ns, dw.xch, 1);
            }
            else if ((r = allreduce_dev(D.Sblk, 36 * (size_t)D.NB + (size_t)D.n, XC_SYSTEM))) return r;
        }
        if (HS.nP > 0) {
            if (solver == SV_BA_SOLVER_CHOLESKY) sv_ba_solve(ctx, s, D);
            else if (solver == SV_BA_SOLVER_PCG_LDS) sv_ba_solve_pcg_lds(ctx, s, D);
            else if (solver == SV_BA_SOLVER_DENSE) sv_ba_solve_dense(ctx, s, D);
            else if (solver == SV_BA_SOLVER_ENVELOPE) {
                if ((r = sv_sky_solve(ctx, s, D))) return r;
            }
            else {
                // PCG: iterations are enqueued in chunks; the control block says when the solve (or the whole optimisation) is over
                sv_pcg_init(ctx, s, D);
                int it0 = 0, chunk = 96;
                for (;;) {
                    sv_pcg_iterate(ctx, s, D, it0, chunk);
                    it0 += chunk;
                    if ((r = read_ctl())) return r;
                    if (h_ctl->phase != 1) {
                        *finished_seen = h_ctl->phase == 2;
                        break;
                    }
                    if (h_ctl->pcg_done) break;
                    chunk = std::min(chunk + chunk / 2, 768);
                }
            }
        }
        if (fused_tail) sv_ba_tail(ctx, s, D);
        else {
            sv_ba_update(ctx, s, D);
            sv_ba_chi2(ctx, s, D, 1, 0, 1);
        }
        if (sharded) {
            sv_ba_fold(s, D, dw.sc, 1);
            if ((r = allreduce_dev(dw.sc, 4, XC_SUMS))) return r;
        }
        sv_ba_decide(s, D);
        return SVGPU_OK;
    };

    // SparseOptimizer::optimize(iterations) with the terminate_action hook; the Levenberg-Marquardt loop itself runs on the device
    int pcg_mi = 0;
    bool first_stage = true;
    // device_boundary: the stage follows k_ba_activity on the stream -- the structure of the previous stage is kept (same pose numbering, the
    // landmark activity already refreshed on the device) and the stage refuses to start if that turned out to be wrong (ctl.structure_changed)
    auto optimize = [&](int iterations, int* iters_done, bool device_boundary = false) -> int {
        *iters_done = 0;
        int r = SVGPU_OK;
        if (device_boundary) sv_ba_zero_inactive(s, D);
        else r = upload_structure();
        if (r) return r;
        if (!observations_finished) {
            if ((r = finish_observations())) return r;
            observations_finished = true;
        }
        const bool nothing = !sharded && HS.nP + HS.nL == 0;
        // the PCG iteration cap depends on the size of the reduced system of this stage
        pcg_mi = pcg_max_it > 0 ? pcg_max_it : std::max(2000, 4 * D.n);
        SV_HIP(ctx, hipMemcpyAsync(&D.ctl->pcg_max_it, &pcg_mi, sizeof(int), hipMemcpyHostToDevice, s));
        if ((r = chi2_begin(first_stage ? 1 : 0))) return r;
        first_stage = false;
        sv_ba_begin(s, D, nothing ? 0 : iterations, (int)(sharded ? 0 : (*flag ? 1 : 0)) | (device_boundary ? 2 : 0));
        // The steps of the whole stage are enqueued before the first read-back (the common case -- every first trial accepted --
        // costs ONE synchronisation per stage); rejected trials consume steps, so the loop tops up until the device reports phase 2.
        const int max_steps = 10 * std::max(iterations, 1);
        const bool trace2 = env.trace == 2;  // one step per read-back, printed
        int steps = 0, todo = nothing ? 0 : (trace2 ? 1 : iterations);
        for (;;) {
            bool finished = false;
            for (int k = 0; k < todo && !finished; ++k, ++steps)
                if ((r = enqueue_step(&finished))) return r;
            if ((r = read_ctl())) return r;
            if (trace2) std::fprintf(stderr, "[ba]     step %3d: it %d phase %d chi2 %.9g temp %.9g lambda %.6g rho %.4g qmax %d pcg_it %d fail %d\n", steps, h_ctl->it, h_ctl->phase, h_ctl->current_chi, h_ctl->temp_chi, h_ctl->lambda, h_ctl->rho, h_ctl->qmax, h_ctl->pcg_it, h_ctl->solve_failures);
            if (h_ctl->phase == 2 || steps >= max_steps) break;
            todo = trace2 ? 1 : std::max(1, std::min(h_ctl->it_max - h_ctl->it, max_steps - steps));
        }
        if (device_boundary && h_ctl->structure_changed) {
            // the stage refused to start (a pose lost its last edge): the control block still carries the PREVIOUS stage's iteration count and
            // terminate verdict -- nothing of it belongs to this stage; the caller rebuilds the structure on the host and runs the stage again
            *iters_done = 0;
            return SVGPU_OK;
        }
        *iters_done = h_ctl->it;
        // errors cached by the last computeActiveErrors (used by the gate and the outlier list)
        if (*iters_done > 0) sv_ba_chi2(ctx, s, D, 0, 1, 0);
        if (h_ctl->stopped_by_terminate) {
            *flag = 1;  // terminate_action writes through the optimizer's force-stop pointer
            st.stopped_by_terminate_action = 1;
        }
        else if (h_ctl->stop) *flag = 1;  // sharded: another rank's caller raised it
        return SVGPU_OK;
    };

    st.chi2_initial = 0;
    int it1 = 0, it2 = 0;
    rc = optimize(pr->num_first_iter, &it1);
    if (rc) return rc;
    if (D.dbg_schur_on) {  // SVGPU_BA_DBG=schur: life of the units of the last k_ba_schur_rhs launch (100 MHz stamps)
        const size_t nu = D.unit_rec ? (size_t)D.num_units : (size_t)D.NB * D.nshare;
        std::vector<unsigned long long> h(8 * nu);
        SV_HIP(ctx, hipMemcpyAsync(h.data(), D.dbg, 8 * h.size(), hipMemcpyDeviceToHost, s));
        SV_HIP(ctx, hipStreamSynchronize(s));
        unsigned long long t0 = ~0ull, t1 = 0;
        for (size_t u = 0; u < nu; ++u)
            if (h[8 * u + 4] < h[8 * u]) h[8 * u + 1] = h[8 * u + 2] = h[8 * u + 3] = h[8 * u + 4] = h[8 * u];  // an empty share: entry stamp only
        for (size_t u = 0; u < nu; ++u) t0 = std::min(t0, h[8 * u]), t1 = std::max(t1, h[8 * u + 4]);
        double sum[5] = {0, 0, 0, 0, 0};
        std::vector<int> per_cu(8 * 64, 0);
        std::vector<double> life(nu);
        for (size_t u = 0; u < nu; ++u) {
            for (int k = 1; k < 5; ++k) sum[k] += (double)(h[8 * u + k] - h[8 * u + k - 1]) * 0.01;
            life[u] = (double)(h[8 * u + 4] - h[8 * u]) * 0.01;
            sum[0] += life[u];
            const unsigned hw = (unsigned)h[8 * u + 5], xcc = (unsigned)(h[8 * u + 5] >> 32) & 15;
            per_cu[(xcc & 7) * 64 + (((hw >> 13) & 3) * 16 + ((hw >> 8) & 15))]++;
        }
        std::sort(life.begin(), life.end());
        int cus = 0, mxu = 0;
        for (int c : per_cu) cus += c > 0, mxu = std::max(mxu, c);
        std::fprintf(stderr, "[ba] schur stamps: %zu units, span %.1f us, mean life %.2f us (p10 %.2f p50 %.2f p90 %.2f max %.2f) -> mean resident %.0f waves; per unit: setup %.2f | first trip %.2f | other trips %.2f | reduce %.2f us; %d (XCC, SE, CU) slots used, max %d units on one\n",
                     nu, (double)(t1 - t0) * 0.01, sum[0] / nu, life[nu / 10], life[nu / 2], life[nu * 9 / 10], life[nu - 1], sum[0] / ((double)(t1 - t0) * 0.01),
                     sum[1] / nu, sum[2] / nu, sum[3] / nu, sum[4] / nu, cus, mxu);
        // start times per XCC: does every XCC receive units at the same rate?
        double last_start[8] = {0}, n_x[8] = {0};
        for (size_t u = 0; u < nu; ++u) {
            const unsigned xcc = (unsigned)(h[8 * u + 5] >> 32) & 7;
            last_start[xcc] = std::max(last_start[xcc], (double)(h[8 * u] - t0) * 0.01), n_x[xcc] += 1;
        }
        for (int x = 0; x < 8; ++x) std::fprintf(stderr, "[ba]   XCC %d: %.0f units, last start at %.1f us\n", x, n_x[x], last_start[x]);
    }
    if (D.dbg && D.dbg_schur_on == 2) {  // SVGPU_BA_DBG=chol: phase stamps of the last k_ba_chol_mfma (100 MHz): load | per panel factor, barrier, update | end
        std::vector<unsigned long long> h(32);
        SV_HIP(ctx, hipMemcpyAsync(h.data(), D.dbg, 8 * h.size(), hipMemcpyDeviceToHost, s));
        SV_HIP(ctx, hipStreamSynchronize(s));
        std::fprintf(stderr, "[ba] chol stamps (us):");
        for (int k = 1; k < 31; ++k)
            if (h[k] >= h[0] && h[k] - h[0] < 100000000ull) std::fprintf(stderr, " %d:%.2f", k, (double)(h[k] - h[0]) * 0.01);
        std::fprintf(stderr, "\n");
    }
    if (D.dbg && !D.dbg_schur_on) {  // SVGPU_BA_DBG: where the time of the last fused tail went (100 MHz stamps, relative to the first workgroup's entry)
        const int nb_lm = Z.nb_lm;
        std::vector<unsigned long long> h(dw.dbg.n);
        SV_HIP(ctx, hipMemcpyAsync(h.data(), D.dbg, 8 * h.size(), hipMemcpyDeviceToHost, s));
        SV_HIP(ctx, hipStreamSynchronize(s));
        unsigned long long t0 = ~0ull;
        for (int b = 0; b < nb_lm; ++b) t0 = std::min(t0, h[8 * (size_t)b]);
        double mx[7] = {0, 0, 0, 0, 0, 0, 0}, mn[7] = {1e30, 1e30, 1e30, 1e30, 1e30, 1e30, 1e30};
        for (int b = 0; b < nb_lm; ++b)
            for (int k = 0; k < 7; ++k) {
                const double us = (double)(h[8 * (size_t)b + k] - t0) * 0.01;
                mx[k] = std::max(mx[k], us), mn[k] = std::min(mn[k], us);
            }
        std::fprintf(stderr, "[ba] tail stamps (us, min..max over %d workgroups): entry %.2f..%.2f | hop1 %.2f..%.2f | staged %.2f..%.2f | poses %.2f..%.2f | sums %.2f..%.2f\n",
                     nb_lm, mn[0], mx[0], mn[1], mx[1], mn[2], mx[2], mn[3], mx[3], mn[4], mx[4]);
    }
    st.chi2_initial = h_ctl->chi_begin;
    st.iters_stage1 = it1;
    lap("stage 1");
    if (sharded && stop_ptr_any && h_ctl->stop && it1 == 0 && !h_ctl->stopped_by_terminate) {  // raised before any work, agreed by all ranks
        st.lm_trials = h_ctl->lm_trials;
        if (stats) *stats = st;
        return SVGPU_STOPPED;
    }
    bool run_robust = !single_stage;
    // :317-321 (only the CALLER's flag is consulted here); sharded: the all-reduced vote and the all-reduced "a pointer exists", never a local fact
    if (sharded ? (stop_ptr_any && h_ctl->stop != 0) : (stop && *stop != 0)) run_robust = false;
    if (run_robust) {
        st.stage2_entered = 1;
        // The stage boundary stays on the device when nothing about it needs the host (one GPU, a reduced system whose blocks are all kept):
        // gate -> landmark activity + gated count + "did a pose lose its last edge" -> the second stage's kernels, enqueued without a
        // synchronisation; only a changed pose numbering (rare: a keyframe of the window left without a single inlier) comes back here.
        bool on_device = !sharded && E > 0 && HS.nP > 0 && HS.nP <= 48 && have_lists && !env.host_boundary;
        if (on_device) {
            sv_ba_gate(s, D, 1, nullptr);
            sv_ba_activity(s, D, dw.pt_free);
            rc = optimize(pr->num_second_iter, &it2, true);
            if (rc) return rc;
            st.num_gated = h_ctl->gated;
            if (h_ctl->structure_changed) on_device = false;  // the stage refused to start: the host path below rebuilds and runs it
        }
        if (!on_device) {
            if (E > 0) {
                if (!h_ctl->structure_changed) sv_ba_gate(s, D, 1, nullptr);  // (else the levels are already set)
                SV_HIP(ctx, hipMemcpyAsync(level.data(), D.e_level, E, hipMemcpyDeviceToHost, s));
                no_levels = false;
                SV_HIP(ctx, hipStreamSynchronize(s));
            }
            double gated = 0;
            for (int e = 0; e < E; ++e) gated += level[e];
            if (sharded) {
                xch_host[0] = gated;
                if ((rc = allreduce_host(1))) return rc;
                gated = xch_host[0];
            }
            st.num_gated = (int32_t)gated;
            rc = optimize(pr->num_second_iter, &it2);
            if (rc) return rc;
        }
        st.iters_stage2 = it2;
        lap("stage 2");
    }
    // ---- outlier list, final chi2, read-back: ONE copy of the output block (control block | poses | points | outlier flags)
    if (E > 0 && outlier_out) sv_ba_gate(s, D, 0, dout.outlier);
    if ((rc = chi2_begin(0))) return rc;
    sv_ba_begin(s, D, 0, 0);  // folds the chi2 of the final estimate into the control block (phase 2: nothing else happens)
    sv_ba_pack_out(s, D, dout.state);
    if (sharded) {  // every rank ends with every landmark: owners contribute their points, the rest zeros (an all-gather through the all-reduce), on the device
        sv_ba_points_share(s, D, ba_out_points(dout, P), dw.xch, 0);
        if ((rc = allreduce_dev(dw.xch, 3 * (size_t)L, XC_SETUP))) return rc;
        sv_ba_points_share(s, D, ba_out_points(dout, P), dw.xch, 1);
    }
    // (a caller that takes no outlier flags -- global BA: 1.2 MB at config 5 -- gets the block without them)
    SV_HIP(ctx, hipMemcpyAsync(hout.ctl, dout.ctl, ba_out_bytes(dout, outlier_out != nullptr), hipMemcpyDeviceToHost, s));
    if ((rc = wait_stream())) return rc;
    memcpy(h_ctl, hout.ctl, hout.ctl.bytes());
    memcpy(pose_out, ba_out_poses(hout, P), ba_out_poses(hout, P).bytes());
    {
        const char* const src = (const char*)ba_out_points(hout, P).p;
        const size_t bytes = ba_out_points(hout, P).bytes();
        if (bytes < ((size_t)16 << 20)) memcpy(points_out, src, bytes);
        else {  // (38 MB at 1.6 M landmarks: one core copies them in ~2 ms)
            const int nt = 4;
            std::vector<std::thread> th;
            auto share = [=](int q) { memcpy((char*)points_out + bytes * q / nt, src + bytes * q / nt, bytes * (q + 1) / nt - bytes * q / nt); };
            int started = 1;  // shares [0, started) have an owner (this thread takes 0)
            try {  // (no exception may cross the C ABI with joinable threads behind it: a share that finds no thread is copied here)
                th.reserve(nt - 1);
                for (int q = 1; q < nt; ++q) {
                    th.emplace_back(share, q);
                    started = q + 1;
                }
            }
            catch (...) {
            }
            share(0);
            for (int q = started; q < nt; ++q) share(q);
            for (auto& t : th) t.join();
        }
    }
    const uint8_t* const outl = hout.outlier;
    if (outlier_out)
        for (int k = 0; k < E; ++k) outlier_out[perm.empty() ? k : perm[k]] = outl[k];
    st.chi2_final = h_ctl->chi_begin;
    st.lm_trials = h_ctl->lm_trials;
    st.cholesky_failures = h_ctl->solve_failures;
    st.pcg_iterations = h_ctl->pcg_total_it;
    lap("read-back");
    st.lambda_final = h_ctl->lambda;
    ctx->ba_xch[8] = st.lm_trials;
    ctx->ba_xch[9] = st.iters_stage1 + st.iters_stage2;
    if (stats) *stats = st;
    return SVGPU_OK;
}

extern "C" {

int svgpu_local_ba(svgpu_ctx* ctx, const svgpu_ba_problem* problem, volatile uint8_t* stop, double* pose_out,
                   double* points_out, uint8_t* outlier_out, svgpu_ba_stats* stats) {
    return local_ba_impl(ctx, problem, false, 0, 1, nullptr, nullptr, stop, pose_out, points_out, outlier_out, stats);
}

// The pose optimizer's arena, described once: with `host_inputs` the input image (pos_w | uvr | inv_sigma_sq | huber, one copy from the
// page-locked staging buffer, same offsets there), then the output block (pose | result[4] | outlier flags, one copy back), then work flags.
struct PoseOptLayout {
    size_t o_pos, o_uvr, o_w, o_h, in_total;           // input image
    size_t off_result, off_outlier, out_bytes;         // output block, relative to d_out
    char *d_in, *d_out;
};
static void lay_pose_opt(Arena& A, int n, bool host_inputs, PoseOptDev& P, PoseOptLayout& Y) {
    Y.d_in = nullptr;
    Y.o_pos = Y.o_uvr = Y.o_w = Y.o_h = Y.in_total = 0;
    if (host_inputs) {
        const size_t o0 = A.off;
        Y.o_pos = 0, P.pos_w = A.take<double>(3 * (size_t)n);
        Y.o_uvr = A.off - o0, P.uvr = A.take<float>(3 * (size_t)n);
        Y.o_w = A.off - o0, P.inv_sigma_sq = A.take<float>(n);
        Y.o_h = A.off - o0, P.huber = A.take<float>(n);
        Y.in_total = A.off - o0;
        Y.d_in = (char*)P.pos_w;
    }
    const size_t o0 = A.off;
    P.pose_out = A.take<double>(12);
    Y.off_result = A.off - o0, P.result = A.take<int>(4);
    Y.off_outlier = A.off - o0, P.outlier = A.take<uint8_t>(n);
    Y.out_bytes = A.off - o0;
    Y.d_out = (char*)P.pose_out;
    P.level = A.take<uint8_t>(n);
    P.robust = A.take<uint8_t>(n);
}

// Shared tail of the two pose-optimizer entry points: arena placed, inputs already on the device (or on their way), results come back in
// ONE copy (pose | result[4] | outlier flags) through the page-locked staging buffer.
static int pose_optimize_run(svgpu_ctx* ctx, PoseOptDev& P, const PoseOptLayout& Y, const double* pose_cw, int n, const double* intrinsics, int num_trials_robust,
                             int num_trials, int num_each_iter, int reset_stop_flag_each_round, char* h_out, double* pose_out, uint8_t* outlier_flags,
                             int* num_valid, int* lm_iterations) {
    char* const d_out = Y.d_out;
    const size_t out_bytes = Y.out_bytes, off_result = Y.off_result, off_outlier = Y.off_outlier;
    hipStream_t s = ctx->stream;
    P.n = n;
    memcpy(P.intr, intrinsics, sizeof(double) * 5);
    memcpy(P.pose_in, pose_cw, sizeof(double) * 12);
    P.num_trials_robust = num_trials_robust;
    P.num_trials = num_trials;
    P.num_each_iter = num_each_iter;
    P.reset_flag_each_round = reset_stop_flag_each_round;
    P.gain_thr = 1e-3;  // terminateAction->setGainThreshold(1e-3), pose_optimizer_g2o.cc:55
    sv_pose_opt(ctx, s, P);
    SV_HIP(ctx, hipGetLastError());
    SV_HIP(ctx, hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, s));
    SV_HIP(ctx, hipStreamSynchronize(s));
    memcpy(pose_out, h_out, sizeof(double) * 12);
    const int* result = (const int*)(h_out + off_result);
    memcpy(outlier_flags, h_out + off_outlier, n);
    *num_valid = result[0];
    if (lm_iterations) *lm_iterations = result[1];
    return SVGPU_OK;
}

int svgpu_pose_optimize(svgpu_ctx* ctx, const double* pose_cw, int n, const double* pos_w, const float* uvr,
                        const float* inv_sigma_sq, const float* huber_delta, const double* intrinsics, int num_trials_robust,
                        int num_trials, int num_each_iter, int reset_stop_flag_each_round, double* pose_out,
                        uint8_t* outlier_flags, int* num_valid, int* lm_iterations) {
    if (!ctx || !pose_cw || !pose_out || !num_valid || n < 0 || num_trials_robust < 0 || num_trials < 0 || num_each_iter < 0
        || (n > 0 && (!pos_w || !uvr || !inv_sigma_sq || !huber_delta || !intrinsics || !outlier_flags)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_pose_optimize: bad arguments");
    memcpy(pose_out, pose_cw, sizeof(double) * 12);
    *num_valid = 0;
    if (lm_iterations) *lm_iterations = 0;
    for (int i = 0; i < n; ++i) outlier_flags[i] = 0;
    if (n < 5) return SVGPU_OK;  // pose_optimizer_g2o.cc:109-111
    SV_HIP(ctx, hipSetDevice(ctx->device));
    // inputs: one page-locked image in device layout (pos_w | uvr | inv_sigma_sq | huber), one copy
    PoseOptDev P;
    memset(&P, 0, sizeof(P));
    PoseOptLayout Y;
    int rc = sv_ensure_scratch(ctx, arena_measure([&](Arena& M) { lay_pose_opt(M, n, true, P, Y); }));
    if (rc) return rc;
    if ((rc = sv_ensure_stage(ctx, Y.in_total + Y.out_bytes))) return rc;
    Arena A(ctx->d_scratch, ctx->scratch_bytes);
    lay_pose_opt(A, n, true, P, Y);
    if (A.overflow) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_pose_optimize: internal arena overflow");
    char* const hs = ctx->h_stage;
    memcpy(hs + Y.o_pos, pos_w, 24 * (size_t)n);
    memcpy(hs + Y.o_uvr, uvr, 12 * (size_t)n);
    memcpy(hs + Y.o_w, inv_sigma_sq, 4 * (size_t)n);
    memcpy(hs + Y.o_h, huber_delta, 4 * (size_t)n);
    SV_HIP(ctx, hipMemcpyAsync(Y.d_in, hs, Y.in_total, hipMemcpyHostToDevice, ctx->stream));
    return pose_optimize_run(ctx, P, Y, pose_cw, n, intrinsics, num_trials_robust, num_trials, num_each_iter, reset_stop_flag_each_round, hs + Y.in_total, pose_out,
                             outlier_flags, num_valid, lm_iterations);
}

int svgpu_pose_optimize_device(svgpu_ctx* ctx, const double* pose_cw, int n, const double* pos_w_dev, const float* uvr_dev,
                               const float* inv_sigma_sq_dev, const float* huber_delta_dev, const double* intrinsics, int num_trials_robust,
                               int num_trials, int num_each_iter, int reset_stop_flag_each_round, double* pose_out,
                               uint8_t* outlier_flags, int* num_valid, int* lm_iterations) {
    if (!ctx || !pose_cw || !pose_out || !num_valid || n < 0 || num_trials_robust < 0 || num_trials < 0 || num_each_iter < 0
        || (n > 0 && (!pos_w_dev || !uvr_dev || !inv_sigma_sq_dev || !huber_delta_dev || !intrinsics || !outlier_flags)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_pose_optimize_device: bad arguments");
    memcpy(pose_out, pose_cw, sizeof(double) * 12);
    *num_valid = 0;
    if (lm_iterations) *lm_iterations = 0;
    for (int i = 0; i < n; ++i) outlier_flags[i] = 0;
    if (n < 5) return SVGPU_OK;
    SV_HIP(ctx, hipSetDevice(ctx->device));
    PoseOptDev P;
    memset(&P, 0, sizeof(P));
    PoseOptLayout Y;
    int rc = sv_ensure_scratch(ctx, arena_measure([&](Arena& M) { lay_pose_opt(M, n, false, P, Y); }));
    if (rc) return rc;
    if ((rc = sv_ensure_stage(ctx, Y.out_bytes))) return rc;
    Arena A(ctx->d_scratch, ctx->scratch_bytes);
    lay_pose_opt(A, n, false, P, Y);
    if (A.overflow) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_pose_optimize: internal arena overflow");
    P.pos_w = pos_w_dev, P.uvr = uvr_dev, P.inv_sigma_sq = inv_sigma_sq_dev, P.huber = huber_delta_dev;
    return pose_optimize_run(ctx, P, Y, pose_cw, n, intrinsics, num_trials_robust, num_trials, num_each_iter, reset_stop_flag_each_round, ctx->h_stage, pose_out,
                             outlier_flags, num_valid, lm_iterations);
}

// Several problems over one frame observation (the candidates of a relocalisation or a loop validation), one workgroup each: one upload,
// one launch, one read-back and one synchronisation per call, whatever the batch size.
int svgpu_pose_optimize_batch(svgpu_ctx* ctx, int num_problems, const int32_t* obs_off, const double* pose_cw, const uint8_t* active,
                              const double* pos_w, const float* uvr, const float* inv_sigma_sq, const float* huber_delta, const uint8_t* select,
                              const double* intrinsics, int num_trials_robust, int num_trials, int num_each_iter, int reset_stop_flag_each_round,
                              double* pose_out, uint8_t* outlier_flags, int32_t* num_valid, int32_t* lm_iterations) {
    const char* const bad = "svgpu_pose_optimize_batch: bad arguments";
    if (!ctx || num_problems < 0) return sv_set_error(ctx, SVGPU_ERR_INVALID, bad);
    if (num_problems == 0) return SVGPU_OK;
    // ---- validation: nothing is launched before all of it has passed
    if (!obs_off || !pose_cw || !pose_out || !num_valid || num_trials_robust < 0 || num_trials < 0 || num_each_iter < 0)
        return sv_set_error(ctx, SVGPU_ERR_INVALID, bad);
    const size_t P = (size_t)num_problems;
    if (!sv_offsets_ok(obs_off, num_problems)) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_pose_optimize_batch: obs_off does not start at 0 or is not monotone");
    const size_t n = (size_t)obs_off[P];
    if (n > 0 && (!pos_w || !uvr || !inv_sigma_sq || !huber_delta || !intrinsics || !outlier_flags)) return sv_set_error(ctx, SVGPU_ERR_INVALID, bad);

    PoseOptBatchPieces Y{};
    StagedCall C;
    int rc = C.open(ctx, "svgpu_pose_optimize_batch: internal arena overflow", [&](UploadArena& A) { poseopt_batch_layout(A, P, n, Y); });
    if (rc) return rc;
    C.up(Y.obs_off, obs_off), C.up(Y.pose_in, pose_cw), C.up(Y.active, active), C.up(Y.pos_w, pos_w);
    C.up(Y.uvr, uvr), C.up(Y.w, inv_sigma_sq), C.up(Y.huber, huber_delta), C.up(Y.select, select);  // active, select: optional, null is no upload
    if ((rc = C.flush())) return rc;

    PoseOptDev D;
    memset(&D, 0, sizeof(D));
    if (intrinsics) memcpy(D.intr, intrinsics, sizeof(double) * 5);
    else D.intr[0] = D.intr[1] = 1.0;  // (no entry at all: every problem is skipped)
    D.num_trials_robust = num_trials_robust, D.num_trials = num_trials, D.num_each_iter = num_each_iter;
    D.reset_flag_each_round = reset_stop_flag_each_round;
    D.gain_thr = 1e-3;  // terminateAction->setGainThreshold(1e-3), pose_optimizer_g2o.cc:55
    D.pos_w = Y.pos_w, D.uvr = Y.uvr, D.inv_sigma_sq = Y.w, D.huber = Y.huber;
    D.trk_pos = Y.c_pos, D.trk_uvr = Y.c_uvr, D.trk_w = Y.c_w, D.trk_h = Y.c_huber, D.trk_kp_of = Y.entry_of;
    D.level = Y.level, D.robust = Y.robust, D.outlier = Y.outlier;
    D.pose_in_dev = Y.pose_in, D.pose_out = Y.pose_out, D.result = Y.result;
    D.bat_off = Y.obs_off, D.bat_select = select ? Y.select : nullptr, D.bat_active = active ? Y.active : nullptr, D.bat_flags = Y.flags;
    sv_pose_opt_batch(ctx, C.s, D, num_problems);

    std::vector<int32_t> result(Y.result.n);
    C.down(pose_out, Y.pose_out), C.down(result.data(), Y.result), C.down(outlier_flags, Y.flags);
    if ((rc = C.finish())) return rc;
    for (size_t p = 0; p < P; ++p) {
        num_valid[p] = result[4 * p];
        if (lm_iterations) lm_iterations[p] = result[4 * p + 1];
    }
    return SVGPU_OK;
}

int svgpu_global_ba(svgpu_ctx* ctx, const svgpu_ba_problem* problem, volatile uint8_t* stop, double* pose_out, double* points_out,
                    svgpu_ba_stats* stats) {
    return local_ba_impl(ctx, problem, true, 0, 1, nullptr, nullptr, stop, pose_out, points_out, nullptr, stats);
}

int svgpu_local_ba_sharded(svgpu_ctx* ctx, const svgpu_ba_problem* shard, int rank, int world, svgpu_allreduce_fn allreduce,
                           void* allreduce_user, volatile uint8_t* stop, double* pose_out, double* points_out,
                           uint8_t* outlier_out, svgpu_ba_stats* stats) {
    if (!ctx) return SVGPU_ERR_INVALID;
    if (!allreduce) {  // the context's own RCCL communicator (svgpu_comm_init)
        if (!ctx->comm) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_local_ba_sharded: no all-reduce callback and no communicator (svgpu_comm_init)");
        if (rank != ctx->comm_rank || world != ctx->comm_world) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_local_ba_sharded: rank / world differ from the communicator's");
        allreduce = rccl_allreduce_cb;
        allreduce_user = ctx;
    }
    return local_ba_impl(ctx, shard, false, rank, world, allreduce, allreduce_user, stop, pose_out, points_out, outlier_out, stats);
}

int svgpu_global_ba_sharded(svgpu_ctx* ctx, const svgpu_ba_problem* shard, int rank, int world, svgpu_allreduce_fn allreduce,
                            void* allreduce_user, volatile uint8_t* stop, double* pose_out, double* points_out, svgpu_ba_stats* stats) {
    if (!ctx) return SVGPU_ERR_INVALID;
    if (!allreduce) {
        if (!ctx->comm) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_global_ba_sharded: no all-reduce callback and no communicator (svgpu_comm_init)");
        if (rank != ctx->comm_rank || world != ctx->comm_world) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_global_ba_sharded: rank / world differ from the communicator's");
        allreduce = rccl_allreduce_cb;
        allreduce_user = ctx;
    }
    return local_ba_impl(ctx, shard, true, rank, world, allreduce, allreduce_user, stop, pose_out, points_out, nullptr, stats);
}

int svgpu_ba_last_exchange(svgpu_ctx* ctx, int64_t* info) {
    if (!ctx || !info) return SVGPU_ERR_INVALID;
    for (int k = 0; k < 10; ++k) info[k] = ctx->ba_xch[k];
    return SVGPU_OK;
}

int svgpu_ba_last_solver(svgpu_ctx* ctx, int* solver) {
    if (!ctx || !solver) return SVGPU_ERR_INVALID;
    *solver = ctx->ba_last_solver;
    return SVGPU_OK;
}

// include/svgpu.h.  The block pattern is built the way the solve builds it (a kept block (a, b) = a free landmark observed from the free
// keyframes a and b; every diagonal block), the cuts come from the solve's own planner (sv_sky_partition_roles).
int svgpu_ba_partition_keyframe_segments(const svgpu_ba_problem* pr, int world, int32_t* landmark_rank, int32_t* info) {
    if (!pr || !landmark_rank || !info || world < 1) return SVGPU_ERR_INVALID;
    const BaEnv env = ba_env();
    const int P = pr->num_poses, L = pr->num_points, E = pr->num_obs;
    for (int k = 0; k < 12; ++k) info[k] = 0;
    for (int l = 0; l < L; ++l) landmark_rank[l] = l % world;
    if (P <= 0 || L <= 0 || E <= 0 || world == 1) return SVGPU_OK;
    for (int e = 0; e < E; ++e)
        if (pr->obs_pose[e] < 0 || pr->obs_pose[e] >= P || pr->obs_point[e] < 0 || pr->obs_point[e] >= L) return SVGPU_ERR_INVALID;
    // free keyframes with an observation, numbered in pose order (activity_only above)
    std::vector<uint8_t> seen(P, 0);
    for (int e = 0; e < E; ++e) seen[pr->obs_pose[e]] = 1;
    std::vector<int> slot(P, -1);
    int nP = 0;
    for (int p = 0; p < P; ++p)
        if (seen[p] && !pr->pose_fixed[p]) slot[p] = nP++;
    info[6] = nP;
    if (nP < 4 || nP > 32768) return SVGPU_OK;  // (the pattern below is a dense BIT table, nP^2 / 8 bytes: 32 MB at 16 384 free keyframes, 128 MB at the 32 768 cap; the a/b scan behind it is O(nP^2); larger graphs keep the whole problem in one segment)
    // observations grouped by landmark
    std::vector<int> off(L + 1, 0), obs(E);
    for (int e = 0; e < E; ++e) ++off[pr->obs_point[e] + 1];
    for (int l = 0; l < L; ++l) off[l + 1] += off[l];
    {
        std::vector<int> fill(off.begin(), off.end() - 1);
        for (int e = 0; e < E; ++e) obs[fill[pr->obs_point[e]]++] = slot[pr->obs_pose[e]];
    }
    std::vector<uint64_t> present(((size_t)nP * nP + 63) / 64, 0);
    auto mark = [&](size_t k) { present[k >> 6] |= 1ull << (k & 63); };
    auto marked = [&](size_t k) -> bool { return (present[k >> 6] >> (k & 63)) & 1ull; };
    for (int l = 0; l < L; ++l) {
        if (pr->point_fixed && pr->point_fixed[l]) continue;
        for (int i = off[l]; i < off[l + 1]; ++i) {
            const int a = obs[i];
            if (a < 0) continue;
            for (int j = i + 1; j < off[l + 1]; ++j) {
                const int b = obs[j];
                if (b >= 0) mark((size_t)std::min(a, b) * nP + std::max(a, b));
            }
        }
    }
    std::vector<int2> blk_ab;
    for (int a = 0; a < nP; ++a)
        for (int b = a; b < nP; ++b)
            if (a == b || marked((size_t)a * nP + b)) {
                int2 ab;
                ab.x = a, ab.y = b;
                blk_ab.push_back(ab);
            }
    info[7] = (int)blk_ab.size();
    std::vector<int> job_of, owner;
    int ncuts = 0, sep_blocks_n = 0;
    long long xch_doubles = 0;
    if (!sv_sky_partition_roles(nP, blk_ab, world, env, job_of, owner, &ncuts, &sep_blocks_n, &xch_doubles)) return SVGPU_OK;
    // a landmark follows the piece of its keyframes.  (A FIXED landmark couples nothing and may be seen from two pieces: its observations
    // cannot be placed on one rank without feeding a foreign piece's pose blocks -- such a problem keeps l % world.)
    std::vector<int32_t> lr(L);
    int shared = 0, sep_only = 0;
    for (int l = 0; l < L; ++l) {
        int job = -1, on_sep = 0;
        for (int i = off[l]; i < off[l + 1]; ++i) {
            const int a = obs[i];
            if (a < 0) continue;
            if (job_of[a] < 0) on_sep = 1;
            else if (job < 0) job = job_of[a];
            else if (job != job_of[a]) return SVGPU_OK;
        }
        lr[l] = job >= 0 ? owner[job] : l % world;
        shared += on_sep;
        sep_only += on_sep && job < 0;
    }
    for (int l = 0; l < L; ++l) landmark_rank[l] = lr[l];
    int nsep = 0;
    for (int a = 0; a < nP; ++a) nsep += job_of[a] < 0;
    info[0] = 1, info[1] = (int)owner.size(), info[2] = ncuts, info[3] = nsep, info[4] = shared, info[5] = sep_only;
    info[8] = sep_blocks_n, info[9] = (int32_t)std::min<long long>(xch_doubles, 0x7fffffff);
    return SVGPU_OK;
}

int svgpu_ba_set_solver(svgpu_ctx* ctx, int solver, double pcg_tolerance, int pcg_max_iterations) {
    if (!ctx || solver < SVGPU_BA_SOLVER_AUTO || (solver > SVGPU_BA_SOLVER_PCG_MULTI && solver != SVGPU_BA_SOLVER_ENVELOPE && solver != SVGPU_BA_SOLVER_CHOLESKY_MFMA)) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_ba_set_solver: bad solver");
    ctx->ba_solver = solver;
    ctx->pcg_tol = pcg_tolerance > 0 ? pcg_tolerance : 1e-10;
    ctx->pcg_max_it = pcg_max_iterations > 0 ? pcg_max_iterations : 0;
    return SVGPU_OK;
}

int svgpu_comm_unique_id(uint8_t* id128) {
    if (!id128) return SVGPU_ERR_INVALID;
    if (!rccl_ready()) return SVGPU_ERR_HIP;
    NcclId id;
    if (g_rccl.get_unique_id(&id) != 0) return SVGPU_ERR_HIP;
    memcpy(id128, id.internal, 128);
    return SVGPU_OK;
}

int svgpu_comm_init(svgpu_ctx* ctx, int rank, int world, const uint8_t* id128) {
    if (!ctx || !id128 || world < 1 || rank < 0 || rank >= world) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_comm_init: bad arguments");
    if (!rccl_ready()) return sv_set_error(ctx, SVGPU_ERR_HIP, "svgpu_comm_init: librccl.so could not be loaded");
    SV_HIP(ctx, hipSetDevice(ctx->device));
    sv_comm_release(ctx);
    NcclId id;
    memcpy(id.internal, id128, 128);
    const int r = g_rccl.comm_init_rank(&ctx->comm, world, id, rank);
    if (r != 0) {
        ctx->comm = nullptr;
        return sv_set_error(ctx, SVGPU_ERR_HIP, g_rccl.get_error_string ? g_rccl.get_error_string(r) : "ncclCommInitRank failed");
    }
    ctx->comm_rank = rank;
    ctx->comm_world = world;
    return SVGPU_OK;
}

void svgpu_comm_destroy(svgpu_ctx* ctx) { sv_comm_release(ctx); }

int svgpu_comm_allreduce_f64(svgpu_ctx* ctx, double* dev_buf, size_t count, void* stream) {
    if (!ctx || !ctx->comm) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_comm_allreduce_f64: no communicator");
    return rccl_allreduce_cb(ctx, dev_buf, count, stream ? stream : (void*)ctx->stream) == 0 ? SVGPU_OK : sv_set_error(ctx, SVGPU_ERR_HIP, "ncclAllReduce failed");
}

}  // extern "C"
