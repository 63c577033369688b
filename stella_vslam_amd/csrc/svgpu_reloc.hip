// svgpu_reloc_refine_batch: module::relocalizer::refine_pose (module/relocalizer.cc:236-297) for all candidates in one staged call.
// Per stage: reprojection of every candidate's still-valid keyframe entries from the candidate's own pose in device memory -> the grid
// walk over the ONE binned frame (all candidates' entries are one concatenation of queries) -> distances and one replay workgroup per
// candidate (k_cand_dist_batch / k_cand_replay_batch) -> the matches are applied to the candidate's landmark state -> the count decision
// -> k_pose_opt_batch over every keypoint that holds a landmark (its `select` compaction is the gather, in keypoint order).  The kernels
// of this file are the glue the per-call path does on the host; the matcher and the optimiser are the existing ones.
#include "svgpu_match_common.h"
#include "reloc_refine_layout.h"
#include "reloc_solve_layout.h"
#include "pnp_kernels.h"
#include "sv_wave.h"
#include "ba_kernels.h"
#include "frame_device.h"
#include "sv_sort.h"
#include "sv_validate.h"

using namespace svm;

namespace {

#define RR_MAX_STAGES 4

// ---- reprojection of all candidates' entries: k_can_observe's body (svfd::reproject_one / reproject_window) with the pose, and the camera
// centre the single call derives from it on the host (cam_center, svgpu_match2.hip), read from candidate p's row of `pose`.  The centre equals
// the host's bit for bit only while this file is compiled without contraction, as the library's flags have it (-ffp-contract=off): a
// fused multiply-add in the three sums below would round differently from cam_center.
struct RelocReproj {
    ReprojProblem R;             // camera, modes, margin and scale factors of the stage; R.n = all entries
    const int32_t* kf_off;       // K + 1
    int K;
    const double* pose;          // K x 12 rows of [R|t]: the stage's input poses
    const uint8_t* active;       // K
    const uint8_t* valid;        // per entry
};
__global__ void __launch_bounds__(256) k_reloc_reproject(RelocReproj Q) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Q.R.n) return;
    const int p = sv_segment_of(Q.kf_off, Q.K, i);
    const bool offered = Q.active[p] && Q.valid[i];
    const double* __restrict__ T = Q.pose + 12 * (size_t)p;
    double rot[9], trans[3], center[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        rot[3 * r] = T[4 * r], rot[3 * r + 1] = T[4 * r + 1], rot[3 * r + 2] = T[4 * r + 2];
        trans[r] = T[4 * r + 3];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) center[r] = ((-rot[r]) * trans[0] + (-rot[3 + r]) * trans[1]) + (-rot[6 + r]) * trans[2];  // projection.cc:223
    svfd::ReprojOut o;
    svfd::reproject_one(Q.R, rot, trans, center, offered, Q.R.pos_w[3 * (size_t)i], Q.R.pos_w[3 * (size_t)i + 1], Q.R.pos_w[3 * (size_t)i + 2], 0.0, 0.0, 0.0,
                        Q.R.min_valid_dist[i], Q.R.max_valid_dist[i], 0, false, o);
    Q.R.visible[i] = o.vis ? 1 : 0;
    svfd::reproject_window(Q.R, o, Q.R.q_xy[2 * (size_t)i], Q.R.q_xy[2 * (size_t)i + 1], Q.R.q_margin[i], Q.R.q_min_level[i], Q.R.q_max_level[i]);
}

// ---- the observation arrays of the pose optimiser, one entry per (candidate, keypoint): what the per-call adaptor gathers on the host
// (pose_optimizer_g2o.cc:86-109): uvr from the undistorted keypoint and x_right (-1 without), the weight by octave, one Huber delta
struct RelocObs {
    int nt, entries;  // entries = K x nt
    const float* t_xy;
    const float* t_xright;  // nullable
    const int32_t* t_octave;
    float inv_level_sigma_sq[SV_MAX_LEVELS];
    float huber_delta;
    float* uvr;
    float* w;
    float* huber;
    int N, K;
    const uint8_t* active;  // K
    int32_t* status;        // K
    int32_t* match_kf;      // N
    int32_t* match_stage;   // N
};
__global__ void __launch_bounds__(256) k_reloc_observations(RelocObs O) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    // (the same launch starts the results that live beside one another at the arena's end: nothing matched yet, status by the input flag)
    if (e < O.N) O.match_kf[e] = O.match_stage[e] = -1;
    if (e < O.K) O.status[e] = O.active[e] ? 0 : -1;
    if (e >= O.entries) return;
    const int t = e % O.nt;
    O.uvr[3 * (size_t)e] = O.t_xy[2 * t];
    O.uvr[3 * (size_t)e + 1] = O.t_xy[2 * t + 1];
    O.uvr[3 * (size_t)e + 2] = O.t_xright ? O.t_xright[t] : -1.0f;
    O.w[e] = O.inv_level_sigma_sq[O.t_octave[t]];
    O.huber[e] = O.huber_delta;
}

// ---- a stage's matches enter the candidate's state: the entry is spent, its keypoint holds the entry's landmark from now on.  The replay
// gives a keypoint to at most one entry of a candidate, so no two threads write the same keypoint.
struct RelocApply {
    int N, K, nt, stage;
    const int32_t* kf_off;
    const int32_t* match_q;  // the stage's result per entry
    const double* pos_w;
    uint8_t* valid;
    uint8_t* occupied;       // K x nt
    double* lm_pos;          // K x nt x 3
    int32_t* match_kf;
    int32_t* match_stage;
};
__global__ void __launch_bounds__(256) k_reloc_apply(RelocApply A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.N) return;
    const int m = A.match_q[i];
    if (m < 0) return;
    const int p = sv_segment_of(A.kf_off, A.K, i);
    const size_t e = (size_t)p * A.nt + m;
    A.match_kf[i] = m;
    A.match_stage[i] = A.stage;
    A.valid[i] = 0;
    A.occupied[e] = 1;
    A.lm_pos[3 * e] = A.pos_w[3 * (size_t)i];
    A.lm_pos[3 * e + 1] = A.pos_w[3 * (size_t)i + 1];
    A.lm_pos[3 * e + 2] = A.pos_w[3 * (size_t)i + 2];
}

// ---- the count decisions.  stage < S: in front of the optimisation of `stage`, count = what the previous optimisation left valid
// (n_already_found in front of the first); stage == S: the final test.  A failed candidate's flag is cleared: every later kernel's
// workgroups of that candidate leave as a whole.
struct RelocDecide {
    int K, S, stage, min_num_valid_obs;
    const int32_t* count0;     // K
    const int32_t* num_found;  // K x S
    const int32_t* result;     // S x K x 4 ([0] = num_valid)
    uint8_t* active;
    int32_t* status;
};
__global__ void __launch_bounds__(256) k_reloc_decide(RelocDecide D) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= D.K || !D.active[p]) return;
    const int count = D.stage == 0 ? D.count0[p] : D.result[((size_t)(D.stage - 1) * D.K + p) * 4];
    const int c = D.stage < D.S ? count + D.num_found[(size_t)p * D.S + D.stage] : count;
    if (c < D.min_num_valid_obs) {
        D.status[p] = 1 + D.stage;
        D.active[p] = 0;
    }
}

struct Tally {  // what the call issues (svgpu_call_stats)
    int launches = 0, copies = 0, syncs = 0;
    void add(const SvIssued& n) { launches += n.launches, copies += n.copies; }  // what a shared launcher says it issued
};

// A candidate's chain without a frame keypoint: nothing can match and nothing is optimised (fewer than 5 observations)
void refine_without_keypoints(int K, int S, const uint8_t* active, const double* pose_cw, const int32_t* n_already_found, int min_num_valid_obs,
                              int32_t* status, double* pose_out, int32_t* num_found, int32_t* num_valid, int32_t* lm_iterations) {
    for (int p = 0; p < K; ++p) {
        std::memcpy(pose_out + 12 * (size_t)p, pose_cw + 12 * (size_t)p, 12 * sizeof(double));
        for (int s = 0; s < S; ++s) num_found[(size_t)p * S + s] = num_valid[(size_t)p * S + s] = 0;
        if (lm_iterations) lm_iterations[p] = 0;
        if (active && !active[p]) {
            status[p] = -1;
            continue;
        }
        int count = n_already_found[p], st = 0;
        for (int s = 0; s < S && !st; ++s) {
            if (count < min_num_valid_obs) st = 1 + s;
            count = 0;  // the optimisation is skipped: num_valid = 0
        }
        if (!st && count < min_num_valid_obs) st = 1 + S;
        status[p] = st;
    }
}


// ================================================================================================ svgpu_reloc_solve_batch
// What the call adds in front of the stages: per 2D-3D match entry the inputs of PnP and of the first optimisation are gathered from the
// frame's arrays by the entry's keypoint (k_reloc_solve_gather); behind PnP (pnp_kernels.hip) and k_pose_opt_batch the bookkeeping of
// relocalizer::reloc_by_candidate (module/relocalizer.cc:103-123) turns their flags into the state the stages start from
// (k_reloc_solve_book).  Every index either kernel dereferences was checked on the host before the launch.
struct SolveCall {  // what svgpu_reloc_solve_batch passes beside the refine call's arguments
    const double* t_bearings;
    const int32_t* match_off;
    const int32_t* m_keypt;
    const double* m_pos_w;
    const int32_t* m_kf_entry;
    int min_num_inliers, num_iter;
    const uint32_t* samples;
    int recompute, gn_iter;
    int min_num_opt_valid_obs;  // the threshold of relocalizer::optimize_pose (min_num_bow_matches_ / 2, :220)
    uint8_t* pnp_valid;
    double* pnp_pose_cw;
    uint8_t* is_inlier;
    int32_t* best_iter;
    double* opt_pose;
    uint8_t* opt_outlier;
    int32_t* opt_num_valid;
};

// One thread per match entry: bearing, max_cos_errors_ by octave (pnp_solver.cc:27-32; the table per level is the host's, so the float is
// the one svgpu_pnp_ransac uploads), and the observation of pose_optimizer_g2o.cc:86-109 as k_reloc_observations writes it per keypoint.
// The same launch starts PnP's results for the problems that do not run: invalid, pose 0, no inlier, best_iter -1.
struct SolveGather {
    int M, K;
    const int32_t* m_keypt;
    const double* t_bearings;
    const float* t_xy;
    const float* t_xright;  // nullable
    const int32_t* t_octave;
    float max_cos_level[SV_MAX_LEVELS];
    float inv_level_sigma_sq[SV_MAX_LEVELS];
    float huber_delta;
    double* bearings;
    float* max_cos;
    float* uvr;
    float* w;
    float* huber;
    uint8_t* pnp_valid;
    double* pnp_pose;
    uint8_t* is_inlier;
    int32_t* best_iter;
};
__global__ void __launch_bounds__(256) k_reloc_solve_gather(SolveGather G) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < G.K) G.pnp_valid[e] = 0, G.best_iter[e] = -1;
    if (e < 12 * G.K) G.pnp_pose[e] = 0.0;
    if (e >= G.M) return;
    const int t = G.m_keypt[e];
    const int oct = G.t_octave[t];
    const double bx = G.t_bearings[3 * (size_t)t], by = G.t_bearings[3 * (size_t)t + 1], bz = G.t_bearings[3 * (size_t)t + 2];
    const float x = G.t_xy[2 * (size_t)t], y = G.t_xy[2 * (size_t)t + 1];
    const float xr = G.t_xright ? G.t_xright[t] : -1.0f;
    G.bearings[3 * (size_t)e] = bx, G.bearings[3 * (size_t)e + 1] = by, G.bearings[3 * (size_t)e + 2] = bz;
    G.max_cos[e] = G.max_cos_level[oct];
    G.uvr[3 * (size_t)e] = x, G.uvr[3 * (size_t)e + 1] = y, G.uvr[3 * (size_t)e + 2] = xr;
    G.w[e] = G.inv_level_sigma_sq[oct];
    G.huber[e] = G.huber_delta;
    G.is_inlier[e] = 0;
}

// One workgroup per candidate.  A candidate that was active on input stops here with SVGPU_RELOC_PNP_FAILED (PnP not valid) or
// SVGPU_RELOC_OPTIMIZE_FAILED (num_valid of the first optimisation below the threshold, relocalizer.cc:216-223); else every match that is a
// PnP inlier (:104-108) and no outlier of the optimisation (:225-231) gives its keypoint the landmark, and the keyframe entry it names is spent
// (already_found_landmarks, :116-123).  m_keypt is strictly ascending and the m_kf_entry >= 0 are distinct inside a candidate, so no two
// threads write one place.  n_already_found is ONE sum in a fixed order: per round of 256 entries the wave prefix sums (sv_wave.h), the
// four wave totals through LDS (double-buffered: one barrier per round), rounds in entry order.
struct SolveBook {
    int K, nt, min_num_valid_obs;
    const int32_t* match_off;
    const int32_t* kf_off;
    const int32_t* m_keypt;
    const int32_t* m_kf_entry;
    const double* m_pos_w;
    const uint8_t* pnp_valid;
    const uint8_t* is_inlier;
    const uint8_t* opt_flags;
    const int32_t* opt_result;  // K x 4 ([0] = num_valid)
    uint8_t* active;
    int32_t* status;
    int32_t* count0;
    uint8_t* occupied;  // K x nt, zero on entry
    double* lm_pos;     // K x nt x 3
    uint8_t* valid;     // per keyframe entry
};
__global__ void __launch_bounds__(256) k_reloc_solve_book(SolveBook B) {
    __shared__ int s_wave[2][4];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool was_active = B.active[p] != 0;
    __syncthreads();  // (thread 0 clears the flag below: every thread has read it)
    if (!was_active) return;
    const int st = !B.pnp_valid[p] ? SVGPU_RELOC_PNP_FAILED : (B.opt_result[4 * (size_t)p] < B.min_num_valid_obs ? SVGPU_RELOC_OPTIMIZE_FAILED : 0);
    if (st) {  // the whole workgroup leaves
        if (tid == 0) B.status[p] = st, B.active[p] = 0;
        return;
    }
    const int lo = B.match_off[p], n = B.match_off[p + 1] - lo;
    const size_t row = (size_t)p * B.nt, kf0 = (size_t)B.kf_off[p];
    int total = 0;
    for (int base = 0, par = 0; base < n; base += 256, par ^= 1) {
        const int i = base + tid;
        const size_t e = (size_t)lo + i;
        const bool held = i < n && B.is_inlier[e] && !B.opt_flags[e];
        const int incl = sv_wave_inclusive_sum<int>(held ? 1 : 0);
        if (lane == 63) s_wave[par][wave] = incl;
        __syncthreads();
        total += (s_wave[par][0] + s_wave[par][1]) + (s_wave[par][2] + s_wave[par][3]);
        if (held) {
            const size_t k = row + B.m_keypt[e];
            const int ke = B.m_kf_entry[e];
            const double x = B.m_pos_w[3 * e], y = B.m_pos_w[3 * e + 1], z = B.m_pos_w[3 * e + 2];
            B.occupied[k] = 1;
            B.lm_pos[3 * k] = x, B.lm_pos[3 * k + 1] = y, B.lm_pos[3 * k + 2] = z;
            if (ke >= 0) B.valid[kf0 + ke] = 0;
        }
    }
    if (tid == 0) B.count0[p] = total;
}

// nt == 0 leaves no match entry (every m_keypt would lie outside the frame): PnP runs for nobody
void solve_without_keypoints(int K, int S, size_t N, const uint8_t* active, const SolveCall& V, int32_t* status, double* pose_out, int32_t* match_kf,
                             int32_t* match_stage, int32_t* num_found, int32_t* num_valid, int32_t* lm_iterations) {
    for (int p = 0; p < K; ++p) {
        status[p] = (active && !active[p]) ? -1 : SVGPU_RELOC_PNP_FAILED;
        V.pnp_valid[p] = 0, V.best_iter[p] = -1, V.opt_num_valid[p] = 0;
        std::memset(V.pnp_pose_cw + 12 * (size_t)p, 0, 96), std::memset(V.opt_pose + 12 * (size_t)p, 0, 96), std::memset(pose_out + 12 * (size_t)p, 0, 96);
        for (int s = 0; s < S; ++s) num_found[(size_t)p * S + s] = num_valid[(size_t)p * S + s] = 0;
        if (lm_iterations) lm_iterations[p] = 0;
    }
    for (size_t i = 0; i < N; ++i) match_kf[i] = match_stage[i] = -1;
}

// The body of both entry points: `V` null is svgpu_reloc_refine_batch; else the steps of svgpu_reloc_solve_batch run in front of the stages,
// which then take pose, n_already_found, frame_has_lm, frame_lm_pos_w and the cleared `valid` bytes from the device (their host arguments are null).
int reloc_call(const char* const who, const SolveCall* const V, svgpu_ctx* ctx, const svgpu_camera* cam, const uint8_t* tdesc, const float* t_xy, const int32_t* t_octave,
                                        const float* t_angle, const float* t_xright, int nt, int grid_cols, int grid_rows, int num_levels,
                                        const float* scale_factors, const float* inv_level_sigma_sq, float log_scale_factor, const double* intrinsics,
                                        int num_trials_robust, int num_trials, int num_each_iter, int reset_stop_flag_each_round, int check_orientation,
                                        int num_candidates, const uint8_t* active, const double* pose_cw, const int32_t* n_already_found,
                                        const uint8_t* frame_has_lm, const double* frame_lm_pos_w, const int32_t* kf_off, const double* pos_w,
                                        const uint8_t* valid, const float* min_valid_dist, const float* max_valid_dist, const uint8_t* lm_desc,
                                        const float* angle_kf, int num_stages, const float* margin, const int32_t* hamm_dist_thr, int min_num_valid_obs,
                                        int32_t* status, double* pose_out, int32_t* match_kf, int32_t* match_stage, uint8_t* outlier,
                                        int32_t* num_found, int32_t* num_valid, int32_t* lm_iterations, svgpu_call_stats* stats) {
    const std::string bad_s = std::string(who) + ": bad arguments";
    const char* const bad = bad_s.c_str();
    auto fail = [&](const char* what) { return sv_set_error(ctx, SVGPU_ERR_INVALID, (std::string(who) + what).c_str()); };
    if (!ctx || num_candidates < 0) return sv_set_error(ctx, SVGPU_ERR_INVALID, bad);
    if (num_candidates == 0) {
        if (stats) *stats = svgpu_call_stats{0, 0, 0};
        return SVGPU_OK;
    }
    // ---- validation: every index a kernel dereferences is checked here; nothing is launched or written before all of it has passed
    const int K = num_candidates, S = num_stages;
    if (!cam || cam->model < SVGPU_CAM_PERSPECTIVE || cam->model > SVGPU_CAM_RADIAL_DIVISION || S < 1 || S > RR_MAX_STAGES || num_levels < 1
        || num_levels > SV_MAX_LEVELS || !scale_factors || !inv_level_sigma_sq || !(log_scale_factor > 0.f) || !intrinsics || num_trials_robust < 0
        || num_trials < 0 || num_each_iter < 0 || nt < 0 || nt >= (1 << 22) || grid_cols < 1 || grid_rows < 1
        || (size_t)grid_cols * grid_rows > (size_t(1) << 22) || !(cam->min_x < cam->max_x) || !(cam->min_y < cam->max_y) || (!V && (!pose_cw || !n_already_found))
        || !kf_off || !margin || !hamm_dist_thr || !status || !pose_out || !num_found || !num_valid
        || (nt > 0 && (!tdesc || !t_xy || !t_octave || (check_orientation && !t_angle) || (!V && (!frame_has_lm || !frame_lm_pos_w)) || !outlier)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, bad);
    if (!sv_offsets_ok(kf_off, K)) return fail(": kf_off does not start at 0 or is not monotone");
    const size_t N = (size_t)kf_off[K], E = (size_t)K * (size_t)nt, lim = (size_t)INT32_MAX;
    if (N > 0 && (!pos_w || !min_valid_dist || !max_valid_dist || !lm_desc || (check_orientation && !angle_kf) || !match_kf || !match_stage))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, bad);
    if (N * 8 > lim || E * 4 > lim || E * (size_t)S > lim) return fail(": totals do not fit int32");
    for (int t = 0; t < nt; ++t)
        if (t_octave[t] < 0 || t_octave[t] >= num_levels) return fail(": octave out of range");
    for (int s = 0; s < S; ++s)
        if (hamm_dist_thr[s] < 0) return sv_set_error(ctx, SVGPU_ERR_INVALID, bad);

    if (nt == 0) {
        if (V) solve_without_keypoints(K, S, N, active, *V, status, pose_out, match_kf, match_stage, num_found, num_valid, lm_iterations);
        else refine_without_keypoints(K, S, active, pose_cw, n_already_found, min_num_valid_obs, status, pose_out, num_found, num_valid, lm_iterations);
        for (size_t i = 0; i < N; ++i) match_kf[i] = match_stage[i] = -1;
        if (stats) *stats = svgpu_call_stats{0, 0, 0};
        return SVGPU_OK;
    }

    RelocRefineShape H;
    H.K = (size_t)K, H.nt = (size_t)nt, H.N = N, H.S = (size_t)S, H.ncell = (size_t)grid_cols * grid_rows;
    H.has_angle = t_angle != nullptr, H.has_xright = t_xright != nullptr, H.has_kf_angle = angle_kf != nullptr;
    H.cand_rec = sizeof(CandProblem), H.replay_rec = sizeof(CandBatchReplay);
    // the form of every candidate's replay (sv_cand_replay_form decides, as for the single call), and the dynamic LDS of the one launch
    std::vector<int> form((size_t)K);
    size_t lds_bytes = 0;
    for (int p = 0; p < K; ++p) {
        const int nq = kf_off[p + 1] - kf_off[p];
        form[p] = sv_cand_replay_form(nq, nt, false, SVGPU_MATCH_BEST_ONLY);
        if (form[p] < 0) H.global_replay = true;
        else lds_bytes = std::max(lds_bytes, sv_cand_lds_bytes(nq, nt, form[p]));
    }
    constexpr float chi_sq_2D = 5.99146, chi_sq_3D = 7.81473;  // pose_optimizer_g2o.cc:98-105
    const float huber_delta = t_xright ? std::sqrt(chi_sq_3D) : std::sqrt(chi_sq_2D);

    // (solve) the candidates whose PnP runs (pnp_solver.cc:49-52, and not those inactive on input), max_cos_errors_ per level
    const size_t M = V ? (size_t)V->match_off[K] : 0;
    std::vector<int32_t> pnp_active;
    float max_cos_level[SV_MAX_LEVELS] = {};
    if (V) {
        for (int p = 0; p < K; ++p) {
            const unsigned np = (unsigned)(V->match_off[p + 1] - V->match_off[p]);
            if ((!active || active[p]) && np >= 4u && np >= (unsigned)V->min_num_inliers) pnp_active.push_back(p);
        }
        for (int l = 0; l < num_levels; ++l) max_cos_level[l] = sv_pnp_max_cos(scale_factors[l]);
    }

    H.cap = std::max<size_t>(4096, N * 64);
    std::vector<CandProblem> cand_tab((size_t)S * K);
    std::vector<CandBatchReplay> replay_tab((size_t)K);
    std::vector<int32_t> result, opt_result;
    std::vector<uint8_t> flags;
    const std::string overflow_s = std::string(who) + ": internal arena overflow";
    Tally T;
    for (int attempt = 0; attempt <= S + 1; ++attempt) {  // (a stage whose lists outgrow the capacity starts the call again: at most once per stage)
        RelocSolvePieces Z{};
        RelocRefinePieces& Y = Z.refine;
        RelocSolveShape HS;
        HS.refine = H;
        if (V) HS.M = M, HS.I = (size_t)V->num_iter, HS.num_active = pnp_active.size(), HS.recompute = V->recompute != 0;
        StagedCall C;
        int rc = C.open(ctx, overflow_s.c_str(), [&](UploadArena& A) {
            if (V) reloc_solve_layout(A, HS, Z);
            else reloc_refine_layout(A, H, Y);
        });
        if (rc) return rc;
        // ---- one upload: the frame, the candidates' state, the entries, the tables
        C.up(Y.tdesc, tdesc, Y.t_xy, t_xy, Y.t_octave, t_octave, Y.t_angle, t_angle, Y.t_xright, t_xright);
        C.up(Y.pose_in, pose_cw, Y.count0, n_already_found, Y.occupied, frame_has_lm, Y.lm_pos, frame_lm_pos_w, Y.kf_off, kf_off);
        if (V) {  // (no keypoint holds a landmark before the bookkeeping kernel says so)
            C.up(Z.t_bearings, V->t_bearings, Z.m_keypt, V->m_keypt, Z.m_kf_entry, V->m_kf_entry, Z.pnp.pos_w, V->m_pos_w);
            C.up(Z.pnp.match_off, V->match_off, Z.pnp.samples, V->samples, Z.pnp.active, (const int32_t*)pnp_active.data());
            std::memset(C.stage(Y.occupied), 0, Y.occupied.bytes());
        }
        C.up(Y.pos_w, pos_w, Y.min_d, min_valid_dist, Y.max_d, max_valid_dist, Y.kf_angle, angle_kf, Y.lm_desc, lm_desc);
        {
            uint8_t* const h_active = C.stage(Y.active);
            int32_t* const h_obs_off = C.stage(Y.obs_off);
            for (int p = 0; p < K; ++p) {
                h_active[p] = (!active || active[p]) ? 1 : 0;
                h_obs_off[p] = (int32_t)((size_t)p * nt);
            }
            h_obs_off[K] = (int32_t)E;
            if (N > 0) {
                uint8_t* const h_valid = C.stage(Y.valid);
                for (size_t i = 0; i < N; ++i) h_valid[i] = (!valid || valid[i]) ? 1 : 0;
            }
        }
        for (int s = 0; s < S; ++s)
            for (int p = 0; p < K; ++p) {
                const size_t r0 = (size_t)kf_off[p];
                CandProblem& P = cand_tab[(size_t)s * K + p];
                P = CandProblem{};
                P.qdesc = (const uint32_t*)Y.lm_desc.p + r0 * 8, P.tdesc = (const uint32_t*)Y.tdesc.p;
                P.t_octave = Y.t_octave, P.t_xy = Y.t_xy;
                P.nq = kf_off[p + 1] - kf_off[p], P.nt = nt;
                // (offsets into the ONE pair of lists: a candidate's nq + 1 entries end where the next candidate's begin; the scan runs over
                // the whole piece, G.cand_off below, whose start is aligned -- an offset part need not be)
                P.cand_off = Y.cand_off.p + r0, P.cand_idx = Y.cand_idx;
                P.q_valid = Y.visible.p + r0, P.occupied = Y.occupied.p + (size_t)p * nt;
                P.q_angle = Y.kf_angle.p ? Y.kf_angle.p + r0 : nullptr, P.t_angle = Y.t_angle;
                P.check_orientation = check_orientation, P.thr = (unsigned)hamm_dist_thr[s], P.lowe_ratio = 0.f, P.mode = SVGPU_MATCH_BEST_ONLY;
                P.dist = Y.dist, P.match_q = Y.match_q.p + r0, P.num = Y.num_found.p + (size_t)p * S + s;
                if (s == 0)
                    replay_tab[p] = CandBatchReplay{form[p], form[p] < 0 ? Y.owner.p + (size_t)p * nt : nullptr, form[p] < 0 ? Y.match_of_row.p + r0 : nullptr};
            }
        C.up(Y.cand_tab, (const char*)cand_tab.data(), Y.replay_tab, (const char*)replay_tab.data());
        if ((rc = C.flush())) return rc;
        ++T.copies;

        // ---- once per call: the observation arrays, the frame's grid
        {
            RelocObs O{};
            O.nt = nt, O.entries = (int)E, O.t_xy = Y.t_xy, O.t_xright = Y.t_xright, O.t_octave = Y.t_octave, O.huber_delta = huber_delta;
            for (int l = 0; l < num_levels; ++l) O.inv_level_sigma_sq[l] = inv_level_sigma_sq[l];
            O.uvr = Y.uvr, O.w = Y.w, O.huber = Y.huber;
            O.N = (int)N, O.K = K, O.active = Y.active, O.status = Y.status, O.match_kf = Y.match_kf, O.match_stage = Y.match_stage;
            const size_t threads = std::max(E, std::max(N, (size_t)K));
            hipLaunchKernelGGL(k_reloc_observations, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, C.s, O);
            ++T.launches;
        }
        if (V) {  // ---- PnP and the first optimisation: which problems run is decided on the device, from the flags the kernel before wrote
            SolveGather Ga{};
            Ga.M = (int)M, Ga.K = K, Ga.m_keypt = Z.m_keypt, Ga.t_bearings = Z.t_bearings, Ga.t_xy = Y.t_xy, Ga.t_xright = Y.t_xright, Ga.t_octave = Y.t_octave;
            for (int l = 0; l < num_levels; ++l) Ga.max_cos_level[l] = max_cos_level[l], Ga.inv_level_sigma_sq[l] = inv_level_sigma_sq[l];
            Ga.huber_delta = huber_delta;
            Ga.bearings = Z.pnp.bearings, Ga.max_cos = Z.pnp.max_cos, Ga.uvr = Z.o_uvr, Ga.w = Z.o_w, Ga.huber = Z.o_huber;
            Ga.pnp_valid = Z.pnp.valid, Ga.pnp_pose = Z.pnp.pose, Ga.is_inlier = Z.pnp.is_inlier, Ga.best_iter = Z.pnp.best_iter;
            const size_t threads = std::max(M, (size_t)12 * K);
            hipLaunchKernelGGL(k_reloc_solve_gather, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, C.s, Ga);
            ++T.launches;
            T.launches += sv_pnp_ransac_enqueue(ctx, C.s, Z.pnp, K, (int)pnp_active.size(), V->num_iter, V->gn_iter, V->min_num_inliers, V->recompute);

            PoseOptDev D0;
            memset(&D0, 0, sizeof(D0));
            memcpy(D0.intr, intrinsics, sizeof(double) * 5);
            D0.num_trials_robust = num_trials_robust, D0.num_trials = num_trials, D0.num_each_iter = num_each_iter;
            D0.reset_flag_each_round = reset_stop_flag_each_round;
            D0.gain_thr = 1e-3;  // terminateAction->setGainThreshold(1e-3), pose_optimizer_g2o.cc:55
            D0.pos_w = Z.pnp.pos_w, D0.uvr = Z.o_uvr, D0.inv_sigma_sq = Z.o_w, D0.huber = Z.o_huber;
            D0.trk_pos = Z.oc_pos, D0.trk_uvr = Z.oc_uvr, D0.trk_w = Z.oc_w, D0.trk_h = Z.oc_huber, D0.trk_kp_of = Z.o_entry_of;
            D0.level = Z.o_level, D0.robust = Z.o_robust, D0.outlier = Z.o_outlier;
            D0.pose_in_dev = Z.pnp.pose, D0.pose_out = Z.opt_pose, D0.result = Z.opt_result, D0.bat_flags = Z.opt_flags;
            D0.bat_off = Z.pnp.match_off, D0.bat_select = Z.pnp.is_inlier, D0.bat_active = Z.pnp.valid;
            sv_pose_opt_batch(ctx, C.s, D0, K);
            ++T.launches;

            SolveBook B{};
            B.K = K, B.nt = nt, B.min_num_valid_obs = V->min_num_opt_valid_obs, B.match_off = Z.pnp.match_off, B.kf_off = Y.kf_off, B.m_keypt = Z.m_keypt;
            B.m_kf_entry = Z.m_kf_entry, B.m_pos_w = Z.pnp.pos_w, B.pnp_valid = Z.pnp.valid, B.is_inlier = Z.pnp.is_inlier, B.opt_flags = Z.opt_flags;
            B.opt_result = Z.opt_result, B.active = Y.active, B.status = Y.status, B.count0 = Y.count0, B.occupied = Y.occupied, B.lm_pos = Y.lm_pos;
            B.valid = Y.valid;
            hipLaunchKernelGGL(k_reloc_solve_book, dim3(K), dim3(256), 0, C.s, B);
            ++T.launches;
        }
        GridProblem G{};
        G.t_xy = Y.t_xy, G.t_octave = Y.t_octave, G.nt = nt, G.nq = (int)N, G.cols = grid_cols, G.rows = grid_rows, G.min_x = cam->min_x, G.min_y = cam->min_y;
        G.inv_w = (double)grid_cols / (cam->max_x - cam->min_x);  // float difference, double quotient: data/common.cc:86-87 via camera::base
        G.inv_h = (double)grid_rows / (cam->max_y - cam->min_y);
        G.cell_of = Y.cell_of, G.cell_off = Y.cell_off, G.cell_items = Y.cell_items;
        G.q_xy = Y.q_xy, G.q_margin = Y.q_margin, G.q_min_level = Y.q_min_level, G.q_max_level = Y.q_max_level, G.q_valid = Y.visible;
        G.cand_off = Y.cand_off, G.cand_idx = Y.cand_idx;
        T.add(sv_launch_grid_frame(C.s, G));  // (one launch, or a memset and three: the launcher decides and says)

        PoseOptDev D;
        memset(&D, 0, sizeof(D));
        memcpy(D.intr, intrinsics, sizeof(double) * 5);
        D.num_trials_robust = num_trials_robust, D.num_trials = num_trials, D.num_each_iter = num_each_iter;
        D.reset_flag_each_round = reset_stop_flag_each_round;
        D.gain_thr = 1e-3;  // terminateAction->setGainThreshold(1e-3), pose_optimizer_g2o.cc:55
        D.pos_w = Y.lm_pos, D.uvr = Y.uvr, D.inv_sigma_sq = Y.w, D.huber = Y.huber;
        D.trk_pos = Y.c_pos, D.trk_uvr = Y.c_uvr, D.trk_w = Y.c_w, D.trk_h = Y.c_huber, D.trk_kp_of = Y.entry_of;
        D.level = Y.level, D.robust = Y.robust, D.outlier = Y.outlier;
        D.bat_off = Y.obs_off, D.bat_select = Y.occupied, D.bat_active = Y.active;

        RelocDecide Dec{};
        Dec.K = K, Dec.S = S, Dec.min_num_valid_obs = min_num_valid_obs, Dec.count0 = Y.count0, Dec.num_found = Y.num_found, Dec.result = Y.result;
        Dec.active = Y.active, Dec.status = Y.status;

        bool again = false;
        for (int s = 0; s < S && !again; ++s) {
            const double* const pose_s = s == 0 ? (V ? Z.opt_pose.p : Y.pose_in.p) : Y.pose_stage.p + (size_t)(s - 1) * K * 12;
            if (N > 0) {
                RelocReproj Q{};
                Q.R.cam = *cam;
                Q.R.n = (int)N;
                Q.R.pos_w = Y.pos_w, Q.R.min_valid_dist = Y.min_d, Q.R.max_valid_dist = Y.max_d;
                Q.R.ray_cos_thr = 0.5f, Q.R.num_levels = (unsigned)num_levels, Q.R.log_scale_factor = log_scale_factor;
                Q.R.visible = Y.visible, Q.R.q_xy = Y.q_xy, Q.R.q_margin = Y.q_margin, Q.R.q_min_level = Y.q_min_level, Q.R.q_max_level = Y.q_max_level;
                Q.R.margin = margin[s];
                for (int l = 0; l < num_levels; ++l) Q.R.scale_factors[l] = scale_factors[l];
                Q.R.dist_mode = 1, Q.R.normal_mode = 2, Q.R.center_mode = 0, Q.R.window_mode = 0;  // projection::match_frame_and_keyframe (svgpu_match2.hip)
                Q.kf_off = Y.kf_off, Q.K = K, Q.pose = pose_s, Q.active = Y.active, Q.valid = Y.valid;
                hipLaunchKernelGGL(k_reloc_reproject, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, C.s, Q);
                ++T.launches;
            }
            if (N > 0) {
                T.add(sv_launch_grid_queries(C.s, G));  // list sizes of all entries + their scan
                int32_t total = 0;
                if ((rc = C.read_now(&total, Y.cand_off.p + N))) return rc;
                ++T.copies, ++T.syncs;
                if (total < 0) return fail(": candidate lists do not fit int32");
                if ((size_t)total > H.cap) {  // nothing of this stage's lists was written: the same call with longer ones
                    H.cap = (size_t)total + (size_t)total / 4 + 4096;
                    again = true;
                    break;
                }
                T.add(sv_launch_grid_fill(C.s, G));
            }
            // (without any entry the replay workgroups still run: they leave every candidate's num_found at 0)
            T.add(sv_launch_cand_batch(ctx, C.s, (const CandProblem*)Y.cand_tab.p + (size_t)s * K, (const CandBatchReplay*)Y.replay_tab.p, Y.kf_off, K, (int)N, lds_bytes));
            if (N > 0) {
                RelocApply Ap{};
                Ap.N = (int)N, Ap.K = K, Ap.nt = nt, Ap.stage = s, Ap.kf_off = Y.kf_off, Ap.match_q = Y.match_q, Ap.pos_w = Y.pos_w;
                Ap.valid = Y.valid, Ap.occupied = Y.occupied, Ap.lm_pos = Y.lm_pos, Ap.match_kf = Y.match_kf, Ap.match_stage = Y.match_stage;
                hipLaunchKernelGGL(k_reloc_apply, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, C.s, Ap);
                ++T.launches;
            }
            Dec.stage = s;
            hipLaunchKernelGGL(k_reloc_decide, dim3((K + 255) / 256), dim3(256), 0, C.s, Dec);
            ++T.launches;
            D.pose_in_dev = pose_s, D.pose_out = Y.pose_stage.p + (size_t)s * K * 12;
            D.result = Y.result.p + (size_t)s * K * 4, D.bat_flags = Y.flags.p + (size_t)s * E;
            sv_pose_opt_batch(ctx, C.s, D, K);
            ++T.launches;
        }
        if (again) {
            SV_HIP(ctx, hipStreamSynchronize(C.s));  // (what was enqueued still reads the arena the next attempt may replace)
            ++T.syncs;
            continue;
        }
        Dec.stage = S;
        hipLaunchKernelGGL(k_reloc_decide, dim3((K + 255) / 256), dim3(256), 0, C.s, Dec);
        ++T.launches;

        result.resize(Y.result.n);
        flags.resize(Y.flags.n);
        C.down(status, Y.status);
        C.down(pose_out, Y.pose_stage.p + (size_t)(S - 1) * K * 12, (size_t)K * 12);
        C.down(match_kf, Y.match_kf), C.down(match_stage, Y.match_stage), C.down(num_found, Y.num_found);
        C.down(result.data(), Y.result), C.down(flags.data(), Y.flags);
        if (V) {
            opt_result.resize(Z.opt_result.n);
            C.down(V->pnp_valid, Z.pnp.valid), C.down(V->pnp_pose_cw, Z.pnp.pose), C.down(V->is_inlier, Z.pnp.is_inlier), C.down(V->best_iter, Z.pnp.best_iter);
            C.down(V->opt_pose, Z.opt_pose), C.down(opt_result.data(), Z.opt_result), C.down(V->opt_outlier, Z.opt_flags);
        }
        {
            std::vector<Downloads::Item> items = C.D.items;
            T.copies += (int)sv_merge_ranges(items, 32768).size();
        }
        if ((rc = C.finish())) return rc;
        ++T.syncs;
        // ---- host out: the counts per stage, and the flags / iteration count of the last optimisation a candidate ran
        for (int p = 0; p < K; ++p) {
            for (int s = 0; s < S; ++s) num_valid[(size_t)p * S + s] = result[((size_t)s * K + p) * 4];
            const int st = status[p];
            const int ran = st < 0 ? -1 : (st == 0 || st == 1 + S ? S - 1 : st - 2);
            if (lm_iterations) lm_iterations[p] = ran >= 0 ? result[((size_t)ran * K + p) * 4 + 1] : 0;
            uint8_t* const o = outlier + (size_t)p * nt;
            if (ran >= 0) std::memcpy(o, flags.data() + (size_t)ran * E + (size_t)p * nt, (size_t)nt);
            else std::memset(o, 0, (size_t)nt);
        }
        if (V)
            for (int p = 0; p < K; ++p) V->opt_num_valid[p] = opt_result[4 * (size_t)p];
        if (stats) *stats = svgpu_call_stats{T.launches, T.copies, T.syncs};
        return SVGPU_OK;
    }
    return fail(": candidate lists kept outgrowing their capacity");
}

}  // namespace

extern "C" int svgpu_reloc_refine_batch(svgpu_ctx* ctx, const svgpu_camera* cam, const uint8_t* tdesc, const float* t_xy, const int32_t* t_octave,
                                        const float* t_angle, const float* t_xright, int nt, int grid_cols, int grid_rows, int num_levels,
                                        const float* scale_factors, const float* inv_level_sigma_sq, float log_scale_factor, const double* intrinsics,
                                        int num_trials_robust, int num_trials, int num_each_iter, int reset_stop_flag_each_round, int check_orientation,
                                        int num_candidates, const uint8_t* active, const double* pose_cw, const int32_t* n_already_found,
                                        const uint8_t* frame_has_lm, const double* frame_lm_pos_w, const int32_t* kf_off, const double* pos_w,
                                        const uint8_t* valid, const float* min_valid_dist, const float* max_valid_dist, const uint8_t* lm_desc,
                                        const float* angle_kf, int num_stages, const float* margin, const int32_t* hamm_dist_thr, int min_num_valid_obs,
                                        int32_t* status, double* pose_out, int32_t* match_kf, int32_t* match_stage, uint8_t* outlier,
                                        int32_t* num_found, int32_t* num_valid, int32_t* lm_iterations, svgpu_call_stats* stats) {
    return reloc_call("svgpu_reloc_refine_batch", nullptr, ctx, cam, tdesc, t_xy, t_octave, t_angle, t_xright, nt, grid_cols, grid_rows, num_levels, scale_factors,
                      inv_level_sigma_sq, log_scale_factor, intrinsics, num_trials_robust, num_trials, num_each_iter, reset_stop_flag_each_round,
                      check_orientation, num_candidates, active, pose_cw, n_already_found, frame_has_lm, frame_lm_pos_w, kf_off, pos_w, valid, min_valid_dist,
                      max_valid_dist, lm_desc, angle_kf, num_stages, margin, hamm_dist_thr, min_num_valid_obs, status, pose_out, match_kf, match_stage, outlier,
                      num_found, num_valid, lm_iterations, stats);
}

extern "C" int svgpu_reloc_solve_batch(svgpu_ctx* ctx, const svgpu_camera* cam, const uint8_t* tdesc, const float* t_xy, const int32_t* t_octave,
                                       const float* t_angle, const float* t_xright, const double* t_bearings, int nt, int grid_cols, int grid_rows,
                                       int num_levels, const float* scale_factors, const float* inv_level_sigma_sq, float log_scale_factor,
                                       const double* intrinsics, int num_trials_robust, int num_trials, int num_each_iter, int reset_stop_flag_each_round,
                                       int check_orientation, int num_candidates, const uint8_t* active, const int32_t* match_off, const int32_t* m_keypt,
                                       const double* m_pos_w, const int32_t* m_kf_entry, int min_num_inliers, int num_iter, const uint32_t* samples,
                                       int recompute, int gauss_newton_num_iter, int min_num_opt_valid_obs, const int32_t* kf_off, const double* pos_w,
                                       const uint8_t* valid, const float* min_valid_dist, const float* max_valid_dist, const uint8_t* lm_desc, const float* angle_kf,
                                       int num_stages, const float* margin, const int32_t* hamm_dist_thr, int min_num_valid_obs, int32_t* status,
                                       uint8_t* pnp_valid, double* pnp_pose_cw, uint8_t* is_inlier, int32_t* best_iter, double* opt_pose,
                                       uint8_t* opt_outlier, int32_t* opt_num_valid, double* pose_out, int32_t* match_kf, int32_t* match_stage,
                                       uint8_t* outlier, int32_t* num_found, int32_t* num_valid, int32_t* lm_iterations, svgpu_call_stats* stats) {
    auto fail = [&](const char* what) { return sv_set_error(ctx, SVGPU_ERR_INVALID, what); };
    if (!ctx || num_candidates < 0) return fail("svgpu_reloc_solve_batch: bad arguments");
    if (num_candidates == 0) {
        if (stats) *stats = svgpu_call_stats{0, 0, 0};
        return SVGPU_OK;
    }
    // ---- validation of what this call adds (the rest is the refine call's, in reloc_call): nothing is launched or written before all of it has passed
    const int K = num_candidates;
    if (nt < 0 || min_num_inliers < 0 || num_iter < 0 || gauss_newton_num_iter < 0 || !match_off || !kf_off || !pnp_valid || !pnp_pose_cw || !best_iter
        || !opt_pose || !opt_num_valid)
        return fail("svgpu_reloc_solve_batch: bad arguments");
    if (!sv_offsets_ok(match_off, K)) return fail("svgpu_reloc_solve_batch: match_off does not start at 0 or is not monotone");
    if (!sv_offsets_ok(kf_off, K)) return fail("svgpu_reloc_solve_batch: kf_off does not start at 0 or is not monotone");
    const size_t M = (size_t)match_off[K];
    if (M > 0 && (!t_bearings || !m_keypt || !m_pos_w || !m_kf_entry || !is_inlier || !opt_outlier)) return fail("svgpu_reloc_solve_batch: bad arguments");
    if (M * 24 > (size_t)INT32_MAX || (size_t)K * (size_t)num_iter * 12 > (size_t)INT32_MAX || M * (size_t)num_iter > (size_t)INT32_MAX)
        return fail("svgpu_reloc_solve_batch: totals do not fit int32");
    std::vector<uint8_t> named;
    for (int p = 0; p < K; ++p) {
        const int lo = match_off[p], np = match_off[p + 1] - lo, nq = kf_off[p + 1] - kf_off[p];
        named.assign((size_t)nq, 0);
        for (int i = 0; i < np; ++i) {
            const int t = m_keypt[lo + i], ke = m_kf_entry[lo + i];
            if (t < 0 || t >= nt || (i > 0 && t <= m_keypt[lo + i - 1])) return fail("svgpu_reloc_solve_batch: m_keypt outside the frame or not strictly ascending");
            if (ke < -1 || ke >= nq) return fail("svgpu_reloc_solve_batch: m_kf_entry outside its candidate's keyframe entries");
            if (ke >= 0 && named[ke]++) return fail("svgpu_reloc_solve_batch: m_kf_entry repeated within a candidate");
        }
        if ((active && !active[p]) || np < 4 || np < min_num_inliers) continue;  // (the samples of a problem that does not run are not read)
        if (num_iter > 0 && !samples) return fail("svgpu_reloc_solve_batch: bad arguments");
        if (const char* what = sv_pnp_check_samples(samples + 4 * (size_t)p * num_iter, num_iter, (unsigned)np)) return fail(what);
    }
    const SolveCall V{t_bearings, match_off, m_keypt, m_pos_w, m_kf_entry, min_num_inliers, num_iter, samples, recompute, gauss_newton_num_iter,
                      min_num_opt_valid_obs, pnp_valid, pnp_pose_cw, is_inlier, best_iter, opt_pose, opt_outlier, opt_num_valid};
    return reloc_call("svgpu_reloc_solve_batch", &V, ctx, cam, tdesc, t_xy, t_octave, t_angle, t_xright, nt, grid_cols, grid_rows, num_levels, scale_factors,
                      inv_level_sigma_sq, log_scale_factor, intrinsics, num_trials_robust, num_trials, num_each_iter, reset_stop_flag_each_round,
                      check_orientation, num_candidates, active, nullptr, nullptr, nullptr, nullptr, kf_off, pos_w, valid, min_valid_dist, max_valid_dist, lm_desc,
                      angle_kf, num_stages, margin, hamm_dist_thr, min_num_valid_obs, status, pose_out, match_kf, match_stage, outlier, num_found, num_valid,
                      lm_iterations, stats);
}
