// svgpu_pnp_compute_pose / svgpu_pnp_ransac_batch / svgpu_pnp_ransac: host glue of the PnP kernels (pnp_kernels.hip).  Host arrays in
// and out, synchronous: one upload, the launches on the context's stream, one read-back and one synchronisation per call.
#include <cmath>

#include "sv_staged_call.h"
#include "sv_validate.h"
#include "pnp_kernels.h"
#include "pnp_layout.h"
#include "sv_trig.h"

// ---- what svgpu_reloc_solve_batch (svgpu_reloc.hip) shares with the entry points of this file
float sv_pnp_max_cos(float scale_factor) {
    constexpr double max_rad_error = 1.0 * M_PI / 180.0;
    return sv_util_cos((float)(scale_factor * max_rad_error));
}

const char* sv_pnp_check_samples(const uint32_t* samples, int num_iter, unsigned np) {
    for (int it = 0; it < num_iter; ++it) {
        const uint32_t* s = samples + 4 * (size_t)it;
        for (int a = 0; a < 4; ++a) {
            if (s[a] >= np) return "svgpu_pnp_ransac: sample index outside its problem";
            for (int b = 0; b < a; ++b)
                if (s[a] == s[b]) return "svgpu_pnp_ransac: index repeated within a sample";
        }
    }
    return nullptr;
}

int sv_pnp_ransac_enqueue(svgpu_ctx* ctx, hipStream_t s, const PnpRansacPieces& Y, int P, int num_active, int I, int gn_iter, int min_num_inliers,
                          int recompute) {
    if (num_active <= 0) return 0;
    PnpRansacProblem R{};
    R.bearings = Y.bearings, R.pos_w = Y.pos_w, R.max_cos = Y.max_cos, R.match_off = Y.match_off, R.samples = Y.samples, R.active = Y.active;
    R.num_problems = P, R.num_active = num_active, R.num_iter = I, R.gn_iter = gn_iter;
    R.min_num_inliers = (unsigned)min_num_inliers;
    R.recompute = recompute != 0;
    R.hyp_pose = Y.hyp_pose, R.hyp_num_inliers = Y.hyp_num_inliers, R.hyp_cost = Y.hyp_cost, R.hyp_inlier = Y.hyp_inlier;
    R.valid = Y.valid, R.pose = Y.pose, R.is_inlier = Y.is_inlier, R.best_iter = Y.best_iter, R.inl_idx = Y.inl_idx, R.inl_count = Y.inl_count;
    {
        SvProfScope prof(ctx, s, "k_pnp_ransac");
        sv_launch_pnp_ransac(s, R);
    }
    {
        SvProfScope prof(ctx, s, "k_pnp_select");
        sv_launch_pnp_select(s, R);
    }
    if (recompute) {  // (:109-123) over the winner's inliers; an invalid problem keeps what k_pnp_select wrote
        PnpPoseProblem Q{};
        Q.bearings = Y.bearings, Q.pos_w = Y.pos_w, Q.off = Y.match_off, Q.idx = Y.inl_idx, Q.count = Y.inl_count, Q.enable = Y.valid;
        Q.sets = Y.active, Q.num_launch = num_active, Q.pose = Y.pose, Q.err = nullptr, Q.num_sets = P, Q.gn_iter = gn_iter, Q.keep_on_failure = 1;
        SvProfScope prof(ctx, s, "k_pnp_pose");
        sv_launch_pnp_pose(s, Q);
    }
    return (I > 0 ? 1 : 0) + 1 + (recompute ? 1 : 0);  // launches
}

namespace {

int ransac_core(svgpu_ctx* ctx, const char* who, int num_problems, const int32_t* match_off, const double* bearings, const double* pos_w,
                const int32_t* octaves, const float* scale_factors, int num_levels, int min_num_inliers, int num_iter, const uint32_t* samples,
                int recompute, int gn_iter, uint8_t* valid, double* pose_cw, uint8_t* is_inlier, int32_t* best_iter, double* hyp_pose,
                int32_t* hyp_num_inliers, double* hyp_cost) {
    if (!ctx || num_problems < 0 || min_num_inliers < 0 || num_iter < 0 || gn_iter < 0) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    if (num_problems == 0) return SVGPU_OK;
    if (!match_off || !valid || !pose_cw || !best_iter || !scale_factors || num_levels < 1 || !sv_offsets_ok(match_off, num_problems))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    const int P = num_problems, I = num_iter, n = match_off[P];
    if (n > 0 && (!bearings || !pos_w || !octaves || !is_inlier)) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    // max_cos_errors_ (:27-32): `scale_factors.at(octaves.at(i)) * max_rad_error` is a double, util::cos takes and returns a float
    std::vector<float> max_cos(n);
    for (int i = 0; i < n; ++i) {
        if (octaves[i] < 0 || octaves[i] >= num_levels) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_pnp_ransac: octave out of range");
        max_cos[i] = sv_pnp_max_cos(scale_factors[octaves[i]]);
    }
    // the problems that run (:49-52), and every index their hypotheses dereference
    std::vector<int32_t> active;
    for (int p = 0; p < P; ++p) {
        const unsigned np = (unsigned)(match_off[p + 1] - match_off[p]);
        if (np < 4u || np < (unsigned)min_num_inliers) continue;
        active.push_back(p);
        if (I > 0 && !samples) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
        if (const char* what = sv_pnp_check_samples(samples + 4 * (size_t)p * I, I, np)) return sv_set_error(ctx, SVGPU_ERR_INVALID, what);
    }
    const int num_active = (int)active.size();
    if (num_active > 0) {
        PnpRansacPieces Y{};
        StagedCall C;
        int rc = C.open(ctx, "svgpu_pnp_ransac: internal arena overflow", [&](UploadArena& A) {
            pnp_ransac_layout(A, (size_t)P, (size_t)n, (size_t)I, (size_t)num_active, recompute != 0, Y);
        });
        if (rc) return rc;
        hipStream_t s = C.s;
        C.up(Y.bearings, bearings), C.up(Y.pos_w, pos_w), C.up(Y.max_cos, max_cos.data());
        C.up(Y.match_off, match_off), C.up(Y.samples, samples), C.up(Y.active, active.data());
        if ((rc = C.flush())) return rc;
        sv_pnp_ransac_enqueue(ctx, s, Y, P, num_active, I, gn_iter, min_num_inliers, recompute);
        C.down(valid, Y.valid), C.down(pose_cw, Y.pose), C.down(is_inlier, Y.is_inlier), C.down(best_iter, Y.best_iter);
        C.down(hyp_pose, Y.hyp_pose), C.down(hyp_num_inliers, Y.hyp_num_inliers), C.down(hyp_cost, Y.hyp_cost);  // optional: null is no request
        if ((rc = C.finish())) return rc;
    }
    // a problem that did not run: solution_is_valid_ = false, nothing else is defined by the reference -- zeros here
    size_t next = 0;
    for (int p = 0; p < P; ++p) {
        if (next < active.size() && active[next] == p) {
            ++next;
            continue;
        }
        valid[p] = 0;
        best_iter[p] = -1;
        std::memset(pose_cw + 12 * (size_t)p, 0, 96);
        if (match_off[p + 1] > match_off[p]) std::memset(is_inlier + match_off[p], 0, (size_t)(match_off[p + 1] - match_off[p]));
        if (hyp_pose && I) std::memset(hyp_pose + 12 * (size_t)p * I, 0, (size_t)I * 96);
        if (hyp_num_inliers && I) std::memset(hyp_num_inliers + (size_t)p * I, 0, (size_t)I * 4);
        if (hyp_cost && I) std::memset(hyp_cost + (size_t)p * I, 0, (size_t)I * 8);
    }
    return SVGPU_OK;
}

}  // namespace

extern "C" {

int svgpu_pnp_compute_pose(svgpu_ctx* ctx, int num_sets, const int32_t* set_off, const double* bearings, const double* pos_w,
                           int gauss_newton_num_iter, double* pose_cw, double* reproj_error) {
    const char* who = "svgpu_pnp_compute_pose: bad arguments";
    if (!ctx || num_sets < 0 || gauss_newton_num_iter < 0) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    if (num_sets == 0) return SVGPU_OK;
    if (!set_off || !bearings || !pos_w || !pose_cw || !sv_offsets_ok(set_off, num_sets)) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    for (int k = 0; k < num_sets; ++k)
        if (set_off[k + 1] - set_off[k] < 4) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_pnp_compute_pose: a set of fewer than 4 correspondences");
    const size_t n = (size_t)set_off[num_sets];
    PnpPosePieces Y{};
    StagedCall C;
    int rc = C.open(ctx, "svgpu_pnp_compute_pose: internal arena overflow", [&](UploadArena& A) { pnp_pose_layout(A, (size_t)num_sets, n, Y); });
    if (rc) return rc;
    hipStream_t s = C.s;
    C.up(Y.bearings, bearings), C.up(Y.pos_w, pos_w), C.up(Y.off, set_off);
    if ((rc = C.flush())) return rc;
    PnpPoseProblem Q{};
    Q.bearings = Y.bearings, Q.pos_w = Y.pos_w, Q.off = Y.off, Q.pose = Y.pose, Q.err = Y.err, Q.num_sets = num_sets, Q.gn_iter = gauss_newton_num_iter;
    {
        SvProfScope prof(ctx, s, "k_pnp_pose");
        sv_launch_pnp_pose(s, Q);
    }
    C.down(pose_cw, Y.pose), C.down(reproj_error, Y.err);
    return C.finish();
}

int svgpu_pnp_ransac_batch(svgpu_ctx* ctx, int num_problems, const int32_t* match_off, const double* bearings, const double* pos_w,
                           const int32_t* octaves, const float* scale_factors, int num_levels, int min_num_inliers, int num_iter,
                           const uint32_t* samples, int recompute, int gauss_newton_num_iter, uint8_t* valid, double* pose_cw,
                           uint8_t* is_inlier, int32_t* best_iter, double* hyp_pose, int32_t* hyp_num_inliers, double* hyp_cost) {
    return ransac_core(ctx, "svgpu_pnp_ransac_batch: bad arguments", num_problems, match_off, bearings, pos_w, octaves, scale_factors, num_levels,
                       min_num_inliers, num_iter, samples, recompute, gauss_newton_num_iter, valid, pose_cw, is_inlier, best_iter, hyp_pose,
                       hyp_num_inliers, hyp_cost);
}

int svgpu_pnp_ransac(svgpu_ctx* ctx, const double* bearings, const double* pos_w, const int32_t* octaves, int num_matches,
                     const float* scale_factors, int num_levels, int min_num_inliers, int num_iter, const uint32_t* samples, int recompute,
                     int gauss_newton_num_iter, uint8_t* valid, double* pose_cw, uint8_t* is_inlier, int32_t* best_iter, double* hyp_pose,
                     int32_t* hyp_num_inliers, double* hyp_cost) {
    if (num_matches < 0) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_pnp_ransac: bad arguments");
    const int32_t off[2] = {0, num_matches};
    return ransac_core(ctx, "svgpu_pnp_ransac: bad arguments", 1, off, bearings, pos_w, octaves, scale_factors, num_levels, min_num_inliers, num_iter,
                       samples, recompute, gauss_newton_num_iter, valid, pose_cw, is_inlier, best_iter, hyp_pose, hyp_num_inliers, hyp_cost);
}

}  // extern "C"
