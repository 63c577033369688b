// svgpu_sim3_transform_optimize_batch / svgpu_sim3_transform_optimize: host glue of the pairwise Sim3 optimizer (sim3opt_kernels.hip).  Host
// arrays in and out, synchronous: one upload, one launch on the context's stream, one read-back and one synchronisation per call, whatever
// the batch size.
#include <cmath>

#include "sv_staged_call.h"
#include "sv_validate.h"
#include "sim3opt_kernels.h"
#include "sim3opt_layout.h"

static_assert(sizeof(Sim3OptProblem) == S3O_LAYOUT_PROBLEM, "sim3opt_layout.h and sim3opt_kernels.h disagree on the problem descriptor");
static_assert(sizeof(svgpu_sim3opt_stats) == S3O_LAYOUT_STATS, "sim3opt_layout.h and svgpu.h disagree on svgpu_sim3opt_stats");

namespace {

// the edge's camera (mutual_reproj_edge_wrapper.h:64-158): false for a model the edges do not cover
bool fill_view(const svgpu_sim3opt_view& v, Sim3OptView& o) {
    const svgpu_camera& c = v.cam;
    switch (c.model) {
        case SVGPU_CAM_PERSPECTIVE:
        case SVGPU_CAM_FISHEYE:
        case SVGPU_CAM_RADIAL_DIVISION:
            o.k[0] = c.fx, o.k[1] = c.fy, o.k[2] = c.cx, o.k[3] = c.cy;
            o.equirect = 0;
            break;
        case SVGPU_CAM_EQUIRECTANGULAR:
            o.k[0] = c.cols, o.k[1] = c.rows, o.k[2] = 0.0, o.k[3] = 0.0;
            o.equirect = 1;
            break;
        default:
            return false;
    }
    o.pad = 0;
    for (int k = 0; k < 12; ++k) o.pose[k] = v.pose_cw[k];
    return true;
}

int optimize_core(svgpu_ctx* ctx, const char* who, int num_problems, const svgpu_sim3opt_view* view1, int view1_shared, const svgpu_sim3opt_view* view2,
                  const int32_t* match_off, const double* obs1, const double* obs2, const float* w1, const float* w2, const double* pos1,
                  const double* pos2, const double* sim3_12, float chi_sq, int fix_scale, int num_iter, double* sim3_out, int32_t* num_inliers,
                  uint8_t* status, svgpu_sim3opt_stats* stats) {
    if (!ctx || num_problems < 0) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    if (num_problems == 0) return SVGPU_OK;
    if (num_iter < 0 || !sv_positive_finite(chi_sq)) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    if (!view1 || !view2 || !match_off || !sim3_12 || !sim3_out || !num_inliers) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    // ---- validation: nothing is launched before all of it has passed
    const int P = num_problems;
    if (match_off[0] != 0) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_sim3_transform_optimize: match_off[0] is not 0");
    if (!sv_offsets_ok(match_off, P)) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_sim3_transform_optimize: offsets are not monotone");
    const size_t n = (size_t)match_off[P];
    if (n > 0 && (!obs1 || !obs2 || !w1 || !w2 || !pos1 || !pos2 || !status)) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    for (size_t i = 0; i < n; ++i)
        if (!sv_positive_finite(w1[i]) || !sv_positive_finite(w2[i]))
            return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_sim3_transform_optimize: an inv_sigma_sq is not positive and finite");
    std::vector<Sim3OptProblem> prob(P);
    for (int p = 0; p < P; ++p) {
        if (!sv_sim3_ok(sim3_12 + 8 * (size_t)p))
            return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_sim3_transform_optimize: a Sim3_12 is not a Sim3 (unit quaternion, positive scale)");
        if (!fill_view(view1[view1_shared ? 0 : p], prob[p].view[0]) || !fill_view(view2[p], prob[p].view[1]))
            return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_sim3_transform_optimize: a camera model the edges do not cover");
        for (int k = 0; k < 8; ++k) prob[p].sim3[k] = sim3_12[8 * (size_t)p + k];
        prob[p].m_lo = match_off[p], prob[p].m_hi = match_off[p + 1];
    }

    Sim3OptPieces Y{};
    StagedCall C;
    int rc = C.open(ctx, "svgpu_sim3_transform_optimize: internal arena overflow", [&](UploadArena& A) { sim3opt_layout(A, (size_t)P, n, Y); });
    if (rc) return rc;
    hipStream_t s = C.s;
    C.up(Y.prob, (const char*)prob.data());
    C.up(Y.obs1, obs1), C.up(Y.obs2, obs2), C.up(Y.w1, w1), C.up(Y.w2, w2), C.up(Y.pos1, pos1), C.up(Y.pos2, pos2);
    if ((rc = C.flush())) return rc;

    Sim3OptDev D{};
    D.num_problems = P, D.fix_scale = fix_scale != 0, D.num_iter = num_iter, D.chi_sq = chi_sq;
    D.prob = (const Sim3OptProblem*)Y.prob.p;
    D.obs1 = Y.obs1, D.obs2 = Y.obs2, D.w1 = Y.w1, D.w2 = Y.w2, D.pos1 = Y.pos1, D.pos2 = Y.pos2;
    D.chi_cache = Y.chi_cache, D.sim3_out = Y.sim3_out, D.num_inliers = Y.num_inliers, D.status = Y.status;
    D.stats = (svgpu_sim3opt_stats*)Y.stats.p;
    {
        SvProfScope prof(ctx, s, "k_sim3_opt");
        sv_launch_sim3opt(s, D);
    }
    C.down(sim3_out, Y.sim3_out), C.down(num_inliers, Y.num_inliers), C.down(status, Y.status), C.down((char*)stats, Y.stats);
    return C.finish();
}

}  // namespace

extern "C" {

int svgpu_sim3_transform_optimize_batch(svgpu_ctx* ctx, int num_problems, const svgpu_sim3opt_view* view1, int view1_shared,
                                        const svgpu_sim3opt_view* view2, const int32_t* match_off, const double* obs1, const double* obs2,
                                        const float* inv_sigma_sq1, const float* inv_sigma_sq2, const double* pos_w_1, const double* pos_w_2,
                                        const double* sim3_12, float chi_sq, int fix_scale, int num_iter, double* sim3_12_out,
                                        int32_t* num_inliers, uint8_t* status, svgpu_sim3opt_stats* stats) {
    return optimize_core(ctx, "svgpu_sim3_transform_optimize_batch: bad arguments", num_problems, view1, view1_shared, view2, match_off, obs1, obs2,
                         inv_sigma_sq1, inv_sigma_sq2, pos_w_1, pos_w_2, sim3_12, chi_sq, fix_scale, num_iter, sim3_12_out, num_inliers, status, stats);
}

int svgpu_sim3_transform_optimize(svgpu_ctx* ctx, const svgpu_sim3opt_view* view1, const svgpu_sim3opt_view* view2, int num_matches,
                                  const double* obs1, const double* obs2, const float* inv_sigma_sq1, const float* inv_sigma_sq2,
                                  const double* pos_w_1, const double* pos_w_2, const double* sim3_12, float chi_sq, int fix_scale, int num_iter,
                                  double* sim3_12_out, int32_t* num_inliers, uint8_t* status, svgpu_sim3opt_stats* stats) {
    if (num_matches < 0) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_sim3_transform_optimize: bad arguments");
    const int32_t off[2] = {0, num_matches};
    return optimize_core(ctx, "svgpu_sim3_transform_optimize: bad arguments", 1, view1, 1, view2, off, obs1, obs2, inv_sigma_sq1, inv_sigma_sq2,
                         pos_w_1, pos_w_2, sim3_12, chi_sq, fix_scale, num_iter, sim3_12_out, num_inliers, status, stats);
}

}  // extern "C"
