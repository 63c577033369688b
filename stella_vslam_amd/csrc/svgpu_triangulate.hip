// svgpu_triangulate_two_views / _batch: host glue of k_triangulate_two_views (triangulate_kernels.hip).  Host arrays in and out,
// synchronous; one upload, one launch and one read-back per call whatever the number of neighbours.
#include <algorithm>
#include <cmath>

#include "sv_staged_call.h"
#include "sv_validate.h"
#include "triangulate_kernels.h"

namespace {

bool view_ok(const svgpu_triangulate_view& v) {
    return v.cam && v.pose_cw && v.n >= 0 && v.cam->model >= SVGPU_CAM_PERSPECTIVE && v.cam->model <= SVGPU_CAM_RADIAL_DIVISION
           && (v.n == 0 || (v.xy && v.octave && v.bearings));
}

struct ViewPieces {
    Piece<float> xy;
    Piece<int32_t> octave;
    Piece<double> bearings;
    Piece<float> xright, depth;
};
// camera, pose and derived constants of one side; the keypoint arrays get their places in the arena
void place_view(UploadArena& A, const svgpu_triangulate_view& v, float scale_factor_1, TriView& T, ViewPieces& Y) {
    T.cam = *v.cam;
    std::memcpy(T.pose_cw, v.pose_cw, sizeof T.pose_cw);
    const double* P = v.pose_cw;
    for (int i = 0; i < 3; ++i)  // keyframe::set_pose_cw (data/keyframe.cc:365-376): trans_wc = -rot_wc * trans_cw
        T.trans_wc[i] = ((-P[i]) * P[3] + (-P[4 + i]) * P[7]) + (-P[8 + i]) * P[11];
    T.true_baseline = v.true_baseline;
    T.fx_inv = 1.0 / v.cam->fx;
    T.fy_inv = 1.0 / v.cam->fy;
    T.ratio_factor = 2.0f * std::max(scale_factor_1, v.scale_factor);
    T.n = v.n;
    const size_t n = (size_t)v.n;
    T.xy = Y.xy = optional_piece<float>(A, v.xy, n * 2);
    T.octave = Y.octave = optional_piece<int32_t>(A, v.octave, n);
    T.bearings = Y.bearings = optional_piece<double>(A, v.bearings, n * 3);
    T.xright = Y.xright = optional_piece<float>(A, v.xright, n);
    T.depth = Y.depth = optional_piece<float>(A, v.depth, n);
}
void up_view(StagedCall& C, const svgpu_triangulate_view& v, const ViewPieces& Y) {
    C.up(Y.xy, v.xy, Y.octave, v.octave, Y.bearings, v.bearings, Y.xright, v.xright, Y.depth, v.depth);
}

int tri_core(svgpu_ctx* ctx, const char* who, const svgpu_triangulate_view* v1, const svgpu_triangulate_view* nb, int K, const int32_t* off,
             const float* scale_factors, const float* level_sigma_sq, int num_levels, float rays_parallax_deg_thr, const int32_t* idx1, const int32_t* idx2,
             double* pos_w, uint8_t* status, int* num_accepted) {
    if (!ctx || !v1 || K < 0 || (K > 0 && (!nb || !off)) || !scale_factors || !level_sigma_sq || num_levels < 1 || num_levels > SV_MAX_LEVELS || !view_ok(*v1))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    if (K > 0 && !sv_offsets_ok(off, K)) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    for (int k = 0; k < K; ++k)
        if (!view_ok(nb[k])) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    const int M = K > 0 ? off[K] : 0;
    if (M > 0 && (!idx1 || !pos_w || !status)) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    if (num_accepted)
        for (int k = 0; k < K; ++k) num_accepted[k] = 0;
    if (M == 0) return SVGPU_OK;
    // every index the kernel dereferences is checked here (the reference's .at() would throw); a stereo keypoint of an equirectangular
    // camera is the reference's "Not implemented" exception (data/common.cc:239-241)
    std::vector<int32_t> nb_of(M), nb_first(K);
    for (int k = 0; k < K; ++k) {
        const svgpu_triangulate_view& v2 = nb[k];
        nb_first[k] = off[k];
        if (!idx2 && off[k + 1] - off[k] != v1->n && off[k + 1] != off[k]) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
        for (int m = off[k]; m < off[k + 1]; ++m) {
            nb_of[m] = k;
            const int i1 = idx2 ? idx1[m] : m - off[k], i2 = idx2 ? idx2[m] : idx1[m];
            if (!idx2 && i2 < 0) continue;
            if (i1 < 0 || i1 >= v1->n || i2 < 0 || i2 >= v2.n || v1->octave[i1] < 0 || v1->octave[i1] >= num_levels || v2.octave[i2] < 0
                || v2.octave[i2] >= num_levels)
                return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
            if ((v1->cam->model == SVGPU_CAM_EQUIRECTANGULAR && v1->xright && 0 <= v1->xright[i1])
                || (v2.cam->model == SVGPU_CAM_EQUIRECTANGULAR && v2.xright && 0 <= v2.xright[i2]))
                return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_triangulate_two_views: stereo keypoint of an equirectangular camera");
        }
    }
    TriProblem P{};
    std::vector<TriView> views(K);
    std::vector<ViewPieces> VY(K + 1);
    Piece<TriView> d_views;
    Piece<int32_t> d_first, d_of, d_idx1, d_idx2;
    StagedCall C;
    int rc = C.open(ctx, "svgpu_triangulate_two_views: internal arena overflow", [&](UploadArena& A) {
        place_view(A, *v1, v1->scale_factor, P.v1, VY[K]);
        for (int k = 0; k < K; ++k) place_view(A, nb[k], v1->scale_factor, views[k], VY[k]);
        P.nb = d_views = A.piece<TriView>(K);
        P.nb_first = d_first = A.piece<int32_t>(K);
        P.nb_of_match = d_of = A.piece<int32_t>(M);
        P.idx1 = d_idx1 = A.piece<int32_t>(M);
        P.idx2 = d_idx2 = optional_piece<int32_t>(A, idx2, M);
        P.pos_w = A.take<double>((size_t)M * 3);
        P.status = A.take<uint8_t>(M);
    });
    if (rc) return rc;
    hipStream_t s = C.s;
    up_view(C, *v1, VY[K]);
    for (int k = 0; k < K; ++k) up_view(C, nb[k], VY[k]);
    // (the views carry device pointers: placed above, copied here; M > 0, so there is a view, and idx1 was checked: only idx2 is optional)
    C.up(d_views, views.data(), d_first, nb_first.data(), d_of, nb_of.data(), d_idx1, idx1, d_idx2, idx2);
    if ((rc = C.flush())) return rc;
    P.num_matches = M;
    for (int l = 0; l < num_levels; ++l) P.scale_factors[l] = scale_factors[l], P.level_sigma_sq[l] = level_sigma_sq[l];
    P.cos_rays_parallax_thr = (float)std::cos(rays_parallax_deg_thr * M_PI / 180.0);  // two_view_triangulator.cc:17 (a float member)
    {
        SvProfScope prof(ctx, s, "k_triangulate_two_views");
        sv_launch_triangulate_two_views(s, P);
    }
    C.down(pos_w, P.pos_w, 3 * (size_t)M);
    C.down(status, P.status, M);
    if ((rc = C.finish())) return rc;
    if (num_accepted)
        for (int m = 0; m < M; ++m) num_accepted[nb_of[m]] += status[m] == SVGPU_TRI_ACCEPTED;
    return SVGPU_OK;
}

}  // namespace

extern "C" {

int svgpu_triangulate_two_views(svgpu_ctx* ctx, const svgpu_camera* cam1, const double* pose_1w, double true_baseline_1, const float* xy1, const int32_t* octave1,
                                const double* bearings1, const float* xright1, const float* depth1, int n1, const svgpu_camera* cam2, const double* pose_2w,
                                double true_baseline_2, const float* xy2, const int32_t* octave2, const double* bearings2, const float* xright2,
                                const float* depth2, int n2, const float* scale_factors, const float* level_sigma_sq, int num_levels, float scale_factor_1,
                                float scale_factor_2, float rays_parallax_deg_thr, const int32_t* idx1, const int32_t* idx2, int num_matches, double* pos_w,
                                uint8_t* status, int* num_accepted) {
    if (num_matches < 0 || (!idx2 && num_matches != 0 && num_matches != n1))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_triangulate_two_views: bad arguments");
    const svgpu_triangulate_view v1{cam1, pose_1w, true_baseline_1, xy1, octave1, bearings1, xright1, depth1, n1, scale_factor_1};
    const svgpu_triangulate_view v2{cam2, pose_2w, true_baseline_2, xy2, octave2, bearings2, xright2, depth2, n2, scale_factor_2};
    const int32_t off[2] = {0, num_matches};
    return tri_core(ctx, "svgpu_triangulate_two_views: bad arguments", &v1, &v2, 1, off, scale_factors, level_sigma_sq, num_levels, rays_parallax_deg_thr, idx1,
                    idx2, pos_w, status, num_accepted);
}

int svgpu_triangulate_two_views_batch(svgpu_ctx* ctx, const svgpu_triangulate_view* view1, const svgpu_triangulate_view* neighbours, int num_neighbours,
                                      const int32_t* match_off, const float* scale_factors, const float* level_sigma_sq, int num_levels,
                                      float rays_parallax_deg_thr, const int32_t* idx1, const int32_t* idx2, double* pos_w, uint8_t* status, int* num_accepted) {
    return tri_core(ctx, "svgpu_triangulate_two_views_batch: bad arguments", view1, neighbours, num_neighbours, match_off, scale_factors, level_sigma_sq,
                    num_levels, rays_parallax_deg_thr, idx1, idx2, pos_w, status, num_accepted);
}

}  // extern "C"
