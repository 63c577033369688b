// The device functions of the two-view triangulator (module/two_view_triangulator.{h,cc}): one match per call.  k_triangulate_two_views
// (triangulate_kernels.hip) and the new-landmark chain (match_kernels.hip) are wrappers of triangulate_match, so a fix is made once.
#pragma once
#include "frame_device.h"
#include "triangulate_kernels.h"

namespace svtri {

constexpr int kJacobiSweeps = 12;            // a 4 x 4 converges in 4 to 6 sweeps; the early-out ends the loop
constexpr double kJacobiTol = 2.220446049250313e-16;  // columns p, q are orthogonal when |a_p . a_q| <= tol |a_p| |a_q|

__device__ inline double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// solve::triangulator::triangulate(bearing_1, bearing_2, cam_pose_1, cam_pose_2), solve/triangulator.h:76-88
__device__ inline void triangulate_linear(const double* __restrict__ p1, const double* __restrict__ p2, double b1x, double b1y, double b1z, double b2x, double b2y,
                                          double b2z, double& ox, double& oy, double& oz) {
    double a[4][4], v[4][4];  // a[c][r] = A(r, c): the Jacobi rotates COLUMNS; v[c] = column c of V
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        a[c][0] = b1x * p1[8 + c] - b1z * p1[c];
        a[c][1] = b1y * p1[8 + c] - b1z * p1[4 + c];
        a[c][2] = b2x * p2[8 + c] - b2z * p2[c];
        a[c][3] = b2y * p2[8 + c] - b2z * p2[4 + c];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[c][r] = r == c ? 1.0 : 0.0;
    }
#pragma unroll 1
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double alpha = (a[p][0] * a[p][0] + a[p][1] * a[p][1]) + (a[p][2] * a[p][2] + a[p][3] * a[p][3]);
                const double beta = (a[q][0] * a[q][0] + a[q][1] * a[q][1]) + (a[q][2] * a[q][2] + a[q][3] * a[q][3]);
                const double gamma = (a[p][0] * a[q][0] + a[p][1] * a[q][1]) + (a[p][2] * a[q][2] + a[p][3] * a[q][3]);
                if (gamma != 0.0 && fabs(gamma) > kJacobiTol * sqrt(alpha * beta)) {
                    rotated = true;
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double ap = a[p][r], aq = a[q][r], vp = v[p][r], vq = v[q][r];
                        a[p][r] = cs * ap - sn * aq;
                        a[q][r] = sn * ap + cs * aq;
                        v[p][r] = cs * vp - sn * vq;
                        v[q][r] = sn * vp + cs * vq;
                    }
                }
            }
        }
        if (!rotated) break;
    }
    // the right singular vector of the smallest singular value: the column of V whose rotated column of A is the shortest
    double best = 1.7976931348623157e308, x0 = 0.0, x1 = 0.0, x2 = 0.0, x3 = 1.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double nrm = (a[c][0] * a[c][0] + a[c][1] * a[c][1]) + (a[c][2] * a[c][2] + a[c][3] * a[c][3]);
        if (nrm < best) best = nrm, x0 = v[c][0], x1 = v[c][1], x2 = v[c][2], x3 = v[c][3];
    }
    ox = x0 / x3, oy = x1 / x3, oz = x2 / x3;
}

// data::triangulate_stereo (data/common.cc:192-261) of a perspective / fisheye / radial-division camera: `(x - cx_) * depth * fx_inv_` is a
// double expression (cx_, fx_inv_ are doubles) rounded to `const float unproj_x`, then widened into pos_c
__device__ inline void triangulate_stereo(const TriView& V, float x, float y, float depth, double& ox, double& oy, double& oz) {
    if (0.0 < depth) {
        const float unproj_x = (float)(((double)x - V.cam.cx) * (double)depth * V.fx_inv);
        const float unproj_y = (float)(((double)y - V.cam.cy) * (double)depth * V.fy_inv);
        const double px = unproj_x, py = unproj_y, pz = depth;
        const double* R = V.pose_cw;  // rot_wc = rot_cw^T
        ox = dot3(R[0], R[4], R[8], px, py, pz) + V.trans_wc[0];
        oy = dot3(R[1], R[5], R[9], px, py, pz) + V.trans_wc[1];
        oz = dot3(R[2], R[6], R[10], px, py, pz) + V.trans_wc[2];
    }
    else ox = oy = oz = 0.0;
}

// check_depth_is_positive + check_reprojection_error of one view (two_view_triangulator.h:89-92, .cc:98-129): 0 = passed
__device__ inline int check_view(const TriView& V, double pwx, double pwy, double pwz, float kx, float ky, float x_right, float sigma_sq, bool is_stereo,
                                 bool& depth_ok) {
    const double* R = V.pose_cw;
    const double X = dot3(R[0], R[1], R[2], pwx, pwy, pwz) + R[3];
    const double Y = dot3(R[4], R[5], R[6], pwx, pwy, pwz) + R[7];
    const double Z = dot3(R[8], R[9], R[10], pwx, pwy, pwz) + R[11];
    depth_ok = V.cam.model == SVGPU_CAM_EQUIRECTANGULAR || 0 < Z;
    if (!depth_ok) return SV_TRI_DEPTH;
    constexpr float chi_sq_2D = 5.99146f, chi_sq_3D = 7.81473f;
    double rx = 0.0, ry = 0.0;
    float xr = 0.f;
    (void)svfd::project_to_image(V.cam, X, Y, Z, rx, ry, xr);  // the reference ignores reproject_to_image's return value
    const double ex = rx - (double)kx, ey = ry - (double)ky;
    const double sq = ex * ex + ey * ey;
    if (is_stereo) {
        const float exr = xr - x_right;
        if ((double)(chi_sq_3D * sigma_sq) < sq + (double)(exr * exr)) return SV_TRI_REPROJECTION;
    }
    else if ((double)(chi_sq_2D * sigma_sq) < sq) return SV_TRI_REPROJECTION;
    return SV_TRI_ACCEPTED;
}
// two_view_triangulator::triangulate (.cc:19-96) for keypoint i1 of V1 and keypoint i2 of V2 (both in range): the status byte, and the
// position of the accepted or rejected candidate (zeros when no mode applies)
__device__ __forceinline__ int triangulate_match(const TriView& V1, const TriView& V2, const int i1, const int i2, const float* scale_factors,
                                                 const float* level_sigma_sq, const float cos_rays_parallax_thr, double& pwx, double& pwy, double& pwz) {
    int st;
    const float k1x = V1.xy[2 * i1], k1y = V1.xy[2 * i1 + 1], k2x = V2.xy[2 * i2], k2y = V2.xy[2 * i2 + 1];
    const float xr1 = V1.xright ? V1.xright[i1] : -1.0f, xr2 = V2.xright ? V2.xright[i2] : -1.0f;
    const bool is_stereo_1 = 0 <= xr1, is_stereo_2 = 0 <= xr2;
    const double b1x = V1.bearings[3 * i1], b1y = V1.bearings[3 * i1 + 1], b1z = V1.bearings[3 * i1 + 2];
    const double b2x = V2.bearings[3 * i2], b2y = V2.bearings[3 * i2 + 1], b2z = V2.bearings[3 * i2 + 2];
    // rays with the world reference: rot_wk * ray_c_k, rot_wk = rot_kw^T
    const double *R1 = V1.pose_cw, *R2 = V2.pose_cw;
    const double w1x = dot3(R1[0], R1[4], R1[8], b1x, b1y, b1z), w1y = dot3(R1[1], R1[5], R1[9], b1x, b1y, b1z), w1z = dot3(R1[2], R1[6], R1[10], b1x, b1y, b1z);
    const double w2x = dot3(R2[0], R2[4], R2[8], b2x, b2y, b2z), w2y = dot3(R2[1], R2[5], R2[9], b2x, b2y, b2z), w2z = dot3(R2[2], R2[6], R2[10], b2x, b2y, b2z);
    const double cos_rays_parallax = dot3(w1x, w1y, w1z, w2x, w2y, w2z);
    const float depth_1 = V1.depth ? V1.depth[i1] : -1.0f, depth_2 = V2.depth ? V2.depth[i2] : -1.0f;
    const double cos_stereo_parallax_1 = is_stereo_1 ? cos(2.0 * atan2(V1.true_baseline / 2.0, (double)depth_1)) : 2.0;
    const double cos_stereo_parallax_2 = is_stereo_2 ? cos(2.0 * atan2(V2.true_baseline / 2.0, (double)depth_2)) : 2.0;
    const double cos_stereo_parallax = fmin(cos_stereo_parallax_1, cos_stereo_parallax_2);
    const bool triangulate_with_two_cameras = ((!is_stereo_1 && !is_stereo_2) && 0.0 < cos_rays_parallax && cos_rays_parallax < (double)cos_rays_parallax_thr)
                                              || ((is_stereo_1 || is_stereo_2) && 0.0 < cos_rays_parallax && cos_rays_parallax < cos_stereo_parallax);
    st = SV_TRI_ACCEPTED;
    if (triangulate_with_two_cameras) triangulate_linear(R1, R2, b1x, b1y, b1z, b2x, b2y, b2z, pwx, pwy, pwz);
    else if (is_stereo_1 && cos_stereo_parallax_1 < cos_stereo_parallax_2) triangulate_stereo(V1, k1x, k1y, depth_1, pwx, pwy, pwz);
    else if (is_stereo_2 && cos_stereo_parallax_2 < cos_stereo_parallax_1) triangulate_stereo(V2, k2x, k2y, depth_2, pwx, pwy, pwz);
    else st = SV_TRI_NO_MODE;
    if (st == SV_TRI_ACCEPTED) {
        const int o1 = V1.octave[i1], o2 = V2.octave[i2];
        bool d1, d2;
        const int c1 = check_view(V1, pwx, pwy, pwz, k1x, k1y, xr1, level_sigma_sq[o1], is_stereo_1, d1);
        const int c2 = check_view(V2, pwx, pwy, pwz, k2x, k2y, xr2, level_sigma_sq[o2], is_stereo_2, d2);
        if (!d1 || !d2) st = SV_TRI_DEPTH;  // both depth tests precede both reprojection tests (.cc:70-82)
        else if (c1 || c2) st = SV_TRI_REPROJECTION;
        else {  // check_scale_factors, two_view_triangulator.h:94-110
            const double u1 = pwx - V1.trans_wc[0], u2 = pwy - V1.trans_wc[1], u3 = pwz - V1.trans_wc[2];
            const double cam_1_to_lm_dist = sqrt((u1 * u1 + u2 * u2) + u3 * u3);
            const double t1 = pwx - V2.trans_wc[0], t2 = pwy - V2.trans_wc[1], t3 = pwz - V2.trans_wc[2];
            const double cam_2_to_lm_dist = sqrt((t1 * t1 + t2 * t2) + t3 * t3);
            if (cam_1_to_lm_dist == 0 || cam_2_to_lm_dist == 0) st = SV_TRI_SCALE;
            else {
                const double ratio_dists = cam_2_to_lm_dist / cam_1_to_lm_dist;
                const float ratio_octave = scale_factors[o1] / scale_factors[o2];
                const double ratio_factor = V2.ratio_factor;
                if (!((double)ratio_octave / ratio_dists < ratio_factor && ratio_dists / (double)ratio_octave < ratio_factor)) st = SV_TRI_SCALE;
            }
        }
    }
    return st;
}

}  // namespace svtri
