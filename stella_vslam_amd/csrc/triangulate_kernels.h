// Two-view triangulation of keypoint matches (module/two_view_triangulator.{h,cc}, solve/triangulator.h:76-88,
// data/common.cc:192-261): one lane per match, every gate of two_view_triangulator::triangulate inside the lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svgpu_internal.h"

// status byte of a match (include/svgpu.h SVGPU_TRI_*)
#define SV_TRI_ACCEPTED 0
#define SV_TRI_NO_MODE 1
#define SV_TRI_DEPTH 2
#define SV_TRI_REPROJECTION 3
#define SV_TRI_SCALE 4
#define SV_TRI_SKIPPED 255

// What the triangulator reads of one keyframe: camera, pose and the per-keypoint arrays of its frame_observation (device pointers).
struct TriView {
    svgpu_camera cam;
    double pose_cw[12];    // rows 0..2 of cam_pose_cw: [rot_cw | trans_cw]
    double trans_wc[3];    // cam_center (keyframe::get_trans_wc)
    double true_baseline;  // camera::base::true_baseline_
    double fx_inv, fy_inv; // perspective.cc:17 fx_inv_(1.0 / fx)
    const float* xy;       // n x 2 undistorted keypoints
    const int32_t* octave; // n
    const double* bearings;// n x 3
    const float* xright;   // n, nullable (stereo_x_right_.empty())
    const float* depth;    // n, nullable (depths_.empty())
    float ratio_factor;    // 2.0f * max(scale_factor_1, scale_factor of this view); side 1 does not use its own
    int n;
};

struct TriProblem {
    TriView v1;                  // the current keyframe (side 1 of every match)
    const TriView* nb;           // num_nb neighbours (device)
    const int32_t* nb_of_match;  // per match the neighbour it belongs to
    const int32_t* nb_first;     // per neighbour its first match (device, num_nb entries): only read in the matched_2_in_1 form
    const int32_t* idx1;
    const int32_t* idx2;         // null: idx1 is matched_2_in_1 per neighbour (entry j of a neighbour's range = keypoint j of side 1)
    int num_matches;
    float scale_factors[SV_MAX_LEVELS];
    float level_sigma_sq[SV_MAX_LEVELS];
    float cos_rays_parallax_thr;  // float, as two_view_triangulator::cos_rays_parallax_thr_
    double* pos_w;                // num_matches x 3
    uint8_t* status;              // num_matches
};
void sv_launch_triangulate_two_views(hipStream_t s, const TriProblem& P);
