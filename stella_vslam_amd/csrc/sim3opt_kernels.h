// Problem descriptor and launcher of the pairwise Sim3 optimizer (sim3opt_kernels.hip): optimize::transform_optimizer
// (optimize/transform_optimizer.cc) on the device -- one Sim3 vertex, two unary reprojection edges per match, numeric Jacobians,
// Levenberg-Marquardt with Huber edges in two stages, one persistent workgroup per problem.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "svgpu.h"

#define S3O_THREADS 256  // one edge per thread and pass: 128 matches

struct Sim3OptView {
    double pose[12];   // rows 0..2 of [rot_cw | trans_cw]
    double k[4];       // fx fy cx cy, or cols rows 0 0 for an equirectangular camera
    int32_t equirect;
    int32_t pad;
};
struct Sim3OptProblem {
    Sim3OptView view[2];  // keyframe 1, keyframe 2
    double sim3[8];       // Sim3_12 as it came
    int32_t m_lo, m_hi;   // its matches
};

struct Sim3OptDev {
    int num_problems, fix_scale, num_iter;
    float chi_sq;
    const Sim3OptProblem* prob;
    const double *obs1, *obs2;  // 2 per match
    const float *w1, *w2;       // inv_sigma_sq
    const double *pos1, *pos2;  // 3 per match: the landmark of keyframe 1 / keyframe 2
    double* chi_cache;          // 2 per match: chi2 of the forward / backward edge at their last evaluation
    double* sim3_out;           // 8 per problem
    int32_t* num_inliers;
    uint8_t* status;            // per match
    svgpu_sim3opt_stats* stats;
};

void sv_launch_sim3opt(hipStream_t s, const Sim3OptDev& D);
