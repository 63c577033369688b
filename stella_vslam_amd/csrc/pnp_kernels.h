// Problem descriptors and launchers of the PnP kernels (pnp_kernels.hip): solve::pnp_solver (solve/pnp_solver.cc) on the device.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// k_pnp_pose: pnp_solver::compute_pose (:155-206) for num_sets correspondence sets, one wavefront per set.  Set s is the range
// off[s] .. off[s + 1] of bearings / pos_w; with `idx` it is the `count[s]` correspondences idx[off[s] + i] of that range (indices local
// to the range, the compacted inliers of k_pnp_select).  `enable` (nullable): sets whose byte is 0 are left alone.  `sets` (nullable):
// workgroup b owns set sets[b] of num_launch listed sets, else set b of num_sets.
struct PnpPoseProblem {
    const double* bearings;
    const double* pos_w;
    const int32_t* off;
    const uint32_t* idx;
    const int32_t* count;
    const uint8_t* enable;
    const int32_t* sets;
    int num_launch;
    double* pose;  // num_sets x 12: rows 0..2 of [R | t], row-major
    double* err;   // nullable: the reprojection error compute_pose returns
    int num_sets;
    int gn_iter;
    int keep_on_failure;  // != 0: a set for which no N gave a comparable error keeps what `pose` holds (the recompute of find_via_ransac)
};

// k_pnp_ransac: find_via_ransac steps 2-1 .. 2-3 (:71-92), one wavefront per hypothesis (active problem x iteration).
// k_pnp_select: step 2-4 and the validity rule (:94-103), one wavefront per active problem.
struct PnpRansacProblem {
    const double* bearings;
    const double* pos_w;
    const float* max_cos;      // max_cos_errors_ per match (a float vector in the reference)
    const int32_t* match_off;  // num_problems + 1
    const uint32_t* samples;   // num_problems x num_iter x 4, local to the problem
    const int32_t* active;     // problems that run (num_matches >= 4 and >= min_num_inliers)
    int num_problems, num_active, num_iter, gn_iter;
    unsigned min_num_inliers;
    int recompute;
    // hypotheses: index p * num_iter + it; inlier bytes of (p, it) at num_iter * match_off[p] + it * n_p
    double* hyp_pose;
    int32_t* hyp_num_inliers;
    double* hyp_cost;
    uint8_t* hyp_inlier;
    // results
    uint8_t* valid;
    double* pose;
    uint8_t* is_inlier;
    int32_t* best_iter;
    uint32_t* inl_idx;   // recompute: the winner's inliers in ascending order, at match_off[p]
    int32_t* inl_count;  // recompute: their number
};

void sv_launch_pnp_pose(hipStream_t s, const PnpPoseProblem& P);
void sv_launch_pnp_ransac(hipStream_t s, const PnpRansacProblem& P);
void sv_launch_pnp_select(hipStream_t s, const PnpRansacProblem& P);

// ---- the host side of find_via_ransac in the form a call takes that has its matches on the device already (svgpu_pnp.hip):
// max_cos_errors_ of one scale factor (:27-32), the check of one problem's num_iter x 4 sample table against its np matches (null, or what
// is wrong with it), and the launches of svgpu_pnp_ransac_batch over placed pieces (pnp_layout.h) -- hypotheses, selection and, with
// `recompute`, the pose over the winner's inliers.  Returns the launches it issued.
struct svgpu_ctx;
struct PnpRansacPieces;
float sv_pnp_max_cos(float scale_factor);
const char* sv_pnp_check_samples(const uint32_t* samples, int num_iter, unsigned np);
int sv_pnp_ransac_enqueue(svgpu_ctx* ctx, hipStream_t s, const PnpRansacPieces& Y, int num_problems, int num_active, int num_iter, int gn_iter,
                          int min_num_inliers, int recompute);
