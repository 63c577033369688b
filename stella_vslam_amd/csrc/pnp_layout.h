// The scratch-arena layouts of the PnP entry points (svgpu_pnp.hip), as functions of an arena: run on a measuring arena they give the
// bytes the call asks for, run on the placing arena they hand out the pieces.  Plain C++ (no HIP): tests/pnp_arena_check.cpp compiles
// this header with sv_arena.h alone.
#pragma once
#include <cstddef>
#include <cstdint>

#include "sv_arena.h"

struct PnpPosePieces {
    double *bearings, *pos_w;  // uploaded
    int32_t* off;              // uploaded
    double *pose, *err;        // results
};
// svgpu_pnp_compute_pose: num_sets sets over n correspondences in all
template <class A>
void pnp_pose_layout(A& arena, size_t num_sets, size_t n, PnpPosePieces& Y) {
    Y.bearings = arena.template take<double>(3 * n);
    Y.pos_w = arena.template take<double>(3 * n);
    Y.off = arena.template take<int32_t>(num_sets + 1);
    Y.pose = arena.template take<double>(12 * num_sets);
    Y.err = arena.template take<double>(num_sets);
}

struct PnpRansacPieces {
    // uploaded
    double *bearings, *pos_w;
    float* max_cos;
    int32_t* match_off;
    uint32_t* samples;
    int32_t* active;
    // hypotheses
    double* hyp_pose;
    int32_t* hyp_num_inliers;
    double* hyp_cost;
    uint8_t* hyp_inlier;
    // results
    uint8_t* valid;
    double* pose;
    uint8_t* is_inlier;
    int32_t* best_iter;
    uint32_t* inl_idx;
    int32_t* inl_count;
};
// svgpu_pnp_ransac_batch: num_problems problems over n matches in all, num_iter hypotheses each, num_active of them running
template <class A>
void pnp_ransac_layout(A& arena, size_t num_problems, size_t n, size_t num_iter, size_t num_active, bool recompute, PnpRansacPieces& Y) {
    const size_t hyp = num_problems * num_iter;
    Y.bearings = arena.template take<double>(3 * n);
    Y.pos_w = arena.template take<double>(3 * n);
    Y.max_cos = arena.template take<float>(n);
    Y.match_off = arena.template take<int32_t>(num_problems + 1);
    Y.samples = arena.template take<uint32_t>(4 * hyp);
    Y.active = arena.template take<int32_t>(num_active);
    Y.hyp_pose = arena.template take<double>(12 * hyp);
    Y.hyp_num_inliers = arena.template take<int32_t>(hyp);
    Y.hyp_cost = arena.template take<double>(hyp);
    Y.hyp_inlier = arena.template take<uint8_t>(num_iter * n);
    Y.valid = arena.template take<uint8_t>(num_problems);
    Y.pose = arena.template take<double>(12 * num_problems);
    Y.is_inlier = arena.template take<uint8_t>(n);
    Y.best_iter = arena.template take<int32_t>(num_problems);
    Y.inl_idx = recompute ? arena.template take<uint32_t>(n) : nullptr;
    Y.inl_count = recompute ? arena.template take<int32_t>(num_problems) : nullptr;
}
