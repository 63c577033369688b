// The scratch-arena layouts of the PnP entry points (svgpu_pnp.hip), as functions of an arena: run on a measuring arena they give the
// bytes the call asks for, run on the placing arena they hand out the pieces.  Plain C++ (no HIP): tests/pnp_arena_check.cpp compiles
// this header with sv_arena.h alone.
#pragma once
#include <cstddef>
#include <cstdint>

#include "sv_arena.h"

struct PnpPosePieces {
    Piece<double> bearings, pos_w;  // uploaded
    Piece<int32_t> off;             // uploaded
    Piece<double> pose, err;        // results
};
// svgpu_pnp_compute_pose: num_sets sets over n correspondences in all
template <class A>
void pnp_pose_layout(A& arena, size_t num_sets, size_t n, PnpPosePieces& Y) {
    Y.bearings = arena.template piece<double>(3 * n);
    Y.pos_w = arena.template piece<double>(3 * n);
    Y.off = arena.template piece<int32_t>(num_sets + 1);
    Y.pose = arena.template piece<double>(12 * num_sets);
    Y.err = arena.template piece<double>(num_sets);
}

struct PnpRansacPieces {
    // uploaded
    Piece<double> bearings, pos_w;
    Piece<float> max_cos;
    Piece<int32_t> match_off;
    Piece<uint32_t> samples;
    Piece<int32_t> active;
    // hypotheses
    Piece<double> hyp_pose;
    Piece<int32_t> hyp_num_inliers;
    Piece<double> hyp_cost;
    Piece<uint8_t> hyp_inlier;
    // results
    Piece<uint8_t> valid;
    Piece<double> pose;
    Piece<uint8_t> is_inlier;
    Piece<int32_t> best_iter;
    Piece<uint32_t> inl_idx;  // these two with `recompute` only, else empty
    Piece<int32_t> inl_count;
};
// svgpu_pnp_ransac_batch: num_problems problems over n matches in all, num_iter hypotheses each, num_active of them running
template <class A>
void pnp_ransac_layout(A& arena, size_t num_problems, size_t n, size_t num_iter, size_t num_active, bool recompute, PnpRansacPieces& Y) {
    const size_t hyp = num_problems * num_iter;
    Y.bearings = arena.template piece<double>(3 * n);
    Y.pos_w = arena.template piece<double>(3 * n);
    Y.max_cos = arena.template piece<float>(n);
    Y.match_off = arena.template piece<int32_t>(num_problems + 1);
    Y.samples = arena.template piece<uint32_t>(4 * hyp);
    Y.active = arena.template piece<int32_t>(num_active);
    Y.hyp_pose = arena.template piece<double>(12 * hyp);
    Y.hyp_num_inliers = arena.template piece<int32_t>(hyp);
    Y.hyp_cost = arena.template piece<double>(hyp);
    Y.hyp_inlier = arena.template piece<uint8_t>(num_iter * n);
    Y.valid = arena.template piece<uint8_t>(num_problems);
    Y.pose = arena.template piece<double>(12 * num_problems);
    Y.is_inlier = arena.template piece<uint8_t>(n);
    Y.best_iter = arena.template piece<int32_t>(num_problems);
    Y.inl_idx = recompute ? arena.template piece<uint32_t>(n) : Piece<uint32_t>{};
    Y.inl_count = recompute ? arena.template piece<int32_t>(num_problems) : Piece<int32_t>{};
}
