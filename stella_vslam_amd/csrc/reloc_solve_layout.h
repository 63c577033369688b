// The scratch-arena layout of svgpu_reloc_solve_batch (svgpu_reloc.hip), as a function of an arena: run on a measuring arena it gives the
// bytes the call asks for, run on the placing arena it hands out the pieces.  It places and does nothing else.  Plain C++ (no HIP):
// tests/reloc_solve_arena_check.cpp compiles this header with sv_arena.h alone.
//
// The call is PnP -> pose optimisation -> bookkeeping -> the stages of svgpu_reloc_refine_batch, so the layout is the refine call's
// (reloc_refine_layout.h) with the pieces of the steps in front of it placed around it:
//   what the call uploads of its own | the refine call's front (its uploads first: ONE copy covers both) | device-only pieces of PnP
//   and the first optimisation | their results | the refine call's results | the candidate lists
// so the results of every step lie next to one another (one copy back) and the lists stay last.
#pragma once
#include <cstddef>
#include <cstdint>

#include "pnp_layout.h"
#include "reloc_refine_layout.h"
#include "sv_arena.h"

struct RelocSolveShape {
    RelocRefineShape refine;  // K, nt, N, S, grid, optional arrays, replay tables, list capacity
    size_t M = 0;             // 2D-3D matches of all candidates (match_off[K])
    size_t I = 0;             // RANSAC iterations
    size_t num_active = 0;    // candidates whose PnP runs
    bool recompute = false;
};

struct RelocSolvePieces {
    // ---- uploaded
    Piece<double> t_bearings;   // nt x 3
    Piece<int32_t> m_keypt;     // M
    Piece<int32_t> m_kf_entry;  // M
    // ---- PnP: match_off, samples, active and pos_w (= m_pos_w) are uploaded; bearings and max_cos are written by the gather kernel;
    //      valid, pose, is_inlier and best_iter are results
    PnpRansacPieces pnp;
    // ---- device only: the first optimisation's observations per match entry (gather kernel), its compacted copies and scratch
    Piece<float> o_uvr, o_w, o_huber;  // M (x 3)
    Piece<double> oc_pos;
    Piece<float> oc_uvr, oc_w, oc_huber;
    Piece<int32_t> o_entry_of;
    Piece<uint8_t> o_level, o_robust, o_outlier;
    // ---- results of the first optimisation, behind PnP's and in front of the refine call's
    Piece<double> opt_pose;      // K x 12 (the stages' input pose)
    Piece<int32_t> opt_result;   // K x 4: num_valid, LM iterations, num_bad, selected entries
    Piece<uint8_t> opt_flags;    // M: outlier flag per match entry, 0 for a non-inlier
    RelocRefinePieces refine;
};

template <class A>
void reloc_solve_layout(A& arena, const RelocSolveShape& H, RelocSolvePieces& Y) {
    const size_t K = H.refine.K, nt = H.refine.nt, M = H.M, hyp = K * H.I;
    Y.t_bearings = arena.template piece<double>(nt * 3);
    Y.m_keypt = arena.template piece<int32_t>(M);
    Y.m_kf_entry = arena.template piece<int32_t>(M);
    Y.pnp.pos_w = arena.template piece<double>(3 * M);
    Y.pnp.match_off = arena.template piece<int32_t>(K + 1);
    Y.pnp.samples = arena.template piece<uint32_t>(4 * hyp);
    Y.pnp.active = arena.template piece<int32_t>(H.num_active);
    reloc_refine_layout_front(arena, H.refine, Y.refine);
    Y.pnp.bearings = arena.template piece<double>(3 * M);
    Y.pnp.max_cos = arena.template piece<float>(M);
    Y.pnp.hyp_pose = arena.template piece<double>(12 * hyp);
    Y.pnp.hyp_num_inliers = arena.template piece<int32_t>(hyp);
    Y.pnp.hyp_cost = arena.template piece<double>(hyp);
    Y.pnp.hyp_inlier = arena.template piece<uint8_t>(H.I * M);
    Y.pnp.inl_idx = optional_piece<uint32_t>(arena, H.recompute, M);
    Y.pnp.inl_count = optional_piece<int32_t>(arena, H.recompute, K);
    Y.o_uvr = arena.template piece<float>(M * 3);
    Y.o_w = arena.template piece<float>(M);
    Y.o_huber = arena.template piece<float>(M);
    Y.oc_pos = arena.template piece<double>(M * 3);
    Y.oc_uvr = arena.template piece<float>(M * 3);
    Y.oc_w = arena.template piece<float>(M);
    Y.oc_huber = arena.template piece<float>(M);
    Y.o_entry_of = arena.template piece<int32_t>(M);
    Y.o_level = arena.template piece<uint8_t>(M);
    Y.o_robust = arena.template piece<uint8_t>(M);
    Y.o_outlier = arena.template piece<uint8_t>(M);
    Y.pnp.valid = arena.template piece<uint8_t>(K);
    Y.pnp.pose = arena.template piece<double>(12 * K);
    Y.pnp.is_inlier = arena.template piece<uint8_t>(M);
    Y.pnp.best_iter = arena.template piece<int32_t>(K);
    Y.opt_pose = arena.template piece<double>(12 * K);
    Y.opt_result = arena.template piece<int32_t>(4 * K);
    Y.opt_flags = arena.template piece<uint8_t>(M);
    reloc_refine_layout_back(arena, H.refine, Y.refine);
}
