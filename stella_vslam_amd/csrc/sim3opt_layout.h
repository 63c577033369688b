// The scratch-arena layout of svgpu_sim3_transform_optimize_batch (svgpu_sim3opt.hip), as a function of an arena: run on a measuring arena
// it gives the bytes the call asks for, run on the placing arena it hands out the pieces.  Plain C++ (no HIP):
// tests/sim3opt_arena_check.cpp compiles this header with sv_arena.h alone.
#pragma once
#include <cstddef>
#include <cstdint>

#include "sv_arena.h"

#define S3O_LAYOUT_PROBLEM 344  // bytes of a problem descriptor (sizeof(Sim3OptProblem) of sim3opt_kernels.h; svgpu_sim3opt.hip asserts they agree)
#define S3O_LAYOUT_STATS 64     // bytes of svgpu_sim3opt_stats (asserted there too)

struct Sim3OptPieces {
    // uploaded
    Piece<char> prob;
    Piece<double> obs1, obs2;
    Piece<float> w1, w2;
    Piece<double> pos1, pos2;
    // device only
    Piece<double> chi_cache;  // the cached chi2 of every edge: two per match
    // results
    Piece<double> sim3_out;
    Piece<int32_t> num_inliers;
    Piece<uint8_t> status;
    Piece<char> stats;
};
// P problems with n matches in all
template <class A>
void sim3opt_layout(A& arena, size_t P, size_t n, Sim3OptPieces& Y) {
    Y.prob = arena.template piece<char>(S3O_LAYOUT_PROBLEM * P);
    Y.obs1 = arena.template piece<double>(2 * n);
    Y.obs2 = arena.template piece<double>(2 * n);
    Y.w1 = arena.template piece<float>(n);
    Y.w2 = arena.template piece<float>(n);
    Y.pos1 = arena.template piece<double>(3 * n);
    Y.pos2 = arena.template piece<double>(3 * n);
    Y.chi_cache = arena.template piece<double>(2 * n);
    Y.sim3_out = arena.template piece<double>(8 * P);
    Y.num_inliers = arena.template piece<int32_t>(P);
    Y.status = arena.template piece<uint8_t>(n);
    Y.stats = arena.template piece<char>(S3O_LAYOUT_STATS * P);
}
