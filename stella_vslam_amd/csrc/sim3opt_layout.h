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
    char* prob;
    double *obs1, *obs2;
    float *w1, *w2;
    double *pos1, *pos2;
    // device only
    double* chi_cache;  // the cached chi2 of every edge: two per match
    // results
    double* sim3_out;
    int32_t* num_inliers;
    uint8_t* status;
    char* stats;
};
// P problems with n matches in all
template <class A>
void sim3opt_layout(A& arena, size_t P, size_t n, Sim3OptPieces& Y) {
    Y.prob = arena.template take<char>(S3O_LAYOUT_PROBLEM * P);
    Y.obs1 = arena.template take<double>(2 * n);
    Y.obs2 = arena.template take<double>(2 * n);
    Y.w1 = arena.template take<float>(n);
    Y.w2 = arena.template take<float>(n);
    Y.pos1 = arena.template take<double>(3 * n);
    Y.pos2 = arena.template take<double>(3 * n);
    Y.chi_cache = arena.template take<double>(2 * n);
    Y.sim3_out = arena.template take<double>(8 * P);
    Y.num_inliers = arena.template take<int32_t>(P);
    Y.status = arena.template take<uint8_t>(n);
    Y.stats = arena.template take<char>(S3O_LAYOUT_STATS * P);
}
