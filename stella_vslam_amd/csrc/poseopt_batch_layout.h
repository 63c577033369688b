// The scratch-arena layout of svgpu_pose_optimize_batch (svgpu_ba.hip), as a function of an arena: run on a measuring arena it gives the
// bytes the call asks for, run on the placing arena it hands out the pieces.  Plain C++ (no HIP):
// tests/poseopt_batch_arena_check.cpp compiles this header with sv_arena.h alone.
#pragma once
#include <cstddef>
#include <cstdint>

#include "sv_arena.h"

struct PoseOptBatchPieces {
    // uploaded
    int32_t* obs_off;   // P + 1
    double* pose_in;    // P x 12
    uint8_t* active;    // P, the caller's or all ones
    double* pos_w;      // n x 3
    float* uvr;         // n x 3
    float *w, *huber;   // n
    uint8_t* select;    // n, the caller's or all ones
    // device only: the compacted copies of the selected entries (problem p's start at obs_off[p], as its entries do) and the per-entry
    // scratch of the optimisation
    double* c_pos;
    float *c_uvr, *c_w, *c_huber;
    int32_t* entry_of;  // compacted observation -> entry of its problem
    uint8_t *level, *robust, *outlier;
    // results, next to one another: one copy back
    double* pose_out;   // P x 12
    int32_t* result;    // P x 4: num_valid, LM iterations, num_bad, selected entries
    uint8_t* flags;     // n
};
// P problems with n entries in all
template <class A>
void poseopt_batch_layout(A& arena, size_t P, size_t n, PoseOptBatchPieces& Y) {
    Y.obs_off = arena.template take<int32_t>(P + 1);
    Y.pose_in = arena.template take<double>(12 * P);
    Y.active = arena.template take<uint8_t>(P);
    Y.pos_w = arena.template take<double>(3 * n);
    Y.uvr = arena.template take<float>(3 * n);
    Y.w = arena.template take<float>(n);
    Y.huber = arena.template take<float>(n);
    Y.select = arena.template take<uint8_t>(n);
    Y.c_pos = arena.template take<double>(3 * n);
    Y.c_uvr = arena.template take<float>(3 * n);
    Y.c_w = arena.template take<float>(n);
    Y.c_huber = arena.template take<float>(n);
    Y.entry_of = arena.template take<int32_t>(n);
    Y.level = arena.template take<uint8_t>(n);
    Y.robust = arena.template take<uint8_t>(n);
    Y.outlier = arena.template take<uint8_t>(n);
    Y.pose_out = arena.template take<double>(12 * P);
    Y.result = arena.template take<int32_t>(4 * P);
    Y.flags = arena.template take<uint8_t>(n);
}
