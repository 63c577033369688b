// The scratch-arena layout of svgpu_pose_optimize_batch (svgpu_ba.hip), as a function of an arena: run on a measuring arena it gives the
// bytes the call asks for, run on the placing arena it hands out the pieces.  Plain C++ (no HIP):
// tests/poseopt_batch_arena_check.cpp compiles this header with sv_arena.h alone.
#pragma once
#include <cstddef>
#include <cstdint>

#include "sv_arena.h"

struct PoseOptBatchPieces {
    // uploaded
    Piece<int32_t> obs_off;  // P + 1
    Piece<double> pose_in;   // P x 12
    Piece<uint8_t> active;   // P, the caller's or all ones
    Piece<double> pos_w;     // n x 3
    Piece<float> uvr;        // n x 3
    Piece<float> w, huber;   // n
    Piece<uint8_t> select;   // n, the caller's or all ones
    // device only: the compacted copies of the selected entries (problem p's start at obs_off[p], as its entries do) and the per-entry
    // scratch of the optimisation
    Piece<double> c_pos;
    Piece<float> c_uvr, c_w, c_huber;
    Piece<int32_t> entry_of;  // compacted observation -> entry of its problem
    Piece<uint8_t> level, robust, outlier;
    // results, next to one another: one copy back
    Piece<double> pose_out;   // P x 12
    Piece<int32_t> result;    // P x 4: num_valid, LM iterations, num_bad, selected entries
    Piece<uint8_t> flags;     // n
};
// P problems with n entries in all
template <class A>
void poseopt_batch_layout(A& arena, size_t P, size_t n, PoseOptBatchPieces& Y) {
    Y.obs_off = arena.template piece<int32_t>(P + 1);
    Y.pose_in = arena.template piece<double>(12 * P);
    Y.active = arena.template piece<uint8_t>(P);
    Y.pos_w = arena.template piece<double>(3 * n);
    Y.uvr = arena.template piece<float>(3 * n);
    Y.w = arena.template piece<float>(n);
    Y.huber = arena.template piece<float>(n);
    Y.select = arena.template piece<uint8_t>(n);
    Y.c_pos = arena.template piece<double>(3 * n);
    Y.c_uvr = arena.template piece<float>(3 * n);
    Y.c_w = arena.template piece<float>(n);
    Y.c_huber = arena.template piece<float>(n);
    Y.entry_of = arena.template piece<int32_t>(n);
    Y.level = arena.template piece<uint8_t>(n);
    Y.robust = arena.template piece<uint8_t>(n);
    Y.outlier = arena.template piece<uint8_t>(n);
    Y.pose_out = arena.template piece<double>(12 * P);
    Y.result = arena.template piece<int32_t>(4 * P);
    Y.flags = arena.template piece<uint8_t>(n);
}
