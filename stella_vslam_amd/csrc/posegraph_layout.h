// The scratch-arena layouts of the pose-graph entry points (svgpu_posegraph.hip), as functions of an arena: run on a measuring arena they
// give the bytes the call asks for, run on the placing arena they hand out the pieces.  Plain C++ (no HIP):
// tests/posegraph_arena_check.cpp compiles this header with sv_arena.h alone.
#pragma once
#include <cstddef>
#include <cstdint>

#include "sv_arena.h"

#define PG_LAYOUT_REC 162     // doubles per edge record (PG_REC of posegraph_kernels.h; svgpu_posegraph.hip asserts they agree)
#define PG_LAYOUT_CTL 128     // bytes reserved for the control block (>= sizeof(PgCtl), asserted there too)

struct PgPieces {
    // uploaded
    Piece<char> ctl;
    Piece<double> est0;  // the estimate buffer the input goes to
    Piece<uint8_t> fixed;
    Piece<int32_t> slot, e_i, e_j;
    Piece<double> meas;
    Piece<int32_t> v_off, v_ent;
    // device only
    Piece<double> est1;
    Piece<double> rec, chi_trial, Hd, b, maxd, Minv, x, r, z, p, Ap, scale_part;
    // results
    Piece<double> out_sim3, out_pose;
};
// svgpu_pose_graph_optimize: N vertices of which nfree are free, E edges, `incident` entries in the free vertices' edge lists (<= 2 E)
template <class A>
void pg_optimize_layout(A& arena, size_t N, size_t E, size_t nfree, size_t incident, PgPieces& Y) {
    const size_t n = 7 * nfree;
    Y.ctl = arena.template piece<char>(PG_LAYOUT_CTL);
    Y.est0 = arena.template piece<double>(8 * N);
    Y.fixed = arena.template piece<uint8_t>(N);
    Y.slot = arena.template piece<int32_t>(N);
    Y.e_i = arena.template piece<int32_t>(E);
    Y.e_j = arena.template piece<int32_t>(E);
    Y.meas = arena.template piece<double>(8 * E);
    Y.v_off = arena.template piece<int32_t>(nfree + 1);
    Y.v_ent = arena.template piece<int32_t>(incident);
    Y.est1 = arena.template piece<double>(8 * N);
    Y.rec = arena.template piece<double>(PG_LAYOUT_REC * E);
    Y.chi_trial = arena.template piece<double>(E);
    Y.Hd = arena.template piece<double>(49 * nfree);
    Y.b = arena.template piece<double>(n);
    Y.maxd = arena.template piece<double>(nfree);
    Y.Minv = arena.template piece<double>(49 * nfree);
    Y.x = arena.template piece<double>(n);
    Y.r = arena.template piece<double>(n);
    Y.z = arena.template piece<double>(n);
    Y.p = arena.template piece<double>(n);
    Y.Ap = arena.template piece<double>(n);
    Y.scale_part = arena.template piece<double>(nfree);
    Y.out_sim3 = arena.template piece<double>(8 * N);
    Y.out_pose = arena.template piece<double>(12 * N);
}

struct PgLandmarkPieces {
    Piece<double> before, after;  // uploaded
    Piece<int32_t> ref;
    Piece<double> pos_in;
    Piece<double> pos_out;        // result
};
// svgpu_pose_graph_correct_landmarks: N vertices, L landmarks
template <class A>
void pg_landmarks_layout(A& arena, size_t N, size_t L, PgLandmarkPieces& Y) {
    Y.before = arena.template piece<double>(8 * N);
    Y.after = arena.template piece<double>(8 * N);
    Y.ref = arena.template piece<int32_t>(L);
    Y.pos_in = arena.template piece<double>(3 * L);
    Y.pos_out = arena.template piece<double>(3 * L);
}
