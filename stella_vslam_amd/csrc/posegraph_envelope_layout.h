// The scratch pieces of the pose graph's envelope solver (posegraph_envelope.hip), as a function of an arena like posegraph_layout.h: the
// envelope's values, the plan arrays of posegraph_envelope_plan.h and the pair lists.  They follow the pieces of pg_optimize_layout in
// the same arena.  Plain C++ (no HIP): tests/posegraph_envelope_arena_check.cpp compiles this header with sv_arena.h alone.
#pragma once
#include <cstddef>
#include <cstdint>

#include "sv_arena.h"

#define PG_ENV_LAYOUT_CTL 64  // bytes reserved for PgEnvCtl (asserted in svgpu_posegraph.hip)

struct PgEnvPieces {
    // uploaded
    Piece<char> ctl;
    Piece<int32_t> order, rowoff, coloff, colrows, colbase, blk_src, pair_off, pair_ent, pair_flag;
    // device only
    Piece<double> val, dinv, y;
};
// nfree block rows, nblocks envelope blocks (diagonal included), num_pairs free-free pairs with pair_entries edges in their lists
template <class A>
void pg_envelope_layout(A& arena, size_t nfree, size_t nblocks, size_t num_pairs, size_t pair_entries, PgEnvPieces& Y) {
    Y.ctl = arena.template piece<char>(PG_ENV_LAYOUT_CTL);
    Y.order = arena.template piece<int32_t>(nfree);
    Y.rowoff = arena.template piece<int32_t>(nfree + 1);
    Y.coloff = arena.template piece<int32_t>(nfree + 1);
    Y.colrows = arena.template piece<int32_t>(nblocks - nfree);
    Y.colbase = arena.template piece<int32_t>(nblocks - nfree);
    Y.blk_src = arena.template piece<int32_t>(nblocks);
    Y.pair_off = arena.template piece<int32_t>(num_pairs + 1);
    Y.pair_ent = arena.template piece<int32_t>(pair_entries);
    Y.pair_flag = arena.template piece<int32_t>(num_pairs);
    Y.val = arena.template piece<double>(49 * nblocks);
    Y.dinv = arena.template piece<double>(49 * nfree);
    Y.y = arena.template piece<double>(7 * nfree);
}

// svgpu_selftest_pose_graph_envelope_solve: the caller's system in front of the solver's pieces
struct PgEnvSelftestPieces {
    Piece<char> ctl;  // a PgCtl whose phase says "a trial runs"
    Piece<double> diag, blocks, rhs, x;
    PgEnvPieces env;
};
template <class A>
void pg_envelope_selftest_layout(A& arena, size_t nfree, size_t nblocks, size_t num_pairs, size_t pair_entries, size_t num_input_pairs, PgEnvSelftestPieces& Y) {
    Y.ctl = arena.template piece<char>(128);
    Y.diag = arena.template piece<double>(49 * nfree);
    Y.blocks = arena.template piece<double>(49 * num_input_pairs);
    Y.rhs = arena.template piece<double>(7 * nfree);
    Y.x = arena.template piece<double>(7 * nfree);
    pg_envelope_layout(arena, nfree, nblocks, num_pairs, pair_entries, Y.env);
}
