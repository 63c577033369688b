// The scratch-arena layouts of the two-pass matchers (svgpu_match.hip, svgpu_match2.hip), as functions of an arena: run on a measuring
// arena they give the bytes a pass asks for, run on the placing arena they hand out the pieces.  They place and do nothing else: the
// call copies and launches.  Plain C++ (no HIP): tests/match_arena_check.cpp compiles this header with sv_arena.h alone.
//
// The prefix invariant.  A second pass whose arena did not regrow reuses what the first pass left in it, so every piece in front of
// the candidate lists must lie at the same offset whether the lists are absent, short or long: the lists are the LAST takes of both
// layouts, and nothing in front of them depends on `lists` or on their capacity.
#pragma once
#include <cstddef>
#include <cstdint>

#include "sv_arena.h"

// Host arrays stand for themselves and for "present": an optional one the caller did not pass (null) gets no piece.
// The query side of svgpu_match_in_cells: the caller's own window arrays.
struct CellQuery {
    const uint8_t* desc;  // nq x 32
    const float *xy, *margin;
    const int32_t *min_level, *max_level;
    const uint8_t* valid;
    const float *angle, *xright, *xr_tol;
    const uint8_t* blocks;
};
struct CellQueryPieces {
    Piece<uint8_t> desc, valid, blocks;  // desc: nq x 32
    Piece<float> xy, margin, angle, xright, xr_tol;
    Piece<int32_t> min_level, max_level;
};
template <class A>
void cell_query_layout(A& arena, size_t nq, const CellQuery& has, CellQueryPieces& Y) {
    Y.desc = arena.template piece<uint8_t>(nq * 32);
    Y.xy = arena.template piece<float>(nq * 2);
    Y.margin = arena.template piece<float>(nq);
    Y.min_level = optional_piece<int32_t>(arena, has.min_level, nq);
    Y.max_level = optional_piece<int32_t>(arena, has.max_level, nq);
    Y.valid = optional_piece<uint8_t>(arena, has.valid, nq);
    Y.angle = optional_piece<float>(arena, has.angle, nq);
    Y.xright = optional_piece<float>(arena, has.xright, nq);
    Y.xr_tol = optional_piece<float>(arena, has.xr_tol, nq);
    Y.blocks = optional_piece<uint8_t>(arena, has.blocks, nq);
}

// The query side of "reproject, then match in cells" (svgpu_match_frame_and_landmarks, the projection family, fuse), and with neither
// descriptors nor windows the whole of svgpu_reproject_landmarks: the landmarks' inputs, the four observability outputs, the four
// window arrays the reprojection writes for the grid lookup.
struct ReprojQuery {
    const uint8_t* desc;  // n x 32
    const double *pos_w, *mean_normal;
    const float *min_valid_dist, *max_valid_dist;
    const uint8_t* skip;
    const int32_t* q_level;
    const float* q_angle;
    const uint8_t* q_blocks;
};
struct ReprojPieces {
    Piece<uint8_t> desc, skip, q_blocks, visible;  // desc: n x 32
    Piece<double> pos_w, mean_normal, reproj;
    Piece<float> min_valid_dist, max_valid_dist, q_angle, x_right, q_xy, q_margin;
    Piece<int32_t> q_level, pred_level, q_min_level, q_max_level;
};
template <class A>
void reproj_layout(A& arena, size_t n, const ReprojQuery& has, bool windows, ReprojPieces& Y) {
    Y.desc = optional_piece<uint8_t>(arena, has.desc, n * 32);
    Y.pos_w = arena.template piece<double>(n * 3);
    Y.mean_normal = optional_piece<double>(arena, has.mean_normal, n * 3);
    Y.min_valid_dist = optional_piece<float>(arena, has.min_valid_dist, n);
    Y.max_valid_dist = optional_piece<float>(arena, has.max_valid_dist, n);
    Y.skip = optional_piece<uint8_t>(arena, has.skip, n);
    Y.q_level = optional_piece<int32_t>(arena, has.q_level, n);
    Y.q_angle = optional_piece<float>(arena, has.q_angle, n);
    Y.q_blocks = optional_piece<uint8_t>(arena, has.q_blocks, n);
    Y.visible = arena.template piece<uint8_t>(n);
    Y.reproj = arena.template piece<double>(n * 2);
    Y.x_right = arena.template piece<float>(n);
    Y.pred_level = arena.template piece<int32_t>(n);
    Y.q_xy = optional_piece<float>(arena, windows, n * 2);
    Y.q_margin = optional_piece<float>(arena, windows, n);
    Y.q_min_level = optional_piece<int32_t>(arena, windows, n);
    Y.q_max_level = optional_piece<int32_t>(arena, windows, n);
}

// The cell matcher: keypoint side, the caller's query side (`query(arena)`, one of the two above), grid, matcher state and -- with
// `lists` -- the candidate lists of capacity `cap`.  With a resident frame the keypoint arrays and the grid are the frame's own: those
// pieces stay empty (`occupied` is a host array either way).
struct CellPieces {
    Piece<uint8_t> tdesc, occupied;  // tdesc: nt x 32
    Piece<float> t_xy, t_angle, t_xright;
    Piece<int32_t> t_octave, cell_of, cell_off, cell_items, cand_off, match_q, num, cand_idx;
    Piece<int> owner, match;
    Piece<unsigned> mdist;
    Piece<uint32_t> dist;
};
template <class A, class Query>
void cell_layout(A& arena, size_t nq, size_t nt, size_t ncell, const void* occupied, const void* t_angle, const void* t_xright, bool resident, bool lists,
                 size_t cap, CellPieces& Y, Query&& query) {
    Y.tdesc = optional_piece<uint8_t>(arena, !resident, nt * 32);
    Y.t_xy = optional_piece<float>(arena, !resident, nt * 2);
    Y.t_octave = optional_piece<int32_t>(arena, !resident, nt);
    Y.occupied = optional_piece<uint8_t>(arena, occupied, nt);
    Y.t_angle = optional_piece<float>(arena, !resident && t_angle, nt);
    Y.t_xright = optional_piece<float>(arena, !resident && t_xright, nt);
    query(arena);
    Y.cell_of = optional_piece<int32_t>(arena, !resident, nt);
    Y.cell_off = optional_piece<int32_t>(arena, !resident, ncell + 1);
    Y.cell_items = optional_piece<int32_t>(arena, !resident, nt);
    Y.cand_off = arena.template piece<int32_t>(nq + 1);
    Y.match_q = arena.template piece<int32_t>(nq);
    Y.num = arena.template piece<int32_t>(1);
    Y.owner = arena.template piece<int>(nt);
    Y.match = arena.template piece<int>(nq);
    Y.mdist = arena.template piece<unsigned>(nt);
    Y.cand_idx = optional_piece<int32_t>(arena, lists, cap);  // the lists: last
    Y.dist = optional_piece<uint32_t>(arena, lists, cap);
}

// The bucket matcher: both sides' inputs, the (node, index) orders and rows, matcher state, the sort's scratch of `sortb` bytes and
// -- with `lists` -- the candidate lists of `total` entries.
struct BucketSide {
    const uint8_t* desc;
    const float* angle;
    const uint8_t* valid;
    const int32_t* node;     // nullable on both sides = one bucket
    const int32_t* octave;   // side 1, triangulation
    const double* bearings;  // triangulation
    const float* xright;     // nullable
    int n;
};
struct BucketPieces {
    Piece<uint8_t> desc1, desc2, valid1, valid2, occupied2, q_valid;  // desc: n x 32
    Piece<float> angle1, angle2, xright1, xright2, qangle_rows;
    Piece<int32_t> node1, node2, octave1, cand_off, match_rows, match, num, cand_idx;
    Piece<double> bearings1, bearings2;
    Piece<unsigned> key1, key2, mdist;
    Piece<int> q_idx, t_sorted, row_lo, row_hi, owner, match_of_row;
    Piece<uint32_t> qdesc_rows, dist;
    Piece<char> sort_scratch;
};
template <class A>
void bucket_layout(A& arena, const BucketSide& S1, const BucketSide& S2, const void* occupied2, size_t sortb, bool lists, size_t total, BucketPieces& Y) {
    const size_t n1 = (size_t)S1.n, n2 = (size_t)S2.n;
    Y.desc1 = arena.template piece<uint8_t>(n1 * 32);
    Y.desc2 = arena.template piece<uint8_t>(n2 * 32);
    Y.angle1 = optional_piece<float>(arena, S1.angle, n1);
    Y.angle2 = optional_piece<float>(arena, S2.angle, n2);
    Y.valid1 = optional_piece<uint8_t>(arena, S1.valid, n1);
    Y.valid2 = optional_piece<uint8_t>(arena, S2.valid, n2);
    Y.node1 = optional_piece<int32_t>(arena, S1.node, n1);
    Y.node2 = optional_piece<int32_t>(arena, S2.node, n2);
    Y.octave1 = optional_piece<int32_t>(arena, S1.octave, n1);
    Y.bearings1 = optional_piece<double>(arena, S1.bearings, n1 * 3);
    Y.bearings2 = optional_piece<double>(arena, S2.bearings, n2 * 3);
    Y.xright1 = optional_piece<float>(arena, S1.xright, n1);
    Y.xright2 = optional_piece<float>(arena, S2.xright, n2);
    Y.occupied2 = optional_piece<uint8_t>(arena, occupied2, n2);
    Y.key1 = arena.template piece<unsigned>(n1);
    Y.q_idx = arena.template piece<int>(n1);
    Y.key2 = arena.template piece<unsigned>(n2);
    Y.t_sorted = arena.template piece<int>(n2);
    Y.row_lo = arena.template piece<int>(n1);
    Y.row_hi = arena.template piece<int>(n1);
    Y.q_valid = arena.template piece<uint8_t>(n1);
    Y.cand_off = arena.template piece<int32_t>(n1 + 1);
    Y.qdesc_rows = arena.template piece<uint32_t>(n1 * 8);
    Y.qangle_rows = arena.template piece<float>(n1);
    Y.match_rows = arena.template piece<int32_t>(n1);
    Y.match = arena.template piece<int32_t>(n1);
    Y.num = arena.template piece<int32_t>(1);
    Y.owner = arena.template piece<int>(n2);
    Y.match_of_row = arena.template piece<int>(n1);
    Y.mdist = arena.template piece<unsigned>(n2);
    Y.sort_scratch = arena.template piece<char>(sortb);
    Y.cand_idx = optional_piece<int32_t>(arena, lists, total);  // the lists: last
    Y.dist = optional_piece<uint32_t>(arena, lists, total);
}
