// The scratch-arena layout of svgpu_reloc_refine_batch (svgpu_reloc.hip), as a function of an arena: run on a measuring arena it gives the
// bytes the call asks for, run on the placing arena it hands out the pieces.  It places and does nothing else.  Plain C++ (no HIP):
// tests/reloc_refine_arena_check.cpp compiles this header with sv_arena.h alone.
//
// The candidate lists are the LAST takes and nothing in front of them depends on their capacity: a call that has to repeat itself with
// longer lists finds every other piece where it was.
#pragma once
#include <cstddef>
#include <cstdint>

#include "sv_arena.h"

struct RelocRefineShape {
    size_t K = 0;       // candidates
    size_t nt = 0;      // keypoints of the frame (shared)
    size_t N = 0;       // keyframe entries of all candidates (kf_off[K])
    size_t S = 0;       // stages
    size_t ncell = 0;   // grid cells
    bool has_angle = false, has_xright = false, has_kf_angle = false;
    bool global_replay = false;  // some candidate's replay keeps its tables in global memory (sv_cand_replay_form < 0)
    size_t cand_rec = 0, replay_rec = 0;  // sizeof(CandProblem), sizeof(CandBatchReplay)
    size_t cap = 0;     // capacity of the candidate lists, entries
};

struct RelocRefinePieces {
    // ---- uploaded: the frame, once for all candidates
    Piece<uint8_t> tdesc;     // nt x 32
    Piece<float> t_xy;        // nt x 2
    Piece<int32_t> t_octave;  // nt
    Piece<float> t_angle, t_xright;  // nt, optional
    // ---- uploaded: per candidate
    Piece<double> pose_in;    // K x 12
    Piece<uint8_t> active;    // K (cleared by the count decision)
    Piece<int32_t> count0;    // K: n_already_found
    Piece<uint8_t> occupied;  // K x nt: keypoint holds a landmark (grows with the matches)
    Piece<double> lm_pos;     // K x nt x 3: its position
    Piece<int32_t> kf_off;    // K + 1 (also the row base of the batched candidate matcher)
    Piece<int32_t> obs_off;   // K + 1: p * nt, the entry slices of the pose optimiser
    // ---- uploaded: per keyframe entry
    Piece<double> pos_w;      // N x 3
    Piece<uint8_t> valid;     // N (cleared by a match)
    Piece<float> min_d, max_d, kf_angle;  // N (kf_angle optional)
    Piece<uint8_t> lm_desc;   // N x 32
    // ---- uploaded: the problem tables of the candidate matcher (S x K records, K records)
    Piece<char> cand_tab, replay_tab;
    // ---- device only: observation arrays of the pose optimiser, one entry per (candidate, keypoint), and its compacted copies and scratch
    Piece<float> uvr, w, huber;           // K x nt (x 3)
    Piece<double> c_pos;
    Piece<float> c_uvr, c_w, c_huber;
    Piece<int32_t> entry_of;
    Piece<uint8_t> level, robust, outlier;
    // ---- device only: the stage's reprojection windows and matcher state
    Piece<uint8_t> visible;               // N
    Piece<float> q_xy, q_margin;          // N x 2, N
    Piece<int32_t> q_min_level, q_max_level;
    Piece<int32_t> cell_of, cell_off, cell_items;  // nt, ncell + 1, nt
    Piece<int32_t> cand_off;              // N + 1
    Piece<int32_t> match_q;               // N: the stage's matches
    Piece<int> owner, match_of_row;       // K x nt, N: only with global_replay
    // ---- results, next to one another: one copy brings them back
    Piece<int32_t> status;                // K
    Piece<double> pose_stage;             // S x K x 12: row s is what the optimisation of stage s leaves (its input where it did not run)
    Piece<int32_t> match_kf, match_stage; // N, start at -1
    Piece<int32_t> num_found;             // K x S
    Piece<int32_t> result;                // S x K x 4: num_valid, LM iterations, num_bad, selected entries
    Piece<uint8_t> flags;                 // S x K x nt
    // ---- the candidate lists: last
    Piece<int32_t> cand_idx;
    Piece<uint32_t> dist;
};

// The layout in two halves, so that a call that runs something in front of the stages (svgpu_reloc_solve_batch, reloc_solve_layout.h) can
// put its own results right in front of these: `front` is everything up to the matcher state, `back` the results and the lists.
template <class A>
void reloc_refine_layout_front(A& arena, const RelocRefineShape& H, RelocRefinePieces& Y) {
    const size_t K = H.K, nt = H.nt, N = H.N, S = H.S, E = K * nt;
    Y.tdesc = arena.template piece<uint8_t>(nt * 32);
    Y.t_xy = arena.template piece<float>(nt * 2);
    Y.t_octave = arena.template piece<int32_t>(nt);
    Y.t_angle = optional_piece<float>(arena, H.has_angle, nt);
    Y.t_xright = optional_piece<float>(arena, H.has_xright, nt);
    Y.pose_in = arena.template piece<double>(K * 12);
    Y.active = arena.template piece<uint8_t>(K);
    Y.count0 = arena.template piece<int32_t>(K);
    Y.occupied = arena.template piece<uint8_t>(E);
    Y.lm_pos = arena.template piece<double>(E * 3);
    Y.kf_off = arena.template piece<int32_t>(K + 1);
    Y.obs_off = arena.template piece<int32_t>(K + 1);
    Y.pos_w = arena.template piece<double>(N * 3);
    Y.valid = arena.template piece<uint8_t>(N);
    Y.min_d = arena.template piece<float>(N);
    Y.max_d = arena.template piece<float>(N);
    Y.kf_angle = optional_piece<float>(arena, H.has_kf_angle, N);
    Y.lm_desc = arena.template piece<uint8_t>(N * 32);
    Y.cand_tab = arena.template piece<char>(S * K * H.cand_rec);
    Y.replay_tab = arena.template piece<char>(K * H.replay_rec);
    Y.uvr = arena.template piece<float>(E * 3);
    Y.w = arena.template piece<float>(E);
    Y.huber = arena.template piece<float>(E);
    Y.c_pos = arena.template piece<double>(E * 3);
    Y.c_uvr = arena.template piece<float>(E * 3);
    Y.c_w = arena.template piece<float>(E);
    Y.c_huber = arena.template piece<float>(E);
    Y.entry_of = arena.template piece<int32_t>(E);
    Y.level = arena.template piece<uint8_t>(E);
    Y.robust = arena.template piece<uint8_t>(E);
    Y.outlier = arena.template piece<uint8_t>(E);
    Y.visible = arena.template piece<uint8_t>(N);
    Y.q_xy = arena.template piece<float>(N * 2);
    Y.q_margin = arena.template piece<float>(N);
    Y.q_min_level = arena.template piece<int32_t>(N);
    Y.q_max_level = arena.template piece<int32_t>(N);
    Y.cell_of = arena.template piece<int32_t>(nt);
    Y.cell_off = arena.template piece<int32_t>(H.ncell + 1);
    Y.cell_items = arena.template piece<int32_t>(nt);
    Y.cand_off = arena.template piece<int32_t>(N + 1);
    Y.match_q = arena.template piece<int32_t>(N);
    Y.owner = optional_piece<int>(arena, H.global_replay, E);
    Y.match_of_row = optional_piece<int>(arena, H.global_replay, N);
}

template <class A>
void reloc_refine_layout_back(A& arena, const RelocRefineShape& H, RelocRefinePieces& Y) {
    const size_t K = H.K, nt = H.nt, N = H.N, S = H.S, E = K * nt;
    Y.status = arena.template piece<int32_t>(K);
    Y.pose_stage = arena.template piece<double>(S * K * 12);
    Y.match_kf = arena.template piece<int32_t>(N);
    Y.match_stage = arena.template piece<int32_t>(N);
    Y.num_found = arena.template piece<int32_t>(K * S);
    Y.result = arena.template piece<int32_t>(S * K * 4);
    Y.flags = arena.template piece<uint8_t>(S * E);
    Y.cand_idx = arena.template piece<int32_t>(H.cap);  // the lists: last
    Y.dist = arena.template piece<uint32_t>(H.cap);
}

template <class A>
void reloc_refine_layout(A& arena, const RelocRefineShape& H, RelocRefinePieces& Y) {
    reloc_refine_layout_front(arena, H, Y);
    reloc_refine_layout_back(arena, H, Y);
}
