// The scratch-arena layout of svgpu_loop_sim3_batch (svgpu_loop.hip), as a function of an arena: run on a measuring arena it gives the
// bytes the call asks for, run on the placing arena it hands out the pieces.  It places and does nothing else.  Plain C++ (no HIP):
// tests/loop_sim3_arena_check.cpp compiles this header with sv_arena.h alone.
//
// Rows: the queries of both matcher passes are ONE concatenation, K x n1 rows of pass A (keyframe 1's landmarks under candidate p's
// transform) followed by the N2 rows of pass B (every candidate's landmarks into keyframe 1).  Keypoint sets: the K candidates' keypoints
// followed by keyframe 1's, binned in one pass over ONE array of (K + 1) x cells counters (sv_launch_grid_sets).
// The candidate lists are the LAST takes and nothing in front of them depends on their capacity: a call that has to repeat itself with
// longer lists finds every other piece where it was.
#pragma once
#include <cstddef>
#include <cstdint>

#include "sv_arena.h"

struct LoopSim3Shape {
    size_t K = 0;      // candidates
    size_t n1 = 0;     // keypoints of keyframe 1 (shared)
    size_t N2 = 0;     // keypoints of all candidates (kf2_off[K])
    size_t ncell = 0;  // grid cells of one keyframe
    bool has_scale_in = false;
    size_t owner_ints = 0, mrow_ints = 0;  // tables of the candidates whose replay keeps them in global memory (sv_cand_replay_form < 0), else 0
    size_t prob_rec = 0, reproj_rec = 0, cand_rec = 0, replay_rec = 0, grid_rec = 0, stats_rec = 0;  // sizeof of the records the tables hold
    size_t cap = 0;    // capacity of the candidate lists, entries
};

struct LoopSim3Pieces {
    // ---- uploaded: keyframe 1, once for all candidates
    Piece<uint8_t> desc1, lm_desc1;        // n1 x 32
    Piece<float> xy1;                      // n1 x 2
    Piece<int32_t> octave1;                // n1
    Piece<double> pos_w1;                  // n1 x 3
    Piece<uint8_t> has_lm1;                // n1
    Piece<float> min1, max1;               // n1
    // ---- uploaded: the candidates' keyframes, concatenated by kf2_off
    Piece<uint8_t> desc2, lm_desc2;        // N2 x 32
    Piece<float> xy2;
    Piece<int32_t> octave2;
    Piece<double> pos_w2;
    Piece<uint8_t> has_lm2;
    Piece<float> min2, max2;
    // ---- uploaded: per candidate
    Piece<int32_t> kf2_off;                // K + 1
    Piece<int32_t> set_base;               // K + 2: the keypoint sets of the binning (the candidates, then keyframe 1)
    Piece<int32_t> row_base;               // 2K + 1: the rows of the 2K matcher problems
    Piece<double> pose_in_cand, pose_2w;   // K x 12
    Piece<double> rot_12, trans_12;        // K x 9, K x 3
    Piece<uint8_t> active;                 // K
    Piece<float> scale_in;                 // K, optional
    Piece<char> prob;                      // K Sim3OptProblem: views and Sim3 from the host, scale and match range from the device
    Piece<char> reproj_tab;                // K ReprojProblem (camera 2, modes, margin)
    Piece<char> grid_tab;                  // 3K + 1 GridProblem: the K + 1 keypoint sets, then the rows of the 2K matcher problems
    Piece<char> cand_tab, replay_tab;      // 2K CandProblem / CandBatchReplay
    // ---- uploaded: the prior matches, K x n1
    Piece<uint8_t> prior_state;
    Piece<int32_t> prior_idx2;
    Piece<double> prior_pos_w;             // x 3
    // ---- device only
    Piece<uint32_t> ratio_bits;            // K x n1: the kept ratios as bit patterns
    Piece<double> xf;                      // K x 24: [s_rot_21w | trans_21w | s_rot_12w | trans_12w]
    Piece<uint8_t> live;                   // K: 1 = the candidate takes part in the later kernels
    Piece<uint8_t> already2;               // N2: is_already_matched_in_keyfrm_2
    Piece<int32_t> cell_cnt;               // (K + 1) x ncell + 1: counters, then offsets (scanned in place)
    Piece<int32_t> cell_of, cell_items;    // N2 + n1
    Piece<uint8_t> visible;                // rows
    Piece<float> q_xy, q_margin;           // rows x 2, rows
    Piece<int32_t> q_min_level, q_max_level;
    Piece<int32_t> cand_off;               // rows + 1
    Piece<int> owner, match_of_row;        // only with a global-memory replay
    Piece<int32_t> num_ab;                 // 2K: matches per matcher problem
    Piece<double> obs1, obs2;              // K x n1 x 2: the edges, candidate p's from p x n1 on
    Piece<float> w1, w2;                   // K x n1
    Piece<double> pos1, pos2;              // K x n1 x 3
    Piece<double> chi_cache;               // K x n1 x 2
    // ---- results, next to one another
    Piece<float> scale;                    // K
    Piece<int32_t> code;                   // K: -1 inactive, 1 no scale, 0 ran
    Piece<int32_t> match_a;                // K x n1: matched_2_in_1
    Piece<int32_t> match_b;                // N2: matched_1_in_2
    Piece<int32_t> mutual;                 // K x n1
    Piece<int32_t> num_mutual, num_edges;  // K
    Piece<int32_t> edge_idx1, edge_idx2;   // K x n1
    Piece<uint8_t> edge_status;            // K x n1
    Piece<double> sim3_out;                // K x 8
    Piece<int32_t> num_inliers;            // K
    Piece<char> stats;                     // K svgpu_sim3opt_stats
    // ---- the candidate lists: last
    Piece<int32_t> cand_idx;
    Piece<uint32_t> dist;
};

template <class A>
void loop_sim3_layout(A& arena, const LoopSim3Shape& H, LoopSim3Pieces& Y) {
    const size_t K = H.K, n1 = H.n1, N2 = H.N2, E = K * n1, R = E + N2, T = N2 + n1;
    Y.desc1 = arena.template piece<uint8_t>(n1 * 32);
    Y.lm_desc1 = arena.template piece<uint8_t>(n1 * 32);
    Y.xy1 = arena.template piece<float>(n1 * 2);
    Y.octave1 = arena.template piece<int32_t>(n1);
    Y.pos_w1 = arena.template piece<double>(n1 * 3);
    Y.has_lm1 = arena.template piece<uint8_t>(n1);
    Y.min1 = arena.template piece<float>(n1);
    Y.max1 = arena.template piece<float>(n1);
    Y.desc2 = arena.template piece<uint8_t>(N2 * 32);
    Y.lm_desc2 = arena.template piece<uint8_t>(N2 * 32);
    Y.xy2 = arena.template piece<float>(N2 * 2);
    Y.octave2 = arena.template piece<int32_t>(N2);
    Y.pos_w2 = arena.template piece<double>(N2 * 3);
    Y.has_lm2 = arena.template piece<uint8_t>(N2);
    Y.min2 = arena.template piece<float>(N2);
    Y.max2 = arena.template piece<float>(N2);
    Y.kf2_off = arena.template piece<int32_t>(K + 1);
    Y.set_base = arena.template piece<int32_t>(K + 2);
    Y.row_base = arena.template piece<int32_t>(2 * K + 1);
    Y.pose_in_cand = arena.template piece<double>(K * 12);
    Y.pose_2w = arena.template piece<double>(K * 12);
    Y.rot_12 = arena.template piece<double>(K * 9);
    Y.trans_12 = arena.template piece<double>(K * 3);
    Y.active = arena.template piece<uint8_t>(K);
    Y.scale_in = optional_piece<float>(arena, H.has_scale_in, K);
    Y.prob = arena.template piece<char>(K * H.prob_rec);
    Y.reproj_tab = arena.template piece<char>(K * H.reproj_rec);
    Y.grid_tab = arena.template piece<char>((3 * K + 1) * H.grid_rec);
    Y.cand_tab = arena.template piece<char>(2 * K * H.cand_rec);
    Y.replay_tab = arena.template piece<char>(2 * K * H.replay_rec);
    Y.prior_state = arena.template piece<uint8_t>(E);
    Y.prior_idx2 = arena.template piece<int32_t>(E);
    Y.prior_pos_w = arena.template piece<double>(E * 3);
    Y.ratio_bits = arena.template piece<uint32_t>(E);
    Y.xf = arena.template piece<double>(K * 24);
    Y.live = arena.template piece<uint8_t>(K);
    Y.already2 = arena.template piece<uint8_t>(N2);
    Y.cell_cnt = arena.template piece<int32_t>((K + 1) * H.ncell + 1);
    Y.cell_of = arena.template piece<int32_t>(T);
    Y.cell_items = arena.template piece<int32_t>(T);
    Y.visible = arena.template piece<uint8_t>(R);
    Y.q_xy = arena.template piece<float>(R * 2);
    Y.q_margin = arena.template piece<float>(R);
    Y.q_min_level = arena.template piece<int32_t>(R);
    Y.q_max_level = arena.template piece<int32_t>(R);
    Y.cand_off = arena.template piece<int32_t>(R + 1);
    Y.owner = optional_piece<int>(arena, H.owner_ints > 0, H.owner_ints);
    Y.match_of_row = optional_piece<int>(arena, H.mrow_ints > 0, H.mrow_ints);
    Y.num_ab = arena.template piece<int32_t>(2 * K);
    Y.obs1 = arena.template piece<double>(E * 2);
    Y.obs2 = arena.template piece<double>(E * 2);
    Y.w1 = arena.template piece<float>(E);
    Y.w2 = arena.template piece<float>(E);
    Y.pos1 = arena.template piece<double>(E * 3);
    Y.pos2 = arena.template piece<double>(E * 3);
    Y.chi_cache = arena.template piece<double>(E * 2);
    Y.scale = arena.template piece<float>(K);
    Y.code = arena.template piece<int32_t>(K);
    Y.match_a = arena.template piece<int32_t>(E);
    Y.match_b = arena.template piece<int32_t>(N2);
    Y.mutual = arena.template piece<int32_t>(E);
    Y.num_mutual = arena.template piece<int32_t>(K);
    Y.num_edges = arena.template piece<int32_t>(K);
    Y.edge_idx1 = arena.template piece<int32_t>(E);
    Y.edge_idx2 = arena.template piece<int32_t>(E);
    Y.edge_status = arena.template piece<uint8_t>(E);
    Y.sim3_out = arena.template piece<double>(K * 8);
    Y.num_inliers = arena.template piece<int32_t>(K);
    Y.stats = arena.template piece<char>(K * H.stats_rec);
    Y.cand_idx = arena.template piece<int32_t>(H.cap);  // the lists: last
    Y.dist = arena.template piece<uint32_t>(H.cap);
}
