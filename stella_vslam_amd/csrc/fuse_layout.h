// The scratch-arena layout of svgpu_fuse_landmarks_batch (svgpu_fuse.hip) and its two sizing rules.  The keyframes' arrays lie one after
// another in slot order (slot 0 = the current keyframe), the landmark table and the observation entries behind them, then the per-row
// state of ONE pass (the passes run one after another on the stream, so they share it), the results as one range, and -- with `lists` --
// the candidate lists of one pass, last: nothing in front of them depends on `lists` or on their capacity (the prefix invariant of
// match_layout.h), so the second pass of the call reuses what the first left in an arena that did not regrow.
// Plain C++ (no HIP): tests/fuse_arena_check.cpp compiles this header with sv_arena.h alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "sv_arena.h"

// ---- sizing rules
// Candidate lists.  The snapshot pass counts, per pass p, the candidates of its checked list under the table state on entry: total0[p].
// The lists of a pass are rebuilt on the state the passes before it left: a refreshed landmark may predict a coarser level (a wider
// window), and a landmark that was no query may become one.  The one arena all passes share holds
//     FUSE_CAND_FACTOR * max_p total0[p] + FUSE_CAND_SLACK
// entries; a pass whose lists outgrow it raises the overflow flag (SVGPU_FUSE_OVERFLOW), it is never written past its end.
constexpr size_t FUSE_CAND_FACTOR = 2;
constexpr size_t FUSE_CAND_SLACK = 1024;
inline size_t fuse_cand_capacity(const int32_t* total0, size_t passes) {
    size_t m = 0;
    for (size_t p = 0; p < passes; ++p) m = std::max(m, (size_t)std::max<int32_t>(total0[p], 0));
    return FUSE_CAND_FACTOR * m + FUSE_CAND_SLACK;
}
// Observation lists.  What the caller should reserve per landmark: a merge adds at most the loser's observations and every pass at most
// one connection, so `cnt + passes` covers the connections and FUSE_OBS_SLACK a merge with a typical loser; a list that still outgrows
// its capacity raises the overflow flag.
constexpr int32_t FUSE_OBS_SLACK = 8;
inline int32_t fuse_obs_capacity(int32_t cnt, int32_t passes) { return cnt + passes + FUSE_OBS_SLACK; }
// the longest observation list the refresh handles (the median's row buffer is walked, never stored: any length works; the bound keeps
// one lane's k x k descriptor walk short)
constexpr int32_t FUSE_OBS_CAP_MAX = 4096;

struct FuseShape {
    std::vector<int32_t> kf_n;        // keypoints per keyframe slot (K + 1)
    std::vector<uint8_t> kf_xright;   // slot has stereo x_right
    std::vector<int32_t> kf_cells;    // grid cells per slot
    size_t num_observers = 0, num_landmarks = 0, num_entries = 0, n_fwd = 0, n_bwd = 0;
    size_t kf_rec = 0, grid_rec = 0;  // bytes of one FuseKf / GridProblem record
};
struct FusePieces {
    // keyframes, concatenated in slot order
    Piece<uint8_t> desc;             // N x 32
    Piece<float> xy, xright;         // N x 2; xright: the stereo slots only
    Piece<int32_t> octave, kp_lm, cell_of, cell_off, cell_items;
    std::vector<size_t> first, first_xr, first_cell;  // per slot: first keypoint, first x_right (~0 = none), first cell counter
    Piece<char> kf_tab;              // K + 1 FuseKf records
    // observers
    Piece<int32_t> observer_rank, observer_kf;
    Piece<double> observer_twc;
    // landmark table
    Piece<double> pos_w, ref_twc, mean_normal;
    Piece<float> ref_sf, min_d, max_d;
    Piece<int32_t> obs_off, obs_cap, obs_cnt, replaced_by, obs_observer, obs_kp, obs_weight;
    Piece<uint8_t> alive, lm_desc, has_desc, has_geom, obs_desc;
    // checked lists and the state of one pass (rows = max(n_fwd, n_bwd))
    Piece<int32_t> fwd_list, bwd_list, q_min_level, q_max_level, cand_off, hit_lm, touch, total0, flag;
    Piece<uint8_t> visible;
    Piece<double> reproj;
    Piece<float> x_right, q_xy, q_margin;
    Piece<int> owner, match;
    // results: one range
    Piece<int32_t> best, num_fused;
    Piece<uint8_t> event;
    // the lists: last
    Piece<int32_t> cand_idx;
    Piece<uint32_t> dist;
};

template <class A>
void fuse_layout(A& arena, const FuseShape& S, bool lists, size_t cap, FusePieces& Y) {
    const size_t slots = S.kf_n.size(), K = slots ? slots - 1 : 0;
    size_t N = 0, NX = 0, NC = 0, nt_max = 0;
    Y.first.assign(slots, 0), Y.first_xr.assign(slots, ~size_t(0)), Y.first_cell.assign(slots, 0);
    for (size_t u = 0; u < slots; ++u) {
        Y.first[u] = N, Y.first_cell[u] = NC;
        if (S.kf_xright[u]) Y.first_xr[u] = NX, NX += (size_t)S.kf_n[u];
        N += (size_t)S.kf_n[u];
        NC += ((size_t)S.kf_cells[u] + 1 + 63) & ~size_t(63);  // (a slot's counters start 256-byte aligned, as a piece of their own would)
        nt_max = std::max(nt_max, (size_t)S.kf_n[u]);
    }
    const size_t L = S.num_landmarks, E = S.num_entries, O = S.num_observers, rows = std::max(S.n_fwd, S.n_bwd);
    Y.desc = arena.template piece<uint8_t>(N * 32);
    Y.xy = arena.template piece<float>(N * 2);
    Y.octave = arena.template piece<int32_t>(N);
    Y.xright = optional_piece<float>(arena, NX > 0, NX);
    Y.kp_lm = arena.template piece<int32_t>(N);
    Y.kf_tab = arena.template piece<char>(slots * S.kf_rec);
    Y.observer_rank = arena.template piece<int32_t>(O);
    Y.observer_kf = arena.template piece<int32_t>(O);
    Y.observer_twc = arena.template piece<double>(O * 3);
    Y.pos_w = arena.template piece<double>(L * 3);
    Y.ref_twc = arena.template piece<double>(L * 3);
    Y.ref_sf = arena.template piece<float>(L);
    Y.obs_off = arena.template piece<int32_t>(L);
    Y.obs_cap = arena.template piece<int32_t>(L);
    Y.alive = arena.template piece<uint8_t>(L);
    Y.lm_desc = arena.template piece<uint8_t>(L * 32);
    Y.mean_normal = arena.template piece<double>(L * 3);
    Y.min_d = arena.template piece<float>(L);
    Y.max_d = arena.template piece<float>(L);
    Y.has_desc = arena.template piece<uint8_t>(L);
    Y.has_geom = arena.template piece<uint8_t>(L);
    Y.obs_cnt = arena.template piece<int32_t>(L);
    Y.replaced_by = arena.template piece<int32_t>(L);
    Y.obs_observer = arena.template piece<int32_t>(E);
    Y.obs_kp = arena.template piece<int32_t>(E);
    Y.obs_desc = arena.template piece<uint8_t>(E * 32);
    Y.obs_weight = arena.template piece<int32_t>(E);
    Y.fwd_list = arena.template piece<int32_t>(S.n_fwd);
    Y.bwd_list = arena.template piece<int32_t>(S.n_bwd);
    Y.cell_of = arena.template piece<int32_t>(N);
    Y.cell_off = arena.template piece<int32_t>(NC);
    Y.cell_items = arena.template piece<int32_t>(N);
    Y.visible = arena.template piece<uint8_t>(rows);
    Y.reproj = arena.template piece<double>(rows * 2);
    Y.x_right = arena.template piece<float>(rows);
    Y.q_xy = arena.template piece<float>(rows * 2);
    Y.q_margin = arena.template piece<float>(rows);
    Y.q_min_level = arena.template piece<int32_t>(rows);
    Y.q_max_level = arena.template piece<int32_t>(rows);
    Y.cand_off = arena.template piece<int32_t>(rows + 1);
    Y.hit_lm = arena.template piece<int32_t>(rows);
    Y.owner = arena.template piece<int>(nt_max);
    Y.match = arena.template piece<int>(rows);
    Y.touch = arena.template piece<int32_t>(L);
    Y.total0 = arena.template piece<int32_t>(K + 1);
    Y.flag = arena.template piece<int32_t>(1);
    Y.best = arena.template piece<int32_t>(K * S.n_fwd + S.n_bwd);
    Y.event = arena.template piece<uint8_t>(K * S.n_fwd + S.n_bwd);
    Y.num_fused = arena.template piece<int32_t>(K + 1);
    Y.cand_idx = optional_piece<int32_t>(arena, lists, cap);  // the lists: last
    Y.dist = optional_piece<uint32_t>(arena, lists, cap);
}
