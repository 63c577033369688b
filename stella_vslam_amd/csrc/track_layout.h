// The persistent buffers of the tracked-frame chain (svgpu_track.hip), as functions of an arena: the capacities with their growth policy,
// the input block (the same layout over the device block and its page-locked image, so one copy carries a range of it), what the kernels
// hand to each other, and the page-locked results.  Plain C++ (no HIP): tests/track_arena_check.cpp compiles this header with sv_arena.h alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "sv_arena.h"

struct TrackCaps {
    int kp = 0;            // keypoints of the current frame
    int q = 0;             // queries (last frame's keypoints / local landmarks)
    size_t cand = 0;       // candidate-list entries BEHIND the per-query slots (lists longer than a slot)
    size_t img_bytes = 0;  // image part of the input block
    size_t obs_bytes = 0;  // read-back of a fresh observation
    bool operator==(const TrackCaps& o) const { return kp == o.kp && q == o.q && cand == o.cand && img_bytes == o.img_bytes && obs_bytes == o.obs_bytes; }
    bool operator!=(const TrackCaps& o) const { return !(*this == o); }
};
// The capacities to hold after a call that wants `want`, holding `have`: grow-only; when anything has to grow the queries get a quarter
// of headroom; floors of 64 keypoints, 64 queries and 65 536 list entries.  Nothing to grow gives `have` back (with the floors: the
// very first call), so a call of the same shape never re-allocates.
inline TrackCaps track_caps(const TrackCaps& have, const TrackCaps& want) {
    TrackCaps c = have;
    if (want.kp > have.kp || want.q > have.q || want.cand > have.cand || want.img_bytes > have.img_bytes || want.obs_bytes > have.obs_bytes) {
        c.kp = std::max(want.kp, have.kp), c.q = std::max(want.q + want.q / 4, have.q), c.cand = std::max(want.cand, have.cand);
        c.img_bytes = std::max(want.img_bytes, have.img_bytes), c.obs_bytes = std::max(want.obs_bytes, have.obs_bytes);
    }
    c.kp = std::max(c.kp, 64), c.q = std::max(c.q, 64), c.cand = std::max(c.cand, (size_t)65536);
    return c;
}

// Input block: [image] | landmark ids.  The two halves of a frame share the id piece:
//   motion      ids[0, n_last)                                the last frame's landmark ids
//   local map   ids[0, nt) and ids[loc_at, loc_at + n_local)  the frame's landmark ids, the local landmarks' ids
// loc_at is the first 256-byte boundary at or behind caps.kp ids, so both lists of the second half are aligned like pieces of their own.
struct TrackIn {
    Piece<char> image;
    Piece<int32_t> ids;
    size_t loc_at = 0;
};
template <class A>
void track_in_layout(A& arena, const TrackCaps& c, TrackIn& Y) {
    Y.image = arena.template piece<char>(c.img_bytes);
    Y.loc_at = pad((size_t)c.kp * 4) / 4;
    Y.ids = arena.template piece<int32_t>(Y.loc_at + (size_t)c.q);
}

// everything the kernels hand to each other (`slot`: the entries of a query's own list slot, TRACK_SLOT of track_kernels.h)
struct TrackWork {
    Piece<int32_t> cand_off, cand_cnt, match_q;
    Piece<int32_t> num;  // [0] matches, [2] the list allocation counter
    Piece<int32_t> who, kp_of, pred_level;
    Piece<uint32_t> dist;
    Piece<uint8_t> q_valid, q_blocks, occupied, visible, outlier_kp, po_outlier, po_level, po_robust;
    Piece<double> reproj, po_pos;
    Piece<float> x_right, po_uvr, po_w, po_h;
    Piece<int> po_result;
    Piece<int32_t> cur_lm_motion;  // the motion half's landmark ids per keypoint (the local-map half's come with its input block)
    Piece<double> pose;            // 12: the pose of the last optimisation
    Piece<int> g_owner, g_match;   // tables of the replay's global-memory form (inputs beyond its LDS form)
};
template <class A>
void track_work_layout(A& arena, const TrackCaps& c, size_t slot, TrackWork& Y) {
    const size_t kp = c.kp, q = c.q;
    Y.cand_off = arena.template piece<int32_t>(q + 1);
    Y.cand_cnt = arena.template piece<int32_t>(q);
    Y.match_q = arena.template piece<int32_t>(q);
    Y.num = arena.template piece<int32_t>(4);
    Y.who = arena.template piece<int32_t>(kp);
    Y.kp_of = arena.template piece<int32_t>(kp);
    Y.pred_level = arena.template piece<int32_t>(q);
    Y.dist = arena.template piece<uint32_t>(q * slot + c.cand);
    Y.q_valid = arena.template piece<uint8_t>(q);
    Y.q_blocks = arena.template piece<uint8_t>(q);
    Y.occupied = arena.template piece<uint8_t>(kp);
    Y.visible = arena.template piece<uint8_t>(q);
    Y.outlier_kp = arena.template piece<uint8_t>(kp);
    Y.po_outlier = arena.template piece<uint8_t>(kp);
    Y.po_level = arena.template piece<uint8_t>(kp);
    Y.po_robust = arena.template piece<uint8_t>(kp);
    Y.reproj = arena.template piece<double>(q * 2);
    Y.po_pos = arena.template piece<double>(kp * 3);
    Y.x_right = arena.template piece<float>(q);
    Y.po_uvr = arena.template piece<float>(kp * 3);
    Y.po_w = arena.template piece<float>(kp);
    Y.po_h = arena.template piece<float>(kp);
    Y.po_result = arena.template piece<int>(4);
    Y.cur_lm_motion = arena.template piece<int32_t>(kp);
    Y.pose = arena.template piece<double>(12);
    Y.g_owner = arena.template piece<int>(kp);
    Y.g_match = arena.template piece<int>(q);
}

// page-locked results: what the kernels write straight to the host, and the read-back of a fresh observation
struct TrackOut {
    Piece<unsigned long long> h_stamps;  // debug (SVGPU_TRACK_STAMPS): phase stamps of the last k_pose_opt
    Piece<int32_t> h_n, h_num;
    Piece<int> h_result;
    Piece<double> h_pose;
    Piece<uint8_t> h_outlier;
    Piece<int32_t> h_match;
    Piece<uint8_t> h_visible;
    Piece<char> h_obs;  // frame_obs_layout (frame_layout.h) is placed over it; like every piece it owns its padding
};
template <class A>
void track_out_layout(A& arena, const TrackCaps& c, TrackOut& Y) {
    Y.h_stamps = arena.template piece<unsigned long long>(64);
    Y.h_n = arena.template piece<int32_t>(4);
    Y.h_num = arena.template piece<int32_t>(4);
    Y.h_result = arena.template piece<int>(4);
    Y.h_pose = arena.template piece<double>(12);
    Y.h_outlier = arena.template piece<uint8_t>(c.kp);
    Y.h_match = arena.template piece<int32_t>(c.q);
    Y.h_visible = arena.template piece<uint8_t>(c.q);
    Y.h_obs = arena.template piece<char>(c.obs_bytes);
}
