// The one device allocation of a resident frame (svgpu_frame.hip), as functions of an arena.  Its head is the observation the host wants
// back of a freshly extracted frame, so that one contiguous copy fetches it (svgpu_track_motion); the same function lays that head out over
// the page-locked copy.  Plain C++ (no HIP): tests/track_arena_check.cpp compiles this header with sv_arena.h, orb_plan.h and svgpu.h alone.
#pragma once
#include <cstddef>
#include <cstdint>

#include "svgpu.h"
#include "orb_plan.h"  // SV_MAX_LEVELS
#include "sv_arena.h"

// data::frame_observation as the fused extraction leaves it
struct FrameObs {
    Piece<svgpu_keypoint> kps_raw;  // distorted keypoints as the extractor wrote them (fused extraction only)
    Piece<uint8_t> desc;            // x 32
    Piece<svgpu_keypoint> undist;   // undistorted keypoint records
    Piece<double> bearings;         // x 3
    Piece<float> xright;            // stereo_x_right_ (valid when has_xright); these two with `stereo` only, else empty
    Piece<float> depth;             // depths_ (written by the fused stereo / RGB-D chain only)
};
template <class A>
void frame_obs_layout(A& arena, size_t cap, bool stereo, FrameObs& Y) {
    Y.kps_raw = arena.template piece<svgpu_keypoint>(cap);
    Y.desc = arena.template piece<uint8_t>(cap * 32);
    Y.undist = arena.template piece<svgpu_keypoint>(cap);
    Y.bearings = arena.template piece<double>(cap * 3);
    Y.xright = stereo ? arena.template piece<float>(cap) : Piece<float>{};
    Y.depth = stereo ? arena.template piece<float>(cap) : Piece<float>{};
}
// what one copy from the first piece on has to carry: through the elements of the last piece taken, without its padding
inline size_t frame_obs_bytes(const FrameObs& o) {
    const size_t head = pad(o.kps_raw.bytes()) + pad(o.desc.bytes()) + pad(o.undist.bytes());
    return o.depth.n ? head + pad(o.bearings.bytes()) + pad(o.xright.bytes()) + o.depth.bytes() : head + o.bearings.bytes();
}

// the slab: the observation first (always with the stereo pieces), then what the matchers read beside it
struct FrameSlab : FrameObs {
    Piece<float> xy;  // x 2
    Piece<int32_t> octave;
    Piece<float> angle;
    Piece<int32_t> cell_of, cell_items;
    Piece<int32_t> counts;  // 1 + SV_MAX_LEVELS: the extractor's counts (fused extraction: [0] = n as the device knows it)
};
template <class A>
void frame_slab_layout(A& arena, size_t cap, FrameSlab& Y) {
    frame_obs_layout(arena, cap, true, Y);
    Y.xy = arena.template piece<float>(cap * 2);
    Y.octave = arena.template piece<int32_t>(cap);
    Y.angle = arena.template piece<float>(cap);
    Y.cell_of = arena.template piece<int32_t>(cap);
    Y.cell_items = arena.template piece<int32_t>(cap);
    Y.counts = arena.template piece<int32_t>(1 + SV_MAX_LEVELS);
}
