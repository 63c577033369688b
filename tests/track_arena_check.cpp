// Host-only check of the tracked-frame chain's persistent buffers (stella_vslam_amd/csrc/track_layout.h) and of the resident frame's slab
// (frame_layout.h), built and run by tests/test_arena_layouts.py: the checks of tests/layout_check.h for the input block, the work block,
// the page-locked results and the slab; what the tracker relies on inside the input block and between the slab and its read-back; and the
// growth policy track_caps.
#include <cstdint>
#include <string>

#include "frame_layout.h"
#include "track_layout.h"
#include "layout_check.h"

static const size_t SLOT = 64;  // TRACK_SLOT of track_kernels.h

static size_t at(const void* p, const char* base) { return (size_t)((const char*)p - base); }

// the observation's bytes as the tracker used to write them out, from the slab's own pointers ...
static size_t old_obs_bytes(const FrameSlab& f, const char* slab, size_t cap, bool stereo) {
    return stereo ? at(f.depth.p, slab) + cap * 4 : at(f.bearings.p, slab) + cap * 24;
}
// ... and by hand
static size_t hand_obs_bytes(size_t cap, bool stereo) {
    const size_t head = pad(28 * cap) + pad(32 * cap) + pad(28 * cap);
    return stereo ? head + pad(24 * cap) + pad(4 * cap) + 4 * cap : head + 24 * cap;
}

static void check_slab(size_t cap) {
    const std::string name = "slab cap " + std::to_string(cap);
    layout_check<FrameSlab>(name.c_str(), [&](Arena& A, FrameSlab& Y) { frame_slab_layout(A, cap, Y); },
        [&](const FrameSlab& Y) {
            return Rows{{Y.kps_raw, 28 * cap}, {Y.desc, 32 * cap}, {Y.undist, 28 * cap}, {Y.bearings, 24 * cap}, {Y.xright, 4 * cap}, {Y.depth, 4 * cap},
                        {Y.xy, 8 * cap}, {Y.octave, 4 * cap}, {Y.angle, 4 * cap}, {Y.cell_of, 4 * cap}, {Y.cell_items, 4 * cap}, {Y.counts, 68}};
        },
        [&](const FrameSlab& Y, const char* base, size_t need) {
            CHECK((const char*)Y.kps_raw.p == base);  // the read-back starts at the first piece
            CHECK(need == 2 * pad(28 * cap) + pad(32 * cap) + pad(24 * cap) + pad(8 * cap) + 6 * pad(4 * cap) + pad(68));  // the twelve takes of before
            for (const bool stereo : {false, true}) {
                // the observation over a buffer of its own = the first four (mono) or six (stereo) pieces of the slab, offset for offset
                FrameObs O;
                Arena A(const_cast<char*>(base), need);
                frame_obs_layout(A, cap, stereo, O);
                CHECK(!A.overflow);
                CHECK(O.kps_raw.p == Y.kps_raw.p && O.desc.p == Y.desc.p && O.undist.p == Y.undist.p && O.bearings.p == Y.bearings.p);
                CHECK(O.kps_raw.n == cap && O.desc.n == 32 * cap && O.undist.n == cap && O.bearings.n == 3 * cap);
                if (stereo) CHECK(O.xright.p == Y.xright.p && O.depth.p == Y.depth.p && O.xright.n == cap && O.depth.n == cap);
                else CHECK(O.xright.p == nullptr && O.xright.n == 0 && O.depth.p == nullptr && O.depth.n == 0);
                CHECK(frame_obs_bytes(O) == old_obs_bytes(Y, base, cap, stereo) && frame_obs_bytes(O) == hand_obs_bytes(cap, stereo));
                FrameObs M;  // (the tracker asks a measured layout: counts alone)
                Arena measure;
                frame_obs_layout(measure, cap, stereo, M);
                CHECK(frame_obs_bytes(M) == frame_obs_bytes(O) && pad(frame_obs_bytes(M)) == measure.off);
                // ... and placed over exactly the bytes of the read-back, padded as the results' piece pads them
                Arena tight(const_cast<char*>(base), pad(frame_obs_bytes(M)));
                FrameObs T;
                frame_obs_layout(tight, cap, stereo, T);
                CHECK(!tight.overflow && T.bearings.p == Y.bearings.p);
            }
        });
}

static void check_tracker(const char* what, const TrackCaps& c, size_t frame_cap = 0, bool stereo = false) {
    const size_t kp = c.kp, q = c.q, cand = c.cand, ib = c.img_bytes, ob = c.obs_bytes;
    char name[160];
    std::snprintf(name, sizeof name, "%s: kp %zu q %zu cand %zu image %zu obs %zu", what, kp, q, cand, ib, ob);
    CHECK(track_caps(c, c) == c);  // a call of the shape the buffers hold does not re-allocate

    layout_check<TrackIn>((std::string("in, ") + name).c_str(), [&](Arena& A, TrackIn& Y) { track_in_layout(A, c, Y); },
        [&](const TrackIn& Y) { return Rows{{Y.image, ib}, {Y.ids, pad(4 * kp) + 4 * q}}; },
        [&](const TrackIn& Y, const char* base, size_t need) {
            CHECK(need == pad(ib) + pad(4 * kp) + pad(4 * q));  // (what was summed by hand, less its 256 spare bytes)
            CHECK(Y.image.p == base && at(Y.ids.p, base) == pad(ib));  // adjacent up to padding: one copy carries the image and the ids behind it
            CHECK(Y.loc_at * 4 % 256 == 0 && Y.loc_at * 4 >= kp * 4 && Y.loc_at * 4 == pad(4 * kp));
            CHECK(at(Y.ids.p + Y.loc_at, base) == pad(ib) + pad(4 * kp));  // the two offsets the call sites used to recompute
            CHECK(Y.ids.n >= Y.loc_at + q);  // local map: the frame's ids in front of loc_at, q local ids behind it
            CHECK(Y.ids.n >= q);             // motion: up to q ids of the last frame from the start of the piece
        });
    {  // the device block and its page-locked image are the same function of the same capacities
        TrackIn D, H;
        const size_t need = arena_measure([&](Arena& A) { track_in_layout(A, c, D); });
        std::vector<char> d(need), h(need);
        Arena AD(d.data(), need), AH(h.data(), need);
        track_in_layout(AD, c, D), track_in_layout(AH, c, H);
        CHECK(!AD.overflow && !AH.overflow && at(D.ids.p, d.data()) == at(H.ids.p, h.data()) && D.loc_at == H.loc_at && D.ids.n == H.ids.n && D.image.n == H.image.n);
    }

    layout_check<TrackWork>((std::string("work, ") + name).c_str(), [&](Arena& A, TrackWork& Y) { track_work_layout(A, c, SLOT, Y); },
        [&](const TrackWork& w) {
            return Rows{{w.cand_off, 4 * (q + 1)}, {w.cand_cnt, 4 * q}, {w.match_q, 4 * q}, {w.num, 16}, {w.who, 4 * kp}, {w.kp_of, 4 * kp}, {w.pred_level, 4 * q},
                        {w.dist, 4 * (64 * q + cand)}, {w.q_valid, q}, {w.q_blocks, q}, {w.occupied, kp}, {w.visible, q}, {w.outlier_kp, kp}, {w.po_outlier, kp},
                        {w.po_level, kp}, {w.po_robust, kp}, {w.reproj, 16 * q}, {w.po_pos, 24 * kp}, {w.x_right, 4 * q}, {w.po_uvr, 12 * kp}, {w.po_w, 4 * kp},
                        {w.po_h, 4 * kp}, {w.po_result, 16}, {w.cur_lm_motion, 4 * kp}, {w.pose, 96}, {w.g_owner, 4 * kp}, {w.g_match, 4 * q}};
        },
        [&](const TrackWork& w, const char* base, size_t) { CHECK((const char*)w.cand_off.p == base); });

    layout_check<TrackOut>((std::string("out, ") + name).c_str(), [&](Arena& A, TrackOut& Y) { track_out_layout(A, c, Y); },
        [&](const TrackOut& o) {
            return Rows{{o.h_stamps, 512}, {o.h_n, 16}, {o.h_num, 16}, {o.h_result, 16}, {o.h_pose, 96}, {o.h_outlier, kp}, {o.h_match, 4 * q}, {o.h_visible, q}, {o.h_obs, ob}};
        },
        [&](const TrackOut& o, const char* base, size_t need) {
            CHECK(o.h_obs.p + pad(ob) == base + need);  // the last piece
            if (!frame_cap) return;
            // the read-back of a frame of this capacity, laid out over h_obs with its padding, stays inside the block
            FrameObs O;
            Arena A(o.h_obs.p, pad(o.h_obs.n));
            frame_obs_layout(A, frame_cap, stereo, O);
            CHECK(!A.overflow && frame_obs_bytes(O) <= o.h_obs.n && (const char*)O.kps_raw.p == o.h_obs.p);
        });
}

static bool no_smaller(const TrackCaps& a, const TrackCaps& b) { return a.kp >= b.kp && a.q >= b.q && a.cand >= b.cand && a.img_bytes >= b.img_bytes && a.obs_bytes >= b.obs_bytes; }

int main() {
    for (const size_t cap : {(size_t)1, (size_t)64, (size_t)(8192 + 8192 / 4 + 64)}) check_slab(cap);

    // the floors: what the very first call holds whatever it asks for
    const TrackCaps none{}, floors = track_caps(none, none);
    CHECK(floors == (TrackCaps{64, 64, 65536, 0, 0}) && track_caps(none, TrackCaps{1, 1, 1, 0, 0}) == floors && track_caps(floors, none) == floors);
    check_tracker("floor", floors);

    // tests/test_gpu_track.py test_candidate_lists_beyond_the_first_capacity: 6 822 keypoints, 6 000 local landmarks on a fresh tracker, then
    // the lists' total (CANDIDATES entries, as an MI355X counts them) with a quarter of headroom and 4 096
    const size_t CANDIDATES = 542978;
    const TrackCaps first = track_caps(none, TrackCaps{6822, 6000, 0, 0, 0});
    CHECK(first == (TrackCaps{6822, 7500, 65536, 0, 0}));
    const TrackCaps grown = track_caps(first, TrackCaps{6822, 6000, CANDIDATES + CANDIDATES / 4 + 4096, 0, 0});
    CHECK(grown == (TrackCaps{6822, 7500, CANDIDATES + CANDIDATES / 4 + 4096, 0, 0}));
    CHECK(track_caps(grown, TrackCaps{6822, 6000, grown.cand, 0, 0}) == grown);  // the call repeated: nothing moves
    check_tracker("after the overflow", grown);

    // 8 192 keypoints of a 640 x 480 image against 8 192 queries, the observation of a frame of the slab's capacity coming back
    const size_t frame_cap = 8192 + 8192 / 4 + 64;
    for (const bool stereo : {false, true}) {
        const TrackCaps big = track_caps(floors, TrackCaps{8192, 8192, floors.cand, 640 * 480, hand_obs_bytes(frame_cap, stereo)});
        CHECK(big == (TrackCaps{8192, 8192 + 2048, 65536, 640 * 480, hand_obs_bytes(frame_cap, stereo)}));
        check_tracker(stereo ? "8192 stereo" : "8192 mono", big, frame_cap, stereo);
    }

    // the policy: never below what is held, never below what is wanted, headroom on the queries only when something grows
    const TrackCaps haves[] = {none, floors, first, grown, TrackCaps{8192, 10240, 65536, 307200, 1000000}};
    const TrackCaps wants[] = {none, TrackCaps{1, 1, 0, 0, 0}, TrackCaps{65, 64, 0, 0, 0}, TrackCaps{64, 65, 0, 0, 0}, TrackCaps{8192, 8192, 0, 307200, 0},
                               TrackCaps{100, 100, 1 << 20, 0, 0}, TrackCaps{6822, 7500, 65536, 0, 1}, TrackCaps{2000, 9000, 70000, 1 << 20, 1 << 20}};
    for (const TrackCaps& have : haves)
        for (const TrackCaps& want : wants) {
            const TrackCaps c = track_caps(have, want);
            CHECK(no_smaller(c, have) && no_smaller(c, want) && no_smaller(c, floors));
            CHECK(track_caps(c, c) == c && track_caps(c, want) == c);  // idempotent; the same call again does not grow
            if (no_smaller(have, want) && no_smaller(have, floors)) CHECK(c == have);
            else if (no_smaller(have, floors)) CHECK(c.q == std::max(want.q + want.q / 4, have.q));
        }
    return layout_check_result("track arena ok");
}
