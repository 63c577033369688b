// module::hip::landmark_fuser::fuse beside mapping_module::fuse_landmark_duplication (mapping_module.cc:417-537) written out over
// match::hip::fuse and the stand-in landmark methods (replace, connect_to_keyframe, compute_descriptor,
// update_mean_normal_and_obs_scale_variance).  A toy map in the style of test_drop_in.cpp: nine keyframes on an arc, the middle one current, six
// fuse targets, two further observers; every point has a landmark held by the current keyframe, half of them a duplicate held by some
// targets, the other targets' keypoints hold nothing (new connections).  The same map is built three times and fused through the one batch
// call, through the class's own chain of single calls, and by the written-out loop; compared: the observation map of every landmark, the
// will_be_erased set, replaced_lms, every keyframe's landmark vector, the descriptors bit for bit, normals within 1e-12 and distance
// limits within 1e-6 relative.  Also the fall-back on SVGPU_FUSE_OVERFLOW.  Built by host/Makefile, run by tests/test_gpu_fuse_chain_drop_in.py.
#include <array>
#include <cmath>
#include <cstdio>
#include <random>

#include "drop_in/hip_backend.h"
#include "drop_in/landmark_fuser_hip.h"
#include "fuse_layout.h"

using namespace stella_vslam;
using lm_ptr = std::shared_ptr<data::landmark>;
using kf_ptr = std::shared_ptr<data::keyframe>;

#define REQUIRE(c)                                                              \
    do {                                                                        \
        if (!(c)) {                                                             \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                           \
        }                                                                       \
    } while (0)

struct toy_map {
    camera::perspective cam{camera::setup_type_t::Monocular, 752, 480, 458.654, 457.296, 367.215, 248.375, 0, 0, 0, 0, 0};
    feature::orb_params orb;
    data::map_database db;
    std::vector<kf_ptr> kfs;
    std::vector<lm_ptr> lms;
    kf_ptr cur;
    std::vector<kf_ptr> targets;
};

static void build(toy_map& M, int n_pts, int n_clutter, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    M.cam.img_bounds_ = camera::image_bounds{0.f, 752.f, 0.f, 480.f};
    const int n_kf = 9;
    std::vector<Vec3_t> pts(n_pts);
    std::vector<std::array<uint8_t, 32>> base(n_pts);
    std::vector<int> oct(n_pts);
    for (int l = 0; l < n_pts; ++l) {
        pts[l](0) = -2.2 + 4.4 * U(rng), pts[l](1) = -1.4 + 2.8 * U(rng), pts[l](2) = 5.0 + 4.0 * U(rng);
        for (auto& b : base[l]) b = (uint8_t)(rng() & 255);
        oct[l] = (int)(rng() % 3);
        M.lms.push_back(std::make_shared<data::landmark>((unsigned)l, pts[l]));
    }
    std::vector<std::vector<int>> kp_of(n_kf, std::vector<int>(n_pts, -1));
    for (int k = 0; k < n_kf; ++k) {
        auto kf = std::make_shared<data::keyframe>((unsigned)(10 + 3 * k), &M.cam, &M.orb);
        Mat44_t T = Mat44_t::Identity();
        T(0, 3) = -(-0.3 + 0.075 * k), T(1, 3) = -0.01 * k;  // camera centre (x, y, 0), no rotation
        kf->set_pose_cw(T);
        std::vector<cv::KeyPoint> kps;
        std::vector<std::array<uint8_t, 32>> descs;
        for (int l = 0; l < n_pts; ++l) {
            const double X = pts[l](0) + T(0, 3), Y = pts[l](1) + T(1, 3), Z = pts[l](2);
            const double u = M.cam.fx_ * X / Z + M.cam.cx_, v = M.cam.fy_ * Y / Z + M.cam.cy_;
            if (u < 8 || u > 744 || v < 8 || v > 472) continue;
            cv::KeyPoint kp;
            kp.octave = oct[l];
            kp.pt.x = (float)(u + 0.6 * (U(rng) - 0.5)), kp.pt.y = (float)(v + 0.6 * (U(rng) - 0.5));
            kp.angle = 0.f;
            auto d = base[l];
            for (int f = (int)(rng() % 12); f > 0; --f) {
                const unsigned bit = rng() & 255;
                d[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
            }
            kp_of[k][l] = (int)kps.size();
            kps.push_back(kp), descs.push_back(d);
        }
        for (int e = 0; e < n_clutter; ++e) {
            cv::KeyPoint kp;
            kp.pt.x = (float)(752 * U(rng)), kp.pt.y = (float)(480 * U(rng)), kp.octave = (int)(rng() % 4), kp.angle = 0.f;
            std::array<uint8_t, 32> d;
            for (auto& b : d) b = (uint8_t)(rng() & 255);
            kps.push_back(kp), descs.push_back(d);
        }
        const int n = (int)kps.size();
        kf->frm_obs_.undist_keypts_ = kps;
        kf->frm_obs_.descriptors_.create(n, 32, CV_8U);
        for (int i = 0; i < n; ++i) std::memcpy(kf->frm_obs_.descriptors_.ptr(i), descs[i].data(), 32);
        kf->landmarks_.assign(n, nullptr);
        M.kfs.push_back(kf);
    }
    M.cur = M.kfs[4];
    for (int k : {1, 2, 3, 5, 6, 7}) M.targets.push_back(M.kfs[k]);
    auto connect = [&](const lm_ptr& lm, int k, int l) {
        if (kp_of[k][l] < 0) return;
        if (lm->ref_keyfrm_.expired()) lm->ref_keyfrm_ = M.kfs[k];
        lm->connect_to_keyframe(M.kfs[k], (unsigned)kp_of[k][l]);
    };
    for (int l = 0; l < n_pts; ++l) {
        connect(M.lms[l], 4, l);
        for (int k : {0, 8})
            if (U(rng) < 0.7) connect(M.lms[l], k, l);
    }
    for (int l = 0; l < n_pts; ++l) {
        if (U(rng) < 0.5 || kp_of[4][l] < 0) continue;
        auto dup = std::make_shared<data::landmark>((unsigned)(n_pts + l), pts[l]);
        bool any = false;
        for (int k : {1, 2, 3, 5, 6, 7})
            if (kp_of[k][l] >= 0 && (!any || U(rng) < 0.6)) connect(dup, k, l), any = true;
        if (any) M.lms.push_back(dup);
    }
    for (auto it = M.lms.begin(); it != M.lms.end();) it = (*it)->has_observation() ? it + 1 : M.lms.erase(it);
    for (auto& lm : M.lms) {
        lm->compute_descriptor();
        lm->update_mean_normal_and_obs_scale_variance();
    }
}

// mapping_module.cc:417-537 (the backward candidates in first appearance, where the reference iterates an unordered_set)
static void reference_loop(const kf_ptr& cur_keyfrm_, const std::vector<kf_ptr>& fuse_tgt_keyfrms, data::map_database* map_db_, std::unordered_map<lm_ptr, lm_ptr>& replaced_lms) {
    match::hip::fuse fuse_matcher(0.6);
    {
        auto cur_landmarks = cur_keyfrm_->get_landmarks();
        for (const auto& fuse_tgt_keyfrm : fuse_tgt_keyfrms) {
            std::unordered_map<lm_ptr, lm_ptr> duplicated_lms_in_keyfrm;
            std::unordered_map<unsigned int, lm_ptr> new_connections;
            const Mat33_t rot_cw = fuse_tgt_keyfrm->get_rot_cw();
            const Vec3_t trans_cw = fuse_tgt_keyfrm->get_trans_cw();
            fuse_matcher.detect_duplication(fuse_tgt_keyfrm, rot_cw, trans_cw, cur_landmarks, 3.0, duplicated_lms_in_keyfrm, new_connections, true);
            for (const auto& lms_pair : duplicated_lms_in_keyfrm) {
                auto lm_to_replace = lms_pair.first;
                auto lm_in_keyfrm = lms_pair.second;
                if (lm_to_replace->num_observations() < lm_in_keyfrm->num_observations()) std::swap(lm_to_replace, lm_in_keyfrm);
                if (lm_to_replace->id_ != lm_in_keyfrm->id_) {
                    replaced_lms[lm_in_keyfrm] = lm_to_replace;
                    lm_in_keyfrm->replace(lm_to_replace, map_db_);
                    if (!lm_to_replace->has_representative_descriptor()) lm_to_replace->compute_descriptor();
                    if (!lm_to_replace->has_valid_prediction_parameters()) lm_to_replace->update_mean_normal_and_obs_scale_variance();
                }
            }
            for (const auto& best_idx_lm : new_connections) {
                const auto& best_idx = best_idx_lm.first;
                auto lm = best_idx_lm.second;
                while (replaced_lms.count(lm)) lm = replaced_lms[lm];
                lm->connect_to_keyframe(fuse_tgt_keyfrm, best_idx);
                lm->update_mean_normal_and_obs_scale_variance();
                lm->compute_descriptor();
            }
        }
    }
    {
        std::vector<lm_ptr> candidate_landmarks_to_fuse;
        std::unordered_set<lm_ptr> seen;
        for (const auto& fuse_tgt_keyfrm : fuse_tgt_keyfrms)
            for (const auto& lm : fuse_tgt_keyfrm->get_landmarks()) {
                if (!lm || lm->will_be_erased() || seen.count(lm)) continue;
                seen.insert(lm);
                candidate_landmarks_to_fuse.push_back(lm);
            }
        std::unordered_map<lm_ptr, lm_ptr> duplicated_lms_in_keyfrm;
        std::unordered_map<unsigned int, lm_ptr> new_connections;
        fuse_matcher.detect_duplication(cur_keyfrm_, cur_keyfrm_->get_rot_cw(), cur_keyfrm_->get_trans_cw(), candidate_landmarks_to_fuse, 3.0, duplicated_lms_in_keyfrm,
                                        new_connections, true);
        for (const auto& lms_pair : duplicated_lms_in_keyfrm) {
            auto lm_to_replace = lms_pair.first;
            auto lm_in_keyfrm = lms_pair.second;
            if (lm_to_replace->num_observations() < lm_in_keyfrm->num_observations()) std::swap(lm_to_replace, lm_in_keyfrm);
            if (lm_to_replace->id_ != lm_in_keyfrm->id_) {
                replaced_lms[lm_in_keyfrm] = lm_to_replace;
                lm_in_keyfrm->replace(lm_to_replace, map_db_);
                if (!lm_to_replace->has_representative_descriptor()) lm_to_replace->compute_descriptor();
                if (!lm_to_replace->has_valid_prediction_parameters()) lm_to_replace->update_mean_normal_and_obs_scale_variance();
            }
        }
        for (const auto& best_idx_lm : new_connections) {
            auto lm = best_idx_lm.second;
            while (replaced_lms.count(lm)) lm = replaced_lms[lm];
            lm->connect_to_keyframe(cur_keyfrm_, best_idx_lm.first);
            lm->update_mean_normal_and_obs_scale_variance();
            lm->compute_descriptor();
        }
    }
}

struct lm_state {
    bool erased;
    std::map<unsigned, unsigned> obs;  // keyframe id -> keypoint
    std::array<uint8_t, 32> desc;
    double normal[3];
    float min_d, max_d;
};
struct snapshot {
    std::map<unsigned, lm_state> lms;
    std::map<unsigned, std::vector<int>> kf_lms;  // keyframe id -> landmark id per keypoint, -1 = none
    std::map<unsigned, unsigned> replaced;
    size_t observations = 0;
};
static snapshot take(toy_map& M, const std::unordered_map<lm_ptr, lm_ptr>& replaced) {
    snapshot S;
    for (auto& lm : M.lms) {
        lm_state s{};
        s.erased = lm->will_be_erased();
        for (const auto& o : lm->get_observations()) s.obs[o.first.lock()->id_] = o.second;
        S.observations += s.obs.size();
        if (!s.erased) std::memcpy(s.desc.data(), lm->get_descriptor().ptr(0), 32);
        const Vec3_t n = lm->get_obs_mean_normal();
        for (int k = 0; k < 3; ++k) s.normal[k] = n(k);
        s.min_d = lm->get_min_valid_distance(), s.max_d = lm->get_max_valid_distance();
        S.lms[lm->id_] = s;
    }
    for (auto& kf : M.kfs) {
        std::vector<int> v;
        for (const auto& lm : kf->get_landmarks()) v.push_back(lm ? (int)lm->id_ : -1);
        S.kf_lms[kf->id_] = v;
    }
    for (const auto& r : replaced) S.replaced[r.first->id_] = r.second->id_;
    return S;
}
static bool same(const snapshot& a, const snapshot& b, const char* what) {
    bool ok = a.kf_lms == b.kf_lms && a.replaced == b.replaced && a.lms.size() == b.lms.size();
    for (const auto& e : a.lms) {
        const auto it = b.lms.find(e.first);
        if (it == b.lms.end()) return false;
        const lm_state &x = e.second, &y = it->second;
        bool one = x.erased == y.erased && x.obs == y.obs;
        if (one && !x.erased) {
            one = x.desc == y.desc && std::fabs(x.max_d - y.max_d) <= 1e-6f * std::fabs(y.max_d) && std::fabs(x.min_d - y.min_d) <= 1e-6f * std::fabs(y.min_d);
            for (int k = 0; k < 3; ++k) one = one && std::fabs(x.normal[k] - y.normal[k]) <= 1e-12;
        }
        if (!one) std::fprintf(stderr, "%s: landmark %u differs\n", what, e.first);
        ok = ok && one;
    }
    return ok;
}

int main() {
    const int n_pts = 160, n_clutter = 120;
    const unsigned seed = 4242;
    snapshot before, by_batch, by_chain, by_reference, by_fallback;
    {
        toy_map M;
        build(M, n_pts, n_clutter, seed);
        before = take(M, {});
        std::unordered_map<lm_ptr, lm_ptr> replaced;
        module::hip::landmark_fuser fuser;
        REQUIRE(fuser.min_targets_for_batch_ == 1);
        fuser.fuse(M.cur, M.targets, &M.db, replaced);
        REQUIRE(fuser.last_took_batch_ && !fuser.last_overflowed_ && fuser.last_stats_.synchronisations == 2);
        by_batch = take(M, replaced);
    }
    {
        toy_map M;
        build(M, n_pts, n_clutter, seed);
        std::unordered_map<lm_ptr, lm_ptr> replaced;
        module::hip::landmark_fuser fuser;
        fuser.min_targets_for_batch_ = 100;  // below the threshold: the class's own chain of single calls
        fuser.fuse(M.cur, M.targets, &M.db, replaced);
        REQUIRE(!fuser.last_took_batch_);
        by_chain = take(M, replaced);
    }
    {
        toy_map M;
        build(M, n_pts, n_clutter, seed);
        std::unordered_map<lm_ptr, lm_ptr> replaced;
        reference_loop(M.cur, M.targets, &M.db, replaced);
        by_reference = take(M, replaced);
    }
    {
        toy_map M;
        build(M, n_pts, n_clutter, seed);
        std::unordered_map<lm_ptr, lm_ptr> replaced;
        module::hip::landmark_fuser fuser;
        fuser.obs_slack_ = -(7 + FUSE_OBS_SLACK);  // every list exactly full: the first merge makes the call report SVGPU_FUSE_OVERFLOW, and the chain runs
        fuser.fuse(M.cur, M.targets, &M.db, replaced);
        REQUIRE(fuser.last_overflowed_ && !fuser.last_took_batch_);
        by_fallback = take(M, replaced);
    }
    // the planted work happened: duplicates were replaced, observations were added, and a survivor of an early target is skipped later
    REQUIRE(by_reference.replaced.size() >= 20);
    REQUIRE(by_reference.observations > before.observations);
    size_t erased = 0;
    for (const auto& e : by_reference.lms) erased += e.second.erased;
    REQUIRE(erased == by_reference.replaced.size());
    REQUIRE(same(by_batch, by_reference, "batch call vs written-out loop"));
    REQUIRE(same(by_chain, by_reference, "single-call chain vs written-out loop"));
    REQUIRE(same(by_batch, by_chain, "batch call vs single-call chain"));
    REQUIRE(same(by_fallback, by_reference, "fall-back vs written-out loop"));
    std::printf("replaced %zu, observations %zu -> %zu\nlandmark fuser drop-in ok\n", by_reference.replaced.size(), before.observations, by_reference.observations);
    return 0;
}
