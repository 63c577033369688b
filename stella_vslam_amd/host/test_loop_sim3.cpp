// module::hip::loop_sim3_validator::validate_batch over the stand-ins, on a toy map (the one of test_bucket_batch.cpp): the current keyframe
// against four candidates in one svgpu_loop_sim3_batch call, compared with the stretch module/loop_detector.cc:537-587 written per candidate
// with the per-call drop-in classes -- the scale (:540-573, restated here), match::hip::projection::match_keyframes_mutually (:577) and
// optimize::hip::transform_optimizer::optimize (:581): the same verdicts, the same scale and Sim3 bit for bit, the same inlier counts, the
// same landmark pointers in curr_match_lms_observed_in_cand, and the first accepted candidate chosen.  Candidate 0 has no prior match (no
// scale), candidate 1 is cut short by the threshold in a second run; priors include entries not observed in the candidate.
// Built by host/Makefile, run by tests/test_gpu_loop_sim3_drop_in.py.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

#include "drop_in/hip_backend.h"
#include "drop_in/loop_detector_hip.h"
#include "drop_in/transform_optimizer_hip.h"

using namespace stella_vslam;
using lm_ptr = std::shared_ptr<data::landmark>;
using kf_ptr = std::shared_ptr<data::keyframe>;
using validator = module::hip::loop_sim3_validator;

#define REQUIRE(c)                                                              \
    do {                                                                        \
        if (!(c)) {                                                             \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                           \
        }                                                                       \
    } while (0)

static Mat44_t look_at(const double c[3], const double target[3]) {
    double z[3] = {target[0] - c[0], target[1] - c[1], target[2] - c[2]};
    const double nz = std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
    for (double& v : z) v /= nz;
    double x[3] = {z[2], 0.0, -z[0]};  // cross((0,1,0), z)
    const double nx = std::sqrt(x[0] * x[0] + x[2] * x[2]);
    for (double& v : x) v /= nx;
    const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
    Mat44_t T = Mat44_t::Identity();
    for (int j = 0; j < 3; ++j) T(0, j) = x[j], T(1, j) = y[j], T(2, j) = z[j];
    for (int i = 0; i < 3; ++i) T(i, 3) = -(T(i, 0) * c[0] + T(i, 1) * c[1] + T(i, 2) * c[2]);
    return T;
}

struct toy_map {
    camera::perspective cam{camera::setup_type_t::Monocular, 752, 480, 458.654, 457.296, 367.215, 248.375, 0, 0, 0, 0, 0};
    feature::orb_params orb;
    std::vector<kf_ptr> kfs;
    std::vector<lm_ptr> lms;
    std::vector<std::vector<int>> truth;  // truth[kf][keypoint] = landmark id or -1
};

static void build(toy_map& M, int n_kf, int n_lm, int n_clutter, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> N(0.0, 1.0);
    M.cam.img_bounds_ = camera::image_bounds{0.f, 752.f, 0.f, 480.f};
    std::vector<std::array<uint8_t, 32>> lm_desc(n_lm);
    std::vector<Vec3_t> pos(n_lm);
    for (int l = 0; l < n_lm; ++l) {
        pos[l](0) = -3.0 + 6.0 * U(rng), pos[l](1) = -1.8 + 3.6 * U(rng), pos[l](2) = 4.5 + 4.0 * U(rng);
        M.lms.push_back(std::make_shared<data::landmark>((unsigned)l, pos[l]));
        for (auto& b : lm_desc[l]) b = (uint8_t)(rng() & 255);
    }
    const double target[3] = {0, 0, 6.5};
    for (int k = 0; k < n_kf; ++k) {
        const double a = -0.06 + 0.12 * k / std::max(1, n_kf - 1);
        const double c[3] = {3.0 * std::sin(a), 0.02 * k, 3.0 - 3.0 * std::cos(a)};
        auto kf = std::make_shared<data::keyframe>((unsigned)k, &M.cam, &M.orb);
        const Mat44_t T = look_at(c, target);
        kf->set_pose_cw(T);
        std::vector<cv::KeyPoint> kps;
        std::vector<std::array<uint8_t, 32>> descs;
        std::vector<int> truth;
        for (int l = 0; l < n_lm; ++l) {
            const Vec3_t& p = pos[l];
            const double X = T(0, 0) * p(0) + T(0, 1) * p(1) + T(0, 2) * p(2) + T(0, 3), Y = T(1, 0) * p(0) + T(1, 1) * p(1) + T(1, 2) * p(2) + T(1, 3);
            const double z = T(2, 0) * p(0) + T(2, 1) * p(1) + T(2, 2) * p(2) + T(2, 3);
            const double u = M.cam.fx_ * X / z + M.cam.cx_, v = M.cam.fy_ * Y / z + M.cam.cy_;
            if (z < 0.5 || u < 8 || u > 744 || v < 8 || v > 472 || U(rng) > 0.85) continue;
            cv::KeyPoint kp;
            const double dist = std::sqrt(std::pow(p(0) - c[0], 2) + std::pow(p(1) - c[1], 2) + std::pow(p(2) - c[2], 2));
            kp.octave = std::min(7, std::max(0, (int)std::lround(std::log(9.0 / dist) / std::log(1.2)) + 1));
            kp.pt.x = (float)(u + 0.4 * N(rng) * M.orb.scale_factors_[kp.octave]);
            kp.pt.y = (float)(v + 0.4 * N(rng) * M.orb.scale_factors_[kp.octave]);
            kp.angle = (float)std::fmod(360.0 + 7.0 * l + 3.0 * N(rng), 360.0);
            auto d = lm_desc[l];
            for (int f = (int)(rng() % 24); f > 0; --f) {
                const unsigned bit = rng() & 255;
                d[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
            }
            kps.push_back(kp), descs.push_back(d), truth.push_back(l);
        }
        for (int e = 0; e < n_clutter; ++e) {
            cv::KeyPoint kp;
            kp.pt.x = (float)(752 * U(rng)), kp.pt.y = (float)(480 * U(rng));
            kp.octave = (int)(rng() % 8), kp.angle = (float)(360 * U(rng));
            std::array<uint8_t, 32> d;
            for (auto& b : d) b = (uint8_t)(rng() & 255);
            kps.push_back(kp), descs.push_back(d), truth.push_back(-1);
        }
        const int n = (int)kps.size();
        kf->frm_obs_.undist_keypts_ = kps;
        kf->frm_obs_.descriptors_.create(n, 32, CV_8U);
        kf->frm_obs_.bearings_.resize(n);
        kf->landmarks_.assign(n, nullptr);
        for (int i = 0; i < n; ++i) {
            std::memcpy(kf->frm_obs_.descriptors_.ptr(i), descs[i].data(), 32);
            const double x = (kps[i].pt.x - M.cam.cx_) / M.cam.fx_, y = (kps[i].pt.y - M.cam.cy_) / M.cam.fy_, l2 = std::sqrt(x * x + y * y + 1.0);
            kf->frm_obs_.bearings_[i](0) = x / l2, kf->frm_obs_.bearings_[i](1) = y / l2, kf->frm_obs_.bearings_[i](2) = 1.0 / l2;
            if (truth[i] >= 0) {
                kf->landmarks_[i] = M.lms[truth[i]];
                M.lms[truth[i]]->add_observation(kf, (unsigned)i);
                if (M.lms[truth[i]]->ref_keyfrm_.expired()) M.lms[truth[i]]->ref_keyfrm_ = kf;
            }
        }
        M.kfs.push_back(kf);
        M.truth.push_back(truth);
    }
    for (auto& lm : M.lms) {
        lm->compute_descriptor();
        lm->update_mean_normal_and_obs_scale_variance();
    }
}

static bool same_sim3(const g2o::Sim3& a, const g2o::Sim3& b) {
    return std::memcmp(a.q, b.q, sizeof a.q) == 0 && std::memcmp(a.t, b.t, sizeof a.t) == 0 && std::memcmp(&a.s, &b.s, sizeof a.s) == 0;
}

// module/loop_detector.cc:540-573: false when there is no scale reference
static bool estimate_scale(const kf_ptr& cur, const Mat44_t& pose_1w_in_cand, const std::vector<lm_ptr>& matched, float& scale_12) {
    const auto lms_curr = cur->get_landmarks();
    const Mat44_t P = cur->get_pose_cw();
    std::vector<float> scales;
    for (unsigned int idx = 0; idx < lms_curr.size(); ++idx) {
        const auto& lm_curr = lms_curr.at(idx);
        const auto& lm_cand = matched.at(idx);
        if (!lm_cand || !lm_curr) continue;
        if (lm_cand->will_be_erased() || lm_curr->will_be_erased()) continue;
        const Vec3_t a = lm_cand->get_pos_in_world(), b = lm_curr->get_pos_in_world();
        double c[3], u[3];
        for (int r = 0; r < 3; ++r) {
            c[r] = ((pose_1w_in_cand(r, 0) * a(0) + pose_1w_in_cand(r, 1) * a(1)) + pose_1w_in_cand(r, 2) * a(2)) + pose_1w_in_cand(r, 3);
            u[r] = ((P(r, 0) * b(0) + P(r, 1) * b(1)) + P(r, 2) * b(2)) + P(r, 3);
        }
        const float n_cand = (float)std::sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]), n_curr = (float)std::sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
        const float cos_parallax = (float)(((c[0] * u[0] + c[1] * u[1]) + c[2] * u[2]) / (n_cand * n_curr));
        constexpr float cos_parallax_thr = 0.99996192306;
        if (!(cos_parallax_thr < cos_parallax)) continue;
        scales.push_back(n_curr / n_cand);
    }
    if (scales.size() < 1) return false;
    std::sort(scales.begin(), scales.end());
    scale_12 = scales[(scales.size() - 1) / 2];
    return true;
}

int main() {
    toy_map M;
    build(M, 6, 260, 60, 11);
    const kf_ptr cur = M.kfs[0];
    const std::vector<kf_ptr> cands{M.kfs[2], M.kfs[3], M.kfs[4], M.kfs[5]};
    const int K = (int)cands.size(), n1 = (int)cur->frm_obs_.undist_keypts_.size();
    const auto lms_curr = cur->get_landmarks();
    // the candidates' inputs: the pose of the current keyframe as the refinement left it (a little off), and the prior matches -- every
    // third landmark of the current keyframe that the candidate observes, plus every 17th whether it observes it or not
    std::mt19937 rng(5);
    std::normal_distribution<double> N(0.0, 1.0);
    std::vector<Mat44_t> poses(K, cur->get_pose_cw());
    std::vector<std::vector<lm_ptr>> priors(K, std::vector<lm_ptr>(n1, nullptr));
    for (int c = 0; c < K; ++c) {
        for (int i = 0; i < 3; ++i) poses[c](i, 3) += 0.002 * N(rng);
        if (c == 0) continue;  // no prior match at all: no scale
        for (int i = 0; i < n1; ++i) {
            const lm_ptr& lm = lms_curr[i];
            if (!lm) continue;
            if ((i % 3 == 0 && lm->is_observed_in_keyframe(cands[c])) || i % 17 == 0) priors[c][i] = lm;
        }
    }
    for (unsigned int thr : {20u, 100000u}) {
        // ---- the batch
        auto matched_batch = priors;
        std::vector<validator::candidate_result> res;
        const validator val(false, thr);
        const int chosen = val.validate_batch(cur, cands, poses, matched_batch, res);
        REQUIRE((int)res.size() == K && val.last_stats_.synchronisations == 2);
        // ---- the reference's loop over the per-call classes
        const match::hip::projection projection_matcher(0.75, true);
        const optimize::hip::transform_optimizer transform_optimizer(false);
        int chosen_ref = -1;
        for (int c = 0; c < K; ++c) {
            auto matched = priors[c];
            float scale_12 = 0.f;
            if (!estimate_scale(cur, poses[c], matched, scale_12)) {
                REQUIRE(res[c].status == SVGPU_LOOP_NO_SCALE && res[c].scale_12 == 0.f && matched_batch[c] == priors[c]);
                continue;
            }
            Mat33_t rot_12;
            Vec3_t trans_12;
            validator::relative_pose(poses[c], cands[c], rot_12, trans_12);
            const unsigned int num_mutual = projection_matcher.match_keyframes_mutually(cur, cands[c], matched, scale_12, rot_12, trans_12, 7.5);
            g2o::Sim3 g2o_sim3_12 = validator::initial_sim3(rot_12, trans_12, scale_12);
            const unsigned int num_optimized_inliers = transform_optimizer.optimize(cur, cands[c], matched, g2o_sim3_12, 10);
            const bool accepted = !(num_optimized_inliers < thr);
            if (accepted && chosen_ref < 0) chosen_ref = c;
            REQUIRE(std::memcmp(&res[c].scale_12, &scale_12, 4) == 0);
            REQUIRE(res[c].num_mutual == num_mutual && res[c].num_optimized_inliers == num_optimized_inliers);
            REQUIRE(res[c].status == (accepted ? 0 : SVGPU_LOOP_FEW_INLIERS));
            REQUIRE(same_sim3(res[c].g2o_sim3_12, g2o_sim3_12));
            REQUIRE(matched_batch[c] == matched);  // the same landmark pointers at the same keypoints
            REQUIRE(num_mutual > 20 && num_optimized_inliers > 40);
            std::printf("thr %u candidate %d: scale %.7f, %u mutual, %u inliers\n", thr, c, scale_12, num_mutual, num_optimized_inliers);
        }
        REQUIRE(chosen == chosen_ref);
        REQUIRE(chosen == (thr == 20u ? 1 : -1));  // the first accepted candidate, not the first candidate
    }
    // no candidate: nothing is called
    std::vector<std::vector<lm_ptr>> none;
    std::vector<validator::candidate_result> res;
    REQUIRE(validator(false, 20).validate_batch(cur, {}, {}, none, res) == -1 && res.empty());
    std::printf("loop sim3 drop-in ok\n");
    return 0;
}
