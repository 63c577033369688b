// module::hip::relocalizer::refine_pose_batch over the stand-ins.
//  (1) host halves alone (`--host-only` stops after them; this part touches no device and is what runs under the sanitizers): `gather`
//      offers exactly the keyframe landmarks that are not null, not will_be_erased and not in already_found_landmarks, flattens the frame's
//      landmark assignment per candidate, and `scatter` puts a planted result back as landmark pointers: matched landmarks added, outliers
//      dropped for an accepted candidate only.
//  (2) on the device: three candidates (accepted; too few matches; accepted from a rolled pose: a start 3 degrees off) against relocalizer::refine_pose written
//      with the per-call drop-in classes (match::hip::projection::match_frame_and_keyframe, optimize::pose_optimizer_hip::optimize) as
//      module/relocalizer.cc:236-297 writes it: the same verdicts, the same poses bit for bit, the same landmark pointers at the same keypoints.
// The toy map is the one of test_bucket_batch.cpp.  Built by host/Makefile, run by tests/test_gpu_reloc_refine_drop_in.py.
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

#include "drop_in/hip_backend.h"
#include "drop_in/pose_optimizer_hip.h"
#include "drop_in/relocalizer_hip.h"

using namespace stella_vslam;
using lm_ptr = std::shared_ptr<data::landmark>;
using kf_ptr = std::shared_ptr<data::keyframe>;
using reloc = module::hip::relocalizer;

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

static bool same_bits(const Mat44_t& a, const Mat44_t& b) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            const double x = a(r, c), y = b(r, c);
            if (std::memcmp(&x, &y, sizeof x) != 0) return false;
        }
    return true;
}

// relocalizer::refine_pose (module/relocalizer.cc:236-297) with the per-call drop-in classes; the frame ends as the reference leaves it
static bool refine_pose_single(data::frame& curr_frm, const kf_ptr& candidate_keyfrm, const std::set<lm_ptr>& already_found_landmarks,
                               const match::hip::projection& proj_matcher, const optimize::pose_optimizer_hip& pose_optimizer, unsigned min_num_valid_obs) {
    auto num_valid_obs = already_found_landmarks.size();
    auto num_found = proj_matcher.match_frame_and_keyframe(curr_frm, candidate_keyfrm, already_found_landmarks, 10, 100);
    if (num_valid_obs + num_found < min_num_valid_obs) return false;
    Mat44_t optimized_pose1;
    std::vector<bool> outlier_flags1;
    auto num_valid_obs1 = pose_optimizer.optimize(curr_frm, optimized_pose1, outlier_flags1);
    curr_frm.set_pose_cw(optimized_pose1);
    std::set<lm_ptr> already_found_landmarks1;
    for (unsigned int idx = 0; idx < curr_frm.frm_obs_.undist_keypts_.size(); ++idx) {
        const auto& lm = curr_frm.get_landmark(idx);
        if (lm) already_found_landmarks1.insert(lm);
    }
    auto num_additional = proj_matcher.match_frame_and_keyframe(curr_frm, candidate_keyfrm, already_found_landmarks1, 3, 64);
    if (num_valid_obs1 + num_additional < min_num_valid_obs) return false;
    Mat44_t optimized_pose2;
    std::vector<bool> outlier_flags2;
    auto num_valid_obs2 = pose_optimizer.optimize(curr_frm, optimized_pose2, outlier_flags2);
    curr_frm.set_pose_cw(optimized_pose2);
    if (num_valid_obs2 < min_num_valid_obs) return false;
    for (unsigned int idx = 0; idx < curr_frm.frm_obs_.undist_keypts_.size(); ++idx)
        if (outlier_flags2.at(idx)) curr_frm.erase_landmark_with_index(idx);
    return true;
}

int main(int argc, char** argv) {
    const bool host_only = argc > 1 && std::strcmp(argv[1], "--host-only") == 0;
    toy_map M;
    build(M, 4, 420, 60, 11);
    // the frame is a copy of keyframe 0's observation; the candidates are keyframes 1 .. 3
    data::frame frm(1000, &M.cam, &M.orb);
    frm.frm_obs_ = M.kfs[0]->frm_obs_;
    const size_t nt = frm.frm_obs_.undist_keypts_.size();
    const std::vector<kf_ptr> cands{M.kfs[1], M.kfs[2], M.kfs[3]};
    // after optimize_pose: the frame holds `take[c]` true landmarks per candidate (the BoW matches that were PnP inliers); the found set is these
    const size_t take[3] = {30, 8, 40};
    std::vector<std::vector<lm_ptr>> frm_lms(3, std::vector<lm_ptr>(nt));
    std::vector<std::set<lm_ptr>> found(3);
    for (int c = 0; c < 3; ++c) {
        size_t got = 0;
        for (size_t k = (size_t)c; k < nt && got < take[c]; k += 3)
            if (M.truth[0][k] >= 0) frm_lms[c][k] = M.lms[M.truth[0][k]], found[c].insert(frm_lms[c][k]), ++got;
    }
    // poses: the frame's own with a small error; candidate 2's rolled by 3 degrees about the optical axis (the outer keypoints wait for stage 2)
    std::vector<Mat44_t> poses(3, M.kfs[0]->get_pose_cw());
    for (int c = 0; c < 3; ++c) poses[c](0, 3) += 0.004 * (c + 1), poses[c](1, 3) -= 0.003;
    {
        const double a = 3.0 * 3.14159265358979323846 / 180.0;
        Mat44_t Rz = Mat44_t::Identity();
        Rz(0, 0) = std::cos(a), Rz(0, 1) = -std::sin(a), Rz(1, 0) = std::sin(a), Rz(1, 1) = std::cos(a);
        poses[2] = Rz * poses[2];
    }
    // candidate 1 offers next to nothing: all but ten of its landmarks are about to be erased ... in a copy of the keyframe, so the others keep theirs
    auto starved = std::make_shared<data::keyframe>(77u, &M.cam, &M.orb);
    starved->frm_obs_ = M.kfs[2]->frm_obs_;
    starved->landmarks_ = M.kfs[2]->landmarks_;
    starved->set_pose_cw(M.kfs[2]->get_pose_cw());
    {
        int kept = 0;
        for (auto& lm : starved->landmarks_)
            if (lm && !found[1].count(lm) && ++kept > 10) lm = nullptr;
    }
    std::vector<kf_ptr> candidates{cands[0], starved, cands[2]};

    // ---- (1) the host halves
    const reloc::flat_problem P = reloc::gather(frm.frm_obs_, candidates, poses, frm_lms, found);
    REQUIRE(P.K == 3 && (size_t)P.nt == nt && P.kf_off.size() == 4 && P.kf_off[0] == 0);
    for (int c = 0; c < 3; ++c) {
        const auto kf_lms = candidates[c]->get_landmarks();
        REQUIRE((size_t)(P.kf_off[c + 1] - P.kf_off[c]) == kf_lms.size());
        REQUIRE(P.n_already_found[c] == (int32_t)found[c].size());
        size_t offered = 0;
        for (size_t i = 0; i < kf_lms.size(); ++i) {
            const size_t e = (size_t)P.kf_off[c] + i;
            const bool want = kf_lms[i] && !kf_lms[i]->will_be_erased() && !found[c].count(kf_lms[i]);
            REQUIRE((P.valid[e] != 0) == want);
            offered += want;
            if (want) {
                const Vec3_t p = kf_lms[i]->get_pos_in_world();
                REQUIRE(P.pos_w[3 * e] == p(0) && P.pos_w[3 * e + 2] == p(2) && P.max_valid_dist[e] == kf_lms[i]->get_max_valid_distance());
                REQUIRE(std::memcmp(&P.lm_desc[32 * e], kf_lms[i]->get_descriptor().ptr(0), 32) == 0);
            }
            REQUIRE(P.angle_kf[e] == candidates[c]->frm_obs_.undist_keypts_[i].angle);
        }
        REQUIRE(c == 1 ? offered == 10 : offered > 150);
        for (size_t k = 0; k < nt; ++k) {
            REQUIRE((P.frame_has_lm[c * nt + k] != 0) == (frm_lms[c][k] != nullptr));
            if (frm_lms[c][k]) REQUIRE(P.frame_lm_pos_w[(c * nt + k) * 3 + 1] == frm_lms[c][k]->get_pos_in_world()(1));
        }
        for (int j = 0; j < 4; ++j) REQUIRE(P.pose_cw[12 * c + 4 + j] == poses[c](1, j));
    }
    {  // a planted result: candidate 0 accepted with one match and one outlier, candidate 1 rejected with one match and a flag that must NOT be applied
        reloc::flat_result R;
        const size_t N = (size_t)P.kf_off[3];
        R.status = {0, 1, 3}, R.pose_out.assign(36, 0.0), R.match_kf.assign(N, -1), R.match_stage.assign(N, -1), R.outlier.assign(3 * nt, 0);
        R.num_found.assign(6, 0), R.num_valid.assign(6, 0), R.lm_iterations.assign(3, 0);
        for (int c = 0; c < 3; ++c)
            for (int j = 0; j < 12; ++j) R.pose_out[12 * c + j] = 100.0 * c + j;
        size_t e0 = 0, e1 = 0, free0 = 0, held0 = 0, free1 = 0, held1 = 0;  // an offered entry, a free and a held keypoint, per candidate
        for (size_t i = (size_t)P.kf_off[0]; i < (size_t)P.kf_off[1]; ++i)
            if (P.valid[i]) e0 = i;
        for (size_t i = (size_t)P.kf_off[1]; i < (size_t)P.kf_off[2]; ++i)
            if (P.valid[i]) e1 = i;
        for (size_t k = 0; k < nt; ++k) {
            if (!frm_lms[0][k]) free0 = k;
            else held0 = k;
            if (!frm_lms[1][k]) free1 = k;
            else held1 = k;
        }
        R.match_kf[e0] = (int32_t)free0, R.match_stage[e0] = 1, R.outlier[0 * nt + held0] = 1, R.num_found[1] = 1, R.num_valid[0] = 31;
        R.match_kf[e1] = (int32_t)free1, R.match_stage[e1] = 0, R.outlier[1 * nt + held1] = 1;
        const auto out = reloc::scatter(P, R, 2, candidates, frm_lms);
        REQUIRE(out.size() == 3 && out[0].accepted && !out[1].accepted && !out[2].accepted && out[2].status == 3);
        REQUIRE(out[0].landmarks[free0] == candidates[0]->get_landmarks()[e0 - (size_t)P.kf_off[0]] && out[0].landmarks[held0] == nullptr);
        REQUIRE(out[1].landmarks[free1] == candidates[1]->get_landmarks()[e1 - (size_t)P.kf_off[1]] && out[1].landmarks[held1] == frm_lms[1][held1]);
        for (size_t k = 0; k < nt; ++k) {
            if (k != free0 && k != held0) REQUIRE(out[0].landmarks[k] == frm_lms[0][k]);
            REQUIRE(out[2].landmarks[k] == frm_lms[2][k]);
        }
        REQUIRE(out[1].pose_cw(0, 1) == 101.0 && out[1].pose_cw(2, 3) == 111.0 && out[1].pose_cw(3, 3) == 1.0 && out[1].pose_cw(3, 0) == 0.0);
        REQUIRE(out[0].num_found.size() == 2 && out[0].num_found[1] == 1 && out[0].num_valid[0] == 31);
    }
    std::printf("relocalizer batch host halves ok\n");
    if (host_only) return 0;

    // ---- (2) on the device, against refine_pose per candidate
    const reloc R(50, true);
    const auto got = R.refine_pose_batch(frm, candidates, poses, frm_lms, found);
    REQUIRE(got.size() == 3);
    const match::hip::projection proj_matcher(0.9f, true);
    const optimize::pose_optimizer_hip pose_optimizer;
    for (int c = 0; c < 3; ++c) {
        data::frame f = frm;
        f.set_landmarks(frm_lms[c]);
        f.set_pose_cw(poses[c]);
        const bool ok = refine_pose_single(f, candidates[c], found[c], proj_matcher, pose_optimizer, 50);
        std::fprintf(stderr, "[reloc batch] candidate %d: single %d, batch status %d, found %u + %u, valid %u / %u\n", c, (int)ok, got[c].status, got[c].num_found[0],
                     got[c].num_found[1], got[c].num_valid[0], got[c].num_valid[1]);
        REQUIRE(ok == got[c].accepted);
        REQUIRE(same_bits(f.get_pose_cw(), got[c].pose_cw));
        REQUIRE(f.get_landmarks() == got[c].landmarks);
    }
    REQUIRE(got[0].accepted && !got[1].accepted && got[1].status == 1 && got[2].accepted);
    REQUIRE(got[0].num_found[0] > 100 && got[2].num_found[0] > 100 && got[1].num_found[0] <= 10);
    REQUIRE(R.last_stats_.synchronisations == 3 && R.last_stats_.launches > 0);
    REQUIRE(R.refine_pose_batch(frm, {}, {}, {}, {}).empty());
    std::printf("relocalizer batch ok\n");
    return 0;
}
