// optimize::pose_optimizer_hip::optimize_batch over the stand-ins: (1) three candidates of one frame observation, one of them with fewer
// than 5 landmarks, give bit for bit what three single calls give; (2) solve::hip::pnp_solver::find_via_ransac_batch -> optimize_batch on
// two synthetic candidates, the way relocalizer::reloc_by_candidate chains them (PnP pose, landmarks of the PnP inliers), brings the
// planted pose back and again equals the single calls.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "drop_in/pnp_solver_hip.h"
#include "drop_in/pose_optimizer_hip.h"

using namespace stella_vslam;

namespace {
unsigned long long g_state = 88172645463325252ull;
double uni() {  // xorshift64, [0, 1)
    g_state ^= g_state << 13, g_state ^= g_state >> 7, g_state ^= g_state << 17;
    return (double)(g_state >> 11) / 9007199254740992.0;
}
int g_fail = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                           \
        }                                                       \
    } while (0)

using lm_ptr = std::shared_ptr<data::landmark>;

Mat44_t pose_about_y(double yaw, double cx, double cy, double cz) {  // pos_c = R (pos_w - centre), R = [c 0 s; 0 1 0; -s 0 c]
    const double c = std::cos(yaw), s = std::sin(yaw);
    Mat44_t T = Mat44_t::Identity();
    T(0, 0) = c, T(0, 2) = s, T(2, 0) = -s, T(2, 2) = c;
    const double ctr[3] = {cx, cy, cz};
    for (int i = 0; i < 3; ++i) T(i, 3) = -(T(i, 0) * ctr[0] + T(i, 1) * ctr[1] + T(i, 2) * ctr[2]);
    return T;
}

// a frame of n keypoints seen from T with half-pixel noise, and the landmark behind every keypoint
struct scene {
    camera::perspective cam{camera::setup_type_t::Monocular, 752, 480, 458.654, 457.296, 367.215, 248.375, 0, 0, 0, 0, 0};
    feature::orb_params orb;
    data::frame_observation obs;
    std::vector<lm_ptr> truth;
    Mat44_t T;
};
void build(scene& S, int n, unsigned first_id) {
    S.T = pose_about_y(0.12, 0.4, -0.1, 0.3);
    const double c = std::cos(0.12), s = std::sin(0.12);
    for (int i = 0; i < n; ++i) {
        const double d = 3.0 + 6.0 * uni();
        const double X = (uni() - 0.5) * d, Y = (uni() - 0.5) * 0.7 * d, Z = d;  // camera frame
        Vec3_t pw;
        pw(0) = c * X - s * Z + 0.4, pw(1) = Y - 0.1, pw(2) = s * X + c * Z + 0.3;
        cv::KeyPoint kp;
        kp.octave = i % 8;
        kp.pt.x = (float)(S.cam.fx_ * X / Z + S.cam.cx_ + (uni() - 0.5) * S.orb.scale_factors_[kp.octave]);
        kp.pt.y = (float)(S.cam.fy_ * Y / Z + S.cam.cy_ + (uni() - 0.5) * S.orb.scale_factors_[kp.octave]);
        S.obs.undist_keypts_.push_back(kp);
        Vec3_t b;
        const double bx = (kp.pt.x - S.cam.cx_) / S.cam.fx_, by = (kp.pt.y - S.cam.cy_) / S.cam.fy_, l = std::sqrt(bx * bx + by * by + 1.0);
        b(0) = bx / l, b(1) = by / l, b(2) = 1.0 / l;
        S.obs.bearings_.push_back(b);
        S.truth.push_back(std::make_shared<data::landmark>(first_id + (unsigned)i, pw));
    }
}

bool same_bits(const Mat44_t& a, const Mat44_t& b) {
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            const double x = a(r, c), y = b(r, c);
            if (std::memcmp(&x, &y, sizeof x) != 0) return false;
        }
    return true;
}

// optimize_batch against one single call per candidate: counts, poses, flags bit for bit, and the iteration counts add up
void check_against_single_calls(const optimize::pose_optimizer_hip& po, const scene& S, const std::vector<Mat44_t>& poses,
                                const std::vector<std::vector<lm_ptr>>& lms, std::vector<Mat44_t>& out, std::vector<unsigned int>& valid) {
    std::vector<std::vector<bool>> flags;
    out = poses;
    valid = po.optimize_batch(poses, S.obs, &S.orb, &S.cam, lms, out, flags);
    const int batch_iterations = po.last_lm_iterations_;
    CHECK(valid.size() == poses.size() && out.size() == poses.size() && flags.size() == poses.size());
    int single_iterations = 0;
    for (size_t c = 0; c < poses.size(); ++c) {
        Mat44_t one = poses[c];
        std::vector<bool> one_flags;
        const unsigned int one_valid = po.optimize(poses[c], S.obs, &S.orb, &S.cam, lms[c], one, one_flags);
        single_iterations += po.last_lm_iterations_;
        CHECK(one_valid == valid[c]);
        CHECK(same_bits(one, out[c]));
        CHECK(one_flags == flags[c]);
    }
    CHECK(single_iterations == batch_iterations && batch_iterations > 0);
}
}  // namespace

int main() {
    optimize::pose_optimizer_hip po;
    {  // (1) three landmark assignments of one frame observation
        scene S;
        build(S, 300, 0);
        const size_t n = S.truth.size();
        std::vector<std::vector<lm_ptr>> lms(3, std::vector<lm_ptr>(n));
        lms[0] = S.truth;
        for (size_t i : {7u, 70u, 150u, 299u}) lms[1][i] = S.truth[i];  // fewer than 5 landmarks: nothing to optimise
        for (size_t i = 0; i < n; i += 2) lms[2][i] = S.truth[i];
        for (size_t i = 0; i < n; i += 26) lms[2][i] = S.truth[(i + 13) % n];  // and a few wrong landmarks
        std::vector<Mat44_t> poses(3, S.T);
        for (int i = 0; i < 3; ++i) poses[0](i, 3) += 0.03 * (i + 1), poses[1](i, 3) -= 0.02, poses[2](i, 3) -= 0.025 * (i + 1);
        std::vector<Mat44_t> out;
        std::vector<unsigned int> valid;
        check_against_single_calls(po, S, poses, lms, out, valid);
        CHECK(valid[0] > 250 && valid[1] == 0 && valid[2] > 120 && valid[2] <= 150);
        CHECK(same_bits(out[1], poses[1]));  // the skipped candidate's pose is left as it was passed
        for (int c : {0, 2}) {  // the perturbed translation comes back towards the frame's (the criterion of test_drop_in's pose optimizer block)
            double e0 = 0, e1 = 0;
            for (int i = 0; i < 3; ++i) e0 += std::fabs(poses[c](i, 3) - S.T(i, 3)), e1 += std::fabs(out[c](i, 3) - S.T(i, 3));
            std::fprintf(stderr, "[pose batch] candidate %d: %u good observations, translation error %.4f -> %.4f\n", c, valid[c], e0, e1);
            CHECK(e1 < 0.2 * e0);
        }
        // no candidate at all
        std::vector<std::vector<bool>> none_flags;
        std::vector<Mat44_t> none_out;
        CHECK(po.optimize_batch({}, S.obs, &S.orb, &S.cam, {}, none_out, none_flags).empty() && po.last_lm_iterations_ == 0);
    }
    {  // (2) PnP for both candidates in one call, then the pose optimisation of both in one call
        scene S;
        build(S, 240, 1000);
        const size_t n = S.truth.size();
        // what the BoW matcher would hand over: candidate 0 matched the even keypoints, candidate 1 two of every three; every tenth match is wrong
        std::vector<std::vector<lm_ptr>> matched(2, std::vector<lm_ptr>(n));
        for (size_t i = 0; i < n; ++i) {
            const lm_ptr lm = i % 10 == 9 ? S.truth[(i + 37) % n] : S.truth[i];
            if (i % 2 == 0) matched[0][i] = lm;
            if (i % 3 != 0) matched[1][i] = lm;
        }
        using solver = solve::hip::pnp_solver;
        std::vector<std::unique_ptr<solver>> solvers;
        std::vector<std::vector<unsigned int>> valid_indices(2);
        for (int c = 0; c < 2; ++c) {  // relocalizer.cc: setup_pnp_solver
            eigen_alloc_vector<Vec3_t> bearings, points;
            std::vector<int> octaves;
            for (unsigned int i = 0; i < n; ++i) {
                if (!matched[c][i]) continue;
                valid_indices[c].push_back(i);
                bearings.push_back(S.obs.bearings_[i]);
                octaves.push_back(S.obs.undist_keypts_[i].octave);
                points.push_back(matched[c][i]->get_pos_in_world());
            }
            solvers.emplace_back(new solver(bearings, octaves, points, S.orb.scale_factors_, 10, true, 10));
        }
        solver::find_via_ransac_batch({solvers[0].get(), solvers[1].get()}, 30, true);
        std::vector<Mat44_t> poses;
        std::vector<std::vector<lm_ptr>> lms;
        for (int c = 0; c < 2; ++c) {  // erase_landmarks(), then the landmarks of the PnP inliers; the PnP pose
            CHECK(solvers[c]->solution_is_valid());
            if (!solvers[c]->solution_is_valid()) continue;
            poses.push_back(solvers[c]->get_best_cam_pose());
            const auto inlier = solvers[c]->get_inlier_flags();
            CHECK(inlier.size() == valid_indices[c].size());
            lms.emplace_back(n);
            for (size_t k = 0; k < inlier.size(); ++k)
                if (inlier[k]) lms.back()[valid_indices[c][k]] = matched[c][valid_indices[c][k]];
        }
        CHECK(poses.size() == 2);
        if (poses.size() == 2) {
            std::vector<Mat44_t> out;
            std::vector<unsigned int> valid;
            check_against_single_calls(po, S, poses, lms, out, valid);
            CHECK(valid[0] >= 90 && valid[1] >= 120);
            // sanity only (the start is the PnP pose, already near the truth): a keypoint is at most 0.5 * 1.2^7 = 1.8 px off, 0.035 m at the
            // scene's 9 m; a pose from 90 and more such observations is not further off than one of them
            for (int c = 0; c < 2; ++c)
                for (int i = 0; i < 3; ++i) CHECK(std::fabs(out[c](i, 3) - S.T(i, 3)) < 0.05);
        }
    }
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("pose_optimizer batch ok\n");
    return 0;
}
