// optimize::pose_optimizer_hip (pose_optimizer_hip.h): gather -> svgpu_pose_optimize[_batch] -> pose(s) and flags back.
#include "drop_in/pose_optimizer_hip.h"

#include <cmath>

namespace stella_vslam {
namespace optimize {

pose_optimizer_hip::pose_optimizer_hip(const unsigned int num_trials_robust, const unsigned int num_trials, const unsigned int num_each_iter)
    : num_trials_robust_(num_trials_robust), num_trials_(num_trials), num_each_iter_(num_each_iter) {}

unsigned int pose_optimizer_hip::optimize(const data::frame& frm, Mat44_t& optimized_pose, std::vector<bool>& outlier_flags) const {
    return optimize(frm.get_pose_cw(), frm.frm_obs_, frm.orb_params_, frm.camera_, frm.get_landmarks(), optimized_pose, outlier_flags);  // pose_optimizer_g2o.cc:26-30
}

unsigned int pose_optimizer_hip::optimize(const data::keyframe* keyfrm, Mat44_t& optimized_pose, std::vector<bool>& outlier_flags) const {
    return optimize(keyfrm->get_pose_cw(), keyfrm->frm_obs_, keyfrm->orb_params_, keyfrm->camera_, keyfrm->get_landmarks(), optimized_pose, outlier_flags);  // :32-36
}

namespace {

// steps 2-3 of pose_optimizer_g2o.cc:62-109 for one landmark assignment: the observations are appended to the flat arrays
struct gathered {
    std::vector<unsigned int> kp_of_obs;
    std::vector<double> pos_w;
    std::vector<float> uvr, inv_sigma_sq, huber;
};
void gather(const data::frame_observation& frm_obs, const feature::orb_params* orb_params, const camera::base* camera,
            const std::vector<std::shared_ptr<data::landmark>>& landmarks, gathered& g) {
    const unsigned int num_keypts = frm_obs.undist_keypts_.size();
    constexpr float chi_sq_2D = 5.99146;
    const float sqrt_chi_sq_2D = std::sqrt(chi_sq_2D);
    constexpr float chi_sq_3D = 7.81473;
    const float sqrt_chi_sq_3D = std::sqrt(chi_sq_3D);
    const float sqrt_chi_sq = camera->setup_type_ == camera::setup_type_t::Monocular ? sqrt_chi_sq_2D : sqrt_chi_sq_3D;  // :103-105
    for (unsigned int idx = 0; idx < num_keypts; ++idx) {  // :86-109
        const auto& lm = landmarks.at(idx);
        if (!lm || lm->will_be_erased()) continue;
        const auto& undist_keypt = frm_obs.undist_keypts_.at(idx);
        const float x_right = frm_obs.stereo_x_right_.empty() ? -1.0f : frm_obs.stereo_x_right_.at(idx);
        const Vec3_t p = lm->get_pos_in_world();
        g.kp_of_obs.push_back(idx);
        for (int k = 0; k < 3; ++k) g.pos_w.push_back(p(k));
        g.uvr.push_back(undist_keypt.pt.x);
        g.uvr.push_back(undist_keypt.pt.y);
        g.uvr.push_back(x_right);
        g.inv_sigma_sq.push_back(orb_params->inv_level_sigma_sq_.at(undist_keypt.octave));
        g.huber.push_back(sqrt_chi_sq);
    }
}
// the edge the wrapper builds per camera model (pose_opt_edge_wrapper.h:57-200): perspective, fisheye and radial division all take the
// perspective edge on the undistorted keypoints; equirectangular its own
void edge_intrinsics(const camera::base* camera, double* K) {
    const svgpu_camera c = hip::to_svgpu_camera(camera);
    if (c.model == SVGPU_CAM_EQUIRECTANGULAR) K[0] = 0, K[1] = 0, K[2] = c.cols, K[3] = c.rows, K[4] = 0;
    else K[0] = c.fx, K[1] = c.fy, K[2] = c.cx, K[3] = c.cy, K[4] = c.focal_x_baseline;
}

}  // namespace

unsigned int pose_optimizer_hip::optimize(const Mat44_t& cam_pose_cw, const data::frame_observation& frm_obs, const feature::orb_params* orb_params,
                                          const camera::base* camera, const std::vector<std::shared_ptr<data::landmark>>& landmarks, Mat44_t& optimized_pose,
                                          std::vector<bool>& outlier_flags) const {
    const unsigned int num_keypts = frm_obs.undist_keypts_.size();
    outlier_flags.resize(num_keypts);  // :68-70
    std::fill(outlier_flags.begin(), outlier_flags.end(), false);
    gathered g;
    gather(frm_obs, orb_params, camera, landmarks, g);
    const int n = (int)g.kp_of_obs.size();
    last_lm_iterations_ = 0;
    if (n < 5) return 0;  // :111-113 (optimized_pose is left as the caller passed it)

    double K[5];
    edge_intrinsics(camera, K);
    double pose_in[12], pose_out[12];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) pose_in[4 * i + j] = cam_pose_cw(i, j);
    std::vector<uint8_t> flags((size_t)n, 0);
    int num_valid = 0;
    hip::check(svgpu_pose_optimize(hip::context(), pose_in, n, g.pos_w.data(), g.uvr.data(), g.inv_sigma_sq.data(), g.huber.data(), K, (int)num_trials_robust_,
                                   (int)num_trials_, (int)num_each_iter_, reset_stop_flag_each_round_, pose_out, flags.data(), &num_valid, &last_lm_iterations_),
               "svgpu_pose_optimize");
    for (int k = 0; k < n; ++k) outlier_flags.at(g.kp_of_obs[k]) = flags[k] != 0;  // :130-160: flags by keypoint index
    optimized_pose = Mat44_t::Identity();  // :171 (to_eigen_mat of the vertex estimate)
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) optimized_pose(i, j) = pose_out[4 * i + j];
    return (unsigned int)num_valid;
}

std::vector<unsigned int> pose_optimizer_hip::optimize_batch(const std::vector<Mat44_t>& cam_poses_cw, const data::frame_observation& frm_obs,
                                                             const feature::orb_params* orb_params, const camera::base* camera,
                                                             const std::vector<std::vector<std::shared_ptr<data::landmark>>>& landmarks_per_candidate,
                                                             std::vector<Mat44_t>& optimized_poses, std::vector<std::vector<bool>>& outlier_flags) const {
    const size_t num_cands = cam_poses_cw.size();
    if (landmarks_per_candidate.size() != num_cands) hip::check(SVGPU_ERR_INVALID, "pose_optimizer_hip::optimize_batch: one landmark assignment per pose");
    const unsigned int num_keypts = frm_obs.undist_keypts_.size();
    optimized_poses.resize(num_cands);  // (an entry of a candidate with fewer than 5 observations is left as the caller passed it, as in the single call)
    outlier_flags.assign(num_cands, std::vector<bool>(num_keypts, false));
    std::vector<unsigned int> num_valid_per_cand(num_cands, 0);
    last_lm_iterations_ = 0;
    if (num_cands == 0) return num_valid_per_cand;

    gathered g;  // the candidates' observations one after another: obs_off[c] .. obs_off[c + 1] are candidate c's
    std::vector<int32_t> obs_off(num_cands + 1, 0);
    std::vector<double> poses_in(12 * num_cands), poses_out(12 * num_cands);
    for (size_t c = 0; c < num_cands; ++c) {
        gather(frm_obs, orb_params, camera, landmarks_per_candidate[c], g);
        obs_off[c + 1] = (int32_t)g.kp_of_obs.size();
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) poses_in[12 * c + 4 * i + j] = cam_poses_cw[c](i, j);
    }
    double K[5];
    edge_intrinsics(camera, K);
    std::vector<uint8_t> flags(g.kp_of_obs.size() + 1, 0);
    std::vector<int32_t> num_valid(num_cands, 0), lm_iterations(num_cands, 0);
    hip::check(svgpu_pose_optimize_batch(hip::context(), (int)num_cands, obs_off.data(), poses_in.data(), nullptr, g.pos_w.data(), g.uvr.data(),
                                         g.inv_sigma_sq.data(), g.huber.data(), nullptr, K, (int)num_trials_robust_, (int)num_trials_, (int)num_each_iter_,
                                         reset_stop_flag_each_round_, poses_out.data(), flags.data(), num_valid.data(), lm_iterations.data()),
               "svgpu_pose_optimize_batch");
    for (size_t c = 0; c < num_cands; ++c) {
        last_lm_iterations_ += lm_iterations[c];
        if (obs_off[c + 1] - obs_off[c] < 5) continue;  // :111-113
        for (int32_t k = obs_off[c]; k < obs_off[c + 1]; ++k) outlier_flags[c].at(g.kp_of_obs[k]) = flags[k] != 0;
        optimized_poses[c] = Mat44_t::Identity();
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) optimized_poses[c](i, j) = poses_out[12 * c + 4 * i + j];
        num_valid_per_cand[c] = (unsigned int)num_valid[c];
    }
    return num_valid_per_cand;
}

namespace hip_backend {
std::unique_ptr<pose_optimizer> create_pose_optimizer(const std::string& backend, const unsigned int num_trials_robust, const unsigned int num_trials,
                                                      const unsigned int num_each_iter) {
    if (backend == "hip") return std::unique_ptr<pose_optimizer>(new pose_optimizer_hip(num_trials_robust, num_trials, num_each_iter));
    return nullptr;
}
}  // namespace hip_backend

}  // namespace optimize
}  // namespace stella_vslam
