// module::hip::relocalizer (relocalizer_hip.h): gather -> svgpu_reloc_refine_batch -> landmark vectors, poses and verdicts back.
#include "drop_in/relocalizer_hip.h"

#include <cstring>

namespace stella_vslam {
namespace hip {  // (hip_backend.h / hip_backend.cc)
svgpu_ctx* context();
svgpu_camera to_svgpu_camera(const camera::base* camera);
void check(int status, const char* where);
}  // namespace hip

namespace module {
namespace hip {

namespace backend = ::stella_vslam::hip;

relocalizer::relocalizer(const unsigned int min_num_valid_obs, const bool check_orientation, const unsigned int num_trials_robust, const unsigned int num_trials,
                         const unsigned int num_each_iter)
    : min_num_valid_obs_(min_num_valid_obs), check_orientation_(check_orientation), num_trials_robust_(num_trials_robust), num_trials_(num_trials),
      num_each_iter_(num_each_iter) {}

relocalizer::flat_problem relocalizer::gather(const data::frame_observation& frm_obs, const std::vector<kf_ptr>& candidate_keyfrms, const std::vector<Mat44_t>& poses_cw,
                                              const std::vector<std::vector<lm_ptr>>& landmarks_per_candidate,
                                              const std::vector<std::set<lm_ptr>>& already_found_landmarks) {
    flat_problem P;
    const size_t K = candidate_keyfrms.size();
    if (poses_cw.size() != K || landmarks_per_candidate.size() != K || already_found_landmarks.size() != K)
        backend::check(SVGPU_ERR_INVALID, "relocalizer::refine_pose_batch: one pose, landmark assignment and found set per candidate");
    const size_t nt = frm_obs.undist_keypts_.size();
    P.nt = (int)nt, P.K = (int)K;
    // the frame, once
    P.tdesc.resize(nt * 32), P.t_xy.resize(nt * 2), P.t_angle.resize(nt), P.t_octave.resize(nt);
    for (size_t i = 0; i < nt; ++i) {
        std::memcpy(&P.tdesc[i * 32], frm_obs.descriptors_.ptr((int)i), 32);
        const auto& kp = frm_obs.undist_keypts_[i];
        P.t_xy[2 * i] = kp.pt.x, P.t_xy[2 * i + 1] = kp.pt.y;
        P.t_angle[i] = kp.angle;
        P.t_octave[i] = kp.octave;
    }
    if (!frm_obs.stereo_x_right_.empty()) P.t_xright.assign(frm_obs.stereo_x_right_.begin(), frm_obs.stereo_x_right_.end());
    // per candidate: pose, the frame's landmarks after optimize_pose, the keyframe's landmark entries
    P.pose_cw.resize(K * 12), P.n_already_found.resize(K), P.frame_has_lm.assign(K * nt, 0), P.frame_lm_pos_w.assign(K * nt * 3, 0.0);
    P.kf_off.assign(K + 1, 0);
    for (size_t c = 0; c < K; ++c) {
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) P.pose_cw[12 * c + 4 * i + j] = poses_cw[c](i, j);
        P.n_already_found[c] = (int32_t)already_found_landmarks[c].size();  // relocalizer.cc:241
        const auto& frm_lms = landmarks_per_candidate[c];
        if (frm_lms.size() != nt) backend::check(SVGPU_ERR_INVALID, "relocalizer::refine_pose_batch: one landmark slot per frame keypoint");
        for (size_t k = 0; k < nt; ++k) {
            const auto& lm = frm_lms[k];
            if (!lm || lm->will_be_erased()) continue;  // (what the pose optimiser's gather skips as well: pose_optimizer_g2o.cc:88-91)
            P.frame_has_lm[c * nt + k] = 1;
            const Vec3_t p = lm->get_pos_in_world();
            for (int d = 0; d < 3; ++d) P.frame_lm_pos_w[(c * nt + k) * 3 + d] = p(d);
        }
        const auto kf_lms = candidate_keyfrms[c]->get_landmarks();
        const auto& kf_obs = candidate_keyfrms[c]->frm_obs_;
        const size_t n = kf_lms.size(), o = P.pos_w.size() / 3;
        P.kf_off[c + 1] = (int32_t)(o + n);
        P.pos_w.resize((o + n) * 3, 0.0), P.valid.resize(o + n, 0), P.min_valid_dist.resize(o + n, 0.f), P.max_valid_dist.resize(o + n, 0.f);
        P.lm_desc.resize((o + n) * 32, 0), P.angle_kf.resize(o + n, 0.f);
        for (size_t i = 0; i < n; ++i) {
            if (i < kf_obs.undist_keypts_.size()) P.angle_kf[o + i] = kf_obs.undist_keypts_[i].angle;
            const auto& lm = kf_lms[i];
            if (!lm || lm->will_be_erased() || already_found_landmarks[c].count(lm)) continue;  // projection.cc:237-245
            const cv::Mat d = lm->get_descriptor();
            if (d.empty()) continue;  // (no representative descriptor yet: nothing to compare)
            P.valid[o + i] = 1;
            const Vec3_t p = lm->get_pos_in_world();
            for (int k = 0; k < 3; ++k) P.pos_w[(o + i) * 3 + k] = p(k);
            P.min_valid_dist[o + i] = lm->get_min_valid_distance();
            P.max_valid_dist[o + i] = lm->get_max_valid_distance();
            std::memcpy(&P.lm_desc[(o + i) * 32], d.ptr(0), 32);
        }
    }
    return P;
}

std::vector<relocalizer::candidate_result> relocalizer::scatter(const flat_problem& P, const flat_result& R, const int num_stages,
                                                                const std::vector<kf_ptr>& candidate_keyfrms,
                                                                const std::vector<std::vector<lm_ptr>>& landmarks_per_candidate) {
    const size_t K = (size_t)P.K, nt = (size_t)P.nt, S = (size_t)num_stages;
    std::vector<candidate_result> out(K);
    for (size_t c = 0; c < K; ++c) {
        candidate_result& r = out[c];
        r.status = R.status.at(c);
        r.accepted = r.status == 0;
        r.pose_cw = Mat44_t::Identity();
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) r.pose_cw(i, j) = R.pose_out.at(12 * c + 4 * i + j);
        r.landmarks = landmarks_per_candidate[c];
        const auto kf_lms = candidate_keyfrms[c]->get_landmarks();
        for (int32_t e = P.kf_off[c]; e < P.kf_off[c + 1]; ++e) {  // projection.cc:313, both stages
            const int32_t k = R.match_kf.at((size_t)e);
            if (0 <= k) r.landmarks.at((size_t)k) = kf_lms.at((size_t)(e - P.kf_off[c]));
        }
        if (r.accepted)  // relocalizer.cc:288-295
            for (size_t k = 0; k < nt; ++k)
                if (R.outlier.at(c * nt + k)) r.landmarks[k] = nullptr;
        for (size_t s = 0; s < S; ++s) {
            r.num_found.push_back((unsigned int)R.num_found.at(c * S + s));
            r.num_valid.push_back((unsigned int)R.num_valid.at(c * S + s));
        }
    }
    return out;
}

std::vector<relocalizer::candidate_result> relocalizer::refine_pose_batch(const data::frame& frm, const std::vector<kf_ptr>& candidate_keyfrms,
                                                                          const std::vector<Mat44_t>& poses_cw,
                                                                          const std::vector<std::vector<lm_ptr>>& landmarks_per_candidate,
                                                                          const std::vector<std::set<lm_ptr>>& already_found_landmarks) const {
    last_stats_ = svgpu_call_stats{0, 0, 0};
    if (candidate_keyfrms.empty()) return {};
    const flat_problem P = gather(frm.frm_obs_, candidate_keyfrms, poses_cw, landmarks_per_candidate, already_found_landmarks);
    const size_t K = (size_t)P.K, nt = (size_t)P.nt, N = (size_t)P.kf_off[K], S = margins_.size();
    if (hamm_dist_thrs_.size() != S) backend::check(SVGPU_ERR_INVALID, "relocalizer::refine_pose_batch: one margin and one threshold per stage");
    const svgpu_camera cam = backend::to_svgpu_camera(frm.camera_);
    double intr[5];  // the edge the pose optimiser builds per camera model (pose_optimizer_hip.cc)
    if (cam.model == SVGPU_CAM_EQUIRECTANGULAR) intr[0] = 0, intr[1] = 0, intr[2] = cam.cols, intr[3] = cam.rows, intr[4] = 0;
    else intr[0] = cam.fx, intr[1] = cam.fy, intr[2] = cam.cx, intr[3] = cam.cy, intr[4] = cam.focal_x_baseline;
    const auto* orb = frm.orb_params_;
    flat_result R;
    R.status.assign(K, 0), R.pose_out.assign(K * 12, 0.0), R.match_kf.assign(N + 1, -1), R.match_stage.assign(N + 1, -1), R.outlier.assign(K * nt + 1, 0);
    R.num_found.assign(K * S, 0), R.num_valid.assign(K * S, 0), R.lm_iterations.assign(K, 0);
    backend::check(svgpu_reloc_refine_batch(backend::context(), &cam, P.tdesc.data(), P.t_xy.data(), P.t_octave.data(), P.t_angle.data(),
                                            P.t_xright.empty() ? nullptr : P.t_xright.data(), P.nt, (int)frm.frm_obs_.num_grid_cols_, (int)frm.frm_obs_.num_grid_rows_,
                                            (int)orb->num_levels_, orb->scale_factors_.data(), orb->inv_level_sigma_sq_.data(), orb->log_scale_factor_, intr,
                                            (int)num_trials_robust_, (int)num_trials_, (int)num_each_iter_, reset_stop_flag_each_round_, check_orientation_ ? 1 : 0,
                                            P.K, nullptr, P.pose_cw.data(), P.n_already_found.data(), P.frame_has_lm.data(), P.frame_lm_pos_w.data(),
                                            P.kf_off.data(), P.pos_w.data(), P.valid.data(), P.min_valid_dist.data(), P.max_valid_dist.data(), P.lm_desc.data(),
                                            P.angle_kf.data(), (int)S, margins_.data(), hamm_dist_thrs_.data(), (int)min_num_valid_obs_, R.status.data(),
                                            R.pose_out.data(), R.match_kf.data(), R.match_stage.data(), R.outlier.data(), R.num_found.data(), R.num_valid.data(),
                                            R.lm_iterations.data(), &last_stats_),
                   "svgpu_reloc_refine_batch");
    return scatter(P, R, (int)S, candidate_keyfrms, landmarks_per_candidate);
}

}  // namespace hip
}  // namespace module
}  // namespace stella_vslam
