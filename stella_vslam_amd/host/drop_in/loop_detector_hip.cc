#include "drop_in/loop_detector_hip.h"

#include <cmath>
#include <cstring>

#include "sv_sim3.h"

namespace stella_vslam {
namespace module {
namespace hip {

namespace {
using lm_ptr = std::shared_ptr<data::landmark>;
using kf_ptr = std::shared_ptr<data::keyframe>;

// one keyframe as the call takes it: its keypoints, and one landmark slot per keypoint
struct flat_keyframe {
    int n = 0;
    std::vector<uint8_t> desc, lm_desc, has_lm;
    std::vector<float> xy, min_d, max_d;
    std::vector<int32_t> octave;
    std::vector<double> pos_w;
};
void append(flat_keyframe& F, const kf_ptr& keyfrm) {
    const auto& o = keyfrm->frm_obs_;
    const auto lms = keyfrm->get_landmarks();
    const int n = (int)o.undist_keypts_.size();
    const size_t at = (size_t)F.n;
    F.n += n;
    F.desc.resize((size_t)F.n * 32, 0), F.lm_desc.resize((size_t)F.n * 32, 0), F.has_lm.resize(F.n, 0);
    F.xy.resize((size_t)F.n * 2, 0.f), F.min_d.resize(F.n, 0.f), F.max_d.resize(F.n, 0.f), F.octave.resize(F.n, 0), F.pos_w.resize((size_t)F.n * 3, 0.0);
    for (int i = 0; i < n; ++i) {
        const size_t g = at + (size_t)i;
        std::memcpy(&F.desc[g * 32], o.descriptors_.ptr(i), 32);
        F.xy[2 * g] = o.undist_keypts_[i].pt.x, F.xy[2 * g + 1] = o.undist_keypts_[i].pt.y;
        F.octave[g] = o.undist_keypts_[i].octave;
        const lm_ptr& lm = lms.at(i);
        if (!lm || lm->will_be_erased()) continue;
        const cv::Mat d = lm->get_descriptor();
        if (d.empty()) continue;  // (a landmark without a descriptor is offered to no matcher: hip_backend.cc, flatten)
        F.has_lm[g] = 1;
        std::memcpy(&F.lm_desc[g * 32], d.ptr(0), 32);
        const Vec3_t p = lm->get_pos_in_world();
        for (int k = 0; k < 3; ++k) F.pos_w[3 * g + k] = p(k);
        F.min_d[g] = lm->get_min_valid_distance(), F.max_d[g] = lm->get_max_valid_distance();
    }
}
void pose12(const Mat44_t& T, double* out) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) out[4 * i + j] = T(i, j);
}
}  // namespace

loop_sim3_validator::loop_sim3_validator(bool fix_scale, unsigned int num_optimized_inliers_thr, unsigned int num_iter, float margin, float chi_sq)
    : fix_scale_(fix_scale), num_optimized_inliers_thr_(num_optimized_inliers_thr), num_iter_(num_iter), margin_(margin), chi_sq_(chi_sq) {}

void loop_sim3_validator::relative_pose(const Mat44_t& pose_1w_in_cand, const kf_ptr& candidate, Mat33_t& rot_12, Vec3_t& trans_12) {
    const Mat33_t rot_2w = candidate->get_rot_cw();
    const Vec3_t trans_2w = candidate->get_trans_cw();
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            rot_12(i, j) = (pose_1w_in_cand(i, 0) * rot_2w(j, 0) + pose_1w_in_cand(i, 1) * rot_2w(j, 1)) + pose_1w_in_cand(i, 2) * rot_2w(j, 2);
    for (int i = 0; i < 3; ++i)
        trans_12(i) = (((-rot_12(i, 0)) * trans_2w(0) + (-rot_12(i, 1)) * trans_2w(1)) + (-rot_12(i, 2)) * trans_2w(2)) + pose_1w_in_cand(i, 3);
}

::g2o::Sim3 loop_sim3_validator::initial_sim3(const Mat33_t& rot_12, const Vec3_t& trans_12, double scale_12) {
    const SvMat3 R{rot_12(0, 0), rot_12(0, 1), rot_12(0, 2), rot_12(1, 0), rot_12(1, 1), rot_12(1, 2), rot_12(2, 0), rot_12(2, 1), rot_12(2, 2)};
    double p8[8];
    sv_rot_to_quat(R, p8[0], p8[1], p8[2], p8[3]);
    const double nrm = std::sqrt((p8[0] * p8[0] + p8[1] * p8[1]) + (p8[2] * p8[2] + p8[3] * p8[3]));
    for (int k = 0; k < 4; ++k) p8[k] /= nrm;
    for (int k = 0; k < 3; ++k) p8[4 + k] = trans_12(k);
    p8[7] = scale_12;
    return ::g2o::Sim3(p8);
}

int loop_sim3_validator::validate_batch(const kf_ptr& cur_keyfrm, const std::vector<kf_ptr>& candidates, const std::vector<Mat44_t>& poses_1w_in_cand,
                                        std::vector<std::vector<lm_ptr>>& matched_lms_per_candidate, std::vector<candidate_result>& results,
                                        const std::vector<float>* scales_12_in) const {
    const int K = (int)candidates.size();
    results.assign((size_t)K, candidate_result{});
    last_stats_ = svgpu_call_stats{0, 0, 0};
    if (K == 0) return -1;
    if ((int)poses_1w_in_cand.size() != K || (int)matched_lms_per_candidate.size() != K || (scales_12_in && (int)scales_12_in->size() != K))
        throw std::invalid_argument("loop_sim3_validator::validate_batch: one pose and one match list per candidate");
    flat_keyframe F1, F2;
    append(F1, cur_keyfrm);
    const int n1 = F1.n;
    const auto lms_curr = cur_keyfrm->get_landmarks();
    std::vector<int32_t> kf2_off(1, 0), prior_idx2((size_t)K * n1, -1);
    std::vector<uint8_t> prior_state((size_t)K * n1, 0);
    std::vector<double> pose_1w(12), pose_2w((size_t)K * 12), pose_in_cand((size_t)K * 12), rot_12((size_t)K * 9), trans_12((size_t)K * 3), sim3((size_t)K * 8),
        prior_pos_w((size_t)K * n1 * 3, 0.0);
    std::vector<svgpu_camera> cam2((size_t)K);
    const svgpu_camera cam1 = stella_vslam::hip::to_svgpu_camera(cur_keyfrm->camera_);
    pose12(cur_keyfrm->get_pose_cw(), pose_1w.data());
    for (int c = 0; c < K; ++c) {
        const kf_ptr& cand = candidates[c];
        if ((int)matched_lms_per_candidate[c].size() != n1) throw std::invalid_argument("loop_sim3_validator::validate_batch: one entry per keypoint of the current keyframe");
        append(F2, cand);
        kf2_off.push_back(F2.n);
        const int n2 = kf2_off[c + 1] - kf2_off[c];
        cam2[c] = stella_vslam::hip::to_svgpu_camera(cand->camera_);
        pose12(cand->get_pose_cw(), &pose_2w[12 * (size_t)c]);
        pose12(poses_1w_in_cand[c], &pose_in_cand[12 * (size_t)c]);
        candidate_result& r = results[c];
        relative_pose(poses_1w_in_cand[c], cand, r.rot_12, r.trans_12);
        r.g2o_sim3_12 = initial_sim3(r.rot_12, r.trans_12, 1.0);
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) rot_12[9 * (size_t)c + 3 * i + j] = r.rot_12(i, j);
            trans_12[3 * (size_t)c + i] = r.trans_12(i);
        }
        for (int k = 0; k < 4; ++k) sim3[8 * (size_t)c + k] = r.g2o_sim3_12.q[k];
        for (int k = 0; k < 3; ++k) sim3[8 * (size_t)c + 4 + k] = r.g2o_sim3_12.t[k];
        sim3[8 * (size_t)c + 7] = 1.0;
        for (int i = 0; i < n1; ++i) {  // curr_match_lms_observed_in_cand, flattened
            const lm_ptr& lm = matched_lms_per_candidate[c][i];
            if (!lm) continue;
            const size_t e = (size_t)c * n1 + i;
            prior_state[e] = lm->will_be_erased() ? 2 : 1;
            const int idx2 = lm->get_index_in_keyframe(cand);
            prior_idx2[e] = (0 <= idx2 && idx2 < n2) ? idx2 : -1;
            const Vec3_t p = lm->get_pos_in_world();
            for (int k = 0; k < 3; ++k) prior_pos_w[3 * e + k] = p(k);
        }
    }
    const auto* op = cur_keyfrm->orb_params_;
    const size_t E = (size_t)K * n1, N2 = (size_t)F2.n;
    std::vector<int32_t> status(K), m21(E ? E : 1), m12(N2 ? N2 : 1), mut(E ? E : 1), num_mutual(K), e1(E ? E : 1), e2(E ? E : 1), num_edges(K), num_inliers(K);
    std::vector<float> scale(K);
    std::vector<uint8_t> edge_status(E ? E : 1);
    std::vector<double> sim3_out((size_t)K * 8);
    std::vector<svgpu_sim3opt_stats> ost((size_t)K);
    stella_vslam::hip::check(
        svgpu_loop_sim3_batch(stella_vslam::hip::context(), &cam1, pose_1w.data(), n1, F1.desc.data(), F1.xy.data(), F1.octave.data(), F1.pos_w.data(), F1.has_lm.data(),
                              F1.min_d.data(), F1.max_d.data(), F1.lm_desc.data(), (int)op->num_levels_, op->scale_factors_.data(), op->inv_level_sigma_sq_.data(),
                              op->log_scale_factor_, (int)cur_keyfrm->frm_obs_.num_grid_cols_, (int)cur_keyfrm->frm_obs_.num_grid_rows_, K, cam2.data(), pose_2w.data(),
                              kf2_off.data(), F2.desc.data(), F2.xy.data(), F2.octave.data(), F2.pos_w.data(), F2.has_lm.data(), F2.min_d.data(), F2.max_d.data(),
                              F2.lm_desc.data(), pose_in_cand.data(), rot_12.data(), trans_12.data(), sim3.data(), nullptr, prior_state.data(), prior_idx2.data(),
                              prior_pos_w.data(), scales_12_in ? scales_12_in->data() : nullptr, margin_, chi_sq_, fix_scale_ ? 1 : 0, (int)num_iter_,
                              (int)num_optimized_inliers_thr_, status.data(), scale.data(), m21.data(), m12.data(), mut.data(), num_mutual.data(), e1.data(), e2.data(),
                              num_edges.data(), edge_status.data(), sim3_out.data(), num_inliers.data(), ost.data(), &last_stats_),
        "svgpu_loop_sim3_batch");
    int chosen = -1;
    for (int c = 0; c < K; ++c) {
        candidate_result& r = results[c];
        r.status = status[c], r.scale_12 = scale[c], r.num_mutual = (unsigned)num_mutual[c], r.num_optimized_inliers = (unsigned)num_inliers[c], r.stats = ost[c];
        if (status[c] < 0 || status[c] == SVGPU_LOOP_NO_SCALE) continue;  // :566-569: the candidate's list stays as it came
        const auto landmarks_2 = candidates[c]->get_landmarks();
        auto& matched = matched_lms_per_candidate[c];
        const size_t r0 = (size_t)c * n1;
        for (int i = 0; i < n1; ++i)
            if (0 <= mut[r0 + i]) matched.at(i) = landmarks_2.at(mut[r0 + i]);  // projection.cc:623
        for (int e = 0; e < num_edges[c]; ++e)
            if (edge_status[r0 + e] != SVGPU_SIM3OPT_INLIER) matched.at(e1[r0 + e]) = nullptr;  // transform_optimizer.cc:115, :146
        r.g2o_sim3_12 = ::g2o::Sim3(&sim3_out[8 * (size_t)c]);  // (on the optimiser's early return: the input with the estimated scale, :580)
        if (chosen < 0 && status[c] == 0) chosen = c;
    }
    return chosen;
}

}  // namespace hip
}  // namespace module
}  // namespace stella_vslam
