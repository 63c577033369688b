#include "drop_in/transform_optimizer_hip.h"

#include <cstdint>

namespace stella_vslam {
namespace optimize {
namespace hip {

namespace {
svgpu_sim3opt_view view_of(const std::shared_ptr<data::keyframe>& keyfrm) {
    svgpu_sim3opt_view v{};
    v.cam = stella_vslam::hip::to_svgpu_camera(keyfrm->camera_);
    const Mat33_t rot_cw = keyfrm->get_rot_cw();
    const Vec3_t trans_cw = keyfrm->get_trans_cw();
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) v.pose_cw[4 * i + j] = rot_cw(i, j);
        v.pose_cw[4 * i + 3] = trans_cw(i);
    }
    return v;
}
}  // namespace

transform_optimizer::transform_optimizer(const bool fix_scale, const unsigned int num_iter) : fix_scale_(fix_scale), num_iter_(num_iter) {}

unsigned int transform_optimizer::optimize(const std::shared_ptr<data::keyframe>& keyfrm_1, const std::shared_ptr<data::keyframe>& keyfrm_2,
                                           std::vector<std::shared_ptr<data::landmark>>& matched_lms_in_keyfrm_2, ::g2o::Sim3& g2o_Sim3_12,
                                           const float chi_sq) const {
    // a copy of the list: if the device call throws, the caller's vector and Sim3 are left as they came
    std::vector<std::vector<std::shared_ptr<data::landmark>>> matched{matched_lms_in_keyfrm_2};
    std::vector<::g2o::Sim3> sim3s{g2o_Sim3_12};
    const auto num_inliers = optimize_batch(keyfrm_1, {keyfrm_2}, matched, sim3s, chi_sq);
    matched_lms_in_keyfrm_2.swap(matched[0]);
    g2o_Sim3_12 = sim3s[0];
    return num_inliers[0];
}

std::vector<unsigned int> transform_optimizer::optimize_batch(const std::shared_ptr<data::keyframe>& keyfrm_1,
                                                              const std::vector<std::shared_ptr<data::keyframe>>& candidates,
                                                              std::vector<std::vector<std::shared_ptr<data::landmark>>>& matched_lms_in_candidates,
                                                              std::vector<::g2o::Sim3>& g2o_Sim3s_12, const float chi_sq) const {
    const int P = (int)candidates.size();
    std::vector<unsigned int> result(P, 0);
    last_stats_.assign(P, svgpu_sim3opt_stats{});
    if (P == 0) return result;
    const svgpu_sim3opt_view view1 = view_of(keyfrm_1);
    std::vector<svgpu_sim3opt_view> view2(P);
    std::vector<int32_t> match_off(P + 1, 0);
    std::vector<unsigned int> idx1_of;  // per valid match: its index in matched_lms_in_keyfrm_2
    std::vector<double> obs1, obs2, pos1, pos2, sim3(8 * (size_t)P);
    std::vector<float> w1, w2;
    // all the 3D points observed in keyframe 1
    const auto lms_in_keyfrm_1 = keyfrm_1->get_landmarks();
    for (int c = 0; c < P; ++c) {
        const auto& keyfrm_2 = candidates[c];
        view2[c] = view_of(keyfrm_2);
        const auto& matched = matched_lms_in_candidates.at(c);
        // the filter of transform_optimizer.cc:64-94, in ascending idx1 order
        for (unsigned int idx1 = 0; idx1 < matched.size(); ++idx1) {
            if (!matched.at(idx1)) continue;
            const auto& lm_1 = lms_in_keyfrm_1.at(idx1);
            const auto& lm_2 = matched.at(idx1);
            if (!lm_1 || !lm_2) continue;
            if (lm_1->will_be_erased() || lm_2->will_be_erased()) continue;
            const auto idx2 = lm_2->get_index_in_keyframe(keyfrm_2);
            if (idx2 < 0) continue;
            // the edges' data (mutual_reproj_edge_wrapper.h:71-77, :178-184)
            const auto& undist_keypt_1 = keyfrm_1->frm_obs_.undist_keypts_.at(idx1);
            const auto& undist_keypt_2 = keyfrm_2->frm_obs_.undist_keypts_.at(idx2);
            obs1.push_back(undist_keypt_1.pt.x), obs1.push_back(undist_keypt_1.pt.y);
            obs2.push_back(undist_keypt_2.pt.x), obs2.push_back(undist_keypt_2.pt.y);
            w1.push_back(keyfrm_1->orb_params_->inv_level_sigma_sq_.at(undist_keypt_1.octave));
            w2.push_back(keyfrm_2->orb_params_->inv_level_sigma_sq_.at(undist_keypt_2.octave));
            const Vec3_t p1 = lm_1->get_pos_in_world(), p2 = lm_2->get_pos_in_world();
            for (int k = 0; k < 3; ++k) pos1.push_back(p1(k)), pos2.push_back(p2(k));
            idx1_of.push_back(idx1);
        }
        match_off[c + 1] = (int32_t)idx1_of.size();
        const ::g2o::Sim3& S = g2o_Sim3s_12.at(c);
        double* s8 = sim3.data() + 8 * (size_t)c;
        for (int k = 0; k < 4; ++k) s8[k] = S.q[k];
        for (int k = 0; k < 3; ++k) s8[4 + k] = S.t[k];
        s8[7] = S.s;
    }
    const size_t n = idx1_of.size();
    std::vector<double> sim3_out(8 * (size_t)P);
    std::vector<int32_t> num_inliers(P, 0);
    std::vector<uint8_t> status(n ? n : 1, 0);
    svgpu_ctx* ctx = stella_vslam::hip::context();
    stella_vslam::hip::check(svgpu_sim3_transform_optimize_batch(ctx, P, &view1, 1, view2.data(), match_off.data(), obs1.data(), obs2.data(), w1.data(), w2.data(),
                                                                 pos1.data(), pos2.data(), sim3.data(), chi_sq, fix_scale_ ? 1 : 0, (int)num_iter_, sim3_out.data(),
                                                                 num_inliers.data(), status.data(), last_stats_.data()),
                             "svgpu_sim3_transform_optimize_batch");
    for (int c = 0; c < P; ++c) {
        // outlier rejection (:115, :146): also when the call returns 0 before its step 7, as the reference leaves the vector
        for (int32_t m = match_off[c]; m < match_off[c + 1]; ++m)
            if (status[m] != SVGPU_SIM3OPT_INLIER) matched_lms_in_candidates[c].at(idx1_of[m]) = nullptr;
        result[c] = (unsigned int)num_inliers[c];
        if (last_stats_[c].early_return) continue;  // :121-123: g2o_Sim3_12 is not written
        g2o_Sim3s_12[c] = ::g2o::Sim3(sim3_out.data() + 8 * (size_t)c);
    }
    return result;
}

}  // namespace hip
}  // namespace optimize
}  // namespace stella_vslam
