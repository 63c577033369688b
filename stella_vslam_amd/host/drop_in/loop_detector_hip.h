// module::hip::loop_sim3_validator -- the middle of loop_detector::select_loop_candidate_via_Sim3 (module/loop_detector.cc:537-587) for ALL
// candidates that survived the pose refinement, in one svgpu_loop_sim3_batch call: the scale from the small-parallax landmark pairs
// (:540-573), projection::match_keyframes_mutually (:577), transform_optimizer::optimize (:581) and the threshold of :585.  The class
// flattens the current keyframe once and every candidate (keypoints, landmark slots, the prior matches
// curr_match_lms_observed_in_cand), computes rot_12 / trans_12 as :570-571 do, makes the call, and writes every candidate's
// curr_match_lms_observed_in_cand back as the two per-candidate calls leave it: the new mutual matches set (projection.cc:623), the
// entries of rejected edges cleared (transform_optimizer.cc:115, :146).  It returns the first accepted candidate in candidate order;
// candidates are independent, so this is the answer of the reference's loop.
// Compiles against the reference tree with -DSVGPU_WITH_STELLA_VSLAM, or against host/standin/stella_standin.h.
#pragma once
#include <cstdint>
#include <memory>
#include <vector>

#include "hip_backend.h"

namespace stella_vslam {
namespace module {
namespace hip {

class loop_sim3_validator {
public:
    using lm_ptr = std::shared_ptr<data::landmark>;
    using kf_ptr = std::shared_ptr<data::keyframe>;

    //! what the stretch :537-587 leaves behind for one candidate
    struct candidate_result {
        int status = 0;          //!< svgpu_loop_sim3_batch: 0 accepted, SVGPU_LOOP_NO_SCALE, SVGPU_LOOP_FEW_INLIERS, -1 not offered
        float scale_12 = 0.f;    //!< :573 (0 where there was no ratio)
        Mat33_t rot_12;          //!< :570
        Vec3_t trans_12;         //!< :571
        ::g2o::Sim3 g2o_sim3_12; //!< :580 before, and what optimize leaves in it (:581)
        unsigned int num_mutual = 0, num_optimized_inliers = 0;
        svgpu_sim3opt_stats stats{};
    };

    //! fix_scale / num_iter: the loop detector's transform_optimizer (module/loop_detector.cc:23); num_optimized_inliers_thr: :585
    loop_sim3_validator(bool fix_scale, unsigned int num_optimized_inliers_thr, unsigned int num_iter = 10, float margin = 7.5f, float chi_sq = 10.0f);

    //! candidates[c] with poses_1w_in_cand[c] (optimized_pose2, :537) and matched_lms_per_candidate[c] (curr_match_lms_observed_in_cand, one
    //! entry per keypoint of cur_keyfrm).  Returns the index of the first accepted candidate, or -1; results[c] and the written-back
    //! matched_lms_per_candidate[c] are filled for every candidate.  scales_12_in (nullable): the scale per candidate instead of the estimate.
    int validate_batch(const kf_ptr& cur_keyfrm, const std::vector<kf_ptr>& candidates, const std::vector<Mat44_t>& poses_1w_in_cand,
                       std::vector<std::vector<lm_ptr>>& matched_lms_per_candidate, std::vector<candidate_result>& results,
                       const std::vector<float>* scales_12_in = nullptr) const;

    //! :570-571: rot_12 = rot_1w_in_cand * rot_2w^T, trans_12 = -rot_12 * trans_2w + trans_1w_in_cand
    static void relative_pose(const Mat44_t& pose_1w_in_cand, const kf_ptr& candidate, Mat33_t& rot_12, Vec3_t& trans_12);
    //! :580: g2o::Sim3(rot_12, trans_12, scale_12), the rotation as a unit quaternion (Eigen's conversion)
    static ::g2o::Sim3 initial_sim3(const Mat33_t& rot_12, const Vec3_t& trans_12, double scale_12);

    mutable svgpu_call_stats last_stats_{0, 0, 0};

private:
    const bool fix_scale_;
    const unsigned int num_optimized_inliers_thr_, num_iter_;
    const float margin_, chi_sq_;
};

}  // namespace hip
}  // namespace module
}  // namespace stella_vslam
