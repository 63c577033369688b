// stella_vslam::optimize::hip::transform_optimizer: optimize/transform_optimizer.h:18-51 with the reference's constructor and `optimize`
// signature, on the device (svgpu_sim3_transform_optimize_batch, include/svgpu.h).  The match filter of transform_optimizer.cc:64-94 runs
// on the host, the two-stage optimisation and both chi2 gates on the device, and the write-back sets the rejected entries of
// matched_lms_in_keyfrm_2 to null (:115, :146).  optimize_batch serves one current keyframe against several candidates in one launch,
// as module::loop_detector meets them (module/loop_detector.cc:581).
#pragma once
#include <memory>
#include <vector>

#include "hip_backend.h"

namespace stella_vslam {
namespace optimize {
namespace hip {

class transform_optimizer {
public:
    //! Constructor (optimize/transform_optimizer.h:25)
    explicit transform_optimizer(const bool fix_scale, const unsigned int num_iter = 10);
    virtual ~transform_optimizer() = default;

    //! Perform optimization (optimize/transform_optimizer.h:41-43): the batch of one
    unsigned int optimize(const std::shared_ptr<data::keyframe>& keyfrm_1, const std::shared_ptr<data::keyframe>& keyfrm_2,
                          std::vector<std::shared_ptr<data::landmark>>& matched_lms_in_keyfrm_2, ::g2o::Sim3& g2o_Sim3_12, const float chi_sq) const;

    //! keyfrm_1 against every candidate in one device call; entry c of the three vectors belongs to candidates[c].  Returns what
    //! optimize would have returned per candidate.
    std::vector<unsigned int> optimize_batch(const std::shared_ptr<data::keyframe>& keyfrm_1, const std::vector<std::shared_ptr<data::keyframe>>& candidates,
                                             std::vector<std::vector<std::shared_ptr<data::landmark>>>& matched_lms_in_candidates,
                                             std::vector<::g2o::Sim3>& g2o_Sim3s_12, const float chi_sq) const;

    //! what the last call's device run reported, per candidate
    mutable std::vector<svgpu_sim3opt_stats> last_stats_;

private:
    //! transform is Sim3 or SE3
    const bool fix_scale_;
    //! number of iterations of optimization
    const unsigned int num_iter_;
};

}  // namespace hip
}  // namespace optimize
}  // namespace stella_vslam
