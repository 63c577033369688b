// stella_vslam::module::hip::landmark_fuser -- mapping_module::fuse_landmark_duplication (mapping_module.cc:417-537) for all fuse targets of
// the current keyframe.  From `min_targets_for_batch_` targets on: the union of the landmarks is flattened once, svgpu_fuse_landmarks_batch
// (include/svgpu.h) runs the forward loop and the backward pass on the device, and the returned events are replayed on the object graph
// (replace, connect_to_keyframe, then the two batch setters).  Below that, and when the call reports SVGPU_FUSE_OVERFLOW or the map holds
// something the flat table does not express, the class runs its own chain of single match::hip::fuse calls.
// The backward candidates are taken in first appearance (target order, then keypoint order) on both paths: the reference iterates an
// unordered_set there, and the greedy claims make the order matter.
#pragma once
#include "hip_backend.h"

namespace stella_vslam {
namespace module {
namespace hip {

class landmark_fuser {
public:
    using lm_ptr = std::shared_ptr<data::landmark>;
    using kf_ptr = std::shared_ptr<data::keyframe>;
    explicit landmark_fuser(float margin = 3.0f, bool do_reprojection_matching = true) : margin_(margin), do_reprojection_matching_(do_reprojection_matching) {}

    //! replaced_lms is filled for tracker_->replace_landmarks_in_last_frm (mapping_module.cc:389-391)
    void fuse(const kf_ptr& cur_keyfrm, const std::vector<kf_ptr>& fuse_tgt_keyfrms, data::map_database* map_db, std::unordered_map<lm_ptr, lm_ptr>& replaced_lms) const;

    //! the chain of single calls alone (what fuse() falls back to)
    void fuse_by_single_calls(const kf_ptr& cur_keyfrm, const std::vector<kf_ptr>& fuse_tgt_keyfrms, data::map_database* map_db,
                              std::unordered_map<lm_ptr, lm_ptr>& replaced_lms) const;

    //! The smallest number of targets at which fuse() takes the one batch call.  1: the batch call was ahead of the single calls at every
    //! measured K, one target included.
    unsigned int min_targets_for_batch_ = 1;
    //! extra slack per observation list beyond fuse_obs_capacity (tests lower it to meet the overflow fallback)
    int obs_slack_ = 0;
    mutable bool last_took_batch_ = false, last_overflowed_ = false;
    mutable svgpu_call_stats last_stats_{0, 0, 0};

private:
    bool fuse_batch(const kf_ptr& cur_keyfrm, const std::vector<kf_ptr>& fuse_tgt_keyfrms, data::map_database* map_db,
                    std::unordered_map<lm_ptr, lm_ptr>& replaced_lms) const;
    const float margin_;
    const bool do_reprojection_matching_;
};

}  // namespace hip
}  // namespace module
}  // namespace stella_vslam
