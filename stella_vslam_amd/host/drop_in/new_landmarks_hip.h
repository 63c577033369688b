// stella_vslam::module::hip::new_landmark_creator -- the loop of mapping_module::create_new_landmarks (mapping_module.cc:286-340) for all
// covisible neighbours of the current keyframe: per neighbour match_for_triangulation, then two_view_triangulator::triangulate, where a
// keypoint that got a landmark at one neighbour is no query for the next.  One device call (svgpu_new_landmarks_batch, include/svgpu.h)
// from `min_neighbours_for_batch` neighbours on, the chain of single calls with the landmark state updated on the host below that.
// Creating the landmark objects, the refresh and local_map_cleaner stay with the caller (triangulate_with_two_keyframes, :343-375).
#pragma once
#include "hip_backend.h"
#include "two_view_triangulator_hip.h"

namespace stella_vslam {
namespace module {
namespace hip {

class new_landmark_creator {
public:
    //! an accepted triangulation: what triangulate_with_two_keyframes turns into a landmark
    struct seed {
        unsigned int idx_1, idx_2;  // keypoint of the current keyframe, keypoint of the neighbour
        Vec3_t pos_w;
    };
    //! use_bow_tree: bow_tree::match_for_triangulation (mapping_module.cc:332) instead of robust's (:335)
    new_landmark_creator(float lowe_ratio, bool check_orientation, bool use_bow_tree, float rays_parallax_deg_thr = 1.0f)
        : lowe_ratio_(lowe_ratio), check_orientation_(check_orientation), use_bow_tree_(use_bow_tree), rays_parallax_deg_thr_(rays_parallax_deg_thr) {}

    //! Per neighbour the accepted (idx_1, idx_2, pos_w) in idx_1 order.  active[k] == false: the baseline `continue` of :303-319, which the
    //! caller decides; an empty `active` means all.
    std::vector<std::vector<seed>> create(const std::shared_ptr<data::keyframe>& cur_keyfrm, const std::vector<std::shared_ptr<data::keyframe>>& neighbours,
                                          const std::vector<bool>& active, float residual_rad_thr) const;

    //! (cur bearing)^T E (ngh bearing) = 0 from the two poses, as solve::essential_solver::create_E_21(ngh, cur) forms it (:323-324)
    static Mat33_t essential(const std::shared_ptr<data::keyframe>& cur_keyfrm, const std::shared_ptr<data::keyframe>& ngh_keyfrm);

    //! the neighbour whose match gave keypoint i of the current keyframe its landmark in the last create(), or -1
    mutable std::vector<int32_t> created_by_;
    //! what the last create() issued when it took the batch call (zeros otherwise)
    mutable svgpu_call_stats last_stats_{0, 0, 0};
    //! The smallest number of neighbours at which create() takes the one batch call; fewer run as single calls.  1: the batch call was ahead
    //! of the single calls at every measured K, a batch of one included.
    unsigned int min_neighbours_for_batch_ = 1;

private:
    const float lowe_ratio_;
    const bool check_orientation_, use_bow_tree_;
    const float rays_parallax_deg_thr_;
};

}  // namespace hip
}  // namespace module
}  // namespace stella_vslam
