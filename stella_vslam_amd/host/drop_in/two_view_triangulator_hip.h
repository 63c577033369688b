// stella_vslam::module::hip::two_view_triangulator -- module/two_view_triangulator.h:20-81 with the reference's constructor and
// triangulate(idx_1, idx_2, pos_w), backed by svgpu_triangulate_two_views (include/svgpu.h), plus the batch form that
// mapping_module::triangulate_with_two_keyframes (mapping_module.cc:343-375) should call: one device call for all matches of a keyframe pair.
#pragma once
#include "hip_backend.h"

namespace stella_vslam {
namespace module {
namespace hip {

class two_view_triangulator {
public:
    explicit two_view_triangulator(const std::shared_ptr<data::keyframe>& keyfrm_1, const std::shared_ptr<data::keyframe>& keyfrm_2,
                                   const float rays_parallax_deg_thr = 1.0);
    ~two_view_triangulator() = default;

    //! Triangulate a landmark between the keypoint idx_1 of keyfrm_1 and the keypoint idx_2 of keyfrm_2 (one device call per match: the
    //! reference's signature, kept for callers that hold a single pair; a loop over matches belongs to the batch form)
    bool triangulate(const unsigned idx_1, const unsigned int idx_2, Vec3_t& pos_w) const;
    //! All matches of the keyframe pair in one device call: pos_w[i] / ok[i] are what triangulate(matches[i].first, matches[i].second, .) gives
    void triangulate(const std::vector<std::pair<unsigned int, unsigned int>>& matches, eigen_alloc_vector<Vec3_t>& pos_w, std::vector<bool>& ok) const;
    //! the status byte of every match of the last batch call (SVGPU_TRI_*: which gate rejected it)
    mutable std::vector<uint8_t> last_status_;

    //! the flattened side of a keyframe, as the C ABI takes it (public for tests that call the ABI on the same arrays)
    struct side {
        svgpu_camera cam;
        double pose_cw[12];
        double true_baseline;
        std::vector<float> xy, xright, depth;
        std::vector<int32_t> octave;
        std::vector<double> bearings;
        float scale_factor;
        int n;
    };
    //! what triangulate reads of one keyframe (also used by new_landmark_creator, which flattens every keyframe once)
    static side flatten(const std::shared_ptr<data::keyframe>& keyfrm);
    const side& side_1() const { return s1_; }
    const side& side_2() const { return s2_; }

private:
    void run(const std::vector<std::pair<unsigned int, unsigned int>>& matches, eigen_alloc_vector<Vec3_t>& pos_w, std::vector<bool>& ok,
             std::vector<uint8_t>& status) const;
    const std::shared_ptr<data::keyframe> keyfrm_1_, keyfrm_2_;
    const float rays_parallax_deg_thr_;
    side s1_, s2_;
};

}  // namespace hip
}  // namespace module
}  // namespace stella_vslam
