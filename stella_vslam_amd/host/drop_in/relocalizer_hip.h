// module::hip::relocalizer -- relocalizer::refine_pose (module/relocalizer.cc:236-297) for ALL candidates that survived optimize_pose, in
// one svgpu_reloc_refine_batch call.  The class does the two host halves around the call: `gather` flattens the frame, every candidate
// keyframe's landmarks (the `valid` rule of projection.cc:209-232: not null, not will_be_erased, not in already_found_landmarks) and the
// frame's landmark assignment per candidate; `scatter` maps entry and keypoint indices back to shared_ptrs and leaves, per candidate, the
// landmark vector refine_pose would leave on the frame: the matched landmarks added (projection.cc:313), and -- for an accepted candidate
// -- the last optimisation's outliers dropped (relocalizer.cc:288-295).  A rejected candidate keeps the matches made up to its rejection,
// as the reference's frame does.
// One difference from the reference's text: its second match offers again a member of already_found_landmarks that optimize_pose's
// outlier rejection took off the frame (:258-267 rebuilds the set from the frame); here an entry that is not offered to the first
// stage is offered to none (the array semantics of svgpu_reloc_refine_batch).
// Compiles against the reference tree with -DSVGPU_WITH_STELLA_VSLAM, or against host/standin/stella_standin.h.
#pragma once
#ifdef SVGPU_WITH_STELLA_VSLAM
#include "stella_vslam/camera/base.h"
#include "stella_vslam/data/frame.h"
#include "stella_vslam/data/keyframe.h"
#include "stella_vslam/data/landmark.h"
#include "stella_vslam/feature/orb_params.h"
#else
#include "standin/stella_standin.h"
#endif
#include <cstdint>
#include <memory>
#include <set>
#include <vector>

#include "svgpu.h"

namespace stella_vslam {
namespace module {
namespace hip {

class relocalizer {
public:
    using lm_ptr = std::shared_ptr<data::landmark>;
    using kf_ptr = std::shared_ptr<data::keyframe>;

    //! what refine_pose leaves behind for one candidate
    struct candidate_result {
        bool accepted = false;
        int status = 0;  //!< svgpu_reloc_refine_batch: 0 accepted, 1 + s failed the count test of stage s, 1 + stages the final test
        Mat44_t pose_cw;
        std::vector<lm_ptr> landmarks;  //!< per frame keypoint
        std::vector<unsigned int> num_found, num_valid;  //!< per stage
    };
    //! the flat arrays of the call (include/svgpu.h names them)
    struct flat_problem {
        int nt = 0, K = 0;
        std::vector<uint8_t> tdesc, frame_has_lm, valid, lm_desc;
        std::vector<float> t_xy, t_angle, t_xright, min_valid_dist, max_valid_dist, angle_kf;
        std::vector<int32_t> t_octave, n_already_found, kf_off;
        std::vector<double> pose_cw, frame_lm_pos_w, pos_w;
    };
    struct flat_result {
        std::vector<int32_t> status, match_kf, match_stage, num_found, num_valid, lm_iterations;
        std::vector<double> pose_out;
        std::vector<uint8_t> outlier;
    };

    explicit relocalizer(unsigned int min_num_valid_obs = 50, bool check_orientation = true, unsigned int num_trials_robust = 2, unsigned int num_trials = 2,
                         unsigned int num_each_iter = 10);

    //! refine_pose for candidate c = (candidate_keyfrms[c], poses_cw[c], landmarks_per_candidate[c], already_found_landmarks[c]): the pose and the
    //! frame's landmark assignment after optimize_pose (outliers already erased), and the set relocalize_by_pnp_solver found.
    std::vector<candidate_result> refine_pose_batch(const data::frame& frm, const std::vector<kf_ptr>& candidate_keyfrms, const std::vector<Mat44_t>& poses_cw,
                                                    const std::vector<std::vector<lm_ptr>>& landmarks_per_candidate,
                                                    const std::vector<std::set<lm_ptr>>& already_found_landmarks) const;

    //! the host halves (no device is touched)
    static flat_problem gather(const data::frame_observation& frm_obs, const std::vector<kf_ptr>& candidate_keyfrms, const std::vector<Mat44_t>& poses_cw,
                               const std::vector<std::vector<lm_ptr>>& landmarks_per_candidate, const std::vector<std::set<lm_ptr>>& already_found_landmarks);
    static std::vector<candidate_result> scatter(const flat_problem& P, const flat_result& R, int num_stages, const std::vector<kf_ptr>& candidate_keyfrms,
                                                 const std::vector<std::vector<lm_ptr>>& landmarks_per_candidate);

    //! the stages of relocalizer.cc:244 and :267
    std::vector<float> margins_{10.0f, 3.0f};
    std::vector<int32_t> hamm_dist_thrs_{100, 64};
    int reset_stop_flag_each_round_ = 0;
    mutable svgpu_call_stats last_stats_{0, 0, 0};

private:
    const unsigned int min_num_valid_obs_;
    const bool check_orientation_;
    const unsigned int num_trials_robust_, num_trials_, num_each_iter_;
};

}  // namespace hip
}  // namespace module
}  // namespace stella_vslam
