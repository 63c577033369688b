// stella_vslam::solve::hip::pnp_solver -- solve/pnp_solver.h:13-137 with the reference's constructor and public methods, backed by
// svgpu_pnp_ransac[_batch] (include/svgpu.h), plus the batch form module::relocalizer::relocalize_by_pnp_solver (module/relocalizer.cc:134-209)
// and module::loop_detector (module/loop_detector.cc:423-446) should call: every candidate keyframe's solver in one device call.
// The RANSAC samples are drawn here, on the host, with the engine and the procedure of util::create_random_engine /
// util::create_random_array (util/random_array.cc:12-63): use_fixed_seed means what it means in the reference.
#pragma once
#include <random>

#include "hip_backend.h"

namespace stella_vslam {
namespace solve {
namespace hip {

class pnp_solver {
public:
    pnp_solver(const eigen_alloc_vector<Vec3_t>& valid_bearings, const std::vector<int>& octaves, const eigen_alloc_vector<Vec3_t>& valid_points,
               const std::vector<float>& scale_factors, unsigned int min_num_inliers = 10, bool use_fixed_seed = false,
               unsigned int gauss_newton_num_iter = 10);
    virtual ~pnp_solver() = default;

    //! Find the most reliable camera pose via RANSAC (one device call)
    void find_via_ransac(const unsigned int max_num_iter, const bool recompute = true);
    //! The same for every solver of the list in ONE device call; each solver ends in the state its own find_via_ransac would leave
    static void find_via_ransac_batch(const std::vector<pnp_solver*>& solvers, const unsigned int max_num_iter, const bool recompute = true);

    bool solution_is_valid() const { return solution_is_valid_; }
    Mat33_t get_best_rotation() const { return best_rot_cw_; }
    Vec3_t get_best_translation() const { return best_trans_cw_; }
    Mat44_t get_best_cam_pose() const;
    std::vector<bool> get_inlier_flags() const { return is_inlier_match; }
    //! the winning RANSAC iteration of the last call, -1 when the solution is invalid
    int best_iter_ = -1;

    //! the sample table of max_num_iter iterations, 4 indices each, drawn as util::create_random_array(4, 0U, num_matches_ - 1, random_engine_)
    //! draws them (:73); advances the engine (public for the test that pins the sequence against the reference's)
    std::vector<uint32_t> draw(const unsigned int max_num_iter);

private:
    const unsigned int num_matches_;
    std::vector<double> bearings_, points_;
    std::vector<int32_t> octaves_;
    std::vector<float> scale_factors_;
    const unsigned int min_num_inliers_;
    std::mt19937 random_engine_;
    const unsigned int gauss_newton_num_iter_;
    bool solution_is_valid_ = false;
    Mat33_t best_rot_cw_;
    Vec3_t best_trans_cw_;
    std::vector<bool> is_inlier_match;
};

}  // namespace hip
}  // namespace solve
}  // namespace stella_vslam
