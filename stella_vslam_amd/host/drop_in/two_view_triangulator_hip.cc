#include "two_view_triangulator_hip.h"

namespace stella_vslam {
namespace module {
namespace hip {

// what two_view_triangulator::triangulate reads of a keyframe (module/two_view_triangulator.cc:8-31, 76-90)
two_view_triangulator::side two_view_triangulator::flatten(const std::shared_ptr<data::keyframe>& keyfrm) {
    two_view_triangulator::side s;
    s.cam = stella_vslam::hip::to_svgpu_camera(keyfrm->camera_);
    const Mat44_t pose_cw = keyfrm->get_pose_cw();
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) s.pose_cw[4 * r + c] = pose_cw(r, c);
    s.true_baseline = keyfrm->camera_->true_baseline_;
    const auto& obs = keyfrm->frm_obs_;
    s.n = (int)obs.undist_keypts_.size();
    s.xy.resize(2 * (size_t)s.n);
    s.octave.resize(s.n);
    s.bearings.resize(3 * (size_t)s.n);
    for (int i = 0; i < s.n; ++i) {
        s.xy[2 * i] = obs.undist_keypts_[i].pt.x;
        s.xy[2 * i + 1] = obs.undist_keypts_[i].pt.y;
        s.octave[i] = obs.undist_keypts_[i].octave;
        for (int j = 0; j < 3; ++j) s.bearings[3 * i + j] = obs.bearings_[i](j);
    }
    s.xright = obs.stereo_x_right_;
    s.depth = obs.depths_;
    s.scale_factor = keyfrm->orb_params_->scale_factor_;
    return s;
}
namespace {
const float* or_null(const std::vector<float>& v) { return v.empty() ? nullptr : v.data(); }
}  // namespace

two_view_triangulator::two_view_triangulator(const std::shared_ptr<data::keyframe>& keyfrm_1, const std::shared_ptr<data::keyframe>& keyfrm_2,
                                             const float rays_parallax_deg_thr)
    : keyfrm_1_(keyfrm_1), keyfrm_2_(keyfrm_2), rays_parallax_deg_thr_(rays_parallax_deg_thr), s1_(flatten(keyfrm_1)), s2_(flatten(keyfrm_2)) {}

void two_view_triangulator::triangulate(const std::vector<std::pair<unsigned int, unsigned int>>& matches, eigen_alloc_vector<Vec3_t>& pos_w,
                                        std::vector<bool>& ok) const {
    run(matches, pos_w, ok, last_status_);
}

void two_view_triangulator::run(const std::vector<std::pair<unsigned int, unsigned int>>& matches, eigen_alloc_vector<Vec3_t>& pos_w, std::vector<bool>& ok,
                                std::vector<uint8_t>& status) const {
    const int m = (int)matches.size();
    std::vector<int32_t> idx1(m), idx2(m);
    for (int i = 0; i < m; ++i) idx1[i] = (int32_t)matches[i].first, idx2[i] = (int32_t)matches[i].second;
    std::vector<double> pos(3 * (size_t)m);
    status.assign(m, 0);
    int num = 0;
    // both keyframes' tables are those of keyframe 1's orb_params (one ORB configuration per system: system.cc:95-108)
    const auto* op = keyfrm_1_->orb_params_;
    stella_vslam::hip::check(
        svgpu_triangulate_two_views(stella_vslam::hip::context(), &s1_.cam, s1_.pose_cw, s1_.true_baseline, s1_.xy.data(), s1_.octave.data(), s1_.bearings.data(),
                                    or_null(s1_.xright), or_null(s1_.depth), s1_.n, &s2_.cam, s2_.pose_cw, s2_.true_baseline, s2_.xy.data(), s2_.octave.data(),
                                    s2_.bearings.data(), or_null(s2_.xright), or_null(s2_.depth), s2_.n, op->scale_factors_.data(), op->level_sigma_sq_.data(),
                                    (int)op->scale_factors_.size(), s1_.scale_factor, s2_.scale_factor, rays_parallax_deg_thr_, idx1.data(), idx2.data(), m,
                                    pos.data(), status.data(), &num),
        "svgpu_triangulate_two_views");
    pos_w.resize(m);
    ok.assign(m, false);
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < 3; ++j) pos_w[i](j) = pos[3 * (size_t)i + j];
        ok[i] = status[i] == SVGPU_TRI_ACCEPTED;
    }
}

bool two_view_triangulator::triangulate(const unsigned idx_1, const unsigned int idx_2, Vec3_t& pos_w) const {
    eigen_alloc_vector<Vec3_t> p;
    std::vector<bool> ok;
    std::vector<uint8_t> status;
    run(std::vector<std::pair<unsigned int, unsigned int>>{{idx_1, idx_2}}, p, ok, status);
    pos_w = p[0];
    return ok[0];
}

}  // namespace hip
}  // namespace module
}  // namespace stella_vslam
