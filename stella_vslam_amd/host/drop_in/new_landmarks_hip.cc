#include "new_landmarks_hip.h"

#include <cstring>
#include <stdexcept>

namespace stella_vslam {
namespace module {
namespace hip {

namespace {
using kf_ptr = std::shared_ptr<data::keyframe>;
using side = two_view_triangulator::side;

// one keyframe, flattened once: the triangulator's side, and what only the matcher reads
struct flat_keyframe {
    side tri;
    std::vector<uint8_t> desc, no_lm;  // no_lm: 1 = keypoint WITHOUT a landmark (robust.cc:47-50, 66-70)
    std::vector<float> angle;
    std::vector<int32_t> node;         // bow_tree only
    const float* xr() const { return tri.xright.empty() ? nullptr : tri.xright.data(); }
    const float* dp() const { return tri.depth.empty() ? nullptr : tri.depth.data(); }
    svgpu_match_view match_view() const {
        svgpu_match_view v{};
        v.desc = desc.data(), v.angle = angle.data(), v.valid = no_lm.data(), v.node = node.empty() ? nullptr : node.data();
        v.octave = tri.octave.data(), v.bearings = tri.bearings.data(), v.xright = xr(), v.n = tri.n;
        return v;
    }
    svgpu_triangulate_view tri_view() const {  // (names the SAME octave / bearings / xright arrays as match_view)
        return svgpu_triangulate_view{&tri.cam, tri.pose_cw, tri.true_baseline, tri.xy.data(), tri.octave.data(), tri.bearings.data(), xr(), dp(), tri.n,
                                      tri.scale_factor};
    }
};
void flatten(const kf_ptr& kf, bool with_nodes, flat_keyframe& f) {
    f.tri = two_view_triangulator::flatten(kf);
    const int n = f.tri.n;
    const auto& obs = kf->frm_obs_;
    const auto lms = kf->get_landmarks();
    f.desc.resize((size_t)n * 32);
    f.angle.resize(n);
    f.no_lm.resize(n);
    for (int i = 0; i < n; ++i) {
        std::memcpy(&f.desc[(size_t)i * 32], obs.descriptors_.ptr(i), 32);
        f.angle[i] = obs.undist_keypts_[i].angle;
        f.no_lm[i] = lms.at(i) ? 0 : 1;
    }
    if (with_nodes) {
        f.node.assign(std::max(n, 1), -1);  // (an empty side still names its array)
        for (const auto& kv : kf->bow_feat_vec_)
            for (const auto idx : kv.second)
                if ((int)idx < n) f.node[idx] = (int32_t)kv.first;
    }
}
}  // namespace

Mat33_t new_landmark_creator::essential(const kf_ptr& cur_keyfrm, const kf_ptr& ngh_keyfrm) {
    const Mat33_t Rc = cur_keyfrm->get_rot_cw(), Rn = ngh_keyfrm->get_rot_cw();
    const Vec3_t tc = cur_keyfrm->get_trans_cw(), tn = ngh_keyfrm->get_trans_cw();
    double R[3][3], t[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = (Rc(i, 0) * Rn(j, 0) + Rc(i, 1) * Rn(j, 1)) + Rc(i, 2) * Rn(j, 2);  // rot_cur_ngh = rot_cw(cur) rot_cw(ngh)^T
    for (int i = 0; i < 3; ++i) t[i] = ((-R[i][0]) * tn(0) + (-R[i][1]) * tn(1) + (-R[i][2]) * tn(2)) + tc(i);
    const double tx[3][3] = {{0, -t[2], t[1]}, {t[2], 0, -t[0]}, {-t[1], t[0], 0}};
    Mat33_t E;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) E(i, j) = (tx[i][0] * R[0][j] + tx[i][1] * R[1][j]) + tx[i][2] * R[2][j];
    return E;
}

std::vector<std::vector<new_landmark_creator::seed>> new_landmark_creator::create(const kf_ptr& cur_keyfrm, const std::vector<kf_ptr>& neighbours,
                                                                                  const std::vector<bool>& active, const float residual_rad_thr) const {
    const size_t K = neighbours.size();
    if (!active.empty() && active.size() != K) throw std::invalid_argument("new_landmark_creator::create: one active flag per neighbour");
    std::vector<std::vector<seed>> out(K);
    last_stats_ = svgpu_call_stats{0, 0, 0};
    flat_keyframe cur;
    flatten(cur_keyfrm, use_bow_tree_, cur);
    const int n1 = cur.tri.n;
    created_by_.assign(n1, -1);
    if (K == 0) return out;
    svgpu_ctx* ctx = stella_vslam::hip::context();
    // every neighbour once; E_12 and the epipole of the current keyframe in the neighbour (robust.cc:22-27) as match_for_triangulation_batch has them
    std::vector<flat_keyframe> nb(K);
    std::vector<svgpu_match_view> m2(K);
    std::vector<svgpu_triangulate_view> t2(K);
    std::vector<double> E(9 * K), epi(3 * K);
    std::vector<int32_t> valid_epi(K);
    std::vector<uint8_t> act(K);
    const Vec3_t c1v = cur_keyfrm->get_trans_wc();
    const double c1[3] = {c1v(0), c1v(1), c1v(2)};
    for (size_t k = 0; k < K; ++k) {
        flatten(neighbours[k], use_bow_tree_, nb[k]);
        m2[k] = nb[k].match_view(), t2[k] = nb[k].tri_view();
        const Mat33_t R = neighbours[k]->get_rot_cw(), Ek = essential(cur_keyfrm, neighbours[k]);
        const Vec3_t t = neighbours[k]->get_trans_cw();
        double R2[9], tt[3] = {t(0), t(1), t(2)};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R2[3 * i + j] = R(i, j), E[9 * k + 3 * i + j] = Ek(i, j);
        int ve = 0;
        stella_vslam::hip::check(svgpu_reproject_to_bearing(&nb[k].tri.cam, R2, tt, c1, &epi[3 * k], &ve), "svgpu_reproject_to_bearing");
        valid_epi[k] = ve;
        act[k] = active.empty() || active[k] ? 1 : 0;
    }
    const auto* op = cur_keyfrm->orb_params_;  // (one ORB configuration per system: system.cc:95-108)
    const int levels = (int)op->scale_factors_.size();
    std::vector<int32_t> m((size_t)K * n1 + 1, -1), num_m(K, 0), num_a(K, 0);
    std::vector<double> pos((size_t)K * n1 * 3 + 1, 0.0);
    std::vector<uint8_t> status((size_t)K * n1 + 1, SVGPU_TRI_SKIPPED);
    if (K >= min_neighbours_for_batch_) {
        const svgpu_match_view m1 = cur.match_view();
        const svgpu_triangulate_view t1 = cur.tri_view();
        stella_vslam::hip::check(
            svgpu_new_landmarks_batch(ctx, &m1, &t1, (int)K, m2.data(), t2.data(), act.data(), E.data(), epi.data(), valid_epi.data(), op->scale_factors_.data(),
                                      op->level_sigma_sq_.data(), levels, residual_rad_thr, lowe_ratio_, check_orientation_ ? 1 : 0, rays_parallax_deg_thr_,
                                      m.data(), pos.data(), status.data(), num_m.data(), num_a.data(), created_by_.data(), &last_stats_),
            "svgpu_new_landmarks_batch");
    }
    else {  // the chain of single calls: the landmark state of the current keyframe is updated here between the neighbours
        std::vector<uint8_t> has_lm1(n1), has_lm2;
        for (int i = 0; i < n1; ++i) has_lm1[i] = cur.no_lm[i] ? 0 : 1;
        for (size_t k = 0; k < K; ++k) {
            if (!act[k] || n1 == 0) continue;
            const flat_keyframe& f = nb[k];
            has_lm2.resize(f.tri.n);
            for (int i = 0; i < f.tri.n; ++i) has_lm2[i] = f.no_lm[i] ? 0 : 1;
            int32_t* mk = m.data() + k * (size_t)n1;
            int num = 0, acc = 0;
            stella_vslam::hip::check(
                svgpu_match_for_triangulation(ctx, cur.desc.data(), cur.angle.data(), cur.tri.octave.data(), cur.tri.bearings.data(), has_lm1.data(), cur.xr(), n1,
                                              f.desc.data(), f.angle.data(), f.tri.bearings.data(), has_lm2.data(), f.xr(), f.tri.n,
                                              use_bow_tree_ ? cur.node.data() : nullptr, use_bow_tree_ ? f.node.data() : nullptr, &E[9 * k], &epi[3 * k],
                                              valid_epi[k], op->scale_factors_.data(), levels, residual_rad_thr, lowe_ratio_, check_orientation_ ? 1 : 0, mk, &num),
                "svgpu_match_for_triangulation");
            stella_vslam::hip::check(
                svgpu_triangulate_two_views(ctx, &cur.tri.cam, cur.tri.pose_cw, cur.tri.true_baseline, cur.tri.xy.data(), cur.tri.octave.data(),
                                            cur.tri.bearings.data(), cur.xr(), cur.dp(), n1, &f.tri.cam, f.tri.pose_cw, f.tri.true_baseline, f.tri.xy.data(),
                                            f.tri.octave.data(), f.tri.bearings.data(), f.xr(), f.dp(), f.tri.n, op->scale_factors_.data(),
                                            op->level_sigma_sq_.data(), levels, cur.tri.scale_factor, f.tri.scale_factor, rays_parallax_deg_thr_, mk, nullptr, n1,
                                            pos.data() + 3 * k * (size_t)n1, status.data() + k * (size_t)n1, &acc),
                "svgpu_triangulate_two_views");
            for (int i = 0; i < n1; ++i)
                if (status[k * (size_t)n1 + i] == SVGPU_TRI_ACCEPTED) has_lm1[i] = 1, created_by_[i] = (int32_t)k;
        }
    }
    for (size_t k = 0; k < K; ++k)
        for (int i = 0; i < n1; ++i) {
            const size_t o = k * (size_t)n1 + i;
            if (status[o] != SVGPU_TRI_ACCEPTED) continue;
            seed s;
            s.idx_1 = (unsigned)i, s.idx_2 = (unsigned)m[o];
            for (int j = 0; j < 3; ++j) s.pos_w(j) = pos[3 * o + j];
            out[k].push_back(s);
        }
    return out;
}

}  // namespace hip
}  // namespace module
}  // namespace stella_vslam
