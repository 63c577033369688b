// module::hip::new_landmark_creator::create beside the loop of mapping_module::create_new_landmarks (mapping_module.cc:286-340) written over the
// per-call drop-in classes -- match::hip::robust / bow_tree::match_for_triangulation and module::hip::two_view_triangulator, with every
// accepted triangulation attached to the current keyframe (and the neighbour) before the next neighbour is matched, as
// triangulate_with_two_keyframes does (:343-375).  Compared: the same pairs, the same positions bit for bit, the same neighbour for every
// created landmark.  The toy map is the one of test_drop_in.cpp (keyframes on an arc, landmarks with descriptors and BoW nodes, clutter).
// Built by host/Makefile, run by tests/test_gpu_new_landmarks_drop_in.py.
#include <cmath>
#include <cstdio>
#include <random>

#include "drop_in/hip_backend.h"
#include "drop_in/new_landmarks_hip.h"

using namespace stella_vslam;
using lm_ptr = std::shared_ptr<data::landmark>;
using kf_ptr = std::shared_ptr<data::keyframe>;

#define REQUIRE(c)                                                              \
    do {                                                                        \
        if (!(c)) {                                                             \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                           \
        }                                                                       \
    } while (0)

static Mat44_t look_at(const double c[3], const double target[3]) {
    double z[3] = {target[0] - c[0], target[1] - c[1], target[2] - c[2]};
    const double nz = std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
    for (double& v : z) v /= nz;
    double x[3] = {z[2], 0.0, -z[0]};  // cross((0,1,0), z)
    const double nx = std::sqrt(x[0] * x[0] + x[2] * x[2]);
    for (double& v : x) v /= nx;
    const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
    Mat44_t T = Mat44_t::Identity();
    for (int j = 0; j < 3; ++j) {
        T(0, j) = x[j];
        T(1, j) = y[j];
        T(2, j) = z[j];
    }
    for (int i = 0; i < 3; ++i) T(i, 3) = -(T(i, 0) * c[0] + T(i, 1) * c[1] + T(i, 2) * c[2]);
    return T;
}

struct toy_map {
    camera::perspective cam{camera::setup_type_t::Monocular, 752, 480, 458.654, 457.296, 367.215, 248.375, 0, 0, 0, 0, 0};
    feature::orb_params orb;
    data::map_database db;
    std::vector<kf_ptr> kfs;
    std::vector<lm_ptr> lms;
    std::vector<std::vector<int>> truth;  // truth[kf][keypoint] = landmark id or -1
    std::vector<Mat44_t> pose_gt;
    std::vector<Vec3_t> pos_gt;
};

static void project(const toy_map& M, const Mat44_t& T, const Vec3_t& p, double& u, double& v, double& z) {
    const double X = T(0, 0) * p(0) + T(0, 1) * p(1) + T(0, 2) * p(2) + T(0, 3), Y = T(1, 0) * p(0) + T(1, 1) * p(1) + T(1, 2) * p(2) + T(1, 3);
    z = T(2, 0) * p(0) + T(2, 1) * p(1) + T(2, 2) * p(2) + T(2, 3);
    u = M.cam.fx_ * X / z + M.cam.cx_;
    v = M.cam.fy_ * Y / z + M.cam.cy_;
}

static void build(toy_map& M, int n_kf, int n_lm, int n_clutter, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> N(0.0, 1.0);
    M.cam.img_bounds_ = camera::image_bounds{0.f, 752.f, 0.f, 480.f};
    std::vector<std::array<uint8_t, 32>> lm_desc(n_lm);
    for (int l = 0; l < n_lm; ++l) {
        Vec3_t p;
        p(0) = -3.0 + 6.0 * U(rng), p(1) = -1.8 + 3.6 * U(rng), p(2) = 4.5 + 4.0 * U(rng);
        M.pos_gt.push_back(p);
        M.lms.push_back(std::make_shared<data::landmark>((unsigned)l, p));
        for (auto& b : lm_desc[l]) b = (uint8_t)(rng() & 255);
    }
    const double target[3] = {0, 0, 6.5};
    for (int k = 0; k < n_kf; ++k) {
        const double a = -0.25 + 0.5 * k / std::max(1, n_kf - 1);
        const double c[3] = {3.0 * std::sin(a), 0.05 * k, 3.0 - 3.0 * std::cos(a)};
        auto kf = std::make_shared<data::keyframe>((unsigned)k, &M.cam, &M.orb);
        const Mat44_t T = look_at(c, target);
        kf->set_pose_cw(T);
        M.pose_gt.push_back(T);
        std::vector<cv::KeyPoint> kps;
        std::vector<std::array<uint8_t, 32>> descs;
        std::vector<int> truth;
        for (int l = 0; l < n_lm; ++l) {
            double u, v, z;
            project(M, T, M.pos_gt[l], u, v, z);
            if (z < 0.5 || u < 8 || u > 744 || v < 8 || v > 472 || U(rng) > 0.8) continue;
            cv::KeyPoint kp;
            const double dist = std::sqrt(std::pow(M.pos_gt[l](0) - c[0], 2) + std::pow(M.pos_gt[l](1) - c[1], 2) + std::pow(M.pos_gt[l](2) - c[2], 2));
            kp.octave = std::min(7, std::max(0, (int)std::lround(std::log(9.0 / dist) / std::log(1.2)) + 1));
            kp.pt.x = (float)(u + 0.5 * N(rng) * M.orb.scale_factors_[kp.octave]);
            kp.pt.y = (float)(v + 0.5 * N(rng) * M.orb.scale_factors_[kp.octave]);
            kp.angle = (float)std::fmod(360.0 + 7.0 * l + 3.0 * N(rng), 360.0);
            auto d = lm_desc[l];
            for (int f = (int)(rng() % 24); f > 0; --f) {
                const unsigned bit = rng() & 255;
                d[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
            }
            kps.push_back(kp);
            descs.push_back(d);
            truth.push_back(l);
        }
        for (int e = 0; e < n_clutter; ++e) {
            cv::KeyPoint kp;
            kp.pt.x = (float)(752 * U(rng)), kp.pt.y = (float)(480 * U(rng));
            kp.octave = (int)(rng() % 8), kp.angle = (float)(360 * U(rng));
            std::array<uint8_t, 32> d;
            for (auto& b : d) b = (uint8_t)(rng() & 255);
            kps.push_back(kp);
            descs.push_back(d);
            truth.push_back(-1);
        }
        const int n = (int)kps.size();
        kf->frm_obs_.undist_keypts_ = kps;
        kf->frm_obs_.descriptors_.create(n, 32, CV_8U);
        kf->frm_obs_.bearings_.resize(n);
        kf->landmarks_.assign(n, nullptr);
        for (int i = 0; i < n; ++i) {
            std::memcpy(kf->frm_obs_.descriptors_.ptr(i), descs[i].data(), 32);
            const double x = (kps[i].pt.x - M.cam.cx_) / M.cam.fx_, y = (kps[i].pt.y - M.cam.cy_) / M.cam.fy_, l2 = std::sqrt(x * x + y * y + 1.0);
            kf->frm_obs_.bearings_[i](0) = x / l2, kf->frm_obs_.bearings_[i](1) = y / l2, kf->frm_obs_.bearings_[i](2) = 1.0 / l2;
            const int node = truth[i] >= 0 ? truth[i] % 60 : (int)(rng() % 60);
            kf->bow_feat_vec_[(unsigned)node].push_back((unsigned)i);
            if (truth[i] >= 0) {
                kf->landmarks_[i] = M.lms[truth[i]];
                M.lms[truth[i]]->add_observation(kf, (unsigned)i);
                if (M.lms[truth[i]]->ref_keyfrm_.expired()) M.lms[truth[i]]->ref_keyfrm_ = kf;
            }
        }
        M.kfs.push_back(kf);
        M.truth.push_back(truth);
    }
    for (auto& lm : M.lms) {
        lm->compute_descriptor();
        lm->update_mean_normal_and_obs_scale_variance();
    }
}

using seed = module::hip::new_landmark_creator::seed;

// the reference loop; `E` per neighbour from new_landmark_creator::essential (create_E_21 of the two poses)
static std::vector<std::vector<seed>> reference_loop(toy_map& M, const kf_ptr& cur, const std::vector<kf_ptr>& nb, const std::vector<bool>& active, bool use_bow,
                                                     float thr, std::vector<int>& created_by) {
    const match::hip::bow_tree tb(0.8, true);
    const match::hip::robust tr(0.8, true);
    std::vector<std::vector<seed>> out(nb.size());
    created_by.assign(cur->landmarks_.size(), -1);
    unsigned next_id = 100000;
    for (size_t k = 0; k < nb.size(); ++k) {
        if (!active.empty() && !active[k]) continue;
        const Mat33_t E = module::hip::new_landmark_creator::essential(cur, nb[k]);
        std::vector<std::pair<unsigned, unsigned>> matches;
        if (use_bow) tb.match_for_triangulation(cur, nb[k], E, matches, thr);
        else tr.match_for_triangulation(cur, nb[k], E, matches, thr);
        const module::hip::two_view_triangulator tri(cur, nb[k], 1.0f);
        eigen_alloc_vector<Vec3_t> pos;
        std::vector<bool> ok;
        tri.triangulate(matches, pos, ok);
        for (size_t i = 0; i < matches.size(); ++i) {
            if (!ok[i]) continue;
            auto lm = std::make_shared<data::landmark>(next_id++, pos[i]);  // :358-367: the landmark sits on both keypoints from here on
            cur->landmarks_[matches[i].first] = lm;
            nb[k]->landmarks_[matches[i].second] = lm;
            M.lms.push_back(lm);
            seed s;
            s.idx_1 = matches[i].first, s.idx_2 = matches[i].second, s.pos_w = pos[i];
            out[k].push_back(s);
            created_by[matches[i].first] = (int)k;
        }
    }
    return out;
}

static bool same(const std::vector<std::vector<seed>>& a, const std::vector<std::vector<seed>>& b) {
    if (a.size() != b.size()) return false;
    for (size_t k = 0; k < a.size(); ++k) {
        if (a[k].size() != b[k].size()) return false;
        for (size_t i = 0; i < a[k].size(); ++i) {
            if (a[k][i].idx_1 != b[k][i].idx_1 || a[k][i].idx_2 != b[k][i].idx_2) return false;
            for (int j = 0; j < 3; ++j) {
                const double x = a[k][i].pos_w(j), y = b[k][i].pos_w(j);
                if (std::memcmp(&x, &y, sizeof x) != 0) return false;  // bit for bit
            }
        }
    }
    return true;
}

int main() {
    toy_map M;
    build(M, 8, 900, 300, 11);
    // new-landmark creation: strip the landmarks of part of the keypoints, as test_bucket_batch.cpp does
    for (auto& kf : M.kfs)
        for (size_t i = 0; i < kf->landmarks_.size(); ++i)
            if (i % 2 == 0 || M.truth[kf->id_][i] % 3 == 0) kf->landmarks_[i] = nullptr;
    const kf_ptr cur = M.kfs[3];
    const std::vector<kf_ptr> nb = {M.kfs[1], M.kfs[2], M.kfs[4], M.kfs[5], M.kfs[6]};
    std::vector<std::vector<lm_ptr>> saved;
    for (const auto& kf : M.kfs) saved.push_back(kf->landmarks_);
    auto restore = [&]() {
        for (size_t k = 0; k < M.kfs.size(); ++k) M.kfs[k]->landmarks_ = saved[k];
    };
    const std::vector<std::vector<bool>> actives = {{}, {true, false, true, true, false}, {false, false, false, false, false}};
    for (int use_bow = 0; use_bow < 2; ++use_bow)
        for (const auto& active : actives) {
            std::vector<int> ref_by;
            const auto ref = reference_loop(M, cur, nb, active, use_bow != 0, 0.02f, ref_by);
            restore();
            size_t total = 0, later = 0;
            for (size_t k = 0; k < ref.size(); ++k) total += ref[k].size(), later += k > 0 ? ref[k].size() : 0;
            for (const unsigned min_batch : {1u, 100u}) {  // the one batch call; the chain of single calls inside the class
                module::hip::new_landmark_creator creator(0.8f, true, use_bow != 0, 1.0f);
                creator.min_neighbours_for_batch_ = min_batch;
                const auto got = creator.create(cur, nb, active, 0.02f);
                REQUIRE(same(got, ref));
                REQUIRE(creator.created_by_.size() == ref_by.size());
                for (size_t i = 0; i < ref_by.size(); ++i) REQUIRE(creator.created_by_[i] == ref_by[i]);
                REQUIRE((creator.last_stats_.synchronisations == 2) == (min_batch == 1 && total > 0));
                for (const auto& kf : M.kfs) REQUIRE(kf->landmarks_ == saved[kf->id_]);  // create() attaches nothing
            }
            const bool none = !active.empty() && !active[0] && !active[2];
            REQUIRE(none ? total == 0 : (total > 60 && later > 10));
            for (const auto& per : ref)
                for (size_t i = 1; i < per.size(); ++i) REQUIRE(per[i - 1].idx_1 < per[i].idx_1);  // idx_1 order
        }
    {  // the carry matters on this map: the independent batch composition accepts keypoints twice, the loop never does
        module::hip::new_landmark_creator creator(0.8f, true, true, 1.0f);
        const auto got = creator.create(cur, nb, {}, 0.02f);
        std::vector<int> times(cur->landmarks_.size(), 0);
        for (const auto& per : got)
            for (const auto& s : per) REQUIRE(++times[s.idx_1] == 1);
        REQUIRE(creator.create(cur, {}, {}, 0.02f).empty());
    }
    std::printf("new landmarks drop-in ok\n");
    return 0;
}
