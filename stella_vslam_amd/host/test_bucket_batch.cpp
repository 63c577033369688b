// The batched bucket matchers of the drop-in classes (host/drop_in/hip_backend.h) beside the per-call methods, on identical stand-in
// objects: bow_tree::match_frame_and_keyframe_batch, match_keyframes_batch and match_for_triangulation_batch on bow_tree and robust must
// fill exactly what K calls of the per-call method fill -- the same landmark pointers at the same keypoints, the same pairs, the same
// counts.  The toy map is the one of test_drop_in.cpp (keyframes on an arc, landmarks with descriptors and BoW nodes, clutter).
// Built by host/Makefile, run by tests/test_gpu_bucket_batch.py.
#include <cmath>
#include <cstdio>
#include <random>

#include "drop_in/hip_backend.h"

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

static data::frame frame_like(toy_map& M, int k, bool with_pose) {
    data::frame f(1000 + k, &M.cam, &M.orb);
    f.frm_obs_ = M.kfs[k]->frm_obs_;
    f.bow_feat_vec_ = M.kfs[k]->bow_feat_vec_;
    f.landmarks_.assign(f.frm_obs_.undist_keypts_.size(), nullptr);
    if (with_pose) f.set_pose_cw(M.kfs[k]->get_pose_cw());
    return f;
}

static Mat33_t essential(const Mat44_t& TA, const Mat44_t& TB) {
    Mat33_t R12, E12;
    double t12[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R12(i, j) = TA(i, 0) * TB(j, 0) + TA(i, 1) * TB(j, 1) + TA(i, 2) * TB(j, 2);
    for (int i = 0; i < 3; ++i) t12[i] = TA(i, 3) - (R12(i, 0) * TB(0, 3) + R12(i, 1) * TB(1, 3) + R12(i, 2) * TB(2, 3));
    const double tx[9] = {0, -t12[2], t12[1], t12[2], 0, -t12[0], -t12[1], t12[0], 0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) E12(i, j) = tx[3 * i] * R12(0, j) + tx[3 * i + 1] * R12(1, j) + tx[3 * i + 2] * R12(2, j);
    return E12;
}

int main() {
    toy_map M;
    build(M, 8, 900, 300, 11);
    const match::hip::bow_tree bow(0.75, true);
    {  // relocalisation: every other keyframe (one of them twice) against a frame with keyframe 3's keypoints
        const std::vector<kf_ptr> cands = {M.kfs[0], M.kfs[2], M.kfs[2], M.kfs[4], M.kfs[5], M.kfs[7]};
        data::frame frm = frame_like(M, 3, false);
        std::vector<std::vector<lm_ptr>> got;
        const auto counts = bow.match_frame_and_keyframe_batch(cands, frm, got);
        REQUIRE(counts.size() == cands.size() && got.size() == cands.size());
        unsigned total = 0;
        for (size_t k = 0; k < cands.size(); ++k) {
            std::vector<lm_ptr> ref;
            const unsigned num = bow.match_frame_and_keyframe(cands[k], frm, ref);
            REQUIRE(num == counts[k] && ref == got[k]);
            total += num;
        }
        REQUIRE(total > 300 && got[1] == got[2]);
        std::vector<std::vector<lm_ptr>> none;
        REQUIRE(bow.match_frame_and_keyframe_batch({}, frm, none).empty() && none.empty());
    }
    {  // loop detection: keyframe 3 against the others
        const std::vector<kf_ptr> cands = {M.kfs[1], M.kfs[2], M.kfs[4], M.kfs[6]};
        std::vector<std::vector<lm_ptr>> got;
        const auto counts = bow.match_keyframes_batch(M.kfs[3], cands, got);
        unsigned total = 0;
        for (size_t k = 0; k < cands.size(); ++k) {
            std::vector<lm_ptr> ref;
            const unsigned num = bow.match_keyframes(M.kfs[3], cands[k], ref);
            REQUIRE(num == counts[k] && ref == got[k]);
            total += num;
        }
        REQUIRE(total > 300);
        std::vector<std::vector<lm_ptr>> one;  // a batch of one
        const auto c1 = bow.match_keyframes_batch(M.kfs[3], {M.kfs[4]}, one);
        REQUIRE(c1.size() == 1 && c1[0] == counts[2] && one[0] == got[2]);
    }
    {  // new-landmark creation: strip the landmarks of part of the keypoints, match keyframe 3's bare keypoints against its neighbours
        for (auto& kf : M.kfs)
            for (size_t i = 0; i < kf->landmarks_.size(); ++i)
                if (i % 2 == 0 || M.truth[kf->id_][i] % 3 == 0) kf->landmarks_[i] = nullptr;
        const std::vector<kf_ptr> nb = {M.kfs[1], M.kfs[2], M.kfs[4], M.kfs[5]};
        std::vector<Mat33_t> E;
        for (const auto& kf : nb) E.push_back(essential(M.kfs[3]->get_pose_cw(), kf->get_pose_cw()));
        for (int variant = 0; variant < 2; ++variant) {
            const match::hip::bow_tree tb(0.8, true);
            const match::hip::robust tr(0.8, true);
            std::vector<std::vector<std::pair<unsigned, unsigned>>> got;
            const auto counts = variant ? tb.match_for_triangulation_batch(M.kfs[3], nb, E, got, 0.02f) : tr.match_for_triangulation_batch(M.kfs[3], nb, E, got, 0.02f);
            REQUIRE(counts.size() == nb.size() && got.size() == nb.size());
            unsigned total = 0;
            for (size_t k = 0; k < nb.size(); ++k) {
                std::vector<std::pair<unsigned, unsigned>> ref;
                const unsigned num = variant ? tb.match_for_triangulation(M.kfs[3], nb[k], E[k], ref, 0.02f) : tr.match_for_triangulation(M.kfs[3], nb[k], E[k], ref, 0.02f);
                REQUIRE(num == counts[k] && ref == got[k] && num == ref.size());
                total += num;
            }
            REQUIRE(total > 100);
        }
    }
    std::printf("bucket batch drop-in ok\n");
    return 0;
}
