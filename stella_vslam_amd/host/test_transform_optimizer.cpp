// optimize::hip::transform_optimizer on a stand-in map of two keyframes.  Without an argument: a map with 30 matches is built here; the
// class is run twice on fresh copies and as a batch of two candidates: the results have to be bit-equal, the filtered entries untouched,
// the gross mismatches null.  With a file name: the map is read from that file (the format tests/test_gpu_sim3opt.py writes), the class
// is run, and the return value, the Sim3 (%.17g) and the null pattern of matched_lms_in_keyfrm_2 are printed.
//   fix_scale num_iter chi_sq
//   two cameras: model (0 perspective, 2 equirectangular) cols rows fx fy cx cy, then 12 doubles pose_cw (3 x 4, row-major)
//   8 doubles Sim3_12 (qx qy qz qw tx ty tz s)
//   N1, per keypoint of keyframe 1: x y octave has_landmark erased X Y Z
//   N2, per keypoint of keyframe 2: x y octave
//   per keypoint of keyframe 1, the entry of matched_lms_in_keyfrm_2: has_landmark erased idx2 (-1: not observed in keyframe 2) X Y Z
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <vector>

#include "drop_in/transform_optimizer_hip.h"
#include "sv_sim3.h"

using namespace stella_vslam;

namespace {
int g_fail = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                           \
        }                                                       \
    } while (0)

struct toy_map {
    std::unique_ptr<camera::base> cam[2];
    feature::orb_params orb;
    std::shared_ptr<data::keyframe> kf[2], other;  // `other`: a keyframe neither landmark list belongs to
    std::vector<std::shared_ptr<data::landmark>> matched;
    g2o::Sim3 sim3;
    int fix_scale = 0, num_iter = 10;
    float chi_sq = 10.0f;
};

std::shared_ptr<data::landmark> read_landmark(std::istream& in, unsigned int id, int& erased) {
    int has;
    Vec3_t p;
    in >> has >> erased;
    return has ? (in >> p(0) >> p(1) >> p(2), std::make_shared<data::landmark>(id, p)) : (in >> p(0) >> p(1) >> p(2), nullptr);
}

bool read_map(std::istream& in, toy_map& M) {
    in >> M.fix_scale >> M.num_iter >> M.chi_sq;
    for (int v = 0; v < 2; ++v) {
        int model;
        unsigned int cols, rows;
        double fx, fy, cx, cy;
        in >> model >> cols >> rows >> fx >> fy >> cx >> cy;
        if (model == 2) M.cam[v].reset(new camera::equirectangular(cols, rows));
        else M.cam[v].reset(new camera::perspective(camera::setup_type_t::Monocular, cols, rows, fx, fy, cx, cy, 0, 0, 0, 0, 0));
        M.kf[v] = std::make_shared<data::keyframe>(v + 1, M.cam[v].get(), &M.orb);
        Mat44_t T = Mat44_t::Identity();
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) in >> T(i, j);
        M.kf[v]->set_pose_cw(T);
    }
    M.other = std::make_shared<data::keyframe>(99, M.cam[0].get(), &M.orb);
    double p8[8];
    for (double& v : p8) in >> v;
    M.sim3 = g2o::Sim3(p8);
    unsigned int next_id = 0;
    int n1, n2;
    in >> n1;
    for (int k = 0; k < n1; ++k) {
        cv::KeyPoint kp;
        int erased;
        in >> kp.pt.x >> kp.pt.y >> kp.octave;
        auto lm = read_landmark(in, next_id++, erased);
        M.kf[0]->frm_obs_.undist_keypts_.push_back(kp);
        M.kf[0]->landmarks_.push_back(lm);
        if (lm) lm->add_observation(M.kf[0], (unsigned int)k);
        if (lm && erased) lm->erase_observation(nullptr, M.other);  // at most two observations left: will_be_erased
    }
    in >> n2;
    for (int k = 0; k < n2; ++k) {
        cv::KeyPoint kp;
        in >> kp.pt.x >> kp.pt.y >> kp.octave;
        M.kf[1]->frm_obs_.undist_keypts_.push_back(kp);
        M.kf[1]->landmarks_.push_back(nullptr);
    }
    for (int k = 0; k < n1; ++k) {
        int has, erased, idx2;
        Vec3_t p;
        in >> has >> erased >> idx2 >> p(0) >> p(1) >> p(2);
        std::shared_ptr<data::landmark> lm = has ? std::make_shared<data::landmark>(next_id++, p) : nullptr;
        if (lm && idx2 >= 0) {
            lm->add_observation(M.kf[1], (unsigned int)idx2);
            M.kf[1]->landmarks_.at(idx2) = lm;
        }
        if (lm && erased) lm->erase_observation(nullptr, M.other);
        M.matched.push_back(lm);
    }
    return (bool)in;
}

// the built-in map as text: 30 matches 4 .. 9 deep, keyframe 2 in a world 1.1 times as large; entry 3 is null, 7 is to be erased, 11 is
// not observed in keyframe 2, keyframe 1 has no landmark at 13, and the last four matches are gross mismatches
std::string builtin_map(int variant) {
    std::ostringstream o;
    o.precision(17);
    const int n = 30;
    o << "0 10 10\n";
    o << "0 640 480 520 515 320.5 240.25  1 0 0 0.3  0 1 0 -1  0 0 1 2\n";
    o << "0 640 480 480 482 330 250  1 0 0 -1.5  0 1 0 0.2  0 0 1 0.7\n";
    const SvSim3 truth = sv_sim3_exp(SvVec7{0.03, -0.12 + 0.01 * variant, 0.02, 0.4, -0.05, 0.1, std::log(1.1)});
    const SvSim3 start = sv_sim3_mul(sv_sim3_exp(SvVec7{0.02, -0.015, 0.01, 0.03, -0.02, 0.03, std::log(1.03)}), truth);
    double p8[8];
    sv_sim3_store(p8, start);
    for (double v : p8) o << v << ' ';
    o << '\n' << n << '\n';
    std::vector<SvVec3> P1(n), P2(n);
    for (int k = 0; k < n; ++k) {
        const double z = 4.0 + 5.0 * ((k * 7) % n) / n;
        P1[k] = sv3(z * 0.45 * std::sin(1.0 + 2.3 * k), z * 0.35 * std::cos(0.5 + 1.7 * k), z);
        P2[k] = sv_sim3_map(sv_sim3_inv(truth), P1[k]);
        const float x = (float)(520 * P1[k].x / P1[k].z + 320.5 + 0.4 * std::sin(5.0 * k)), y = (float)(515 * P1[k].y / P1[k].z + 240.25 + 0.4 * std::cos(3.0 * k));
        o << x << ' ' << y << ' ' << k % 3 << ' ' << (k != 13) << " 0 " << P1[k].x - 0.3 << ' ' << P1[k].y + 1.0 << ' ' << P1[k].z - 2.0 << '\n';
    }
    o << n << '\n';
    for (int k = 0; k < n; ++k) {
        float x = (float)(480 * P2[k].x / P2[k].z + 330 + 0.4 * std::cos(4.0 * k)), y = (float)(482 * P2[k].y / P2[k].z + 250 + 0.4 * std::sin(2.0 * k));
        if (k >= n - 4) x += 40.0f, y -= 35.0f;
        o << x << ' ' << y << ' ' << (k + 1) % 3 << '\n';
    }
    for (int k = 0; k < n; ++k)
        o << (k != 3) << ' ' << (k == 7) << ' ' << (k == 11 ? -1 : k) << ' ' << P2[k].x + 1.5 << ' ' << P2[k].y - 0.2 << ' ' << P2[k].z - 0.7 << '\n';
    return o.str();
}

bool load(toy_map& M, int variant) {
    std::istringstream in(builtin_map(variant));
    return read_map(in, M);
}
bool same_sim3(const g2o::Sim3& a, const g2o::Sim3& b) {
    return std::memcmp(a.q, b.q, sizeof a.q) == 0 && std::memcmp(a.t, b.t, sizeof a.t) == 0 && std::memcmp(&a.s, &b.s, sizeof a.s) == 0;
}
}  // namespace

int main(int argc, char** argv) {
    toy_map M;
    if (argc > 1) {
        std::ifstream in(argv[1]);
        if (!read_map(in, M)) return 3;
        optimize::hip::transform_optimizer opt(M.fix_scale != 0, (unsigned int)M.num_iter);
        const unsigned int ret = opt.optimize(M.kf[0], M.kf[1], M.matched, M.sim3, M.chi_sq);
        std::printf("RET %u\nSIM3", ret);
        for (double v : M.sim3.q) std::printf(" %.17g", v);
        for (double v : M.sim3.t) std::printf(" %.17g", v);
        std::printf(" %.17g\nNULL", M.sim3.s);
        for (const auto& lm : M.matched) std::printf(" %d", lm ? 0 : 1);
        const auto& st = opt.last_stats_.at(0);
        std::printf("\nSTATS %d %d %d %d %d %d\n", st.lm_iterations[0], st.lm_iterations[1], st.lm_trials[0], st.lm_trials[1], st.early_return, st.num_survivors);
        return 0;
    }
    CHECK(load(M, 0));
    const g2o::Sim3 before = M.sim3;
    const auto matched_before = M.matched;
    optimize::hip::transform_optimizer opt(false);
    const unsigned int ret = opt.optimize(M.kf[0], M.kf[1], M.matched, M.sim3, 10.0f);
    CHECK(ret == 22);  // 30 - 4 filtered - 4 gross mismatches
    CHECK(!same_sim3(M.sim3, before) && std::fabs(M.sim3.s - 1.1) < 0.02);
    for (int k = 0; k < 30; ++k) {
        const bool filtered = k == 3 || k == 7 || k == 11 || k == 13, gross = k >= 26;
        if (filtered) CHECK(M.matched[k] == matched_before[k]);  // the filter leaves an entry as it came, null or not
        else CHECK((M.matched[k] == nullptr) == gross);
    }
    CHECK(opt.last_stats_.at(0).lm_iterations[0] == 5 && opt.last_stats_[0].lm_iterations[1] >= 1 && opt.last_stats_[0].num_survivors == 22);
    // a fresh copy gives the same bits; a batch of two candidates gives what the single calls give
    toy_map A, B, C;
    CHECK(load(A, 0) && load(B, 1) && load(C, 1));
    optimize::hip::transform_optimizer opt2(false);
    const unsigned int ret_c = opt2.optimize(C.kf[0], C.kf[1], C.matched, C.sim3, 10.0f);
    std::vector<std::vector<std::shared_ptr<data::landmark>>> matched{A.matched, B.matched};
    // both candidates against A's keyframe 1: B's keyframe 1 is a copy of it with landmarks of its own, so B's matches are re-seated
    for (size_t k = 0; k < B.kf[0]->landmarks_.size(); ++k)
        if (B.kf[0]->landmarks_[k] && A.kf[0]->landmarks_[k]) CHECK(std::memcmp(B.kf[0]->landmarks_[k]->pos_w_.data(), A.kf[0]->landmarks_[k]->pos_w_.data(), 24) == 0);
    std::vector<g2o::Sim3> sim3s{A.sim3, B.sim3};
    const auto rets = opt2.optimize_batch(A.kf[0], {A.kf[1], B.kf[1]}, matched, sim3s, 10.0f);
    CHECK(rets.size() == 2 && rets[0] == ret && rets[1] == ret_c);
    CHECK(same_sim3(sim3s[0], M.sim3) && same_sim3(sim3s[1], C.sim3));
    for (int k = 0; k < 30; ++k) CHECK((matched[0][k] == nullptr) == (M.matched[k] == nullptr) && (matched[1][k] == nullptr) == (C.matched[k] == nullptr));
    // fewer than 10 survivors: 0, the Sim3 as it came, the rejected matches null
    toy_map E;
    CHECK(load(E, 0));
    for (int k = 12; k < 26; ++k) E.matched[k] = nullptr;  // 12 - 3 filtered = 9 valid matches and the 4 gross ones
    const g2o::Sim3 e_before = E.sim3;
    CHECK(opt2.optimize(E.kf[0], E.kf[1], E.matched, E.sim3, 10.0f) == 0 && same_sim3(E.sim3, e_before) && opt2.last_stats_[0].early_return == 1);
    for (int k = 26; k < 30; ++k) CHECK(E.matched[k] == nullptr);
    // a refused call (a start that is not a Sim3) throws and leaves the caller's list and Sim3 as they came
    toy_map R;
    CHECK(load(R, 0));
    R.sim3.q[3] *= 1.01;
    const auto r_before = R.matched;
    bool thrown = false;
    try {
        opt2.optimize(R.kf[0], R.kf[1], R.matched, R.sim3, 10.0f);
    }
    catch (const std::exception&) {
        thrown = true;
    }
    CHECK(thrown && R.matched == r_before);
    std::printf("inliers %u, LM iterations %d + %d, scale %.6f\n", ret, opt.last_stats_[0].lm_iterations[0], opt.last_stats_[0].lm_iterations[1], M.sim3.s);
    if (g_fail) return 1;
    std::printf("transform_optimizer ok\n");
    return 0;
}
