// module::hip::two_view_triangulator on stand-in keyframes (mono and stereo): the single-match form, the batch form and the C ABI called on
// the same flattened arrays agree bit for bit, and the planted points come back.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "drop_in/two_view_triangulator_hip.h"

using namespace stella_vslam;

namespace {
unsigned long long g_state = 88172645463325252ull;
double uni() {  // xorshift64, [0, 1)
    g_state ^= g_state << 13, g_state ^= g_state >> 7, g_state ^= g_state << 17;
    return (double)(g_state >> 11) / 9007199254740992.0;
}
int g_fail = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                           \
        }                                                       \
    } while (0)

Mat44_t make_pose(double yaw, double cx, double cy, double cz) {  // camera centre (cx, cy, cz), rotation about y
    Mat44_t P = Mat44_t::Identity();
    const double c = std::cos(yaw), s = std::sin(yaw);
    P(0, 0) = c, P(0, 2) = s, P(2, 0) = -s, P(2, 2) = c;
    for (int i = 0; i < 3; ++i) P(i, 3) = -(P(i, 0) * cx + P(i, 1) * cy + P(i, 2) * cz);
    return P;
}

int run_case(bool stereo) {
    const double fx = 520.0, fy = 515.0, cx = 320.5, cy = 240.25, fxb = stereo ? 52.0 : 0.0;
    camera::perspective cam(stereo ? camera::setup_type_t::Stereo : camera::setup_type_t::Monocular, 640, 480, fx, fy, cx, cy, 0, 0, 0, 0, 0, fxb);
    cam.img_bounds_ = camera::image_bounds{0.f, 640.f, 0.f, 480.f};
    feature::orb_params orb(1.2f, 8);
    auto kf1 = std::make_shared<data::keyframe>(1, &cam, &orb), kf2 = std::make_shared<data::keyframe>(2, &cam, &orb);
    kf1->set_pose_cw(make_pose(0.01, 0.0, 0.0, 0.0));
    kf2->set_pose_cw(stereo ? make_pose(-0.02, 0.05, 0.0, 0.2) : make_pose(-0.03, 0.4, 0.02, -0.05));
    const int n = 300;
    std::vector<std::pair<unsigned, unsigned>> matches;
    eigen_alloc_vector<Vec3_t> planted;
    for (int i = 0; i < n; ++i) {
        Vec3_t pw;
        const double d = 1.5 + 20.0 * uni() * uni();
        pw(0) = (uni() - 0.5) * d, pw(1) = (uni() - 0.5) * 0.7 * d, pw(2) = d;
        planted.push_back(pw);
        const bool outlier = i % 7 == 3;
        for (auto& kf : {kf1, kf2}) {
            const Mat44_t P = kf->get_pose_cw();
            const double X = P(0, 0) * pw(0) + P(0, 1) * pw(1) + P(0, 2) * pw(2) + P(0, 3), Y = P(1, 0) * pw(0) + P(1, 1) * pw(1) + P(1, 2) * pw(2) + P(1, 3),
                         Z = P(2, 0) * pw(0) + P(2, 1) * pw(1) + P(2, 2) * pw(2) + P(2, 3);
            cv::KeyPoint kp;
            kp.pt.x = (float)(fx * X / Z + cx + (uni() - 0.5) + (outlier && kf == kf2 ? 40.0 : 0.0));
            kp.pt.y = (float)(fy * Y / Z + cy + (uni() - 0.5));
            kp.octave = i % 8;
            kf->frm_obs_.undist_keypts_.push_back(kp);
            const double x = (kp.pt.x - cx) / fx, y = (kp.pt.y - cy) / fy, l = std::sqrt(x * x + y * y + 1.0);
            Vec3_t b;
            b(0) = x / l, b(1) = y / l, b(2) = 1.0 / l;
            kf->frm_obs_.bearings_.push_back(b);
            if (stereo) {
                const bool has = i % 5 != 0;
                kf->frm_obs_.stereo_x_right_.push_back(has ? (float)(kp.pt.x - fxb / Z) : -1.0f);
                kf->frm_obs_.depths_.push_back(has ? (float)(Z * (1.0 + 0.02 * (uni() - 0.5))) : -1.0f);
            }
        }
        matches.emplace_back((unsigned)i, (unsigned)((i * 7) % n));  // a third of the pairs are right, the rest mismatched keypoints
        if (i % 3 == 0) matches.back().second = (unsigned)i;
    }
    const module::hip::two_view_triangulator tri(kf1, kf2, 1.0);
    eigen_alloc_vector<Vec3_t> pos;
    std::vector<bool> ok;
    tri.triangulate(matches, pos, ok);
    CHECK((int)pos.size() == n && (int)ok.size() == n);
    int accepted = 0, close = 0;
    for (int i = 0; i < n; ++i) {
        if (!ok[i]) continue;
        ++accepted;
        if (matches[i].first == matches[i].second) {
            double e = 0, s = 0;
            for (int j = 0; j < 3; ++j) e += (pos[i](j) - planted[i](j)) * (pos[i](j) - planted[i](j)), s += planted[i](j) * planted[i](j);
            close += std::sqrt(e / s) < 0.2;
        }
    }
    CHECK(accepted >= 40 && accepted < n && close >= 30);
    // the reference's single-match signature gives the same bits
    for (int i = 0; i < n; i += 5) {
        Vec3_t p;
        const bool r = tri.triangulate(matches[i].first, matches[i].second, p);
        CHECK(r == ok[i] && std::memcmp(p.data(), pos[i].data(), 24) == 0);
    }
    // the C ABI on the same flattened arrays
    const auto &a = tri.side_1(), &b = tri.side_2();
    std::vector<int32_t> i1(n), i2(n);
    for (int i = 0; i < n; ++i) i1[i] = (int32_t)matches[i].first, i2[i] = (int32_t)matches[i].second;
    std::vector<double> pw(3 * (size_t)n);
    std::vector<uint8_t> st(n);
    int num = 0;
    hip::check(svgpu_triangulate_two_views(hip::context(), &a.cam, a.pose_cw, a.true_baseline, a.xy.data(), a.octave.data(), a.bearings.data(),
                                           a.xright.empty() ? nullptr : a.xright.data(), a.depth.empty() ? nullptr : a.depth.data(), a.n, &b.cam, b.pose_cw,
                                           b.true_baseline, b.xy.data(), b.octave.data(), b.bearings.data(), b.xright.empty() ? nullptr : b.xright.data(),
                                           b.depth.empty() ? nullptr : b.depth.data(), b.n, orb.scale_factors_.data(), orb.level_sigma_sq_.data(), 8, 1.2f, 1.2f,
                                           1.0f, i1.data(), i2.data(), n, pw.data(), st.data(), &num),
               "svgpu_triangulate_two_views");
    CHECK(num == accepted);
    for (int i = 0; i < n; ++i) CHECK((st[i] == SVGPU_TRI_ACCEPTED) == ok[i] && st[i] == tri.last_status_[i] && std::memcmp(&pw[3 * (size_t)i], pos[i].data(), 24) == 0);
    if (stereo) CHECK(a.true_baseline == 0.1 && !a.xright.empty());
    std::printf("%s: %d of %d matches accepted, %d right pairs within 20 %% of the planted point\n", stereo ? "stereo" : "mono", accepted, n, close);
    return accepted;
}
}  // namespace

int main() {
    try {
        run_case(false);
        run_case(true);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    if (g_fail) return 1;
    std::printf("two_view_triangulator ok\n");
    return 0;
}
