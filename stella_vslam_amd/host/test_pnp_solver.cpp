// solve::hip::pnp_solver on planted 2D-3D matches: with use_fixed_seed the single form is reproducible from solver to solver, the batch
// form leaves every solver in the state its own find_via_ransac leaves it in (bit for bit), and the planted pose comes back.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "drop_in/pnp_solver_hip.h"

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

struct problem {
    eigen_alloc_vector<Vec3_t> bearings, points;
    std::vector<int> octaves;
    double yaw, centre[3];
};

problem make_problem(int n, double yaw, double cx, double cy, double cz) {  // camera centre (cx, cy, cz), rotation about y, every fifth match an outlier
    problem p;
    p.yaw = yaw, p.centre[0] = cx, p.centre[1] = cy, p.centre[2] = cz;
    const double c = std::cos(yaw), s = std::sin(yaw);
    for (int i = 0; i < n; ++i) {
        const double d = 3.0 + 6.0 * uni();
        const double X = (uni() - 0.5) * d, Y = (uni() - 0.5) * 0.7 * d, Z = d;  // camera frame
        Vec3_t pw, b;
        // pos_c = R (pos_w - centre), R = [c 0 s; 0 1 0; -s 0 c]  ->  pos_w = R^T pos_c + centre
        pw(0) = c * X - s * Z + cx, pw(1) = Y + cy, pw(2) = s * X + c * Z + cz;
        double bx = X, by = Y, bz = Z;
        if (i % 5 == 4) bx += (uni() < 0.5 ? -0.4 : 0.4) * Z, by += 0.2 * Z;  // at least 20 degrees off: beyond every octave's threshold
        const double l = std::sqrt(bx * bx + by * by + bz * bz);
        b(0) = bx / l, b(1) = by / l, b(2) = bz / l;
        p.points.push_back(pw);
        p.bearings.push_back(b);
        p.octaves.push_back(i % 8);
    }
    return p;
}

bool same_state(const solve::hip::pnp_solver& a, const solve::hip::pnp_solver& b) {
    if (a.solution_is_valid() != b.solution_is_valid() || a.best_iter_ != b.best_iter_ || a.get_inlier_flags() != b.get_inlier_flags()) return false;
    if (!a.solution_is_valid()) return true;
    const Mat44_t pa = a.get_best_cam_pose(), pb = b.get_best_cam_pose();
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            const double x = pa(r, c), y = pb(r, c);
            if (std::memcmp(&x, &y, sizeof x) != 0) return false;
        }
    return true;
}
}  // namespace

// --draws: the sample tables a fresh fixed-seed solver draws for 80, 5 and 300 matches, 30 iterations each (no device needed):
// tests/test_pnp_problem_classes.py compares them with what the reference's util::create_random_array gave (tests/golden/pnp_random_array.json)
int print_draws() {
    const unsigned ns[3] = {80, 5, 300};
    std::printf("[");
    for (int k = 0; k < 3; ++k) {
        eigen_alloc_vector<Vec3_t> v(ns[k]);
        std::vector<int> oct(ns[k], 0);
        solve::hip::pnp_solver s(v, oct, v, {1.0f}, 0, true, 10);
        const auto t = s.draw(30);
        std::printf("%s[", k ? ", " : "");
        for (size_t i = 0; i < t.size(); ++i) std::printf("%s%u", i ? ", " : "", t[i]);
        std::printf("]");
    }
    std::printf("]\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--draws") == 0) return print_draws();
    std::vector<float> scale_factors(8, 1.0f);
    for (int l = 1; l < 8; ++l) scale_factors[l] = 1.2f * scale_factors[l - 1];
    const int sizes[] = {150, 80, 3, 300, 9, 64, 0, 65};
    std::vector<problem> probs;
    for (int j = 0; j < 8; ++j) probs.push_back(make_problem(sizes[j], 0.05 * (j + 1), 0.3 * j, -0.1 * j, 0.2 * j));
    using solver = solve::hip::pnp_solver;
    std::vector<std::unique_ptr<solver>> first, second, batched;
    for (auto* list : {&first, &second, &batched})
        for (const problem& p : probs) list->emplace_back(new solver(p.bearings, p.octaves, p.points, scale_factors, 10, true, 10));
    for (auto& s : first) s->find_via_ransac(30, true);
    for (auto& s : second) s->find_via_ransac(30, true);
    std::vector<solver*> ptrs;
    for (auto& s : batched) ptrs.push_back(s.get());
    solver::find_via_ransac_batch(ptrs, 30, true);
    int valid = 0;
    for (size_t j = 0; j < probs.size(); ++j) {
        CHECK(same_state(*first[j], *second[j]));   // use_fixed_seed: reproducible
        CHECK(same_state(*first[j], *batched[j]));  // the batch form equals the single solvers
        const bool small = sizes[j] < 10;
        CHECK(first[j]->solution_is_valid() == !small);
        if (!first[j]->solution_is_valid()) continue;
        ++valid;
        const Mat44_t P = first[j]->get_best_cam_pose();
        const double c = std::cos(probs[j].yaw), s = std::sin(probs[j].yaw);
        CHECK(std::fabs(P(0, 0) - c) < 1e-6 && std::fabs(P(0, 2) - s) < 1e-6 && std::fabs(P(1, 1) - 1.0) < 1e-6 && std::fabs(P(2, 0) + s) < 1e-6);
        const double* ctr = probs[j].centre;
        for (int r = 0; r < 3; ++r) CHECK(std::fabs(P(r, 3) + (P(r, 0) * ctr[0] + P(r, 1) * ctr[1] + P(r, 2) * ctr[2])) < 1e-6);
        const auto flags = first[j]->get_inlier_flags();
        CHECK((int)flags.size() == sizes[j]);
        int wrong = 0;
        for (int i = 0; i < sizes[j]; ++i) wrong += flags[i] == (i % 5 == 4);
        CHECK(wrong == 0);
    }
    CHECK(valid == 5);
    // a second call on the same solver goes on drawing from the same engine, as the reference does
    first[0]->find_via_ransac(30, true);
    CHECK(first[0]->solution_is_valid());
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("pnp_solver ok: %d valid of %zu\n", valid, probs.size());
    return 0;
}
