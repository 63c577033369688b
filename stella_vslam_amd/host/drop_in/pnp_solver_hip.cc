#include "pnp_solver_hip.h"

#include <algorithm>
#include <stdexcept>

namespace stella_vslam {
namespace solve {
namespace hip {

namespace {
// The engine of util::create_random_engine (util/random_array.cc:12-24): default-seeded when the seed is fixed, else seeded from ten
// words of the system's entropy source.
std::mt19937 make_engine(bool fixed) {
    if (fixed) return std::mt19937();
    std::random_device entropy;
    std::uint_least32_t words[10];
    for (auto& w : words) w = entropy();
    std::seed_seq seq(words, words + 10);
    return std::mt19937(seq);
}
// The procedure of util::create_random_array(count, lo, hi, engine) (util/random_array.cc:26-63), whose consumption of the engine a fixed
// seed makes observable: top the pool up to floor(1.2 count) uniform draws, sort, drop duplicates, cut to `count`; repeat while fewer
// than `count` are left; then std::shuffle with the same engine.
void draw_distinct(unsigned count, unsigned lo, unsigned hi, std::mt19937& engine, uint32_t* out) {
    std::uniform_int_distribution<unsigned> pick(lo, hi);
    const size_t pool_size = (size_t)(count * 1.2);
    std::vector<unsigned> pool;
    do {
        while (pool.size() < pool_size) pool.push_back(pick(engine));
        std::sort(pool.begin(), pool.end());
        pool.erase(std::unique(pool.begin(), pool.end()), pool.end());
        if (pool.size() > count) pool.resize(count);
    } while (pool.size() != count);
    std::shuffle(pool.begin(), pool.end(), engine);
    std::copy(pool.begin(), pool.end(), out);
}
}  // namespace

pnp_solver::pnp_solver(const eigen_alloc_vector<Vec3_t>& valid_bearings, const std::vector<int>& octaves, const eigen_alloc_vector<Vec3_t>& valid_points,
                       const std::vector<float>& scale_factors, unsigned int min_num_inliers, bool use_fixed_seed, unsigned int gauss_newton_num_iter)
    : num_matches_((unsigned int)valid_bearings.size()), octaves_(octaves.begin(), octaves.end()), scale_factors_(scale_factors),
      min_num_inliers_(min_num_inliers), random_engine_(make_engine(use_fixed_seed)), gauss_newton_num_iter_(gauss_newton_num_iter) {
    if (octaves.size() != num_matches_ || valid_points.size() != num_matches_) throw std::invalid_argument("pnp_solver: array sizes differ");
    bearings_.resize(3 * (size_t)num_matches_);
    points_.resize(3 * (size_t)num_matches_);
    for (unsigned int i = 0; i < num_matches_; ++i)
        for (int j = 0; j < 3; ++j) bearings_[3 * (size_t)i + j] = valid_bearings[i](j), points_[3 * (size_t)i + j] = valid_points[i](j);
    for (int r = 0; r < 3; ++r) {
        best_trans_cw_(r) = 0.0;
        for (int c = 0; c < 3; ++c) best_rot_cw_(r, c) = r == c ? 1.0 : 0.0;
    }
}

Mat44_t pnp_solver::get_best_cam_pose() const {
    Mat44_t pose = Mat44_t::Identity();
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) pose(r, c) = best_rot_cw_(r, c);
        pose(r, 3) = best_trans_cw_(r);
    }
    return pose;
}

std::vector<uint32_t> pnp_solver::draw(const unsigned int max_num_iter) {
    std::vector<uint32_t> samples(4 * (size_t)max_num_iter, 0u);
    if (num_matches_ < 4 || num_matches_ < min_num_inliers_) return samples;  // (:49-52: the reference returns before it draws)
    for (unsigned int iter = 0; iter < max_num_iter; ++iter) draw_distinct(4, 0U, num_matches_ - 1, random_engine_, &samples[4 * (size_t)iter]);
    return samples;
}

void pnp_solver::find_via_ransac(const unsigned int max_num_iter, const bool recompute) {
    find_via_ransac_batch({this}, max_num_iter, recompute);
}

void pnp_solver::find_via_ransac_batch(const std::vector<pnp_solver*>& solvers, const unsigned int max_num_iter, const bool recompute) {
    const int P = (int)solvers.size();
    if (P == 0) return;
    std::vector<int32_t> off(P + 1, 0), octaves;
    std::vector<double> bearings, points;
    std::vector<uint32_t> samples;
    for (int p = 0; p < P; ++p) {
        pnp_solver& s = *solvers[p];
        if (s.min_num_inliers_ != solvers[0]->min_num_inliers_ || s.gauss_newton_num_iter_ != solvers[0]->gauss_newton_num_iter_
            || s.scale_factors_ != solvers[0]->scale_factors_)
            throw std::invalid_argument("pnp_solver::find_via_ransac_batch: the solvers of one batch share min_num_inliers, gauss_newton_num_iter and scale_factors");
        off[p + 1] = off[p] + (int32_t)s.num_matches_;
        bearings.insert(bearings.end(), s.bearings_.begin(), s.bearings_.end());
        points.insert(points.end(), s.points_.begin(), s.points_.end());
        octaves.insert(octaves.end(), s.octaves_.begin(), s.octaves_.end());
        const auto drawn = s.draw(max_num_iter);
        samples.insert(samples.end(), drawn.begin(), drawn.end());
    }
    std::vector<uint8_t> valid(P), is_inlier(std::max<size_t>(off[P], 1));
    std::vector<double> pose(12 * (size_t)P);
    std::vector<int32_t> best(P);
    const pnp_solver& s0 = *solvers[0];
    stella_vslam::hip::check(
        svgpu_pnp_ransac_batch(stella_vslam::hip::context(), P, off.data(), bearings.data(), points.data(), octaves.data(), s0.scale_factors_.data(),
                               (int)s0.scale_factors_.size(), (int)s0.min_num_inliers_, (int)max_num_iter, samples.data(), recompute ? 1 : 0,
                               (int)s0.gauss_newton_num_iter_, valid.data(), pose.data(), is_inlier.data(), best.data(), nullptr, nullptr, nullptr),
        "svgpu_pnp_ransac_batch");
    for (int p = 0; p < P; ++p) {
        pnp_solver& s = *solvers[p];
        s.solution_is_valid_ = valid[p] != 0;
        s.best_iter_ = best[p];
        const bool ran = !(s.num_matches_ < 4 || s.num_matches_ < s.min_num_inliers_);
        if (ran) s.is_inlier_match.assign(is_inlier.begin() + off[p], is_inlier.begin() + off[p + 1]);  // (:55; untouched when the call returns at :49-52)
        if (!s.solution_is_valid_) continue;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) s.best_rot_cw_(r, c) = pose[12 * (size_t)p + 4 * r + c];
            s.best_trans_cw_(r) = pose[12 * (size_t)p + 4 * r + 3];
        }
    }
}

}  // namespace hip
}  // namespace solve
}  // namespace stella_vslam
