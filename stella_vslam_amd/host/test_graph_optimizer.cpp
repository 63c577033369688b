// optimize::hip::graph_optimizer on a stand-in map.  Without an argument: a map of 12 keyframes on a circle with one loop is built here,
// the class is run on two fresh copies of it: poses and landmarks have to come out bit-equal, the root stays, every landmark is
// refreshed once and chi2 falls.  With a file name: the map is read
// from that file (the format tests/test_gpu_posegraph.py writes), the class is run, and poses and landmarks are printed with %.17g.
// A trailing argument "envelope" (or "pcg") selects the linear solver in either mode.
//   n curr_id loop_id min_num_shared_lms fix_scale
//   per keyframe: id parent_id(-1 none) is_root erased, 12 doubles pose_cw (3 x 4, row-major), has_non_corrected + 8 doubles,
//                 has_pre_corrected + 8 doubles, L + L loop-edge ids, C + C (id weight) covisibilities in descending weight
//   M, per loop connection: key id, K, K ids
//   NL, per landmark: id ref_keyframe_id x y z, K, K observing keyframe ids
//   F, per entry of found_lm_to_ref_keyfrm_id: landmark id, keyframe id
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "drop_in/graph_optimizer_hip.h"
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
    camera::perspective cam{camera::setup_type_t::Monocular, 640, 480, 500, 500, 320, 240, 0, 0, 0, 0, 0};
    feature::orb_params orb;
    std::vector<std::shared_ptr<data::keyframe>> kfs;
    std::map<unsigned int, std::shared_ptr<data::keyframe>> by_id;
    std::vector<std::shared_ptr<data::landmark>> lms;
    module::keyframe_Sim3_pairs_t non_corrected, pre_corrected;
    std::map<std::shared_ptr<data::keyframe>, std::set<std::shared_ptr<data::keyframe>>> loop_connections;
    std::unordered_map<unsigned int, unsigned int> found;
    unsigned int curr_id = 0, loop_id = 0, min_shared = 100;
    int fix_scale = 0;
};

bool read_map(std::istream& in, toy_map& M) {
    int n;
    in >> n >> M.curr_id >> M.loop_id >> M.min_shared >> M.fix_scale;
    struct links {
        long long parent;
        std::vector<unsigned int> loop, covis, weight;
    };
    std::vector<links> L(n);
    for (int k = 0; k < n; ++k) {
        unsigned int id;
        int root, erased, has, cnt;
        in >> id >> L[k].parent >> root >> erased;
        auto kf = std::make_shared<data::keyframe>(id, &M.cam, &M.orb);
        kf->graph_node_->owner_keyfrm_ = kf;
        kf->graph_node_->spanning_root_ = root != 0;
        kf->will_be_erased_ = erased != 0;
        Mat44_t T = Mat44_t::Identity();
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) in >> T(i, j);
        kf->set_pose_cw(T);
        double p[8];
        in >> has;
        for (double& v : p) in >> v;
        if (has) M.non_corrected[kf] = g2o::Sim3(p);
        in >> has;
        for (double& v : p) in >> v;
        if (has) M.pre_corrected[kf] = g2o::Sim3(p);
        in >> cnt;
        L[k].loop.resize(cnt);
        for (auto& v : L[k].loop) in >> v;
        in >> cnt;
        L[k].covis.resize(cnt), L[k].weight.resize(cnt);
        for (int j = 0; j < cnt; ++j) in >> L[k].covis[j] >> L[k].weight[j];
        M.kfs.push_back(kf);
        M.by_id[id] = kf;
    }
    for (int k = 0; k < n; ++k) {
        auto& g = *M.kfs[k]->graph_node_;
        if (L[k].parent >= 0) {
            auto p = M.by_id.at((unsigned int)L[k].parent);
            g.spanning_parent_ = p;
            p->graph_node_->spanning_children_.push_back(M.kfs[k]);
        }
        for (auto i : L[k].loop) g.loop_edges_.insert(M.by_id.at(i));
        for (size_t j = 0; j < L[k].covis.size(); ++j) {
            g.covisibilities_.push_back(M.by_id.at(L[k].covis[j]));
            g.num_shared_lms_.push_back(L[k].weight[j]);
        }
    }
    int m;
    in >> m;
    for (int c = 0; c < m; ++c) {
        unsigned int key;
        int cnt;
        in >> key >> cnt;
        auto& s = M.loop_connections[M.by_id.at(key)];
        for (int j = 0; j < cnt; ++j) {
            unsigned int v;
            in >> v;
            s.insert(M.by_id.at(v));
        }
    }
    int nl;
    in >> nl;
    for (int l = 0; l < nl; ++l) {
        unsigned int id, ref;
        Vec3_t p;
        int cnt;
        in >> id >> ref >> p(0) >> p(1) >> p(2) >> cnt;
        auto lm = std::make_shared<data::landmark>(id, p);
        lm->ref_keyfrm_ = M.by_id.at(ref);
        for (int j = 0; j < cnt; ++j) {
            unsigned int k;
            in >> k;
            auto kf = M.by_id.at(k);
            const unsigned int idx = (unsigned int)kf->landmarks_.size();
            kf->landmarks_.push_back(lm);
            kf->frm_obs_.undist_keypts_.emplace_back();
            lm->add_observation(kf, idx);
        }
        M.lms.push_back(lm);
    }
    int f;
    in >> f;
    for (int j = 0; j < f; ++j) {
        unsigned int a, b;
        in >> a >> b;
        M.found[a] = b;
    }
    return (bool)in;
}

// the built-in map as text: 12 keyframes on a circle, chain parents, curr = 11, loop = 0, the last three keyframes pre-corrected
std::string builtin_map() {
    std::ostringstream o;
    o.precision(17);
    const int n = 12;
    o << n << " 11 0 100 0\n";
    std::vector<SvSim3> S(n);
    for (int k = 0; k < n; ++k) {
        const double a = 2.0 * M_PI * k / n * 0.92;
        S[k] = sv_sim3_exp(SvVec7{0.05 * std::sin(3 * a), a, 0.02, 0, 0, 0, 0});
        S[k].t = sv3(4.0 * std::cos(a), 0.2 * std::sin(2 * a), 4.0 * std::sin(a));
    }
    const SvSim3 corr = sv_sim3_exp(SvVec7{0.02, -0.03, 0.01, 0.2, -0.1, 0.15, std::log(1.05)});
    for (int k = 0; k < n; ++k) {
        double pose[12], p8[8];
        sv_sim3_to_pose(S[k], pose);
        o << k << ' ' << (k ? k - 1 : -1) << ' ' << (k == 0) << " 0";
        for (double v : pose) o << ' ' << v;
        const bool pre = k >= 9;
        sv_sim3_store(p8, S[k]);
        o << ' ' << pre;
        for (double v : p8) o << ' ' << v;
        sv_sim3_store(p8, pre ? sv_sim3_mul(corr, S[k]) : S[k]);
        o << ' ' << pre;
        for (double v : p8) o << ' ' << v;
        o << " 0";
        std::vector<std::pair<int, int>> cov;  // (weight, id): neighbours within 3, and the loop side for the last keyframes
        for (int j = 0; j < n; ++j)
            if (j != k && std::abs(j - k) <= 3) cov.push_back({200 - 30 * std::abs(j - k), j});
        if (k >= 10) cov.push_back({105, k - 10}), cov.push_back({60, k - 9});
        if (k <= 1) cov.push_back({105, k + 10});
        if (k >= 1 && k <= 2) cov.push_back({60, k + 9});
        std::sort(cov.rbegin(), cov.rend());
        o << ' ' << cov.size();
        for (auto& c : cov) o << ' ' << c.second << ' ' << c.first;
        o << '\n';
    }
    o << "2 11 2 0 1 10 2 0 1\n";
    const int nl = 40;
    o << nl << '\n';
    for (int l = 0; l < nl; ++l) {
        const int ref = l % n;
        const SvVec3 pc = sv3(0.3 * std::sin(1.0 + l), 0.2 * std::cos(2.0 * l), 3.0 + 0.1 * (l % 7));
        const SvVec3 pw = sv_sim3_map(sv_sim3_inv(S[ref]), pc);
        o << l << ' ' << ref << ' ' << pw.x << ' ' << pw.y << ' ' << pw.z << " 2 " << ref << ' ' << (ref + 1) % n << '\n';
    }
    o << "2 3 11 5 0\n";
    return o.str();
}
}  // namespace

int main(int argc, char** argv) {
    // an optional trailing "envelope" / "pcg" selects the linear solver (graph_optimizer::set_linear_solver); without it: the default
    svgpu_pose_graph_solver solver = SVGPU_PG_SOLVER_PCG;
    if (argc > 1 && (std::string(argv[argc - 1]) == "envelope" || std::string(argv[argc - 1]) == "pcg")) {
        if (std::string(argv[argc - 1]) == "envelope") solver = SVGPU_PG_SOLVER_ENVELOPE;
        --argc;
    }
    toy_map M;
    if (argc > 1) {
        std::ifstream in(argv[1]);
        if (!read_map(in, M)) return 3;
    }
    else {
        std::istringstream in(builtin_map());
        if (!read_map(in, M)) return 3;
    }
    YAML::Node yaml;
    yaml.kv["min_num_shared_lms"] = std::to_string(M.min_shared);
    optimize::hip::graph_optimizer opt(yaml, M.fix_scale != 0);
    opt.set_linear_solver(solver);
    const auto curr = M.by_id.at(M.curr_id), loop = M.by_id.at(M.loop_id);
    std::vector<Mat44_t> before;
    for (auto& kf : M.kfs) before.push_back(kf->get_pose_cw());
    opt.optimize(loop, curr, M.non_corrected, M.pre_corrected, M.loop_connections, M.found);
    if (argc > 1) {
        for (auto& kf : M.kfs) {
            std::printf("KF %u", kf->id_);
            const Mat44_t T = kf->get_pose_cw();
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 4; ++j) std::printf(" %.17g", T(i, j));
            std::printf("\n");
        }
        for (auto& lm : M.lms) {
            const Vec3_t p = lm->get_pos_in_world();
            std::printf("LM %u %.17g %.17g %.17g\n", lm->id_, p(0), p(1), p(2));
        }
        if (solver == SVGPU_PG_SOLVER_PCG)
            std::printf("STATS %d %d %d\n", opt.last_stats_.lm_iterations, opt.last_stats_.lm_trials, opt.last_stats_.stopped_by_gain);
        else  // (the solver that ran and its envelope behind the three figures of the default)
            std::printf("STATS %d %d %d %d %d\n", opt.last_stats_.lm_iterations, opt.last_stats_.lm_trials, opt.last_stats_.stopped_by_gain,
                        opt.last_solver_stats_.solver, opt.last_solver_stats_.envelope_blocks);
        return 0;
    }
    // the same run twice on a fresh copy of the map gives the same bits, the fixed keyframes keep their rotation, something moved
    toy_map M2;
    std::istringstream in2(builtin_map());
    CHECK(read_map(in2, M2));
    optimize::hip::graph_optimizer opt2(yaml, false);
    opt2.set_linear_solver(solver);
    opt2.optimize(M2.by_id.at(M2.loop_id), M2.by_id.at(M2.curr_id), M2.non_corrected, M2.pre_corrected, M2.loop_connections, M2.found);
    double moved = 0.0;
    for (size_t k = 0; k < M.kfs.size(); ++k) {
        const Mat44_t a = M.kfs[k]->get_pose_cw(), b = M2.kfs[k]->get_pose_cw();
        CHECK(std::memcmp(a.data(), b.data(), sizeof(double) * 16) == 0);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) moved = std::max(moved, std::fabs(a(i, j) - before[k](i, j)));
        if (M.kfs[k]->id_ == 0)
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 4; ++j) CHECK(std::fabs(a(i, j) - before[k](i, j)) < 1e-12);  // the root is fixed
    }
    for (size_t l = 0; l < M.lms.size(); ++l) {
        const Vec3_t a = M.lms[l]->get_pos_in_world(), b = M2.lms[l]->get_pos_in_world();
        CHECK(std::memcmp(a.data(), b.data(), sizeof(double) * 3) == 0);
        CHECK(M.lms[l]->num_geometry_refreshes_ == 1);
    }
    CHECK(moved > 1e-3);
    CHECK(opt.last_stats_.lm_iterations >= 1 && opt.last_stats_.final_chi2 < opt.last_stats_.initial_chi2);
    std::printf("LM iterations %d, trials %d, chi2 %.6e -> %.6e, largest pose change %.3e\n", opt.last_stats_.lm_iterations, opt.last_stats_.lm_trials,
                opt.last_stats_.initial_chi2, opt.last_stats_.final_chi2, moved);
    if (g_fail) return 1;
    std::printf("graph_optimizer ok\n");
    return 0;
}
