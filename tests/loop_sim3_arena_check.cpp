// Host-only check of the scratch layout of svgpu_loop_sim3_batch (stella_vslam_amd/csrc/loop_sim3_layout.h), built and run by
// tests/test_loop_sim3_layout.py: the checks of tests/layout_check.h for the smallest and the largest shapes of tests/test_gpu_loop_sim3.py,
// that the uploads come first, that the results lie next to one another in front of the lists, and that nothing in front of the lists
// moves with their capacity.
#include <cstdint>

#include "layout_check.h"
#include "loop_sim3_layout.h"

static const size_t PROB = 344, REPROJ = 408, CAND = 312, REPLAY = 24, GRID = 152, STATS = 64, NCELL = 64 * 48;

static void check(size_t K, size_t n1, size_t N2, bool scale_in, size_t owner, size_t mrow, size_t cap) {
    char name[96];
    std::snprintf(name, sizeof name, "K %zu n1 %zu N2 %zu cap %zu", K, n1, N2, cap);
    LoopSim3Shape H;
    H.K = K, H.n1 = n1, H.N2 = N2, H.ncell = NCELL, H.has_scale_in = scale_in, H.owner_ints = owner, H.mrow_ints = mrow;
    H.prob_rec = PROB, H.reproj_rec = REPROJ, H.cand_rec = CAND, H.replay_rec = REPLAY, H.grid_rec = GRID, H.stats_rec = STATS, H.cap = cap;
    const size_t E = K * n1, R = E + N2, T = N2 + n1;
    layout_check<LoopSim3Pieces>(
        name, [&](Arena& A, LoopSim3Pieces& Y) { loop_sim3_layout(A, H, Y); },
        [&](const LoopSim3Pieces& Y) {
            return Rows{{Y.desc1, n1 * 32}, {Y.lm_desc1, n1 * 32}, {Y.xy1, n1 * 8}, {Y.octave1, n1 * 4}, {Y.pos_w1, n1 * 24}, {Y.has_lm1, n1}, {Y.min1, n1 * 4},
                        {Y.max1, n1 * 4}, {Y.desc2, N2 * 32}, {Y.lm_desc2, N2 * 32}, {Y.xy2, N2 * 8}, {Y.octave2, N2 * 4}, {Y.pos_w2, N2 * 24}, {Y.has_lm2, N2},
                        {Y.min2, N2 * 4}, {Y.max2, N2 * 4}, {Y.kf2_off, (K + 1) * 4}, {Y.set_base, (K + 2) * 4}, {Y.row_base, (2 * K + 1) * 4},
                        {Y.pose_in_cand, K * 96}, {Y.pose_2w, K * 96}, {Y.rot_12, K * 72}, {Y.trans_12, K * 24}, {Y.active, K}, {Y.scale_in, scale_in ? K * 4 : 0},
                        {Y.prob, K * PROB}, {Y.reproj_tab, K * REPROJ}, {Y.grid_tab, (3 * K + 1) * GRID}, {Y.cand_tab, 2 * K * CAND}, {Y.replay_tab, 2 * K * REPLAY},
                        {Y.prior_state, E}, {Y.prior_idx2, E * 4}, {Y.prior_pos_w, E * 24}, {Y.ratio_bits, E * 4}, {Y.xf, K * 192}, {Y.live, K}, {Y.already2, N2},
                        {Y.cell_cnt, ((K + 1) * NCELL + 1) * 4}, {Y.cell_of, T * 4}, {Y.cell_items, T * 4}, {Y.visible, R}, {Y.q_xy, R * 8}, {Y.q_margin, R * 4},
                        {Y.q_min_level, R * 4}, {Y.q_max_level, R * 4}, {Y.cand_off, (R + 1) * 4}, {Y.owner, owner * 4}, {Y.match_of_row, mrow * 4},
                        {Y.num_ab, 2 * K * 4}, {Y.obs1, E * 16}, {Y.obs2, E * 16}, {Y.w1, E * 4}, {Y.w2, E * 4}, {Y.pos1, E * 24}, {Y.pos2, E * 24},
                        {Y.chi_cache, E * 16}, {Y.scale, K * 4}, {Y.code, K * 4}, {Y.match_a, E * 4}, {Y.match_b, N2 * 4}, {Y.mutual, E * 4}, {Y.num_mutual, K * 4},
                        {Y.num_edges, K * 4}, {Y.edge_idx1, E * 4}, {Y.edge_idx2, E * 4}, {Y.edge_status, E}, {Y.sim3_out, K * 64}, {Y.num_inliers, K * 4},
                        {Y.stats, K * STATS}, {Y.cand_idx, cap * 4}, {Y.dist, cap * 4}};
        },
        [&](const LoopSim3Pieces& Y, const char* base, size_t need) {
            // the uploads come first (one copy of the touched range), the results lie together in front of the lists, the lists are last
            CHECK((const char*)Y.desc1.p == base);
            CHECK((const char*)Y.prior_pos_w.p < (const char*)Y.ratio_bits.p);
            CHECK((const char*)Y.chi_cache.p < (const char*)Y.scale.p && (const char*)Y.scale.p < (const char*)Y.match_a.p);
            CHECK((const char*)Y.match_a.p < (const char*)Y.sim3_out.p && (const char*)Y.sim3_out.p < (const char*)Y.stats.p);
            CHECK((const char*)Y.stats.p + pad(K * STATS) == (const char*)Y.cand_idx.p);
            CHECK((const char*)Y.dist.p + pad(cap * 4) == base + need);
            // longer lists move nothing else
            LoopSim3Shape H2 = H;
            H2.cap = 3 * cap + 1000;
            const size_t need2 = arena_measure([&](Arena& M) { LoopSim3Pieces Z; loop_sim3_layout(M, H2, Z); });
            CHECK(need2 - 2 * pad(H2.cap * 4) == need - 2 * pad(cap * 4));
        });
}

int main() {
    check(1, 150, 20, false, 0, 0, 10880);          // the smallest: a scale class
    check(1, 1100, 20, false, 0, 0, 71680);         // more kept ratios than a workgroup has threads
    check(4, 320, 551, false, 0, 0, 117184);        // unequal keyframes, one of them empty
    check(2, 320, 500, true, 0, 0, 72960);          // scale_12_in
    check(40, 150, 1200, false, 0, 0, 460800);      // the largest: many tiny candidates
    check(10, 2000, 20000, false, 44000, 44000, 2560000);  // the benchmark's shape, with a global-memory replay's tables
    return layout_check_result("loop sim3 arena ok");
}
