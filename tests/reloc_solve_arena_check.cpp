// Host-only check of the scratch layout of svgpu_reloc_solve_batch (stella_vslam_amd/csrc/reloc_solve_layout.h), built and run by
// tests/test_reloc_solve_problem_classes.py: the checks of tests/layout_check.h (pieces counted, aligned, non-overlapping, the total equal
// to the sum) for K = 0, 1, 5, candidates without matches and candidates without keyframe entries; that the call's own uploads and the
// refine call's lie in front of every device-only piece, that the results of all steps lie next to one another in front of the lists,
// and that nothing in front of the lists moves with their capacity.
#include <cstdint>

#include "layout_check.h"
#include "reloc_solve_layout.h"

static void check(size_t K, size_t nt, size_t N, size_t M, size_t I, size_t act, size_t S, bool xright, bool recompute, size_t cap) {
    char name[112];
    std::snprintf(name, sizeof name, "K %zu nt %zu N %zu M %zu I %zu S %zu cap %zu", K, nt, N, M, I, S, cap);
    RelocSolveShape H;
    H.refine.K = K, H.refine.nt = nt, H.refine.N = N, H.refine.S = S, H.refine.ncell = 64 * 48;
    H.refine.has_angle = true, H.refine.has_xright = xright, H.refine.has_kf_angle = true, H.refine.global_replay = false;
    H.refine.cand_rec = 312, H.refine.replay_rec = 24, H.refine.cap = cap;
    H.M = M, H.I = I, H.num_active = act, H.recompute = recompute;
    const size_t E = K * nt, hyp = K * I;
    layout_check<RelocSolvePieces>(
        name, [&](Arena& A, RelocSolvePieces& Z) { reloc_solve_layout(A, H, Z); },
        [&](const RelocSolvePieces& Z) {
            const RelocRefinePieces& Y = Z.refine;
            return Rows{{Z.t_bearings, nt * 24}, {Z.m_keypt, M * 4}, {Z.m_kf_entry, M * 4}, {Z.pnp.pos_w, M * 24}, {Z.pnp.match_off, (K + 1) * 4},
                        {Z.pnp.samples, hyp * 16}, {Z.pnp.active, act * 4}, {Z.pnp.bearings, M * 24}, {Z.pnp.max_cos, M * 4}, {Z.pnp.hyp_pose, hyp * 96},
                        {Z.pnp.hyp_num_inliers, hyp * 4}, {Z.pnp.hyp_cost, hyp * 8}, {Z.pnp.hyp_inlier, I * M}, {Z.pnp.inl_idx, recompute ? M * 4 : 0},
                        {Z.pnp.inl_count, recompute ? K * 4 : 0}, {Z.o_uvr, M * 12}, {Z.o_w, M * 4}, {Z.o_huber, M * 4}, {Z.oc_pos, M * 24},
                        {Z.oc_uvr, M * 12}, {Z.oc_w, M * 4}, {Z.oc_huber, M * 4}, {Z.o_entry_of, M * 4}, {Z.o_level, M}, {Z.o_robust, M}, {Z.o_outlier, M},
                        {Z.pnp.valid, K}, {Z.pnp.pose, K * 96}, {Z.pnp.is_inlier, M}, {Z.pnp.best_iter, K * 4}, {Z.opt_pose, K * 96},
                        {Z.opt_result, K * 16}, {Z.opt_flags, M},
                        // the refine call's pieces, as tests/reloc_refine_arena_check.cpp lists them
                        {Y.tdesc, nt * 32}, {Y.t_xy, nt * 8}, {Y.t_octave, nt * 4}, {Y.t_angle, nt * 4}, {Y.t_xright, xright ? nt * 4 : 0}, {Y.pose_in, K * 96},
                        {Y.active, K}, {Y.count0, K * 4}, {Y.occupied, E}, {Y.lm_pos, E * 24}, {Y.kf_off, (K + 1) * 4}, {Y.obs_off, (K + 1) * 4},
                        {Y.pos_w, N * 24}, {Y.valid, N}, {Y.min_d, N * 4}, {Y.max_d, N * 4}, {Y.kf_angle, N * 4}, {Y.lm_desc, N * 32},
                        {Y.cand_tab, S * K * 312}, {Y.replay_tab, K * 24}, {Y.uvr, E * 12}, {Y.w, E * 4}, {Y.huber, E * 4}, {Y.c_pos, E * 24},
                        {Y.c_uvr, E * 12}, {Y.c_w, E * 4}, {Y.c_huber, E * 4}, {Y.entry_of, E * 4}, {Y.level, E}, {Y.robust, E}, {Y.outlier, E},
                        {Y.visible, N}, {Y.q_xy, N * 8}, {Y.q_margin, N * 4}, {Y.q_min_level, N * 4}, {Y.q_max_level, N * 4}, {Y.cell_of, nt * 4},
                        {Y.cell_off, (64 * 48 + 1) * 4}, {Y.cell_items, nt * 4}, {Y.cand_off, (N + 1) * 4}, {Y.match_q, N * 4}, {Y.owner, 0},
                        {Y.match_of_row, 0}, {Y.status, K * 4}, {Y.pose_stage, S * K * 96}, {Y.match_kf, N * 4}, {Y.match_stage, N * 4},
                        {Y.num_found, K * S * 4}, {Y.result, S * K * 16}, {Y.flags, S * E}, {Y.cand_idx, cap * 4}, {Y.dist, cap * 4}};
        },
        [&](const RelocSolvePieces& Z, const char* base, size_t need) {
            const RelocRefinePieces& Y = Z.refine;
            auto at = [](const void* p) { return (const char*)p; };
            // uploads first: the call's own, then the refine call's front; device-only pieces of PnP and the optimiser behind them
            CHECK(at(Z.t_bearings.p) == base);
            CHECK(at(Z.pnp.match_off.p) < at(Y.tdesc.p) && at(Y.replay_tab.p) < at(Y.uvr.p) && at(Y.cand_off.p) < at(Z.pnp.bearings.p));
            // the results of every step next to one another: PnP's, the first optimisation's, the refine call's, then the lists
            CHECK(at(Z.o_outlier.p) + pad(M) == at(Z.pnp.valid.p) || M == 0);
            CHECK(at(Z.pnp.valid.p) < at(Z.pnp.pose.p) && at(Z.pnp.pose.p) < at(Z.pnp.best_iter.p) && at(Z.pnp.best_iter.p) < at(Z.opt_pose.p));
            CHECK(at(Z.opt_pose.p) < at(Z.opt_result.p) && at(Z.opt_result.p) + pad(K * 16) + pad(M) == at(Y.status.p));
            CHECK(at(Y.flags.p) + pad(S * E) == at(Y.cand_idx.p));
            CHECK(at(Y.dist.p) + pad(cap * 4) == base + need);
            RelocSolveShape H2 = H;
            H2.refine.cap = 3 * cap + 1000;
            const size_t need2 = arena_measure([&](Arena& A) { RelocSolvePieces W; reloc_solve_layout(A, H2, W); });
            CHECK(need2 - 2 * pad(H2.refine.cap * 4) == need - 2 * pad(cap * 4));
        });
}

int main() {
    {  // K = 0: the call returns before it lays anything out; the layout itself still adds up (offset tables of one entry, the lists)
        RelocSolveShape H;
        H.refine.ncell = 64 * 48, H.refine.cap = 4096;
        RelocSolvePieces Z;
        const size_t need = arena_measure([&](Arena& A) { reloc_solve_layout(A, H, Z); });
        CHECK(need == pad(4) * 4 + pad((64 * 48 + 1) * 4) + 2 * pad(4096 * 4));  // match_off, kf_off, obs_off, cand_off of one entry; the grid; the lists
        CHECK(Z.pnp.match_off.n == 1 && Z.refine.kf_off.n == 1 && Z.m_keypt.n == 0 && Z.opt_pose.n == 0);
        std::printf("ok K 0: %zu bytes\n", need);
    }
    check(1, 320, 300, 60, 12, 1, 2, false, false, 19200);    // one candidate
    check(5, 320, 1500, 300, 12, 5, 2, true, true, 96000);    // five, stereo, with the recompute's pieces
    check(5, 320, 1500, 0, 12, 0, 2, false, false, 96000);    // candidates without a match: PnP runs for nobody
    check(5, 320, 0, 300, 12, 5, 1, false, false, 4096);      // candidates without keyframe entries
    check(16, 2000, 4800, 1600, 30, 16, 2, false, false, 307200);  // the benchmark's shape
    return layout_check_result("reloc solve arena ok");
}
