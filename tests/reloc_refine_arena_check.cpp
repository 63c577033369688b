// Host-only check of the scratch layout of svgpu_reloc_refine_batch (stella_vslam_amd/csrc/reloc_refine_layout.h), built and run by
// tests/test_reloc_refine_problem_classes.py: the checks of tests/layout_check.h for the shapes of tests/test_gpu_reloc_refine.py, that the
// results lie next to one another in front of the lists, and that nothing in front of the lists moves with their capacity.
#include <cstdint>

#include "layout_check.h"
#include "reloc_refine_layout.h"

static RelocRefineShape shape(size_t K, size_t nt, size_t N, size_t S, bool angle, bool xright, bool global_replay, size_t cap) {
    RelocRefineShape H;
    H.K = K, H.nt = nt, H.N = N, H.S = S, H.ncell = 64 * 48;
    H.has_angle = angle, H.has_xright = xright, H.has_kf_angle = angle, H.global_replay = global_replay;
    H.cand_rec = 312, H.replay_rec = 24, H.cap = cap;
    return H;
}

static void check(size_t K, size_t nt, size_t N, size_t S, bool angle, bool xright, bool global_replay, size_t cap) {
    char name[96];
    std::snprintf(name, sizeof name, "K %zu nt %zu N %zu S %zu cap %zu", K, nt, N, S, cap);
    const RelocRefineShape H = shape(K, nt, N, S, angle, xright, global_replay, cap);
    const size_t E = K * nt;
    layout_check<RelocRefinePieces>(
        name, [&](Arena& A, RelocRefinePieces& Y) { reloc_refine_layout(A, H, Y); },
        [&](const RelocRefinePieces& Y) {
            return Rows{{Y.tdesc, nt * 32}, {Y.t_xy, nt * 8}, {Y.t_octave, nt * 4}, {Y.t_angle, angle ? nt * 4 : 0}, {Y.t_xright, xright ? nt * 4 : 0},
                        {Y.pose_in, K * 96}, {Y.active, K}, {Y.count0, K * 4}, {Y.occupied, E}, {Y.lm_pos, E * 24}, {Y.kf_off, (K + 1) * 4},
                        {Y.obs_off, (K + 1) * 4}, {Y.pos_w, N * 24}, {Y.valid, N}, {Y.min_d, N * 4}, {Y.max_d, N * 4}, {Y.kf_angle, angle ? N * 4 : 0},
                        {Y.lm_desc, N * 32}, {Y.cand_tab, S * K * 312}, {Y.replay_tab, K * 24}, {Y.uvr, E * 12}, {Y.w, E * 4}, {Y.huber, E * 4},
                        {Y.c_pos, E * 24}, {Y.c_uvr, E * 12}, {Y.c_w, E * 4}, {Y.c_huber, E * 4}, {Y.entry_of, E * 4}, {Y.level, E}, {Y.robust, E},
                        {Y.outlier, E}, {Y.visible, N}, {Y.q_xy, N * 8}, {Y.q_margin, N * 4}, {Y.q_min_level, N * 4}, {Y.q_max_level, N * 4},
                        {Y.cell_of, nt * 4}, {Y.cell_off, (64 * 48 + 1) * 4}, {Y.cell_items, nt * 4}, {Y.cand_off, (N + 1) * 4}, {Y.match_q, N * 4},
                        {Y.owner, global_replay ? E * 4 : 0}, {Y.match_of_row, global_replay ? N * 4 : 0}, {Y.status, K * 4}, {Y.pose_stage, S * K * 96},
                        {Y.match_kf, N * 4}, {Y.match_stage, N * 4}, {Y.num_found, K * S * 4}, {Y.result, S * K * 16}, {Y.flags, S * E},
                        {Y.cand_idx, cap * 4}, {Y.dist, cap * 4}};
        },
        [&](const RelocRefinePieces& Y, const char* base, size_t need) {
            // the uploads come first (one copy of the touched range), the results lie together in front of the lists, the lists are last
            CHECK((const char*)Y.tdesc.p == base);
            CHECK((const char*)Y.replay_tab.p < (const char*)Y.uvr.p);
            CHECK((const char*)Y.status.p < (const char*)Y.pose_stage.p && (const char*)Y.pose_stage.p < (const char*)Y.num_found.p);
            CHECK((const char*)Y.num_found.p < (const char*)Y.result.p && (const char*)Y.result.p < (const char*)Y.flags.p);
            CHECK((const char*)Y.flags.p + pad(S * E) == (const char*)Y.cand_idx.p);
            CHECK((const char*)Y.dist.p + pad(cap * 4) == base + need);
            // longer lists move nothing else
            RelocRefineShape H2 = H;
            H2.cap = 3 * cap + 1000;
            const size_t need2 = arena_measure([&](Arena& M) { RelocRefinePieces Z; reloc_refine_layout(M, H2, Z); });
            CHECK(need2 - 2 * pad(H2.cap * 4) == need - 2 * pad(cap * 4));
        });
}

int main() {
    check(1, 320, 300, 2, true, false, false, 19200);     // one candidate
    check(6, 320, 1650, 2, true, true, false, 105600);    // every status beside accepted ones, stereo
    check(4, 320, 1100, 4, false, false, false, 70400);   // four stages, no orientation test
    check(260, 64, 10400, 2, true, false, false, 665600); // more candidates than compute units
    check(16, 2000, 4800, 2, true, false, true, 307200);  // the benchmark's shape, with the global-memory replay's tables
    return layout_check_result("reloc refine arena ok");
}
