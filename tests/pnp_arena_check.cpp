// Host-only check of the PnP scratch layouts (stella_vslam_amd/csrc/pnp_layout.h), built and run by tests/test_arena_layouts.py: the
// checks of tests/layout_check.h for the smallest and the largest shape of tests/test_gpu_pnp.py.
#include <cstdint>

#include "layout_check.h"
#include "pnp_layout.h"

static void check_ransac(size_t P, size_t n, size_t I, size_t act, bool recompute) {
    char name[96];
    std::snprintf(name, sizeof name, "ransac P %zu n %zu I %zu active %zu recompute %d", P, n, I, act, (int)recompute);
    layout_check<PnpRansacPieces>(name, [&](Arena& A, PnpRansacPieces& Y) { pnp_ransac_layout(A, P, n, I, act, recompute, Y); }, [&](const PnpRansacPieces& Y) {
        return Rows{{Y.bearings, n * 24}, {Y.pos_w, n * 24}, {Y.max_cos, n * 4}, {Y.match_off, (P + 1) * 4}, {Y.samples, P * I * 16}, {Y.active, act * 4},
                    {Y.hyp_pose, P * I * 96}, {Y.hyp_num_inliers, P * I * 4}, {Y.hyp_cost, P * I * 8}, {Y.hyp_inlier, I * n}, {Y.valid, P}, {Y.pose, P * 96},
                    {Y.is_inlier, n}, {Y.best_iter, P * 4}, {Y.inl_idx, recompute ? n * 4 : 0}, {Y.inl_count, recompute ? P * 4 : 0}};
    });
}

static void check_pose(size_t sets, size_t n) {
    char name[64];
    std::snprintf(name, sizeof name, "pose sets %zu n %zu", sets, n);
    layout_check<PnpPosePieces>(name, [&](Arena& A, PnpPosePieces& Y) { pnp_pose_layout(A, sets, n, Y); }, [&](const PnpPosePieces& Y) {
        return Rows{{Y.bearings, n * 24}, {Y.pos_w, n * 24}, {Y.off, (sets + 1) * 4}, {Y.pose, sets * 96}, {Y.err, sets * 8}};
    });
}

int main() {
    check_pose(1, 4);          // the smallest set
    check_pose(54, 4545);      // the over-determined classes in one call
    check_ransac(1, 4, 1, 1, false);
    check_ransac(1, 80, 30, 1, true);
    check_ransac(17, 1292, 30, 12, true);   // the 17-problem batch
    check_ransac(17, 1292, 30, 12, false);
    return layout_check_result("pnp arena ok");
}
