// Host-only check of the scratch layout of svgpu_sim3_transform_optimize_batch (stella_vslam_amd/csrc/sim3opt_layout.h), built and run by
// tests/test_arena_layouts.py: the checks of tests/layout_check.h for the smallest and the largest shape of tests/test_gpu_sim3opt.py.
#include <cstdint>

#include "layout_check.h"
#include "sim3opt_layout.h"

static void check(size_t P, size_t n) {
    char name[64];
    std::snprintf(name, sizeof name, "P %zu n %zu", P, n);
    layout_check<Sim3OptPieces>(name, [&](Arena& A, Sim3OptPieces& Y) { sim3opt_layout(A, P, n, Y); }, [&](const Sim3OptPieces& Y) {
        return Rows{{Y.prob, P * S3O_LAYOUT_PROBLEM}, {Y.obs1, n * 16}, {Y.obs2, n * 16}, {Y.w1, n * 4}, {Y.w2, n * 4}, {Y.pos1, n * 24},
                    {Y.pos2, n * 24}, {Y.chi_cache, n * 16}, {Y.sim3_out, P * 64}, {Y.num_inliers, P * 4}, {Y.status, n},
                    {Y.stats, P * S3O_LAYOUT_STATS}};
    });
}

int main() {
    check(1, 0);      // one empty problem
    check(1, 10);     // the smallest planted case
    check(1, 257);    // the largest
    check(3, 80);     // a batch with an empty problem in the middle
    check(26, 2200);  // every case in one batch
    return layout_check_result("sim3opt arena ok");
}
