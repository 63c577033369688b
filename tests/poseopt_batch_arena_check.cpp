// Host-only check of the scratch layout of svgpu_pose_optimize_batch (stella_vslam_amd/csrc/poseopt_batch_layout.h), built and run by
// tests/test_arena_layouts.py: the checks of tests/layout_check.h for the smallest and the largest batch of tests/test_gpu_poseopt_batch.py,
// and the adjacency of the three results.
#include <cstdint>

#include "layout_check.h"
#include "poseopt_batch_layout.h"

static void check(size_t P, size_t n) {
    char name[64];
    std::snprintf(name, sizeof name, "P %zu n %zu", P, n);
    layout_check<PoseOptBatchPieces>(
        name, [&](Arena& A, PoseOptBatchPieces& Y) { poseopt_batch_layout(A, P, n, Y); },
        [&](const PoseOptBatchPieces& Y) {
            return Rows{{Y.obs_off, (P + 1) * 4}, {Y.pose_in, P * 96}, {Y.active, P}, {Y.pos_w, n * 24}, {Y.uvr, n * 12}, {Y.w, n * 4},
                        {Y.huber, n * 4}, {Y.select, n}, {Y.c_pos, n * 24}, {Y.c_uvr, n * 12}, {Y.c_w, n * 4}, {Y.c_huber, n * 4},
                        {Y.entry_of, n * 4}, {Y.level, n}, {Y.robust, n}, {Y.outlier, n}, {Y.pose_out, P * 96}, {Y.result, P * 16}, {Y.flags, n}};
        },
        // the results lie next to one another, in this order: one copy brings them back
        [&](const PoseOptBatchPieces& Y, const char* base, size_t need) {
            if (n) CHECK((const char*)Y.pose_out.p < (const char*)Y.result.p && (const char*)Y.result.p < (const char*)Y.flags.p && (const char*)Y.flags.p + n == base + need - (pad(n) - n));
        });
}

int main() {
    check(1, 0);       // one empty problem: the smallest batch of the GPU test
    check(1, 5);       // the smallest problem that is optimised
    check(2, 366);     // the equirectangular call
    check(2, 370);     // the stereo call
    check(16, 3279);   // every perspective class in one batch
    check(300, 19500); // 300 copies of the 65-entry problem: the largest batch of the GPU test
    return layout_check_result("poseopt batch arena ok");
}
