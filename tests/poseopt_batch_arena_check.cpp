// Host-only check of the scratch layout of svgpu_pose_optimize_batch (stella_vslam_amd/csrc/poseopt_batch_layout.h): built and run by
// tests/test_poseopt_batch_arena.py.  Both runs of the layout (measuring, placing) are made over a host buffer (pointers compared, never
// dereferenced) for the smallest and the largest batch of tests/test_gpu_poseopt_batch.py: every piece lies inside the measured size, pieces
// do not overlap, and one byte less overflows.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "poseopt_batch_layout.h"

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                  \
        }                                                                \
    } while (0)

using Piece = std::pair<const void*, size_t>;  // start, bytes the kernel or a copy touches

static void check(size_t P, size_t n) {
    PoseOptBatchPieces M{};
    const size_t need = arena_measure([&](Arena& A) { poseopt_batch_layout(A, P, n, M); });
    CHECK(M.obs_off == nullptr && M.flags == nullptr);
    std::vector<char> buf(need + 512);
    PoseOptBatchPieces Y{};
    Arena A(buf.data(), need);
    poseopt_batch_layout(A, P, n, Y);
    CHECK(!A.overflow && A.off == need);
    std::vector<Piece> pieces = {{Y.obs_off, (P + 1) * 4}, {Y.pose_in, P * 96}, {Y.active, P}, {Y.pos_w, n * 24}, {Y.uvr, n * 12}, {Y.w, n * 4},
                                 {Y.huber, n * 4}, {Y.select, n}, {Y.c_pos, n * 24}, {Y.c_uvr, n * 12}, {Y.c_w, n * 4}, {Y.c_huber, n * 4},
                                 {Y.entry_of, n * 4}, {Y.level, n}, {Y.robust, n}, {Y.outlier, n}, {Y.pose_out, P * 96}, {Y.result, P * 16}, {Y.flags, n}};
    std::sort(pieces.begin(), pieces.end());
    const char* end = buf.data();
    for (const Piece& p : pieces) {
        if (!p.second) continue;
        const char* b = (const char*)p.first;
        CHECK(b != nullptr && b >= end && b + p.second <= buf.data() + need);
        if (b) end = b + p.second;
    }
    // the results lie next to one another, in this order: one copy brings them back
    if (n) CHECK((const char*)Y.pose_out < (const char*)Y.result && (const char*)Y.result < (const char*)Y.flags && (const char*)Y.flags + n == buf.data() + need - (pad(n) - n));
    std::printf("ok P %zu n %zu: %zu bytes, %zu pieces\n", P, n, need, pieces.size());
    Arena S(buf.data(), need - 1);
    PoseOptBatchPieces Z{};
    poseopt_batch_layout(S, P, n, Z);
    CHECK(S.overflow);
}

int main() {
    check(1, 0);       // one empty problem: the smallest batch of the GPU test
    check(1, 5);       // the smallest problem that is optimised
    check(2, 366);     // the equirectangular call
    check(2, 370);     // the stereo call
    check(16, 3279);   // every perspective class in one batch
    check(300, 19500); // 300 copies of the 65-entry problem: the largest batch of the GPU test
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("poseopt batch arena ok\n");
    return 0;
}
