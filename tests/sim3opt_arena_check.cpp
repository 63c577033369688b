// Host-only check of the scratch layout of svgpu_sim3_transform_optimize_batch (stella_vslam_amd/csrc/sim3opt_layout.h): built and run by
// tests/test_sim3opt_arena.py.  Both runs of the layout (measuring, placing) are made over a host buffer (pointers compared, never
// dereferenced) for the smallest and the largest shape of tests/test_gpu_sim3opt.py: every piece lies inside the measured size, pieces do
// not overlap, and one byte less overflows.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "sim3opt_layout.h"

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                  \
        }                                                                \
    } while (0)

using Piece = std::pair<const void*, size_t>;  // start, bytes the kernel touches

static void check(size_t P, size_t n) {
    Sim3OptPieces M{};
    const size_t need = arena_measure([&](Arena& A) { sim3opt_layout(A, P, n, M); });
    CHECK(M.prob == nullptr && M.status == nullptr);
    std::vector<char> buf(need + 512);
    Sim3OptPieces Y{};
    Arena A(buf.data(), need);
    sim3opt_layout(A, P, n, Y);
    CHECK(!A.overflow && A.off == need);
    std::vector<Piece> pieces = {{Y.prob, P * S3O_LAYOUT_PROBLEM}, {Y.obs1, n * 16}, {Y.obs2, n * 16}, {Y.w1, n * 4}, {Y.w2, n * 4}, {Y.pos1, n * 24},
                                 {Y.pos2, n * 24}, {Y.chi_cache, n * 16}, {Y.sim3_out, P * 64}, {Y.num_inliers, P * 4}, {Y.status, n},
                                 {Y.stats, P * S3O_LAYOUT_STATS}};
    std::sort(pieces.begin(), pieces.end());
    const char* end = buf.data();
    for (const Piece& p : pieces) {
        if (!p.second) continue;
        const char* b = (const char*)p.first;
        CHECK(b != nullptr && b >= end && b + p.second <= buf.data() + need);
        if (b) end = b + p.second;
    }
    std::printf("ok P %zu n %zu: %zu bytes, %zu pieces\n", P, n, need, pieces.size());
    Arena S(buf.data(), need - 1);
    Sim3OptPieces Z{};
    sim3opt_layout(S, P, n, Z);
    CHECK(S.overflow);
}

int main() {
    check(1, 0);      // one empty problem
    check(1, 10);     // the smallest planted case
    check(1, 257);    // the largest
    check(3, 80);     // a batch with an empty problem in the middle
    check(26, 2200);  // every case in one batch
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("sim3opt arena ok\n");
    return 0;
}
