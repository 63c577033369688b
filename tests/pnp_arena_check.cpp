// Host-only check of the PnP scratch layouts (stella_vslam_amd/csrc/pnp_layout.h): built and run by tests/test_pnp_arena.py.
// The entry points size the arena by running the layout on a measuring arena and place the pieces by running the same layout on the
// buffer; here both runs are made over a host buffer (pointers compared, never dereferenced) for the smallest and the largest shape of
// tests/test_gpu_pnp.py: every piece lies inside the measured size, pieces do not overlap, and one byte less overflows.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "pnp_layout.h"

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                  \
        }                                                                \
    } while (0)

using Piece = std::pair<const void*, size_t>;  // start, bytes the kernels touch

static void check_pieces(const char* name, char* base, size_t need, std::vector<Piece> pieces) {
    std::sort(pieces.begin(), pieces.end());
    const char* end = base;
    for (const Piece& p : pieces) {
        if (!p.second) continue;
        const char* b = (const char*)p.first;
        CHECK(b != nullptr && b >= end && b + p.second <= base + need);
        if (b) end = b + p.second;
    }
    std::printf("ok %s: %zu bytes, %zu pieces\n", name, need, pieces.size());
}

static void check_ransac(size_t P, size_t n, size_t I, size_t act, bool recompute) {
    PnpRansacPieces M{};
    const size_t need = arena_measure([&](Arena& A) { pnp_ransac_layout(A, P, n, I, act, recompute, M); });
    CHECK(M.bearings == nullptr && M.hyp_inlier == nullptr);
    std::vector<char> buf(need + 512);
    PnpRansacPieces Y{};
    Arena A(buf.data(), need);
    pnp_ransac_layout(A, P, n, I, act, recompute, Y);
    CHECK(!A.overflow && A.off == need);
    char name[96];
    std::snprintf(name, sizeof name, "ransac P %zu n %zu I %zu active %zu recompute %d", P, n, I, act, (int)recompute);
    check_pieces(name, buf.data(), need,
                 {{Y.bearings, n * 24}, {Y.pos_w, n * 24}, {Y.max_cos, n * 4}, {Y.match_off, (P + 1) * 4}, {Y.samples, P * I * 16}, {Y.active, act * 4},
                  {Y.hyp_pose, P * I * 96}, {Y.hyp_num_inliers, P * I * 4}, {Y.hyp_cost, P * I * 8}, {Y.hyp_inlier, I * n}, {Y.valid, P}, {Y.pose, P * 96},
                  {Y.is_inlier, n}, {Y.best_iter, P * 4}, {Y.inl_idx, recompute ? n * 4 : 0}, {Y.inl_count, recompute ? P * 4 : 0}});
    if (need > 0) {
        Arena S(buf.data(), need - 1);
        PnpRansacPieces Z{};
        pnp_ransac_layout(S, P, n, I, act, recompute, Z);
        CHECK(S.overflow);
    }
}

static void check_pose(size_t sets, size_t n) {
    PnpPosePieces M{};
    const size_t need = arena_measure([&](Arena& A) { pnp_pose_layout(A, sets, n, M); });
    std::vector<char> buf(need + 512);
    PnpPosePieces Y{};
    Arena A(buf.data(), need);
    pnp_pose_layout(A, sets, n, Y);
    CHECK(!A.overflow && A.off == need);
    char name[64];
    std::snprintf(name, sizeof name, "pose sets %zu n %zu", sets, n);
    check_pieces(name, buf.data(), need, {{Y.bearings, n * 24}, {Y.pos_w, n * 24}, {Y.off, (sets + 1) * 4}, {Y.pose, sets * 96}, {Y.err, sets * 8}});
}

int main() {
    check_pose(1, 4);          // the smallest set
    check_pose(54, 4545);      // the over-determined classes in one call
    check_ransac(1, 4, 1, 1, false);
    check_ransac(1, 80, 30, 1, true);
    check_ransac(17, 1292, 30, 12, true);   // the 17-problem batch
    check_ransac(17, 1292, 30, 12, false);
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("pnp arena ok\n");
    return 0;
}
