// Host-only check of the pose-graph scratch layouts (stella_vslam_amd/csrc/posegraph_layout.h): built and run by
// tests/test_posegraph_arena.py.  Both runs of a layout (measuring, placing) are made over a host buffer (pointers compared, never
// dereferenced) for the smallest and the largest shape of tests/test_gpu_posegraph.py: every piece lies inside the measured size, pieces
// do not overlap, and one byte less overflows.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "posegraph_layout.h"

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

static void check_optimize(size_t N, size_t E, size_t nfree, size_t incident) {
    PgPieces M{};
    const size_t need = arena_measure([&](Arena& A) { pg_optimize_layout(A, N, E, nfree, incident, M); });
    CHECK(M.ctl == nullptr && M.rec == nullptr);
    std::vector<char> buf(need + 512);
    PgPieces Y{};
    Arena A(buf.data(), need);
    pg_optimize_layout(A, N, E, nfree, incident, Y);
    CHECK(!A.overflow && A.off == need);
    const size_t n = 7 * nfree;
    char name[96];
    std::snprintf(name, sizeof name, "optimize N %zu E %zu free %zu incident %zu", N, E, nfree, incident);
    check_pieces(name, buf.data(), need,
                 {{Y.ctl, PG_LAYOUT_CTL}, {Y.est0, N * 64}, {Y.fixed, N}, {Y.slot, N * 4}, {Y.e_i, E * 4}, {Y.e_j, E * 4}, {Y.meas, E * 64},
                  {Y.v_off, (nfree + 1) * 4}, {Y.v_ent, incident * 4}, {Y.est1, N * 64}, {Y.rec, E * PG_LAYOUT_REC * 8}, {Y.chi_trial, E * 8},
                  {Y.Hd, nfree * 392}, {Y.b, n * 8}, {Y.maxd, nfree * 8}, {Y.Minv, nfree * 392}, {Y.x, n * 8}, {Y.r, n * 8}, {Y.z, n * 8},
                  {Y.p, n * 8}, {Y.Ap, n * 8}, {Y.scale_part, nfree * 8}, {Y.out_sim3, N * 64}, {Y.out_pose, N * 96}});
    Arena S(buf.data(), need - 1);
    PgPieces Z{};
    pg_optimize_layout(S, N, E, nfree, incident, Z);
    CHECK(S.overflow);
}

static void check_landmarks(size_t N, size_t L) {
    PgLandmarkPieces M{};
    const size_t need = arena_measure([&](Arena& A) { pg_landmarks_layout(A, N, L, M); });
    std::vector<char> buf(need + 512);
    PgLandmarkPieces Y{};
    Arena A(buf.data(), need);
    pg_landmarks_layout(A, N, L, Y);
    CHECK(!A.overflow && A.off == need);
    char name[64];
    std::snprintf(name, sizeof name, "landmarks N %zu L %zu", N, L);
    check_pieces(name, buf.data(), need, {{Y.before, N * 64}, {Y.after, N * 64}, {Y.ref, L * 4}, {Y.pos_in, L * 24}, {Y.pos_out, L * 24}});
}

int main() {
    check_optimize(2, 2, 1, 2);            // class (a)
    check_optimize(4, 4, 2, 5);            // class (g): an edge between two fixed vertices
    check_optimize(65, 130, 64, 256);      // the largest ring
    check_optimize(300, 897, 297, 1779);   // class (e)
    check_landmarks(8, 1);
    check_landmarks(8, 1000);
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("posegraph arena ok\n");
    return 0;
}
