// Host-only check of the pose-graph scratch layouts (stella_vslam_amd/csrc/posegraph_layout.h), built and run by
// tests/test_arena_layouts.py: the checks of tests/layout_check.h for the smallest and the largest shape of tests/test_gpu_posegraph.py.
#include <cstdint>

#include "layout_check.h"
#include "posegraph_layout.h"

static void check_optimize(size_t N, size_t E, size_t nfree, size_t incident) {
    const size_t n = 7 * nfree;
    char name[96];
    std::snprintf(name, sizeof name, "optimize N %zu E %zu free %zu incident %zu", N, E, nfree, incident);
    layout_check<PgPieces>(name, [&](Arena& A, PgPieces& Y) { pg_optimize_layout(A, N, E, nfree, incident, Y); }, [&](const PgPieces& Y) {
        return Rows{{Y.ctl, PG_LAYOUT_CTL}, {Y.est0, N * 64}, {Y.fixed, N}, {Y.slot, N * 4}, {Y.e_i, E * 4}, {Y.e_j, E * 4}, {Y.meas, E * 64},
                    {Y.v_off, (nfree + 1) * 4}, {Y.v_ent, incident * 4}, {Y.est1, N * 64}, {Y.rec, E * PG_LAYOUT_REC * 8}, {Y.chi_trial, E * 8},
                    {Y.Hd, nfree * 392}, {Y.b, n * 8}, {Y.maxd, nfree * 8}, {Y.Minv, nfree * 392}, {Y.x, n * 8}, {Y.r, n * 8}, {Y.z, n * 8},
                    {Y.p, n * 8}, {Y.Ap, n * 8}, {Y.scale_part, nfree * 8}, {Y.out_sim3, N * 64}, {Y.out_pose, N * 96}};
    });
}

static void check_landmarks(size_t N, size_t L) {
    char name[64];
    std::snprintf(name, sizeof name, "landmarks N %zu L %zu", N, L);
    layout_check<PgLandmarkPieces>(name, [&](Arena& A, PgLandmarkPieces& Y) { pg_landmarks_layout(A, N, L, Y); }, [&](const PgLandmarkPieces& Y) {
        return Rows{{Y.before, N * 64}, {Y.after, N * 64}, {Y.ref, L * 4}, {Y.pos_in, L * 24}, {Y.pos_out, L * 24}};
    });
}

int main() {
    check_optimize(2, 2, 1, 2);            // class (a)
    check_optimize(4, 4, 2, 5);            // class (g): an edge between two fixed vertices
    check_optimize(65, 130, 64, 256);      // the largest ring
    check_optimize(300, 897, 297, 1779);   // class (e)
    check_landmarks(8, 1);
    check_landmarks(8, 1000);
    return layout_check_result("posegraph arena ok");
}
