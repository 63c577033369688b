// Host-only check of the scratch layout of the pose graph's envelope solver (stella_vslam_amd/csrc/posegraph_envelope_layout.h), built and
// run by tests/test_arena_layouts.py: the checks of tests/layout_check.h for the smallest shape and for the 2 049-vertex chain, for the
// solver's pieces alone and where its two callers place them: behind the self-test's system, and behind pg_optimize_layout.
#include <cstdint>

#include "layout_check.h"
#include "posegraph_envelope_layout.h"
#include "posegraph_layout.h"

static Rows env_rows(const PgEnvPieces& Y, size_t nfree, size_t nblocks, size_t pairs, size_t entries) {
    return {{Y.ctl, PG_ENV_LAYOUT_CTL}, {Y.order, nfree * 4}, {Y.rowoff, (nfree + 1) * 4}, {Y.coloff, (nfree + 1) * 4}, {Y.colrows, (nblocks - nfree) * 4},
            {Y.colbase, (nblocks - nfree) * 4}, {Y.blk_src, nblocks * 4}, {Y.pair_off, (pairs + 1) * 4}, {Y.pair_ent, entries * 4}, {Y.pair_flag, pairs * 4},
            {Y.val, nblocks * 392}, {Y.dinv, nfree * 392}, {Y.y, nfree * 56}};
}

static void check_envelope(size_t nfree, size_t nblocks, size_t pairs, size_t entries) {
    char name[96];
    std::snprintf(name, sizeof name, "envelope free %zu blocks %zu pairs %zu entries %zu", nfree, nblocks, pairs, entries);
    layout_check<PgEnvPieces>(name, [&](Arena& A, PgEnvPieces& Y) { pg_envelope_layout(A, nfree, nblocks, pairs, entries, Y); },
                              [&](const PgEnvPieces& Y) { return env_rows(Y, nfree, nblocks, pairs, entries); });
}

static void check_selftest(size_t nfree, size_t nblocks, size_t pairs, size_t entries, size_t input_pairs) {
    char name[96];
    std::snprintf(name, sizeof name, "self-test free %zu blocks %zu input pairs %zu", nfree, nblocks, input_pairs);
    layout_check<PgEnvSelftestPieces>(
        name, [&](Arena& A, PgEnvSelftestPieces& Y) { pg_envelope_selftest_layout(A, nfree, nblocks, pairs, entries, input_pairs, Y); },
        [&](const PgEnvSelftestPieces& Y) {
            Rows rows = env_rows(Y.env, nfree, nblocks, pairs, entries);
            rows.insert(rows.end(), {{Y.ctl, 128}, {Y.diag, nfree * 392}, {Y.blocks, input_pairs * 392}, {Y.rhs, nfree * 56}, {Y.x, nfree * 56}});
            return rows;
        },
        // the solver's pieces follow the caller's system, which the one upload range starts with
        [&](const PgEnvSelftestPieces& Y, const char* base, size_t) { CHECK((const char*)Y.ctl.p == base && (const char*)Y.env.ctl.p > (const char*)Y.x.p); });
}

// svgpu_pose_graph_optimize_ex with the envelope solver: both layouts in one arena, the solver's pieces directly behind the last result
struct DirectPieces {
    PgPieces g;
    PgEnvPieces e;
};
static void check_direct(size_t N, size_t E, size_t nfree, size_t incident, size_t nblocks, size_t pairs, size_t entries) {
    char name[96];
    std::snprintf(name, sizeof name, "optimize N %zu E %zu with envelope free %zu blocks %zu", N, E, nfree, nblocks);
    layout_check<DirectPieces>(
        name,
        [&](Arena& A, DirectPieces& Y) {
            pg_optimize_layout(A, N, E, nfree, incident, Y.g);
            pg_envelope_layout(A, nfree, nblocks, pairs, entries, Y.e);
        },
        [&](const DirectPieces& Y) {
            Rows rows = env_rows(Y.e, nfree, nblocks, pairs, entries);
            rows.insert(rows.end(), {{Y.g.ctl, PG_LAYOUT_CTL}, {Y.g.out_pose, N * 96}});
            return rows;
        },
        [&](const DirectPieces& Y, const char* base, size_t) { CHECK((const char*)Y.g.ctl.p == base && (const char*)Y.e.ctl.p == (const char*)Y.g.out_pose.p + pad(N * 96)); });
}

int main() {
    check_envelope(1, 1, 0, 0);                  // one free vertex, no pair
    check_envelope(2049, 10235, 6142, 6142);     // the chain of 2 049 with window 3 and a far loop pair
    check_envelope(297, 1757, 882, 885);         // class (e)
    check_selftest(1, 1, 0, 0, 0);
    check_selftest(2049, 10235, 6142, 6142, 6142);
    check_direct(300, 897, 297, 1779, 1757, 882, 885);   // class (e)
    return layout_check_result("posegraph envelope arena ok");
}
