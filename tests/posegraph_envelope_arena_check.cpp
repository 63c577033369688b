// Host-only check of the scratch layout of the pose graph's envelope solver (stella_vslam_amd/csrc/posegraph_envelope_layout.h): built
// and run by tests/test_posegraph_envelope.py with sv_arena.h alone.  Both runs of a layout (measuring, placing) are made over a host
// buffer (pointers compared, never dereferenced) for the smallest shape and for the 2 049-vertex chain: every piece lies inside the
// measured size, pieces do not overlap, and one byte less overflows.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "posegraph_envelope_layout.h"

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

static std::vector<Piece> env_pieces(const PgEnvPieces& Y, size_t nfree, size_t nblocks, size_t pairs, size_t entries) {
    return {{Y.ctl, PG_ENV_LAYOUT_CTL}, {Y.order, nfree * 4}, {Y.rowoff, (nfree + 1) * 4}, {Y.coloff, (nfree + 1) * 4}, {Y.colrows, (nblocks - nfree) * 4},
            {Y.colbase, (nblocks - nfree) * 4}, {Y.blk_src, nblocks * 4}, {Y.pair_off, (pairs + 1) * 4}, {Y.pair_ent, entries * 4}, {Y.pair_flag, pairs * 4},
            {Y.val, nblocks * 392}, {Y.dinv, nfree * 392}, {Y.y, nfree * 56}};
}

static void check_envelope(size_t nfree, size_t nblocks, size_t pairs, size_t entries) {
    PgEnvPieces M{};
    const size_t need = arena_measure([&](Arena& A) { pg_envelope_layout(A, nfree, nblocks, pairs, entries, M); });
    CHECK(M.ctl == nullptr && M.val == nullptr);
    std::vector<char> buf(need + 512);
    PgEnvPieces Y{};
    Arena A(buf.data(), need);
    pg_envelope_layout(A, nfree, nblocks, pairs, entries, Y);
    CHECK(!A.overflow && A.off == need);
    char name[96];
    std::snprintf(name, sizeof name, "envelope free %zu blocks %zu pairs %zu entries %zu", nfree, nblocks, pairs, entries);
    check_pieces(name, buf.data(), need, env_pieces(Y, nfree, nblocks, pairs, entries));
    Arena S(buf.data(), need - 1);
    PgEnvPieces Z{};
    pg_envelope_layout(S, nfree, nblocks, pairs, entries, Z);
    CHECK(S.overflow);
}

static void check_selftest(size_t nfree, size_t nblocks, size_t pairs, size_t entries, size_t input_pairs) {
    PgEnvSelftestPieces M{};
    const size_t need = arena_measure([&](Arena& A) { pg_envelope_selftest_layout(A, nfree, nblocks, pairs, entries, input_pairs, M); });
    std::vector<char> buf(need + 512);
    PgEnvSelftestPieces Y{};
    Arena A(buf.data(), need);
    pg_envelope_selftest_layout(A, nfree, nblocks, pairs, entries, input_pairs, Y);
    CHECK(!A.overflow && A.off == need);
    std::vector<Piece> pieces = env_pieces(Y.env, nfree, nblocks, pairs, entries);
    pieces.insert(pieces.end(), {{Y.ctl, 128}, {Y.diag, nfree * 392}, {Y.blocks, input_pairs * 392}, {Y.rhs, nfree * 56}, {Y.x, nfree * 56}});
    char name[96];
    std::snprintf(name, sizeof name, "self-test free %zu blocks %zu input pairs %zu", nfree, nblocks, input_pairs);
    check_pieces(name, buf.data(), need, pieces);
}

int main() {
    check_envelope(1, 1, 0, 0);                  // one free vertex, no pair
    check_envelope(2049, 10235, 6142, 6142);     // the chain of 2 049 with window 3 and a far loop pair
    check_envelope(297, 1757, 882, 885);         // class (e)
    check_selftest(1, 1, 0, 0, 0);
    check_selftest(2049, 10235, 6142, 6142, 6142);
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("posegraph envelope arena ok\n");
    return 0;
}
