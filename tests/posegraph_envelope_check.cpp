// Host-only check of the envelope planner of the pose graph's direct solver (stella_vslam_amd/csrc/posegraph_envelope_plan.h): built and
// run by tests/test_posegraph_envelope.py (and by the GPU self-test, for the block counts) on a graph file
//   nfree E natural_blocks interleaved_blocks        (the two envelope sizes computed independently by the caller; -1: not given)
//   E lines "a b": the free slots of the edge's ends, -1 for a fixed end
// It checks the plan's invariants, then runs the plain fp64 elimination on a system with deterministic, strictly diagonally dominant
// blocks (every diagonal entry = its row's absolute sum + 1) and on the same system with one negative diagonal block, and prints
//   PLAN <envelope blocks> <max column rows> <ordering> / RESIDUAL <|Ax - b| / |b|> / "envelope plan ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "posegraph_envelope_plan.h"

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// entry (r, c) of the block of pair k (rows lo, columns hi); entry of the off-diagonal part of slot s's diagonal block (symmetric)
static double pair_entry(int k, int r, int c) { return (double)(((k * 49 + r * 7 + c) * 37 + 11) % 101) / 101.0 - 0.5; }
static double diag_entry(int s, int r, int c) { return (double)(((s * 49 + std::min(r, c) * 7 + std::max(r, c)) * 53 + 29) % 103) / 103.0 - 0.5; }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int nfree = 0, E = 0;
    long long natural = -1, interleaved = -1;
    if (std::fscanf(f, "%d %d %lld %lld", &nfree, &E, &natural, &interleaved) != 4) return 2;
    std::vector<int32_t> sa((size_t)E), sb((size_t)E);
    for (int e = 0; e < E; ++e)
        if (std::fscanf(f, "%d %d", &sa[(size_t)e], &sb[(size_t)e]) != 2) return 2;
    std::fclose(f);
    PgEnvPlan P;
    pg_env_plan(nfree, E, sa.data(), sb.data(), P);
    CHECK(P.fits);
    const size_t n = (size_t)nfree;
    // the order is a permutation, pos its inverse
    CHECK(P.order.size() == n && P.pos.size() == n);
    std::vector<int> seen(n, 0);
    for (size_t p = 0; p < n; ++p) {
        CHECK(P.order[p] >= 0 && P.order[p] < nfree);
        if (P.order[p] >= 0 && P.order[p] < nfree) {
            ++seen[(size_t)P.order[p]];
            CHECK(P.pos[(size_t)P.order[p]] == (int)p);
        }
    }
    for (size_t s = 0; s < n; ++s) CHECK(seen[s] == 1);
    // first[row] <= row; the block count is the sum of the row lengths; the column lists mirror the rows
    CHECK(P.first.size() == n && P.rowoff.size() == n + 1 && P.coloff.size() == n + 1);
    long long sum = 0;
    int tallest = 0;
    std::vector<int> colcount(n, 0);
    for (int i = 0; i < nfree; ++i) {
        CHECK(P.first[(size_t)i] >= 0 && P.first[(size_t)i] <= i);
        CHECK(P.rowoff[(size_t)i] == sum);
        sum += i - P.first[(size_t)i] + 1;
        for (int j = P.first[(size_t)i]; j < i; ++j) ++colcount[(size_t)j];
    }
    CHECK(P.nblocks == sum && P.rowoff[n] == sum);
    CHECK((long long)P.colrows.size() == sum - nfree && P.colbase.size() == P.colrows.size() && (long long)P.blk_src.size() == sum);
    for (int j = 0; j < nfree; ++j) {
        const int c0 = P.coloff[(size_t)j], m = P.coloff[(size_t)j + 1] - c0;
        CHECK(m == colcount[(size_t)j]);
        tallest = std::max(tallest, m);
        for (int r = 0; r < m; ++r) {
            const int i = P.colrows[(size_t)(c0 + r)];
            CHECK(i > j && i < nfree && P.first[(size_t)i] <= j);
            CHECK(r == 0 || i > P.colrows[(size_t)(c0 + r - 1)]);
            CHECK(P.colbase[(size_t)(c0 + r)] == P.rowoff[(size_t)i] - P.first[(size_t)i]);
            CHECK(P.colbase[(size_t)(c0 + r)] + j >= P.rowoff[(size_t)i] && P.colbase[(size_t)(c0 + r)] + j < P.rowoff[(size_t)i + 1] - 1);
        }
    }
    CHECK(tallest == P.max_column_rows);
    // no larger than the natural and the interleaved envelope as the caller computed them
    if (natural >= 0) CHECK(P.nblocks <= natural);
    if (interleaved >= 0) CHECK(P.nblocks <= interleaved);
    if (P.ordering == PG_ENV_ORDER_NATURAL && natural >= 0) CHECK(P.nblocks == natural);
    if (P.ordering == PG_ENV_ORDER_INTERLEAVED && interleaved >= 0) CHECK(P.nblocks == interleaved);
    // pairs: distinct, ascending; every free-free edge is in exactly one list, lists ascend in edge index, flags say "the edge runs hi -> lo"
    CHECK((int)P.pair_a.size() == P.num_pairs && (int)P.pair_off.size() == P.num_pairs + 1 && P.pair_off[0] == 0);
    std::vector<int> listed((size_t)E, 0);
    for (int k = 0; k < P.num_pairs; ++k) {
        const int lo = P.pair_a[(size_t)k], hi = P.pair_b[(size_t)k];
        CHECK(lo >= 0 && lo < hi && hi < nfree);
        if (k) CHECK(P.pair_a[(size_t)k - 1] < lo || (P.pair_a[(size_t)k - 1] == lo && P.pair_b[(size_t)k - 1] < hi));
        CHECK(P.pair_off[(size_t)k + 1] > P.pair_off[(size_t)k]);
        for (int q = P.pair_off[(size_t)k]; q < P.pair_off[(size_t)k + 1]; ++q) {
            const int e = P.pair_ent[(size_t)q] >> 1, t = P.pair_ent[(size_t)q] & 1;
            CHECK(e >= 0 && e < E);
            if (e < 0 || e >= E) continue;
            ++listed[(size_t)e];
            CHECK(q == P.pair_off[(size_t)k] || e > (P.pair_ent[(size_t)q - 1] >> 1));
            if (t) CHECK(sa[(size_t)e] == hi && sb[(size_t)e] == lo);
            else CHECK(sa[(size_t)e] == lo && sb[(size_t)e] == hi);
        }
        // the pair's block lies inside the envelope, below the diagonal, and the flag follows the positions
        const int plo = P.pos[(size_t)lo], phi = P.pos[(size_t)hi], row = std::max(plo, phi), col = std::min(plo, phi);
        CHECK(col >= P.first[(size_t)row] && col < row);
        CHECK(P.pair_blk[(size_t)k] == P.rowoff[(size_t)row] + col - P.first[(size_t)row]);
        CHECK(P.pair_flag[(size_t)k] == (plo > phi ? 0 : 1));
        CHECK(P.blk_src[(size_t)P.pair_blk[(size_t)k]] == nfree + k);
    }
    if (P.num_pairs) CHECK(P.pair_off[(size_t)P.num_pairs] == (int)P.pair_ent.size());
    for (int e = 0; e < E; ++e) CHECK(listed[(size_t)e] == ((sa[(size_t)e] >= 0 && sb[(size_t)e] >= 0 && sa[(size_t)e] != sb[(size_t)e]) ? 1 : 0));
    for (int i = 0; i < nfree; ++i) CHECK(P.blk_src[(size_t)P.rowoff[(size_t)i + 1] - 1] == i);
    std::printf("PLAN %lld %d %d\n", (long long)P.nblocks, P.max_column_rows, P.ordering);

    // ---- host elimination on a diagonally dominant system, residual against the system in SLOT order
    const size_t N = 7 * n;
    std::vector<double> rowsum(N, 0.0), b(N);
    for (int k = 0; k < P.num_pairs; ++k)
        for (int r = 0; r < 7; ++r)
            for (int c = 0; c < 7; ++c) {
                rowsum[(size_t)P.pair_a[(size_t)k] * 7 + (size_t)r] += std::fabs(pair_entry(k, r, c));
                rowsum[(size_t)P.pair_b[(size_t)k] * 7 + (size_t)c] += std::fabs(pair_entry(k, r, c));
            }
    const auto diag = [&](int s, int r, int c) {
        if (r != c) return diag_entry(s, r, c);
        double v = 1.0 + rowsum[(size_t)s * 7 + (size_t)r];
        for (int k = 0; k < 7; ++k)
            if (k != r) v += std::fabs(diag_entry(s, r, k));
        return v;
    };
    for (size_t t = 0; t < N; ++t) b[t] = (double)((t * 31 + 7) % 17) - 8.0;
    for (int variant = 0; variant < 2; ++variant) {  // 1: the diagonal block of the slot in the middle negated
        const int bad = variant ? nfree / 2 : -1;
        std::vector<double> val((size_t)P.nblocks * 49, 0.0), y(N);
        for (int p = 0; p < nfree; ++p) {
            const int s = P.order[(size_t)p];
            double* D = val.data() + ((size_t)P.rowoff[(size_t)p + 1] - 1) * 49;
            for (int r = 0; r < 7; ++r)
                for (int c = 0; c < 7; ++c) D[r * 7 + c] = (s == bad ? -1.0 : 1.0) * diag(s, r, c);
            for (int c = 0; c < 7; ++c) y[(size_t)p * 7 + (size_t)c] = b[(size_t)s * 7 + (size_t)c];
        }
        for (int k = 0; k < P.num_pairs; ++k) {
            double* B = val.data() + (size_t)P.pair_blk[(size_t)k] * 49;
            for (int r = 0; r < 7; ++r)
                for (int c = 0; c < 7; ++c) B[r * 7 + c] = P.pair_flag[(size_t)k] ? pair_entry(k, c, r) : pair_entry(k, r, c);
        }
        const bool ok = pg_env_host_factor(P, val.data());
        if (variant) {
            CHECK(!ok);
            continue;
        }
        CHECK(ok);
        if (!ok) continue;
        pg_env_host_solve(P, val.data(), y.data());
        std::vector<double> x(N), res(N);
        for (int p = 0; p < nfree; ++p)
            for (int c = 0; c < 7; ++c) x[(size_t)P.order[(size_t)p] * 7 + (size_t)c] = y[(size_t)p * 7 + (size_t)c];
        for (size_t t = 0; t < N; ++t) res[t] = -b[t];
        for (int s = 0; s < nfree; ++s)
            for (int r = 0; r < 7; ++r)
                for (int c = 0; c < 7; ++c) res[(size_t)s * 7 + (size_t)r] += diag(s, r, c) * x[(size_t)s * 7 + (size_t)c];
        for (int k = 0; k < P.num_pairs; ++k) {
            const size_t lo = (size_t)P.pair_a[(size_t)k] * 7, hi = (size_t)P.pair_b[(size_t)k] * 7;
            for (int r = 0; r < 7; ++r)
                for (int c = 0; c < 7; ++c) {
                    res[lo + (size_t)r] += pair_entry(k, r, c) * x[hi + (size_t)c];
                    res[hi + (size_t)c] += pair_entry(k, r, c) * x[lo + (size_t)r];
                }
        }
        double rr = 0.0, bb = 0.0;
        for (size_t t = 0; t < N; ++t) rr += res[t] * res[t], bb += b[t] * b[t];
        const double rel = std::sqrt(rr / bb);
        std::printf("RESIDUAL %.3e\n", rel);
        CHECK(rel <= 1e-12);
    }
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("envelope plan ok\n");
    return 0;
}
