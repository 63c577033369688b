// Host-only check of the coefficient-sum property of the resize tables (stella_vslam_amd/csrc/orb_plan.h): built and run by
// tests/test_orb_coef_sums.py.  k_pyramid_lds packs four results of a row step into a dword without masking them to a byte; that is only
// sound while every column pair (a0, a1) and every row pair (b0, b1) sums to at most 2049.  The planner verifies it and refuses a table
// that breaks it; this program checks the verifier on the shapes of tests/orb_plan_check.cpp and on tables broken on purpose, and restates
// the bound the kernel's pack relies on by exhausting the worst case.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orb_plan.h"

static int failures = 0;
static char where[128] = "";
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            if (failures < 40) std::printf("FAIL %s:%d [%s]: %s\n", __FILE__, __LINE__, where, #cond); \
            ++failures;                                                              \
        }                                                                            \
    } while (0)

// the property, restated from the tables (not through orb_plan_coef_sums_ok); also the largest sums seen
static void check_tables(const OrbPlan& P, int& max_a, int& max_b) {
    const OrbTables& T = P.tables;
    for (const OrbShort2& a : T.xa) {
        CHECK(a.x >= 0 && a.y >= 0 && a.x + a.y <= 2049);
        max_a = std::max(max_a, a.x + a.y);
    }
    for (const OrbShort2& b : T.yb) {
        CHECK(b.x >= 0 && b.y >= 0 && b.x + b.y <= 2049);
        max_b = std::max(max_b, b.x + b.y);
    }
    CHECK(T.xg.size() % 8 == 0);
    for (size_t r = 0; r + 8 <= T.xg.size(); r += 8)
        for (int i = 2; i < 6; ++i) CHECK((T.xg[r + i] & 0xffffu) + (T.xg[r + i] >> 16) <= 2049u);
    for (const OrbShort4& y : T.yrow) CHECK(y.z >= 0 && y.w >= 0 && y.z + y.w <= 2049);
    CHECK(T.yrow.size() == T.yb.size());
    CHECK(orb_plan_coef_sums_ok(T));
}

static bool build(int w, int h, int levels, int max_batch, float sf, OrbPlan& P) {
    std::snprintf(where, sizeof where, "%dx%d levels %d max_batch %d scale %.2f", w, h, levels, max_batch, (double)sf);
    const char* err = orb_plan_build(w, h, max_batch, sf, levels, 20, 7, 800, OrbEnv(), P);
    CHECK(err == nullptr);
    return err == nullptr;
}

// one entry of one table pushed to a pair that sums to `sum`: is the table still accepted?
static bool accepted_with(const OrbPlan& P, int table, int sum) {
    OrbTables T = P.tables;
    const short hi = (short)(sum - 1000), lo = 1000;
    switch (table) {
    case 0: T.xa[T.xa.size() / 2] = OrbShort2{lo, hi}; break;
    case 1: T.yb[T.yb.size() / 3] = OrbShort2{hi, lo}; break;
    case 2: T.xg[8 * (T.xg.size() / 16) + 5] = (uint32_t)(unsigned short)lo | ((uint32_t)(unsigned short)hi << 16); break;
    case 3: T.yrow.back().w = hi, T.yrow.back().z = lo; break;
    }
    return orb_plan_coef_sums_ok(T);
}

int main() {
    int max_a = 0, max_b = 0;
    const struct { int w, h; } shapes[] = {{640, 480}, {752, 480}, {1241, 376}, {320, 240}, {203, 157}, {1920, 1080}};
    OrbPlan P;
    for (const auto& s : shapes)
        for (int max_batch : {1, 4, 5, 1024})
            if (build(s.w, s.h, 8, max_batch, 1.2f, P)) check_tables(P, max_a, max_b);
    if (build(4920, 48, 2, 1, 1.2f, P)) check_tables(P, max_a, max_b);
    if (build(40, 40, 8, 1, 1.2f, P)) check_tables(P, max_a, max_b);
    for (float sf : {1.1f, 1.3f, 1.5f, 2.0f})  // the scale factors of the random-geometry GPU test
        if (build(331, 250, 4, 2, sf, P)) check_tables(P, max_a, max_b);
    std::snprintf(where, sizeof where, "largest sums");
    CHECK(max_a >= 2048 && max_a <= 2049 && max_b >= 2048 && max_b <= 2049);

    // a table broken on purpose: a pair that sums to 2050 anywhere is refused, one that sums to 2049 is not
    if (build(640, 480, 8, 4, 1.2f, P)) {
        for (int table = 0; table < 4; ++table) {
            std::snprintf(where, sizeof where, "broken table %d", table);
            CHECK(accepted_with(P, table, 2049));
            CHECK(!accepted_with(P, table, 2050));
            CHECK(!accepted_with(P, table, 4096));
        }
    }

    // the bound the pack of k_pyramid_lds relies on: with H <= 255 * (a0 + a1) and the sums at their limit, every result fits a byte.
    // Exhaustive over the row pair (b0, 2049 - b0) at the largest H of both rows (the expression is monotone in H0, H1, b0 and b1).
    std::snprintf(where, sizeof where, "pack bound");
    const uint32_t Hmax = 255u * 2049u;
    uint32_t vmax = 0;
    for (uint32_t b0 = 0; b0 <= 2049; ++b0) {
        const uint32_t b1 = 2049 - b0;
        const uint32_t v = (((b0 * (Hmax >> 4)) >> 16) + ((b1 * (Hmax >> 4)) >> 16) + 2) >> 2;
        vmax = std::max(vmax, v);
    }
    CHECK(vmax == 255);
    CHECK((2048u << 12) < (1u << 24) && (Hmax & ~15u) < (1u << 24));  // both factors of v_mul_hi_u32_u24 stay below 2^24

    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("orb coefficient sums ok (largest column pair %d, row pair %d)\n", max_a, max_b);
    return 0;
}
