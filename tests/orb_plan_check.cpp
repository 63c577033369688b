// Host-only check of the ORB planner (stella_vslam_amd/csrc/orb_plan.h): built and run by tests/test_orb_plan.py.
// Every check restates what a kernel of orb_kernels.hip relies on when it reads the tables, not the planner's own formula: a wrong band
// table would otherwise show only as a bit mismatch, or as an LDS overrun, on the device.
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

static const int DB_MAX_KP = 128;                 // keypoints of a band of k_describe_bands
static const size_t DB_LDS_HARD = 80 * 1024;      // staged rows of a band: two workgroups per CU
static const int PYR_MAX_GROUPS = 1024;           // k_pyramid_lds: one thread per group of 4 columns

// ---- k_describe_bands: the band table
static void check_describe_bands(const OrbConfig& C, const OrbTables& T) {
    if (C.dbands.empty()) return;
    std::vector<int> owner(C.total_grid, 0);
    int prev_bytes = 1 << 30;
    for (const DescBand& b : C.dbands) {
        CHECK(b.lv >= 0 && b.lv < C.num_levels);
        const OrbLevel& L = C.levels[b.lv];
        CHECK(L.has_cells);
        CHECK(b.cell0 >= L.grid_first && b.cell0 < b.cell1 && b.cell1 <= L.grid_first + L.grid_x * L.grid_y);
        CHECK(b.cell1 - b.cell0 <= DB_MAX_KP);
        for (int c = std::max(b.cell0, 0); c < std::min(b.cell1, C.total_grid); ++c) ++owner[c];
        CHECK(b.lp >= L.w && b.lp % 16 == 0 && b.lp % 64 == 32);
        // whole grid rows, and every level row a keypoint of those grid rows can lie on has both of its patches staged
        CHECK((b.cell0 - L.grid_first) % L.grid_x == 0 && (b.cell1 - L.grid_first) % L.grid_x == 0);
        const int g0 = (b.cell0 - L.grid_first) / L.grid_x, g1 = (b.cell1 - L.grid_first) / L.grid_x;
        const int rh = L.h - 2 * SV_PATCH_RADIUS;
        for (int yy = 0; yy < rh; ++yy) {
            const int g = T.gtab[L.gtab_y_off + yy], y = SV_PATCH_RADIUS + yy;
            if (g < g0 || g >= g1) continue;
            CHECK(y - 15 >= b.yu0 && y + 16 < b.yu0 + b.nru);
            CHECK(y - 18 >= b.yb0 && y + 18 < b.yb0 + b.nrb);
        }
        // a staging instruction (64 lanes x 16 bytes) carries whole rows: the last group may reach past the band's last row
        const int rows_per_instr = std::max(1, 1024 / b.lp), rows = std::max<int>(b.nru, b.nrb);
        CHECK((size_t)b.img_bytes >= (size_t)((rows + rows_per_instr - 1) / rows_per_instr * rows_per_instr) * b.lp);
        CHECK((size_t)b.img_bytes <= DB_LDS_HARD);
        CHECK((size_t)b.img_bytes + 2 * DB_MAX_KP * sizeof(OrbInt2) <= C.dband_lds_bytes);
        CHECK(b.img_bytes <= prev_bytes);  // heaviest first
        prev_bytes = b.img_bytes;
    }
    CHECK(C.dband_lds_bytes <= DB_LDS_HARD + 2 * 1024);
    for (int l = 0; l < C.num_levels; ++l) {
        const OrbLevel& L = C.levels[l];
        if (!L.has_cells) continue;
        for (int c = L.grid_first; c < L.grid_first + L.grid_x * L.grid_y; ++c) CHECK(owner[c] == 1);
    }
}

// ---- k_pyramid / k_pyramid_lds: the rows of every level a band computes
static void check_pyramid_bands(const OrbConfig& C, const OrbTables& T) {
    const int K = C.pyr_bands, NL = C.num_levels;
    CHECK(K >= 1 && T.band_rows.size() == (size_t)K * NL);
    if (T.band_rows.size() != (size_t)K * NL) return;
    size_t worst = 0;
    std::vector<int> owned_to(NL, 0);  // per level: the rows [0, owned_to) are owned by the bands so far
    for (int k = 0; k < K; ++k) {
        const OrbInt2* BR = &T.band_rows[(size_t)k * NL];
        for (int l = 1; l < NL; ++l) {
            const OrbLevel& L = C.levels[l];
            const int lo = (int)((long long)k * L.h / K), hi = (int)((long long)(k + 1) * L.h / K);
            CHECK(lo == owned_to[l] && lo <= hi);  // consecutive bands meet ...
            owned_to[l] = hi;
            if (k == K - 1) CHECK(hi == L.h);      // ... and the last one ends the level: [0, h) is tiled
            CHECK(BR[l].x >= 0 && BR[l].x <= BR[l].y && BR[l].y <= L.h);
            if (hi > lo) CHECK(BR[l].x <= lo && hi <= BR[l].y);
            for (int dy = BR[l].x; dy < BR[l].y; ++dy) {  // both source rows of every row the band computes are rows it holds
                const OrbShort2 o = T.yofs[L.ytab_off + dy];
                CHECK(o.x >= BR[l - 1].x && o.x < BR[l - 1].y && o.y >= BR[l - 1].x && o.y < BR[l - 1].y);
            }
        }
        if (NL > 1) CHECK(BR[0].x >= 0 && BR[0].y <= C.levels[0].h);
        // the LDS map of k_pyramid_lds: odd levels share one region, even levels (level 0 included) the other, pitch = w rounded up to 4,
        // each region rounded up to 16 bytes; then one 8-byte record per row of the levels >= 1
        size_t region[2] = {0, 0}, records = 0;
        for (int l = 0; l < NL; ++l) {
            const size_t rows = (size_t)(BR[l].y - BR[l].x);
            region[l & 1] = std::max(region[l & 1], rows * (size_t)((C.levels[l].w + 3) / 4 * 4));
            if (l >= 1) records += rows * 8;
        }
        worst = std::max(worst, (region[0] + 15) / 16 * 16 + (region[1] + 15) / 16 * 16 + records);
    }
    if (C.pyr_lds_bytes > 0) {
        CHECK(C.pyr_lds_bytes <= (size_t)SV_PYR_LDS_MAX);
        CHECK(C.pyr_lds_bytes >= worst);
        for (int l = 1; l < NL; ++l) CHECK((C.levels[l].w + 3) / 4 <= PYR_MAX_GROUPS);
    }
}

// ---- k_fast / k_select: cells, selection grid, lookup tables
static void check_cells_and_grid(const OrbConfig& C, const OrbTables& T) {
    int grid_sum = 0;
    for (int l = 0; l < C.num_levels; ++l) {
        const OrbLevel& L = C.levels[l];
        grid_sum += L.grid_x * L.grid_y;
        CHECK(L.cell_first >= 0 && L.cell_count >= 0 && (size_t)(L.cell_first + L.cell_count) <= C.cells.size());
        CHECK((L.has_cells != 0) == (L.w > 2 * SV_PATCH_RADIUS && L.h > 2 * SV_PATCH_RADIUS));
        if (!L.has_cells) {
            CHECK(L.cell_count == 0 && L.grid_x * L.grid_y == 0);
            continue;
        }
        CHECK(L.grid_first == grid_sum - L.grid_x * L.grid_y && L.grid_x >= 1 && L.grid_y >= 1);
        const int rw = L.w - 2 * SV_PATCH_RADIUS, rh = L.h - 2 * SV_PATCH_RADIUS;
        std::vector<unsigned char> covered((size_t)rw * rh, 0);
        for (int i = 0; i < L.cell_count; ++i) {
            const FastCell& c = C.cells[L.cell_first + i];
            CHECK(c.lv == l && c.w >= 1 && c.h >= 1 && c.w <= SV_ROI_MAX && c.h <= SV_ROI_MAX);
            CHECK(c.min_x >= SV_PATCH_RADIUS && c.min_y >= SV_PATCH_RADIUS && c.min_x + c.w <= L.w - SV_PATCH_RADIUS && c.min_y + c.h <= L.h - SV_PATCH_RADIUS);
            CHECK(c.cj >= 0 && c.cj < L.cells_x);
            if (i > 0) CHECK(c.order_base > C.cells[L.cell_first + i - 1].order_base);
            CHECK((c.order_base & ((1 << 14) - 1)) == 0);
            for (int y = std::max<int>(c.min_y, SV_PATCH_RADIUS); y < std::min(c.min_y + c.h, L.h - SV_PATCH_RADIUS); ++y)
                memset(&covered[(size_t)(y - SV_PATCH_RADIUS) * rw + std::max<int>(c.min_x, SV_PATCH_RADIUS) - SV_PATCH_RADIUS], 1,
                       (size_t)std::max(0, std::min(c.min_x + c.w, L.w - SV_PATCH_RADIUS) - std::max<int>(c.min_x, SV_PATCH_RADIUS)));
        }
        // The reference drops a cell that starts within SV_OVERLAP px of the far border (orb_extractor.cc:201, :211): the cell before it reaches
        // that far.  A region of at most SV_OVERLAP px in either direction loses its first cell too, and with it all of them.
        if (rw > SV_OVERLAP && rh > SV_OVERLAP) CHECK(std::find(covered.begin(), covered.end(), 0) == covered.end());
        else CHECK(L.cell_count == 0);
        CHECK(L.gtab_x_off >= 0 && (size_t)(L.gtab_x_off + rw) <= T.gtab.size() && L.gtab_y_off >= 0 && (size_t)(L.gtab_y_off + rh) <= T.gtab.size());
        for (int x = 0; x < rw; ++x) CHECK(T.gtab[L.gtab_x_off + x] < L.grid_x);
        for (int y = 0; y < rh; ++y) CHECK(T.gtab[L.gtab_y_off + y] < L.grid_y);
    }
    CHECK(C.total_grid == grid_sum);
}

// ---- k_pyramid / k_pyramid_lds: cv::resize coefficient tables and the packed column-group records
static void check_resize_tables(const OrbConfig& C, const OrbTables& T) {
    for (int l = 1; l < C.num_levels; ++l) {
        const OrbLevel &L = C.levels[l], &P = C.levels[l - 1];
        CHECK((size_t)(L.xtab_off + L.w) <= T.xofs.size() && T.xa.size() == T.xofs.size());
        CHECK((size_t)(L.ytab_off + L.h) <= T.yofs.size() && T.yb.size() == T.yofs.size() && T.yrow.size() == T.yofs.size());
        for (int x = 0; x < L.w; ++x) {
            const int sx = T.xofs[L.xtab_off + x];
            const OrbShort2 a = T.xa[L.xtab_off + x];
            CHECK(a.x + a.y == 2048);
            CHECK(sx >= 0 && sx <= P.w - 1 && (sx + 1 <= P.w - 1 || a.y == 0));  // the right tap of the last column has no weight
        }
        for (int y = 0; y < L.h; ++y) {
            const OrbShort2 o = T.yofs[L.ytab_off + y], b = T.yb[L.ytab_off + y];
            CHECK(b.x + b.y == 2048);
            CHECK(o.x >= 0 && o.x <= P.h - 1 && o.y >= 0 && o.y <= P.h - 1);
            const OrbShort4 r = T.yrow[L.ytab_off + y];
            CHECK(r.x == o.x && r.y == o.y && r.z == b.x && r.w == b.y);
        }
        if (C.pyr_lds_bytes == 0) continue;
        // records are in use: 8 words per 4 columns; byte selectors 0..6 inside the two 8-byte windows, and they name the table's columns
        CHECK((size_t)(L.xg_off + (L.w + 3) / 4) * 8 <= T.xg.size());
        for (int c = 0; c < L.w; c += 4) {
            const uint32_t* R = &T.xg[(size_t)(L.xg_off + c / 4) * 8];
            const int base[2] = {(int)(R[0] & 0xffff), (int)(R[0] >> 16)};
            for (int i = 0; i < 4; ++i) {
                const int k = (R[1] >> (8 * i)) & 255, col = std::min(c + i, L.w - 1);
                CHECK(k <= 6);
                CHECK(4 * base[i / 2] + k == T.xofs[L.xtab_off + col]);
                const OrbShort2 a = T.xa[L.xtab_off + col];
                CHECK(R[2 + i] == ((uint32_t)(unsigned short)a.x | ((uint32_t)(unsigned short)a.y << 16)) && a.x >= 0 && a.y >= 0);
            }
        }
    }
}

// ---- k_blur / k_blur_gather: work items
static void check_blur_items(const OrbConfig& C) {
    int tiles = 0, bands = 0;
    for (int l = 0; l < C.num_levels; ++l) {
        const OrbLevel& L = C.levels[l];
        CHECK(L.btile_first == tiles && L.bband_first == bands);
        CHECK(L.btiles_x * BLUR_TW >= L.w && L.btiles_y * 4 * C.blur_rows >= L.h);
        CHECK(L.bband_segs * BLUR_SEG >= L.w && (L.bband_segs - 1) * BLUR_SEG < L.w);
        const int edge_tiles = ((L.h + 7) / 8 + 63) / 64;  // 64 strips of 8 rows each
        tiles += L.btiles_x * L.btiles_y + edge_tiles;
        bands += L.bband_segs * ((L.h + BLUR_ROWS - 1) / BLUR_ROWS);
    }
    CHECK(C.total_btiles == tiles && C.total_bbands == bands);
    CHECK(C.blur_rows == (C.max_batch <= BLUR_SMALL_BATCH ? BLUR_ROWS_SMALL : BLUR_ROWS));
}

enum Expect { EMPTY, NONEMPTY };

static bool build(int w, int h, int levels, int max_batch, const OrbEnv& env, OrbPlan& P) {
    std::snprintf(where, sizeof where, "%dx%d levels %d max_batch %d", w, h, levels, max_batch);
    const char* err = orb_plan_build(w, h, max_batch, 1.2f, levels, 20, 7, 800, env, P);
    CHECK(err == nullptr);
    return err == nullptr;
}

static void check_shape(int w, int h, int levels, int max_batch, const OrbEnv& env, Expect dbands, Expect pyr_lds) {
    OrbPlan P;
    if (!build(w, h, levels, max_batch, env, P)) return;
    const OrbConfig& C = P.config;
    CHECK(!C.configured && C.width == w && C.height == h && C.num_levels == levels && C.max_batch == max_batch);
    CHECK(C.dbands.empty() == (dbands == EMPTY));
    CHECK((C.pyr_lds_bytes == 0) == (pyr_lds == EMPTY));
    check_describe_bands(C, P.tables);
    check_pyramid_bands(C, P.tables);
    check_cells_and_grid(C, P.tables);
    check_resize_tables(C, P.tables);
    check_blur_items(C);
    std::printf("ok %s: %zu cells, grid %d, %zu describe bands (%zu B LDS), %d pyramid bands (%zu B LDS)\n", where, C.cells.size(), C.total_grid,
                C.dbands.size(), C.dband_lds_bytes, C.pyr_bands, C.pyr_lds_bytes);
}

static void check_launch_plan() {
    const OrbEnv none;
    OrbPlan P;
    if (!build(640, 480, 8, 1024, none, P)) return;
    const OrbConfig& C = P.config;
    std::snprintf(where, sizeof where, "launch plan 640x480");
    // the batch at which each threshold flips, from the plan's own counts
    const int cells = (int)C.cells.size(), b_cpw = (ORB_FAST_CPW4_MIN_CELLS + cells - 1) / cells;
    const int b_bands = (ORB_DESCRIBE_BANDS_MIN_KP + C.total_grid - 1) / C.total_grid;
    CHECK(b_cpw > 1 && b_cpw <= 1024 && b_bands > 1 && b_bands <= 1024);
    CHECK(orb_launch_plan(C, b_cpw - 1, true, none).fast_cpw == 1 && orb_launch_plan(C, b_cpw, true, none).fast_cpw == 4);
    CHECK(!orb_launch_plan(C, b_bands - 1, true, none).describe_bands && orb_launch_plan(C, b_bands, true, none).describe_bands);
    OrbLaunch L = orb_launch_plan(C, 1, true, none);
    CHECK(L.pyramid_lds && L.blur_bands && !L.need_gather && L.fast_cpw == 1 && !L.describe_bands);
    CHECK(orb_launch_plan(C, 1, false, none).need_gather);  // caller image not 4-byte aligned
    // overrides
    OrbEnv e;
    e.fast_cpw = 2;
    CHECK(orb_launch_plan(C, 1, true, e).fast_cpw == 2 && orb_launch_plan(C, 1024, true, e).fast_cpw == 2);
    e = OrbEnv();
    e.describe_bands = true;
    CHECK(orb_launch_plan(C, 1, true, e).describe_bands);
    // the switches of configure do nothing at launch: same plan, whatever they say
    e = OrbEnv();
    e.describe_legacy = true;
    e.desc_band_kb = 1;
    e.pyr_bands = 3;
    e.fork_blur = true;
    const OrbLaunch a = orb_launch_plan(C, b_bands, true, e), b = orb_launch_plan(C, b_bands, true, none);
    CHECK(a.pyramid_lds == b.pyramid_lds && a.blur_bands == b.blur_bands && a.need_gather == b.need_gather && a.fast_cpw == b.fast_cpw &&
          a.describe_bands == b.describe_bands);
    // a context without a band table keeps k_describe, whatever the batch or the switch
    OrbEnv legacy;
    legacy.describe_legacy = true;
    OrbPlan Q;
    if (build(640, 480, 8, 1024, legacy, Q)) {
        e = OrbEnv();
        e.describe_bands = true;
        CHECK(Q.config.dbands.empty() && !orb_launch_plan(Q.config, 1024, true, e).describe_bands);
    }
    // a context of a few frames streams the blur; a level narrower than 16 px needs the gather kernel; a wide image takes k_pyramid
    if (build(640, 480, 8, BLUR_SMALL_BATCH, none, Q)) CHECK(!orb_launch_plan(Q.config, 1, true, none).blur_bands);
    if (build(640, 480, 8, BLUR_SMALL_BATCH + 1, none, Q)) CHECK(orb_launch_plan(Q.config, 1, true, none).blur_bands);
    if (build(40, 40, 8, 1, none, Q)) {
        CHECK(Q.config.levels[7].w < 16);
        CHECK(orb_launch_plan(Q.config, 1, true, none).need_gather);
    }
    if (build(4920, 48, 2, 1, none, Q)) CHECK(!orb_launch_plan(Q.config, 1, true, none).pyramid_lds);
}

int main() {
    const OrbEnv none;
    // What the band table of k_describe_bands is at each shape was read off the planner before it was moved here (the same function, then
    // inside svgpu_orb_configure): 45 / 56 / 58 / 10 / 8 bands at the first five shapes and 1 at 40 x 40; none at 1920 x 1080 and none at
    // 4920 x 48 (the rows of one grid row of level 0 exceed the 80 KB a band may stage).
    const struct { int w, h; Expect dbands; } shapes[] = {{640, 480, NONEMPTY}, {752, 480, NONEMPTY}, {1241, 376, NONEMPTY},
                                                          {320, 240, NONEMPTY}, {203, 157, NONEMPTY}, {1920, 1080, EMPTY}};
    for (const auto& s : shapes)
        for (int max_batch : {1, 4, 5, 1024}) check_shape(s.w, s.h, 8, max_batch, none, s.dbands, NONEMPTY);
    check_shape(4920, 48, 2, 1, none, EMPTY, EMPTY);  // level 1 is 4100 px wide: more than 1024 column groups, the global pyramid variant
    check_shape(40, 40, 8, 1, none, NONEMPTY, NONEMPTY);  // levels 1.. have no cells
    {
        OrbPlan P;  // 8 / 1.2^10 rounds to 1 px
        const char* err = orb_plan_build(8, 8, 1, 1.2f, 16, 20, 7, 800, none, P);
        std::snprintf(where, sizeof where, "8x8 levels 16");
        CHECK(err != nullptr && std::strstr(err, "smaller than 2 px") != nullptr);
    }
    // the switches of configure: the tables they shape obey the same contracts
    OrbEnv e;
    e.desc_band_kb = 80;
    e.pyr_bands = 20;
    check_shape(640, 480, 8, 1024, e, NONEMPTY, NONEMPTY);
    e = OrbEnv();
    e.desc_band_kb = 1;  // below one grid row: single-row bands
    e.pyr_bands = 1;     // one band does not fit LDS: the count grows until it does
    check_shape(752, 480, 8, 5, e, NONEMPTY, NONEMPTY);
    e = OrbEnv();
    e.describe_legacy = true;
    check_shape(640, 480, 8, 1024, e, EMPTY, NONEMPTY);
    check_launch_plan();
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("orb plan ok\n");
    return 0;
}
