// What the host planner (stella_vslam_amd/csrc/orb_plan.h) decides for one configuration, printed for tests/test_gpu_orb_prologues.py:
//   orb_prologue_plan W H BATCH SCALE LEVELS INI MIN AREA ALIGNED
// line "plan":  pyramid_lds describe_bands(with SVGPU_DESCRIBE_BANDS set) pyr_bands pyr_lds_bytes pyr_cpr0 desc_max_cpr rc1 rc_more
//   pyr_cpr0 = 16-byte pieces of a staged level-0 row of k_pyramid_lds, desc_max_cpr = the most pieces per row of a k_describe_bands band
//   (more than 64: db_stage_rows_wide), rc1 / rc_more = (band, level >= 1) pairs whose threads walk one row / more than one row
// lines "band": cell0 cell1 level y0 y1 -- the level rows [y0, y1] whose keypoints a k_describe_bands workgroup describes
#include <cstdio>
#include <cstdlib>

#include "orb_plan.h"

int main(int argc, char** argv) {
    if (argc != 10) return 2;
    const int w = atoi(argv[1]), h = atoi(argv[2]), batch = atoi(argv[3]), nl = atoi(argv[5]), ini = atoi(argv[6]), mn = atoi(argv[7]);
    const float sf = (float)atof(argv[4]);
    const unsigned area = (unsigned)atoi(argv[8]);
    const bool aligned = atoi(argv[9]) != 0;
    OrbEnv env;
    env.describe_bands = true;
    OrbPlan plan;
    if (const char* err = orb_plan_build(w, h, batch, sf, nl, ini, mn, area, env, plan)) {
        printf("FAIL %s\n", err);
        return 1;
    }
    const OrbConfig& C = plan.config;
    const OrbLaunch P = orb_launch_plan(C, batch, aligned, env);
    int max_cpr = 0;
    for (const DescBand& bd : C.dbands) max_cpr = std::max(max_cpr, bd.lp >> 4);
    int rc1 = 0, rc_more = 0;
    for (int k = 0; k < C.pyr_bands; ++k)
        for (int l = 1; l < nl; ++l) {  // the thread -> (chunk, group) map of k_pyramid_lds
            const OrbInt2 r = plan.tables.band_rows[(size_t)k * nl + l];
            const int groups = (C.levels[l].w + 3) >> 2, nrows = r.y - r.x;
            if (nrows <= 0) continue;
            const int chunks = std::max(std::min(1024 / groups, nrows), 1), rc = (nrows + chunks - 1) / chunks;
            if (rc == 1) ++rc1;
            else ++rc_more;
        }
    printf("plan %d %d %d %zu %d %d %d %d\n", (int)P.pyramid_lds, (int)P.describe_bands, C.pyr_bands, C.pyr_lds_bytes, ((C.levels[0].w + 3) & ~3) >> 4,
           max_cpr, rc1, rc_more);
    for (const DescBand& bd : C.dbands) printf("band %d %d %d %d %d\n", bd.cell0, bd.cell1, (int)bd.lv, bd.yu0 + 15, bd.yu0 + bd.nru - 17);
    return 0;
}
