// Host-side plan of the ORB front end: the geometry / coefficient tables (bit-identical to the reference's host arithmetic), the work-item
// tables of the kernels, and the per-call launch decisions.  Plain C++17 with no HIP include: libsvgpu (svgpu_orb.hip uploads what
// orb_plan_build returns, orb_kernels.hip reads the constants and the device-resident structs) and the g++-built tests/orb_plan_check.cpp
// share it.
//   orb_params scale tables        feature/orb_params.cc:41-71
//   level sizes                    feature/orb_extractor.cc:157-159
//   cv::resize coefficient tables  OpenCV 4.x imgproc/src/resize.cpp (8-bit fixed point, 11-bit coefficients)
//   FAST cell lattice              feature/orb_extractor.cc:179-217
//   selection grid                 feature/orb_extractor.cc:292-305
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#if defined(__clang__)
#pragma clang fp contract(off)
#pragma STDC FP_CONTRACT OFF
#endif

#define SV_MAX_LEVELS 16
#define SV_PATCH_RADIUS 19  // orb_extractor.h:107 orb_patch_radius_
#define SV_CELL 64          // orb_extractor.cc:173 cell_size
#define SV_OVERLAP 6        // orb_extractor.cc:172 overlap
#define SV_ROI_MAX 70       // SV_CELL + SV_OVERLAP
// k_blur tiling (shared by the kernels and the host-side work-item counts).
// Batches: a workgroup of BLUR_BAND_THREADS threads blurs BLUR_ROWS output rows of one column segment of a level from LDS (k_blur<BLUR_ROWS>).
// The three values were picked together by measurement in the pipeline: LDS per workgroup, and with it the number of
// workgroups that stage and compute side by side on a CU, weighs more than halo rows or the six warm-up rows of a chunk.
#ifndef BLUR_ROWS
#define BLUR_ROWS 48                // output rows of a band: the band stages BLUR_ROWS + 6 source rows, (R + 6) / R of the level's bytes
#endif
#ifndef BLUR_SEG
#define BLUR_SEG 320                // widest column segment of a band, a multiple of 16: wider levels are split, each segment re-reading
#endif                              // 16 bytes per row on either side.  LDS per workgroup: (BLUR_ROWS + 8) x (BLUR_SEG + 32) bytes = 19 712
#ifndef BLUR_BAND_THREADS
#define BLUR_BAND_THREADS 256       // thread = (chunk of rows, group of 4 columns): 320 px = 80 groups x 3 chunks of 16 rows
#endif
// Contexts configured for at most BLUR_SMALL_BATCH frames: latency, not traffic, is what counts -- the streaming kernel, a thread walks
// BLUR_ROWS_SMALL rows of 4 columns straight from global memory.  k_blur_gather uses the same tiles with OrbConfig::blur_rows rows.
#define BLUR_ROWS_SMALL 16
#define BLUR_SMALL_BATCH 4
#define BLUR_TW 256                 // tile width  = 64 threads x 4 px; tile height = 4 strips of OrbConfig::blur_rows rows
#define SV_PYR_LDS_MAX (156 * 1024)  // dynamic LDS budget of k_pyramid_lds (160 KB per CU minus its static tables)
#define SV_PYR_LDS_HALF (78 * 1024)  // ... of which two fit a CU

// ---- per-level geometry, read by every ORB kernel (lives in device memory, one array per context)
struct OrbLevel {
    int w, h;               // level size in pixels
    int pitch;              // row pitch (bytes) of the stored pyramid / blurred level
    int has_cells;          // 0 if the level is too small for a 19-px border
    long long pyr_off;      // byte offset of this level inside one frame's pyramid block (levels >= 1)
    long long blur_off;     // byte offset inside one frame's blurred block (all levels)
    int xtab_off, ytab_off; // resize coefficient tables (level produced from level-1)
    int xg_off;             // first 32-byte column-group record of this level in the packed table of k_pyramid_lds
    int cell_first, cell_count;     // FAST cells of this level in the cell table
    int cells_x;                    // num_cols of the FAST cell lattice (orb_extractor.cc:186)
    int grid_x, grid_y, grid_first; // selection grid (distribute_keypoints) and its offset in the key array
    int gtab_x_off, gtab_y_off;     // region coordinate -> grid index lookup tables
    int btile_first, btiles_x, btiles_y;  // blur tiles
    int bband_first, bband_segs;          // blur bands of k_blur<BLUR_ROWS>: first work item, column segments per band (BLUR_SEG px each)
    float scale;            // scale_factors_[level]
    float kp_size;          // (float)(unsigned)(31 * scale)
};

struct FastCell {
    short min_x, min_y;  // ROI origin in level coordinates
    short w, h;          // ROI size (<= 70)
    short lv, cj;        // pyramid level; cell column (j in orb_extractor.cc:199-217)
    int order_base;      // (ci * num_cols + cj) << 14 : emission order prefix
};

// k_describe_bands: a band = consecutive rows of one level's selection grid whose pixels one workgroup stages in LDS (orb_kernels.hip)
struct DescBand {
    int cell0, cell1;  // selection-grid cells [cell0, cell1) (indices into the per-frame key / position arrays)
    int img_bytes;     // LDS bytes of the staged rows (the larger of the two phases), a multiple of 16
    short lv, lp;      // level; LDS row pitch (multiple of 16, = 32 mod 64)
    short yu0, nru;    // un-blurred rows [yu0, yu0 + nru)  (every keypoint's y - 15 .. y + 16)
    short yb0, nrb;    // blurred rows    [yb0, yb0 + nrb)  (every keypoint's y - 18 .. y + 18)
};

struct OrbConfig {
    int width = 0, height = 0, max_batch = 0, num_levels = 0;
    float scale_factor = 0;
    int ini_thr = 0, min_thr = 0;
    unsigned min_area_sqrt = 0;
    float scale_factors[SV_MAX_LEVELS];
    OrbLevel levels[SV_MAX_LEVELS];
    std::vector<FastCell> cells;
    int total_grid = 0;    // sum of grid cells over levels = max keypoints per frame
    int total_btiles = 0, total_bbands = 0;
    int blur_rows = BLUR_ROWS;  // BLUR_ROWS: the band kernel; BLUR_ROWS_SMALL: the streaming kernel (a context of a few frames)
    size_t pyr_frame_bytes = 0, blur_frame_bytes = 0;
    std::vector<DescBand> dbands;  // empty: the configuration does not fit the band kernel, k_describe takes it
    size_t dband_lds_bytes = 0;    // dynamic LDS of k_describe_bands
    int pyr_bands = 0;             // workgroups per frame of the pyramid kernels
    size_t pyr_lds_bytes = 0;      // dynamic LDS of k_pyramid_lds for this configuration; 0 = use the global-memory variant (k_pyramid)
    bool configured = false;
};

// element types of the uploaded tables: layout-equal to HIP's short2 / int2 / short4 (svgpu_orb.hip asserts it at every upload)
struct alignas(4) OrbShort2 {
    short x, y;
};
struct alignas(8) OrbInt2 {
    int x, y;
};
struct alignas(8) OrbShort4 {
    short x, y, z, w;
};

// the host images of the device tables a configuration uploads
struct OrbTables {
    std::vector<short> xofs;            // per level >= 1: source column
    std::vector<OrbShort2> xa;          // (a0, a1) 11-bit coefficients
    std::vector<OrbShort2> yofs;        // (row0, row1) clamped
    std::vector<OrbShort2> yb;          // (b0, b1)
    std::vector<uint32_t> xg;           // k_pyramid_lds: 8 words per group of 4 output columns (orb_plan_pyramid_records)
    std::vector<OrbShort4> yrow;        // k_pyramid_lds: (row0, row1, b0, b1) per output row
    std::vector<unsigned short> gtab;   // region coordinate -> selection-grid index, x then y of every level with cells
    std::vector<OrbInt2> band_rows;     // [pyr_bands][levels]: rows of each level a pyramid band computes
};

// The ORB environment switches as values (svgpu_orb.hip orb_env() reads them; nothing in this header calls getenv).
struct OrbEnv {
    bool describe_legacy = false;  // SVGPU_DESCRIBE_LEGACY is set
    int desc_band_kb = 0;          // SVGPU_DESC_BAND_KB (>= 1); 0: not set
    int pyr_bands = 0;             // SVGPU_PYR_BANDS (>= 1); 0: not set
    bool describe_bands = false;   // SVGPU_DESCRIBE_BANDS is set
    int fast_cpw = 0;              // SVGPU_FAST_CPW (>= 1); 0: not set
    bool fork_blur = false;        // SVGPU_FORK_BLUR is set
};

struct OrbPlan {
    OrbConfig config;  // `configured` stays false: the caller sets it once the device side exists
    OrbTables tables;
};

namespace orb_plan_detail {

inline int cv_floor_f(float v) {
    int i = (int)v;
    return i - (i > v);
}
inline int cv_round_f(float v) { return (int)lrintf(v); }  // round half to even (default rounding mode)
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// per level and selection-grid row: first / last level row its keypoints can lie on
using GridRows = std::vector<std::pair<int, int>>;

}  // namespace orb_plan_detail

// orb_params.cc:41-71 -- four independent fp32 recurrences (any output may be null)
inline void orb_plan_scale_tables(float scale_factor, int num_levels, float* scale_factors, float* inv_scale_factors, float* level_sigma_sq,
                                  float* inv_level_sigma_sq) {
    float s = 1.0f, inv = 1.0f;
    for (int l = 0; l < num_levels; ++l) {
        if (l > 0) {
            s = scale_factor * s;
            inv = (1.0f / scale_factor) * inv;
        }
        if (scale_factors) scale_factors[l] = s;
        if (inv_scale_factors) inv_scale_factors[l] = inv;
        if (level_sigma_sq) level_sigma_sq[l] = l == 0 ? 1.0f : s * s;
        if (inv_level_sigma_sq) inv_level_sigma_sq[l] = l == 0 ? 1.0f : 1.0f / (s * s);
    }
}

// ---- level l: size, pitch, offsets inside a frame's pyramid / blurred block.  False: the level is smaller than 2 px.
inline bool orb_plan_level(OrbConfig& C, int l, size_t& pyr_off, size_t& blur_off) {
    using namespace orb_plan_detail;
    OrbLevel& L = C.levels[l];
    memset(&L, 0, sizeof(L));
    const float s = C.scale_factors[l];
    if (l == 0) {
        L.w = C.width;
        L.h = C.height;
    }
    else {  // orb_extractor.cc:157-159
        const double scale = (double)s;
        L.w = (int)std::round(C.width * 1.0 / scale);
        L.h = (int)std::round(C.height * 1.0 / scale);
    }
    if (L.w < 2 || L.h < 2) return false;
    L.pitch = (int)align_up(L.w, 64);
    L.scale = s;
    L.kp_size = (float)(unsigned)(31u * s);  // orb_extractor.cc:274
    L.blur_off = (long long)blur_off;
    blur_off += align_up((size_t)L.pitch * L.h, 256);
    if (l > 0) {
        L.pyr_off = (long long)pyr_off;
        pyr_off += align_up((size_t)L.pitch * L.h, 256);
    }
    return true;
}

// ---- resize tables (level l >= 1 from level l-1)
inline void orb_plan_resize_tables(OrbConfig& C, int l, OrbTables& T) {
    using namespace orb_plan_detail;
    OrbLevel& L = C.levels[l];
    const OrbLevel& P = C.levels[l - 1];
    const double inv_scale_x = (double)L.w / P.w, inv_scale_y = (double)L.h / P.h;
    const double scale_x = 1. / inv_scale_x, scale_y = 1. / inv_scale_y;
    L.xtab_off = (int)T.xofs.size();
    L.ytab_off = (int)T.yofs.size();
    for (int dx = 0; dx < L.w; ++dx) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = cv_floor_f(fx);
        fx -= sx;
        if (sx < 0) {
            fx = 0;
            sx = 0;
        }
        if (sx >= P.w - 1) {
            fx = 0;
            sx = P.w - 1;
        }
        T.xofs.push_back((short)sx);
        OrbShort2 a;
        a.x = (short)cv_round_f((1.f - fx) * 2048);
        a.y = (short)cv_round_f(fx * 2048);
        T.xa.push_back(a);
    }
    for (int dy = 0; dy < L.h; ++dy) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = cv_floor_f(fy);
        fy -= sy;
        OrbShort2 o, bb;
        o.x = (short)(sy < 0 ? 0 : (sy > P.h - 1 ? P.h - 1 : sy));
        o.y = (short)(sy + 1 < 0 ? 0 : (sy + 1 > P.h - 1 ? P.h - 1 : sy + 1));
        bb.x = (short)cv_round_f((1.f - fy) * 2048);
        bb.y = (short)cv_round_f(fy * 2048);
        T.yofs.push_back(o);
        T.yb.push_back(bb);
    }
}

// ---- packed records for k_pyramid_lds (level l >= 1).  One record per 4 output columns c..c+3 (columns past w-1 repeat w-1):
//      w0 = dword index of sx[c] | dword index of sx[c+2] << 16 (two 8-byte windows per source row),
//      w1 = byte index inside its window of sx[c], sx[c+1] (window 0), sx[c+2], sx[c+3] (window 1),
//      w2..w5 = (a0 | a1 << 16) of the four columns.  sx+1 is always the next byte (its weight is 0 when clamped).
//      False: the level shrinks by more than 3x (the byte windows of the records do not fit) or a coefficient is negative.
inline bool orb_plan_pyramid_records(OrbConfig& C, int l, OrbTables& T) {
    OrbLevel& L = C.levels[l];
    bool xg_ok = true;
    L.xg_off = (int)(T.xg.size() / 8);
    for (int c = 0; c < L.w; c += 4) {
        int sxs[4];
        for (int i = 0; i < 4; ++i) sxs[i] = T.xofs[L.xtab_off + std::min(c + i, L.w - 1)];
        const int base0 = sxs[0] >> 2, base2 = sxs[2] >> 2;
        const int k[4] = {sxs[0] - 4 * base0, sxs[1] - 4 * base0, sxs[2] - 4 * base2, sxs[3] - 4 * base2};
        for (int i = 0; i < 4; ++i) xg_ok = xg_ok && k[i] >= 0 && k[i] <= 6;
        T.xg.push_back((uint32_t)base0 | ((uint32_t)base2 << 16));
        T.xg.push_back((uint32_t)(k[0] & 255) | ((uint32_t)(k[1] & 255) << 8) | ((uint32_t)(k[2] & 255) << 16) | ((uint32_t)(k[3] & 255) << 24));
        for (int i = 0; i < 4; ++i) {
            const OrbShort2 a = T.xa[L.xtab_off + std::min(c + i, L.w - 1)];
            xg_ok = xg_ok && a.x >= 0 && a.y >= 0;
            T.xg.push_back((uint32_t)(unsigned short)a.x | ((uint32_t)(unsigned short)a.y << 16));
        }
        T.xg.push_back(0);
        T.xg.push_back(0);
    }
    for (int dy = 0; dy < L.h; ++dy) {
        const OrbShort2 o = T.yofs[L.ytab_off + dy], c = T.yb[L.ytab_off + dy];
        xg_ok = xg_ok && c.x >= 0 && c.y >= 0;
        T.yrow.push_back(OrbShort4{o.x, o.y, c.x, c.y});
    }
    return xg_ok;
}

// ---- every coefficient pair of the resize tables sums to at most SV_RESIZE_COEF_SUM_MAX (round(f * 2048) + round((1 - f) * 2048) is 2048,
//      or 2049 when both halves round up).  k_pyramid_lds packs its four results of a row step without masking them to a byte: with
//      a0 + a1 <= 2049 and b0 + b1 <= 2049 no result exceeds 255 (the argument stands at the pack).  Checked on the tables the kernels read --
//      the plain pairs and their packed copies -- so a table that breaks it never reaches the device.
#define SV_RESIZE_COEF_SUM_MAX 2049
inline bool orb_plan_coef_sums_ok(const OrbTables& T) {
    bool ok = true;
    for (const OrbShort2& a : T.xa) ok = ok && (int)a.x + (int)a.y <= SV_RESIZE_COEF_SUM_MAX;
    for (const OrbShort2& b : T.yb) ok = ok && (int)b.x + (int)b.y <= SV_RESIZE_COEF_SUM_MAX;
    for (size_t r = 0; r + 8 <= T.xg.size(); r += 8)
        for (int i = 2; i < 6; ++i) ok = ok && (T.xg[r + i] & 0xffffu) + (T.xg[r + i] >> 16) <= SV_RESIZE_COEF_SUM_MAX;
    for (const OrbShort4& y : T.yrow) ok = ok && (int)y.z + (int)y.w <= SV_RESIZE_COEF_SUM_MAX;
    return ok;
}

// ---- blur tiles and bands of level l
inline void orb_plan_blur_items(OrbConfig& C, int l, int& btile_first, int& bband_first) {
    OrbLevel& L = C.levels[l];
    L.btile_first = btile_first;
    L.btiles_x = (L.w + BLUR_TW - 1) / BLUR_TW;
    L.btiles_y = (L.h + 4 * C.blur_rows - 1) / (4 * C.blur_rows);
    btile_first += L.btiles_x * L.btiles_y + ((L.h + 7) / 8 + 63) / 64;  // + edge tiles (64 strips of BLUR_EDGE_ROWS rows each)
    L.bband_first = bband_first;
    L.bband_segs = (L.w + BLUR_SEG - 1) / BLUR_SEG;
    bband_first += L.bband_segs * ((L.h + BLUR_ROWS - 1) / BLUR_ROWS);
}

// ---- FAST cell lattice and selection grid of level l
inline void orb_plan_cells_and_grid(OrbConfig& C, int l, OrbTables& T, int& grid_first, orb_plan_detail::GridRows& grid_rows) {
    OrbLevel& L = C.levels[l];
    const float s = C.scale_factors[l];
    std::vector<unsigned short>& gtab = T.gtab;
    L.cell_first = (int)C.cells.size();
    L.grid_first = grid_first;
    L.gtab_x_off = L.gtab_y_off = (int)gtab.size();
    if (L.w > 2 * SV_PATCH_RADIUS && L.h > 2 * SV_PATCH_RADIUS) {
        L.has_cells = 1;
        const unsigned min_bx = SV_PATCH_RADIUS, min_by = SV_PATCH_RADIUS;
        const unsigned max_bx = L.w - SV_PATCH_RADIUS, max_by = L.h - SV_PATCH_RADIUS;
        const unsigned rw = max_bx - min_bx, rh = max_by - min_by;
        const unsigned num_cols = rw / SV_CELL + 1, num_rows = rh / SV_CELL + 1;
        L.cells_x = (int)num_cols;
        for (unsigned i = 0; i < num_rows; ++i) {
            const unsigned min_y = min_by + i * SV_CELL;
            if (max_by - SV_OVERLAP <= min_y) continue;
            unsigned max_y = min_y + SV_CELL + SV_OVERLAP;
            if (max_by < max_y) max_y = max_by;
            for (unsigned j = 0; j < num_cols; ++j) {
                const unsigned min_x = min_bx + j * SV_CELL;
                if (max_bx - SV_OVERLAP <= min_x) continue;
                unsigned max_x = min_x + SV_CELL + SV_OVERLAP;
                if (max_bx < max_x) max_x = max_bx;
                FastCell c;
                c.min_x = (short)min_x;
                c.min_y = (short)min_y;
                c.w = (short)(max_x - min_x);
                c.h = (short)(max_y - min_y);
                c.lv = (short)l;
                c.cj = (short)j;
                c.order_base = (int)((i * num_cols + j) << 14);
                C.cells.push_back(c);
            }
        }
        // distribute_keypoints (:292-305)
        const double scaled_min_area_sqrt = C.min_area_sqrt / s;  // fp32 division, widened
        const unsigned gx = (unsigned)std::ceil((int)rw / scaled_min_area_sqrt);
        const unsigned gy = (unsigned)std::ceil((int)rh / scaled_min_area_sqrt);
        const double delta_x = (double)(int)rw / gx, delta_y = (double)(int)rh / gy;
        L.grid_x = (int)gx;
        L.grid_y = (int)gy;
        L.gtab_x_off = (int)gtab.size();
        for (unsigned x = 0; x < rw; ++x) {
            unsigned ix = (unsigned)((float)x / delta_x);
            gtab.push_back((unsigned short)(ix < gx ? ix : gx - 1));
        }
        L.gtab_y_off = (int)gtab.size();
        grid_rows.assign(gy, std::make_pair(1 << 30, -1));
        for (unsigned y = 0; y < rh; ++y) {
            unsigned iy = (unsigned)((float)y / delta_y);
            iy = iy < gy ? iy : gy - 1;
            gtab.push_back((unsigned short)iy);
            grid_rows[iy].first = std::min(grid_rows[iy].first, (int)(min_by + y));
            grid_rows[iy].second = std::max(grid_rows[iy].second, (int)(min_by + y));
        }
        grid_first += (int)(gx * gy);
    }
    L.cell_count = (int)C.cells.size() - L.cell_first;
}

// ---- bands of k_describe_bands: as many consecutive selection-grid rows of a level as fit the LDS budget (and DB_MAX_KP = 128 keypoints).
//      A keypoint of grid row g lies on level rows [first(g), last(g)]; its patches need rows y - 15 .. y + 16 (un-blurred; row y + 16 carries
//      zero weights but is read) and y - 18 .. y + 18 (blurred).  LDS pitch: the level width rounded up to 16-byte pieces, then to 32 mod 64
//      (eight rows of dword reads then fall into 64 different banks); pieces beyond the level's own pitch read the next row's first bytes.
inline void orb_plan_describe_bands(OrbConfig& C, const orb_plan_detail::GridRows* grid_rows, const OrbEnv& env) {
    const int num_levels = C.num_levels;
    C.dbands.clear();
    C.dband_lds_bytes = 0;
    size_t budget = 48 * 1024;  // three 512-thread workgroups per CU
    if (env.desc_band_kb) budget = (size_t)env.desc_band_kb * 1024;
    const size_t hard_limit = 80 * 1024;  // two workgroups per CU; wider images than that take k_describe
    bool ok = C.total_grid > 0 && !env.describe_legacy;
    for (int l = 0; l < num_levels && ok; ++l) {
        const OrbLevel& L = C.levels[l];
        if (!L.has_cells) continue;
        int lp = (L.w + 15) / 16 * 16;
        while (lp % 64 != 32) lp += 16;
        if (lp > 32000) ok = false;
        const int gy = L.grid_y, gx = L.grid_x;
        auto band_bytes = [&](int g0, int g1, DescBand* out) {  // rows of grid rows [g0, g1)
            int y0 = 1 << 30, y1 = -1;
            for (int g = g0; g < g1; ++g)
                if (grid_rows[l][g].second >= 0) {
                    y0 = std::min(y0, grid_rows[l][g].first);
                    y1 = std::max(y1, grid_rows[l][g].second);
                }
            if (y1 < 0) y0 = y1 = SV_PATCH_RADIUS;  // (grid rows no level row maps to: no keypoints either)
            const int nru = y1 - y0 + 32, nrb = y1 - y0 + 37;
            const int rpi = std::max(1, 64 / (lp / 16));  // a staging instruction carries whole groups of rpi rows: room for the last group
            const size_t bytes = (size_t)((std::max(nru, nrb) + rpi - 1) / rpi * rpi) * lp;
            if (out) {
                out->lv = (short)l;
                out->lp = (short)lp;
                out->yu0 = (short)(y0 - 15);
                out->nru = (short)nru;
                out->yb0 = (short)(y0 - 18);
                out->nrb = (short)nrb;
                out->img_bytes = (int)bytes;
                out->cell0 = L.grid_first + g0 * gx;
                out->cell1 = L.grid_first + g1 * gx;
            }
            return bytes;
        };
        if (gx > 128) ok = false;
        for (int g0 = 0; g0 < gy && ok;) {
            int g1 = g0 + 1;
            if (band_bytes(g0, g1, nullptr) > hard_limit) ok = false;
            while (g1 < gy && (g1 + 1 - g0) * gx <= 128 && band_bytes(g0, g1 + 1, nullptr) <= budget) ++g1;
            DescBand bd;
            C.dband_lds_bytes = std::max(C.dband_lds_bytes, band_bytes(g0, g1, &bd));
            C.dbands.push_back(bd);
            g0 = g1;
        }
    }
    if (!ok) C.dbands.clear();
    // heaviest bands first (level 0 stages the most bytes per keypoint): the tail of the launch is made of the light ones
    std::stable_sort(C.dbands.begin(), C.dbands.end(), [](const DescBand& a, const DescBand& b) { return a.img_bytes > b.img_bytes; });
    if (!C.dbands.empty()) C.dband_lds_bytes += 2 * 128 * sizeof(OrbInt2);  // + the per-keypoint arrays (DB_MAX_KP)
}

// ---- pyramid bands: band k owns rows [k*h/K, (k+1)*h/K) of every level; bottom-up it also needs the source rows
//      of everything it computes at the next level (two taps per output row, clamped -- the yofs table).
//      Returns the largest per-band LDS footprint of k_pyramid_lds.
inline size_t orb_plan_make_pyramid_bands(const OrbConfig& C, const OrbTables& T, int bands, std::vector<OrbInt2>& band_rows) {
    const int num_levels = C.num_levels;
    band_rows.assign((size_t)bands * num_levels, OrbInt2{0, 0});
    size_t worst = 0;
    for (int k = 0; k < bands; ++k) {
        int need_lo = 0, need_hi = 0;
        for (int l = num_levels - 1; l >= 1; --l) {
            const OrbLevel& Lv = C.levels[l];
            int lo = (int)((long long)k * Lv.h / bands), hi = (int)((long long)(k + 1) * Lv.h / bands);
            if (l < num_levels - 1 && need_hi > need_lo) {
                lo = std::min(lo, need_lo);
                hi = std::max(hi, need_hi);
            }
            band_rows[(size_t)k * num_levels + l] = OrbInt2{lo, hi};
            // rows of level l-1 read by rows [lo, hi) of level l
            need_lo = 1 << 30;
            need_hi = 0;
            for (int dy = lo; dy < hi; ++dy) {
                const OrbShort2 o = T.yofs[Lv.ytab_off + dy];
                need_lo = std::min(need_lo, (int)o.x);
                need_hi = std::max(need_hi, (int)o.y + 1);
            }
        }
        if (need_hi > need_lo) band_rows[(size_t)k * num_levels] = OrbInt2{need_lo, need_hi};  // level-0 rows the band reads
        size_t size_a = 0, size_b = 0;  // must mirror the LDS map of k_pyramid_lds: odd / even levels (level 0 included) alternate in two regions
        for (int l = 0; l < num_levels; ++l) {
            const OrbInt2 r = band_rows[(size_t)k * num_levels + l];
            const size_t b = (size_t)(r.y - r.x) * (size_t)((C.levels[l].w + 3) & ~3);
            if (l & 1) size_a = std::max(size_a, b);
            else size_b = std::max(size_b, b);
        }
        size_a = (size_a + 15) & ~(size_t)15;
        size_b = (size_b + 15) & ~(size_t)15;
        size_t bytes = size_a + size_b;
        for (int l = 1; l < num_levels; ++l) {
            const OrbInt2 r = band_rows[(size_t)k * num_levels + l];
            bytes += (size_t)(r.y - r.x) * 8;
        }
        worst = std::max(worst, bytes);
    }
    return worst;
}

// ---- the band count K: the smallest (>= the starting count) whose per-band LDS footprint fits k_pyramid_lds; none fits -> global variant.
inline void orb_plan_pyramid_bands(OrbConfig& C, OrbTables& T, bool xg_ok, const OrbEnv& env) {
    const int num_levels = C.num_levels, max_batch = C.max_batch;
    // few, tall bands recompute the fewest halo rows; small batches need more bands to fill the 256 CUs.  A footprint of at most half the
    // CU's LDS lets two workgroups share a CU (one computes while the other waits at a level barrier): preferred while <= 32 bands reach it.
    int bands = std::max(8, std::min(32, (512 + max_batch - 1) / std::max(max_batch, 1)));
    bool forced = false;
    if (env.pyr_bands) {
        bands = env.pyr_bands;
        forced = true;
    }
    xg_ok = xg_ok && (num_levels < 2 || C.levels[1].w <= 4 * 1024);  // one thread per column group of a level: at most 1024 groups
    size_t lds = 0;
    if (!forced && xg_ok) {
        std::vector<OrbInt2> trial;
        for (int k = bands; k <= 32; k += 2)
            if (orb_plan_make_pyramid_bands(C, T, k, trial) <= SV_PYR_LDS_HALF) {
                bands = k;
                break;
            }
    }
    for (;; bands += 2) {
        lds = orb_plan_make_pyramid_bands(C, T, bands, T.band_rows);
        if (lds <= SV_PYR_LDS_MAX && xg_ok) break;
        if (bands >= 256 || !xg_ok) {  // very wide images: chain the levels through global memory instead (k_pyramid)
            bands = 16;
            orb_plan_make_pyramid_bands(C, T, bands, T.band_rows);
            lds = 0;
            break;
        }
    }
    C.pyr_bands = bands;
    C.pyr_lds_bytes = lds;
}

// Everything svgpu_orb_configure decides before it touches the device.  The caller has range-checked the arguments (8 <= width, height
// <= 16384, max_batch >= 1, 1 <= num_levels <= SV_MAX_LEVELS, scale_factor > 1).  Returns null, or the text of the error.
inline const char* orb_plan_build(int width, int height, int max_batch, float scale_factor, int num_levels, int ini_fast_thr, int min_fast_thr,
                                  unsigned min_area, const OrbEnv& env, OrbPlan& plan) {
    plan = OrbPlan();
    OrbConfig& C = plan.config;
    OrbTables& T = plan.tables;
    C.width = width;
    C.height = height;
    C.max_batch = max_batch;
    C.blur_rows = max_batch <= BLUR_SMALL_BATCH ? BLUR_ROWS_SMALL : BLUR_ROWS;
    C.num_levels = num_levels;
    C.scale_factor = scale_factor;
    C.ini_thr = ini_fast_thr < 0 ? 0 : (ini_fast_thr > 255 ? 255 : ini_fast_thr);  // cv::FAST clamps (fast.cpp)
    C.min_thr = min_fast_thr < 0 ? 0 : (min_fast_thr > 255 ? 255 : min_fast_thr);
    C.min_area_sqrt = (unsigned)std::sqrt((double)min_area);  // orb_extractor.cc:20 (unsigned member)
    orb_plan_scale_tables(scale_factor, num_levels, C.scale_factors, nullptr, nullptr, nullptr);

    bool xg_ok = true;  // false: the packed records of k_pyramid_lds cannot express some level
    size_t pyr_off = 0, blur_off = 0;
    int grid_first = 0, btile_first = 0, bband_first = 0;
    orb_plan_detail::GridRows grid_rows[SV_MAX_LEVELS];
    for (int l = 0; l < num_levels; ++l) {
        if (!orb_plan_level(C, l, pyr_off, blur_off)) return "pyramid level smaller than 2 px";
        if (l > 0) {
            orb_plan_resize_tables(C, l, T);
            xg_ok = orb_plan_pyramid_records(C, l, T) && xg_ok;
        }
        orb_plan_blur_items(C, l, btile_first, bband_first);
        orb_plan_cells_and_grid(C, l, T, grid_first, grid_rows[l]);
    }
    if (!orb_plan_coef_sums_ok(T)) return "resize coefficient pair sums to more than 2049";
    C.total_grid = grid_first;
    C.total_btiles = btile_first;
    C.total_bbands = bband_first;
    orb_plan_describe_bands(C, grid_rows, env);
    C.pyr_frame_bytes = pyr_off ? pyr_off : 256;
    C.blur_frame_bytes = blur_off;
    orb_plan_pyramid_bands(C, T, xg_ok, env);
    return nullptr;
}

// ---- what one extract call launches
struct OrbLaunch {
    bool pyramid_lds;     // k_pyramid_lds; false: k_pyramid, the levels chained through global memory
    bool blur_bands;      // k_blur<BLUR_ROWS> (row bands in LDS); false: the streaming kernel k_blur<BLUR_ROWS_SMALL>
    bool need_gather;     // k_blur_gather runs behind either blur kernel for the levels it cannot take
    int fast_cpw;         // FAST cells per workgroup of k_fast
    bool describe_bands;  // k_describe_bands; false: the per-keypoint kernel k_describe
};

#define ORB_FAST_CPW4_MIN_CELLS 16384     // cells x batch from which a k_fast workgroup takes four cells
#define ORB_DESCRIBE_BANDS_MIN_KP 32768   // batch x total_grid from which k_describe_bands describes the keypoints

inline OrbLaunch orb_launch_plan(const OrbConfig& C, int batch, bool caller_image_4byte_aligned, const OrbEnv& env) {
    OrbLaunch P;
    P.pyramid_lds = C.pyr_lds_bytes > 0;
    // a context configured for a few frames streams (latency); any larger one takes the band kernel whatever the batch it is given
    P.blur_bands = C.blur_rows != BLUR_ROWS_SMALL;
    // levels the band / streaming kernel cannot take (caller image not 4-byte aligned, level narrower than 16 px) -> gather kernel
    P.need_gather = !caller_image_4byte_aligned;
    for (int l = 0; l < C.num_levels; ++l) P.need_gather = P.need_gather || C.levels[l].w < 16;
    // cells per workgroup: four once the batch alone fills the chip many times over, one for a few frames (latency: more workgroups)
    P.fast_cpw = (long long)C.cells.size() * batch >= ORB_FAST_CPW4_MIN_CELLS ? 4 : 1;
    if (env.fast_cpw) P.fast_cpw = env.fast_cpw;
    // bands when the batch alone fills the chip (they are bound by throughput: 0.80 against 1.20 ms per 1 024 frames); for a few frames the
    // per-keypoint kernel's many short workgroups finish sooner (one frame: 11 against 17 us, break-even near 16 frames of 2 400 keypoints)
    P.describe_bands = !C.dbands.empty() && ((long long)batch * C.total_grid >= ORB_DESCRIBE_BANDS_MIN_KP || env.describe_bands);
    return P;
}
