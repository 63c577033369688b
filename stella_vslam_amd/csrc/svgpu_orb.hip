// Host side of the ORB front end: environment switches, device workspace (uploads what the planner of orb_plan.h returns), launch sequence.
#include <cstdlib>

#include "svgpu_internal.h"

namespace {

// The ORB environment switches, all read here (a switch that takes a number: at least 1):
//   name                    takes effect at      meaning
//   SVGPU_DESCRIBE_LEGACY   configure            no band table: the per-keypoint kernel k_describe serves every batch
//   SVGPU_DESC_BAND_KB      configure            LDS budget of a band of k_describe_bands in KB (default 48)
//   SVGPU_PYR_BANDS         configure            pyramid bands per frame, taken as given (no search for the count that fits half a CU's LDS)
//   SVGPU_DESCRIBE_BANDS    every extract call   k_describe_bands for any batch, where the configuration has a band table
//   SVGPU_FAST_CPW          every extract call   FAST cells per workgroup of k_fast
//   SVGPU_FORK_BLUR         once per process     the blur runs on the auxiliary stream beside FAST and selection (opt-in)
// svgpu_orb_configure and every extract call read them afresh; each uses only its own rows of the table.
OrbEnv orb_env() {
    auto number = [](const char* name) {
        const char* e = getenv(name);
        return e ? std::max(1, atoi(e)) : 0;
    };
    static const bool fork_blur = getenv("SVGPU_FORK_BLUR") != nullptr;
    OrbEnv E;
    E.describe_legacy = getenv("SVGPU_DESCRIBE_LEGACY") != nullptr;
    E.desc_band_kb = number("SVGPU_DESC_BAND_KB");
    E.pyr_bands = number("SVGPU_PYR_BANDS");
    E.describe_bands = getenv("SVGPU_DESCRIBE_BANDS") != nullptr;
    E.fast_cpw = number("SVGPU_FAST_CPW");
    E.fork_blur = fork_blur;
    return E;
}

// D: the element type the kernels read; H: the planner's plain twin of it
template <class D, class H>
int upload(svgpu_ctx* ctx, D** dptr, const std::vector<H>& v) {
    static_assert(sizeof(D) == sizeof(H) && alignof(D) == alignof(H), "a planner table element must be layout-equal to what the kernels read");
    if (*dptr) {
        SV_HIP(ctx, hipFree(*dptr));
        *dptr = nullptr;
    }
    const size_t n = v.empty() ? 1 : v.size();
    SV_HIP(ctx, hipMalloc((void**)dptr, n * sizeof(D)));
    if (!v.empty()) SV_HIP(ctx, hipMemcpy(*dptr, v.data(), v.size() * sizeof(D), hipMemcpyHostToDevice));
    return SVGPU_OK;
}

template <class T>
void free_dev(T*& p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}

}  // namespace

void sv_orb_release(svgpu_ctx* ctx) {
    free_dev(ctx->d_levels);
    free_dev(ctx->d_cells);
    free_dev(ctx->d_xofs);
    free_dev(ctx->d_xa);
    free_dev(ctx->d_yofs);
    free_dev(ctx->d_yb);
    free_dev(ctx->d_xg);
    free_dev(ctx->d_yrow);
    free_dev(ctx->d_band_rows);
    free_dev(ctx->d_gtab);
    free_dev(ctx->d_pyr);
    free_dev(ctx->d_blur);
    free_dev(ctx->d_keys);
    free_dev(ctx->d_sel);
    free_dev(ctx->d_cellpos);
    free_dev(ctx->d_dbands);
    free_dev(ctx->d_img);
    free_dev(ctx->d_mask);
    free_dev(ctx->d_kps);
    free_dev(ctx->d_desc);
    free_dev(ctx->d_counts);
    ctx->orb.configured = false;
    ctx->last_extract_n = -1;  // d_kps / d_desc are gone: nothing left to adopt (svgpu_frame_adopt_extraction)
    ctx->last_batch = 0;
}

extern "C" {

int svgpu_orb_scale_tables(float scale_factor, int num_levels, float* scale_factors, float* inv_scale_factors,
                           float* level_sigma_sq, float* inv_level_sigma_sq) {
    if (num_levels < 1) return SVGPU_ERR_INVALID;
    orb_plan_scale_tables(scale_factor, num_levels, scale_factors, inv_scale_factors, level_sigma_sq, inv_level_sigma_sq);
    return SVGPU_OK;
}

int svgpu_orb_configure(svgpu_ctx* ctx, int width, int height, int max_batch, float scale_factor, int num_levels,
                        int ini_fast_thr, int min_fast_thr, unsigned min_area) {
    if (!ctx) return SVGPU_ERR_INVALID;
    if (width < 8 || height < 8 || width > 16384 || height > 16384 || max_batch < 1 || num_levels < 1
        || num_levels > SV_MAX_LEVELS || !(scale_factor > 1.0f))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_orb_configure: bad geometry/parameters");
    SV_HIP(ctx, hipSetDevice(ctx->device));
    SV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    sv_orb_release(ctx);
    OrbPlan plan;
    if (const char* err = orb_plan_build(width, height, max_batch, scale_factor, num_levels, ini_fast_thr, min_fast_thr, min_area, orb_env(), plan))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, err);
    OrbConfig& C = ctx->orb;
    C = std::move(plan.config);
    const OrbTables& T = plan.tables;
    const std::vector<OrbLevel> lv(C.levels, C.levels + num_levels);
    int rc;
    if ((rc = upload(ctx, &ctx->d_band_rows, T.band_rows))) return rc;  // int2 <- OrbInt2
    if ((rc = upload(ctx, &ctx->d_levels, lv))) return rc;
    if ((rc = upload(ctx, &ctx->d_cells, C.cells))) return rc;
    if ((rc = upload(ctx, &ctx->d_xofs, T.xofs))) return rc;
    if ((rc = upload(ctx, &ctx->d_xa, T.xa))) return rc;      // short2 <- OrbShort2
    if ((rc = upload(ctx, &ctx->d_yofs, T.yofs))) return rc;  // short2 <- OrbShort2
    if ((rc = upload(ctx, &ctx->d_yb, T.yb))) return rc;      // short2 <- OrbShort2
    if ((rc = upload(ctx, &ctx->d_xg, T.xg))) return rc;
    if ((rc = upload(ctx, &ctx->d_yrow, T.yrow))) return rc;  // short4 <- OrbShort4
    if ((rc = upload(ctx, &ctx->d_gtab, T.gtab))) return rc;
    if (C.pyr_lds_bytes) SV_HIP(ctx, sv_pyramid_prepare());
    if (!C.dbands.empty()) {
        if ((rc = upload(ctx, &ctx->d_dbands, C.dbands))) return rc;
        SV_HIP(ctx, sv_describe_bands_prepare(C.dband_lds_bytes));
    }
    const size_t B = (size_t)max_batch, G = (size_t)(C.total_grid > 0 ? C.total_grid : 1);
    SV_HIP(ctx, hipMalloc((void**)&ctx->d_pyr, B * C.pyr_frame_bytes + 256));
    SV_HIP(ctx, hipMalloc((void**)&ctx->d_blur, B * C.blur_frame_bytes + 4096));  // + slack: the band kernel's row pieces run past the last row's end
    SV_HIP(ctx, hipMalloc((void**)&ctx->d_cellpos, B * (G + 1) * sizeof(int32_t)));
    SV_HIP(ctx, hipMalloc((void**)&ctx->d_keys, B * G * sizeof(unsigned long long)));
    SV_HIP(ctx, hipMemset(ctx->d_keys, 0, B * G * sizeof(unsigned long long)));
    SV_HIP(ctx, hipMalloc((void**)&ctx->d_sel, (B * G + 8) * sizeof(int4)));  // + slack: k_describe reads whole groups of DESC_KPW entries
    // staging for the single-frame host entry point
    SV_HIP(ctx, hipMalloc((void**)&ctx->d_img, (size_t)C.levels[0].pitch * height));
    SV_HIP(ctx, hipMalloc((void**)&ctx->d_mask, (size_t)C.levels[0].pitch * height));
    SV_HIP(ctx, hipMalloc((void**)&ctx->d_kps, G * sizeof(svgpu_keypoint)));
    SV_HIP(ctx, hipMalloc((void**)&ctx->d_desc, G * 32));
    SV_HIP(ctx, hipMalloc((void**)&ctx->d_counts, (1 + SV_MAX_LEVELS) * sizeof(int32_t)));
    C.configured = true;
    return SVGPU_OK;
}

int svgpu_orb_max_keypoints(const svgpu_ctx* ctx) { return (ctx && ctx->orb.configured) ? ctx->orb.total_grid : -1; }

int svgpu_orb_level_size(const svgpu_ctx* ctx, int level, int* width, int* height) {
    if (!ctx || !ctx->orb.configured) return SVGPU_ERR_NOT_CONFIGURED;
    if (level < 0 || level >= ctx->orb.num_levels) return SVGPU_ERR_INVALID;
    if (width) *width = ctx->orb.levels[level].w;
    if (height) *height = ctx->orb.levels[level].h;
    return SVGPU_OK;
}

int svgpu_orb_extract_batch_device(svgpu_ctx* ctx, const uint8_t* imgs_dev, int batch, size_t frame_stride,
                                   int row_stride, const uint8_t* mask_dev, size_t mask_frame_stride,
                                   int mask_row_stride, svgpu_keypoint* kps_dev, uint8_t* desc_dev, int cap,
                                   int32_t* counts_dev, void* stream) {
    return svgpu_orb_extract_batch_device_angles(ctx, imgs_dev, batch, frame_stride, row_stride, mask_dev, mask_frame_stride, mask_row_stride, kps_dev, desc_dev, cap,
                                                 counts_dev, nullptr, stream);
}

int svgpu_orb_extract_batch_device_angles(svgpu_ctx* ctx, const uint8_t* imgs_dev, int batch, size_t frame_stride,
                                          int row_stride, const uint8_t* mask_dev, size_t mask_frame_stride,
                                          int mask_row_stride, svgpu_keypoint* kps_dev, uint8_t* desc_dev, int cap,
                                          int32_t* counts_dev, float* angles_dev, void* stream) {
    if (!ctx) return SVGPU_ERR_INVALID;
    OrbConfig& C = ctx->orb;
    if (!C.configured) return sv_set_error(ctx, SVGPU_ERR_NOT_CONFIGURED, "svgpu_orb_configure has not been called");
    if (!imgs_dev || !kps_dev || !desc_dev || !counts_dev || batch < 1 || batch > C.max_batch || cap < 1
        || row_stride < C.width)
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_orb_extract_batch_device: bad arguments");
    SV_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    ctx->last_extract_n = -1;  // whatever the last svgpu_orb_extract left behind is stale from here on (it sets the count again after its own call)
    // 0. plan: which kernels this call takes, and the images every one of them reads
    const OrbEnv env = orb_env();
    const bool aligned = (((size_t)imgs_dev | (size_t)frame_stride | (size_t)row_stride) & 3) == 0;
    const OrbLaunch plan = orb_launch_plan(C, batch, aligned, env);
    const OrbFrames F{ctx->d_levels, C.num_levels, imgs_dev, frame_stride, row_stride, ctx->d_pyr, C.pyr_frame_bytes, ctx->d_blur, C.blur_frame_bytes, batch};
    // 1. pyramid: chained bilinear resize (level l from level l-1), all levels in one launch (banded, see k_pyramid)
    if (C.num_levels > 1) {
        SvProfScope ps(ctx, s, "k_resize");
        sv_launch_pyramid(s, F, plan, ctx->d_band_rows, C.pyr_bands, C.pyr_lds_bytes, ctx->d_xofs, ctx->d_xa, ctx->d_yofs, ctx->d_yb, ctx->d_xg, ctx->d_yrow);
    }
    // 2. blurred copy of every level -- on the auxiliary stream, beside steps 3-4: the blur waits on memory where FAST is bound by
    //    instruction issue, so the two share the CUs well; step 5 joins them
    hipStream_t sb = (ctx->stream_aux && env.fork_blur) ? ctx->stream_aux : s;
    if (sb != s) {
        SV_HIP(ctx, hipEventRecord(ctx->ev_fork, s));
        SV_HIP(ctx, hipStreamWaitEvent(sb, ctx->ev_fork, 0));
    }
    {
        SvProfScope ps(ctx, sb, "k_blur");
        sv_launch_blur(sb, F, plan, C.total_btiles, C.total_bbands);
    }
    if (sb != s) SV_HIP(ctx, hipEventRecord(ctx->ev_join, sb));
    // 3. FAST per cell + selection-grid arg-max
    SV_HIP(ctx, hipEventRecord(ctx->ev_stage[0], s));
    {
        SvProfScope ps(ctx, s, "k_fast");
        sv_launch_fast(s, F, plan.fast_cpw, ctx->d_cells, (int)C.cells.size(), ctx->d_gtab, ctx->d_keys, C.total_grid, C.ini_thr, C.min_thr, mask_dev,
                       mask_frame_stride, mask_row_stride, C.width, C.height);
    }
    // 4. ordered compaction (+ key reset for the next call)
    {
        SvProfScope ps(ctx, s, "k_select");
        sv_launch_select(s, F, ctx->d_keys, C.total_grid, ctx->d_sel, counts_dev, C.dbands.empty() ? nullptr : ctx->d_cellpos);
    }
    // 5. orientation, descriptor, scale correction
    if (sb != s) SV_HIP(ctx, hipStreamWaitEvent(s, ctx->ev_join, 0));
    SV_HIP(ctx, hipEventRecord(ctx->ev_stage[1], s));
    ctx->stage_recorded = true;
    SvProfScope ps(ctx, s, "k_describe");
    if (plan.describe_bands)
        sv_launch_describe_bands(s, F, ctx->d_dbands, (int)C.dbands.size(), C.dband_lds_bytes, ctx->d_sel, C.total_grid, ctx->d_cellpos, counts_dev, kps_dev,
                                 desc_dev, cap, angles_dev);
    else
        sv_launch_describe(s, F, ctx->d_sel, C.total_grid, counts_dev, kps_dev, desc_dev, cap, angles_dev);
    SV_HIP(ctx, hipGetLastError());
    ctx->last_batch = batch;
    ctx->last_imgs = imgs_dev;
    ctx->last_frame_stride = frame_stride;
    ctx->last_row_stride = row_stride;
    return SVGPU_OK;
}

int svgpu_orb_stream_wait_stage(svgpu_ctx* ctx, int stage, void* stream) {
    if (!ctx || stage < 0 || stage > 1 || !stream) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_orb_stream_wait_stage: bad arguments");
    if (!ctx->stage_recorded) return SVGPU_OK;  // no extraction enqueued yet: nothing to wait for
    SV_HIP(ctx, hipSetDevice(ctx->device));
    SV_HIP(ctx, hipStreamWaitEvent((hipStream_t)stream, ctx->ev_stage[stage], 0));
    return SVGPU_OK;
}

int svgpu_orb_extract(svgpu_ctx* ctx, const uint8_t* img, int stride, const uint8_t* mask, int mask_stride,
                      svgpu_keypoint* kps, uint8_t* desc, int cap, int* n_out, int* level_counts) {
    if (!ctx) return SVGPU_ERR_INVALID;
    OrbConfig& C = ctx->orb;
    if (!C.configured) return sv_set_error(ctx, SVGPU_ERR_NOT_CONFIGURED, "svgpu_orb_configure has not been called");
    if (!img || !n_out || stride < C.width || cap < 0 || (cap > 0 && (!kps || !desc)) || (mask && mask_stride < C.width))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_orb_extract: bad arguments");
    SV_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int pitch = C.levels[0].pitch;
    SV_HIP(ctx, hipMemcpy2DAsync(ctx->d_img, pitch, img, stride, C.width, C.height, hipMemcpyHostToDevice, s));
    if (mask) SV_HIP(ctx, hipMemcpy2DAsync(ctx->d_mask, pitch, mask, mask_stride, C.width, C.height, hipMemcpyHostToDevice, s));
    const int icap = C.total_grid > 0 ? C.total_grid : 1;
    int rc = svgpu_orb_extract_batch_device(ctx, ctx->d_img, 1, (size_t)pitch * C.height, pitch, mask ? ctx->d_mask : nullptr, 0,
                                            pitch, ctx->d_kps, ctx->d_desc, icap, ctx->d_counts, s);
    if (rc) return rc;
    int32_t counts[1 + SV_MAX_LEVELS];
    SV_HIP(ctx, hipMemcpyAsync(counts, ctx->d_counts, (1 + C.num_levels) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SV_HIP(ctx, hipStreamSynchronize(s));
    const int n = counts[0];
    *n_out = n;
    ctx->last_extract_n = n < icap ? n : icap;
    if (level_counts)
        for (int l = 0; l < C.num_levels; ++l) level_counts[l] = counts[1 + l];
    const int m = n < cap ? n : cap;
    if (m > 0) {
        SV_HIP(ctx, hipMemcpyAsync(kps, ctx->d_kps, (size_t)m * sizeof(svgpu_keypoint), hipMemcpyDeviceToHost, s));
        SV_HIP(ctx, hipMemcpyAsync(desc, ctx->d_desc, (size_t)m * 32, hipMemcpyDeviceToHost, s));
        SV_HIP(ctx, hipStreamSynchronize(s));
    }
    return n > cap ? sv_set_error(ctx, SVGPU_ERR_CAPACITY, "svgpu_orb_extract: more keypoints than cap") : SVGPU_OK;
}

static int download_level(svgpu_ctx* ctx, const uint8_t* base, size_t frame_bytes, long long off, int frame, int level,
                          uint8_t* dst, int dst_stride) {
    OrbConfig& C = ctx->orb;
    const OrbLevel& L = C.levels[level];
    if (!dst || dst_stride < L.w) return sv_set_error(ctx, SVGPU_ERR_INVALID, "download: bad destination");
    SV_HIP(ctx, hipSetDevice(ctx->device));
    SV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SV_HIP(ctx, hipMemcpy2D(dst, dst_stride, base + (size_t)frame * frame_bytes + off, L.pitch, L.w, L.h, hipMemcpyDeviceToHost));
    return SVGPU_OK;
}

int svgpu_orb_pyramid_download(svgpu_ctx* ctx, int frame, int level, uint8_t* dst, int dst_stride) {
    if (!ctx) return SVGPU_ERR_INVALID;
    OrbConfig& C = ctx->orb;
    if (!C.configured || ctx->last_batch == 0) return sv_set_error(ctx, SVGPU_ERR_NOT_CONFIGURED, "no extract call yet");
    if (frame < 0 || frame >= ctx->last_batch || level < 0 || level >= C.num_levels)
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "pyramid_download: bad frame/level");
    if (level == 0) {
        if (!dst || dst_stride < C.width) return sv_set_error(ctx, SVGPU_ERR_INVALID, "download: bad destination");
        SV_HIP(ctx, hipSetDevice(ctx->device));
        SV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        SV_HIP(ctx, hipMemcpy2D(dst, dst_stride, ctx->last_imgs + (size_t)frame * ctx->last_frame_stride, ctx->last_row_stride,
                                C.width, C.height, hipMemcpyDeviceToHost));
        return SVGPU_OK;
    }
    return download_level(ctx, ctx->d_pyr, C.pyr_frame_bytes, C.levels[level].pyr_off, frame, level, dst, dst_stride);
}

int svgpu_orb_blurred_download(svgpu_ctx* ctx, int frame, int level, uint8_t* dst, int dst_stride) {
    if (!ctx) return SVGPU_ERR_INVALID;
    OrbConfig& C = ctx->orb;
    if (!C.configured || ctx->last_batch == 0) return sv_set_error(ctx, SVGPU_ERR_NOT_CONFIGURED, "no extract call yet");
    if (frame < 0 || frame >= ctx->last_batch || level < 0 || level >= C.num_levels)
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "blurred_download: bad frame/level");
    return download_level(ctx, ctx->d_blur, C.blur_frame_bytes, C.levels[level].blur_off, frame, level, dst, dst_stride);
}

}  // extern "C"
