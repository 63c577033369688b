// svgpu_ingest_*: host glue of the image ingest kernels (ingest_kernels.hip).  Every argument is checked before anything is launched;
// map VALUES are never checked (the compiled map clamps, tests/ingest_problems.py says what an entry outside the source gives).
#include <cmath>
#include <new>

#include "ingest_kernels.h"
#include "svgpu_internal.h"

namespace {

inline size_t pad16(size_t b) { return (b + 15) & ~size_t(15); }

bool depth_args_ok(const void* src, int src_type, int src_stride, int width, int height, double factor, const float* dst, int dst_stride) {
    if (!src || !dst || width < 1 || height < 1 || height > 65535 || !std::isfinite(factor) || factor == 0.0) return false;
    const int es = src_type == SVGPU_DEPTH_U16 ? 2 : src_type == SVGPU_DEPTH_F32 ? 4 : 0;
    if (!es || (long long)src_stride < (long long)width * es || (long long)dst_stride < (long long)width * 4) return false;
    return src_stride % es == 0 && dst_stride % 4 == 0 && (uintptr_t)src % es == 0 && (uintptr_t)dst % 4 == 0;
}

}  // namespace

extern "C" {

int svgpu_ingest_create(svgpu_ctx* ctx, int width, int height, int channels, int color_order, const float* map_x, const float* map_y, int map_stride,
                        svgpu_ingest** out) {
    if (!ctx || !out || width < 1 || height < 1 || width > 32760 || height > 32760 || (channels != 1 && channels != 3 && channels != 4)
        || color_order < SVGPU_COLOR_GRAY || color_order > SVGPU_COLOR_BGR || (channels != 1 && color_order == SVGPU_COLOR_GRAY) || (!map_x) != (!map_y)
        || (map_x && ((long long)map_stride < (long long)width * 4 || map_stride % 4 != 0)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_ingest_create: bad arguments");
    SV_HIP(ctx, hipSetDevice(ctx->device));
    svgpu_ingest* g = new (std::nothrow) svgpu_ingest();
    if (!g) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_ingest_create: out of memory");
    g->device = ctx->device, g->width = width, g->height = height, g->channels = channels, g->color_order = color_order;
    if (map_x) {
        // the float maps go down once, are compiled, and are dropped
        g->map_pitch = width;
        const size_t fbytes = (size_t)width * height * 4;
        float* d_f = nullptr;
        hipError_t e = hipMalloc((void**)&d_f, 2 * fbytes);
        if (e == hipSuccess) e = hipMalloc((void**)&g->d_map, (size_t)g->map_pitch * height * sizeof(uint2));
        if (e == hipSuccess) e = hipMemcpy2DAsync(d_f, (size_t)width * 4, map_x, (size_t)map_stride, (size_t)width * 4, height, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess)
            e = hipMemcpy2DAsync(d_f + (size_t)width * height, (size_t)width * 4, map_y, (size_t)map_stride, (size_t)width * 4, height, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) {
            sv_launch_ingest_compile_map(ctx->stream, d_f, d_f + (size_t)width * height, width, width, height, g->d_map, g->map_pitch);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (d_f) (void)hipFree(d_f);
        if (e != hipSuccess) {
            if (g->d_map) (void)hipFree(g->d_map);
            delete g;
            return sv_set_error(ctx, SVGPU_ERR_HIP, "svgpu_ingest_create: compiling the maps", e);
        }
    }
    *out = g;
    return SVGPU_OK;
}

void svgpu_ingest_destroy(svgpu_ingest* g) {
    if (!g) return;
    if (g->d_map) {
        (void)hipSetDevice(g->device);
        (void)hipFree(g->d_map);
    }
    delete g;
}

int svgpu_ingest_gray_batch_device(svgpu_ctx* ctx, const svgpu_ingest* g, const uint8_t* src_dev, int batch, size_t src_frame_stride, int src_row_stride,
                                   uint8_t* dst_dev, size_t dst_frame_stride, int dst_row_stride, void* stream) {
    if (!ctx || !g || batch < 0 || batch > 65535 || g->device != ctx->device) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_ingest_gray_batch_device: bad arguments");
    if (batch == 0) return SVGPU_OK;
    const long long src_row = (long long)g->width * g->channels;
    if (!src_dev || !dst_dev || src_row_stride < src_row || dst_row_stride < g->width || (long long)src_row_stride * g->height > 0x7fffffffLL
        || (batch > 1 && (src_frame_stride < (size_t)src_row_stride * (g->height - 1) + (size_t)src_row || dst_frame_stride < (size_t)dst_row_stride * (g->height - 1) + (size_t)g->width)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_ingest_gray_batch_device: a stride is shorter than a row (or a frame)");
    SV_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    IngestProblem P{};
    P.src = src_dev, P.src_frame_stride = src_frame_stride, P.src_row_stride = src_row_stride;
    P.dst = dst_dev, P.dst_frame_stride = dst_frame_stride, P.dst_row_stride = dst_row_stride;
    P.width = g->width, P.height = g->height, P.channels = g->channels, P.swap_rb = g->color_order == SVGPU_COLOR_BGR;
    P.map = g->d_map, P.map_pitch = g->map_pitch, P.batch = batch;
    {
        SvProfScope prof(ctx, s, "k_ingest_gray");
        sv_launch_ingest_gray(s, P);
    }
    SV_HIP(ctx, hipGetLastError());
    return SVGPU_OK;
}

int svgpu_ingest_gray(svgpu_ctx* ctx, const svgpu_ingest* g, const uint8_t* src, int src_stride, uint8_t* dst, int dst_stride) {
    if (!ctx || !g || !src || !dst || g->device != ctx->device || (long long)src_stride < (long long)g->width * g->channels || dst_stride < g->width)
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_ingest_gray: bad arguments");
    SV_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t src_pitch = pad16((size_t)g->width * g->channels), dst_pitch = pad16((size_t)g->width);
    const size_t src_bytes = src_pitch * g->height, dst_bytes = dst_pitch * g->height;
    int rc;
    if ((rc = sv_ensure_scratch(ctx, src_bytes + dst_bytes))) return rc;
    uint8_t* d_src = (uint8_t*)ctx->d_scratch;
    uint8_t* d_dst = d_src + src_bytes;
    SV_HIP(ctx, hipMemcpy2DAsync(d_src, src_pitch, src, (size_t)src_stride, (size_t)g->width * g->channels, g->height, hipMemcpyHostToDevice, s));
    if ((rc = svgpu_ingest_gray_batch_device(ctx, g, d_src, 1, src_bytes, (int)src_pitch, d_dst, dst_bytes, (int)dst_pitch, s))) return rc;
    SV_HIP(ctx, hipMemcpy2DAsync(dst, (size_t)dst_stride, d_dst, dst_pitch, (size_t)g->width, g->height, hipMemcpyDeviceToHost, s));
    SV_HIP(ctx, hipStreamSynchronize(s));
    return SVGPU_OK;
}

int svgpu_ingest_depth_device(svgpu_ctx* ctx, const void* src_dev, int src_type, int src_stride, int width, int height, double depthmap_factor, float* dst_dev,
                              int dst_stride, void* stream) {
    if (!ctx || !depth_args_ok(src_dev, src_type, src_stride, width, height, depthmap_factor, dst_dev, dst_stride))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_ingest_depth_device: bad arguments");
    SV_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    {
        SvProfScope prof(ctx, s, "k_ingest_depth");
        sv_launch_ingest_depth(s, src_dev, src_type == SVGPU_DEPTH_U16, src_stride, width, height, (float)(1.0 / depthmap_factor), dst_dev, dst_stride);
    }
    SV_HIP(ctx, hipGetLastError());
    return SVGPU_OK;
}

int svgpu_ingest_depth(svgpu_ctx* ctx, const void* src, int src_type, int src_stride, int width, int height, double depthmap_factor, float* dst, int dst_stride) {
    if (!ctx || !depth_args_ok(src, src_type, src_stride, width, height, depthmap_factor, dst, dst_stride))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_ingest_depth: bad arguments");
    SV_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t es = src_type == SVGPU_DEPTH_U16 ? 2 : 4;
    const size_t src_pitch = pad16((size_t)width * es), dst_pitch = pad16((size_t)width * 4);
    int rc;
    if ((rc = sv_ensure_scratch(ctx, (src_pitch + dst_pitch) * height))) return rc;
    char* d_src = (char*)ctx->d_scratch;
    float* d_dst = (float*)(d_src + src_pitch * height);
    SV_HIP(ctx, hipMemcpy2DAsync(d_src, src_pitch, src, (size_t)src_stride, (size_t)width * es, height, hipMemcpyHostToDevice, s));
    if ((rc = svgpu_ingest_depth_device(ctx, d_src, src_type, (int)src_pitch, width, height, depthmap_factor, d_dst, (int)dst_pitch, s))) return rc;
    SV_HIP(ctx, hipMemcpy2DAsync(dst, (size_t)dst_stride, d_dst, dst_pitch, (size_t)width * 4, height, hipMemcpyDeviceToHost, s));
    SV_HIP(ctx, hipStreamSynchronize(s));
    return SVGPU_OK;
}

}  // extern "C"
