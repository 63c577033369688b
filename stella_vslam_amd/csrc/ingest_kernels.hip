// Image ingest: raw frame -> grey level 0 in ONE pass (the rectified colour image is never written), map compilation, true depth.
// The arithmetic is OpenCV's 8-bit fixed point as tests/ingest_problems.py states it.
//   k_ingest_stream   no maps: a pure stream.  A lane takes INGEST_PX = 16 pixels of a row: CH dwordx4 loads, one dwordx4 store.
//   k_ingest_remap    with maps: a lane owns one destination pixel, turns its compiled map entry into tap offsets and weights ONCE and
//                     walks the frames of its batch slice -- per frame it reads source bytes (a gather through L2) and writes one byte,
//                     a wave 64 neighbouring ones.
//   k_ingest_compile_map   float maps -> 8-byte entries, once per ingest.
//   k_ingest_depth    convertTo(CV_32F, 1 / factor): one fp32 product per pixel.
#include "ingest_kernels.h"

namespace {

constexpr uint32_t CR = 9798, CG = 19235, CB = 3735;  // cv::cvtColor 8U: R2Y, G2Y, B2Y at 15 fractional bits

__device__ __forceinline__ uint32_t grey_of(uint32_t r, uint32_t g, uint32_t b) { return (r * CR + g * CG + b * CB + (1u << 14)) >> 15; }

template <bool SWAP>
__device__ __forceinline__ uint32_t grey_px(uint32_t c0, uint32_t c1, uint32_t c2) {
    return SWAP ? grey_of(c2, c1, c0) : grey_of(c0, c1, c2);
}

template <int N>
__device__ __forceinline__ uint32_t byte_of(const uint32_t (&w)[N], int i) {  // i is a constant after unrolling
    return (w[i >> 2] >> ((i & 3) * 8)) & 0xffu;
}

__global__ __launch_bounds__(256) void k_ingest_compile_map(const float* __restrict__ map_x, const float* __restrict__ map_y, int pitch, int width,
                                                            int height, uint2* __restrict__ out, int out_pitch) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= out_pitch) return;
    int ix = -2, iy = -2;
    uint32_t fx = 0, fy = 0;
    if (x < width) {
        const float vx = rintf(map_x[(size_t)y * pitch + x] * 32.0f), vy = rintf(map_y[(size_t)y * pitch + x] * 32.0f);  // half to even
        if (fabsf(vx) < 1073741824.0f && fabsf(vy) < 1073741824.0f) {  // (false for NaN)
            const int sx = (int)vx, sy = (int)vy;
            ix = min(max(sx >> 5, -2), width), iy = min(max(sy >> 5, -2), height);
            fx = (uint32_t)(sx & 31), fy = (uint32_t)(sy & 31);
        }
    }
    out[(size_t)y * out_pitch + x] = make_uint2((uint32_t)(ix + 2) | ((uint32_t)(iy + 2) << 16), fx | (fy << 5));
}

template <int CH, bool SWAP>
__global__ __launch_bounds__(256) void k_ingest_stream(const IngestProblem P, int groups, int vec) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= groups * P.height) return;
    const int y = idx / groups, g = idx - y * groups, x0 = g * INGEST_PX;
    const uint8_t* s = P.src + (size_t)blockIdx.y * P.src_frame_stride + (size_t)y * P.src_row_stride + (size_t)x0 * CH;
    uint8_t* d = P.dst + (size_t)blockIdx.y * P.dst_frame_stride + (size_t)y * P.dst_row_stride + x0;
    if (vec && x0 + INGEST_PX <= P.width) {
        uint32_t w[4 * CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const uint4 v = reinterpret_cast<const uint4*>(s)[c];
            w[4 * c] = v.x, w[4 * c + 1] = v.y, w[4 * c + 2] = v.z, w[4 * c + 3] = v.w;
        }
        uint32_t o[4] = {0, 0, 0, 0};
        if (CH == 1) {
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = w[i];
        } else {
#pragma unroll
            for (int p = 0; p < INGEST_PX; ++p)
                o[p >> 2] |= grey_px<SWAP>(byte_of(w, p * CH), byte_of(w, p * CH + 1), byte_of(w, p * CH + 2)) << ((p & 3) * 8);
        }
        *reinterpret_cast<uint4*>(d) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {  // the last pixels of a row, and buffers that are not 16-byte aligned
        const int n = min(INGEST_PX, P.width - x0);
        for (int p = 0; p < n; ++p) d[p] = CH == 1 ? s[p] : (uint8_t)grey_px<SWAP>(s[p * CH], s[p * CH + 1], s[p * CH + 2]);
    }
}

template <int CH, bool SWAP>
__global__ __launch_bounds__(256) void k_ingest_remap(const IngestProblem P, int frames_per_block) {
    const int W = P.width, H = P.height;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= W * H) return;
    const int y = idx / W, x = idx - y * W;
    const uint2 m = P.map[(size_t)y * P.map_pitch + x];
    const int ix = (int)(m.x & 0xffffu) - 2, iy = (int)(m.x >> 16) - 2;
    const uint32_t fx = m.y & 31u, fy = (m.y >> 5) & 31u;
    // a tap outside the source counts as 0: its weight goes, its address is clamped into the source
    const uint32_t wx0 = (uint32_t)ix < (uint32_t)W ? 32u - fx : 0u, wx1 = (uint32_t)(ix + 1) < (uint32_t)W ? fx : 0u;
    const uint32_t wy0 = (uint32_t)iy < (uint32_t)H ? 32u - fy : 0u, wy1 = (uint32_t)(iy + 1) < (uint32_t)H ? fy : 0u;
    const uint32_t c0 = (uint32_t)min(max(ix, 0), W - 1) * CH, c1 = (uint32_t)min(max(ix + 1, 0), W - 1) * CH;
    const uint32_t r0 = (uint32_t)min(max(iy, 0), H - 1) * (uint32_t)P.src_row_stride, r1 = (uint32_t)min(max(iy + 1, 0), H - 1) * (uint32_t)P.src_row_stride;
    const uint32_t off[4] = {r0 + c0, r0 + c1, r1 + c0, r1 + c1};                  // taps (0,0) (1,0) (0,1) (1,1)
    const uint32_t wt[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};
    const int b0 = blockIdx.y * frames_per_block, b1 = min(b0 + frames_per_block, P.batch);
    constexpr int NC = CH == 1 ? 1 : 3;  // (alpha is never read)
    uint8_t* d = P.dst + (size_t)y * P.dst_row_stride + x;
    for (int b = b0; b < b1; ++b) {
        const uint8_t* s = P.src + (size_t)b * P.src_frame_stride;
        uint32_t c[3] = {0, 0, 0};
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) {
            const uint32_t acc = (wt[0] * s[off[0] + ch] + wt[1] * s[off[1] + ch]) + (wt[2] * s[off[2] + ch] + wt[3] * s[off[3] + ch]);
            c[ch] = (acc + 512u) >> 10;  // = (32 acc + (1 << 14)) >> 15: the weights of the table are these times 32
        }
        d[(size_t)b * P.dst_frame_stride] = (uint8_t)(NC == 1 ? c[0] : grey_px<SWAP>(c[0], c[1], c[2]));
    }
}

template <bool U16>
__global__ __launch_bounds__(256) void k_ingest_depth(const uint8_t* __restrict__ src, int src_stride, int width, float scale, uint8_t* __restrict__ dst,
                                                      int dst_stride) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= width) return;
    const uint8_t* row = src + (size_t)y * src_stride;
    const float v = U16 ? (float)reinterpret_cast<const uint16_t*>(row)[x] : reinterpret_cast<const float*>(row)[x];
    reinterpret_cast<float*>(dst + (size_t)y * dst_stride)[x] = v * scale;
}

inline bool aligned16(const void* p, size_t a, size_t b) { return (((uintptr_t)p | a | b) & 15u) == 0; }

template <int CH, bool SWAP>
void launch_gray(hipStream_t s, const IngestProblem& P) {
    if (!P.map) {
        const int groups = (P.width + INGEST_PX - 1) / INGEST_PX;
        const int vec = aligned16(P.src, P.src_frame_stride, (size_t)P.src_row_stride) && aligned16(P.dst, P.dst_frame_stride, (size_t)P.dst_row_stride);
        const dim3 grid((unsigned)(((size_t)groups * P.height + 255) / 256), (unsigned)P.batch);
        hipLaunchKernelGGL((k_ingest_stream<CH, SWAP>), grid, dim3(256), 0, s, P, groups, vec);
    } else {
        const unsigned bx = (unsigned)(((size_t)P.width * P.height + 255) / 256);
        // a block walks up to 8 frames with its map entries, tap offsets and weights in registers, as long as the grid still fills the device a few times over
        int fpb = 8;
        while (fpb > 1 && (size_t)bx * ((P.batch + fpb - 1) / fpb) < 4096) fpb >>= 1;
        const dim3 grid(bx, (unsigned)((P.batch + fpb - 1) / fpb));
        hipLaunchKernelGGL((k_ingest_remap<CH, SWAP>), grid, dim3(256), 0, s, P, fpb);
    }
}

}  // namespace

void sv_launch_ingest_compile_map(hipStream_t s, const float* map_x, const float* map_y, int pitch_floats, int width, int height, uint2* out, int out_pitch) {
    hipLaunchKernelGGL(k_ingest_compile_map, dim3((unsigned)((out_pitch + 255) / 256), (unsigned)height), dim3(256), 0, s, map_x, map_y, pitch_floats, width, height,
                       out, out_pitch);
}

void sv_launch_ingest_gray(hipStream_t s, const IngestProblem& P) {
    if (P.channels == 1) launch_gray<1, false>(s, P);
    else if (P.channels == 3) P.swap_rb ? launch_gray<3, true>(s, P) : launch_gray<3, false>(s, P);
    else P.swap_rb ? launch_gray<4, true>(s, P) : launch_gray<4, false>(s, P);
}

void sv_launch_ingest_depth(hipStream_t s, const void* src, int is_u16, int src_stride, int width, int height, float scale, float* dst, int dst_stride) {
    const dim3 grid((unsigned)((width + 255) / 256), (unsigned)height);
    if (is_u16) hipLaunchKernelGGL(k_ingest_depth<true>, grid, dim3(256), 0, s, (const uint8_t*)src, src_stride, width, scale, (uint8_t*)dst, dst_stride);
    else hipLaunchKernelGGL(k_ingest_depth<false>, grid, dim3(256), 0, s, (const uint8_t*)src, src_stride, width, scale, (uint8_t*)dst, dst_stride);
}
