// Image ingest kernels (ingest_kernels.hip): colour to grey, rectification, true depth.  Semantics: tests/ingest_problems.py.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// One compiled map entry, 8 bytes:  .x = (ix + 2) | (iy + 2) << 16,  .y = fx | fy << 5
// ix, iy = integer source position of the top-left tap, clamped to [-2, width] / [-2, height] (every clamped value has all its taps on one
// side outside the source, as the unclamped one had); fx, fy = the 5-bit fractions.  Non-finite and huge entries compile to (-2, -2).
#define INGEST_PX 16  // pixels of one lane of the streaming kernel

struct IngestProblem {
    const uint8_t* src;
    size_t src_frame_stride;
    int src_row_stride;
    uint8_t* dst;
    size_t dst_frame_stride;
    int dst_row_stride;
    int width, height, channels;
    int swap_rb;        // BGR(A): the first byte of a pixel is blue
    const uint2* map;   // compiled map (null: no rectification)
    int map_pitch;      // entries per row of it
    int batch;
};

void sv_launch_ingest_compile_map(hipStream_t s, const float* map_x, const float* map_y, int pitch_floats, int width, int height, uint2* out, int out_pitch);
void sv_launch_ingest_gray(hipStream_t s, const IngestProblem& P);
// dst[y][x] = (float)src[y][x] * scale;  is_u16: CV_16U source, else CV_32F;  strides in bytes
void sv_launch_ingest_depth(hipStream_t s, const void* src, int is_u16, int src_stride, int width, int height, float scale, float* dst, int dst_stride);
