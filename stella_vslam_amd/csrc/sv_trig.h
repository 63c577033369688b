// util::cos / util::sin of the reference (util/trigonometric.h:11-47): a degree-4 polynomial on a folded argument, all in float.  One
// restatement for the device (ORB orientation, orb_kernels.hip) and the host (the cosine thresholds of svgpu_pnp.hip); pinned by
// tests/golden/reference_kats.json.  Compiled without contraction on both sides.
#pragma once
#include <hip/hip_runtime.h>

__host__ __device__ inline float sv_cos_poly(float v) {  // util/trigonometric.h:17-24
    const float c1 = 0.99940307f, c2 = -0.49558072f, c3 = 0.03679168f;
    const float v2 = v * v;
    return c1 + v2 * (c2 + c3 * v2);
}
__host__ __device__ inline float sv_util_cos(float v) {  // util/trigonometric.h:26-42
    constexpr float PI_ = 3.14159265358979f;
    constexpr float PI_2 = PI_ / 2.0f;
    constexpr float TWO_PI = 2.0f * PI_;
    constexpr float INV_TWO_PI = 1.0f / TWO_PI;
    constexpr float THREE_PI_2 = 3.0f * PI_2;
    v = v - (float)(int)floorf(v * INV_TWO_PI) * TWO_PI;
    v = (0.0f < v) ? v : -v;
    if (v < PI_2) return sv_cos_poly(v);
    else if (v < PI_) return -sv_cos_poly(PI_ - v);
    else if (v < THREE_PI_2) return -sv_cos_poly(v - PI_);
    else return sv_cos_poly(TWO_PI - v);
}
__host__ __device__ inline float sv_util_sin(float v) {
    constexpr float PI_2 = 3.14159265358979f / 2.0f;
    return sv_util_cos(PI_2 - v);
}
