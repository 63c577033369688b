// k_triangulate_two_views: module::two_view_triangulator::triangulate (module/two_view_triangulator.cc:19-96) for a list of keypoint
// matches between one keyframe and K neighbours, one lane per match.  fp64 throughout except where the reference computes in `float`;
// every expression keeps the reference's operation order (compiled without contraction).  The one deliberate difference is the null
// vector of solve::triangulator::triangulate (solve/triangulator.h:76-88): Eigen's two-sided JacobiSVD is replaced by a one-sided
// (Hestenes) Jacobi on the four columns of A held in registers -- v[:3] / v[3] does not depend on the sign or scale of v, so the result
// agrees with any accurate SVD up to rounding.  The body of a match is svtri::triangulate_match (triangulate_device.h).
#include "triangulate_kernels.h"

#include "triangulate_device.h"

namespace {

__global__ __launch_bounds__(256) void k_triangulate_two_views(const TriProblem P) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= P.num_matches) return;
    const int k = P.nb_of_match[m];
    const TriView& V1 = P.v1;
    const TriView& V2 = P.nb[k];
    int i1, i2;
    if (P.idx2) i1 = P.idx1[m], i2 = P.idx2[m];
    else i1 = m - P.nb_first[k], i2 = P.idx1[m];  // matched_2_in_1 of this neighbour
    double pwx = 0.0, pwy = 0.0, pwz = 0.0;
    int st = SV_TRI_SKIPPED;
    if (0 <= i2) st = svtri::triangulate_match(V1, V2, i1, i2, P.scale_factors, P.level_sigma_sq, P.cos_rays_parallax_thr, pwx, pwy, pwz);
    P.pos_w[3 * (size_t)m] = pwx;
    P.pos_w[3 * (size_t)m + 1] = pwy;
    P.pos_w[3 * (size_t)m + 2] = pwz;
    P.status[m] = (uint8_t)st;
}

}  // namespace

void sv_launch_triangulate_two_views(hipStream_t s, const TriProblem& P) {
    if (P.num_matches <= 0) return;
    hipLaunchKernelGGL(k_triangulate_two_views, dim3((P.num_matches + 255) / 256), dim3(256), 0, s, P);
}
