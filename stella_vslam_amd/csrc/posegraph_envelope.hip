// Direct solve of the pose graph's damped system (H + lambda I) dx = b: block envelope ("skyline") Cholesky with 7x7 blocks on the device,
// the per-call alternative to k_pg_precond + k_pg_solve (posegraph_kernels.hip).  The free vertices of a spanning chain with windowed
// covisibility and a few loop connections are block-banded once ordered (posegraph_envelope_plan.h picks the order on the host), so the
// lower envelope holds the whole fill and a solve costs one pass over the columns instead of one PCG iteration per unknown.
//
//   k_pg_env_assemble       every envelope block is written once: zero, a diagonal block Hd + lambda I, or the sum over its pair's edges
//                           in list order of Ji^T Jj read directly or transposed (PG_REC_HIJ of k_pg_linearize's record); b in plan order
//   k_pg_env_factor_solve   ONE workgroup walks the block columns (right-looking LL^T, the structure of k_sky_factor_solve in
//                           ba_skyline.hip): pivot L_jj = chol(D_jj) on the first wave (rows on lanes) together with z_j = L_jj^-1 y_j,
//                           column L_ij = S_ij L_jj^-T and y_i -= L_ij z_j (the forward substitution rides along), update
//                           S_ik -= L_ij L_kj^T over the pairs of rows of the column; then the backward substitution over the same
//                           column lists and the scatter of the solution to slot order (the x that k_pg_update reads).
// The index arrays and the right-hand side stay in global memory (L2): at 2 000+ columns they fit no LDS.  A column of up to PG_ENV_MAXM
// rows is staged in LDS for its update; a taller one (a hub) is read back from the envelope, where the column step has already put it.
// fp64 without contraction, no atomics, every sum in a fixed order: a solve is bit-reproducible.  A pivot that is not positive and finite
// marks the trial as a failed solve (PgEnvCtl), the solution is then zero and k_pg_decide rejects the trial.
#include <algorithm>

#include "posegraph_kernels.h"

namespace {

#define PG_ENV_T 256
#define PG_ENV_MAXM 32   // rows of one column staged in LDS (32 x 392 B = 12.25 KB)
#define PG_ENV_PARTS 32  // partial sums per component of a backward-substitution step

__global__ __launch_bounds__(256) void k_pg_env_assemble(PgEnvDev K) {
    if (K.ctl->phase != 1) return;
    const double lambda = K.damped ? K.ctl->lambda : 0.0;
    const size_t total = (size_t)K.nblocks * 49, stride = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t t = t0; t < total; t += stride) {
        const int blk = (int)(t / 49), e = (int)(t - (size_t)blk * 49), r = e / 7, c = e - 7 * r;
        const int src = K.blk_src[blk];
        double v = 0.0;
        if (src >= K.nP) {
            const int k = src - K.nP, flag = K.pair_flag[k];
            for (int q = K.pair_off[k]; q < K.pair_off[k + 1]; ++q) {
                const int ent = K.pair_ent[q];
                const double* B = K.blk + (size_t)(ent >> 1) * K.blk_stride;
                v += ((ent & 1) ^ flag) ? B[7 * c + r] : B[7 * r + c];
            }
        }
        else if (src >= 0) {
            v = K.Hd[(size_t)K.order[src] * 49 + e];
            if (r == c) v += lambda;
        }
        K.val[t] = v;
    }
    for (size_t t = t0; t < (size_t)K.nP * 7; t += stride) {
        const int p = (int)(t / 7), c = (int)(t - (size_t)p * 7);
        K.y[t] = K.b[(size_t)K.order[p] * 7 + c];
    }
}

// x in [0, m (m + 1) / 2) -> (p, q) with q <= p < m, row-major over the lower triangle
__device__ __forceinline__ void pg_tri_index(int x, int& p, int& q) {
    p = (int)((sqrtf(8.0f * (float)x + 1.0f) - 1.0f) * 0.5f);
    while ((p + 1) * (p + 2) / 2 <= x) ++p;
    while (p * (p + 1) / 2 > x) --p;
    q = x - p * (p + 1) / 2;
}
__device__ __forceinline__ double pg_lane_bcast(double v, int src) {  // v of lane `src` (a constant) as a wave-uniform value
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)u, src), hi = __builtin_amdgcn_readlane((int)(unsigned)(u >> 32), src);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// The 7x7 pivot of column j on the first wave: lane r < 7 holds row r of the block (the lanes behind mirror row 6 and write nothing).
// L = chol(block) goes back to the block (upper triangle zeroed), L^-1 (lower triangular, column c on lane c) to dinv and s_Li, and
// z = L^-1 y_j, by forward substitution on the wave-uniform factor, to y_j and s_z.
__device__ __forceinline__ void pg_env_pivot(double* blk, double* dinv, double* s_Li, double* yj, double* s_z, int* s_fail, int lane) {
    const int r = min(lane, 6);
    double a[7], Lm[7][7], rd[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) a[c] = blk[r * 7 + c];
    bool bad = false;
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        double v = a[c];
#pragma unroll
        for (int k = 0; k < 7; ++k)
            if (k < c) v -= a[k] * Lm[c][k];  // a[k] = L[r][k] by now
        const double dcc = pg_lane_bcast(v, c);
        bad = bad || !(dcc > 0.0 && dcc <= 1.7976931348623157e308);
        const double rs = rsqrt(dcc);
        rd[c] = rs;
        a[c] = v * rs;  // L[r][c]; on lane c: dcc / sqrt(dcc)
#pragma unroll
        for (int rr = 0; rr < 7; ++rr)
            if (rr >= c) Lm[rr][c] = pg_lane_bcast(a[c], rr);
    }
    if (bad) {
        if (lane == 0) *s_fail = 1;
        return;
    }
    // column cc of L^-1 on lane cc: x_cc = 1 / L_cc,cc, x_rr = -(sum_{k = cc}^{rr - 1} L_rr,k x_k) / L_rr,rr
    double x[7];
#pragma unroll
    for (int rr = 0; rr < 7; ++rr) {
        double v = rr == r ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k)
            if (k < rr) v -= (k >= r ? Lm[rr][k] : 0.0) * x[k];
        x[rr] = rr >= r ? v * rd[rr] : 0.0;
    }
    // z = L^-1 y_j (every lane the same values)
    double z[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        double v = yj[c];
#pragma unroll
        for (int k = 0; k < 7; ++k)
            if (k < c) v -= Lm[c][k] * z[k];
        z[c] = v * rd[c];
    }
    if (lane < 7) {
#pragma unroll
        for (int c = 0; c < 7; ++c) blk[lane * 7 + c] = c <= lane ? a[c] : 0.0;
#pragma unroll
        for (int rr = 0; rr < 7; ++rr) {
            s_Li[rr * 7 + lane] = x[rr];
            dinv[rr * 7 + lane] = x[rr];
        }
        const double zl = lane == 0 ? z[0] : lane == 1 ? z[1] : lane == 2 ? z[2] : lane == 3 ? z[3] : lane == 4 ? z[4] : lane == 5 ? z[5] : z[6];
        s_z[lane] = zl;
        yj[lane] = zl;
    }
}

__global__ __launch_bounds__(PG_ENV_T) void k_pg_env_factor_solve(PgEnvDev K) {
    if (K.ctl->phase != 1) return;
    __shared__ double s_col[PG_ENV_MAXM * 49];
    __shared__ double s_Li[49];
    __shared__ double s_z[7];
    __shared__ double s_part[PG_ENV_PARTS][7];
    __shared__ int s_fail;
    const int tid = threadIdx.x, nP = K.nP;
    if (tid == 0) s_fail = 0;
    __syncthreads();
    // ---------------------------------------------------------------- factorisation and forward substitution
    for (int j = 0; j < nP; ++j) {
        const int c0 = K.coloff[j], m = K.coloff[j + 1] - c0;
        const int32_t* rows = K.colrows + c0;
        const int32_t* base = K.colbase + c0;
        if (tid < 64) pg_env_pivot(K.val + (size_t)(K.rowoff[j + 1] - 1) * 49, K.dinv + (size_t)j * 49, s_Li, K.y + (size_t)j * 7, s_z, &s_fail, tid);
        __syncthreads();
        if (s_fail) break;
        const bool staged = m <= PG_ENV_MAXM;
        // column: one thread per (row of the column, row a of its block): L_ij[a][b] = sum_{c <= b} S_ij[a][c] Li[b][c], then y_i[a] -= L_ij[a] . z_j
        for (int t = tid; t < m * 7; t += PG_ENV_T) {
            const int r = t / 7, a = t - 7 * r;
            double* Bl = K.val + (size_t)(base[r] + j) * 49 + a * 7;
            double s[7], o[7];
#pragma unroll
            for (int c = 0; c < 7; ++c) s[c] = Bl[c];
#pragma unroll
            for (int b = 0; b < 7; ++b) {
                double v = 0.0;
#pragma unroll
                for (int c = 0; c < 7; ++c)
                    if (c <= b) v += s[c] * s_Li[b * 7 + c];
                o[b] = v;
            }
            double u = o[0] * s_z[0];
#pragma unroll
            for (int c = 1; c < 7; ++c) u += o[c] * s_z[c];
#pragma unroll
            for (int b = 0; b < 7; ++b) Bl[b] = o[b];
            if (staged) {
#pragma unroll
                for (int b = 0; b < 7; ++b) s_col[t * 7 + b] = o[b];  // (r * 49 + a * 7 + b)
            }
            K.y[(size_t)rows[r] * 7 + a] -= u;
        }
        __syncthreads();
        // update: one thread per (pair of rows p >= q of the column, row a of the block): S_{ip, iq}[a] -= L_p[a] L_q^T
        const int nitem = m * (m + 1) / 2 * 7;
        for (int t = tid; t < nitem; t += PG_ENV_T) {
            const int x = t / 7, a = t - 7 * x;
            int p, q;
            pg_tri_index(x, p, q);
            double la[7], d[7];
            double* Dst = K.val + (size_t)(base[p] + rows[q]) * 49 + a * 7;
            if (staged) {
#pragma unroll
                for (int c = 0; c < 7; ++c) la[c] = s_col[p * 49 + a * 7 + c];
#pragma unroll
                for (int b = 0; b < 7; ++b) {
                    double v = la[0] * s_col[q * 49 + b * 7];
#pragma unroll
                    for (int c = 1; c < 7; ++c) v += la[c] * s_col[q * 49 + b * 7 + c];
                    d[b] = v;
                }
            }
            else {
                const double* Lp = K.val + (size_t)(base[p] + j) * 49 + a * 7;
                const double* Lq = K.val + (size_t)(base[q] + j) * 49;
#pragma unroll
                for (int c = 0; c < 7; ++c) la[c] = Lp[c];
#pragma unroll
                for (int b = 0; b < 7; ++b) {
                    double v = la[0] * Lq[b * 7];
#pragma unroll
                    for (int c = 1; c < 7; ++c) v += la[c] * Lq[b * 7 + c];
                    d[b] = v;
                }
            }
#pragma unroll
            for (int b = 0; b < 7; ++b) Dst[b] -= d[b];
        }
        __syncthreads();
    }
    if (s_fail) {
        if (tid == 0) K.env->solve_failed = 1;
        for (int t = tid; t < nP * 7; t += PG_ENV_T) K.x[t] = 0.0;
        return;
    }
    // ---------------------------------------------------------------- L^T x = z: x_j = L_jj^-T (z_j - sum_{i in rows(j)} L_ij^T x_i)
    for (int j = nP - 1; j >= 0; --j) {
        const int c0 = K.coloff[j], m = K.coloff[j + 1] - c0;
        const int32_t* rows = K.colrows + c0;
        const int32_t* base = K.colbase + c0;
        if (tid < 7 * PG_ENV_PARTS) {  // (part, component a): the part's rows in ascending order
            const int part = tid / 7, a = tid - 7 * part;
            double v = 0.0;
            for (int r = part; r < m; r += PG_ENV_PARTS) {
                const double* Bl = K.val + (size_t)(base[r] + j) * 49;
                const double* xi = K.y + (size_t)rows[r] * 7;
#pragma unroll
                for (int c = 0; c < 7; ++c) v += Bl[c * 7 + a] * xi[c];
            }
            s_part[part][a] = v;
        }
        __syncthreads();
        if (tid < 64) {
            const int a = min(tid, 6), np = min(m, PG_ENV_PARTS);
            double tot = 0.0;
            for (int p = 0; p < np; ++p) tot += s_part[p][a];
            const double w = K.y[(size_t)j * 7 + a] - tot;
            const double* Li = K.dinv + (size_t)j * 49;
            double x = 0.0;
#pragma unroll
            for (int c = 0; c < 7; ++c) {
                const double wc = pg_lane_bcast(w, c);
                x += (c >= a ? Li[c * 7 + a] : 0.0) * wc;
            }
            if (tid < 7) K.y[(size_t)j * 7 + tid] = x;
        }
        __syncthreads();
    }
    for (int t = tid; t < nP * 7; t += PG_ENV_T) {
        const int p = t / 7, c = t - 7 * p;
        K.x[(size_t)K.order[p] * 7 + c] = K.y[t];
    }
    if (tid == 0) K.env->solve_failed = 0;
}

}  // namespace

void sv_pg_env_assemble(hipStream_t s, const PgEnvDev& K) {
    if (K.nP <= 0) return;
    const size_t items = (size_t)K.nblocks * 49;
    const int blocks = (int)std::min<size_t>((items + 255) / 256, 2048);
    hipLaunchKernelGGL(k_pg_env_assemble, dim3(blocks), dim3(256), 0, s, K);
}
void sv_pg_env_factor_solve(hipStream_t s, const PgEnvDev& K) {
    if (K.nP > 0) hipLaunchKernelGGL(k_pg_env_factor_solve, dim3(1), dim3(PG_ENV_T), 0, s, K);
}
