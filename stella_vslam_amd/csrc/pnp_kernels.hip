// EPnP + RANSAC of solve::pnp_solver (solve/pnp_solver.cc) on the device.  One wavefront (a workgroup of 64 threads) owns one
// correspondence set or one RANSAC hypothesis.  fp64 throughout, compiled without contraction, every expression in the reference's
// operation order where that order is defined.
//   * Per-point sums (centroid, PW0^T PW0, M^T M, pc0, CM, the errors): lane l takes points l, l + 64, ... in ascending order and the 64
//     partial sums are added by an xor butterfly -- a fixed tree, the same in every lane, no atomics.
//   * The small matrices live in LDS.  Eigen's JacobiSVD is replaced by the project's own Jacobi iterations (precedent:
//     triangulate_kernels.hip): a cyclic two-sided Jacobi for the symmetric PW0^T PW0 (3 x 3) and M^T M (12 x 12), a one-sided (Hestenes)
//     Jacobi on the columns of the general CC, CM (3 x 3) and L_6xk (k = 3, 4, 5).  Lane r updates row r of the two rotated columns; the
//     rotation itself is computed redundantly by every lane from broadcast LDS reads.
//   * What is wave-uniform and small (control points, CC_inv, betas, the 6 x 4 Householder QR of gauss_newton) is computed redundantly in
//     every lane, in registers, with compile-time indices only.
// Signs and order of singular vectors are those of the Jacobi, not Eigen's: the pose does not depend on them where it is unique.
#include "pnp_kernels.h"

namespace {

constexpr double kEps = 2.220446049250313e-16;
constexpr double kDblMax = 1.7976931348623157e308;
constexpr double kDblMin = 2.2250738585072014e-308;
constexpr int kSymSweeps = 40;   // a 12 x 12 converges in 6 to 9 sweeps; the early-out ends the loop
constexpr int kColSweeps = 30;

struct PnpShared {
    double A[144];   // symmetric matrix being diagonalised, row-major, leading dimension 12
    double V[144];   // its eigenvectors, V[r * 12 + c] = component r of vector c
    double d[12];    // eigenvalues
    double T[40];    // reduced sums of M^T M: pair (i <= j) at (j (j + 1) / 2 + i) * 4
    double Un[48];   // Un[j * 12 + r] = U(r, 11 - j), the four singular vectors EPnP uses
    double L[60];    // L_6x10, row-major
    double B[30];    // general matrix of the one-sided Jacobi, column c at B + 6 c
    double W[25];    // its right singular vectors, column c at W + 5 c
    double s2[5];    // squared singular values (squared norms of the rotated columns)
    int order[12];   // indices by descending value
};

// one correspondence set: point i is entry (idx ? idx[i] : i) of bearings / pos_w, both already offset to the set's range
struct PnpSet {
    const double* brg;
    const double* pw;
    const uint32_t* idx;
    int n;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }
__device__ __forceinline__ void load3(const double* p, int g, double& x, double& y, double& z) {
    x = p[3 * (size_t)g], y = p[3 * (size_t)g + 1], z = p[3 * (size_t)g + 2];
}
__device__ __forceinline__ int point_of(const PnpSet& S, int i) { return S.idx ? (int)S.idx[i] : i; }

// order[k] = index of the k-th largest of d[0 .. n); equal values keep their index order
__device__ inline void sort_desc(const double* d, int* order, int n, int lane) {
    if (lane < n) order[lane] = lane;
    __syncthreads();
    if (lane < n) {
        const double dj = d[lane];
        int rank = 0;
        for (int i = 0; i < n; ++i) {
            const double di = d[i];
            rank += (di > dj || (di == dj && i < lane)) ? 1 : 0;
        }
        order[rank] = lane;
    }
    __syncthreads();
}

// cyclic Jacobi of the symmetric n x n matrix in S.A (n <= 12): eigenvalues to S.d, eigenvectors to the columns of S.V
__device__ inline void jacobi_sym(PnpShared& S, int n, int lane) {
    double* A = S.A;
    double* V = S.V;
    for (int t = lane; t < 144; t += 64) V[t] = (t / 12 == t % 12) ? 1.0 : 0.0;
    __syncthreads();
#pragma unroll 1
    for (int sweep = 0; sweep < kSymSweeps; ++sweep) {
        bool rotated = false;
#pragma unroll 1
        for (int p = 0; p < n - 1; ++p) {
#pragma unroll 1
            for (int q = p + 1; q < n; ++q) {
                const double app = A[p * 12 + p], aqq = A[q * 12 + q], apq = A[p * 12 + q];
                if (apq != 0.0 && fabs(apq) > kEps * sqrt(fabs(app * aqq))) {  // (wave-uniform)
                    rotated = true;
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(1.0 + theta * theta));
                    const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                    double akp = 0.0, akq = 0.0, vkp = 0.0, vkq = 0.0;
                    if (lane < n) akp = A[lane * 12 + p], akq = A[lane * 12 + q], vkp = V[lane * 12 + p], vkq = V[lane * 12 + q];
                    __syncthreads();
                    if (lane < n) {
                        V[lane * 12 + p] = cs * vkp - sn * vkq;
                        V[lane * 12 + q] = sn * vkp + cs * vkq;
                        if (lane == p) {
                            A[p * 12 + p] = app - t * apq;
                            A[p * 12 + q] = 0.0;
                        }
                        else if (lane == q) {
                            A[q * 12 + q] = aqq + t * apq;
                            A[q * 12 + p] = 0.0;
                        }
                        else {
                            const double np_ = cs * akp - sn * akq, nq_ = sn * akp + cs * akq;
                            A[lane * 12 + p] = np_;
                            A[p * 12 + lane] = np_;
                            A[lane * 12 + q] = nq_;
                            A[q * 12 + lane] = nq_;
                        }
                    }
                    __syncthreads();
                }
            }
        }
        if (!rotated) break;
    }
    if (lane < n) S.d[lane] = A[lane * 12 + lane];
    __syncthreads();
}

// one-sided Jacobi on the k columns (m rows, k <= m <= 6) of S.B: on return the columns are U S, S.W holds V, S.s2 the squared singular
// values and S.order their descending order
__device__ inline void jacobi_cols(PnpShared& S, int m, int k, int lane) {
    double* B = S.B;
    double* W = S.W;
    if (lane < 25) W[lane] = (lane / 5 == lane % 5) ? 1.0 : 0.0;
    __syncthreads();
#pragma unroll 1
    for (int sweep = 0; sweep < kColSweeps; ++sweep) {
        bool rotated = false;
#pragma unroll 1
        for (int p = 0; p < k - 1; ++p) {
#pragma unroll 1
            for (int q = p + 1; q < k; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int r = 0; r < m; ++r) {
                    const double bp = B[6 * p + r], bq = B[6 * q + r];
                    alpha += bp * bp;
                    beta += bq * bq;
                    gamma += bp * bq;
                }
                if (gamma != 0.0 && fabs(gamma) > kEps * sqrt(alpha * beta)) {  // (wave-uniform)
                    rotated = true;
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                    double bp = 0.0, bq = 0.0, wp = 0.0, wq = 0.0;
                    if (lane < m) bp = B[6 * p + lane], bq = B[6 * q + lane];
                    if (lane < k) wp = W[5 * p + lane], wq = W[5 * q + lane];
                    __syncthreads();
                    if (lane < m) {
                        B[6 * p + lane] = cs * bp - sn * bq;
                        B[6 * q + lane] = sn * bp + cs * bq;
                    }
                    if (lane < k) {
                        W[5 * p + lane] = cs * wp - sn * wq;
                        W[5 * q + lane] = sn * wp + cs * wq;
                    }
                    __syncthreads();
                }
            }
        }
        if (!rotated) break;
    }
    if (lane < k) {
        double s = 0.0;
        for (int r = 0; r < m; ++r) s += B[6 * lane + r] * B[6 * lane + r];
        S.s2[lane] = s;
    }
    __syncthreads();
    sort_desc(S.s2, S.order, k, lane);
}

// JacobiSVD::solve(Rho) of the 6 x k matrix in S.B (find_initial_betas_N): x = V S^-1 U^T rho over the singular values Eigen's rank rule
// keeps (SVDBase::rank: s_j >= max(s_0 * k * epsilon, DBL_MIN))
__device__ inline void svd_solve(PnpShared& S, int k, const double (&rho)[6], double (&x)[5], int lane) {
    jacobi_cols(S, 6, k, lane);
    const double s0 = sqrt(S.s2[S.order[0]]);
    const double keep = fmax(s0 * ((double)k * kEps), kDblMin);
#pragma unroll
    for (int c = 0; c < 5; ++c) x[c] = 0.0;
    for (int j = 0; j < k; ++j) {
        const int o = S.order[j];
        const double s = sqrt(S.s2[o]);
        if (s < keep) continue;
        const double* b = S.B + 6 * o;
        double ut = 0.0;  // U(:, j)^T rho, U(:, j) = b / s
#pragma unroll
        for (int r = 0; r < 6; ++r) ut += (b[r] / s) * rho[r];
        const double c_ = ut / s;
#pragma unroll
        for (int c = 0; c < 5; ++c)
            if (c < k) x[c] += S.W[5 * o + c] * c_;
    }
    __syncthreads();
}

// pnp_solver::gauss_newton (:566-579): betas += A.householderQr().solve(b), A and b of compute_A_and_b_for_gauss_newton (:550-564).
// Householder QR as Eigen's unblocked kernel forms it (makeHouseholderInPlace / applyHouseholderOnTheLeft), b carried as a fifth column.
__device__ inline void gauss_newton(const PnpShared& S, const double (&rho)[6], double (&bt)[4], int num_iter) {
#pragma unroll 1
    for (int it = 0; it < num_iter; ++it) {
        double a[6][5];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const double* l = S.L + 10 * i;
            const double l0 = l[0], l1 = l[1], l2 = l[2], l3 = l[3], l4 = l[4], l5 = l[5], l6 = l[6], l7 = l[7], l8 = l[8], l9 = l[9];
            a[i][0] = ((2 * l0 * bt[0] + l1 * bt[1]) + l3 * bt[2]) + l6 * bt[3];
            a[i][1] = ((l1 * bt[0] + 2 * l2 * bt[1]) + l4 * bt[2]) + l7 * bt[3];
            a[i][2] = ((l3 * bt[0] + l4 * bt[1]) + 2 * l5 * bt[2]) + l8 * bt[3];
            a[i][3] = ((l6 * bt[0] + l7 * bt[1]) + l8 * bt[2]) + 2 * l9 * bt[3];
            a[i][4] = rho[i]
                      - (((((((((l0 * bt[0] * bt[0] + l1 * bt[0] * bt[1]) + l2 * bt[1] * bt[1]) + l3 * bt[0] * bt[2]) + l4 * bt[1] * bt[2]) + l5 * bt[2] * bt[2])
                            + l6 * bt[0] * bt[3])
                           + l7 * bt[1] * bt[3])
                          + l8 * bt[2] * bt[3])
                         + l9 * bt[3] * bt[3]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double tail = 0.0;
#pragma unroll
            for (int r = k + 1; r < 6; ++r) tail += a[r][k] * a[r][k];
            const double c0 = a[k][k];
            double tau = 0.0, beta = c0;
            if (!(tail <= kDblMin)) {
                beta = sqrt(c0 * c0 + tail);
                if (c0 >= 0.0) beta = -beta;
#pragma unroll
                for (int r = k + 1; r < 6; ++r) a[r][k] = a[r][k] / (c0 - beta);
                tau = (beta - c0) / beta;
            }
            else {
#pragma unroll
                for (int r = k + 1; r < 6; ++r) a[r][k] = 0.0;
            }
            a[k][k] = beta;
#pragma unroll
            for (int c = k + 1; c < 5; ++c) {
                double tmp = 0.0;
#pragma unroll
                for (int r = k + 1; r < 6; ++r) tmp += a[r][k] * a[r][c];
                tmp += a[k][c];
                a[k][c] -= tau * tmp;
#pragma unroll
                for (int r = k + 1; r < 6; ++r) a[r][c] -= tau * a[r][k] * tmp;
            }
        }
        // R x = (Q^T b)[0 .. 4), column-oriented back substitution
        double c[4] = {a[0][4], a[1][4], a[2][4], a[3][4]};
#pragma unroll
        for (int i = 3; i >= 0; --i) {
            c[i] = c[i] / a[i][i];
#pragma unroll
            for (int r = 0; r < i; ++r) c[r] -= a[r][i] * c[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) bt[i] += c[i];
    }
}

// pnp_solver::compute_pose (:155-206).  Every lane returns the same pose and error; a pose is NaN when no N gave a comparable error.
__device__ void compute_pose(PnpShared& S, const PnpSet& P, int gn_iter, int lane, double (&pose)[12], double& err_out) {
    const int n = P.n;
    const double dn = (double)(unsigned)n;
    // ---- choose_control_points (:208-238)
    double c0[3];
    {
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int i = lane; i < n; i += 64) {
            double x, y, z;
            load3(P.pw, point_of(P, i), x, y, z);
            sx += x, sy += y, sz += z;
        }
        c0[0] = wave_sum(sx) / dn, c0[1] = wave_sum(sy) / dn, c0[2] = wave_sum(sz) / dn;
    }
    {
        double q[6] = {0, 0, 0, 0, 0, 0};
        for (int i = lane; i < n; i += 64) {
            double x, y, z;
            load3(P.pw, point_of(P, i), x, y, z);
            x -= c0[0], y -= c0[1], z -= c0[2];
            q[0] += x * x, q[1] += x * y, q[2] += x * z, q[3] += y * y, q[4] += y * z, q[5] += z * z;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) q[k] = wave_sum(q[k]);
        __syncthreads();
        if (lane == 0) {
            S.A[0] = q[0], S.A[1] = q[1], S.A[2] = q[2];
            S.A[12] = q[1], S.A[13] = q[3], S.A[14] = q[4];
            S.A[24] = q[2], S.A[25] = q[4], S.A[26] = q[5];
        }
        __syncthreads();
    }
    jacobi_sym(S, 3, lane);
    sort_desc(S.d, S.order, 3, lane);
    double cw[4][3];  // control points
#pragma unroll
    for (int r = 0; r < 3; ++r) cw[0][r] = c0[r];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        const int o = S.order[i - 1];
        const double ev = S.d[o];
        const double k = sqrt((ev < 0.0 ? 0.0 : ev) / dn);  // (a slightly negative eigenvalue of the positive semi-definite matrix is 0)
#pragma unroll
        for (int r = 0; r < 3; ++r) cw[i][r] = c0[r] + k * S.V[r * 12 + o];
    }
    __syncthreads();
    // ---- compute_barycentric_coordinates (:240-275): CC_inv = V S U^T with S(i, i) = D(i) > 1e-6 ? 1 / D(i) : 0
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int r = 0; r < 3; ++r) S.B[6 * i + r] = cw[i + 1][r] - cw[0][r];
    }
    __syncthreads();
    jacobi_cols(S, 3, 3, lane);
    double ci[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) ci[r][c] = 0.0;
    for (int j = 0; j < 3; ++j) {
        const int o = S.order[j];
        const double D = sqrt(S.s2[o]);
        if (D > 1e-6) {
            const double inv = 1 / D;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) ci[r][c] += (S.W[5 * o + r] * inv) * (S.B[6 * o + c] / D);
        }
    }
    __syncthreads();
    const auto alphas = [&](double x, double y, double z, double (&a)[4]) {
        x -= cw[0][0], y -= cw[0][1], z -= cw[0][2];
        a[1] = dot3(ci[0][0], ci[0][1], ci[0][2], x, y, z);
        a[2] = dot3(ci[1][0], ci[1][1], ci[1][2], x, y, z);
        a[3] = dot3(ci[2][0], ci[2][1], ci[2][2], x, y, z);
        a[0] = 1.0 - a[1] - a[2] - a[3];
    };
    // ---- M^T M (compute_M :277-301): block (i, j) is the sum over the points of alpha_i alpha_j [1 0 -u; 0 1 -v; -u -v u^2 + v^2]
    {
        double acc[10][4];
#pragma unroll
        for (int k = 0; k < 10; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[k][e] = 0.0;
        for (int i = lane; i < n; i += 64) {
            const int g = point_of(P, i);
            double x, y, z, bx, by, bz, a[4];
            load3(P.pw, g, x, y, z);
            load3(P.brg, g, bx, by, bz);
            alphas(x, y, z, a);
            const double u = bx / bz, v = by / bz;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int ii = 0; ii <= jj; ++ii) {
                    const int k = jj * (jj + 1) / 2 + ii;
                    const double mu_i = -a[ii] * u, mu_j = -a[jj] * u, mv_i = -a[ii] * v, mv_j = -a[jj] * v;
                    acc[k][0] += a[ii] * a[jj];
                    acc[k][1] += a[ii] * mu_j;
                    acc[k][2] += a[ii] * mv_j;
                    acc[k][3] += mu_i * mu_j + mv_i * mv_j;
                }
        }
#pragma unroll
        for (int k = 0; k < 10; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double s = wave_sum(acc[k][e]);
                if (lane == 0) S.T[4 * k + e] = s;
            }
        __syncthreads();
        for (int t = lane; t < 144; t += 64) {
            const int r = t / 12, c = t % 12;
            const int bi = r / 3, ri = r % 3, bj = c / 3, rj = c % 3;
            const int i = bi < bj ? bi : bj, j = bi < bj ? bj : bi;
            const double* s = S.T + 4 * (j * (j + 1) / 2 + i);
            double v = 0.0;
            if (ri == rj) v = ri == 2 ? s[3] : s[0];
            else if (ri + rj == 2) v = s[1];  // (0, 2), (2, 0)
            else if (ri + rj == 3) v = s[2];  // (1, 2), (2, 1)
            S.A[t] = v;
        }
        __syncthreads();
    }
    jacobi_sym(S, 12, lane);
    sort_desc(S.d, S.order, 12, lane);
    if (lane < 48) S.Un[lane] = S.V[(lane % 12) * 12 + S.order[11 - lane / 12]];
    __syncthreads();
    // ---- compute_L_6x10 (:502-537), compute_rho (:539-548)
    if (lane < 60) {
        const int i = lane / 10, c = lane % 10;
        const int y = c >= 6 ? 3 : c >= 3 ? 2 : c >= 1 ? 1 : 0, x = c - y * (y + 1) / 2;
        const int a = i < 3 ? 0 : i < 5 ? 1 : 2, b = i < 3 ? i + 1 : i < 5 ? i - 1 : 3;
        const double *ux = S.Un + 12 * x, *uy = S.Un + 12 * y;
        const double d = dot3(ux[3 * a] - ux[3 * b], ux[3 * a + 1] - ux[3 * b + 1], ux[3 * a + 2] - ux[3 * b + 2], uy[3 * a] - uy[3 * b],
                              uy[3 * a + 1] - uy[3 * b + 1], uy[3 * a + 2] - uy[3 * b + 2]);
        S.L[lane] = x == y ? d : 2.0 * d;
    }
    double rho[6];
    {
        int k = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = a + 1; b < 4; ++b, ++k) {
                const double x = cw[a][0] - cw[b][0], y = cw[a][1] - cw[b][1], z = cw[a][2] - cw[b][2];
                rho[k] = (x * x + y * y) + z * z;
            }
    }
    __syncthreads();
    // bearing of the first correspondence: the side of the camera the points have to be on
    double b0x, b0y, b0z, p0x, p0y, p0z, a0[4];
    load3(P.brg, point_of(P, 0), b0x, b0y, b0z);
    load3(P.pw, point_of(P, 0), p0x, p0y, p0z);
    alphas(p0x, p0y, p0z, a0);
    const bool bearing_z_sign = b0z > 0;
    double best = kDblMax;
#pragma unroll
    for (int e = 0; e < 12; ++e) pose[e] = __builtin_nan("");
#pragma unroll 1
    for (int N = 2; N <= 4; ++N) {
        // ---- find_initial_betas_N (:386-500)
        const int k = N == 2 ? 3 : N == 3 ? 5 : 4;
        if (lane < 6 * k) {
            const int c = lane / 6, r = lane % 6;
            const int src = N == 4 ? (c == 2 ? 3 : c == 3 ? 6 : c) : c;
            S.B[lane] = S.L[10 * r + src];
        }
        __syncthreads();
        double x[5], bt[4];
        svd_solve(S, k, rho, x, lane);
        if (N == 4) {
            if (x[0] < 0) {
                bt[0] = sqrt(-x[0]);
                bt[1] = -x[1] / bt[0], bt[2] = -x[2] / bt[0], bt[3] = -x[3] / bt[0];
            }
            else {
                bt[0] = sqrt(x[0]);
                bt[1] = x[1] / bt[0], bt[2] = x[2] / bt[0], bt[3] = x[3] / bt[0];
            }
        }
        else {
            if (x[0] < 0) {
                bt[0] = sqrt(-x[0]);
                bt[1] = (x[2] < 0) ? sqrt(-x[2]) : 0.0;
            }
            else {
                bt[0] = sqrt(x[0]);
                bt[1] = (x[2] > 0) ? sqrt(x[2]) : 0.0;
            }
            if (x[1] < 0) bt[0] = -bt[0];
            bt[2] = N == 3 ? x[3] / bt[0] : 0.0;
            bt[3] = 0.0;
        }
        gauss_newton(S, rho, bt, gn_iter);
        // ---- compute_ccs (:303-316), compute_pcs with the z-sign flip (:318-334)
        double cc[4][3];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < 4; ++j) s += bt[j] * S.Un[12 * j + 3 * i + r];
                cc[i][r] = s;
            }
        const auto pc_of = [&](const double (&a)[4], int r) { return ((a[0] * cc[0][r] + a[1] * cc[1][r]) + a[2] * cc[2][r]) + a[3] * cc[3][r]; };
        const bool flip = (pc_of(a0, 2) > 0) != bearing_z_sign;
        // ---- estimate_R_and_t (:350-384); pw0 is the centroid of choose_control_points (the same sum)
        double pc0[3];
        {
            double sx = 0.0, sy = 0.0, sz = 0.0;
            for (int i = lane; i < n; i += 64) {
                double px, py, pz, a[4];
                load3(P.pw, point_of(P, i), px, py, pz);
                alphas(px, py, pz, a);
                double cx = pc_of(a, 0), cy = pc_of(a, 1), cz = pc_of(a, 2);
                if (flip) cx *= -1, cy *= -1, cz *= -1;
                sx += cx, sy += cy, sz += cz;
            }
            pc0[0] = wave_sum(sx) / dn, pc0[1] = wave_sum(sy) / dn, pc0[2] = wave_sum(sz) / dn;
        }
        {
            double cm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int i = lane; i < n; i += 64) {
                double px, py, pz, a[4];
                load3(P.pw, point_of(P, i), px, py, pz);
                alphas(px, py, pz, a);
                double cx = pc_of(a, 0), cy = pc_of(a, 1), cz = pc_of(a, 2);
                if (flip) cx *= -1, cy *= -1, cz *= -1;
                cx -= pc0[0], cy -= pc0[1], cz -= pc0[2];
                px -= c0[0], py -= c0[1], pz -= c0[2];
                cm[0] += cx * px, cm[1] += cx * py, cm[2] += cx * pz;
                cm[3] += cy * px, cm[4] += cy * py, cm[5] += cy * pz;
                cm[6] += cz * px, cm[7] += cz * py, cm[8] += cz * pz;
            }
#pragma unroll
            for (int e = 0; e < 9; ++e) {
                const double s = wave_sum(cm[e]);
                if (lane == 0) S.B[6 * (e % 3) + e / 3] = s;  // CM(r, c), column-major
            }
            __syncthreads();
        }
        jacobi_cols(S, 3, 3, lane);
        double rot[9], tr[3];
        {
            // U: the two leading left singular vectors, the third their cross product (its sign is what the det < 0 repair settles; a
            // coplanar set has a zero third singular value and no direction of its own there)
            const int o0 = S.order[0], o1 = S.order[1], o2 = S.order[2];
            const double s0 = sqrt(S.s2[o0]), s1 = sqrt(S.s2[o1]);
            double u[3][3], w[3][3];  // u[j][r] = U(r, j), w[j][r] = V(r, j)
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                u[0][r] = S.B[6 * o0 + r] / s0, u[1][r] = S.B[6 * o1 + r] / s1;
                w[0][r] = S.W[5 * o0 + r], w[1][r] = S.W[5 * o1 + r], w[2][r] = S.W[5 * o2 + r];
            }
            u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
            u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
            u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) rot[3 * r + c] = (u[0][r] * w[0][c] + u[1][r] * w[1][c]) + u[2][r] * w[2][c];
            const double det = (rot[0] * (rot[4] * rot[8] - rot[5] * rot[7]) - rot[1] * (rot[3] * rot[8] - rot[5] * rot[6]))
                               + rot[2] * (rot[3] * rot[7] - rot[4] * rot[6]);
            if (det < 0) {
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) rot[3 * r + c] = (u[0][r] * w[0][c] + u[1][r] * w[1][c]) + (-u[2][r]) * w[2][c];
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) tr[r] = pc0[r] - dot3(rot[3 * r], rot[3 * r + 1], rot[3 * r + 2], c0[0], c0[1], c0[2]);
        }
        __syncthreads();
        // ---- reprojection_error (:336-348)
        double es = 0.0;
        for (int i = lane; i < n; i += 64) {
            const int g = point_of(P, i);
            double px, py, pz, bx, by, bz;
            load3(P.pw, g, px, py, pz);
            load3(P.brg, g, bx, by, bz);
            const double X = dot3(rot[0], rot[1], rot[2], px, py, pz) + tr[0];
            const double Y = dot3(rot[3], rot[4], rot[5], px, py, pz) + tr[1];
            const double Z = dot3(rot[6], rot[7], rot[8], px, py, pz) + tr[2];
            const double cos_angle = dot3(X, Y, Z, bx, by, bz) / sqrt((X * X + Y * Y) + Z * Z);
            es += 1.0 - cos_angle;
        }
        const double err = wave_sum(es) / dn;
        if (err < best) {
            best = err;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                pose[4 * r] = rot[3 * r], pose[4 * r + 1] = rot[3 * r + 1], pose[4 * r + 2] = rot[3 * r + 2];
                pose[4 * r + 3] = tr[r];
            }
        }
    }
    err_out = best;
}

__global__ __launch_bounds__(64) void k_pnp_pose(const PnpPoseProblem P) {
    __shared__ PnpShared S;
    const int lane = threadIdx.x;
    const int s = P.sets ? P.sets[blockIdx.x] : (int)blockIdx.x;
    if (P.enable && !P.enable[s]) return;
    const int first = P.off[s];
    const int n = P.count ? P.count[s] : P.off[s + 1] - first;
    if (n < 1) return;
    const PnpSet set{P.bearings + 3 * (size_t)first, P.pos_w + 3 * (size_t)first, P.idx ? P.idx + first : nullptr, n};
    double pose[12], err;
    compute_pose(S, set, P.gn_iter, lane, pose, err);
    // (:123: a recompute for which no N gave a comparable error leaves best_rot_cw_ / best_trans_cw_ at the winning hypothesis)
    if (P.keep_on_failure && !(err < kDblMax)) return;
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 12; ++e) P.pose[12 * (size_t)s + e] = pose[e];
        if (P.err) P.err[s] = err;
    }
}

__global__ __launch_bounds__(64) void k_pnp_ransac(const PnpRansacProblem P) {
    __shared__ PnpShared S;
    const int lane = threadIdx.x;
    const int a = blockIdx.x / P.num_iter, it = blockIdx.x % P.num_iter;
    if (a >= P.num_active) return;
    const int p = P.active[a];
    const int first = P.match_off[p], n = P.match_off[p + 1] - first;
    const size_t h = (size_t)p * P.num_iter + it;
    const double* brg = P.bearings + 3 * (size_t)first;
    const double* pw = P.pos_w + 3 * (size_t)first;
    // 2-1, 2-2: the minimum set and its pose.  A pose without a comparable error is NaN here (the reference keeps the previous
    // iteration's pose, which can never win the strict selection again): no match is an inlier of it.
    const PnpSet set{brg, pw, P.samples + 4 * h, 4};
    double pose[12], err;
    compute_pose(S, set, P.gn_iter, lane, pose, err);
    // 2-3: check_inliers (:126-153)
    const float* mce = P.max_cos + first;
    uint8_t* flags = P.hyp_inlier + (size_t)P.num_iter * first + (size_t)it * n;
    double cost = 0.0;
    int num = 0;
    for (int i = lane; i < n; i += 64) {
        double px, py, pz, bx, by, bz;
        load3(pw, i, px, py, pz);
        load3(brg, i, bx, by, bz);
        const double X = dot3(pose[0], pose[1], pose[2], px, py, pz) + pose[3];
        const double Y = dot3(pose[4], pose[5], pose[6], px, py, pz) + pose[7];
        const double Z = dot3(pose[8], pose[9], pose[10], px, py, pz) + pose[11];
        const double cos_angle = dot3(X, Y, Z, bx, by, bz) / sqrt((X * X + Y * Y) + Z * Z);
        const float m = mce[i];
        const bool in = (double)m < cos_angle;
        if (in) cost += 1 - cos_angle, ++num;
        else cost += (double)(1 - m);  // (`1 - max_cos_errors_.at(i)` is a float expression)
        flags[i] = in ? 1 : 0;
    }
    cost = wave_sum(cost);
    num = wave_sum(num);
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 12; ++e) P.hyp_pose[12 * h + e] = pose[e];
        P.hyp_num_inliers[h] = num;
        P.hyp_cost[h] = cost;
    }
}

__global__ __launch_bounds__(64) void k_pnp_select(const PnpRansacProblem P) {
    const int p = P.active[blockIdx.x], lane = threadIdx.x;
    const int first = P.match_off[p], n = P.match_off[p + 1] - first;
    double min_cost = kDblMax;
    int best = -1;
    for (int it = 0; it < P.num_iter; ++it) {  // (wave-uniform walk, in iteration order; a NaN cost fails `min_cost > cost`)
        const size_t h = (size_t)p * P.num_iter + it;
        const unsigned num = (unsigned)P.hyp_num_inliers[h];
        const double cost = P.hyp_cost[h];
        if (num > P.min_num_inliers && min_cost > cost) min_cost = cost, best = it;
    }
    const bool valid = min_cost < kDblMax;
    if (!valid) best = -1;
    const uint8_t* flags = best >= 0 ? P.hyp_inlier + (size_t)P.num_iter * first + (size_t)best * n : nullptr;
    int count = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool in = i < n && flags && flags[i];
        if (i < n) P.is_inlier[first + i] = in ? 1 : 0;
        if (P.recompute) {
            const unsigned long long mask = __ballot(in);
            if (in) P.inl_idx[first + count + __popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)i;
            count += __popcll(mask);
        }
    }
    if (lane < 12) P.pose[12 * (size_t)p + lane] = best >= 0 ? P.hyp_pose[12 * ((size_t)p * P.num_iter + best) + lane] : 0.0;
    if (lane == 0) {
        P.valid[p] = valid ? 1 : 0;
        P.best_iter[p] = best;
        if (P.recompute) P.inl_count[p] = count;
    }
}

}  // namespace

void sv_launch_pnp_pose(hipStream_t s, const PnpPoseProblem& P) {
    const int blocks = P.sets ? P.num_launch : P.num_sets;
    if (blocks > 0) hipLaunchKernelGGL(k_pnp_pose, dim3(blocks), dim3(64), 0, s, P);
}
void sv_launch_pnp_ransac(hipStream_t s, const PnpRansacProblem& P) {
    if (P.num_active > 0 && P.num_iter > 0) hipLaunchKernelGGL(k_pnp_ransac, dim3((unsigned)P.num_active * (unsigned)P.num_iter), dim3(64), 0, s, P);
}
void sv_launch_pnp_select(hipStream_t s, const PnpRansacProblem& P) {
    if (P.num_active > 0) hipLaunchKernelGGL(k_pnp_select, dim3(P.num_active), dim3(64), 0, s, P);
}
