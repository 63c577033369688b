// Pairwise Sim3 optimisation: optimize::transform_optimizer::optimize (optimize/transform_optimizer.cc:20-158) on the device.
//
// k_sim3_opt is ONE persistent workgroup per problem (grid = loop candidates), after the model of k_pose_opt (ba_kernels.hip): the problem
// is a single 7-dof vertex with two unary edges per match, i.e. a chain of dependent fp64 steps that is launch-latency-bound if cut into
// kernels.  Both stages, both chi2 gates, every 7x7 solve (thread 0) and the early return run inside the launch.
//   per evaluation point   lanes 0..14 write the estimate and its 14 perturbed neighbours exp(+-1e-9 e_c) * estimate, and their inverses,
//                          to LDS; they are uniform over the workgroup
//   per edge               a lane takes edge e = 2 * match + side, e ascending with stride S3O_THREADS: 15 projections give the error and
//                          g2o's numeric Jacobian, then the lane's share of the 28 + 7 + 1 sums of H, b and the robust chi2
//   sums                   lane-strided ascending partials, a transpose through LDS and a fixed tree per wavefront, the wavefronts in
//                          ascending order: no atomics, the result does not depend on scheduling
// fp64 without contraction; the Levenberg-Marquardt rules are those of k_pg_decide (posegraph_kernels.hip) minus terminate_action, the
// Huber weighting that of k_pose_opt.
#include "sim3opt_kernels.h"
#include "sv_sim3.h"

namespace {

constexpr double S3O_DELTA = 1e-9;
constexpr int S3O_WAVES = S3O_THREADS / 64;
constexpr int S3O_HALF = 18;   // sums per transposition round
constexpr int S3O_PITCH = 65;  // doubles per row of the transposition buffer: lanes reading different rows hit different banks

__device__ __forceinline__ void s3o_huber(double e, double delta, double* rho0, double* rho1) {  // g2o RobustKernelHuber, as ba_kernels.hip
    const double dsqr = delta * delta;
    if (e <= dsqr) {
        *rho0 = e;
        *rho1 = 1.0;
    }
    else {
        const double sqrte = sqrt(e);
        *rho0 = 2 * sqrte * delta - dsqr;
        *rho1 = delta / sqrte;
    }
}

// one edge: the point in the OTHER keyframe's camera, the observation, its information and the camera it is projected with
struct S3oEdge {
    SvVec3 p;
    double ox, oy, w;
    const double* k;  // LDS
    bool eq;
};

// obs - project(S.map(p)); S is 8 doubles in LDS, the same for every lane
__device__ __forceinline__ void s3o_error(const S3oEdge& E, const double* S, double& ex, double& ey) {
    const SvVec3 q = sv_sim3_map(sv_sim3_load(S), E.p);
    double u, v;
    if (E.eq) {  // forward_reproj_edge.h:110-114
        constexpr double PI = 3.14159265358979323846;
        const double theta = atan2(q.x, q.z);
        const double phi = -asin(q.y / sqrt(q.x * q.x + q.y * q.y + q.z * q.z));
        u = E.k[0] * (0.5 + theta / (2 * PI));
        v = E.k[1] * (0.5 - phi / PI);
    }
    else {       // :92-94
        u = E.k[0] * q.x / q.z + E.k[2];
        v = E.k[1] * q.y / q.z + E.k[3];
    }
    ex = E.ox - u;
    ey = E.oy - v;
}

// Everything the workgroup shares.  One object at namespace scope, so that the phases below, which are functions of their own, address it
// as LDS without taking it as an argument.
struct S3oShared {
    double w[S3O_WAVES][S3O_HALF][S3O_PITCH];  // transposition buffer of the sums; before them, a lane's Jacobian (14 x S3O_THREADS)
    double part[S3O_WAVES][36];
    double red[36];  // H upper triangle (28), b (7), robust chi2
    double p[S3O_WAVES];
    double pose[2][12], k[2][4];
    double X[14][8];     // exp(+-delta e_c): the same for every linearisation
    double est[8];       // the estimate
    double S[2][15][8];  // [forward | inverse][estimate, then + and - per coordinate]
    double T[2][8];      // the trial estimate and its inverse
    double x[7];
    int ok2;
    // the problem's slices of the call's arrays, its edge count and camera kinds
    const double *obs1, *obs2, *pos1, *pos2;
    const float *w1, *w2;
    uint8_t* status;
    double* chi_cache;
    int ne, eq1, eq2, fix_scale;
    double delta;  // Huber width
};
static_assert(14 * S3O_THREADS <= S3O_WAVES * S3O_HALF * S3O_PITCH, "the Jacobian columns do not fit the transposition buffer");
__shared__ S3oShared sh;

// edge e of the problem: match e >> 1; side 0 is the forward edge (keyframe 2's landmark into keyframe 1's camera, through S12),
// side 1 the backward edge (keyframe 1's landmark into keyframe 2's camera, through S12^-1)
__device__ __forceinline__ S3oEdge s3o_load_edge(int e) {
    const int side = e & 1;
    const size_t m = (size_t)(e >> 1);
    const double* X = (side ? sh.pos1 : sh.pos2) + 3 * m;
    const double* T = sh.pose[side ? 0 : 1];
    const double* o = (side ? sh.obs2 : sh.obs1) + 2 * m;
    S3oEdge E;
    E.p = sv3(T[0] * X[0] + T[1] * X[1] + T[2] * X[2] + T[3], T[4] * X[0] + T[5] * X[1] + T[6] * X[2] + T[7],
              T[8] * X[0] + T[9] * X[1] + T[10] * X[2] + T[11]);
    E.ox = o[0], E.oy = o[1];
    E.w = (double)(side ? sh.w2 : sh.w1)[m];
    E.k = sh.k[side];
    E.eq = (side ? sh.eq2 : sh.eq1) != 0;
    return E;
}

// sum of one value per thread, fixed order, the total in every thread
__device__ __forceinline__ double s3o_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();  // sh.p may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) sh.p[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < S3O_WAVES; ++w) t += sh.p[w];
    return t;
}

// the 36 sums of a linearisation: per wavefront a transpose through LDS (18 values a round), lane k adding row k in four interleaved
// ascending chains that a fixed tree joins; then the wavefronts' partials in ascending order
__device__ __forceinline__ void s3o_reduce36(const double (&acc)[36]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int k = 0; k < S3O_HALF; ++k) sh.w[wave][k][lane] = acc[S3O_HALF * half + k];
        __syncthreads();
        if (lane < S3O_HALF) {
            const double* r = sh.w[wave][lane];
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
            for (int j = 0; j < 64; j += 4) {
                a0 += r[j];
                a1 += r[j + 1];
                a2 += r[j + 2];
                a3 += r[j + 3];
            }
            sh.part[wave][S3O_HALF * half + lane] = (a0 + a1) + (a2 + a3);
        }
        __syncthreads();
    }
    if (threadIdx.x < 36) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < S3O_WAVES; ++w) t += sh.part[w][threadIdx.x];
        sh.red[threadIdx.x] = t;
    }
    __syncthreads();
}

// (H + lambda I) x = b for the 7x7 system, H given by its 28 upper-triangle sums (row-major: (a, c >= a) at a * 7 - a (a - 1) / 2 + c - a).
// Unrolled as po_chol6 (ba_kernels.hip): every index is a compile-time constant, the factor lives in registers, divisions stay divisions.
__device__ __forceinline__ bool s3o_chol7(const double* Hu, double lambda, const double* b, double* x) {
    double A[49];
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int lo = i < j ? i : j, hi = i < j ? j : i;
            A[7 * i + j] = Hu[lo * 7 - lo * (lo - 1) / 2 + (hi - lo)];
        }
#pragma unroll
    for (int i = 0; i < 7; ++i) A[8 * i] += lambda;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        double d = A[8 * j];
#pragma unroll
        for (int k = 0; k < 7; ++k)
            if (k < j) d -= A[7 * j + k] * A[7 * j + k];
        ok = ok && d > 0.0;
        d = sqrt(d);
        A[8 * j] = d;
#pragma unroll
        for (int i = 0; i < 7; ++i)
            if (i > j) {
                double sum = A[7 * i + j];
#pragma unroll
                for (int k = 0; k < 7; ++k)
                    if (k < j) sum -= A[7 * i + k] * A[7 * j + k];
                A[7 * i + j] = sum / d;
            }
    }
    if (!ok) return false;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        double sum = b[i];
#pragma unroll
        for (int k = 0; k < 7; ++k)
            if (k < i) sum -= A[7 * i + k] * x[k];
        x[i] = sum / A[8 * i];
    }
#pragma unroll
    for (int i = 6; i >= 0; --i) {
        double sum = x[i];
#pragma unroll
        for (int k = 0; k < 7; ++k)
            if (k > i) sum -= A[7 * k + i] * x[k];
        x[i] = sum / A[8 * i];
    }
    return true;
}

// ---- The phases of an LM iteration, each a function that takes its inputs from `sh` and leaves its results there.  This file is built
// with machine-level loop-invariant code motion off (csrc/Makefile): with it on, the 64-bit coefficients of atan2 / asin / sin / cos / exp
// / pow, which are SGPR pairs, and the poses and camera parameters were hoisted out of the whole loop nest and stayed live through the
// kernel: 39 SGPR spills and 82 AGPRs of overflow.

// the 15 evaluation points: the estimate and exp(+-delta e_c) * estimate, and their inverses
__device__ __forceinline__ void s3o_phase_points() {
    const int tid = threadIdx.x;
    if (tid < 15) {
        const SvSim3 est = sv_sim3_load(sh.est);
        const SvSim3 F = tid == 0 ? est : sv_sim3_mul(sv_sim3_load(sh.X[tid - 1]), est);
        sv_sim3_store(sh.S[0][tid], F);
        sv_sim3_store(sh.S[1][tid], sv_sim3_inv(F));
    }
    __syncthreads();
}

// linearise at the 15 points: H (28 unique), b (7) and the robust chi2 into sh.red
__device__ __forceinline__ void s3o_phase_linearise() {
    const int tid = threadIdx.x;
    constexpr double scalar = 1.0 / (2.0 * S3O_DELTA);
    double* const s_J = &sh.w[0][0][0];
    double acc[36];
#pragma unroll
    for (int k = 0; k < 36; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (int e = tid; e < sh.ne; e += S3O_THREADS) {
        if (sh.status[e >> 1] != SVGPU_SIM3OPT_INLIER) continue;
        const S3oEdge E = s3o_load_edge(e);
        const double(*S)[8] = sh.S[e & 1];
        double ex, ey, J0[7], J1[7];
        s3o_error(E, S[0], ex, ey);
        // the Jacobian one coordinate at a time through a column of LDS that belongs to this lane: the loop stays rolled, so two of the
        // 15 Sim3s are in registers at a time and not all of them
#pragma unroll 1
        for (int c = 0; c < 7; ++c) {
            double ax, ay, bx, by;
            s3o_error(E, S[1 + 2 * c], ax, ay);
            s3o_error(E, S[2 + 2 * c], bx, by);
            s_J[(2 * c) * S3O_THREADS + tid] = scalar * (ax - bx);
            s_J[(2 * c + 1) * S3O_THREADS + tid] = scalar * (ay - by);
        }
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            J0[c] = s_J[(2 * c) * S3O_THREADS + tid];
            J1[c] = s_J[(2 * c + 1) * S3O_THREADS + tid];
        }
        const double chi = (ex * ex + ey * ey) * E.w;
        double rho0, rho1;
        s3o_huber(chi, sh.delta, &rho0, &rho1);
        const double w = E.w * rho1;
        int k = 0;
#pragma unroll
        for (int a = 0; a < 7; ++a)
#pragma unroll
            for (int c = a; c < 7; ++c) {
                acc[k] += J0[a] * w * J0[c] + J1[a] * w * J1[c];
                ++k;
            }
#pragma unroll
        for (int a = 0; a < 7; ++a) acc[28 + a] += J0[a] * (-w * ex) + J1[a] * (-w * ey);
        acc[35] += rho0;
    }
    __syncthreads();  // every lane is done with its Jacobian column: the buffer goes to the sums
    s3o_reduce36(acc);
}

// one damping trial's solve, on thread 0: (H + lambda I) x = b, the trial estimate exp(x) * estimate and its inverse
__device__ __forceinline__ void s3o_phase_solve(double lambda) {
    if (threadIdx.x == 0) {
        double x[7] = {0, 0, 0, 0, 0, 0, 0};
        const bool ok2 = s3o_chol7(sh.red, lambda, sh.red + 28, x);
        if (!ok2)
#pragma unroll
            for (int a = 0; a < 7; ++a) x[a] = 0.0;
#pragma unroll
        for (int a = 0; a < 7; ++a) sh.x[a] = x[a];
        SvVec7 u = SvVec7{x[0], x[1], x[2], x[3], x[4], x[5], x[6]};
        if (sh.fix_scale) u.sg = 0.0;  // transform_vertex::oplusImpl
        const SvSim3 T = sv_sim3_mul(sv_sim3_exp(u), sv_sim3_load(sh.est));
        sv_sim3_store(sh.T[0], T);
        sv_sim3_store(sh.T[1], sv_sim3_inv(T));
        sh.ok2 = ok2 ? 1 : 0;
    }
    __syncthreads();
}

// the trial: every active edge's error is cached (g2o's _error), accepted or not; returns the robust chi2 at the trial estimate
__device__ __forceinline__ double s3o_phase_trial() {
    double tmp = 0.0;
#pragma unroll 1
    for (int e = threadIdx.x; e < sh.ne; e += S3O_THREADS) {
        if (sh.status[e >> 1] != SVGPU_SIM3OPT_INLIER) continue;
        const S3oEdge E = s3o_load_edge(e);
        double ex, ey;
        s3o_error(E, sh.T[e & 1], ex, ey);
        const double chi = (ex * ex + ey * ey) * E.w;
        sh.chi_cache[e] = chi;
        double rho0, rho1;
        s3o_huber(chi, sh.delta, &rho0, &rho1);
        tmp += rho0;
    }
    return s3o_sum(tmp);
}

// exp(+-delta e_c), once per launch
__device__ __forceinline__ void s3o_phase_perturbations() {
    const int tid = threadIdx.x;
    if (tid < 14) {
        const int c = tid >> 1;
        double d = (tid & 1) ? -S3O_DELTA : S3O_DELTA;
        if (sh.fix_scale && c == 6) d = 0.0;  // transform_vertex::oplusImpl
        sv_sim3_store(sh.X[tid], sv_sim3_exp(sv_sim3_unit_update(c, d)));
    }
}

__global__ __launch_bounds__(S3O_THREADS) void k_sim3_opt(Sim3OptDev D) {
    const int tid = threadIdx.x;
    const Sim3OptProblem& Q = D.prob[blockIdx.x];
    const int lo = Q.m_lo, n = Q.m_hi - lo;
    if (tid < 12) sh.pose[0][tid] = Q.view[0].pose[tid], sh.pose[1][tid] = Q.view[1].pose[tid];
    if (tid < 4) sh.k[0][tid] = Q.view[0].k[tid], sh.k[1][tid] = Q.view[1].k[tid];
    if (tid < 8) sh.est[tid] = Q.sim3[tid];
    if (tid == 0) {
        sh.obs1 = D.obs1 + 2 * (size_t)lo, sh.obs2 = D.obs2 + 2 * (size_t)lo;
        sh.pos1 = D.pos1 + 3 * (size_t)lo, sh.pos2 = D.pos2 + 3 * (size_t)lo;
        sh.w1 = D.w1 + lo, sh.w2 = D.w2 + lo;
        sh.status = D.status + lo;
        sh.chi_cache = D.chi_cache + 2 * (size_t)lo;
        sh.ne = 2 * n, sh.eq1 = Q.view[0].equirect, sh.eq2 = Q.view[1].equirect, sh.fix_scale = D.fix_scale;
        sh.delta = (double)sqrtf(D.chi_sq);
    }
    for (int i = tid; i < n; i += S3O_THREADS) D.status[lo + i] = SVGPU_SIM3OPT_INLIER;
    __syncthreads();
    s3o_phase_perturbations();
    __syncthreads();

    const double chi_sq = (double)D.chi_sq;
    // per-stage figures as named scalars (an array indexed by the stage would live in scratch memory)
    int iters1 = 0, iters2 = 0, trials1 = 0, trials2 = 0, early = 0, survivors = 0, inliers = 0;
    double first1 = 0.0, first2 = 0.0, last1 = 0.0, last2 = 0.0;
    double lambda = 0.0, ni = 2.0;
#pragma unroll 1
    for (int stage = 0; stage < 2; ++stage) {
        const int iters = stage == 0 ? 5 : D.num_iter;
        bool ok = true;
        int it = 0;
#pragma unroll 1
        for (; it < iters && ok && n > 0; ++it) {
            s3o_phase_points();
            s3o_phase_linearise();
            double cur = sh.red[35];
            if (it == 0) {  // computeLambdaInit: the damping restarts with every optimize()
                double md = 0.0;
#pragma unroll
                for (int a = 0; a < 7; ++a) md = fmax(md, fabs(sh.red[a * 7 - a * (a - 1) / 2]));
                lambda = 1e-5 * md;
                ni = 2.0;
                if (stage == 0) first1 = cur;
                else first2 = cur;
            }
            double rho = 0.0;
            int qmax = 0;
            do {
                s3o_phase_solve(lambda);
                double temp_chi = s3o_phase_trial();
                if (!sh.ok2) temp_chi = 1.7976931348623157e308;
                double scale = 0.0;
#pragma unroll
                for (int a = 0; a < 7; ++a) scale += sh.x[a] * (lambda * sh.x[a] + sh.red[28 + a]);
                scale += 1e-3;
                rho = (cur - temp_chi) / scale;
                if (stage == 0) ++trials1;
                else ++trials2;
                __syncthreads();  // sh.x, sh.ok2 and sh.T have been read by everyone
                if (rho > 0 && isfinite(temp_chi)) {
                    double alpha = 1. - pow((2 * rho - 1), 3);
                    alpha = fmin(alpha, 2. / 3.);
                    lambda *= fmax(1. / 3., alpha);
                    ni = 2.0;
                    cur = temp_chi;
                    if (tid < 8) sh.est[tid] = sh.T[0][tid];  // accept: the trial state becomes the estimate
                    __syncthreads();
                }
                else {
                    lambda *= ni;
                    ni *= 2.0;
                    if (!isfinite(lambda)) break;
                }
                ++qmax;
            } while (rho < 0 && qmax < 10);
            if (qmax == 10 || rho == 0 || !isfinite(lambda)) ok = false;
            if (stage == 0) last1 = cur;
            else last2 = cur;
        }
        if (stage == 0) iters1 = it;
        else iters2 = it;
        // ---- the gate on the cached chi2 (transform_optimizer.cc:104-119, :133-151)
        __syncthreads();
        double cnt = 0.0;
        for (int i = tid; i < n; i += S3O_THREADS) {
            if (D.status[lo + i] != SVGPU_SIM3OPT_INLIER) continue;
            const double c12 = D.chi_cache[2 * ((size_t)lo + i)], c21 = D.chi_cache[2 * ((size_t)lo + i) + 1];
            const bool out = stage == 0 ? !(c12 < chi_sq && c21 < chi_sq) : (chi_sq < c12 || chi_sq < c21);
            if (out) D.status[lo + i] = stage == 0 ? SVGPU_SIM3OPT_REJECTED_STAGE1 : SVGPU_SIM3OPT_REJECTED_STAGE2;
            else cnt += 1.0;
        }
        const int left = (int)s3o_sum(cnt);
        if (stage == 0) {
            survivors = left;
            if (left < 10) {  // :121-123: the reference returns before it writes the estimate back
                early = 1;
                break;
            }
        }
        else inliers = left;
    }
    if (tid < 8) D.sim3_out[8 * (size_t)blockIdx.x + tid] = early ? Q.sim3[tid] : sh.est[tid];
    if (tid == 0) {
        D.num_inliers[blockIdx.x] = inliers;
        svgpu_sim3opt_stats& st = D.stats[blockIdx.x];
        st.lm_iterations[0] = iters1, st.lm_iterations[1] = iters2;
        st.lm_trials[0] = trials1, st.lm_trials[1] = trials2;
        st.early_return = early;
        st.num_survivors = survivors;
        st.first_chi2[0] = first1, st.first_chi2[1] = first2;
        st.last_chi2[0] = last1, st.last_chi2[1] = last2;
        st.lambda = lambda;
    }
}

}  // namespace

void sv_launch_sim3opt(hipStream_t s, const Sim3OptDev& D) {
    if (D.num_problems > 0) hipLaunchKernelGGL(k_sim3_opt, dim3(D.num_problems), dim3(S3O_THREADS), 0, s, D);
}
