// Pose-graph optimisation kernels: optimize::graph_optimizer::optimize (optimize/graph_optimizer.cc:26-303) on the device.
//
// A vertex is a Sim3 (sv_sim3.h), an edge the error log(C * v1 * v2^-1) with identity information and g2o's numeric Jacobian (central
// differences, delta 1e-9, through the vertex's own oplus = exp(update) * estimate).  Everything is fp64 without contraction, sums run in
// a fixed order and there are no atomics: a call's result does not depend on scheduling.
//
//   k_pg_linearize   one lane per error evaluation (1 + 28 per edge, two edges per wavefront) -> per-edge record
//   k_pg_assemble    one wavefront per free vertex: diagonal block and right-hand side over its edges in ascending edge order
//   k_pg_prepare     chi2 of the estimate, lambda0 = 1e-5 max diag H on the first iteration
//   k_pg_precond     inverse of every damped diagonal block (block-Jacobi preconditioner)
//   k_pg_solve       PCG of (H + lambda I) dx = b in ONE workgroup: off-diagonal blocks stay per edge
//                    (or, per call, the direct solver of posegraph_envelope.hip in place of k_pg_precond and k_pg_solve)
//   k_pg_update      trial estimate exp(dx) * estimate, the vertex's share of dx^T (lambda dx + b)
//   k_pg_chi2        error of every edge at the trial estimate
//   k_pg_decide      rho test, damping update, terminate_action: the rules of k_ba_decide (ba_kernels.hip)
//   k_pg_output      Sim3 and [R | t / s] of the final estimate
// The host enqueues steps of these nine launches; each kernel looks at PgCtl::phase and returns when it has nothing to do.
#include "posegraph_kernels.h"
#include "sv_sim3.h"

namespace {

constexpr double PG_DELTA = 1e-9;

// graph_opt_edge::computeError
__device__ SvVec7 pg_error(const SvSim3& C, const SvSim3& v1, const SvSim3& v2) { return sv_sim3_log(sv_sim3_mul(sv_sim3_mul(C, v1), sv_sim3_inv(v2))); }

__device__ double pg_chi(const SvVec7& e) { return e.w0 * e.w0 + e.w1 * e.w1 + e.w2 * e.w2 + e.u0 * e.u0 + e.u1 * e.u1 + e.u2 * e.u2 + e.sg * e.sg; }

// sum over the workgroup in a fixed order: lane-strided partial, wavefront tree, then the wavefronts' partials in ascending order
template <int NW>
__device__ double pg_block_sum(double v, double* sw) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();  // sw may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) t += sw[w];
    return t;
}

// ---------------------------------------------------------------------------------------------------------------- linearisation
__global__ __launch_bounds__(64) void k_pg_linearize(PgDev D) {
    if (D.ctl->phase != 0) return;
    __shared__ double s_e[2][29][7];
    __shared__ double s_J[2][7][15];  // columns 0..6 vertex i, 7..13 vertex j, 14 the error
    const int lane = threadIdx.x, q = lane & 31, eh = lane >> 5;
    const int e = 2 * blockIdx.x + eh;
    const bool live = e < D.E;
    const int ee = live ? e : 0;
    const int vi = D.e_i[ee], vj = D.e_j[ee];
    const bool fix_i = D.fixed[vi] != 0, fix_j = D.fixed[vj] != 0;
    const double* est = D.est[D.ctl->cur & 1];
    if (live && q < 29) {
        SvSim3 Si = sv_sim3_load(est + (size_t)vi * 8), Sj = sv_sim3_load(est + (size_t)vj * 8);
        const SvSim3 C = sv_sim3_load(D.meas + (size_t)ee * 8);
        bool run = true;
        if (q > 0) {
            const int c = (q - 1) >> 1, side = c >= 7, coord = side ? c - 7 : c;
            run = side ? !fix_j : !fix_i;
            double d = ((q - 1) & 1) ? -PG_DELTA : PG_DELTA;
            if (D.fix_scale && coord == 6) d = 0.0;  // shot_vertex::oplusImpl
            if (run) {
                const SvSim3 X = sv_sim3_exp(sv_sim3_unit_update(coord, d));
                if (side) Sj = sv_sim3_mul(X, Sj);
                else Si = sv_sim3_mul(X, Si);
            }
        }
        SvVec7 err = SvVec7{0, 0, 0, 0, 0, 0, 0};
        if (run) err = pg_error(C, Si, Sj);
        double* o = s_e[eh][q];
        o[0] = err.w0, o[1] = err.w1, o[2] = err.w2, o[3] = err.u0, o[4] = err.u1, o[5] = err.u2, o[6] = err.sg;
    }
    __syncthreads();
    if (live) {
        constexpr double scalar = 1.0 / (2.0 * PG_DELTA);
        for (int k = q; k < 7 * 15; k += 32) {
            const int r = k / 15, c = k % 15;
            double v;
            if (c == 14) v = s_e[eh][0][r];
            else if (c < 7 ? fix_i : fix_j) v = 0.0;  // a fixed vertex gets no Jacobian
            else v = scalar * (s_e[eh][1 + 2 * c][r] - s_e[eh][2 + 2 * c][r]);
            s_J[eh][r][c] = v;
        }
    }
    __syncthreads();
    if (!live) return;
    double* rec = D.rec + (size_t)e * PG_REC;
    for (int o = q; o < PG_REC; o += 32) {
        int ca, cb;
        double sign = 1.0;
        if (o < PG_REC_BI) {
            const int blk = o / 49, rem = o % 49;
            ca = (blk == 2 ? 7 : 0) + rem / 7;
            cb = (blk == 0 ? 0 : 7) + rem % 7;
        }
        else if (o < PG_REC_CHI) {
            ca = o - PG_REC_BI;
            cb = 14;
            sign = -1.0;
        }
        else ca = cb = 14;
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < 7; ++r) acc += s_J[eh][r][ca] * s_J[eh][r][cb];
        rec[o] = sign * acc;
    }
}

// ---------------------------------------------------------------------------------------------------------------- assembly
__global__ __launch_bounds__(64) void k_pg_assemble(PgDev D) {
    if (D.ctl->phase != 0) return;
    __shared__ double s_d[64];
    const int slot = blockIdx.x, lane = threadIdx.x;
    if (slot >= D.nfree) return;
    const int lo = D.v_off[slot], hi = D.v_off[slot + 1];
    double acc = 0.0;
    if (lane < 56) {
        for (int k = lo; k < hi; ++k) {
            const int ent = D.v_ent[k], e = ent >> 1, side = ent & 1;
            const double* rec = D.rec + (size_t)e * PG_REC;
            acc += lane < 49 ? rec[(side ? PG_REC_HJJ : 0) + lane] : rec[(side ? PG_REC_BJ : PG_REC_BI) + (lane - 49)];
        }
        if (lane < 49) D.Hd[(size_t)slot * 49 + lane] = acc;
        else D.b[(size_t)slot * 7 + (lane - 49)] = acc;
    }
    s_d[lane] = acc;
    __syncthreads();
    if (lane == 0) {
        double m = 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) m = fmax(fabs(s_d[8 * k]), m);
        D.maxd[slot] = m;
    }
}

// ---------------------------------------------------------------------------------------------------------------- start of an iteration
__global__ __launch_bounds__(256) void k_pg_prepare(PgDev D) {
    __shared__ double sw[4];
    const int phase = D.ctl->phase, it = D.ctl->it;
    if (phase != 0) return;
    double c = 0.0;
    for (int e = threadIdx.x; e < D.E; e += 256) c += D.rec[(size_t)e * PG_REC + PG_REC_CHI];
    const double chi = pg_block_sum<4>(c, sw);
    double m = 0.0;
    if (it == 0) {
        for (int v = threadIdx.x; v < D.nfree; v += 256) m = fmax(D.maxd[v], m);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_down(m, o, 64));
        __syncthreads();
        if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = m;
        __syncthreads();
        m = fmax(fmax(sw[0], sw[1]), fmax(sw[2], sw[3]));
    }
    if (threadIdx.x != 0) return;
    PgCtl& k = *D.ctl;
    k.current_chi = chi;
    k.temp_chi = chi;
    if (it == 0) {
        k.chi_begin = chi;
        k.lambda = 1e-5 * m;
        k.ni = 2.0;
    }
    k.qmax = 0;
    k.rho = 0.0;
    if (D.env) D.env->failed_in_iteration = 0;
    k.phase = (it < k.it_max && D.nfree > 0) ? 1 : 2;
}

// ---------------------------------------------------------------------------------------------------------------- preconditioner
// inverse of the symmetric positive definite 7x7 block Hd + lambda I by Gauss-Jordan elimination without pivoting, in registers
__global__ __launch_bounds__(64) void k_pg_precond(PgDev D) {
    if (D.ctl->phase != 1) return;
    const int slot = blockIdx.x * 64 + threadIdx.x;
    if (slot >= D.nfree) return;
    const double lambda = D.ctl->lambda;
    double a[49], inv[49];
#pragma unroll
    for (int k = 0; k < 49; ++k) {
        a[k] = D.Hd[(size_t)slot * 49 + k];
        inv[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        a[8 * k] += lambda;
        inv[8 * k] = 1.0;
    }
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        const double piv = 1.0 / a[8 * c];
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            a[7 * c + j] *= piv;
            inv[7 * c + j] *= piv;
        }
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            if (r == c) continue;
            const double f = a[7 * r + c];
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                a[7 * r + j] -= f * a[7 * c + j];
                inv[7 * r + j] -= f * inv[7 * c + j];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 49; ++k) D.Minv[(size_t)slot * 49 + k] = inv[k];
}

// ---------------------------------------------------------------------------------------------------------------- PCG
#define PG_SOLVE_T 1024
__global__ __launch_bounds__(PG_SOLVE_T) void k_pg_solve(PgDev D) {
    if (D.ctl->phase != 1) return;
    __shared__ double sw[16];
    const int tid = threadIdx.x, n = D.n;
    const double lambda = D.ctl->lambda;
    // z = Minv r of the rows this thread owns
    auto precond_rows = [&]() {
        double acc = 0.0;
        for (int row = tid; row < n; row += PG_SOLVE_T) {
            const int v = row / 7, k = row % 7;
            const double* M = D.Minv + (size_t)v * 49 + 7 * k;
            const double* rv = D.r + (size_t)v * 7;
            double zz = 0.0;
#pragma unroll
            for (int j = 0; j < 7; ++j) zz += M[j] * rv[j];
            D.z[row] = zz;
            acc += D.r[row] * zz;
        }
        return acc;
    };
    double t_bb = 0.0;
    for (int row = tid; row < n; row += PG_SOLVE_T) {
        const double bv = D.b[row];
        D.x[row] = 0.0;
        D.r[row] = bv;
        t_bb += bv * bv;
    }
    const double bb = pg_block_sum<16>(t_bb, sw);  // (its barriers also make r visible to the whole workgroup)
    int iters = 0, capped = 0;
    if (bb > 0.0) {
        double rz = pg_block_sum<16>(precond_rows(), sw);
        for (int row = tid; row < n; row += PG_SOLVE_T) D.p[row] = D.z[row];
        __syncthreads();
        const int max_it = PG_PCG_CAP_MULT * n;
        const double stop = (PG_PCG_TOL * PG_PCG_TOL) * bb;
        for (;;) {
            // Ap = (H + lambda I) p: the diagonal block, then the vertex's edges in ascending order with B_e or B_e^T
            double t_pap = 0.0;
            for (int row = tid; row < n; row += PG_SOLVE_T) {
                const int v = row / 7, k = row % 7;
                const double* Hd = D.Hd + (size_t)v * 49 + 7 * k;
                const double* pv = D.p + (size_t)v * 7;
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j < 7; ++j) acc += Hd[j] * pv[j];
                acc += lambda * pv[k];
                const int lo = D.v_off[v], hi = D.v_off[v + 1];
                for (int c = lo; c < hi; ++c) {
                    const int ent = D.v_ent[c], e = ent >> 1, side = ent & 1;
                    const int other = D.slot[side ? D.e_i[e] : D.e_j[e]];
                    if (other < 0) continue;
                    const double* B = D.rec + (size_t)e * PG_REC + PG_REC_HIJ;
                    const double* po = D.p + (size_t)other * 7;
                    double s = 0.0;
                    if (side) {
#pragma unroll
                        for (int j = 0; j < 7; ++j) s += B[7 * j + k] * po[j];
                    }
                    else {
#pragma unroll
                        for (int j = 0; j < 7; ++j) s += B[7 * k + j] * po[j];
                    }
                    acc += s;
                }
                D.Ap[row] = acc;
                t_pap += pv[k] * acc;
            }
            const double pap = pg_block_sum<16>(t_pap, sw);
            const double alpha = rz / pap;
            double t_rr = 0.0;
            for (int row = tid; row < n; row += PG_SOLVE_T) {
                D.x[row] += alpha * D.p[row];
                const double rn = D.r[row] - alpha * D.Ap[row];
                D.r[row] = rn;
                t_rr += rn * rn;
            }
            const double rr = pg_block_sum<16>(t_rr, sw);
            ++iters;
            if (!(rr > stop)) break;  // also leaves on a NaN
            if (iters >= max_it) {
                capped = 1;
                break;
            }
            const double rz_new = pg_block_sum<16>(precond_rows(), sw);
            const double beta = rz_new / rz;
            rz = rz_new;
            for (int row = tid; row < n; row += PG_SOLVE_T) D.p[row] = D.z[row] + beta * D.p[row];
            __syncthreads();
        }
    }
    if (tid == 0) {
        D.ctl->pcg_last_it = iters;
        D.ctl->pcg_total_it += iters;
        D.ctl->pcg_capped += capped;
    }
}

// ---------------------------------------------------------------------------------------------------------------- trial state
__global__ __launch_bounds__(64) void k_pg_update(PgDev D) {
    if (D.ctl->phase != 1) return;
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= D.N) return;
    const int cur = D.ctl->cur & 1;
    const double* src = D.est[cur] + (size_t)v * 8;
    double* dst = D.est[cur ^ 1] + (size_t)v * 8;
    const int slot = D.slot[v];
    if (slot < 0) {  // a fixed vertex keeps its bits
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[k] = src[k];
        return;
    }
    const double lambda = D.ctl->lambda;
    const double* x = D.x + (size_t)slot * 7;
    const double* b = D.b + (size_t)slot * 7;
    double sc = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) sc += x[k] * (lambda * x[k] + b[k]);
    D.scale_part[slot] = sc;
    SvVec7 u = SvVec7{x[0], x[1], x[2], x[3], x[4], x[5], x[6]};
    if (D.fix_scale) u.sg = 0.0;
    sv_sim3_store(dst, sv_sim3_mul(sv_sim3_exp(u), sv_sim3_load(src)));
}

__global__ __launch_bounds__(64) void k_pg_chi2(PgDev D) {
    if (D.ctl->phase != 1) return;
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= D.E) return;
    const double* est = D.est[(D.ctl->cur & 1) ^ 1];
    const SvVec7 err = pg_error(sv_sim3_load(D.meas + (size_t)e * 8), sv_sim3_load(est + (size_t)D.e_i[e] * 8), sv_sim3_load(est + (size_t)D.e_j[e] * 8));
    D.chi_trial[e] = pg_chi(err);
}

// ---------------------------------------------------------------------------------------------------------------- decision
// OptimizationAlgorithmLevenberg::solve's acceptance test and terminate_action, as lm_decide of ba_kernels.hip states them (no caller's
// stop flag here).  A failed solve -- only the envelope solver reports one (PgEnvCtl) -- rejects the trial whatever its chi2, as there.
__global__ __launch_bounds__(256) void k_pg_decide(PgDev D) {
    __shared__ double sw[4];
    if (D.ctl->phase != 1) return;
    double t_chi = 0.0, t_sc = 0.0;
    for (int e = threadIdx.x; e < D.E; e += 256) t_chi += D.chi_trial[e];
    for (int v = threadIdx.x; v < D.nfree; v += 256) t_sc += D.scale_part[v];
    const double temp_chi_sum = pg_block_sum<4>(t_chi, sw);
    double scale = pg_block_sum<4>(t_sc, sw);
    if (threadIdx.x != 0) return;
    PgCtl& c = *D.ctl;
    ++c.lm_trials;
    double temp_chi = temp_chi_sum;
    if (D.env && D.env->solve_failed) {
        temp_chi = 1.7976931348623157e308;
        ++D.env->failed_solves;
        ++D.env->failed_in_iteration;
    }
    double rho = c.current_chi - temp_chi;
    scale += 1e-3;
    rho /= scale;
    c.temp_chi = temp_chi;
    c.scale = scale;
    bool lambda_bad = false;
    if (rho > 0 && isfinite(temp_chi)) {
        double alpha = 1. - pow((2 * rho - 1), 3);
        alpha = fmin(alpha, 2. / 3.);
        c.lambda *= fmax(1. / 3., alpha);
        c.ni = 2.0;
        c.current_chi = temp_chi;
        c.cur ^= 1;  // accept: the trial state becomes the estimate
    }
    else {
        c.lambda *= c.ni;
        c.ni *= 2.0;
        lambda_bad = !isfinite(c.lambda);
    }
    ++c.qmax;
    c.rho = rho;
    if (!lambda_bad && rho < 0 && c.qmax < 10) return;  // another trial on the same linearisation (phase stays 1)
    if (c.qmax == 10 || rho == 0 || !isfinite(c.lambda)) c.ok = 0;
    if (D.env && c.qmax == 10 && D.env->failed_in_iteration == 10) D.env->numeric = 1;
    // postIteration: terminate_action on the chi2 of the estimate
    if (c.it == 0) c.last_chi = c.current_chi;
    else {
        const double gain = (c.last_chi - c.current_chi) / c.current_chi;
        c.last_chi = c.current_chi;
        if (gain >= 0 && gain < c.gain_thr) {
            c.stop = 1;
            c.stopped_by_gain = 1;
        }
    }
    ++c.it;
    c.phase = (c.it < c.it_max && !c.stop && c.ok) ? 0 : 2;
}

__global__ __launch_bounds__(64) void k_pg_output(PgDev D) {
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= D.N) return;
    const double* src = D.est[D.ctl->cur & 1] + (size_t)v * 8;
    double* o = D.out_sim3 + (size_t)v * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = src[k];
    double pose[12];
    sv_sim3_to_pose(sv_sim3_load(src), pose);
#pragma unroll
    for (int k = 0; k < 12; ++k) D.out_pose[(size_t)v * 12 + k] = pose[k];
}

__global__ __launch_bounds__(64) void k_pg_correct_landmarks(PgLandmarks P) {
    const int l = blockIdx.x * 64 + threadIdx.x;
    if (l >= P.L) return;
    const int r = P.ref[l];
    const SvSim3 cw = sv_sim3_load(P.sim3_before + (size_t)r * 8);
    const SvSim3 corrected_wc = sv_sim3_inv(sv_sim3_load(P.sim3_after + (size_t)r * 8));
    const SvVec3 p = sv3(P.pos_in[(size_t)l * 3], P.pos_in[(size_t)l * 3 + 1], P.pos_in[(size_t)l * 3 + 2]);
    const SvVec3 o = sv_sim3_map(corrected_wc, sv_sim3_map(cw, p));
    P.pos_out[(size_t)l * 3] = o.x, P.pos_out[(size_t)l * 3 + 1] = o.y, P.pos_out[(size_t)l * 3 + 2] = o.z;
}

inline int pg_blocks(int n, int per) { return (n + per - 1) / per; }

}  // namespace

void sv_pg_linearize(hipStream_t s, const PgDev& D) { hipLaunchKernelGGL(k_pg_linearize, dim3(pg_blocks(D.E, 2)), dim3(64), 0, s, D); }
void sv_pg_assemble(hipStream_t s, const PgDev& D) {
    if (D.nfree > 0) hipLaunchKernelGGL(k_pg_assemble, dim3(D.nfree), dim3(64), 0, s, D);
}
void sv_pg_prepare(hipStream_t s, const PgDev& D) { hipLaunchKernelGGL(k_pg_prepare, dim3(1), dim3(256), 0, s, D); }
void sv_pg_precond(hipStream_t s, const PgDev& D) {
    if (D.nfree > 0) hipLaunchKernelGGL(k_pg_precond, dim3(pg_blocks(D.nfree, 64)), dim3(64), 0, s, D);
}
void sv_pg_solve(hipStream_t s, const PgDev& D) {
    if (D.nfree > 0) hipLaunchKernelGGL(k_pg_solve, dim3(1), dim3(PG_SOLVE_T), 0, s, D);
}
void sv_pg_update(hipStream_t s, const PgDev& D) { hipLaunchKernelGGL(k_pg_update, dim3(pg_blocks(D.N, 64)), dim3(64), 0, s, D); }
void sv_pg_chi2(hipStream_t s, const PgDev& D) { hipLaunchKernelGGL(k_pg_chi2, dim3(pg_blocks(D.E, 64)), dim3(64), 0, s, D); }
void sv_pg_decide(hipStream_t s, const PgDev& D) { hipLaunchKernelGGL(k_pg_decide, dim3(1), dim3(256), 0, s, D); }
void sv_pg_output(hipStream_t s, const PgDev& D) { hipLaunchKernelGGL(k_pg_output, dim3(pg_blocks(D.N, 64)), dim3(64), 0, s, D); }
void sv_pg_correct_landmarks(hipStream_t s, const PgLandmarks& P) {
    if (P.L > 0) hipLaunchKernelGGL(k_pg_correct_landmarks, dim3(pg_blocks(P.L, 64)), dim3(64), 0, s, P);
}
