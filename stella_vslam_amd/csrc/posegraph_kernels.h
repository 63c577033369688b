// Problem descriptor and launchers of the pose-graph kernels (posegraph_kernels.hip): optimize::graph_optimizer
// (optimize/graph_optimizer.cc) on the device -- Sim3 vertices, binary edges log(C * v1 * v2^-1) with numeric Jacobians, Levenberg-Marquardt.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// The damped system (H + lambda I) dx = b is solved by block-Jacobi preconditioned conjugate gradients.  It stops when
// |r|^2 <= PG_PCG_TOL^2 |b|^2, r being the recursively updated residual, or after PG_PCG_CAP_MULT * (7 * free vertices) iterations.
#define PG_PCG_TOL 1e-14
#define PG_PCG_CAP_MULT 10

// per-edge record of k_pg_linearize, in doubles: Ji^T Ji, Ji^T Jj, Jj^T Jj (7x7 row-major each), -Ji^T e, -Jj^T e, e^T e
#define PG_REC 162
#define PG_REC_HIJ 49
#define PG_REC_HJJ 98
#define PG_REC_BI 147
#define PG_REC_BJ 154
#define PG_REC_CHI 161

// Levenberg-Marquardt control block, resident in device memory: the damping loop of OptimizationAlgorithmLevenberg::solve and the
// terminate_action hook as k_ba_decide states them (ba_kernels.hip).  Phases as in BaCtl: 0 = the next step linearises, 1 = a
// linearisation is in place and a trial runs, 2 = optimize() has finished and every kernel returns at once.
struct PgCtl {
    double lambda, ni, current_chi, last_chi, temp_chi, scale, rho, chi_begin;
    double gain_thr, pad0;
    int cur;  // which of the two estimate buffers holds the estimate (the other receives the trial)
    int it, it_max, qmax, phase, ok, stop, stopped_by_gain;
    int lm_trials, pcg_total_it, pcg_last_it, pcg_capped;
};

struct PgDev {
    int N, E, nfree, n;  // vertices, edges, free vertices, unknowns = 7 * nfree
    int fix_scale;
    PgCtl* ctl;
    double* est[2];         // N x 8 (qx qy qz qw tx ty tz s)
    const uint8_t* fixed;   // N
    const int32_t* slot;    // N: index among the free vertices or -1
    const int32_t* e_i;     // E: vertex 0 of the edge
    const int32_t* e_j;     // E: vertex 1
    const double* meas;     // E x 8: Sim3_21
    const int32_t* v_off;   // nfree + 1: incident edges of a free vertex, ascending edge order
    const int32_t* v_ent;   // edge << 1 | side (0: the vertex is vertex 0 of the edge)
    double* rec;            // E x PG_REC
    double* chi_trial;      // E
    double* Hd;             // nfree x 49
    double* b;              // n
    double* maxd;           // nfree: largest |diagonal| of the vertex's block
    double* Minv;           // nfree x 49: inverse of the damped diagonal block
    double *x, *r, *z, *p, *Ap;  // n each
    double* scale_part;     // nfree: the vertex's share of dx^T (lambda dx + b)
    double* out_sim3;       // N x 8
    double* out_pose;       // N x 12: [R | t / s]
    struct PgEnvCtl* env;   // the envelope solver's control block; null when the PCG solves
};

// The direct solver (posegraph_envelope.hip): block envelope LL^T of the damped system in the order posegraph_envelope_plan.h chose.
// Its control block: k_pg_env_factor_solve reports a pivot that is not positive and finite, k_pg_decide counts it as a failed trial.
struct PgEnvCtl {
    int solve_failed;         // the trial in flight
    int failed_solves;        // over the run
    int failed_in_iteration;  // since the last linearisation
    int numeric;              // all 10 trials of an iteration failed: the run ended on it
};
struct PgEnvDev {
    const PgCtl* ctl;          // phase and lambda
    PgEnvCtl* env;
    int nP, nblocks, max_m;    // block rows, envelope blocks, tallest column (rows below the diagonal)
    int damped;                // 1: lambda of the control block goes on the diagonal (0: the self-test's system as it is)
    const double* Hd;          // nP x 49 diagonal blocks, slot order
    const double* b;           // 7 nP right-hand side, slot order
    double* x;                 // 7 nP solution, slot order
    const double* blk;         // per edge: the 7x7 block Ji^T Jj at blk + edge * blk_stride
    int blk_stride;
    const int32_t *order, *rowoff, *coloff, *colrows, *colbase, *blk_src, *pair_off, *pair_ent, *pair_flag;
    double *val, *dinv, *y;    // envelope blocks, inverse diagonal factors, right-hand side in plan order
};
void sv_pg_env_assemble(hipStream_t s, const PgEnvDev& K);
void sv_pg_env_factor_solve(hipStream_t s, const PgEnvDev& K);

void sv_pg_linearize(hipStream_t s, const PgDev& D);
void sv_pg_assemble(hipStream_t s, const PgDev& D);
void sv_pg_prepare(hipStream_t s, const PgDev& D);
void sv_pg_precond(hipStream_t s, const PgDev& D);
void sv_pg_solve(hipStream_t s, const PgDev& D);
void sv_pg_update(hipStream_t s, const PgDev& D);
void sv_pg_chi2(hipStream_t s, const PgDev& D);
void sv_pg_decide(hipStream_t s, const PgDev& D);
void sv_pg_output(hipStream_t s, const PgDev& D);

// corrected_Sim3_wc.map(Sim3_cw.map(pos_w)) per landmark (graph_optimizer.cc:284-301)
struct PgLandmarks {
    int L, N;
    const double* sim3_before;  // N x 8
    const double* sim3_after;   // N x 8
    const int32_t* ref;         // L: reference vertex
    const double* pos_in;       // L x 3
    double* pos_out;            // L x 3
};
void sv_pg_correct_landmarks(hipStream_t s, const PgLandmarks& P);
