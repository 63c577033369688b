// svgpu_pose_graph_optimize / svgpu_pose_graph_correct_landmarks: host glue of the pose-graph kernels (posegraph_kernels.hip).  Host arrays
// in and out, synchronous: one upload, the launches on the context's stream, one read-back.  The Levenberg-Marquardt decisions are taken
// on the device (PgCtl); the host enqueues batches of damping trials and reads the control block between batches only to learn whether the
// run has ended.
#include <algorithm>
#include <cmath>

#include "sv_staged_call.h"
#include "sv_validate.h"
#include "posegraph_kernels.h"
#include "posegraph_layout.h"
#include "posegraph_envelope_layout.h"
#include "posegraph_envelope_plan.h"

static_assert(PG_LAYOUT_REC == PG_REC, "posegraph_layout.h and posegraph_kernels.h disagree on the edge record");
static_assert(sizeof(PgCtl) <= PG_LAYOUT_CTL, "posegraph_layout.h reserves too little for PgCtl");
static_assert(sizeof(PgEnvCtl) <= PG_ENV_LAYOUT_CTL, "posegraph_envelope_layout.h reserves too little for PgEnvCtl");

namespace {

// one damping trial; the kernels of a step that has nothing to do (PgCtl::phase) return at once.  K: the envelope solver's descriptor
// when it solves (its two kernels then stand where the preconditioner and the PCG stand), else null
void enqueue_step(svgpu_ctx* ctx, hipStream_t s, const PgDev& D, const PgEnvDev* K) {
    {
        SvProfScope prof(ctx, s, "k_pg_linearize");
        sv_pg_linearize(s, D);
    }
    {
        SvProfScope prof(ctx, s, "k_pg_assemble");
        sv_pg_assemble(s, D);
    }
    sv_pg_prepare(s, D);
    if (K) {
        {
            SvProfScope prof(ctx, s, "k_pg_env_assemble");
            sv_pg_env_assemble(s, *K);
        }
        SvProfScope prof(ctx, s, "k_pg_env_factor_solve");
        sv_pg_env_factor_solve(s, *K);
    }
    else {
        SvProfScope prof(ctx, s, "k_pg_solve");
        sv_pg_precond(s, D);
        sv_pg_solve(s, D);
    }
    {
        SvProfScope prof(ctx, s, "k_pg_trial");
        sv_pg_update(s, D);
        sv_pg_chi2(s, D);
        sv_pg_decide(s, D);
    }
}

void upload_plan(StagedCall& C, const PgEnvPieces& Y, const PgEnvPlan& P) {
    const PgEnvCtl e0{};
    // (the vector's own length, which the plan promises to be the piece's: one that disagreed is refused, not read or written past its end)
    const auto up = [&](Piece<int32_t> dst, const std::vector<int32_t>& v) { C.up(dst, v.data(), v.size()); };
    C.up(Y.ctl, (const char*)&e0, sizeof e0);  // the reservation is rounder than PgEnvCtl
    up(Y.order, P.order), up(Y.rowoff, P.rowoff), up(Y.coloff, P.coloff), up(Y.colrows, P.colrows), up(Y.colbase, P.colbase);
    up(Y.blk_src, P.blk_src), up(Y.pair_off, P.pair_off), up(Y.pair_ent, P.pair_ent), up(Y.pair_flag, P.pair_flag);
}

PgEnvDev plan_descriptor(const PgEnvPieces& Y, const PgEnvPlan& P) {
    PgEnvDev K{};
    K.env = (PgEnvCtl*)Y.ctl.p;
    K.nP = P.nfree, K.nblocks = (int)P.nblocks, K.max_m = P.max_column_rows;
    K.order = Y.order, K.rowoff = Y.rowoff, K.coloff = Y.coloff, K.colrows = Y.colrows, K.colbase = Y.colbase, K.blk_src = Y.blk_src;
    K.pair_off = Y.pair_off, K.pair_ent = Y.pair_ent, K.pair_flag = Y.pair_flag;
    K.val = Y.val, K.dinv = Y.dinv, K.y = Y.y;
    return K;
}

void fill_solver_stats(svgpu_pose_graph_solver_stats* st, int solver, const PgEnvPlan* P, int failed) {
    if (!st) return;
    st->solver = solver;
    st->ordering = P ? P->ordering : 0;
    st->envelope_blocks = P ? (int32_t)P->nblocks : 0;
    st->max_column_rows = P ? P->max_column_rows : 0;
    st->failed_solves = failed;
}

}  // namespace

extern "C" {

int svgpu_pose_graph_optimize(svgpu_ctx* ctx, int num_vertices, const double* sim3, const uint8_t* fixed, int num_edges, const int32_t* edge_v1,
                              const int32_t* edge_v2, const double* edge_sim3_21, int fix_scale, int max_iterations, double gain_threshold,
                              double* sim3_out, double* pose_cw_out, svgpu_pose_graph_stats* stats) {
    return svgpu_pose_graph_optimize_ex(ctx, num_vertices, sim3, fixed, num_edges, edge_v1, edge_v2, edge_sim3_21, fix_scale, max_iterations, gain_threshold,
                                        sim3_out, pose_cw_out, stats, nullptr, nullptr);
}

int svgpu_pose_graph_optimize_ex(svgpu_ctx* ctx, int num_vertices, const double* sim3, const uint8_t* fixed, int num_edges, const int32_t* edge_v1,
                              const int32_t* edge_v2, const double* edge_sim3_21, int fix_scale, int max_iterations, double gain_threshold,
                                 double* sim3_out, double* pose_cw_out, svgpu_pose_graph_stats* stats, const svgpu_pose_graph_options* options,
                                 svgpu_pose_graph_solver_stats* solver_stats) {
    const char* who = "svgpu_pose_graph_optimize: bad arguments";
    const int solver = options ? options->solver : SVGPU_PG_SOLVER_PCG;
    if (options && (options->reserved[0] || options->reserved[1] || options->reserved[2] || (solver != SVGPU_PG_SOLVER_PCG && solver != SVGPU_PG_SOLVER_ENVELOPE)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_pose_graph_optimize_ex: unknown solver or a reserved option that is not zero");
    const bool direct = solver == SVGPU_PG_SOLVER_ENVELOPE;
    if (!ctx || num_vertices < 1 || num_edges < 1 || max_iterations < 0 || !sim3 || !fixed || !edge_v1 || !edge_v2 || !edge_sim3_21 || !sim3_out)
        return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    const int N = num_vertices, E = num_edges;
    // ---- validation and structure: nothing is launched before all of it has passed
    std::vector<int32_t> slot(N);
    int nfree = 0;
    for (int v = 0; v < N; ++v) {
        if (!sv_sim3_ok(sim3 + 8 * (size_t)v)) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_pose_graph_optimize: a vertex is not a Sim3 (unit quaternion, positive scale)");
        slot[v] = fixed[v] ? -1 : nfree++;
    }
    if (nfree == N) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_pose_graph_optimize: no fixed vertex");
    std::vector<int32_t> v_off((size_t)nfree + 1, 0);
    for (int e = 0; e < E; ++e) {
        const int a = edge_v1[e], b = edge_v2[e];
        if (a < 0 || a >= N || b < 0 || b >= N) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_pose_graph_optimize: vertex index out of range");
        if (a == b) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_pose_graph_optimize: an edge from a vertex to itself");
        if (!sv_sim3_ok(edge_sim3_21 + 8 * (size_t)e)) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_pose_graph_optimize: a measurement is not a Sim3");
        if (slot[a] >= 0) ++v_off[slot[a] + 1];
        if (slot[b] >= 0) ++v_off[slot[b] + 1];
    }
    for (int k = 0; k < nfree; ++k) {
        if (v_off[k + 1] == 0) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_pose_graph_optimize: a free vertex without an edge");
        v_off[k + 1] += v_off[k];
    }
    // the free vertices' edge lists, in ascending edge order (built once: the structure does not change between iterations)
    const size_t incident = (size_t)v_off[nfree];
    std::vector<int32_t> v_ent(incident), fill(v_off.begin(), v_off.end() - 1);
    for (int e = 0; e < E; ++e) {
        const int sa = slot[edge_v1[e]], sb = slot[edge_v2[e]];
        if (sa >= 0) v_ent[fill[sa]++] = e << 1;
        if (sb >= 0) v_ent[fill[sb]++] = e << 1 | 1;
    }
    // the envelope solver's plan: elimination order, envelope and pair lists (host only)
    PgEnvPlan plan;
    if (direct) {
        std::vector<int32_t> sa(E), sb(E);
        for (int e = 0; e < E; ++e) sa[e] = slot[edge_v1[e]], sb[e] = slot[edge_v2[e]];
        pg_env_plan(nfree, E, sa.data(), sb.data(), plan);
        if (!plan.fits) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_pose_graph_optimize_ex: the envelope's value count is beyond 32-bit indexing");
    }

    PgPieces Y{};
    PgEnvPieces Ye{};
    StagedCall C;
    int rc = C.open(ctx, "svgpu_pose_graph_optimize: internal arena overflow", [&](UploadArena& A) {
        pg_optimize_layout(A, (size_t)N, (size_t)E, (size_t)nfree, incident, Y);
        if (direct) pg_envelope_layout(A, (size_t)nfree, (size_t)plan.nblocks, (size_t)plan.num_pairs, plan.pair_ent.size(), Ye);
    });
    if (rc) return rc;
    hipStream_t s = C.s;
    PgCtl c0{};
    c0.ni = 2.0;
    c0.gain_thr = gain_threshold;
    c0.it_max = max_iterations;
    c0.ok = 1;
    C.up(Y.ctl, (const char*)&c0, sizeof c0);  // the reservation is rounder than PgCtl
    C.up(Y.est0, sim3), C.up(Y.fixed, fixed), C.up(Y.slot, slot.data());
    C.up(Y.e_i, edge_v1), C.up(Y.e_j, edge_v2), C.up(Y.meas, edge_sim3_21), C.up(Y.v_off, v_off.data()), C.up(Y.v_ent, v_ent.data());
    if (direct) upload_plan(C, Ye, plan);
    if ((rc = C.flush())) return rc;

    PgDev D{};
    D.N = N, D.E = E, D.nfree = nfree, D.n = 7 * nfree, D.fix_scale = fix_scale != 0;
    D.ctl = (PgCtl*)Y.ctl.p;
    D.est[0] = Y.est0, D.est[1] = Y.est1;
    D.fixed = Y.fixed, D.slot = Y.slot, D.e_i = Y.e_i, D.e_j = Y.e_j, D.meas = Y.meas, D.v_off = Y.v_off, D.v_ent = Y.v_ent;
    D.rec = Y.rec, D.chi_trial = Y.chi_trial, D.Hd = Y.Hd, D.b = Y.b, D.maxd = Y.maxd, D.Minv = Y.Minv;
    D.x = Y.x, D.r = Y.r, D.z = Y.z, D.p = Y.p, D.Ap = Y.Ap, D.scale_part = Y.scale_part;
    D.out_sim3 = Y.out_sim3, D.out_pose = Y.out_pose;
    PgEnvDev K{};
    if (direct) {
        K = plan_descriptor(Ye, plan);
        K.ctl = D.ctl, K.damped = 1;
        K.Hd = Y.Hd, K.b = Y.b, K.x = Y.x, K.blk = Y.rec + PG_REC_HIJ, K.blk_stride = PG_REC;
        D.env = K.env;
    }

    // at most 10 trials per iteration; the first step also serves max_iterations == 0 (chi2 of the input, then phase 2)
    const long max_steps = std::max(1L, 10L * max_iterations);
    PgCtl* c_host = (PgCtl*)C.host(Y.ctl.p);
    long done = 0;
    int batch = 8;
    for (;;) {
        const long count = std::min<long>(batch, max_steps - done);
        for (long k = 0; k < count; ++k) enqueue_step(ctx, s, D, direct ? &K : nullptr);
        done += count;
        SV_HIP(ctx, hipGetLastError());
        SV_HIP(ctx, hipMemcpyAsync(c_host, Y.ctl, sizeof(PgCtl), hipMemcpyDeviceToHost, s));
        SV_HIP(ctx, hipStreamSynchronize(s));
        if (c_host->phase == 2 || done >= max_steps) break;
        batch = 16;
    }
    const PgCtl c = *c_host;
    sv_pg_output(s, D);
    PgEnvCtl ec{};
    if (direct) C.down((char*)&ec, Ye.ctl, sizeof ec);  // PgEnvCtl, in front of its reservation
    C.down(sim3_out, Y.out_sim3), C.down(pose_cw_out, Y.out_pose);
    if ((rc = C.finish())) return rc;
    if (stats) {
        stats->lm_iterations = c.it;
        stats->lm_trials = c.lm_trials;
        stats->pcg_iterations = c.pcg_total_it;
        stats->pcg_capped = c.pcg_capped;
        stats->stopped_by_gain = c.stopped_by_gain;
        stats->num_free = nfree;
        stats->initial_chi2 = c.chi_begin;
        stats->final_chi2 = c.current_chi;
        stats->lambda = c.lambda;
    }
    fill_solver_stats(solver_stats, solver, direct ? &plan : nullptr, ec.failed_solves);
    if (ec.numeric) return sv_set_error(ctx, SVGPU_ERR_NUMERIC, "svgpu_pose_graph_optimize_ex: the damped system was not positive definite at any of the 10 dampings of an iteration");
    return SVGPU_OK;
}

int svgpu_selftest_pose_graph_envelope_solve(svgpu_ctx* ctx, int nfree, int num_pairs, const int32_t* pair_a, const int32_t* pair_b, const double* diag_blocks,
                                             const double* pair_blocks, const double* rhs, double* x_out, svgpu_pose_graph_solver_stats* solver_stats) {
    const char* who = "svgpu_selftest_pose_graph_envelope_solve: bad arguments";
    if (!ctx || nfree < 1 || num_pairs < 0 || !diag_blocks || !rhs || !x_out || (num_pairs > 0 && (!pair_a || !pair_b || !pair_blocks)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    for (int k = 0; k < num_pairs; ++k)
        if (pair_a[k] < 0 || pair_a[k] >= nfree || pair_b[k] < 0 || pair_b[k] >= nfree || pair_a[k] == pair_b[k]) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    PgEnvPlan plan;
    pg_env_plan(nfree, num_pairs, pair_a, pair_b, plan);
    if (!plan.fits) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_selftest_pose_graph_envelope_solve: the envelope's value count is beyond 32-bit indexing");
    PgEnvSelftestPieces Y{};
    StagedCall C;
    int rc = C.open(ctx, "svgpu_selftest_pose_graph_envelope_solve: internal arena overflow", [&](UploadArena& A) {
        pg_envelope_selftest_layout(A, (size_t)nfree, (size_t)plan.nblocks, (size_t)plan.num_pairs, plan.pair_ent.size(), (size_t)num_pairs, Y);
    });
    if (rc) return rc;
    hipStream_t s = C.s;
    PgCtl c0{};
    c0.phase = 1;
    C.up(Y.ctl, (const char*)&c0, sizeof c0);  // the reservation is rounder than PgCtl
    C.up(Y.diag, diag_blocks), C.up(Y.blocks, pair_blocks), C.up(Y.rhs, rhs);
    upload_plan(C, Y.env, plan);
    if ((rc = C.flush())) return rc;
    PgEnvDev K = plan_descriptor(Y.env, plan);
    K.ctl = (const PgCtl*)Y.ctl.p, K.damped = 0;
    K.Hd = Y.diag, K.b = Y.rhs, K.x = Y.x, K.blk = Y.blocks, K.blk_stride = 49;
    {
        SvProfScope prof(ctx, s, "k_pg_env_assemble");
        sv_pg_env_assemble(s, K);
    }
    {
        SvProfScope prof(ctx, s, "k_pg_env_factor_solve");
        sv_pg_env_factor_solve(s, K);
    }
    PgEnvCtl ec{};
    std::vector<double> x(Y.x.n);
    C.down((char*)&ec, Y.env.ctl, sizeof ec);  // PgEnvCtl, in front of its reservation
    C.down(x.data(), Y.x);
    if ((rc = C.finish())) return rc;
    fill_solver_stats(solver_stats, SVGPU_PG_SOLVER_ENVELOPE, &plan, ec.solve_failed ? 1 : 0);
    if (ec.solve_failed) return sv_set_error(ctx, SVGPU_ERR_NUMERIC, "svgpu_selftest_pose_graph_envelope_solve: the system is not positive definite");
    std::copy(x.begin(), x.end(), x_out);
    return SVGPU_OK;
}

int svgpu_pose_graph_correct_landmarks(svgpu_ctx* ctx, int num_vertices, const double* sim3_before, const double* sim3_after, int num_landmarks,
                                       const int32_t* ref_vertex, const double* pos_w, double* pos_w_out) {
    const char* who = "svgpu_pose_graph_correct_landmarks: bad arguments";
    if (!ctx || num_vertices < 1 || num_landmarks < 0 || !sim3_before || !sim3_after) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    if (num_landmarks == 0) return SVGPU_OK;
    if (!ref_vertex || !pos_w || !pos_w_out) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    const size_t N = (size_t)num_vertices, L = (size_t)num_landmarks;
    for (size_t l = 0; l < L; ++l)
        if (ref_vertex[l] < 0 || ref_vertex[l] >= num_vertices)
            return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_pose_graph_correct_landmarks: reference vertex out of range");
    for (size_t v = 0; v < N; ++v)
        if (!sv_sim3_ok(sim3_before + 8 * v) || !sv_sim3_ok(sim3_after + 8 * v))
            return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_pose_graph_correct_landmarks: a vertex is not a Sim3");
    PgLandmarkPieces Y{};
    StagedCall C;
    int rc = C.open(ctx, "svgpu_pose_graph_correct_landmarks: internal arena overflow", [&](UploadArena& A) { pg_landmarks_layout(A, N, L, Y); });
    if (rc) return rc;
    hipStream_t s = C.s;
    C.up(Y.before, sim3_before), C.up(Y.after, sim3_after), C.up(Y.ref, ref_vertex), C.up(Y.pos_in, pos_w);
    if ((rc = C.flush())) return rc;
    PgLandmarks P{};
    P.L = num_landmarks, P.N = num_vertices, P.sim3_before = Y.before, P.sim3_after = Y.after, P.ref = Y.ref, P.pos_in = Y.pos_in, P.pos_out = Y.pos_out;
    {
        SvProfScope prof(ctx, s, "k_pg_correct_landmarks");
        sv_pg_correct_landmarks(s, P);
    }
    C.down(pos_w_out, Y.pos_out);
    return C.finish();
}

}  // extern "C"
