// Shared host-side pieces of the matcher entry points (svgpu_match.hip, svgpu_match2.hip): the sort scratch, the frame side of the
// cell matchers with its reprojected query side, and the cell matcher with its pass loop.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "sv_staged_call.h"
#include "match_layout.h"
#include "match_kernels.h"
#include "frame_kernels.h"

namespace svm {

// scratch for the angle-bin sorted copies of both sides (see k_bf_binsort)
inline void take_sort(Arena& A, BfProblem& P, int pairs, int cap1, int cap2) {
    const size_t p = (size_t)pairs;
    P.sd1 = A.take<uint32_t>(p * cap1 * 8);
    P.sd2 = A.take<uint32_t>(p * cap2 * 8);
    P.sa1 = A.take<float>(p * cap1);
    P.si1 = A.take<int>(p * cap1);
    P.sa2 = A.take<float>(p * cap2);
    P.si2 = A.take<int>(p * cap2);
    P.bs1 = A.take<int>(p * 362);
    P.bs2 = A.take<int>(p * 362);
    P.prune_ok = A.take<int>(p * 2);
}

// The frame side of the cell matcher (keypoints that get binned) -- host pointers.
struct InCellsFrame {
    const uint8_t* tdesc;
    const float* t_xy;
    const int32_t* t_octave;
    int nt;
    const uint8_t* occupied;
    const float* t_angle;
    const float* t_xright;
    float min_x, max_x, min_y, max_y;
    int grid_cols, grid_rows;
    const svgpu_frame* res = nullptr;  // resident frame (svgpu_frame_bind): tdesc / t_xy / t_octave / t_angle / t_xright are then ITS device arrays,
                                       // nothing of the keypoint side is uploaded and its grid is not rebuilt; `occupied` stays a host array
};
// svgpu_frame_bind: the keypoint-side arguments of the entry point that calls this are replaced by the bound frame's (one-shot)
inline const svgpu_frame* sv_take_bound_frame(svgpu_ctx* ctx) {
    if (!ctx) return nullptr;
    const svgpu_frame* f = ctx->bound_frame;
    ctx->bound_frame = nullptr;
    return f;
}

// Candidate lists built on the device + candidate matcher, in up to two passes on one StagedCall: the lists are sized from a total only
// the device knows.
//   exact        pass 0 stages, counts the candidates and reads the total back (read_now: a synchronisation in the middle of the call);
//                pass 1 places the lists and fills, matches and reads back.
//   speculative  (a capacity that sufficed for this context before: ctx->cand_cap_hint) everything is enqueued in pass 0 against that
//                capacity, the kernels do nothing if the total exceeds it, and the total comes back with the results: one
//                synchronisation per call.  A miss falls through to the exact pass 1.
// Pass 1 places again, and the arena may have to grow for the lists, which discards its contents: only then are staging and counting
// repeated.  Otherwise the arena pass 0 filled is reused, which rests on the prefix invariant of match_layout.h.
// The caller owns the query side: `place_q(A, P, G)` places it (between the keypoint side and the grid) and points P / G at it,
// `first_q(C)` uploads it, flushes -- the keypoint side's arrays travel in the same range -- and launches what writes the query windows;
// `extras(C)` names its further results, due even when there is no candidate at all.
template <class PlaceQ, class FirstQ, class Extras>
int in_cells_core(svgpu_ctx* ctx, int nq, const InCellsFrame& F, int check_orientation, unsigned thr, float lowe_ratio, int mode, PlaceQ&& place_q,
                  FirstQ&& first_q, Extras&& extras, int32_t* match_q, int* num_matches) {
    static const bool mtrace = std::getenv("SVGPU_MATCH_TRACE") != nullptr;  // host-side phase times of a call, to stderr
    auto tnow = [] { return std::chrono::steady_clock::now(); };
    auto t_prev = tnow();
    auto lap = [&](const char* what) {
        if (!mtrace) return;
        const auto t = tnow();
        std::fprintf(stderr, "[match] %-22s %7.1f us\n", what, std::chrono::duration<double, std::micro>(t - t_prev).count());
        t_prev = t;
    };
    const int nt = F.nt, ncell = F.grid_cols * F.grid_rows;
    CellPieces Y;
    CandProblem P;
    GridProblem G;
    bool lists = false;
    size_t cap = 0;
    auto layout = [&](UploadArena& A) {
        P = CandProblem{};
        G = GridProblem{};
        cell_layout(A, nq, nt, ncell, F.occupied, F.t_angle, F.t_xright, F.res != nullptr, lists, cap, Y, [&](UploadArena& Aq) { place_q(Aq, P, G); });
        // (resident frame: the keypoint side is the frame's own device arrays, binned when the frame was created)
        G.t_xy = P.t_xy = F.res ? F.t_xy : Y.t_xy.p;
        G.t_octave = P.t_octave = F.res ? F.t_octave : Y.t_octave.p;
        G.nq = P.nq = nq, G.nt = P.nt = nt, G.cols = F.grid_cols, G.rows = F.grid_rows, G.min_x = F.min_x, G.min_y = F.min_y;
        G.inv_w = (double)F.grid_cols / (F.max_x - F.min_x);  // float difference, double quotient: data/common.cc:86-87 via camera::base
        G.inv_h = (double)F.grid_rows / (F.max_y - F.min_y);
        G.cell_of = F.res ? F.res->cell_of : Y.cell_of.p;
        G.cell_off = F.res ? F.res->cell_off : Y.cell_off.p;
        G.cell_items = F.res ? F.res->cell_items : Y.cell_items.p;
        P.cand_off = G.cand_off = Y.cand_off, P.cand_idx = G.cand_idx = Y.cand_idx;
        const float* const t_xright = F.res ? F.t_xright : Y.t_xright.p;
        P.tdesc = (const uint32_t*)(F.res ? F.tdesc : Y.tdesc.p);
        P.occupied = Y.occupied;
        P.t_angle = F.res ? F.t_angle : Y.t_angle.p;
        P.t_xright = P.q_xright ? t_xright : nullptr;
        P.chi_t_xright = P.chi_gate ? t_xright : nullptr;
        P.check_orientation = check_orientation, P.thr = thr, P.lowe_ratio = lowe_ratio, P.mode = mode;
        P.dist = Y.dist, P.match_q = Y.match_q, P.num = Y.num;
    };
    const size_t guess = std::getenv("SVGPU_MATCH_EXACT_SIZING") ? 0 : ctx->cand_cap_hint;
    StagedCall C;
    int32_t total = 0, num = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const bool speculative = !pass && guess > 0;
        lists = pass || speculative;
        cap = pass ? (size_t)total : guess;
        bool survived = false;
        int rc = pass ? C.reopen(layout, survived) : C.open(ctx, "cell matcher: internal arena overflow", layout);
        if (rc) return rc;
        const bool fresh = !pass || !survived;
        if (fresh) {
            if (!F.res) C.up(Y.tdesc, F.tdesc, Y.t_xy, F.t_xy, Y.t_octave, F.t_octave, Y.t_angle, F.t_angle, Y.t_xright, F.t_xright);
            C.up(Y.occupied, F.occupied);
            if ((rc = first_q(C))) return rc;
        }
        lap(pass ? "stage (pass 1)" : "stage: uploads");
        if (fresh && F.res) sv_launch_grid_queries(C.s, G);
        else if (fresh) sv_launch_grid_build(C.s, G);
        if (!lists) {
            if ((rc = C.read_now(&total, G.cand_off + nq))) return rc;
            lap("grid + total read-back");
            if (mtrace) std::fprintf(stderr, "[match] nq %d nt %d candidates %d (%.1f per query)\n", nq, nt, total, nq ? (double)total / nq : 0.0);
            if (total > 0) continue;
            extras(C);
            return C.finish();
        }
        G.cap = P.cap = speculative ? (int)cap : 0;  // > 0: the capacity the kernels check
        sv_launch_grid_fill(C.s, G);
        sv_launch_cand(ctx, C.s, P, Y.owner, Y.match, Y.mdist);
        C.down(match_q, Y.match_q);
        C.down(&num, Y.num);
        extras(C);
        if (speculative) C.down(&total, G.cand_off + nq, 1);
        lap("lists + matcher enqueued");
        if ((rc = C.finish())) return rc;
        lap("final sync");
        if (speculative && (size_t)total > cap) {  // the guess was too small: nothing was written; size exactly
            ctx->cand_cap_hint = (size_t)total + (size_t)total / 4 + 4096;
            continue;
        }
        ctx->cand_cap_hint = std::max(ctx->cand_cap_hint, (size_t)total + (size_t)total / 4 + 4096);
        *num_matches = num;
        return SVGPU_OK;
    }
    return SVGPU_OK;
}

// The query side of "reproject, then match in cells" (ReprojQuery, match_layout.h): landmarks (host arrays) that are reprojected into
// the frame; the reprojection writes the window arrays the grid lookup reads, and `visible` is the queries' validity.
inline void reproj_bind(const ReprojPieces& Y, ReprojProblem& R) {
    R.pos_w = Y.pos_w, R.mean_normal = Y.mean_normal, R.min_valid_dist = Y.min_valid_dist, R.max_valid_dist = Y.max_valid_dist;  // inputs
    R.skip = Y.skip, R.q_level = Y.q_level;
    R.visible = Y.visible, R.reproj = Y.reproj, R.x_right = Y.x_right, R.pred_level = Y.pred_level;  // results
    R.q_xy = Y.q_xy, R.q_margin = Y.q_margin, R.q_min_level = Y.q_min_level, R.q_max_level = Y.q_max_level;  // windows
}
inline void reproj_place(UploadArena& A, const ReprojQuery& Q, ReprojPieces& Y, ReprojProblem& R, CandProblem& P, GridProblem& G) {
    reproj_layout(A, (size_t)R.n, Q, true, Y);
    reproj_bind(Y, R);
    G.q_xy = Y.q_xy, G.q_margin = Y.q_margin, G.q_min_level = Y.q_min_level, G.q_max_level = Y.q_max_level;
    G.q_valid = P.q_valid = Y.visible;
    P.qdesc = (const uint32_t*)Y.desc.p, P.q_angle = Y.q_angle, P.q_blocks = Y.q_blocks;
}
// one batched upload, then the reprojection that consumes it
inline int reproj_first(StagedCall& C, const ReprojQuery& Q, const ReprojPieces& Y, const ReprojProblem& R) {
    C.up(Y.desc, Q.desc, Y.pos_w, Q.pos_w, Y.mean_normal, Q.mean_normal, Y.min_valid_dist, Q.min_valid_dist, Y.max_valid_dist, Q.max_valid_dist,
         Y.skip, Q.skip, Y.q_level, Q.q_level, Y.q_angle, Q.q_angle, Y.q_blocks, Q.q_blocks);
    const int rc = C.flush();
    if (rc) return rc;
    sv_launch_reproject(C.s, R);
    return SVGPU_OK;
}
inline void reproj_down(StagedCall& C, const ReprojPieces& Y, uint8_t* visible, double* reproj, float* x_right, int32_t* pred_level) {
    C.down(visible, Y.visible), C.down(reproj, Y.reproj), C.down(x_right, Y.x_right), C.down(pred_level, Y.pred_level);
}

}  // namespace svm
