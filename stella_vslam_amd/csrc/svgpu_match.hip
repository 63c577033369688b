// Host side of the matchers: staging of host buffers into the context's scratch arena, launches.
#include <algorithm>
#include <cmath>
#include <utility>

#include "svgpu_match_common.h"

using namespace svm;

extern "C" {

int svgpu_hamming_distance(svgpu_ctx* ctx, const uint8_t* a, const uint8_t* b, int n, uint32_t* dist) {
    if (!ctx || n < 0 || (n > 0 && (!a || !b || !dist))) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_hamming_distance");
    if (n == 0) return SVGPU_OK;
    uint32_t *da, *db, *dd;
    StagedCall C;
    int rc = C.open(ctx, "svgpu_hamming_distance: internal arena overflow", [&](UploadArena& A) {
        da = A.take<uint32_t>((size_t)n * 8);
        db = A.take<uint32_t>((size_t)n * 8);
        dd = A.take<uint32_t>(n);
    });
    if (rc) return rc;
    C.up(da, (const uint32_t*)a, (size_t)n * 8);
    C.up(db, (const uint32_t*)b, (size_t)n * 8);
    if ((rc = C.flush())) return rc;
    sv_launch_hamming_pairs(C.s, da, db, n, dd);
    C.down(dist, dd, n);
    return C.finish();
}

int svgpu_hamming_matrix(svgpu_ctx* ctx, const uint8_t* desc1, int n1, const uint8_t* desc2, int n2, uint16_t* out) {
    if (!ctx || n1 < 0 || n2 < 0) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_hamming_matrix");
    if (n1 == 0 || n2 == 0) return SVGPU_OK;
    if (!desc1 || !desc2 || !out) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_hamming_matrix: null pointer");
    uint32_t *d1, *d2;
    uint16_t* dm;
    StagedCall C;
    int rc = C.open(ctx, "svgpu_hamming_matrix: internal arena overflow", [&](UploadArena& A) {
        d1 = A.take<uint32_t>((size_t)n1 * 8);
        d2 = A.take<uint32_t>((size_t)n2 * 8);
        dm = A.take<uint16_t>((size_t)n1 * n2);  // behind both inputs: the upload stops short of it
    });
    if (rc) return rc;
    C.up(d1, (const uint32_t*)desc1, (size_t)n1 * 8);
    C.up(d2, (const uint32_t*)desc2, (size_t)n2 * 8);
    if ((rc = C.flush())) return rc;
    sv_launch_hamming_matrix(C.s, d1, n1, d2, n2, dm);
    C.down(out, dm, (size_t)n1 * n2);
    return C.finish();
}

}  // extern "C"

namespace {
int bf_batch_device(svgpu_ctx* ctx, int pairs, int ring1, const uint8_t* desc1_dev, const svgpu_keypoint* kps1_dev, const int32_t* n1_dev,
                    int cap1, const uint8_t* desc2_dev, const svgpu_keypoint* kps2_dev, const int32_t* n2_dev, int cap2, int n_stride,
                    const uint8_t* valid2_dev, float lowe_ratio, int check_orientation, int32_t* matched_dev, int32_t* num_dev,
                    void* stream, const float* angles1_dev = nullptr, const float* angles2_dev = nullptr) {
    if (!ctx || pairs < 1 || !desc1_dev || !kps1_dev || !n1_dev || !desc2_dev || !kps2_dev || !n2_dev || cap1 < 1 || cap2 < 1
        || cap1 > 65535 || cap2 > 65535 || !matched_dev || !num_dev)
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_match_bruteforce_batch_device: bad arguments");
    SV_HIP(ctx, hipSetDevice(ctx->device));
    BfProblem P{};
    int *g_owner, *g_match;
    auto layout = [&](Arena& A) {
        P.topk = A.take<uint32_t>((size_t)pairs * cap2 * BF_LIST);
        P.cnt = A.take<int32_t>((size_t)pairs * cap2);
        g_owner = A.take<int>((size_t)pairs * cap1);
        g_match = A.take<int>((size_t)pairs * cap2);
        take_sort(A, P, pairs, cap1, cap2);
    };
    int rc = sv_scratch_layout(ctx, "svgpu_match_bruteforce_batch_device: internal arena overflow", layout);
    if (rc) return rc;
    P.desc1 = (const uint32_t*)desc1_dev;
    P.desc2 = (const uint32_t*)desc2_dev;
    if (angles1_dev && angles2_dev) {  // packed copies (svgpu_orb_extract_batch_device_angles): 4 bytes per keypoint instead of a 28-byte stride
        P.angle1 = angles1_dev;
        P.angle2 = angles2_dev;
        P.angle_stride = 1;
    }
    else {
        P.angle1 = &kps1_dev->angle;
        P.angle2 = &kps2_dev->angle;
        P.angle_stride = sizeof(svgpu_keypoint) / sizeof(float);
    }
    P.n1_dev = n1_dev;
    P.n2_dev = n2_dev;
    P.n_stride = n_stride;
    P.cap1 = cap1;
    P.cap2 = cap2;
    P.ring1 = ring1;
    P.valid2 = valid2_dev;
    P.lowe_ratio = lowe_ratio;
    P.check_orientation = check_orientation;
    P.matched = matched_dev;
    P.num = num_dev;
    sv_launch_bf(ctx, stream ? (hipStream_t)stream : ctx->stream, P, pairs, g_owner, g_match);
    SV_HIP(ctx, hipGetLastError());
    return SVGPU_OK;
}
}  // namespace

extern "C" {

int svgpu_match_bruteforce_batch_device(svgpu_ctx* ctx, int pairs, const uint8_t* desc1_dev,
                                        const svgpu_keypoint* kps1_dev, const int32_t* n1_dev, int cap1,
                                        const uint8_t* desc2_dev, const svgpu_keypoint* kps2_dev,
                                        const int32_t* n2_dev, int cap2, int n_stride, const uint8_t* valid2_dev,
                                        float lowe_ratio, int check_orientation, int32_t* matched_dev,
                                        int32_t* num_dev, void* stream) {
    return bf_batch_device(ctx, pairs, 0, desc1_dev, kps1_dev, n1_dev, cap1, desc2_dev, kps2_dev, n2_dev, cap2, n_stride, valid2_dev, lowe_ratio,
                           check_orientation, matched_dev, num_dev, stream);
}

int svgpu_match_consecutive_batch_device(svgpu_ctx* ctx, int frames, const uint8_t* desc_dev, const svgpu_keypoint* kps_dev,
                                         const int32_t* n_dev, int cap, int n_stride, const uint8_t* valid_dev, float lowe_ratio,
                                         int check_orientation, int32_t* matched_dev, int32_t* num_dev, void* stream) {
    if (frames < 2) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_match_consecutive_batch_device: needs at least two frames");
    return bf_batch_device(ctx, frames, frames, desc_dev, kps_dev, n_dev, cap, desc_dev, kps_dev, n_dev, cap, n_stride, valid_dev, lowe_ratio,
                           check_orientation, matched_dev, num_dev, stream);
}

int svgpu_match_consecutive_batch_device_angles(svgpu_ctx* ctx, int frames, const uint8_t* desc_dev, const svgpu_keypoint* kps_dev, const float* angles_dev,
                                                const int32_t* n_dev, int cap, int n_stride, const uint8_t* valid_dev, float lowe_ratio,
                                                int check_orientation, int32_t* matched_dev, int32_t* num_dev, void* stream) {
    if (frames < 2) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_match_consecutive_batch_device: needs at least two frames");
    return bf_batch_device(ctx, frames, frames, desc_dev, kps_dev, n_dev, cap, desc_dev, kps_dev, n_dev, cap, n_stride, valid_dev, lowe_ratio,
                           check_orientation, matched_dev, num_dev, stream, angles_dev, angles_dev);
}

int svgpu_match_bruteforce(svgpu_ctx* ctx, const uint8_t* desc1, const float* angle1, int n1, const uint8_t* desc2,
                           const float* angle2, const uint8_t* valid2, int n2, float lowe_ratio,
                           int check_orientation, int32_t* matched_2_in_1, int* num_matches) {
    if (!ctx || n1 < 0 || n2 < 0 || n1 > 65535 || n2 > 65535 || !num_matches)
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_match_bruteforce: bad sizes");
    *num_matches = 0;
    if (n1 > 0 && !matched_2_in_1) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_match_bruteforce: null output");
    for (int i = 0; i < n1; ++i) matched_2_in_1[i] = -1;
    if (n1 == 0 || n2 == 0) return SVGPU_OK;
    if (!desc1 || !desc2 || (check_orientation && (!angle1 || !angle2)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_match_bruteforce: null input");
    uint32_t *d1, *d2;
    float *a1, *a2;
    uint8_t* v2;
    int *g_owner, *g_match;
    BfProblem P{};
    // inputs through the page-locked mirror of the arena: one copy down (the five arrays are the first takes: one contiguous range), one up
    StagedCall C;
    int rc = C.open(ctx, "svgpu_match_bruteforce: internal arena overflow", [&](UploadArena& A) {
        d1 = A.take<uint32_t>((size_t)n1 * 8);
        d2 = A.take<uint32_t>((size_t)n2 * 8);
        a1 = A.take<float>(n1);
        a2 = A.take<float>(n2);
        v2 = A.take<uint8_t>(n2);
        P.topk = A.take<uint32_t>((size_t)n2 * BF_LIST);
        P.cnt = A.take<int32_t>(n2);
        P.matched = A.take<int32_t>(n1);
        g_owner = A.take<int>(n1);
        g_match = A.take<int>(n2);
        P.num = A.take<int32_t>(1);
        take_sort(A, P, 1, n1, n2);
    });
    if (rc) return rc;
    hipStream_t s = C.s;
    C.up(d1, (const uint32_t*)desc1, (size_t)n1 * 8);
    C.up(d2, (const uint32_t*)desc2, (size_t)n2 * 8);
    if (angle1) C.up(a1, angle1, n1);
    else memset(C.stage(a1, n1), 0, (size_t)n1 * 4);  // no angles: zeroed rows, written in the mirror, travel with the range
    if (angle2) C.up(a2, angle2, n2);
    else memset(C.stage(a2, n2), 0, (size_t)n2 * 4);
    C.up(v2, valid2, n2);
    if ((rc = C.flush())) return rc;
    P.desc1 = d1;
    P.desc2 = d2;
    P.angle1 = a1;
    P.angle2 = a2;
    P.angle_stride = 1;
    P.n1 = n1;
    P.n2 = n2;
    P.cap1 = n1;
    P.cap2 = n2;
    P.valid2 = valid2 ? v2 : nullptr;
    P.lowe_ratio = lowe_ratio;
    P.check_orientation = check_orientation;
    sv_launch_bf(ctx, s, P, 1, g_owner, g_match);
    int32_t num = 0;
    C.down(matched_2_in_1, P.matched, n1);
    C.down(&num, P.num, 1);
    if ((rc = C.finish())) return rc;
    *num_matches = num;
    return SVGPU_OK;
}

int svgpu_match_candidates(svgpu_ctx* ctx, const uint8_t* qdesc, int nq, const uint8_t* tdesc, const int32_t* t_octave,
                           int nt, const int32_t* cand_off, const int32_t* cand_idx, const uint8_t* cand_skip,
                           const uint8_t* q_valid, const uint8_t* occupied, const float* q_angle, const float* t_angle, int check_orientation,
                           const float* q_xright, const float* t_xright, const float* q_xr_tol, unsigned thr,
                           float lowe_ratio, int mode, int32_t* match_q, int* num_matches) {
    if (!ctx || nq < 0 || nt < 0 || nt >= (1 << 22) || !num_matches || (mode < SVGPU_MATCH_BEST_ONLY || mode > SVGPU_MATCH_AREA))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_match_candidates: bad arguments");
    *num_matches = 0;
    if (nq == 0) return SVGPU_OK;
    if (!match_q || !cand_off) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_match_candidates: null pointer");
    for (int q = 0; q < nq; ++q) match_q[q] = -1;
    const int nc = cand_off[nq];
    if (nc == 0 || nt == 0) return SVGPU_OK;
    if (!qdesc || !tdesc || !cand_idx || (check_orientation && (!q_angle || !t_angle))
        || ((q_xright || t_xright || q_xr_tol) && !(q_xright && t_xright && q_xr_tol)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_match_candidates: inconsistent inputs");
    for (int q = 0; q < nq; ++q)
        if (cand_off[q + 1] < cand_off[q]) return sv_set_error(ctx, SVGPU_ERR_INVALID, "cand_off not monotone");
    for (int c = 0; c < nc; ++c)
        if (cand_idx[c] < 0 || cand_idx[c] >= nt) return sv_set_error(ctx, SVGPU_ERR_INVALID, "cand_idx out of range");
    CandProblem P{};
    Piece<uint8_t> d_qdesc, d_tdesc, d_skip, d_qvalid, d_occ;
    Piece<int32_t> d_toct, d_off, d_idx;
    Piece<float> d_qang, d_tang, d_qxr, d_txr, d_qtol;
    int *owner, *match;
    unsigned* mdist;
    StagedCall C;
    int rc = C.open(ctx, "svgpu_match_candidates: internal arena overflow", [&](UploadArena& A) {
        P.qdesc = (const uint32_t*)(d_qdesc = A.piece<uint8_t>((size_t)nq * 32)).p;  // (descriptors, offsets and indices were checked above)
        P.tdesc = (const uint32_t*)(d_tdesc = A.piece<uint8_t>((size_t)nt * 32)).p;
        P.t_octave = d_toct = optional_piece<int32_t>(A, t_octave, nt);
        P.cand_off = d_off = A.piece<int32_t>((size_t)nq + 1);
        P.cand_idx = d_idx = A.piece<int32_t>(nc);
        P.cand_skip = d_skip = optional_piece<uint8_t>(A, cand_skip, nc);
        P.q_valid = d_qvalid = optional_piece<uint8_t>(A, q_valid, nq);
        P.occupied = d_occ = optional_piece<uint8_t>(A, occupied, nt);
        P.q_angle = d_qang = optional_piece<float>(A, q_angle, nq);
        P.t_angle = d_tang = optional_piece<float>(A, t_angle, nt);
        P.q_xright = d_qxr = optional_piece<float>(A, q_xright, nq);
        P.t_xright = d_txr = optional_piece<float>(A, t_xright, nt);
        P.q_xr_tol = d_qtol = optional_piece<float>(A, q_xr_tol, nq);
        P.dist = A.take<uint32_t>(nc);
        P.match_q = A.take<int32_t>(nq);
        P.num = A.take<int32_t>(1);
        owner = A.take<int>(nt);
        match = A.take<int>(nq);
        mdist = A.take<unsigned>(nt);
    });
    if (rc) return rc;
    hipStream_t s = C.s;
    C.up(d_qdesc, qdesc, d_tdesc, tdesc, d_toct, t_octave, d_off, cand_off, d_idx, cand_idx, d_skip, cand_skip, d_qvalid, q_valid, d_occ, occupied);
    C.up(d_qang, q_angle, d_tang, t_angle, d_qxr, q_xright, d_txr, t_xright, d_qtol, q_xr_tol);
    if ((rc = C.flush())) return rc;
    P.nq = nq, P.nt = nt, P.check_orientation = check_orientation, P.thr = thr, P.lowe_ratio = lowe_ratio, P.mode = mode;
    sv_launch_cand(ctx, s, P, owner, match, mdist);
    int32_t num = 0;
    C.down(match_q, P.match_q, nq);
    C.down(&num, P.num, 1);
    if ((rc = C.finish())) return rc;
    *num_matches = num;
    return SVGPU_OK;
}

int svgpu_selftest_cand_replay_form(int nq, int nt, int with_cnt, int mode) {
    if (nq < 0 || nt < 0 || mode < SVGPU_MATCH_BEST_ONLY || mode > SVGPU_MATCH_AREA) return -2;
    return sv_cand_replay_form(nq, nt, with_cnt != 0, mode);
}

int svgpu_match_in_cells(svgpu_ctx* ctx, const uint8_t* qdesc, int nq, const float* q_xy, const float* q_margin,
                         const int32_t* q_min_level, const int32_t* q_max_level, const uint8_t* q_valid, const float* q_angle,
                         const float* q_xright, const float* q_xr_tol, const uint8_t* tdesc, const float* t_xy,
                         const int32_t* t_octave, int nt, const uint8_t* occupied, const float* t_angle, const float* t_xright,
                         float min_x, float max_x, float min_y, float max_y, int grid_cols, int grid_rows,
                         int check_orientation, unsigned thr, float lowe_ratio, int mode, int32_t* match_q, int* num_matches) {
    // both one-shots are consumed FIRST, whatever happens next: an early error return must not leave them armed for an unrelated call
    const svgpu_frame* rf = sv_take_bound_frame(ctx);
    const uint8_t* const q_blocks = ctx ? ctx->next_q_blocks : nullptr;  // svgpu_match_set_query_blocks
    if (ctx) ctx->next_q_blocks = nullptr;
    if (rf) {  // resident keypoint side: the frame's own device arrays, bounds and grid (svgpu_frame_bind)
        tdesc = rf->desc, t_xy = rf->xy, t_octave = rf->octave, nt = rf->n;
        t_angle = check_orientation ? rf->angle : nullptr;
        t_xright = (q_xright && rf->has_xright) ? rf->xright : nullptr;
        if (!t_xright) q_xright = nullptr, q_xr_tol = nullptr;  // (a monocular frame has no stereo gate: projection.cc:57)
        min_x = rf->min_x, max_x = rf->max_x, min_y = rf->min_y, max_y = rf->max_y, grid_cols = rf->grid_cols, grid_rows = rf->grid_rows;
    }
    if (!ctx || nq < 0 || nt < 0 || nt >= (1 << 22) || !num_matches || mode < SVGPU_MATCH_BEST_ONLY || mode > SVGPU_MATCH_AREA || grid_cols < 1 || grid_rows < 1
        || (size_t)grid_cols * grid_rows > (size_t(1) << 22) || !(min_x < max_x) || !(min_y < max_y))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_match_in_cells: bad arguments");
    *num_matches = 0;
    if (nq == 0) return SVGPU_OK;
    if (!match_q) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_match_in_cells: null pointer");
    for (int q = 0; q < nq; ++q) match_q[q] = -1;
    if (nt == 0) return SVGPU_OK;
    if (!qdesc || !q_xy || !q_margin || !tdesc || !t_xy || !t_octave || (check_orientation && (!q_angle || !t_angle))
        || ((q_xright || t_xright || q_xr_tol) && !(q_xright && t_xright && q_xr_tol)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_match_in_cells: inconsistent inputs");
    InCellsFrame F{tdesc, t_xy, t_octave, nt, occupied, t_angle, t_xright, min_x, max_x, min_y, max_y, grid_cols, grid_rows};
    F.res = rf;
    const CellQuery S{qdesc, q_xy, q_margin, q_min_level, q_max_level, q_valid, q_angle, q_xright, q_xr_tol, q_blocks};
    CellQueryPieces Q;
    return in_cells_core(
        ctx, nq, F, check_orientation, thr, lowe_ratio, mode,
        [&](UploadArena& A, CandProblem& P, GridProblem& G) {
            cell_query_layout(A, nq, S, Q);
            P.qdesc = (const uint32_t*)Q.desc.p;
            G.q_xy = Q.xy, G.q_margin = Q.margin, G.q_min_level = Q.min_level, G.q_max_level = Q.max_level;
            G.q_valid = P.q_valid = Q.valid;
            P.q_angle = Q.angle, P.q_xright = Q.xright, P.q_xr_tol = Q.xr_tol, P.q_blocks = Q.blocks;
        },
        [&](StagedCall& C) {
            C.up(Q.desc, S.desc, Q.xy, S.xy, Q.margin, S.margin, Q.min_level, S.min_level, Q.max_level, S.max_level);
            C.up(Q.valid, S.valid, Q.angle, S.angle, Q.xright, S.xright, Q.xr_tol, S.xr_tol, Q.blocks, S.blocks);
            return C.flush();
        },
        [](StagedCall&) {}, match_q, num_matches);
}

int svgpu_camera_image_bounds(svgpu_ctx* ctx, svgpu_camera* cam) {
    if (!ctx || !cam || cam->model < SVGPU_CAM_PERSPECTIVE || cam->model > SVGPU_CAM_RADIAL_DIVISION)
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_camera_image_bounds: bad arguments");
    const float cols = (float)cam->cols, rows = (float)cam->rows;
    const int nd = cam->model == SVGPU_CAM_PERSPECTIVE ? 5 : cam->model == SVGPU_CAM_FISHEYE ? 4 : cam->model == SVGPU_CAM_RADIAL_DIVISION ? 1 : 0;
    bool none = true;
    for (int i = 0; i < nd; ++i) none = none && cam->dist[i] == 0;
    if (none) {  // "any distortion does not exist"
        cam->min_x = 0.0f, cam->max_x = cols, cam->min_y = 0.0f, cam->max_y = rows;
        return SVGPU_OK;
    }
    bool wide = false;
    if (cam->model == SVGPU_CAM_FISHEYE) {  // fisheye.cc:76-83 (issue #83): corners beyond 90 degrees
        const double pwx = (0.0 - cam->cx) / cam->fx, pwy = (0.0 - cam->cy) / cam->fy;
        wide = std::sqrt(pwx * pwx + pwy * pwy) > M_PI / 2;
    }
    svgpu_keypoint q[4] = {}, u[4];
    if (wide) {
        q[0].x = (float)cam->cx, q[0].y = 0.f, q[1].x = cols, q[1].y = (float)cam->cy, q[2].x = 0.f, q[2].y = (float)cam->cy, q[3].x = (float)cam->cx, q[3].y = rows;
    }
    else {
        q[0].x = 0.f, q[0].y = 0.f, q[1].x = cols, q[1].y = 0.f, q[2].x = 0.f, q[2].y = rows, q[3].x = cols, q[3].y = rows;
    }
    int rc = svgpu_frame_observation(ctx, cam, q, 4, 1, 1, u, nullptr, nullptr, nullptr);
    if (rc) return rc;
    if (wide) {  // fisheye.cc:98-116
        constexpr float deg_thr = 5.0;
        const float tx = cam->fx / std::tan(deg_thr * M_PI / 180.0), ty = cam->fy / std::tan(deg_thr * M_PI / 180.0);
        const float mnx = -tx + cam->cx, mxx = tx + cam->cx, mny = -ty + cam->cy, mxy = ty + cam->cy;
        const float a = u[2].x, b = u[1].x, c = u[0].y, d = u[3].y;
        cam->min_x = (a < mnx || a > cam->cx) ? mnx : a;
        cam->max_x = (b > mxx || b < cam->cx) ? mxx : b;
        cam->min_y = (c < mny || c > cam->cy) ? mny : c;
        cam->max_y = (d > mxy || d < cam->cy) ? mxy : d;
    }
    else {
        cam->min_x = std::min(u[0].x, u[2].x);
        cam->max_x = std::max(u[1].x, u[3].x);
        cam->min_y = std::min(u[0].y, u[1].y);
        cam->max_y = std::max(u[2].y, u[3].y);
    }
    return SVGPU_OK;
}

int svgpu_frame_observation(svgpu_ctx* ctx, const svgpu_camera* cam, const svgpu_keypoint* kps, int n, int grid_cols,
                            int grid_rows, svgpu_keypoint* undist_kps, double* bearings, int32_t* cell_off, int32_t* cell_items) {
    if (!ctx || !cam || n < 0 || cam->model < SVGPU_CAM_PERSPECTIVE || cam->model > SVGPU_CAM_RADIAL_DIVISION || grid_cols < 1 || grid_rows < 1
        || (size_t)grid_cols * grid_rows > (size_t(1) << 22) || (n > 0 && !kps))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_frame_observation: bad arguments");
    const bool want_grid = cell_off != nullptr;
    if (want_grid && (!(cam->min_x < cam->max_x) || !(cam->min_y < cam->max_y)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_frame_observation: image bounds are not set (svgpu_camera_image_bounds)");
    const int ncell = grid_cols * grid_rows;
    if (n == 0) {
        if (want_grid) std::memset(cell_off, 0, (size_t)(ncell + 1) * sizeof(int32_t));
        return SVGPU_OK;
    }
    FrameObsProblem P{};
    GridProblem G{};
    svgpu_keypoint* d_in;
    StagedCall C;
    int rc = C.open(ctx, "svgpu_frame_observation: internal arena overflow", [&](UploadArena& A) {
        P.kps = d_in = A.take<svgpu_keypoint>(n);
        P.undist = undist_kps ? A.take<svgpu_keypoint>(n) : nullptr;
        P.undist_xy = A.take<float>((size_t)n * 2);
        P.bearings = bearings ? A.take<double>((size_t)n * 3) : nullptr;
        if (want_grid) {
            G.cell_of = A.take<int32_t>(n);
            G.cell_off = A.take<int32_t>(ncell + 1);
            G.cell_items = A.take<int32_t>(n);
            G.cand_off = A.take<int32_t>(1);
        }
    });
    if (rc) return rc;
    hipStream_t s = C.s;
    P.cam = *cam;
    P.n = n;
    C.up(d_in, kps, n);
    if ((rc = C.flush())) return rc;
    sv_launch_frame_observation(s, P);
    C.down(undist_kps, P.undist, n);
    C.down(bearings, P.bearings, 3 * (size_t)n);
    if (want_grid) {
        G.t_xy = P.undist_xy;
        G.nt = n;
        G.min_x = cam->min_x;
        G.min_y = cam->min_y;
        G.inv_w = (double)grid_cols / (cam->max_x - cam->min_x);
        G.inv_h = (double)grid_rows / (cam->max_y - cam->min_y);
        G.cols = grid_cols;
        G.rows = grid_rows;
        G.nq = 0;
        sv_launch_grid_build(s, G);
        C.down(cell_off, G.cell_off, (size_t)ncell + 1);
        if (cell_items) C.keep(G.cell_items, n);  // how many of them count is known only with cell_off: the whole piece comes back
    }
    if ((rc = C.finish())) return rc;
    if (want_grid && cell_items && cell_off[ncell] > 0) std::memcpy(cell_items, C.host(G.cell_items), (size_t)cell_off[ncell] * sizeof(int32_t));
    return SVGPU_OK;
}

int svgpu_keypoints_to_bearings(svgpu_ctx* ctx, const svgpu_camera* cam, const svgpu_keypoint* undist_kps, int n, double* bearings) {
    if (!ctx || !cam || n < 0 || cam->model < SVGPU_CAM_PERSPECTIVE || cam->model > SVGPU_CAM_RADIAL_DIVISION || (n > 0 && (!undist_kps || !bearings)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_keypoints_to_bearings: bad arguments");
    if (n == 0) return SVGPU_OK;
    FrameObsProblem P{};
    svgpu_keypoint* d_in;
    StagedCall C;
    int rc = C.open(ctx, "svgpu_keypoints_to_bearings: internal arena overflow", [&](UploadArena& A) {
        P.kps = d_in = A.take<svgpu_keypoint>(n);
        P.bearings = A.take<double>((size_t)n * 3);
    });
    if (rc) return rc;
    P.cam = *cam;
    P.n = n;
    P.already_undistorted = 1;
    C.up(d_in, undist_kps, n);
    if ((rc = C.flush())) return rc;
    sv_launch_frame_observation(C.s, P);
    C.down(bearings, P.bearings, 3 * (size_t)n);
    return C.finish();
}

}  // extern "C"

namespace {
// Shared argument checks + ReprojProblem fill of the two reprojection entry points (host-side scalars only).
int fill_reproj(svgpu_ctx* ctx, const char* who, ReprojProblem& R, const svgpu_camera* cam, const double* rot_cw, const double* trans_cw,
                const double* trans_wc, int n, const double* pos_w, const double* mean_normal, const float* min_valid_dist,
                const float* max_valid_dist, float ray_cos_thr, int num_levels, float log_scale_factor) {
    if (!ctx || !cam || n < 0 || cam->model < SVGPU_CAM_PERSPECTIVE || cam->model > SVGPU_CAM_RADIAL_DIVISION || !rot_cw || !trans_cw || !trans_wc
        || num_levels < 1 || num_levels > SV_MAX_LEVELS || !(log_scale_factor > 0.f)
        || (n > 0 && (!pos_w || !mean_normal || !min_valid_dist || !max_valid_dist)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    R.cam = *cam;
    std::memcpy(R.rot_cw, rot_cw, sizeof R.rot_cw);
    std::memcpy(R.trans_cw, trans_cw, sizeof R.trans_cw);
    std::memcpy(R.trans_wc, trans_wc, sizeof R.trans_wc);
    R.n = n;
    R.ray_cos_thr = ray_cos_thr;
    R.num_levels = (unsigned)num_levels;
    R.log_scale_factor = log_scale_factor;
    return SVGPU_OK;
}
}  // namespace

extern "C" {

int svgpu_reproject_landmarks(svgpu_ctx* ctx, const svgpu_camera* cam, const double* rot_cw, const double* trans_cw,
                              const double* trans_wc, int n, const double* pos_w, const double* mean_normal,
                              const float* min_valid_dist, const float* max_valid_dist, const uint8_t* skip, float ray_cos_thr,
                              int num_levels, float log_scale_factor, uint8_t* visible, double* reproj, float* x_right,
                              int32_t* pred_scale_level) {
    ReprojProblem R{};
    int rc = fill_reproj(ctx, "svgpu_reproject_landmarks: bad arguments", R, cam, rot_cw, trans_cw, trans_wc, n, pos_w, mean_normal, min_valid_dist,
                         max_valid_dist, ray_cos_thr, num_levels, log_scale_factor);
    if (rc) return rc;
    if (n == 0) return SVGPU_OK;
    if (!visible || !reproj || !x_right || !pred_scale_level) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_reproject_landmarks: null output");
    // one upload and one read-back through the page-locked mirror of the arena (StagedCall): nine separate copies from / to pageable
    // memory were nine staging kernels on the stream
    const ReprojQuery Q{nullptr, pos_w, mean_normal, min_valid_dist, max_valid_dist, skip, nullptr, nullptr, nullptr};
    ReprojPieces Y;
    StagedCall C;
    rc = C.open(ctx, "svgpu_reproject_landmarks: internal arena overflow", [&](UploadArena& A) { reproj_layout(A, (size_t)n, Q, false, Y); });
    if (rc) return rc;
    reproj_bind(Y, R);
    if ((rc = reproj_first(C, Q, Y, R))) return rc;
    reproj_down(C, Y, visible, reproj, x_right, pred_scale_level);
    return C.finish();
}

int svgpu_match_frame_and_landmarks(svgpu_ctx* ctx, const svgpu_camera* cam, const double* rot_cw, const double* trans_cw,
                                    const double* trans_wc, int n, const double* pos_w, const double* mean_normal,
                                    const float* min_valid_dist, const float* max_valid_dist, const uint8_t* skip,
                                    const uint8_t* lm_desc, float ray_cos_thr, int num_levels, const float* scale_factors,
                                    float log_scale_factor, float margin, const uint8_t* tdesc, const float* t_xy,
                                    const int32_t* t_octave, int nt, const uint8_t* occupied, const float* t_xright,
                                    int grid_cols, int grid_rows, unsigned thr, float lowe_ratio, int32_t* match_lm,
                                    int* num_matches, uint8_t* visible, double* reproj, float* x_right,
                                    int32_t* pred_scale_level) {
    ReprojProblem R{};
    const svgpu_frame* rf = sv_take_bound_frame(ctx);
    if (rf) {  // resident keypoint side (svgpu_frame_bind)
        tdesc = rf->desc, t_xy = rf->xy, t_octave = rf->octave, nt = rf->n, grid_cols = rf->grid_cols, grid_rows = rf->grid_rows;
        t_xright = rf->has_xright ? rf->xright : nullptr;
    }
    int rc = fill_reproj(ctx, "svgpu_match_frame_and_landmarks: bad arguments", R, cam, rot_cw, trans_cw, trans_wc, n, pos_w, mean_normal,
                         min_valid_dist, max_valid_dist, ray_cos_thr, num_levels, log_scale_factor);
    if (rc) return rc;
    if (nt < 0 || nt >= (1 << 22) || !num_matches || !scale_factors || grid_cols < 1 || grid_rows < 1 || (size_t)grid_cols * grid_rows > (size_t(1) << 22)
        || !(cam->min_x < cam->max_x) || !(cam->min_y < cam->max_y) || (n > 0 && (!lm_desc || !match_lm)) || (nt > 0 && (!tdesc || !t_xy || !t_octave)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_match_frame_and_landmarks: bad arguments");
    *num_matches = 0;
    if (n == 0) return SVGPU_OK;
    for (int i = 0; i < n; ++i) match_lm[i] = -1;
    if (nt == 0)  // no keypoints: only the observability outputs are meaningful
        return (visible && reproj && x_right && pred_scale_level)
                   ? svgpu_reproject_landmarks(ctx, cam, rot_cw, trans_cw, trans_wc, n, pos_w, mean_normal, min_valid_dist, max_valid_dist, skip,
                                               ray_cos_thr, num_levels, log_scale_factor, visible, reproj, x_right, pred_scale_level)
                   : SVGPU_OK;
    R.margin = margin;
    for (int l = 0; l < num_levels; ++l) R.scale_factors[l] = scale_factors[l];
    InCellsFrame F{tdesc, t_xy, t_octave, nt, occupied, nullptr, t_xright, cam->min_x, cam->max_x, cam->min_y, cam->max_y, grid_cols, grid_rows};
    if (rf) F.min_x = rf->min_x, F.max_x = rf->max_x, F.min_y = rf->min_y, F.max_y = rf->max_y, F.res = rf;
    const ReprojQuery Q{lm_desc, pos_w, mean_normal, min_valid_dist, max_valid_dist, skip, nullptr, nullptr, nullptr};
    ReprojPieces Y;
    return in_cells_core(
        ctx, n, F, 0, thr, lowe_ratio, SVGPU_MATCH_RATIO_SAME_OCTAVE,
        [&](UploadArena& A, CandProblem& P, GridProblem& G) {
            reproj_place(A, Q, Y, R, P, G);
            if (t_xright) {  // projection.cc:57-62: |lm_to_x_right - stereo_x_right| against margin * scale
                P.q_xright = R.x_right;
                P.q_xr_tol = R.q_margin;
            }
        },
        [&](StagedCall& C) { return reproj_first(C, Q, Y, R); },
        [&](StagedCall& C) { reproj_down(C, Y, visible, reproj, x_right, pred_scale_level); }, match_lm, num_matches);
}

int svgpu_stereo_match(svgpu_ctx* ctx_left, svgpu_ctx* ctx_right, const svgpu_keypoint* kps_left, const uint8_t* desc_left,
                       int n_left, const svgpu_keypoint* kps_right, const uint8_t* desc_right, int n_right,
                       float focal_x_baseline, float true_baseline, float* stereo_x_right, float* depths) {
    svgpu_ctx* ctx = ctx_left;
    if (!ctx_left || !ctx_right || n_left < 0 || n_right < 0 || n_right > 65535)
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_stereo_match: bad arguments");
    if (n_left == 0) return SVGPU_OK;
    if (!kps_left || !desc_left || !stereo_x_right || !depths || (n_right > 0 && (!kps_right || !desc_right)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_stereo_match: null pointer");
    const OrbConfig& CL = ctx_left->orb;
    const OrbConfig& CR = ctx_right->orb;
    if (!CL.configured || !CR.configured || ctx_left->last_batch == 0 || ctx_right->last_batch == 0)
        return sv_set_error(ctx, SVGPU_ERR_NOT_CONFIGURED, "svgpu_stereo_match: both contexts need a previous extract call");
    if (ctx_left->device != ctx_right->device || CL.width != CR.width || CL.height != CR.height || CL.num_levels != CR.num_levels
        || CL.scale_factor != CR.scale_factor)
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_stereo_match: the two extractors must share device, geometry and ORB parameters");
    for (int i = 0; i < n_left; ++i) {
        stereo_x_right[i] = -1.0f;
        depths[i] = -1.0f;
        if (kps_left[i].octave < 0 || kps_left[i].octave >= CL.num_levels) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_stereo_match: octave out of range");
    }
    for (int i = 0; i < n_right; ++i)
        if (kps_right[i].octave < 0 || kps_right[i].octave >= CL.num_levels) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_stereo_match: octave out of range");
    if (n_right == 0) return SVGPU_OK;
    SV_HIP(ctx, hipSetDevice(ctx->device));
    SV_HIP(ctx, hipStreamSynchronize(ctx_right->stream));  // the right pyramid must be complete
    const int rows = CL.levels[0].h, rows_per_kp = 2 * (int)std::ceil(2.0 * std::pow((double)CL.scale_factor, CL.num_levels - 1)) + 3;  // rows of the widest band, one to spare
    StereoProblem P{};
    svgpu_keypoint *dkl, *dkr;
    uint32_t *ddl, *ddr;
    StagedCall C;  // staged on the left context
    int rc = C.open(ctx, "svgpu_stereo_match: internal arena overflow", [&](UploadArena& A) {
        dkl = A.take<svgpu_keypoint>(n_left);
        dkr = A.take<svgpu_keypoint>(n_right);
        ddl = A.take<uint32_t>((size_t)n_left * 8);
        ddr = A.take<uint32_t>((size_t)n_right * 8);
        P.xr = A.take<float>(n_left);
        P.depth = A.take<float>(n_left);
        P.corr = A.take<float>(n_left);
        P.row_off = A.take<int32_t>((size_t)rows + 1);
        P.row_fill = A.take<int32_t>(rows);
        P.row_items = A.take<int32_t>((size_t)n_right * rows_per_kp);
    });
    if (rc) return rc;
    P.rows = rows, P.rows_per_kp = rows_per_kp;
    hipStream_t s = C.s;
    C.up(dkl, kps_left, n_left);
    C.up(dkr, kps_right, n_right);
    C.up(ddl, (const uint32_t*)desc_left, (size_t)n_left * 8);
    C.up(ddr, (const uint32_t*)desc_right, (size_t)n_right * 8);
    if ((rc = C.flush())) return rc;
    P.kl = dkl;
    P.kr = dkr;
    P.dl = ddl;
    P.dr = ddr;
    P.nl = n_left;
    P.nr = n_right;
    P.num_levels = CL.num_levels;
    float inv[SV_MAX_LEVELS];
    svgpu_orb_scale_tables(CL.scale_factor, CL.num_levels, P.sf, inv, nullptr, nullptr);
    for (int l = 0; l < CL.num_levels; ++l) {
        P.isf[l] = inv[l];
        P.w[l] = CL.levels[l].w;
        P.h[l] = CL.levels[l].h;
        if (l == 0) {
            P.lev_l[0] = ctx_left->last_imgs;
            P.pitch_l[0] = ctx_left->last_row_stride;
            P.lev_r[0] = ctx_right->last_imgs;
            P.pitch_r[0] = ctx_right->last_row_stride;
        }
        else {
            P.lev_l[l] = ctx_left->d_pyr + CL.levels[l].pyr_off;
            P.pitch_l[l] = CL.levels[l].pitch;
            P.lev_r[l] = ctx_right->d_pyr + CR.levels[l].pyr_off;
            P.pitch_r[l] = CR.levels[l].pitch;
        }
    }
    P.fxb = focal_x_baseline;
    P.min_disp = 0.0f;                                // stereo.cc:18
    P.max_disp = focal_x_baseline / true_baseline;    // stereo.cc:18
    P.thr = 75;                                       // (HAMMING_DIST_THR_HIGH + HAMMING_DIST_THR_LOW) / 2, stereo.h:99
    sv_launch_stereo(ctx, s, P);
    sv_launch_stereo_median(s, P, 1);  // median filter of the correlations (stereo.cc:94-113) on the device
    C.down(stereo_x_right, P.xr, n_left);
    C.down(depths, P.depth, n_left);
    return C.finish();
}

int svgpu_stereo_match_batch_device(svgpu_ctx* ctx_left, svgpu_ctx* ctx_right, int pairs, const svgpu_keypoint* kps_left_dev, const uint8_t* desc_left_dev,
                                    const int32_t* n_left_dev, const svgpu_keypoint* kps_right_dev, const uint8_t* desc_right_dev,
                                    const int32_t* n_right_dev, int cap, int n_stride, float focal_x_baseline, float true_baseline,
                                    float* stereo_x_right_dev, float* depths_dev, void* stream) {
    svgpu_ctx* ctx = ctx_left;
    if (!ctx_left || !ctx_right || pairs < 0 || cap < 0 || cap > 65535 || n_stride < 1 || !(true_baseline > 0.f)
        || (pairs > 0 && cap > 0 && (!kps_left_dev || !desc_left_dev || !n_left_dev || !kps_right_dev || !desc_right_dev || !n_right_dev || !stereo_x_right_dev || !depths_dev)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_stereo_match_batch_device: bad arguments");
    if (pairs == 0 || cap == 0) return SVGPU_OK;
    const OrbConfig& CL = ctx_left->orb;
    const OrbConfig& CR = ctx_right->orb;
    if (!CL.configured || !CR.configured || ctx_left->last_batch < pairs || ctx_right->last_batch < pairs)
        return sv_set_error(ctx, SVGPU_ERR_NOT_CONFIGURED, "svgpu_stereo_match_batch_device: both contexts need a previous batch extraction of >= `pairs` frames");
    if (ctx_left->device != ctx_right->device || CL.width != CR.width || CL.height != CR.height || CL.num_levels != CR.num_levels
        || CL.scale_factor != CR.scale_factor)
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_stereo_match_batch_device: the two extractors must share device, geometry and ORB parameters");
    SV_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const int rows = CL.levels[0].h, rows_per_kp = 2 * (int)std::ceil(2.0 * std::pow((double)CL.scale_factor, CL.num_levels - 1)) + 3;  // rows of the widest band, one to spare
    StereoProblem P{};
    auto layout = [&](Arena& A) {
        P.row_off = A.take<int32_t>((size_t)pairs * (rows + 1));
        P.row_fill = A.take<int32_t>((size_t)pairs * rows);
        P.row_items = A.take<int32_t>((size_t)pairs * cap * rows_per_kp);
        P.corr = A.take<float>((size_t)pairs * cap);
    };
    int rc = sv_scratch_layout(ctx, "svgpu_stereo_match_batch_device: internal arena overflow", layout);
    if (rc) return rc;
    P.rows = rows, P.rows_per_kp = rows_per_kp;
    P.kl = kps_left_dev;
    P.kr = kps_right_dev;
    P.dl = (const uint32_t*)desc_left_dev;
    P.dr = (const uint32_t*)desc_right_dev;
    P.nl_dev = n_left_dev;
    P.nr_dev = n_right_dev;
    P.n_stride = n_stride;
    P.cap = cap;
    P.xr = stereo_x_right_dev;
    P.depth = depths_dev;
    P.num_levels = CL.num_levels;
    float inv[SV_MAX_LEVELS];
    svgpu_orb_scale_tables(CL.scale_factor, CL.num_levels, P.sf, inv, nullptr, nullptr);
    for (int l = 0; l < CL.num_levels; ++l) {
        P.isf[l] = inv[l];
        P.w[l] = CL.levels[l].w;
        P.h[l] = CL.levels[l].h;
        if (l == 0) {
            P.lev_l[0] = ctx_left->last_imgs;
            P.pitch_l[0] = ctx_left->last_row_stride;
            P.lev_r[0] = ctx_right->last_imgs;
            P.pitch_r[0] = ctx_right->last_row_stride;
        }
        else {
            P.lev_l[l] = ctx_left->d_pyr + CL.levels[l].pyr_off;
            P.pitch_l[l] = CL.levels[l].pitch;
            P.lev_r[l] = ctx_right->d_pyr + CR.levels[l].pyr_off;
            P.pitch_r[l] = CR.levels[l].pitch;
        }
    }
    P.img_stride_l = ctx_left->last_frame_stride;
    P.img_stride_r = ctx_right->last_frame_stride;
    P.pyr_stride_l = CL.pyr_frame_bytes;
    P.pyr_stride_r = CR.pyr_frame_bytes;
    P.fxb = focal_x_baseline;
    P.min_disp = 0.0f;
    P.max_disp = focal_x_baseline / true_baseline;
    P.thr = 75;
    sv_launch_stereo(ctx, s, P, pairs);
    sv_launch_stereo_median(s, P, pairs);
    SV_HIP(ctx, hipGetLastError());
    return SVGPU_OK;
}

}  // extern "C"
