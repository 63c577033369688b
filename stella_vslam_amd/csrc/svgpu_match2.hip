// Host side of the function-specific matchers (every match::* method with its own candidate source and gates):
//   projection::match_current_and_last_frames / match_frame_and_keyframe / match_by_Sim3_transform / match_keyframes_mutually
//   fuse::detect_duplication
//   robust::match_for_triangulation, bow_tree::match_for_triangulation / match_frame_and_keyframe / match_keyframes
// Reprojection, grid lookup, pair gates, Hamming distances and the exact greedy replay all run on the device; the host only
// stages the flat arrays and derives the handful of 3x3 quantities each method computes once per call.
#include "svgpu_match_common.h"
#include "bucket_batch_layout.h"
#include "sv_sort.h"

using namespace svm;

namespace {

// keypoint side of a projection-family call: the caller's host arrays, or the resident frame bound with svgpu_frame_bind
InCellsFrame frame_side(const svgpu_frame* rf, const svgpu_camera* cam, const uint8_t* tdesc, const float* t_xy, const int32_t* t_octave, int nt,
                        const uint8_t* occupied, const float* t_angle, const float* t_xright, bool want_angle, bool want_xright, int grid_cols, int grid_rows) {
    if (!rf) return InCellsFrame{tdesc, t_xy, t_octave, nt, occupied, t_angle, t_xright, cam->min_x, cam->max_x, cam->min_y, cam->max_y, grid_cols, grid_rows};
    InCellsFrame F{rf->desc, rf->xy, rf->octave, rf->n, occupied, want_angle ? rf->angle : nullptr, want_xright && rf->has_xright ? rf->xright : nullptr,
                   rf->min_x, rf->max_x, rf->min_y, rf->max_y, rf->grid_cols, rf->grid_rows};
    F.res = rf;
    return F;
}

struct ProjQueries {  // host pointers: the landmarks that get reprojected (= the queries of the cell matcher)
    int n;
    const double* pos_w;           // n x 3
    const double* mean_normal;     // n x 3, nullable with normal_mode 2
    const float* min_valid_dist;   // nullable with q_level
    const float* max_valid_dist;
    const uint8_t* valid;          // nullable: 0 = landmark not offered (null / will_be_erased / already matched ...)
    const int32_t* q_level;        // nullable
    const uint8_t* desc;           // n x 32
    const float* q_angle;          // nullable: keypoint angle on the query side (orientation gate)
    const uint8_t* q_blocks;       // nullable
};
struct ProjOpts {
    int dist_mode, normal_mode, center_mode, window_mode;
    float margin;
    int check_orientation;
    unsigned thr;
    float lowe_ratio;
    int mode;
    int stereo_gate;  // |x_right - stereo_x_right| <= margin * scale for stereo keypoints (projection.cc:57-62, 172-177)
    int chi_gate;     // fuse.cc:92-119
    int no_claims;
    const float* inv_level_sigma_sq;
};

// landmark reprojection -> query windows -> device-built candidate lists -> candidate matcher; match_q[i] = keypoint or -1
int proj_match(svgpu_ctx* ctx, const char* who, const svgpu_camera* cam, const double* rot_cw, const double* trans_cw, const double* trans_wc,
               const ProjQueries& Q, int num_levels, const float* scale_factors, float log_scale_factor, const InCellsFrame& F, const ProjOpts& O,
               int32_t* match_q, int* num_matches, uint8_t* visible, double* reproj, float* x_right, int32_t* pred_level) {
    const int n = Q.n, nt = F.nt;
    if (!ctx || !cam || n < 0 || cam->model < SVGPU_CAM_PERSPECTIVE || cam->model > SVGPU_CAM_RADIAL_DIVISION || !rot_cw || !trans_cw || !trans_wc
        || num_levels < 1 || num_levels > SV_MAX_LEVELS || !scale_factors || (!Q.q_level && !(log_scale_factor > 0.f)) || !num_matches
        || nt < 0 || nt >= (1 << 22) || F.grid_cols < 1 || F.grid_rows < 1 || (size_t)F.grid_cols * F.grid_rows > (size_t(1) << 22)
        || !(F.min_x < F.max_x) || !(F.min_y < F.max_y)
        || (n > 0 && (!Q.pos_w || !Q.desc || !match_q || (O.normal_mode != 2 && !Q.mean_normal) || (!Q.q_level && (!Q.min_valid_dist || !Q.max_valid_dist))
                      || (O.check_orientation && !Q.q_angle)))
        || (nt > 0 && (!F.tdesc || !F.t_xy || !F.t_octave || (O.check_orientation && !F.t_angle))) || (O.chi_gate && !O.inv_level_sigma_sq))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    *num_matches = 0;
    if (n == 0) return SVGPU_OK;
    for (int i = 0; i < n; ++i) match_q[i] = -1;
    if (nt == 0) return SVGPU_OK;
    ReprojProblem R{};
    R.cam = *cam;
    std::memcpy(R.rot_cw, rot_cw, sizeof R.rot_cw);
    std::memcpy(R.trans_cw, trans_cw, sizeof R.trans_cw);
    std::memcpy(R.trans_wc, trans_wc, sizeof R.trans_wc);
    R.n = n;
    R.ray_cos_thr = 0.5f;
    R.num_levels = (unsigned)num_levels;
    R.log_scale_factor = log_scale_factor;
    R.margin = O.margin;
    for (int l = 0; l < num_levels; ++l) R.scale_factors[l] = scale_factors[l];
    R.dist_mode = O.dist_mode;
    R.normal_mode = O.normal_mode;
    R.center_mode = O.center_mode;
    R.window_mode = O.window_mode;
    std::vector<uint8_t> skip;
    if (Q.valid) {
        skip.resize(n);
        for (int i = 0; i < n; ++i) skip[i] = Q.valid[i] ? 0 : 1;
    }
    InCellsFrame Fq = F;
    if (!O.stereo_gate && !O.chi_gate) Fq.t_xright = nullptr;
    const ReprojQuery RQ{Q.desc, Q.pos_w, Q.mean_normal, Q.min_valid_dist, Q.max_valid_dist, Q.valid ? skip.data() : nullptr, Q.q_level, Q.q_angle, Q.q_blocks};
    ReprojPieces Y;
    return in_cells_core(
        ctx, n, Fq, O.check_orientation, O.thr, O.lowe_ratio, O.mode,
        [&](UploadArena& A, CandProblem& P, GridProblem& G) {
            reproj_place(A, RQ, Y, R, P, G);
            P.no_claims = O.no_claims;
            if (O.stereo_gate && F.t_xright) {
                P.q_xright = R.x_right;
                P.q_xr_tol = R.q_margin;
            }
            if (O.chi_gate) {
                P.chi_gate = 1;
                P.q_reproj = R.reproj;
                P.q_reproj_xr = R.x_right;
                for (int l = 0; l < num_levels; ++l) P.inv_level_sigma_sq[l] = O.inv_level_sigma_sq[l];
            }
        },
        [&](StagedCall& C) { return reproj_first(C, RQ, Y, R); },
        [&](StagedCall& C) { reproj_down(C, Y, visible, reproj, x_right, pred_level); }, match_q, num_matches);
}

// -R^T t and R v + t as the reference writes them (Eigen 3-vectors: ((a0 b0 + a1 b1) + a2 b2); compiled without contraction)
inline void cam_center(const double* R, const double* t, double* c) {
    for (int i = 0; i < 3; ++i) c[i] = ((-R[i]) * t[0] + (-R[3 + i]) * t[1]) + (-R[6 + i]) * t[2];
}
inline void mat_vec(const double* M, const double* v, double* o) {
    for (int i = 0; i < 3; ++i) o[i] = (M[3 * i] * v[0] + M[3 * i + 1] * v[1]) + M[3 * i + 2] * v[2];
}
inline void mat_mul(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

// bucketed candidate lists (bucket_kernels.hip) + candidate matcher; match_1to2[i] = side-2 keypoint or -1
int bucket_match(svgpu_ctx* ctx, const char* who, const BucketSide& S1, const BucketSide& S2, const uint8_t* occupied2, int tri, const double* E12,
                 const double* epipole, int valid_epipole, const float* scale_factors, int num_levels, float residual_rad_thr, unsigned thr,
                 float lowe_ratio, int check_orientation, int mode, int32_t* match_1to2, int* num_matches) {
    const int n1 = S1.n, n2 = S2.n;
    if (!ctx || n1 < 0 || n2 < 0 || n2 >= (1 << 22) || !num_matches || (n1 > 0 && (!S1.desc || !match_1to2)) || (n2 > 0 && !S2.desc)
        || ((S1.node == nullptr) != (S2.node == nullptr)) || (check_orientation && ((n1 > 0 && !S1.angle) || (n2 > 0 && !S2.angle)))
        || (tri && (!E12 || !epipole || !scale_factors || num_levels < 1 || num_levels > 16 || (n1 > 0 && (!S1.bearings || !S1.octave)) || (n2 > 0 && !S2.bearings))))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    *num_matches = 0;
    for (int i = 0; i < n1; ++i) match_1to2[i] = -1;
    if (n1 == 0 || n2 == 0) return SVGPU_OK;
    if (tri)
        for (int i = 0; i < n1; ++i)
            if (S1.octave[i] < 0 || S1.octave[i] >= num_levels) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    const size_t sortb = std::max(sv_bucket_sort_bytes(n1), sv_bucket_sort_bytes(n2));
    BucketPieces Y;
    BucketProblem B;
    CandProblem P;
    bool lists = false;
    int32_t total = 0, num = 0;
    auto layout = [&](UploadArena& A) {
        bucket_layout(A, S1, S2, occupied2, sortb, lists, (size_t)total, Y);
        B = BucketProblem{};
        B.n1 = n1, B.n2 = n2, B.check_orientation = check_orientation, B.tri = tri, B.thr = thr;
        B.desc1 = (const uint32_t*)Y.desc1.p, B.desc2 = (const uint32_t*)Y.desc2.p;
        B.angle1 = Y.angle1, B.angle2 = Y.angle2, B.valid1 = Y.valid1, B.valid2 = Y.valid2;
        B.octave1 = Y.octave1, B.bearings1 = Y.bearings1, B.bearings2 = Y.bearings2, B.xright1 = Y.xright1, B.xright2 = Y.xright2;
        if (tri) {
            std::memcpy(B.E12, E12, sizeof B.E12);
            std::memcpy(B.epipole, epipole, sizeof B.epipole);
            B.valid_epipole = valid_epipole;
            for (int l = 0; l < num_levels; ++l) B.scale_factors[l] = scale_factors[l];
            B.residual_rad_thr = residual_rad_thr;
        }
        B.key1 = Y.key1, B.q_idx = Y.q_idx, B.key2 = Y.key2, B.t_sorted = Y.t_sorted, B.row_lo = Y.row_lo, B.row_hi = Y.row_hi;
        P = CandProblem{};
        P.q_valid = B.q_valid = Y.q_valid, P.cand_off = B.cand_off = Y.cand_off, P.cand_idx = B.cand_idx = Y.cand_idx;
        P.qdesc = Y.qdesc_rows, P.tdesc = B.desc2, P.nq = n1, P.nt = n2, P.occupied = Y.occupied2;
        P.check_orientation = 0;  // gated in the scan
        P.thr = thr, P.lowe_ratio = lowe_ratio, P.mode = mode;
        P.dist = Y.dist, P.match_q = Y.match_rows, P.num = Y.num;
    };
    StagedCall C;
    auto count = [&]() -> int {  // uploads, sorts, rows and the candidate count: pass 0, and again if the arena regrew for the lists
        C.up(Y.desc1, S1.desc, Y.desc2, S2.desc, Y.angle1, S1.angle, Y.angle2, S2.angle, Y.valid1, S1.valid, Y.valid2, S2.valid);
        C.up(Y.node1, S1.node, Y.node2, S2.node, Y.octave1, S1.octave, Y.bearings1, S1.bearings, Y.bearings2, S2.bearings);
        C.up(Y.xright1, S1.xright, Y.xright2, S2.xright, Y.occupied2, occupied2);
        int r = C.flush();
        if (!r) r = sv_bucket_sort(ctx, C.s, Y.node1, n1, Y.sort_scratch, sortb, Y.key1, Y.q_idx);
        if (!r) r = sv_bucket_sort(ctx, C.s, Y.node2, n2, Y.sort_scratch, sortb, Y.key2, Y.t_sorted);
        if (r) return r;
        sv_bucket_rows(C.s, B);
        sv_bucket_count(C.s, B);
        return SVGPU_OK;
    };
    // The two passes, always sized exactly (no guess), and no page-locked mirror, on purpose: every array is a copy of its own and the
    // results come straight to the caller's arrays.  The second pass reuses the arena of the first unless it regrew (prefix invariant).
    int rc = C.open(ctx, "bucket matcher: internal arena overflow", layout, false);
    if (!rc) rc = count();
    if (!rc) rc = C.read_now(&total, B.cand_off + n1);
    if (rc || total == 0) return rc;
    bool survived = false;
    lists = true;
    if ((rc = C.reopen(layout, survived))) return rc;
    if (!survived && (rc = count())) return rc;
    sv_bucket_fill(C.s, B);
    sv_bucket_gather_rows(C.s, B, Y.qdesc_rows, Y.qangle_rows);
    sv_launch_cand(ctx, C.s, P, Y.owner, Y.match_of_row, Y.mdist);
    SV_HIP(ctx, hipMemsetAsync(Y.match, 0xFF, (size_t)n1 * 4, C.s));
    sv_bucket_scatter(C.s, B, Y.match_rows, Y.match);
    C.down(match_1to2, Y.match);
    C.down(&num, Y.num);
    if ((rc = C.finish())) return rc;
    *num_matches = num;
    return SVGPU_OK;
}


// K problems of the bucket matcher in one staged call (svgpu_bow_match_batch, svgpu_match_for_triangulation_batch): the same two passes
// as bucket_match over the concatenation of all problems' rows.  A shared side is uploaded, ordered and (side 1) gathered once; every
// kernel finds its problem's record in a table in device memory, and the replay runs one workgroup per problem.  Problem p's result
// is what bucket_match returns for its two sides: its rows, buckets, lists, owner table and matches are its own.
int bucket_match_batch(svgpu_ctx* ctx, const char* who, int K, const svgpu_match_view* side1, int shared1, const svgpu_match_view* side2, int shared2, int tri,
                       const double* E12, const double* epipole, const int32_t* valid_epipole, const float* scale_factors, int num_levels,
                       float residual_rad_thr, unsigned thr, float lowe_ratio, int check_orientation, int mode, int32_t* match_1to2, int32_t* num_matches) {
    if (!ctx || K < 0) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    if (K == 0) return SVGPU_OK;
    if (!side1 || !side2 || !num_matches || (shared1 && shared2 && K > 1)
        || (tri && (!E12 || !epipole || !valid_epipole || !scale_factors || num_levels < 1 || num_levels > 16)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    BucketBatchShape S;
    S.num_problems = K, S.shared1 = shared1 != 0, S.shared2 = shared2 != 0;
    const size_t U1 = shared1 ? 1 : (size_t)K, U2 = shared2 ? 1 : (size_t)K;
    size_t N1 = 0, N2 = 0, R = 0, pairs = 0;
    for (size_t u = 0; u < U1; ++u) {
        const svgpu_match_view& v = side1[u];
        if (v.n < 0 || v.occupied || (v.n > 0 && (!v.desc || (check_orientation && !v.angle) || (tri && (!v.bearings || !v.octave)))))
            return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
        if (tri)
            for (int i = 0; i < v.n; ++i)
                if (v.octave[i] < 0 || v.octave[i] >= num_levels) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
        S.side1.push_back(BucketSide{v.desc, v.angle, v.valid, v.node, tri ? v.octave : nullptr, tri ? v.bearings : nullptr, tri ? v.xright : nullptr, v.n});
        N1 += (size_t)v.n;
    }
    for (size_t u = 0; u < U2; ++u) {
        const svgpu_match_view& v = side2[u];
        if (v.n < 0 || v.n >= (1 << 22) || (tri && v.occupied) || (v.n > 0 && (!v.desc || (check_orientation && !v.angle) || (tri && !v.bearings))))
            return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
        S.side2.push_back(BucketSide{v.desc, v.angle, v.valid, v.node, nullptr, tri ? v.bearings : nullptr, tri ? v.xright : nullptr, v.n});
        S.occupied2.push_back(v.occupied);
        N2 += (size_t)v.n;
    }
    bool work = false;
    for (int p = 0; p < K; ++p) {
        const BucketSide &a = S.s1(p), &b = S.s2(p);
        if ((a.node == nullptr) != (b.node == nullptr)) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
        R += (size_t)a.n;
        pairs += (size_t)a.n * (size_t)b.n;  // (no list can hold more than its bucket: the lists' total stays below this)
        work = work || (a.n > 0 && b.n > 0);
    }
    const size_t lim = (size_t)INT32_MAX;
    if (R + (size_t)K > lim || N1 * 8 > lim || N2 * 8 > lim || pairs > lim || (R > 0 && !match_1to2))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    for (int p = 0; p < K; ++p) num_matches[p] = 0;
    for (size_t i = 0; i < R; ++i) match_1to2[i] = -1;
    if (!work) return SVGPU_OK;

    // the form of every problem's replay (sv_cand_replay_form decides), and the dynamic LDS of the one launch
    std::vector<int> form((size_t)K);
    S.global_form.assign((size_t)K, 0);
    size_t lds_bytes = 0;
    int max_small = 0;
    for (int p = 0; p < K; ++p) {
        const int n1 = S.s1(p).n, n2 = S.s2(p).n;
        form[p] = sv_cand_replay_form(n1, n2, false, mode);
        if (form[p] < 0) S.global_form[p] = 1;
        else lds_bytes = std::max(lds_bytes, sv_cand_lds_bytes(n1, n2, form[p]));
    }
    for (const std::vector<BucketSide>* L : {&S.side1, &S.side2})
        for (const BucketSide& b : *L) {
            S.sortb = std::max(S.sortb, sv_bucket_sort_bytes(b.n));
            if (b.n <= SV_SORT_SMALL_MAX) max_small = std::max(max_small, b.n);
        }
    S.scan_ints = sv_scan_scratch_ints(R);
    S.side_rec = sizeof(SvSortSide), S.gather_rec = sizeof(BucketBatchSide), S.bucket_rec = sizeof(BucketProblem), S.cand_rec = sizeof(CandProblem);
    S.replay_rec = sizeof(CandBatchReplay);

    BucketBatchPieces Y;
    std::vector<SvSortSide> sort_tab(U1 + U2);
    std::vector<BucketBatchSide> gather_tab(U1);
    std::vector<BucketProblem> bucket_tab((size_t)K);
    std::vector<CandProblem> cand_tab((size_t)K);
    std::vector<CandBatchReplay> replay_tab((size_t)K);
    std::vector<int32_t> row_base((size_t)K + 1), side1_base(U1 + 1);
    bool lists = false;
    int32_t total = 0;
    auto layout = [&](UploadArena& A) {
        bucket_batch_layout(A, S, lists, (size_t)total, Y);
        for (size_t u = 0; u < U1; ++u) {
            const BucketSidePlace& a = Y.at1[u];
            sort_tab[u] = SvSortSide{a.node, S.side1[u].n, a.key, a.order};
            gather_tab[u] = BucketBatchSide{(const uint32_t*)a.desc, a.order, a.desc_rows};
            side1_base[u] = (int32_t)a.first;
        }
        side1_base[U1] = (int32_t)N1;
        for (size_t u = 0; u < U2; ++u) sort_tab[U1 + u] = SvSortSide{Y.at2[u].node, S.side2[u].n, Y.at2[u].key, Y.at2[u].order};
        for (int p = 0; p < K; ++p) {
            const BucketSidePlace &a = Y.at1[shared1 ? 0 : p], &b = Y.at2[shared2 ? 0 : p];
            const size_t r0 = Y.row_first[p];
            row_base[p] = (int32_t)r0;
            BucketProblem& B = bucket_tab[p];
            B = BucketProblem{};
            B.n1 = S.s1(p).n, B.n2 = S.s2(p).n, B.check_orientation = check_orientation, B.tri = tri, B.thr = thr;
            B.desc1 = (const uint32_t*)a.desc, B.desc2 = (const uint32_t*)b.desc;
            B.angle1 = a.angle, B.angle2 = b.angle, B.valid1 = a.valid, B.valid2 = b.valid;
            B.octave1 = a.octave, B.bearings1 = a.bearings, B.bearings2 = b.bearings, B.xright1 = a.xright, B.xright2 = b.xright;
            if (tri) {
                std::memcpy(B.E12, E12 + 9 * (size_t)p, sizeof B.E12);
                std::memcpy(B.epipole, epipole + 3 * (size_t)p, sizeof B.epipole);
                B.valid_epipole = valid_epipole[p];
                for (int l = 0; l < num_levels; ++l) B.scale_factors[l] = scale_factors[l];
                B.residual_rad_thr = residual_rad_thr;
            }
            B.key1 = a.key, B.q_idx = a.order, B.key2 = b.key, B.t_sorted = b.order;
            // (the per-problem arrays: rows r0 .. of the concatenations; cand_off holds offsets into the ONE pair of lists, so a problem's
            //  n1 + 1 entries end where the next problem's begin)
            B.row_lo = Y.row_lo.p ? Y.row_lo.p + r0 : nullptr, B.row_hi = Y.row_hi.p ? Y.row_hi.p + r0 : nullptr;
            B.q_valid = Y.q_valid.p ? Y.q_valid.p + r0 : nullptr, B.cand_off = Y.cand_off.p ? Y.cand_off.p + r0 : nullptr, B.cand_idx = Y.cand_idx;
            CandProblem& P = cand_tab[p];
            P = CandProblem{};
            P.q_valid = B.q_valid, P.cand_off = B.cand_off, P.cand_idx = B.cand_idx;
            P.qdesc = a.desc_rows, P.tdesc = B.desc2, P.nq = B.n1, P.nt = B.n2, P.occupied = b.occupied;
            P.check_orientation = 0;  // gated in the scan
            P.thr = thr, P.lowe_ratio = lowe_ratio, P.mode = mode;
            P.dist = Y.dist, P.match_q = Y.match_rows.p ? Y.match_rows.p + r0 : nullptr, P.num = Y.num.p ? Y.num.p + p : nullptr;
            replay_tab[p] = CandBatchReplay{form[p], form[p] < 0 && Y.owner.p ? Y.owner.p + Y.owner_first[p] : nullptr,
                                            form[p] < 0 && Y.match_of_row.p ? Y.match_of_row.p + Y.mrow_first[p] : nullptr};
        }
        row_base[K] = (int32_t)R;
    };
    StagedCall C;
    auto tables = [&]() {  // (after every layout: the records hold arena addresses)
        C.up(Y.side_tab, (const char*)sort_tab.data(), Y.gather_tab, (const char*)gather_tab.data(), Y.bucket_tab, (const char*)bucket_tab.data());
        C.up(Y.cand_tab, (const char*)cand_tab.data(), Y.replay_tab, (const char*)replay_tab.data());
        C.up(Y.row_base, row_base.data(), Y.side1_base, side1_base.data());
    };
    auto count = [&]() -> int {  // uploads, orders, rows and the candidate count of all problems: pass 0, and again if the arena regrew for the lists
        for (size_t u = 0; u < U1; ++u) {
            const BucketSide& h = S.side1[u];
            const BucketSidePlace& a = Y.at1[u];
            const size_t n = (size_t)h.n;
            C.up(a.desc, h.desc, n * 32), C.up(a.angle, h.angle, n), C.up(a.valid, h.valid, n), C.up(a.node, h.node, n);
            C.up(a.octave, h.octave, n), C.up(a.bearings, h.bearings, n * 3), C.up(a.xright, h.xright, n);
        }
        for (size_t u = 0; u < U2; ++u) {
            const BucketSide& h = S.side2[u];
            const BucketSidePlace& b = Y.at2[u];
            const size_t n = (size_t)h.n;
            C.up(b.desc, h.desc, n * 32), C.up(b.angle, h.angle, n), C.up(b.valid, h.valid, n), C.up(b.node, h.node, n);
            C.up(b.bearings, h.bearings, n * 3), C.up(b.xright, h.xright, n), C.up(b.occupied, S.occupied2[u], n);
        }
        tables();
        int r = C.flush();
        if (r) return r;
        SvProfScope ps(ctx, C.s, "k_bucket_batch");
        // every side of at most SV_SORT_SMALL_MAX keypoints in one launch, a workgroup each; longer ones one after another by the general sort
        const bool small = sv_sort_small_sides(C.s, (const SvSortSide*)Y.side_tab.p, (int)(U1 + U2), max_small);
        for (size_t u = 0; u < U1 + U2 && !r; ++u)
            if (!small || sort_tab[u].n > SV_SORT_SMALL_MAX)
                r = sv_bucket_sort(ctx, C.s, sort_tab[u].node, sort_tab[u].n, Y.sort_scratch, S.sortb, sort_tab[u].keys_out, sort_tab[u].idx_out);
        if (r) return r;
        sv_bucket_batch_rows_count(ctx, C.s, (const BucketProblem*)Y.bucket_tab.p, Y.row_base, K, (int)R, Y.cand_off, Y.scan_scratch);
        return SVGPU_OK;
    };
    int rc = C.open(ctx, "bucket matcher batch: internal arena overflow", layout, false);
    if (!rc) rc = count();
    if (!rc) rc = C.read_now(&total, Y.cand_off.p + R);
    if (rc || total == 0) return rc;
    if (total < 0) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    bool survived = false;
    lists = true;
    if ((rc = C.reopen(layout, survived))) return rc;
    if (!survived) {
        if ((rc = count())) return rc;
    }
    else {
        tables();  // the records now name the lists
        if ((rc = C.flush())) return rc;
    }
    {
        SvProfScope ps(ctx, C.s, "k_bucket_batch");
        sv_bucket_batch_fill(C.s, (const BucketProblem*)Y.bucket_tab.p, Y.row_base, K, (int)R);
        sv_bucket_batch_gather(C.s, (const BucketBatchSide*)Y.gather_tab.p, Y.side1_base, (int)U1, (int)N1);
    }
    sv_launch_cand_batch(ctx, C.s, (const CandProblem*)Y.cand_tab.p, (const CandBatchReplay*)Y.replay_tab.p, Y.row_base, K, (int)R, lds_bytes);
    {  // (no memset of Y.match: a problem's rows are a permutation of its keypoints, the scatter writes all R entries)
        SvProfScope ps(ctx, C.s, "k_bucket_batch");
        sv_bucket_batch_scatter(C.s, (const BucketProblem*)Y.bucket_tab.p, Y.row_base, K, (int)R, Y.match_rows, Y.match);
    }
    C.down(match_1to2, Y.match);
    C.down(num_matches, Y.num);
    return C.finish();
}

}  // namespace

extern "C" {

int svgpu_bow_match_batch(svgpu_ctx* ctx, int num_problems, const svgpu_match_view* side1, int side1_shared, const svgpu_match_view* side2, int side2_shared,
                          float lowe_ratio, int check_orientation, int32_t* match_1to2, int32_t* num_matches) {
    const char* who = "svgpu_bow_match_batch: bad arguments";
    if (num_problems > 0 && side1 && side2)  // node ids are required, as in svgpu_bow_match
        for (int u = 0; u < (side1_shared ? 1 : num_problems); ++u)
            if (!side1[u].node) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_bow_match_batch: node ids are required");
    return bucket_match_batch(ctx, who, num_problems, side1, side1_shared, side2, side2_shared, 0, nullptr, nullptr, nullptr, nullptr, 0, 0.f, 50u, lowe_ratio,
                              check_orientation, SVGPU_MATCH_RATIO, match_1to2, num_matches);
}

int svgpu_match_for_triangulation_batch(svgpu_ctx* ctx, int num_problems, const svgpu_match_view* side1, int side1_shared, const svgpu_match_view* side2,
                                        int side2_shared, const double* E_12, const double* epipole_in_2, const int32_t* valid_epipole,
                                        const float* scale_factors, int num_levels, float residual_rad_thr, float lowe_ratio, int check_orientation,
                                        int32_t* matched_2_in_1, int32_t* num_matches) {
    return bucket_match_batch(ctx, "svgpu_match_for_triangulation_batch: bad arguments", num_problems, side1, side1_shared, side2, side2_shared, 1, E_12,
                              epipole_in_2, valid_epipole, scale_factors, num_levels, residual_rad_thr, 50u, lowe_ratio, check_orientation,
                              SVGPU_MATCH_TRIANGULATION, matched_2_in_1, num_matches);
}

int svgpu_reproject_to_bearing(const svgpu_camera* cam, const double* rot_cw, const double* trans_cw, const double* pos_w, double* bearing, int* valid) {
    if (!cam || !rot_cw || !trans_cw || !pos_w || !bearing || !valid) return SVGPU_ERR_INVALID;
    double p[3];
    for (int i = 0; i < 3; ++i) p[i] = ((rot_cw[3 * i] * pos_w[0] + rot_cw[3 * i + 1] * pos_w[1]) + rot_cw[3 * i + 2] * pos_w[2]) + trans_cw[i];
    auto normalize = [&]() {
        const double nrm = std::sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
        for (int i = 0; i < 3; ++i) bearing[i] = p[i] / nrm;
    };
    if (cam->model == SVGPU_CAM_EQUIRECTANGULAR) {  // equirectangular.cc:75-80
        normalize();
        *valid = 1;
        return SVGPU_OK;
    }
    if (p[2] <= 0.0) {  // perspective.cc:155-157: the un-normalised camera-frame point is what the caller is left with
        for (int i = 0; i < 3; ++i) bearing[i] = p[i];
        *valid = 0;
        return SVGPU_OK;
    }
    const double z_inv = 1.0 / p[2];
    const double x = cam->fx * p[0] * z_inv + cam->cx, y = cam->fy * p[1] * z_inv + cam->cy;
    if (cam->model == SVGPU_CAM_RADIAL_DIVISION) {  // radial_division.cc:146-155: inclusive bounds, normalised only when inside
        if (x < cam->min_x || x > cam->max_x || y < cam->min_y || y > cam->max_y) {
            for (int i = 0; i < 3; ++i) bearing[i] = p[i];
            *valid = 0;
            return SVGPU_OK;
        }
        normalize();
        *valid = 1;
        return SVGPU_OK;
    }
    normalize();  // perspective.cc:165-169, fisheye.cc:204-208
    *valid = (cam->min_x < x && x < cam->max_x && cam->min_y < y && y < cam->max_y) ? 1 : 0;
    return SVGPU_OK;
}

int svgpu_match_current_and_last_frames(svgpu_ctx* ctx, const svgpu_camera* cam, const double* rot_cw, const double* trans_cw, const double* rot_lw,
                                        const double* trans_lw, int is_monocular, float true_baseline, int n_last, const double* pos_w,
                                        const uint8_t* valid, const uint8_t* lm_desc, const int32_t* octave_last, const float* angle_last,
                                        const uint8_t* lm_has_observation, int num_levels, const float* scale_factors, float margin,
                                        const uint8_t* tdesc, const float* t_xy, const int32_t* t_octave, const float* t_angle, int nt,
                                        const uint8_t* occupied, const float* t_xright, int grid_cols, int grid_rows, int check_orientation,
                                        int32_t* match_last, int* num_matches) {
    const svgpu_frame* const bound = sv_take_bound_frame(ctx);  // one-shot: consumed before anything can fail
    if (!ctx || !cam || !rot_cw || !trans_cw || !rot_lw || !trans_lw || (n_last > 0 && !octave_last))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_match_current_and_last_frames: bad arguments");
    for (int i = 0; i < n_last; ++i)
        if (octave_last[i] < 0 || octave_last[i] >= num_levels) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_match_current_and_last_frames: octave out of range");
    double trans_wc[3], trans_lc[3];
    cam_center(rot_cw, trans_cw, trans_wc);            // projection.cc:101
    mat_vec(rot_lw, trans_wc, trans_lc);               // :106
    for (int i = 0; i < 3; ++i) trans_lc[i] += trans_lw[i];
    const bool fwd = is_monocular ? false : trans_lc[2] > (double)true_baseline;    // :110-116
    const bool bwd = is_monocular ? false : -trans_lc[2] > (double)true_baseline;
    ProjQueries Q{n_last, pos_w, nullptr, nullptr, nullptr, valid, octave_last, lm_desc, angle_last, lm_has_observation};
    ProjOpts O{2, 2, 0, fwd ? 1 : (bwd ? 2 : 0), margin, check_orientation, 100u, 0.f, SVGPU_MATCH_BEST_ONLY, 1, 0, 0, nullptr};
    const InCellsFrame F = frame_side(bound, cam, tdesc, t_xy, t_octave, nt, occupied, t_angle, t_xright, true, true, grid_cols, grid_rows);
    return proj_match(ctx, "svgpu_match_current_and_last_frames: bad arguments", cam, rot_cw, trans_cw, trans_wc, Q, num_levels, scale_factors, 1.f, F, O,
                      match_last, num_matches, nullptr, nullptr, nullptr, nullptr);
}

int svgpu_match_frame_and_keyframe_projection(svgpu_ctx* ctx, const svgpu_camera* cam, const double* rot_cw, const double* trans_cw, int n_kf,
                                              const double* pos_w, const uint8_t* valid, const float* min_valid_dist, const float* max_valid_dist,
                                              const uint8_t* lm_desc, const float* angle_kf, int num_levels, const float* scale_factors,
                                              float log_scale_factor, float margin, unsigned hamm_dist_thr, const uint8_t* tdesc, const float* t_xy,
                                              const int32_t* t_octave, const float* t_angle, int nt, const uint8_t* occupied, int grid_cols,
                                              int grid_rows, int check_orientation, int32_t* match_kf, int* num_matches) {
    const svgpu_frame* const bound = sv_take_bound_frame(ctx);  // one-shot: consumed before anything can fail
    if (!ctx || !cam || !rot_cw || !trans_cw) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_match_frame_and_keyframe_projection: bad arguments");
    double center[3];
    cam_center(rot_cw, trans_cw, center);  // projection.cc:223
    ProjQueries Q{n_kf, pos_w, nullptr, min_valid_dist, max_valid_dist, valid, nullptr, lm_desc, angle_kf, nullptr};
    ProjOpts O{1, 2, 0, 0, margin, check_orientation, hamm_dist_thr, 0.f, SVGPU_MATCH_BEST_ONLY, 0, 0, 0, nullptr};
    const InCellsFrame F = frame_side(bound, cam, tdesc, t_xy, t_octave, nt, occupied, t_angle, nullptr, true, false, grid_cols, grid_rows);
    return proj_match(ctx, "svgpu_match_frame_and_keyframe_projection: bad arguments", cam, rot_cw, trans_cw, center, Q, num_levels, scale_factors,
                      log_scale_factor, F, O, match_kf, num_matches, nullptr, nullptr, nullptr, nullptr);
}

int svgpu_match_by_sim3_transform(svgpu_ctx* ctx, const svgpu_camera* cam, const double* sim3_cw, int n, const double* pos_w, const uint8_t* valid,
                                  const float* min_valid_dist, const float* max_valid_dist, const double* mean_normal, const uint8_t* lm_desc,
                                  int num_levels, const float* scale_factors, float log_scale_factor, float margin, const uint8_t* tdesc,
                                  const float* t_xy, const int32_t* t_octave, int nt, const uint8_t* occupied, int grid_cols, int grid_rows,
                                  int32_t* match_lm, int* num_matches) {
    const svgpu_frame* const bound = sv_take_bound_frame(ctx);  // one-shot: consumed before anything can fail
    if (!ctx || !cam || !sim3_cw) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_match_by_sim3_transform: bad arguments");
    // Sim3 -> SE3, projection.cc:326-330
    const double s_cw = std::sqrt((sim3_cw[0] * sim3_cw[0] + sim3_cw[1] * sim3_cw[1]) + sim3_cw[2] * sim3_cw[2]);
    double rot[9], trans[3], center[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) rot[3 * i + j] = sim3_cw[4 * i + j] / s_cw;
        trans[i] = sim3_cw[4 * i + 3] / s_cw;
    }
    cam_center(rot, trans, center);
    ProjQueries Q{n, pos_w, mean_normal, min_valid_dist, max_valid_dist, valid, nullptr, lm_desc, nullptr, nullptr};
    ProjOpts O{1, 1, 0, 0, margin, 0, 50u, 0.f, SVGPU_MATCH_BEST_ONLY, 0, 0, 0, nullptr};
    const InCellsFrame F = frame_side(bound, cam, tdesc, t_xy, t_octave, nt, occupied, nullptr, nullptr, false, false, grid_cols, grid_rows);
    return proj_match(ctx, "svgpu_match_by_sim3_transform: bad arguments", cam, rot, trans, center, Q, num_levels, scale_factors, log_scale_factor, F, O,
                      match_lm, num_matches, nullptr, nullptr, nullptr, nullptr);
}

int svgpu_match_keyframes_mutually(svgpu_ctx* ctx, const svgpu_camera* cam1, const svgpu_camera* cam2, const double* rot_1w, const double* trans_1w,
                                   const double* rot_2w, const double* trans_2w, float s_12, const double* rot_12, const double* trans_12,
                                   int n1, const double* pos_w1, const uint8_t* valid1, const float* min_valid1, const float* max_valid1,
                                   const uint8_t* lm_desc1, const uint8_t* desc1, const float* xy1, const int32_t* octave1,
                                   int n2, const double* pos_w2, const uint8_t* valid2, const float* min_valid2, const float* max_valid2,
                                   const uint8_t* lm_desc2, const uint8_t* desc2, const float* xy2, const int32_t* octave2,
                                   int num_levels, const float* scale_factors, float log_scale_factor, float margin, int grid_cols, int grid_rows,
                                   int32_t* matched_2_in_1, int32_t* matched_1_in_2, int32_t* mutual_2_in_1, int* num_matches) {
    if (!ctx || !cam1 || !cam2 || !rot_1w || !trans_1w || !rot_2w || !trans_2w || !rot_12 || !trans_12 || !num_matches
        || (n1 > 0 && (!matched_2_in_1 || !mutual_2_in_1)) || (n2 > 0 && !matched_1_in_2))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_match_keyframes_mutually: bad arguments");
    // similarity between the keyframes, projection.cc:428-431
    double s_rot_12[9], s_rot_21[9], trans_21[3];
    const double inv_s = 1.0 / (double)s_12;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            s_rot_12[3 * i + j] = (double)s_12 * rot_12[3 * i + j];
            s_rot_21[3 * i + j] = inv_s * rot_12[3 * j + i];
        }
    for (int i = 0; i < 3; ++i) trans_21[i] = ((-s_rot_21[3 * i]) * trans_12[0] + (-s_rot_21[3 * i + 1]) * trans_12[1]) + (-s_rot_21[3 * i + 2]) * trans_12[2];
    double s_rot_21w[9], trans_21w[3], s_rot_12w[9], trans_12w[3], zero[3] = {0, 0, 0};
    mat_mul(s_rot_21, rot_1w, s_rot_21w);  // :457-458
    mat_vec(s_rot_21, trans_1w, trans_21w);
    for (int i = 0; i < 3; ++i) trans_21w[i] += trans_21[i];
    mat_mul(s_rot_12, rot_2w, s_rot_12w);  // :529-530
    mat_vec(s_rot_12, trans_2w, trans_12w);
    for (int i = 0; i < 3; ++i) trans_12w[i] += trans_12[i];
    int num = 0;
    for (int i = 0; i < n1; ++i) matched_2_in_1[i] = mutual_2_in_1[i] = -1;
    for (int i = 0; i < n2; ++i) matched_1_in_2[i] = -1;
    *num_matches = 0;
    {  // landmarks of keyframe 1 into keyframe 2 (:459-523); the image test uses keyframe 2's camera
        ProjQueries Q{n1, pos_w1, nullptr, min_valid1, max_valid1, valid1, nullptr, lm_desc1, nullptr, nullptr};
        ProjOpts O{1, 2, 1, 0, margin, 0, 100u, 0.f, SVGPU_MATCH_BEST_ONLY, 0, 0, 1, nullptr};
        InCellsFrame F{desc2, xy2, octave2, n2, nullptr, nullptr, nullptr, cam2->min_x, cam2->max_x, cam2->min_y, cam2->max_y, grid_cols, grid_rows};
        int rc = proj_match(ctx, "svgpu_match_keyframes_mutually: bad arguments", cam2, s_rot_21w, trans_21w, zero, Q, num_levels, scale_factors,
                            log_scale_factor, F, O, matched_2_in_1, &num, nullptr, nullptr, nullptr, nullptr);
        if (rc) return rc;
    }
    {  // landmarks of keyframe 2 into keyframe 1 (:531-595); the reference reprojects with keyframe 2's camera here as well (:550) and
       // looks the keypoints up in keyframe 1's grid (:571)
        ProjQueries Q{n2, pos_w2, nullptr, min_valid2, max_valid2, valid2, nullptr, lm_desc2, nullptr, nullptr};
        ProjOpts O{1, 2, 1, 0, margin, 0, 100u, 0.f, SVGPU_MATCH_BEST_ONLY, 0, 0, 1, nullptr};
        InCellsFrame F{desc1, xy1, octave1, n1, nullptr, nullptr, nullptr, cam1->min_x, cam1->max_x, cam1->min_y, cam1->max_y, grid_cols, grid_rows};
        int rc = proj_match(ctx, "svgpu_match_keyframes_mutually: bad arguments", cam2, s_rot_12w, trans_12w, zero, Q, num_levels, scale_factors,
                            log_scale_factor, F, O, matched_1_in_2, &num, nullptr, nullptr, nullptr, nullptr);
        if (rc) return rc;
    }
    num = 0;
    for (int i = 0; i < n1; ++i) {  // cross-check, :598-610
        const int idx_2 = matched_2_in_1[i];
        if (idx_2 < 0) continue;
        if (matched_1_in_2[idx_2] == i) {
            mutual_2_in_1[i] = idx_2;
            ++num;
        }
    }
    *num_matches = num;
    return SVGPU_OK;
}

int svgpu_fuse_detect_duplication(svgpu_ctx* ctx, const svgpu_camera* cam, const double* rot_cw, const double* trans_cw, int n, const double* pos_w,
                                  const uint8_t* valid, const float* min_valid_dist, const float* max_valid_dist, const double* mean_normal,
                                  const uint8_t* lm_desc, int num_levels, const float* scale_factors, const float* inv_level_sigma_sq,
                                  float log_scale_factor, float margin, int do_reprojection_matching, const uint8_t* tdesc, const float* t_xy,
                                  const int32_t* t_octave, const float* t_xright, int nt, int grid_cols, int grid_rows, int32_t* best_idx,
                                  int* num_fused) {
    const svgpu_frame* const bound = sv_take_bound_frame(ctx);  // one-shot: consumed before anything can fail
    if (!ctx || !cam || !rot_cw || !trans_cw) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_fuse_detect_duplication: bad arguments");
    double center[3];
    cam_center(rot_cw, trans_cw, center);  // fuse.cc:20
    ProjQueries Q{n, pos_w, mean_normal, min_valid_dist, max_valid_dist, valid, nullptr, lm_desc, nullptr, nullptr};
    ProjOpts O{1, 1, 0, 0, margin, 0, 50u, 0.f, SVGPU_MATCH_BEST_ONLY, 0, do_reprojection_matching ? 1 : 0, 0, inv_level_sigma_sq};
    const InCellsFrame F = frame_side(bound, cam, tdesc, t_xy, t_octave, nt, nullptr, nullptr, t_xright, false, true, grid_cols, grid_rows);
    return proj_match(ctx, "svgpu_fuse_detect_duplication: bad arguments", cam, rot_cw, trans_cw, center, Q, num_levels, scale_factors, log_scale_factor, F,
                      O, best_idx, num_fused, nullptr, nullptr, nullptr, nullptr);
}

int svgpu_match_for_triangulation(svgpu_ctx* ctx, const uint8_t* desc1, const float* angle1, const int32_t* octave1, const double* bearings1,
                                  const uint8_t* has_lm1, const float* xright1, int n1, const uint8_t* desc2, const float* angle2,
                                  const double* bearings2, const uint8_t* has_lm2, const float* xright2, int n2, const int32_t* node1,
                                  const int32_t* node2, const double* E_12, const double* epipole_in_2, int valid_epipole, const float* scale_factors,
                                  int num_levels, float residual_rad_thr, float lowe_ratio, int check_orientation, int32_t* matched_2_in_1,
                                  int* num_matches) {
    std::vector<uint8_t> v1(n1 > 0 ? n1 : 0), v2(n2 > 0 ? n2 : 0);  // queries / candidates = keypoints WITHOUT a landmark (robust.cc:47-50, 66-70)
    for (int i = 0; i < n1; ++i) v1[i] = has_lm1 ? !has_lm1[i] : 1;
    for (int i = 0; i < n2; ++i) v2[i] = has_lm2 ? !has_lm2[i] : 1;
    BucketSide S1{desc1, angle1, v1.data(), node1, octave1, bearings1, xright1, n1};
    BucketSide S2{desc2, angle2, v2.data(), node2, nullptr, bearings2, xright2, n2};
    return bucket_match(ctx, "svgpu_match_for_triangulation: bad arguments", S1, S2, nullptr, 1, E_12, epipole_in_2, valid_epipole, scale_factors, num_levels,
                        residual_rad_thr, 50u, lowe_ratio, check_orientation, SVGPU_MATCH_TRIANGULATION, matched_2_in_1, num_matches);
}

int svgpu_bow_match(svgpu_ctx* ctx, const uint8_t* desc1, const float* angle1, const uint8_t* valid1, const int32_t* node1, int n1,
                    const uint8_t* desc2, const float* angle2, const uint8_t* valid2, const int32_t* node2, int n2, const uint8_t* occupied2,
                    float lowe_ratio, int check_orientation, int32_t* match_1to2, int* num_matches) {
    if (!node1 || !node2) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_bow_match: node ids are required");
    BucketSide S1{desc1, angle1, valid1, node1, nullptr, nullptr, nullptr, n1};
    BucketSide S2{desc2, angle2, valid2, node2, nullptr, nullptr, nullptr, n2};
    return bucket_match(ctx, "svgpu_bow_match: bad arguments", S1, S2, occupied2, 0, nullptr, nullptr, 0, nullptr, 0, 0.f, 50u, lowe_ratio, check_orientation,
                        SVGPU_MATCH_RATIO, match_1to2, num_matches);
}

}  // extern "C"
