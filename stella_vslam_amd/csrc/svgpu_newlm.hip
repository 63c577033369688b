// svgpu_new_landmarks_batch: the loop of mapping_module::create_new_landmarks (mapping_module.cc:275-341) in one staged call -- per
// neighbour match_for_triangulation, then two_view_triangulator::triangulate, with the keypoints that got a landmark leaving the queries
// of every later neighbour.  Candidate lists and distances of all active neighbours are built beside each other by the batched bucket
// matcher's kernels under the initial landmark state; the part that depends on the neighbours before it is the chain of
// k_newlm_replay / k_newlm_triangulate launches (match_kernels.hip), in neighbour order on the one stream.  DESIGN section 20.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "sv_staged_call.h"
#include "match_kernels.h"
#include "newlm_layout.h"
#include "sv_sort.h"
#include "triangulate_kernels.h"

namespace {

bool tri_view_ok(const svgpu_triangulate_view& v) {
    return v.cam && v.pose_cw && v.n >= 0 && v.cam->model >= SVGPU_CAM_PERSPECTIVE && v.cam->model <= SVGPU_CAM_RADIAL_DIVISION
           && (v.n == 0 || (v.xy && v.octave && v.bearings));
}
// the two views of one keyframe: the same keypoints, and the arrays both view types carry are the same arrays
bool views_agree(const svgpu_match_view& m, const svgpu_triangulate_view& t, bool side1) {
    return m.n == t.n && m.bearings == t.bearings && m.xright == t.xright && (m.octave == t.octave || (!side1 && !m.octave));
}
// what the device dereferences by a keypoint's own values: octaves index the ORB tables; a stereo keypoint of an equirectangular camera
// is the reference's "Not implemented" exception (data/common.cc:239-241)
bool keypoints_ok(const svgpu_triangulate_view& v, int num_levels) {
    for (int i = 0; i < v.n; ++i) {
        if (v.octave[i] < 0 || v.octave[i] >= num_levels) return false;
        if (v.cam->model == SVGPU_CAM_EQUIRECTANGULAR && v.xright && 0 <= v.xright[i]) return false;
    }
    return true;
}
void fill_view(const svgpu_triangulate_view& v, float scale_factor_1, TriView& T) {
    T = TriView{};
    T.cam = *v.cam;
    std::memcpy(T.pose_cw, v.pose_cw, sizeof T.pose_cw);
    const double* P = v.pose_cw;
    for (int i = 0; i < 3; ++i)  // keyframe::set_pose_cw (data/keyframe.cc:365-376): trans_wc = -rot_wc * trans_cw
        T.trans_wc[i] = ((-P[i]) * P[3] + (-P[4 + i]) * P[7]) + (-P[8 + i]) * P[11];
    T.true_baseline = v.true_baseline;
    T.fx_inv = 1.0 / v.cam->fx;
    T.fy_inv = 1.0 / v.cam->fy;
    T.ratio_factor = 2.0f * std::max(scale_factor_1, v.scale_factor);
    T.n = v.n;
}

}  // namespace

extern "C" int svgpu_new_landmarks_batch(svgpu_ctx* ctx, const svgpu_match_view* side1, const svgpu_triangulate_view* view1, int num_neighbours,
                                         const svgpu_match_view* side2, const svgpu_triangulate_view* neighbours, const uint8_t* active, const double* E_12,
                                         const double* epipole_in_2, const int32_t* valid_epipole, const float* scale_factors, const float* level_sigma_sq,
                                         int num_levels, float residual_rad_thr, float lowe_ratio, int check_orientation, float rays_parallax_deg_thr,
                                         int32_t* matched_2_in_1, double* pos_w, uint8_t* status, int32_t* num_matches, int32_t* num_accepted,
                                         int32_t* created_by, svgpu_call_stats* stats) {
    const char* who = "svgpu_new_landmarks_batch: bad arguments";
    const int K = num_neighbours;
    if (!ctx || K < 0) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    if (K == 0) return SVGPU_OK;
    if (!side1 || !view1 || !side2 || !neighbours || !E_12 || !epipole_in_2 || !valid_epipole || !scale_factors || !level_sigma_sq || !num_matches
        || !num_accepted || num_levels < 1 || num_levels > SV_MAX_LEVELS)
        return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    const svgpu_match_view& m1 = *side1;
    if (m1.n < 0 || m1.occupied || !tri_view_ok(*view1) || !views_agree(m1, *view1, true) || (m1.n > 0 && (!m1.desc || (check_orientation && !m1.angle)))
        || !keypoints_ok(*view1, num_levels))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    const int n1 = m1.n;
    size_t N2 = 0, pairs = 0;
    std::vector<int32_t> prob_of_nb((size_t)K, -1);
    std::vector<int> nb_of_prob;
    bool work = false;
    for (int k = 0; k < K; ++k) {
        const svgpu_match_view& m = side2[k];
        if (m.n < 0 || m.n >= (1 << 22) || m.occupied || !tri_view_ok(neighbours[k]) || !views_agree(m, neighbours[k], false)
            || (m.n > 0 && (!m.desc || (check_orientation && !m.angle))) || (m1.node == nullptr) != (m.node == nullptr) || !keypoints_ok(neighbours[k], num_levels))
            return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
        if (active && !active[k]) continue;
        prob_of_nb[k] = (int32_t)nb_of_prob.size();
        nb_of_prob.push_back(k);
        N2 += (size_t)m.n;
        pairs += (size_t)n1 * (size_t)m.n;  // (no list can hold more than its bucket: the lists' total stays below this)
        work = work || (n1 > 0 && m.n > 0);
    }
    const int M = (int)nb_of_prob.size();
    const size_t lim = (size_t)INT32_MAX, cells = (size_t)K * (size_t)n1, R = (size_t)M * (size_t)n1;
    if (cells * 3 + (size_t)K > lim || (size_t)n1 * 8 > lim || N2 * 8 > lim || pairs > lim || (cells > 0 && (!matched_2_in_1 || !pos_w || !status))
        || (n1 > 0 && !created_by))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    // ---- nothing can fail on the arguments from here on: the results of a call that finds no candidate
    for (int k = 0; k < K; ++k) num_matches[k] = num_accepted[k] = 0;
    for (size_t i = 0; i < cells; ++i) matched_2_in_1[i] = -1, status[i] = SVGPU_TRI_SKIPPED;
    for (size_t i = 0; i < cells * 3; ++i) pos_w[i] = 0.0;
    for (int i = 0; i < n1; ++i) created_by[i] = -1;
    struct Tally {  // what the call issues (svgpu_call_stats)
        int launches = 0, copies = 0, syncs = 0;
        void add(const SvIssued& n) { launches += n.launches, copies += n.copies; }
    } T;
    auto report = [&]() {
        if (stats) *stats = svgpu_call_stats{T.launches, T.copies, T.syncs};
    };
    report();
    if (!work) return SVGPU_OK;

    NewLmShape S;
    BucketBatchShape& H = S.match;
    H.num_problems = M, H.shared1 = true, H.shared2 = false;
    H.side1.push_back(BucketSide{m1.desc, m1.angle, m1.valid, m1.node, m1.octave, m1.bearings, m1.xright, n1});
    S.num_neighbours = (size_t)K, S.depth1 = view1->depth != nullptr, S.view_rec = sizeof(TriView);
    std::vector<int> form((size_t)M);
    H.global_form.assign((size_t)M, 0);
    size_t lds_bytes = 0;
    int max_small = n1 <= SV_SORT_SMALL_MAX ? n1 : 0;
    H.sortb = sv_bucket_sort_bytes(n1);
    for (int p = 0; p < M; ++p) {
        const svgpu_match_view& m = side2[nb_of_prob[p]];
        H.side2.push_back(BucketSide{m.desc, m.angle, m.valid, m.node, nullptr, m.bearings, m.xright, m.n});
        H.occupied2.push_back(nullptr);
        S.depth2.push_back(neighbours[nb_of_prob[p]].depth != nullptr);
        form[p] = sv_cand_replay_form(n1, m.n, false, SVGPU_MATCH_TRIANGULATION);
        if (form[p] < 0) H.global_form[p] = 1;
        else lds_bytes = std::max(lds_bytes, sv_cand_lds_bytes(n1, m.n, form[p]));
        H.sortb = std::max(H.sortb, sv_bucket_sort_bytes(m.n));
        if (m.n <= SV_SORT_SMALL_MAX) max_small = std::max(max_small, m.n);
    }
    H.scan_ints = sv_scan_scratch_ints(R);
    H.side_rec = sizeof(SvSortSide), H.gather_rec = sizeof(BucketBatchSide), H.bucket_rec = sizeof(BucketProblem), H.cand_rec = sizeof(CandProblem);
    H.replay_rec = sizeof(CandBatchReplay);

    std::vector<uint8_t> taken0((size_t)n1);
    for (int i = 0; i < n1; ++i) taken0[i] = m1.valid ? !m1.valid[i] : 0;
    NewLmPieces Y;
    std::vector<SvSortSide> sort_tab((size_t)M + 1);
    std::vector<BucketBatchSide> gather_tab(1);
    std::vector<BucketProblem> bucket_tab((size_t)M);
    std::vector<CandProblem> cand_tab((size_t)M);
    std::vector<CandBatchReplay> replay_tab((size_t)M);
    std::vector<TriView> views((size_t)K + 1);
    std::vector<int32_t> row_base((size_t)M + 1), side1_base{0, n1};
    bool lists = false;
    int32_t total = 0;
    auto layout = [&](UploadArena& A) {
        newlm_layout(A, S, lists, (size_t)total, Y);
        const BucketBatchPieces& B = Y.B;
        const BucketSidePlace& a = B.at1[0];
        sort_tab[0] = SvSortSide{a.node, n1, a.key, a.order};
        gather_tab[0] = BucketBatchSide{(const uint32_t*)a.desc, a.order, a.desc_rows};
        fill_view(*view1, view1->scale_factor, views[(size_t)K]);
        views[(size_t)K].xy = Y.xy1, views[(size_t)K].octave = a.octave, views[(size_t)K].bearings = a.bearings, views[(size_t)K].xright = a.xright;
        views[(size_t)K].depth = Y.depth1;
        for (int k = 0; k < K; ++k)
            if (prob_of_nb[k] < 0) fill_view(neighbours[k], view1->scale_factor, views[k]);  // (an inactive neighbour's view names no array: nothing reads it)
        for (int p = 0; p < M; ++p) {
            const int nb = nb_of_prob[p];
            const BucketSidePlace& b = B.at2[p];
            sort_tab[(size_t)p + 1] = SvSortSide{b.node, H.side2[p].n, b.key, b.order};
            const size_t r0 = B.row_first[p];
            row_base[p] = (int32_t)r0;
            BucketProblem& Q = bucket_tab[p];
            Q = BucketProblem{};
            Q.n1 = n1, Q.n2 = H.side2[p].n, Q.check_orientation = check_orientation, Q.tri = 1, Q.thr = 50u;
            Q.desc1 = (const uint32_t*)a.desc, Q.desc2 = (const uint32_t*)b.desc;
            Q.angle1 = a.angle, Q.angle2 = b.angle, Q.valid1 = a.valid, Q.valid2 = b.valid;
            Q.octave1 = a.octave, Q.bearings1 = a.bearings, Q.bearings2 = b.bearings, Q.xright1 = a.xright, Q.xright2 = b.xright;
            std::memcpy(Q.E12, E_12 + 9 * (size_t)nb, sizeof Q.E12);
            std::memcpy(Q.epipole, epipole_in_2 + 3 * (size_t)nb, sizeof Q.epipole);
            Q.valid_epipole = valid_epipole[nb];
            for (int l = 0; l < num_levels; ++l) Q.scale_factors[l] = scale_factors[l];
            Q.residual_rad_thr = residual_rad_thr;
            Q.key1 = a.key, Q.q_idx = a.order, Q.key2 = b.key, Q.t_sorted = b.order;
            Q.row_lo = B.row_lo.p ? B.row_lo.p + r0 : nullptr, Q.row_hi = B.row_hi.p ? B.row_hi.p + r0 : nullptr;
            Q.q_valid = B.q_valid.p ? B.q_valid.p + r0 : nullptr, Q.cand_off = B.cand_off.p ? B.cand_off.p + r0 : nullptr, Q.cand_idx = B.cand_idx;
            CandProblem& P = cand_tab[p];
            P = CandProblem{};
            P.q_valid = Q.q_valid, P.cand_off = Q.cand_off, P.cand_idx = Q.cand_idx;
            P.qdesc = a.desc_rows, P.tdesc = Q.desc2, P.nq = n1, P.nt = Q.n2;
            P.check_orientation = 0;  // gated in the scan
            P.thr = 50u, P.lowe_ratio = lowe_ratio, P.mode = SVGPU_MATCH_TRIANGULATION;
            P.dist = B.dist, P.match_q = B.match_rows.p ? B.match_rows.p + r0 : nullptr, P.num = B.num.p ? B.num.p + p : nullptr;
            replay_tab[p] = CandBatchReplay{form[p], form[p] < 0 && B.owner.p ? B.owner.p + B.owner_first[p] : nullptr,
                                            form[p] < 0 && B.match_of_row.p ? B.match_of_row.p + B.mrow_first[p] : nullptr};
            TriView& V = views[nb];
            fill_view(neighbours[nb], view1->scale_factor, V);
            V.xy = Y.xy2.p ? Y.xy2.p + 2 * Y.first2[p] : nullptr, V.octave = Y.octave2.p ? Y.octave2.p + Y.first2[p] : nullptr;
            V.bearings = b.bearings, V.xright = b.xright, V.depth = Y.depth2_at[p];
        }
        row_base[M] = (int32_t)R;
    };
    StagedCall C;
    auto tables = [&]() {  // (after every layout: the records hold arena addresses; the seven pieces lie next to one another)
        const BucketBatchPieces& B = Y.B;
        C.up(B.side_tab, (const char*)sort_tab.data(), B.gather_tab, (const char*)gather_tab.data(), B.bucket_tab, (const char*)bucket_tab.data());
        C.up(B.cand_tab, (const char*)cand_tab.data(), B.replay_tab, (const char*)replay_tab.data());
        C.up(B.row_base, row_base.data(), B.side1_base, side1_base.data());
    };
    auto count = [&]() -> int {  // one upload of every keyframe, then orders, rows and the candidate count of all active neighbours
        const BucketBatchPieces& B = Y.B;
        {
            const BucketSide& h = H.side1[0];
            const BucketSidePlace& a = B.at1[0];
            const size_t n = (size_t)n1;
            C.up(a.desc, h.desc, n * 32), C.up(a.angle, h.angle, n), C.up(a.valid, h.valid, n), C.up(a.node, h.node, n);
            C.up(a.octave, h.octave, n), C.up(a.bearings, h.bearings, n * 3), C.up(a.xright, h.xright, n);
            C.up(Y.xy1, view1->xy), C.up(Y.depth1, view1->depth), C.up(Y.taken, taken0.data());
        }
        for (int p = 0; p < M; ++p) {
            const BucketSide& h = H.side2[p];
            const BucketSidePlace& b = B.at2[p];
            const svgpu_triangulate_view& v = neighbours[nb_of_prob[p]];
            const size_t n = (size_t)h.n;
            C.up(b.desc, h.desc, n * 32), C.up(b.angle, h.angle, n), C.up(b.valid, h.valid, n), C.up(b.node, h.node, n);
            C.up(b.bearings, h.bearings, n * 3), C.up(b.xright, h.xright, n);
            C.up(Y.xy2.p + 2 * Y.first2[p], v.xy, n * 2), C.up(Y.octave2.p + Y.first2[p], v.octave, n), C.up(Y.depth2_at[p], v.depth, n);
        }
        C.up(Y.view_tab, (const char*)views.data()), C.up(Y.prob_of_nb, prob_of_nb.data());
        tables();
        int r = C.flush();
        if (r) return r;
        ++T.copies;
        SvProfScope ps(ctx, C.s, "k_bucket_batch");
        // every side of at most SV_SORT_SMALL_MAX keypoints in one launch, a workgroup each; longer ones one after another by the general
        // sort (whose launches the tally does not count)
        const bool small = sv_sort_small_sides(C.s, (const SvSortSide*)B.side_tab.p, M + 1, max_small);
        T.launches += small ? 1 : 0;
        for (int u = 0; u <= M && !r; ++u)
            if (!small || sort_tab[u].n > SV_SORT_SMALL_MAX)
                r = sv_bucket_sort(ctx, C.s, sort_tab[u].node, sort_tab[u].n, B.sort_scratch, H.sortb, sort_tab[u].keys_out, sort_tab[u].idx_out);
        if (r) return r;
        sv_bucket_batch_rows_count(ctx, C.s, (const BucketProblem*)B.bucket_tab.p, B.row_base, M, (int)R, B.cand_off, B.scan_scratch);
        T.launches += 2 + (H.scan_ints ? 3 : 1);  // rows, counts, their scan
        return SVGPU_OK;
    };
    int rc = C.open(ctx, "svgpu_new_landmarks_batch: internal arena overflow", layout);
    if (!rc) rc = count();
    if (!rc) {
        rc = C.read_now(&total, Y.B.cand_off.p + R);
        ++T.copies, ++T.syncs;
    }
    report();
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
        ++T.copies;
    }
    const BucketBatchPieces& B = Y.B;
    {
        SvProfScope ps(ctx, C.s, "k_bucket_batch");
        sv_bucket_batch_fill(C.s, (const BucketProblem*)B.bucket_tab.p, B.row_base, M, (int)R);
        sv_bucket_batch_gather(C.s, (const BucketBatchSide*)B.gather_tab.p, B.side1_base, 1, n1);
        T.launches += 2;
    }
    T.add(sv_launch_cand_dist_batch(ctx, C.s, (const CandProblem*)B.cand_tab.p, B.row_base, M, (int)R));
    NewLmChain N{};
    N.num_neighbours = K, N.n1 = n1, N.prob_of_nb = Y.prob_of_nb, N.cand_tab = (const CandProblem*)B.cand_tab.p;
    N.form = (const CandBatchReplay*)B.replay_tab.p, N.q_idx = B.at1[0].order, N.q_valid = B.q_valid, N.match_rows = B.match_rows;
    N.views = (const TriView*)Y.view_tab.p;
    for (int l = 0; l < num_levels; ++l) N.scale_factors[l] = scale_factors[l], N.level_sigma_sq[l] = level_sigma_sq[l];
    N.cos_rays_parallax_thr = (float)std::cos(rays_parallax_deg_thr * M_PI / 180.0);  // two_view_triangulator.cc:17 (a float member)
    N.taken = Y.taken, N.match = Y.match, N.pos_w = Y.pos_w, N.status = Y.status, N.num_matches = Y.num_matches, N.num_accepted = Y.num_accepted;
    N.created_by = Y.created_by;
    T.add(sv_launch_newlm_chain(ctx, C.s, N, prob_of_nb.data(), lds_bytes));
    C.down(matched_2_in_1, Y.match), C.down(pos_w, Y.pos_w), C.down(status, Y.status), C.down(num_matches, Y.num_matches);
    C.down(num_accepted, Y.num_accepted), C.down(created_by, Y.created_by);
    {
        std::vector<Downloads::Item> items = C.D.items;
        T.copies += (int)sv_merge_ranges(items, 32768).size();  // the results lie next to one another: one read-back
    }
    rc = C.finish();
    ++T.syncs;
    report();
    return rc;
}
