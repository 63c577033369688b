// svgpu_loop_sim3_batch: the middle of module::loop_detector::select_loop_candidate_via_Sim3 (module/loop_detector.cc:537-587) for all
// candidates in one staged call.  Per candidate: the scale from the small-parallax landmark pairs (:540-573) -> the similarity transforms of
// projection::match_keyframes_mutually formed on the device (match/projection.cc:428-431, :461-462, :540-541) -> both matcher passes over
// ONE concatenation of rows (K x n1 rows of keyframe 1's landmarks into the candidates, then every candidate's landmarks into the one
// binned keyframe 1) -> k_cand_dist_batch / k_cand_replay_batch with 2K problem records -> cross-check and the ordered edge gather of
// optimize::transform_optimizer (optimize/transform_optimizer.cc:64-94) straight into the arrays k_sim3_opt reads -> sv_launch_sim3opt.
// The kernels of this file are the glue the per-call path does on the host; the replay and the optimiser are the existing ones.
// Every double expression keeps the operation order of the host code it replaces (svgpu_match2.hip:521-541) and this file is compiled
// without contraction, as the library's flags have it: the transforms equal the host's bit for bit.
#include "svgpu_match_common.h"
#include "loop_sim3_layout.h"
#include "sim3opt_kernels.h"
#include "frame_device.h"
#include "sv_sort.h"
#include "sv_validate.h"

using namespace svm;

namespace {

#define LOOP_NO_RATIO 0xFFFFFFFFu  // ratio_bits of a pair that gives no ratio (no kept ratio has this pattern: it is a NaN's)

struct LoopDev {
    int K, n1, N2;
    int rows_a, rows_all;  // K x n1, K x n1 + N2
    float inv_level_sigma_sq[SV_MAX_LEVELS];
    double pose_1w[12];
    // keyframe 1
    const float* xy1;
    const int32_t* octave1;
    const double* pos_w1;
    const uint8_t* has_lm1;
    const float *min1, *max1;
    // the candidates' keyframes
    const float* xy2;
    const int32_t* octave2;
    const double* pos_w2;
    const uint8_t* has_lm2;
    const float *min2, *max2;
    const int32_t* kf2_off;
    const double *pose_in_cand, *pose_2w, *rot_12, *trans_12;
    const uint8_t* active;
    const float* scale_in;  // nullable
    Sim3OptProblem* prob;
    const ReprojProblem* reproj_tab;
    const uint8_t* prior_state;
    const int32_t* prior_idx2;
    const double* prior_pos_w;
    uint32_t* ratio_bits;
    double* xf;
    uint8_t *live, *already2;
    uint8_t* visible;
    float *q_xy, *q_margin;
    int32_t *q_min_level, *q_max_level;
    double *obs1, *obs2, *pos1, *pos2;
    float *w1, *w2;
    float* scale;
    int32_t *code, *match_a, *match_b, *mutual, *num_mutual, *num_edges, *edge_idx1, *edge_idx2;
    uint8_t* edge_status;
};

// ---- step 1: one workgroup per candidate.  The ratios of the kept pairs stay where their pair is (ratio_bits, LOOP_NO_RATIO elsewhere);
// element (count - 1) / 2 of their ascending order is found by a radix selection over the bit patterns, most significant byte first --
// the ratios are non-negative floats, whose order is the order of their patterns, and the element of a rank is a property of the multiset:
// what std::sort + scales[(size - 1) / 2] gives (:572-573), for any count, also beyond the workgroup's threads.  A thread reads back only
// what it wrote.  The same workgroup marks is_already_matched_in_keyfrm_2 (projection.cc:440-450) and forms the candidate's transforms.
__global__ void __launch_bounds__(1024) k_loop_scale(LoopDev D) {
    __shared__ int s_hist[256];
    __shared__ int s_count, s_k;
    __shared__ unsigned s_prefix;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int lo2 = D.kf2_off[p], hi2 = D.kf2_off[p + 1];
    const size_t r0 = (size_t)p * D.n1;
    for (int j = lo2 + tid; j < hi2; j += 1024) D.already2[j] = 0;
    if (tid == 0) s_count = 0;
    __syncthreads();
    if (!D.active[p]) {
        if (tid == 0) D.live[p] = 0, D.code[p] = -1, D.scale[p] = 0.f;
        return;
    }
    const double* __restrict__ T = D.pose_in_cand + 12 * (size_t)p;
    int kept = 0;
    for (int i = tid; i < D.n1; i += 1024) {
        const int st = D.prior_state[r0 + i], idx2 = D.prior_idx2[r0 + i];
        if (st != 0 && idx2 >= 0) D.already2[lo2 + idx2] = 1;
        uint32_t bits = LOOP_NO_RATIO;
        if (!D.scale_in && st == 1 && D.has_lm1[i]) {  // loop_detector.cc:545-550
            const double* __restrict__ a = D.prior_pos_w + 3 * (r0 + i);
            const double* __restrict__ b = D.pos_w1 + 3 * (size_t)i;
            const double c0 = ((T[0] * a[0] + T[1] * a[1]) + T[2] * a[2]) + T[3], c1 = ((T[4] * a[0] + T[5] * a[1]) + T[6] * a[2]) + T[7],
                         c2 = ((T[8] * a[0] + T[9] * a[1]) + T[10] * a[2]) + T[11];  // :553
            const double u0 = ((D.pose_1w[0] * b[0] + D.pose_1w[1] * b[1]) + D.pose_1w[2] * b[2]) + D.pose_1w[3],
                         u1 = ((D.pose_1w[4] * b[0] + D.pose_1w[5] * b[1]) + D.pose_1w[6] * b[2]) + D.pose_1w[7],
                         u2 = ((D.pose_1w[8] * b[0] + D.pose_1w[9] * b[1]) + D.pose_1w[10] * b[2]) + D.pose_1w[11];  // :554
            const float n_cand = (float)sqrt((c0 * c0 + c1 * c1) + c2 * c2), n_curr = (float)sqrt((u0 * u0 + u1 * u1) + u2 * u2);  // :555-556
            const double dot = (c0 * u0 + c1 * u1) + c2 * u2;
            const float cos_parallax = (float)(dot / (double)(n_cand * n_curr));  // :557
            if (0.99996192306f < cos_parallax) {  // :559-563, strict
                bits = __float_as_uint(n_curr / n_cand);  // :564
                ++kept;
            }
        }
        D.ratio_bits[r0 + i] = bits;
    }
    if (kept) atomicAdd(&s_count, kept);
    __syncthreads();
    float scale;
    if (D.scale_in) scale = D.scale_in[p];
    else {
        const int count = s_count;
        if (count == 0) {  // :566-569
            if (tid == 0) D.live[p] = 0, D.code[p] = 1, D.scale[p] = 0.f;
            return;
        }
        if (tid == 0) s_prefix = 0u, s_k = (count - 1) / 2;
#pragma unroll 1
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) s_hist[tid] = 0;
            __syncthreads();
            const unsigned prefix = s_prefix, mask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
            for (int i = tid; i < D.n1; i += 1024) {
                const uint32_t bits = D.ratio_bits[r0 + i];
                if (bits != LOOP_NO_RATIO && (bits & mask) == prefix) atomicAdd(&s_hist[(bits >> shift) & 255u], 1);
            }
            __syncthreads();
            if (tid == 0) {  // the byte whose bin holds rank k among the patterns that share the prefix
                int k = s_k, d = 0;
                while (d < 255 && k >= s_hist[d]) k -= s_hist[d], ++d;
                s_k = k;
                s_prefix = prefix | ((unsigned)d << shift);
            }
            __syncthreads();
        }
        scale = __uint_as_float(s_prefix);
    }
    if (tid == 0) {  // svgpu_match2.hip:521-541 (projection.cc:428-431, :461-462, :540-541)
        const double* __restrict__ rot_12 = D.rot_12 + 9 * (size_t)p;
        const double* __restrict__ trans_12 = D.trans_12 + 3 * (size_t)p;
        const double* __restrict__ P2 = D.pose_2w + 12 * (size_t)p;
        double* __restrict__ X = D.xf + 24 * (size_t)p;
        const double s = (double)scale, inv_s = 1.0 / (double)scale;
        double s_rot_12[9], s_rot_21[9], trans_21[3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                s_rot_12[3 * i + j] = s * rot_12[3 * i + j];
                s_rot_21[3 * i + j] = inv_s * rot_12[3 * j + i];
            }
#pragma unroll
        for (int i = 0; i < 3; ++i)
            trans_21[i] = ((-s_rot_21[3 * i]) * trans_12[0] + (-s_rot_21[3 * i + 1]) * trans_12[1]) + (-s_rot_21[3 * i + 2]) * trans_12[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                X[3 * i + j] = (s_rot_21[3 * i] * D.pose_1w[j] + s_rot_21[3 * i + 1] * D.pose_1w[4 + j]) + s_rot_21[3 * i + 2] * D.pose_1w[8 + j];
                X[12 + 3 * i + j] = (s_rot_12[3 * i] * P2[j] + s_rot_12[3 * i + 1] * P2[4 + j]) + s_rot_12[3 * i + 2] * P2[8 + j];
            }
            const double t21 = (s_rot_21[3 * i] * D.pose_1w[3] + s_rot_21[3 * i + 1] * D.pose_1w[7]) + s_rot_21[3 * i + 2] * D.pose_1w[11];
            X[9 + i] = t21 + trans_21[i];
            const double t12 = (s_rot_12[3 * i] * P2[3] + s_rot_12[3 * i + 1] * P2[7]) + s_rot_12[3 * i + 2] * P2[11];
            X[21 + i] = t12 + trans_12[i];
        }
        D.prob[p].sim3[7] = s;  // g2o::Sim3(rot_12, trans_12, scale_12), :580
        D.live[p] = 1, D.code[p] = 0, D.scale[p] = scale;
    }
}

// the row's candidate and pass: rows [0, K n1) are pass A (p = row / n1), the rest pass B (rows of candidate p from K n1 + kf2_off[p])
struct LoopRow {
    int p, q;    // candidate, query index inside the problem
    bool a;
};
__device__ __forceinline__ LoopRow loop_row(const LoopDev& D, int g) {
    LoopRow r;
    r.a = g < D.rows_a;
    if (r.a) r.p = g / D.n1, r.q = g - r.p * D.n1;
    else r.p = sv_segment_of(D.kf2_off, D.K, g - D.rows_a), r.q = g - D.rows_a - D.kf2_off[r.p];
    return r;
}

// ---- reprojection of all rows: k_can_observe's body (svfd::reproject_one / reproject_window) with the candidate's transform from device
// memory and keyframe 2's camera in BOTH passes (projection.cc:483, :562); the distance range with the 1.3 margins in double, no normal
// test, the distance of the transformed point (dist_mode 1, normal_mode 2, center_mode 1: svgpu_match2.hip:541-556)
__global__ void __launch_bounds__(256) k_loop_reproject(LoopDev D) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= D.rows_all) return;
    const LoopRow r = loop_row(D, g);
    const ReprojProblem& R = D.reproj_tab[r.p];
    const double* __restrict__ X = D.xf + 24 * (size_t)r.p + (r.a ? 0 : 12);
    bool offered = D.live[r.p] != 0;
    const double* pw;
    float minv, maxv;
    if (r.a) {  // :464-474
        const size_t e = (size_t)r.p * D.n1 + r.q;
        offered = offered && D.has_lm1[r.q] && !(D.prior_state[e] != 0 && D.prior_idx2[e] >= 0);
        pw = D.pos_w1 + 3 * (size_t)r.q, minv = D.min1[r.q], maxv = D.max1[r.q];
    }
    else {  // :543-553
        const size_t j = (size_t)D.kf2_off[r.p] + r.q;
        offered = offered && D.has_lm2[j] && !D.already2[j];
        pw = D.pos_w2 + 3 * j, minv = D.min2[j], maxv = D.max2[j];
    }
    const double zero[3] = {0.0, 0.0, 0.0};
    svfd::ReprojOut o;
    svfd::reproject_one(R, X, X + 9, zero, offered, pw[0], pw[1], pw[2], 0.0, 0.0, 0.0, minv, maxv, 0, false, o);
    D.visible[g] = o.vis ? 1 : 0;
    svfd::reproject_window(R, o, D.q_xy[2 * (size_t)g], D.q_xy[2 * (size_t)g + 1], D.q_margin[g], D.q_min_level[g], D.q_max_level[g]);
}

// ---- step 2's cross-check (projection.cc:613-626) and step 3, one workgroup per candidate: an ordered compaction of the edges in
// ascending idx1 (ballots and a scan of the waves' counts, no atomics), written where k_sim3_opt reads them, candidate p's from p x n1 on
__global__ void __launch_bounds__(1024) k_loop_edges(LoopDev D) {
    __shared__ int s_edge[16], s_mut[16];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lo2 = D.kf2_off[p];
    const size_t r0 = (size_t)p * D.n1;
    const bool live = D.live[p] != 0;
    int base = 0, mutuals = 0;
    for (int c0 = 0; c0 < D.n1; c0 += 1024) {
        const int i = c0 + tid;
        bool edge = false, isnew = false, prior = false;
        int idx2 = -1;
        if (i < D.n1) {
            const int m21 = live ? D.match_a[r0 + i] : -1;
            isnew = m21 >= 0 && D.match_b[lo2 + m21] == i;
            D.mutual[r0 + i] = isnew ? m21 : -1;
            D.edge_status[r0 + i] = 0;
            if (live && D.has_lm1[i]) {
                const int pidx = D.prior_idx2[r0 + i];
                if (isnew) edge = true, idx2 = m21;  // :623: the new match takes the entry, whatever it held
                else if (D.prior_state[r0 + i] == 1 && pidx >= 0) edge = prior = true, idx2 = pidx;  // transform_optimizer.cc:66-85
            }
        }
        const unsigned long long be = __ballot(edge), bm = __ballot(isnew);
        if (lane == 0) s_edge[wave] = __popcll(be), s_mut[wave] = __popcll(bm);
        __syncthreads();
        int off = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            off += w < wave ? s_edge[w] : 0;
            all += s_edge[w];
            mutuals += s_mut[w];
        }
        if (edge) {
            const size_t e = r0 + base + off + __popcll(be & ((1ull << lane) - 1ull));
            const size_t j = (size_t)lo2 + idx2;
            const double* __restrict__ p2 = prior ? D.prior_pos_w + 3 * (r0 + i) : D.pos_w2 + 3 * j;
            D.obs1[2 * e] = (double)D.xy1[2 * i], D.obs1[2 * e + 1] = (double)D.xy1[2 * i + 1];
            D.obs2[2 * e] = (double)D.xy2[2 * j], D.obs2[2 * e + 1] = (double)D.xy2[2 * j + 1];
            D.w1[e] = D.inv_level_sigma_sq[D.octave1[i]];
            D.w2[e] = D.inv_level_sigma_sq[D.octave2[j]];
#pragma unroll
            for (int k = 0; k < 3; ++k) D.pos1[3 * e + k] = D.pos_w1[3 * (size_t)i + k], D.pos2[3 * e + k] = p2[k];
            D.edge_idx1[e] = i, D.edge_idx2[e] = idx2;
        }
        base += all;
        __syncthreads();
    }
    for (int e = base + tid; e < D.n1; e += 1024) D.edge_idx1[r0 + e] = D.edge_idx2[r0 + e] = -1;
    if (tid == 0) {
        D.num_edges[p] = base, D.num_mutual[p] = mutuals;
        D.prob[p].m_lo = (int32_t)r0, D.prob[p].m_hi = (int32_t)r0 + base;
    }
}

// the edge's camera (mutual_reproj_edge_wrapper.h:64-158), as svgpu_sim3_transform_optimize fills it
bool loop_fill_view(const svgpu_camera& c, const double* pose_cw, Sim3OptView& o) {
    switch (c.model) {
        case SVGPU_CAM_PERSPECTIVE:
        case SVGPU_CAM_FISHEYE:
        case SVGPU_CAM_RADIAL_DIVISION:
            o.k[0] = c.fx, o.k[1] = c.fy, o.k[2] = c.cx, o.k[3] = c.cy;
            o.equirect = 0;
            break;
        case SVGPU_CAM_EQUIRECTANGULAR:
            o.k[0] = c.cols, o.k[1] = c.rows, o.k[2] = 0.0, o.k[3] = 0.0;
            o.equirect = 1;
            break;
        default:
            return false;
    }
    o.pad = 0;
    for (int k = 0; k < 12; ++k) o.pose[k] = pose_cw[k];
    return true;
}
bool loop_camera_ok(const svgpu_camera& c) {
    return c.model >= SVGPU_CAM_PERSPECTIVE && c.model <= SVGPU_CAM_RADIAL_DIVISION && c.min_x < c.max_x && c.min_y < c.max_y;
}
}  // namespace

extern "C" int svgpu_loop_sim3_batch(svgpu_ctx* ctx, const svgpu_camera* cam1, const double* pose_1w, int n1, const uint8_t* desc1, const float* xy1,
                                     const int32_t* octave1, const double* pos_w1, const uint8_t* has_lm1, const float* min_valid1,
                                     const float* max_valid1, const uint8_t* lm_desc1, int num_levels, const float* scale_factors,
                                     const float* inv_level_sigma_sq, float log_scale_factor, int grid_cols, int grid_rows, int num_candidates,
                                     const svgpu_camera* cam2, const double* pose_2w, const int32_t* kf2_off, const uint8_t* desc2, const float* xy2,
                                     const int32_t* octave2, const double* pos_w2, const uint8_t* has_lm2, const float* min_valid2,
                                     const float* max_valid2, const uint8_t* lm_desc2, const double* pose_1w_in_cand, const double* rot_12,
                                     const double* trans_12, const double* sim3_12, const uint8_t* active, const uint8_t* prior_state,
                                     const int32_t* prior_idx2, const double* prior_pos_w, const float* scale_12_in, float margin, float chi_sq,
                                     int fix_scale, int num_iter, int min_num_inliers, int32_t* status, float* scale_12, int32_t* matched_2_in_1,
                                     int32_t* matched_1_in_2, int32_t* mutual_2_in_1, int32_t* num_mutual, int32_t* edge_idx1, int32_t* edge_idx2,
                                     int32_t* num_edges, uint8_t* edge_status, double* sim3_12_out, int32_t* num_inliers,
                                     svgpu_sim3opt_stats* opt_stats, svgpu_call_stats* stats) {
    const char* const bad = "svgpu_loop_sim3_batch: bad arguments";
    if (!ctx || num_candidates < 0) return sv_set_error(ctx, SVGPU_ERR_INVALID, bad);
    if (num_candidates == 0) {
        if (stats) *stats = svgpu_call_stats{0, 0, 0};
        return SVGPU_OK;
    }
    // ---- validation: every index a kernel dereferences is checked here; nothing is launched or written before all of it has passed
    const int K = num_candidates;
    if (!cam1 || !pose_1w || n1 < 0 || n1 >= (1 << 22) || num_levels < 1 || num_levels > SV_MAX_LEVELS || !scale_factors || !inv_level_sigma_sq
        || !(log_scale_factor > 0.f) || grid_cols < 1 || grid_rows < 1 || (size_t)grid_cols * grid_rows > (size_t(1) << 22) || !cam2 || !pose_2w || !kf2_off
        || !pose_1w_in_cand || !rot_12 || !trans_12 || !sim3_12 || !(margin >= 0.f) || !sv_positive_finite(chi_sq) || num_iter < 0 || !status || !scale_12
        || !num_mutual || !num_edges || !sim3_12_out || !num_inliers
        || (n1 > 0 && (!desc1 || !xy1 || !octave1 || !pos_w1 || !has_lm1 || !min_valid1 || !max_valid1 || !lm_desc1 || !prior_state || !prior_idx2
                       || !prior_pos_w || !matched_2_in_1 || !mutual_2_in_1 || !edge_idx1 || !edge_idx2 || !edge_status)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, bad);
    if (!sv_offsets_ok(kf2_off, K)) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_loop_sim3_batch: kf2_off does not start at 0 or is not monotone");
    for (int p = 0; p < K; ++p)
        if (kf2_off[p + 1] - kf2_off[p] >= (1 << 22)) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_loop_sim3_batch: a keyframe of 1 << 22 keypoints or more");
    const size_t N2 = (size_t)kf2_off[K], E = (size_t)K * (size_t)n1, R = E + N2, lim = (size_t)INT32_MAX;
    const size_t ncell = (size_t)grid_cols * grid_rows;
    if (N2 > 0 && (!desc2 || !xy2 || !octave2 || !pos_w2 || !has_lm2 || !min_valid2 || !max_valid2 || !lm_desc2 || !matched_1_in_2))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, bad);
    if (E * 8 > lim || N2 * 8 > lim || R * 8 > lim || ((size_t)K + 1) * ncell > (size_t)SV_SCAN_MAX)
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_loop_sim3_batch: totals do not fit int32");
    Sim3OptView view1;
    if (!loop_camera_ok(*cam1) || !loop_fill_view(*cam1, pose_1w, view1))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_loop_sim3_batch: a camera model the edges do not cover");
    for (int l = 0; l < num_levels; ++l)
        if (!sv_positive_finite(inv_level_sigma_sq[l])) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_loop_sim3_batch: an inv_level_sigma_sq is not positive and finite");
    for (int i = 0; i < n1; ++i)
        if (octave1[i] < 0 || octave1[i] >= num_levels) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_loop_sim3_batch: octave out of range");
    for (size_t j = 0; j < N2; ++j)
        if (octave2[j] < 0 || octave2[j] >= num_levels) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_loop_sim3_batch: octave out of range");
    std::vector<Sim3OptProblem> prob((size_t)K);
    for (int p = 0; p < K; ++p) {
        const int n2 = kf2_off[p + 1] - kf2_off[p];
        const double* const s8 = sim3_12 + 8 * (size_t)p;
        double q2 = 0.0;
        for (int k = 0; k < 7; ++k)
            if (!std::isfinite(s8[k])) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_loop_sim3_batch: a Sim3_12 is not finite");
        for (int k = 0; k < 4; ++k) q2 += s8[k] * s8[k];
        if (!(std::fabs(q2 - 1.0) <= 1e-9)) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_loop_sim3_batch: a Sim3_12 without a unit quaternion");
        if (scale_12_in && !sv_positive_finite(scale_12_in[p])) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_loop_sim3_batch: a scale_12_in is not positive and finite");
        prob[p].view[0] = view1;
        if (!loop_camera_ok(cam2[p]) || !loop_fill_view(cam2[p], pose_2w + 12 * (size_t)p, prob[p].view[1]))
            return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_loop_sim3_batch: a camera model the edges do not cover");
        for (int k = 0; k < 8; ++k) prob[p].sim3[k] = s8[k];
        prob[p].m_lo = prob[p].m_hi = 0;
        for (int i = 0; i < n1; ++i)
            if (prior_idx2[(size_t)p * n1 + i] >= n2) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_loop_sim3_batch: a prior_idx2 beyond its keyframe");
    }

    LoopSim3Shape H;
    H.K = (size_t)K, H.n1 = (size_t)n1, H.N2 = N2, H.ncell = ncell, H.has_scale_in = scale_12_in != nullptr;
    H.prob_rec = sizeof(Sim3OptProblem), H.reproj_rec = sizeof(ReprojProblem), H.cand_rec = sizeof(CandProblem), H.replay_rec = sizeof(CandBatchReplay);
    H.grid_rec = sizeof(GridProblem), H.stats_rec = sizeof(svgpu_sim3opt_stats);
    // the 2K matcher problems: A_p = keyframe 1's landmarks into candidate p, B_p = candidate p's landmarks into keyframe 1.  The form of
    // every replay (sv_cand_replay_form decides, as for the single call), and the dynamic LDS of the one launch
    std::vector<int> form(2 * (size_t)K);
    std::vector<size_t> owner_first(2 * (size_t)K, 0), mrow_first(2 * (size_t)K, 0);
    std::vector<int32_t> row_base(2 * (size_t)K + 1), set_base((size_t)K + 2);
    size_t lds_bytes = 0;
    for (int u = 0; u < 2 * K; ++u) {
        const int p = u < K ? u : u - K, n2 = kf2_off[p + 1] - kf2_off[p];
        const int nq = u < K ? n1 : n2, nt = u < K ? n2 : n1;
        row_base[u] = u < K ? (int32_t)((size_t)p * n1) : (int32_t)(E + (size_t)kf2_off[p]);
        form[u] = sv_cand_replay_form(nq, nt, false, SVGPU_MATCH_BEST_ONLY);
        if (form[u] < 0) {
            owner_first[u] = H.owner_ints, mrow_first[u] = H.mrow_ints;
            H.owner_ints += (size_t)nt, H.mrow_ints += (size_t)nq;
        }
        else lds_bytes = std::max(lds_bytes, sv_cand_lds_bytes(nq, nt, form[u]));
    }
    row_base[2 * (size_t)K] = (int32_t)R;
    for (int p = 0; p <= K; ++p) set_base[p] = kf2_off[p];
    set_base[(size_t)K + 1] = (int32_t)(N2 + (size_t)n1);

    // the first capacity of the lists: 16 entries per row (a 7.5 px window lists well under one keypoint per row), at most 4 Mi entries
    // (32 MB of arena and mirror) whatever R; lists beyond it start the call again, sized exactly
    H.cap = std::min<size_t>(std::max<size_t>(4096, R * 16), size_t(1) << 22);
    std::vector<ReprojProblem> reproj_tab((size_t)K);
    std::vector<GridProblem> grid_tab(3 * (size_t)K + 1);  // the K + 1 keypoint sets (the candidates, then keyframe 1), then the 2K matcher problems' rows
    std::vector<CandProblem> cand_tab(2 * (size_t)K);
    std::vector<CandBatchReplay> replay_tab(2 * (size_t)K);
    std::vector<int32_t> code((size_t)K);
    struct Tally {  // what the call issues (svgpu_call_stats)
        int launches = 0, copies = 0, syncs = 0;
        void add(const SvIssued& n) { launches += n.launches, copies += n.copies; }  // what a shared launcher says it issued
    } T;
    for (int attempt = 0; attempt < 3; ++attempt) {  // (lists that outgrow the capacity start the call again, once, sized exactly; the tally runs on: it reports what the call issued)
        LoopSim3Pieces Y{};
        StagedCall C;
        int rc = C.open(ctx, "svgpu_loop_sim3_batch: internal arena overflow", [&](UploadArena& A) { loop_sim3_layout(A, H, Y); });
        if (rc) return rc;
        // ---- one upload: keyframe 1 once, the candidates' keyframes, the priors, the tables
        C.up(Y.desc1, desc1, Y.lm_desc1, lm_desc1, Y.xy1, xy1, Y.octave1, octave1, Y.pos_w1, pos_w1, Y.has_lm1, has_lm1, Y.min1, min_valid1, Y.max1, max_valid1);
        C.up(Y.desc2, desc2, Y.lm_desc2, lm_desc2, Y.xy2, xy2, Y.octave2, octave2, Y.pos_w2, pos_w2, Y.has_lm2, has_lm2, Y.min2, min_valid2, Y.max2, max_valid2);
        C.up(Y.kf2_off, kf2_off, Y.set_base, set_base.data(), Y.row_base, row_base.data(), Y.pose_in_cand, pose_1w_in_cand, Y.pose_2w, pose_2w);
        C.up(Y.rot_12, rot_12, Y.trans_12, trans_12, Y.scale_in, scale_12_in, Y.prior_state, prior_state, Y.prior_idx2, prior_idx2, Y.prior_pos_w, prior_pos_w);
        {
            uint8_t* const h_active = C.stage(Y.active);
            for (int p = 0; p < K; ++p) h_active[p] = (!active || active[p]) ? 1 : 0;
        }
        for (int p = 0; p < K; ++p) {
            ReprojProblem& Q = reproj_tab[p];
            Q = ReprojProblem{};
            Q.cam = cam2[p];  // keyframe 2's camera in both passes
            Q.ray_cos_thr = 0.5f, Q.num_levels = (unsigned)num_levels, Q.log_scale_factor = log_scale_factor, Q.margin = margin;
            for (int l = 0; l < num_levels; ++l) Q.scale_factors[l] = scale_factors[l];
            Q.dist_mode = 1, Q.normal_mode = 2, Q.center_mode = 1, Q.window_mode = 0;
        }
        // the grid records (the conventions of sv_launch_grid_sets): set u's cells are cell_cnt + u x ncell of the ONE counter array, its
        // cell_of the one array from set_base[u] on; every piece is offset by whole elements from its 256-byte aligned start, and the scans
        // run over the pieces themselves (cell_cnt, cand_off), never over an offset part
        for (int u = 0; u <= K; ++u) {
            const svgpu_camera& c = u < K ? cam2[u] : *cam1;
            const size_t o2 = u < K ? (size_t)kf2_off[u] : 0;
            GridProblem& G = grid_tab[u];
            G = GridProblem{};
            G.t_xy = u < K ? Y.xy2.p + 2 * o2 : Y.xy1.p, G.t_octave = u < K ? Y.octave2.p + o2 : Y.octave1.p, G.nt = set_base[u + 1] - set_base[u];
            G.min_x = c.min_x, G.min_y = c.min_y, G.cols = grid_cols, G.rows = grid_rows;
            G.inv_w = (double)grid_cols / (c.max_x - c.min_x), G.inv_h = (double)grid_rows / (c.max_y - c.min_y);  // float difference, double quotient (data/common.cc:86-87 via camera::base)
            G.cell_of = Y.cell_of.p + set_base[u], G.cell_off = Y.cell_cnt.p + (size_t)u * ncell, G.cell_items = Y.cell_items;
        }
        for (int u = 0; u < 2 * K; ++u) {
            const int p = u < K ? u : u - K, n2 = kf2_off[p + 1] - kf2_off[p];
            const size_t o2 = (size_t)kf2_off[p], r0 = (size_t)row_base[u];
            CandProblem& P = cand_tab[u];
            P = CandProblem{};
            if (u < K) {
                P.qdesc = (const uint32_t*)Y.lm_desc1.p, P.tdesc = (const uint32_t*)Y.desc2.p + o2 * 8;
                P.t_octave = Y.octave2.p + o2, P.t_xy = Y.xy2.p + 2 * o2, P.nq = n1, P.nt = n2, P.match_q = Y.match_a.p + r0;
            }
            else {
                P.qdesc = (const uint32_t*)Y.lm_desc2.p + o2 * 8, P.tdesc = (const uint32_t*)Y.desc1.p;
                P.t_octave = Y.octave1, P.t_xy = Y.xy1, P.nq = n2, P.nt = n1, P.match_q = Y.match_b.p + o2;
            }
            // (offsets into the ONE pair of lists: a problem's nq + 1 entries end where the next problem's begin)
            P.cand_off = Y.cand_off.p + r0, P.cand_idx = Y.cand_idx, P.q_valid = Y.visible.p + r0;
            P.check_orientation = 0, P.thr = 100u /* HAMMING_DIST_THR_HIGH */, P.lowe_ratio = 0.f, P.mode = SVGPU_MATCH_BEST_ONLY, P.no_claims = 1;
            P.dist = Y.dist, P.num = Y.num_ab.p + u;
            GridProblem& G = grid_tab[(size_t)K + 1 + u] = grid_tab[u < K ? p : K];  // the rows of problem u walk the grid of their target set
            G.q_xy = Y.q_xy.p + 2 * r0, G.q_margin = Y.q_margin.p + r0, G.q_min_level = Y.q_min_level.p + r0, G.q_max_level = Y.q_max_level.p + r0;
            G.q_valid = P.q_valid, G.nq = P.nq, G.cand_off = Y.cand_off.p + r0, G.cand_idx = Y.cand_idx;
            replay_tab[u] = CandBatchReplay{form[u], form[u] < 0 ? Y.owner.p + owner_first[u] : nullptr, form[u] < 0 ? Y.match_of_row.p + mrow_first[u] : nullptr};
        }
        C.up(Y.prob, (const char*)prob.data(), Y.reproj_tab, (const char*)reproj_tab.data(), Y.grid_tab, (const char*)grid_tab.data());
        C.up(Y.cand_tab, (const char*)cand_tab.data(), Y.replay_tab, (const char*)replay_tab.data());
        if ((rc = C.flush())) return rc;
        ++T.copies;

        LoopDev D{};
        D.K = K, D.n1 = n1, D.N2 = (int)N2, D.rows_a = (int)E, D.rows_all = (int)R;
        for (int l = 0; l < num_levels; ++l) D.inv_level_sigma_sq[l] = inv_level_sigma_sq[l];
        std::memcpy(D.pose_1w, pose_1w, sizeof D.pose_1w);
        D.xy1 = Y.xy1, D.octave1 = Y.octave1, D.pos_w1 = Y.pos_w1, D.has_lm1 = Y.has_lm1, D.min1 = Y.min1, D.max1 = Y.max1;
        D.xy2 = Y.xy2, D.octave2 = Y.octave2, D.pos_w2 = Y.pos_w2, D.has_lm2 = Y.has_lm2, D.min2 = Y.min2, D.max2 = Y.max2;
        D.kf2_off = Y.kf2_off, D.pose_in_cand = Y.pose_in_cand, D.pose_2w = Y.pose_2w, D.rot_12 = Y.rot_12, D.trans_12 = Y.trans_12;
        D.active = Y.active, D.scale_in = Y.scale_in, D.prob = (Sim3OptProblem*)Y.prob.p, D.reproj_tab = (const ReprojProblem*)Y.reproj_tab.p;
        D.prior_state = Y.prior_state, D.prior_idx2 = Y.prior_idx2, D.prior_pos_w = Y.prior_pos_w;
        D.ratio_bits = Y.ratio_bits, D.xf = Y.xf, D.live = Y.live, D.already2 = Y.already2;
        D.visible = Y.visible, D.q_xy = Y.q_xy, D.q_margin = Y.q_margin, D.q_min_level = Y.q_min_level, D.q_max_level = Y.q_max_level;
        D.obs1 = Y.obs1, D.obs2 = Y.obs2, D.pos1 = Y.pos1, D.pos2 = Y.pos2, D.w1 = Y.w1, D.w2 = Y.w2;
        D.scale = Y.scale, D.code = Y.code, D.match_a = Y.match_a, D.match_b = Y.match_b, D.mutual = Y.mutual, D.num_mutual = Y.num_mutual;
        D.num_edges = Y.num_edges, D.edge_idx1 = Y.edge_idx1, D.edge_idx2 = Y.edge_idx2, D.edge_status = Y.edge_status;

        const int keypoints = (int)(N2 + (size_t)n1);
        const GridProblem* const set_tab = (const GridProblem*)Y.grid_tab.p;
        const GridProblem* const row_tab = set_tab + K + 1;
        bool again = false;
        SV_HIP(ctx, hipMemsetAsync(Y.cell_cnt.p, 0, Y.cell_cnt.bytes(), C.s));
        ++T.copies;
        {
            SvProfScope ps(ctx, C.s, "k_loop_scale");
            hipLaunchKernelGGL(k_loop_scale, dim3(K), dim3(1024), 0, C.s, D);
            ++T.launches;
        }
        if (keypoints > 0) {
            SvProfScope ps(ctx, C.s, "k_loop_bin");  // count, scan, place
            T.add(sv_launch_grid_sets(C.s, set_tab, Y.set_base, K + 1, keypoints, Y.cell_cnt, (int)(((size_t)K + 1) * ncell)));
        }
        if (R > 0) {
            {
                SvProfScope ps(ctx, C.s, "k_loop_reproject");
                hipLaunchKernelGGL(k_loop_reproject, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, C.s, D);
                ++T.launches;
            }
            SvProfScope ps(ctx, C.s, "k_loop_walk");  // list sizes and their scan here, the lists below
            T.add(sv_launch_grid_queries_batch(C.s, row_tab, Y.row_base, 2 * K, (int)R, Y.cand_off));
        }
        if (R > 0) {
            int32_t total = 0;
            if ((rc = C.read_now(&total, Y.cand_off.p + R))) return rc;
            ++T.copies, ++T.syncs;
            if (total < 0) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_loop_sim3_batch: candidate lists do not fit int32");
            if ((size_t)total > H.cap) {  // nothing of the lists was written: the same call with longer ones
                H.cap = (size_t)total;
                again = true;
            }
        }
        if (again) continue;  // (read_now synchronised: nothing enqueued still reads the arena the next attempt may replace)
        if (R > 0) {
            SvProfScope ps(ctx, C.s, "k_loop_walk");
            T.add(sv_launch_grid_fill_batch(C.s, row_tab, Y.row_base, 2 * K, (int)R, (int)std::min(H.cap, lim)));
        }
        // (without any row the replay workgroups still run: they leave every problem's count at 0)
        T.add(sv_launch_cand_batch(ctx, C.s, (const CandProblem*)Y.cand_tab.p, (const CandBatchReplay*)Y.replay_tab.p, Y.row_base, 2 * K, (int)R, lds_bytes));
        {
            SvProfScope ps(ctx, C.s, "k_loop_edges");
            hipLaunchKernelGGL(k_loop_edges, dim3(K), dim3(1024), 0, C.s, D);
            ++T.launches;
        }
        Sim3OptDev S{};
        S.num_problems = K, S.fix_scale = fix_scale != 0, S.num_iter = num_iter, S.chi_sq = chi_sq;
        S.prob = (const Sim3OptProblem*)Y.prob.p;
        S.obs1 = Y.obs1, S.obs2 = Y.obs2, S.w1 = Y.w1, S.w2 = Y.w2, S.pos1 = Y.pos1, S.pos2 = Y.pos2;
        S.chi_cache = Y.chi_cache, S.sim3_out = Y.sim3_out, S.num_inliers = Y.num_inliers, S.status = Y.edge_status;
        S.stats = (svgpu_sim3opt_stats*)Y.stats.p;
        {
            SvProfScope ps(ctx, C.s, "k_sim3_opt");
            sv_launch_sim3opt(C.s, S);
            ++T.launches;
        }
        C.down(scale_12, Y.scale), C.down(code.data(), Y.code), C.down(matched_2_in_1, Y.match_a), C.down(matched_1_in_2, Y.match_b);
        C.down(mutual_2_in_1, Y.mutual), C.down(num_mutual, Y.num_mutual), C.down(num_edges, Y.num_edges), C.down(edge_idx1, Y.edge_idx1);
        C.down(edge_idx2, Y.edge_idx2), C.down(edge_status, Y.edge_status), C.down(sim3_12_out, Y.sim3_out), C.down(num_inliers, Y.num_inliers);
        C.down((char*)opt_stats, Y.stats);
        {
            std::vector<Downloads::Item> items = C.D.items;
            T.copies += (int)sv_merge_ranges(items, 32768).size();
        }
        if ((rc = C.finish())) return rc;
        ++T.syncs;
        // ---- host out: the decision (:585) on what the optimiser returned
        for (int p = 0; p < K; ++p) {
            if (code[p] != 0) {  // the optimiser saw no edge of this candidate: nothing it reports belongs to it
                status[p] = code[p] < 0 ? -1 : SVGPU_LOOP_NO_SCALE;
                num_inliers[p] = 0;
                if (opt_stats) opt_stats[p] = svgpu_sim3opt_stats{};
                continue;
            }
            status[p] = num_inliers[p] < min_num_inliers ? SVGPU_LOOP_FEW_INLIERS : 0;
        }
        if (stats) *stats = svgpu_call_stats{T.launches, T.copies, T.syncs};
        return SVGPU_OK;
    }
    return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_loop_sim3_batch: candidate lists kept outgrowing their capacity");
}
