// svgpu_fuse_landmarks_batch: mapping_module::fuse_landmark_duplication (mapping_module.cc:417-537) in one staged call -- per target
// fuse::detect_duplication of the current keyframe's landmarks on the CURRENT landmark table, then the replace / connect_to_keyframe /
// refresh bookkeeping on the device, and the backward pass at the end.  Everything is uploaded once; the keyframes are binned once; a
// snapshot pass counts the candidates of every pass for the lists' capacity (the first synchronisation); the passes then run in stream
// order, eight launches each, with no host synchronisation between them.  DESIGN section 23.
#include <algorithm>
#include <cstring>
#include <unordered_set>
#include <vector>

#include "sv_staged_call.h"
#include "frame_device.h"
#include "fuse_layout.h"
#include "match_device.h"
#include "match_kernels.h"

namespace {

using svmd::hamming256;

struct FuseKf {  // one keyframe slot, in device memory
    const uint32_t* desc;
    const float* xy;
    const int32_t* octave;
    const float* xright;  // nullable
    int32_t* kp_lm;
    int32_t n, observer;
};
struct FuseTab {  // the landmark table, the observers and the keyframe records (device pointers)
    int L;
    float inv_sf_last;
    const double* pos_w;
    const double* ref_twc;
    const float* ref_sf;
    const int32_t* obs_off;
    const int32_t* obs_cap;
    uint8_t* alive;
    uint32_t* desc;
    double* mean_normal;
    float* min_d;
    float* max_d;
    uint8_t* has_desc;
    uint8_t* has_geom;
    int32_t* obs_cnt;
    int32_t* obs_observer;
    int32_t* obs_kp;
    uint32_t* obs_desc;
    int32_t* obs_weight;
    int32_t* replaced_by;
    const int32_t* observer_rank;
    const int32_t* observer_kf;
    const double* observer_twc;
    const FuseKf* kfs;
    int32_t* flag;
};
struct FusePass {  // one detect_duplication + update: the checked list into keyframe slot `kf`
    int kf, n, cap, chi_gate;
    const int32_t* list;
    float inv_level_sigma_sq[16];
    const uint8_t* visible;
    const double* reproj;
    const float* x_right;
    const int32_t* cand_off;
    const int32_t* cand_idx;
    uint32_t* dist;
    int* owner;
    int* match;
    int32_t* hit_lm;
    int32_t* touch;
    int32_t* best_out;
    uint8_t* event_out;
    int32_t* num_fused_out;
};

__device__ __forceinline__ int fuse_find_obs(const FuseTab& T, int l, int o) {
    const int off = T.obs_off[l], cnt = T.obs_cnt[l];
    for (int e = 0; e < cnt; ++e)
        if (T.obs_observer[off + e] == o) return e;
    return -1;
}
__device__ __forceinline__ int fuse_num_observations(const FuseTab& T, int l) {  // landmark::num_observations(): stereo observations count twice
    const int off = T.obs_off[l], cnt = T.obs_cnt[l];
    int s = 0;
    for (int e = 0; e < cnt; ++e) s += T.obs_weight[off + e];
    return s;
}
// observations_[keyfrm] = idx in map order (ascending observer rank); add_observation clears both flags (data/landmark.cc:106-122)
__device__ bool fuse_insert_obs(const FuseTab& T, int l, int o, int kp, const uint32_t* __restrict__ d8, int w) {
    const int off = T.obs_off[l], cnt = T.obs_cnt[l];
    if (cnt >= T.obs_cap[l]) {
        atomicExch(T.flag, 1);
        return false;
    }
    const int r = T.observer_rank[o];
    int pos = cnt;
    while (pos > 0 && T.observer_rank[T.obs_observer[off + pos - 1]] > r) {
        const int a = off + pos, b = a - 1;
        T.obs_observer[a] = T.obs_observer[b], T.obs_kp[a] = T.obs_kp[b], T.obs_weight[a] = T.obs_weight[b];
#pragma unroll
        for (int k = 0; k < 8; ++k) T.obs_desc[(size_t)a * 8 + k] = T.obs_desc[(size_t)b * 8 + k];
        --pos;
    }
    const int a = off + pos;
    T.obs_observer[a] = o, T.obs_kp[a] = kp, T.obs_weight[a] = w;
#pragma unroll
    for (int k = 0; k < 8; ++k) T.obs_desc[(size_t)a * 8 + k] = d8[k];
    T.obs_cnt[l] = cnt + 1;
    T.has_desc[l] = 0, T.has_geom[l] = 0;
    return true;
}
// landmark::compute_descriptor (data/landmark.cc:199-254): the first observation whose row of the k x k Hamming matrix has the smallest
// lower median; the median by counting, as k_lm_median does (landmark_kernels.hip), in list order
__device__ void fuse_refresh_descriptor(const FuseTab& T, int l) {
    const int off = T.obs_off[l], k = T.obs_cnt[l];
    if (k <= 0) return;
    const int m = (int)(unsigned)(0.5 * (k - 1));
    unsigned best_median = 256;
    int best = 0;
    for (int i = 0; i < k; ++i) {
        uint32_t a[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) a[w] = T.obs_desc[(size_t)(off + i) * 8 + w];
        int lo = 0, hi = 256;
        while (lo < hi) {
            const int v = (lo + hi) >> 1;
            int cnt = 0;
            for (int j = 0; j < k; ++j) cnt += (int)hamming256(a, T.obs_desc + (size_t)(off + j) * 8) <= v;
            if (cnt >= m + 1) hi = v;
            else lo = v + 1;
        }
        if ((unsigned)lo < best_median) best_median = (unsigned)lo, best = i;
    }
#pragma unroll
    for (int w = 0; w < 8; ++w) T.desc[(size_t)l * 8 + w] = T.obs_desc[(size_t)(off + best) * 8 + w];
    T.has_desc[l] = 1;
}
// landmark::update_mean_normal_and_obs_scale_variance (data/landmark.cc:256-318): the expressions of k_lm_geometry, in list order by this lane
__device__ void fuse_refresh_geometry(const FuseTab& T, int l) {
    const int off = T.obs_off[l], k = T.obs_cnt[l];
    const double p0 = T.pos_w[3 * l], p1 = T.pos_w[3 * l + 1], p2 = T.pos_w[3 * l + 2];
    double m0 = 0.0, m1 = 0.0, m2 = 0.0;
    for (int e = 0; e < k; ++e) {
        const double* c = T.observer_twc + 3 * (size_t)T.obs_observer[off + e];
        const double v0 = p0 - c[0], v1 = p1 - c[1], v2 = p2 - c[2];
        const double sq = (v0 * v0 + v1 * v1) + v2 * v2;
        if (sq > 0.0) {
            const double nr = sqrt(sq);
            m0 = m0 + v0 / nr, m1 = m1 + v1 / nr, m2 = m2 + v2 / nr;
        }
        else m0 = m0 + v0, m1 = m1 + v1, m2 = m2 + v2;
    }
    const double sq = (m0 * m0 + m1 * m1) + m2 * m2;
    if (sq > 0.0) {
        const double nr = sqrt(sq);
        m0 = m0 / nr, m1 = m1 / nr, m2 = m2 / nr;
    }
    T.mean_normal[3 * l] = m0, T.mean_normal[3 * l + 1] = m1, T.mean_normal[3 * l + 2] = m2;
    const double w0 = p0 - T.ref_twc[3 * l], w1 = p1 - T.ref_twc[3 * l + 1], w2 = p2 - T.ref_twc[3 * l + 2];
    const double dist = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
    const float mx = (float)(dist * T.ref_sf[l]);
    T.max_d[l] = mx;
    T.min_d[l] = mx * T.inv_sf_last;
    T.has_geom[l] = 1;
}

// mapping_module.cc:436-456 for checked row i: the duplicate recorded at detection time
__device__ void fuse_do_duplicate(const FuseTab& T, const FusePass& P, int i) {
    const int A = P.list[i], B = P.hit_lm[i];
    if (A == B) {
        P.event_out[i] = SVGPU_FUSE_SAME_ID;
        return;
    }
    if (!T.alive[A] || !T.alive[B]) {
        P.event_out[i] = SVGPU_FUSE_SKIPPED;
        return;
    }
    int S = A, X = B;
    if (fuse_num_observations(T, A) < fuse_num_observations(T, B)) S = B, X = A;  // :442
    P.event_out[i] = S == A ? SVGPU_FUSE_DUP_SURVIVED : SVGPU_FUSE_DUP_LOST;
    // landmark::replace (data/landmark.cc:382-414): every keypoint of the loser lets go of it, then the survivor takes the observations it has none of
    const int off = T.obs_off[X], cnt = T.obs_cnt[X];
    for (int e = 0; e < cnt; ++e) {
        const int o = T.obs_observer[off + e], kp = T.obs_kp[off + e], kf = T.observer_kf[o];
        if (kf >= 0) T.kfs[kf].kp_lm[kp] = -1;
        if (fuse_find_obs(T, S, o) >= 0) continue;
        if (!fuse_insert_obs(T, S, o, kp, T.obs_desc + (size_t)(off + e) * 8, T.obs_weight[off + e])) return;
        if (kf >= 0) T.kfs[kf].kp_lm[kp] = S;
    }
    T.alive[X] = 0;
    T.obs_cnt[X] = 0;
    T.replaced_by[X] = S;
    if (!T.has_desc[S]) fuse_refresh_descriptor(T, S);
    if (!T.has_geom[S]) fuse_refresh_geometry(T, S);
}
// mapping_module.cc:458-467 for checked row i
__device__ void fuse_do_connection(const FuseTab& T, const FusePass& P, int i) {
    int S = P.list[i];
    for (int hop = 0; hop < T.L && T.replaced_by[S] >= 0; ++hop) S = T.replaced_by[S];  // :461-463
    const FuseKf& F = T.kfs[P.kf];
    const int t = P.match[i], o = F.observer;
    const int w = (F.xright && 0.f <= F.xright[t]) ? 2 : 1;
    P.event_out[i] = SVGPU_FUSE_NEW_CONNECTION;
    F.kp_lm[t] = S;  // keyfrm->add_landmark
    const int e = fuse_find_obs(T, S, o);
    if (e >= 0) {  // observations_[keyfrm] = idx on an existing key
        const int a = T.obs_off[S] + e;
        T.obs_kp[a] = t;
        T.obs_weight[a] += w;
        for (int k = 0; k < 8; ++k) T.obs_desc[(size_t)a * 8 + k] = F.desc[(size_t)t * 8 + k];
        T.has_desc[S] = 0, T.has_geom[S] = 0;
    }
    else if (!fuse_insert_obs(T, S, o, t, F.desc + (size_t)t * 8, w)) return;
    fuse_refresh_geometry(T, S);
    fuse_refresh_descriptor(T, S);
}

__global__ void __launch_bounds__(256) k_fuse_init(FuseTab T, int32_t* best, uint8_t* event, int n_out, int32_t* num_fused, int32_t* total0, int passes) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g < T.L) T.replaced_by[g] = -1;
    if (g < n_out) best[g] = -1, event[g] = SVGPU_FUSE_NONE;
    if (g < passes) num_fused[g] = 0, total0[g] = 0;
    if (g == 0) *T.flag = 0;
}

// fuse.cc:26-74 for every checked row: validity on the current table, reprojection, gates, predicted level and the window
__global__ void __launch_bounds__(256) k_fuse_reproject(ReprojProblem R, FuseTab T, const int32_t* __restrict__ list, int observer) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R.n || *T.flag) return;
    const int l = list[i];
    const bool offered = l >= 0 && T.alive[l] && fuse_find_obs(T, l, observer) < 0;
    const int s = offered ? l : 0;
    const bool any = T.L > 0;
    svfd::ReprojOut o;
    svfd::reproject_one(R, R.rot_cw, R.trans_cw, R.trans_wc, offered && any, any ? T.pos_w[3 * s] : 0.0, any ? T.pos_w[3 * s + 1] : 0.0, any ? T.pos_w[3 * s + 2] : 0.0,
                        any ? T.mean_normal[3 * s] : 0.0, any ? T.mean_normal[3 * s + 1] : 0.0, any ? T.mean_normal[3 * s + 2] : 0.0, any ? T.min_d[s] : 0.f,
                        any ? T.max_d[s] : 0.f, 0, false, o);
    R.visible[i] = o.vis ? 1 : 0;
    R.reproj[2 * i] = o.vis ? o.rx : 0.0;
    R.reproj[2 * i + 1] = o.vis ? o.ry : 0.0;
    R.x_right[i] = o.vis ? o.xr : 0.f;
    svfd::reproject_window(R, o, R.q_xy[2 * i], R.q_xy[2 * i + 1], R.q_margin[i], R.q_min_level[i], R.q_max_level[i]);
}

// fuse.cc:86-128 per candidate: the chi-square gate (the expressions of cand_dist_body, match_kernels.hip) and the Hamming distance; an
// entry that cannot be a best (d > HAMMING_DIST_THR_LOW) is gated.  One wave per row.  A pass whose lists outgrew the arena raises the flag.
__global__ void __launch_bounds__(256) k_fuse_dist(FuseTab T, FusePass P) {
    if (*T.flag) return;
    const int total = P.cand_off[P.n];
    if (total > P.cap) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicExch(T.flag, 1);
        return;
    }
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= P.n || !P.visible[q]) return;
    const FuseKf& F = T.kfs[P.kf];
    const uint32_t* qdp = T.desc + (size_t)P.list[q] * 8;
    uint32_t qd[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) qd[k] = qdp[k];
    for (int c = P.cand_off[q] + lane; c < P.cand_off[q + 1]; c += 64) {
        const int t = P.cand_idx[c];
        bool gated = false;
        if (P.chi_gate) {
            const double e_x = P.reproj[2 * q] - (double)F.xy[2 * t], e_y = P.reproj[2 * q + 1] - (double)F.xy[2 * t + 1];
            const double inv_sigma_sq = (double)P.inv_level_sigma_sq[(unsigned)F.octave[t]];
            if (F.xright && F.xright[t] >= 0.f) {
                const float e_xr = P.x_right[q] - F.xright[t];
                const double err = (e_x * e_x + e_y * e_y) + (double)(e_xr * e_xr);
                if ((double)7.81473f < err * inv_sigma_sq) gated = true;
            }
            else {
                const double err = e_x * e_x + e_y * e_y;
                if ((double)5.99146f < err * inv_sigma_sq) gated = true;
            }
        }
        uint32_t e = 0xFFFFFFFFu;
        if (!gated) {
            const unsigned d = hamming256(qd, F.desc + (size_t)t * 8);
            if (d <= svmd::HAMMING_DIST_THR_LOW) e = (d << 22) | (uint32_t)t;
        }
        P.dist[c] = e;
    }
}

// One workgroup per pass: the fixed-point replay of the greedy claims (best only: the first smallest distance in scan order among the
// keypoints no earlier row holds; the sweeps of cand_replay_body, match_kernels.hip) and what every hit found at its keypoint; then, as a
// launch of its own (one kernel holds both halves' pointers live at once only by spilling scalar registers), the update of the table.
__device__ __forceinline__ int fuse_decide(const FusePass& P, int q) {
    if (!P.visible[q]) return -1;
    unsigned best = svmd::MAX_HAMMING_DIST;
    int best_idx = -1;
    for (int c = P.cand_off[q]; c < P.cand_off[q + 1]; ++c) {
        const uint32_t e = P.dist[c];
        if (e == 0xFFFFFFFFu) continue;
        const int t = (int)(e & 0x3FFFFFu);
        if (P.owner[t] < q) continue;
        const unsigned d = e >> 22;
        if (d < best) best = d, best_idx = t;
    }
    return best_idx;
}
__global__ void __launch_bounds__(1024) k_fuse_replay(FuseTab T, FusePass P) {
    __shared__ int s_changed, s_count;
    if (*T.flag) return;
    const int tid = threadIdx.x, n = P.n;
    const FuseKf& F = T.kfs[P.kf];
    const int nt = F.n;
    for (int t = tid; t < nt; t += 1024) P.owner[t] = 0x7FFFFFFF;
    for (int q = tid; q < n; q += 1024) P.match[q] = -2;
    for (int l = tid; l < T.L; l += 1024) P.touch[l] = 0;
    if (tid == 0) s_changed = 0, s_count = 0;
    __syncthreads();
    for (int sweep = 0; sweep <= n; ++sweep) {
        int local_changed = 0;
        for (int q = tid; q < n; q += 1024) {
            const int d = fuse_decide(P, q);
            if (d != P.match[q]) local_changed = 1;
            P.match[q] = d;
        }
        if (local_changed) s_changed = 1;
        __syncthreads();
        if (!s_changed) break;
        for (int t = tid; t < nt; t += 1024) P.owner[t] = 0x7FFFFFFF;
        __syncthreads();
        if (tid == 0) s_changed = 0;
        for (int q = tid; q < n; q += 1024)
            if (P.match[q] >= 0) atomicMin(&P.owner[P.match[q]], q);
        __syncthreads();
    }
    // fuse.cc:135-148: what the claimed keypoint holds at detection time; the landmarks every hit will touch
    int local = 0;
    for (int i = tid; i < n; i += 1024) {
        const int b = P.match[i];
        P.best_out[i] = b;
        int hit = -1;
        if (b >= 0) {
            ++local;
            const int A = P.list[i], B = F.kp_lm[b];
            if (B < 0) hit = -2, atomicAdd(&P.touch[A], 1);
            else if (!T.alive[B]) hit = -3;
            else {
                hit = B;
                atomicAdd(&P.touch[A], 1);
                if (B != A) atomicAdd(&P.touch[B], 1);
            }
        }
        P.hit_lm[i] = hit;
    }
    if (local) atomicAdd(&s_count, local);
    __syncthreads();
    if (tid == 0) *P.num_fused_out = s_count;
}
// CONN = false: the duplicates (:436-456); true: the new connections (:458-467), behind them on the stream
template <bool CONN>
__global__ void __launch_bounds__(1024) k_fuse_update(FuseTab T, FusePass P) {
    __shared__ int s_conflict;
    if (*T.flag) return;
    const int tid = threadIdx.x, n = P.n;
    if (tid == 0) s_conflict = 0;
    __syncthreads();
    for (int l = tid; l < T.L; l += 1024)
        if (P.touch[l] > 1) s_conflict = 1;
    __syncthreads();
    // Hits touch disjoint landmarks and keypoints when kp_lm and the observation lists agree: one lane per hit.  Otherwise (a checked
    // landmark that is also the kp_lm of another hit) one lane takes them in ascending list index.
    const int start = s_conflict ? (tid == 0 ? 0 : n) : tid, step = s_conflict ? 1 : 1024;
    for (int i = start; i < n; i += step) {
        if (!CONN && P.hit_lm[i] >= 0) fuse_do_duplicate(T, P, i);
        if (CONN && P.hit_lm[i] == -2) fuse_do_connection(T, P, i);
    }
}

inline void cam_center(const double* R, const double* t, double* c) {  // fuse.cc:20, as svgpu_match2.hip writes it
    for (int i = 0; i < 3; ++i) c[i] = ((-R[i]) * t[0] + (-R[3 + i]) * t[1]) + (-R[6 + i]) * t[2];
}

}  // namespace

extern "C" int svgpu_fuse_landmarks_batch(svgpu_ctx* ctx, int num_targets, const svgpu_fuse_keyframe* keyframes, int num_observers,
                                          const int32_t* observer_rank, const double* observer_trans_wc, const svgpu_fuse_table* table, int n_fwd,
                                          const int32_t* fwd_list, int n_bwd, const int32_t* bwd_list, int num_levels, const float* scale_factors,
                                          const float* inv_level_sigma_sq, float log_scale_factor, float inv_scale_factor_last, float margin,
                                          int do_reprojection_matching, int32_t* best_idx, uint8_t* event, int32_t* num_fused, svgpu_call_stats* stats) {
    const char* who = "svgpu_fuse_landmarks_batch: bad arguments";
    const int K = num_targets;
    if (!ctx || K < 0) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    if (K == 0) {
        if (stats) *stats = svgpu_call_stats{0, 0, 0};
        return SVGPU_OK;
    }
    if (!keyframes || !table || num_observers < 1 || !observer_rank || !observer_trans_wc || n_fwd < 0 || n_bwd < 0 || (n_fwd > 0 && !fwd_list)
        || (n_bwd > 0 && !bwd_list) || num_levels < 1 || num_levels > SV_MAX_LEVELS || !scale_factors || !inv_level_sigma_sq || !(log_scale_factor > 0.f)
        || !num_fused || ((size_t)K * n_fwd + n_bwd > 0 && (!best_idx || !event)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    const svgpu_fuse_table& Tb = *table;
    const int L = Tb.num_landmarks, E = Tb.num_entries, O = num_observers;
    if (L < 0 || E < 0
        || (L > 0 && (!Tb.pos_w || !Tb.ref_trans_wc || !Tb.ref_scale_factor || !Tb.obs_off || !Tb.obs_cap || !Tb.alive || !Tb.descriptor || !Tb.mean_normal
                      || !Tb.min_valid_dist || !Tb.max_valid_dist || !Tb.has_descriptor || !Tb.has_geometry || !Tb.obs_cnt || !Tb.replaced_by))
        || (E > 0 && (!Tb.obs_observer || !Tb.obs_kp || !Tb.obs_desc || !Tb.obs_weight)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    const size_t lim = (size_t)INT32_MAX;
    FuseShape S;
    std::vector<int32_t> observer_kf((size_t)O, -1);
    size_t N = 0;
    for (int u = 0; u <= K; ++u) {
        const svgpu_fuse_keyframe& f = keyframes[u];
        if (!f.cam || f.cam->model < SVGPU_CAM_PERSPECTIVE || f.cam->model > SVGPU_CAM_RADIAL_DIVISION || !f.rot_cw || !f.trans_cw || f.n < 0 || f.n > 8192
            || f.grid_cols < 1 || f.grid_rows < 1 || (size_t)f.grid_cols * f.grid_rows > 4096 || !(f.cam->min_x < f.cam->max_x) || !(f.cam->min_y < f.cam->max_y)
            || f.observer < 0 || f.observer >= O || observer_kf[f.observer] >= 0 || (f.n > 0 && (!f.desc || !f.xy || !f.octave || !f.kp_lm)))
            return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
        observer_kf[f.observer] = u;
        for (int i = 0; i < f.n; ++i)
            if (f.octave[i] < 0 || f.octave[i] >= num_levels || f.kp_lm[i] < -1 || f.kp_lm[i] >= L) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
        S.kf_n.push_back(f.n), S.kf_xright.push_back(f.xright != nullptr), S.kf_cells.push_back(f.grid_cols * f.grid_rows);
        N += (size_t)f.n;
    }
    {
        std::unordered_set<int32_t> ranks;
        for (int o = 0; o < O; ++o)
            if (!ranks.insert(observer_rank[o]).second) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
        std::vector<uint8_t> used((size_t)E, 0);
        std::unordered_set<uint64_t> seen;
        for (int l = 0; l < L; ++l) {
            const int off = Tb.obs_off[l], cap = Tb.obs_cap[l], cnt = Tb.obs_cnt[l];
            if (off < 0 || cap < 0 || cap > FUSE_OBS_CAP_MAX || cnt < 0 || cnt > cap || (size_t)off + (size_t)cap > (size_t)E) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
            for (int e = off; e < off + cap; ++e) {
                if (used[e]) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);  // overlapping ranges
                used[e] = 1;
            }
            for (int e = off; e < off + cnt; ++e) {
                const int o = Tb.obs_observer[e], kp = Tb.obs_kp[e];
                if (o < 0 || o >= O || kp < 0 || Tb.obs_weight[e] < 1 || Tb.obs_weight[e] > 2) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
                if (observer_kf[o] >= 0 && kp >= keyframes[observer_kf[o]].n) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
                if (e > off && observer_rank[Tb.obs_observer[e - 1]] >= observer_rank[o]) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);  // map order
                if (!seen.insert(((uint64_t)(uint32_t)o << 32) | (uint32_t)kp).second) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);  // one landmark per keypoint
            }
        }
        std::vector<uint8_t> in_bwd((size_t)L, 0);
        for (int i = 0; i < n_fwd; ++i)
            if (fwd_list[i] < -1 || fwd_list[i] >= L) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
        for (int i = 0; i < n_bwd; ++i) {
            if (bwd_list[i] < 0 || bwd_list[i] >= L || in_bwd[bwd_list[i]]) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
            in_bwd[bwd_list[i]] = 1;
        }
    }
    const size_t n_out = (size_t)K * n_fwd + n_bwd;
    if (N * 32 > lim || (size_t)E * 32 > lim || n_out > lim || (size_t)L * 32 > lim) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    S.num_observers = (size_t)O, S.num_landmarks = (size_t)L, S.num_entries = (size_t)E, S.n_fwd = (size_t)n_fwd, S.n_bwd = (size_t)n_bwd;
    S.kf_rec = sizeof(FuseKf), S.grid_rec = sizeof(GridProblem);

    struct Tally {
        int launches = 0, copies = 0, syncs = 0;
        void add(const SvIssued& n) { launches += n.launches, copies += n.copies; }
    } Tl;
    auto report = [&]() {
        if (stats) *stats = svgpu_call_stats{Tl.launches, Tl.copies, Tl.syncs};
    };
    const int passes = K + 1;
    FusePieces Y;
    std::vector<FuseKf> kf_tab((size_t)K + 1);
    std::vector<GridProblem> grids((size_t)K + 1);
    FuseTab T{};
    bool lists = false;
    size_t cap = 0;
    auto layout = [&](UploadArena& A) {
        fuse_layout(A, S, lists, cap, Y);
        for (int u = 0; u <= K; ++u) {
            const svgpu_fuse_keyframe& f = keyframes[u];
            const size_t a = Y.first[u];
            FuseKf& F = kf_tab[u];
            F.desc = Y.desc.p ? (const uint32_t*)(Y.desc.p + a * 32) : nullptr;
            F.xy = Y.xy.p ? Y.xy.p + a * 2 : nullptr;
            F.octave = Y.octave.p ? Y.octave.p + a : nullptr;
            F.xright = (f.xright && Y.xright.p) ? Y.xright.p + Y.first_xr[u] : nullptr;
            F.kp_lm = Y.kp_lm.p ? Y.kp_lm.p + a : nullptr;
            F.n = f.n, F.observer = f.observer;
            GridProblem& G = grids[u];
            G = GridProblem{};
            G.t_xy = F.xy, G.t_octave = F.octave, G.nt = f.n, G.min_x = f.cam->min_x, G.min_y = f.cam->min_y;
            G.inv_w = (double)f.grid_cols / (f.cam->max_x - f.cam->min_x);
            G.inv_h = (double)f.grid_rows / (f.cam->max_y - f.cam->min_y);
            G.cols = f.grid_cols, G.rows = f.grid_rows;
            G.cell_of = Y.cell_of.p ? Y.cell_of.p + a : nullptr;
            G.cell_off = Y.cell_off.p ? Y.cell_off.p + Y.first_cell[u] : nullptr;
            G.cell_items = Y.cell_items.p ? Y.cell_items.p + a : nullptr;
            G.q_xy = Y.q_xy, G.q_margin = Y.q_margin, G.q_min_level = Y.q_min_level, G.q_max_level = Y.q_max_level, G.q_valid = Y.visible;
            G.cand_off = Y.cand_off, G.cand_idx = Y.cand_idx, G.cap = (int)cap;
        }
        T.L = L, T.inv_sf_last = inv_scale_factor_last;
        T.pos_w = Y.pos_w, T.ref_twc = Y.ref_twc, T.ref_sf = Y.ref_sf, T.obs_off = Y.obs_off, T.obs_cap = Y.obs_cap, T.alive = Y.alive;
        T.desc = (uint32_t*)Y.lm_desc.p, T.mean_normal = Y.mean_normal, T.min_d = Y.min_d, T.max_d = Y.max_d, T.has_desc = Y.has_desc, T.has_geom = Y.has_geom;
        T.obs_cnt = Y.obs_cnt, T.obs_observer = Y.obs_observer, T.obs_kp = Y.obs_kp, T.obs_desc = (uint32_t*)Y.obs_desc.p, T.obs_weight = Y.obs_weight;
        T.replaced_by = Y.replaced_by, T.observer_rank = Y.observer_rank, T.observer_kf = Y.observer_kf, T.observer_twc = Y.observer_twc;
        T.kfs = (const FuseKf*)Y.kf_tab.p, T.flag = Y.flag;
    };
    StagedCall C;
    // the checked list of pass p (p < K: the forward list into slot p + 1; p == K: the backward list into slot 0)
    auto pass_slot = [&](int p) { return p < K ? p + 1 : 0; };
    auto pass_n = [&](int p) { return p < K ? n_fwd : n_bwd; };
    auto pass_list = [&](int p) -> const int32_t* { return p < K ? Y.fwd_list.p : Y.bwd_list.p; };
    auto reproject = [&](int p) {  // validity, reprojection and windows of pass p on the table as it stands; then the list sizes and their scan
        const int u = pass_slot(p), n = pass_n(p);
        const svgpu_fuse_keyframe& f = keyframes[u];
        ReprojProblem R{};
        R.cam = *f.cam;
        std::memcpy(R.rot_cw, f.rot_cw, sizeof R.rot_cw);
        std::memcpy(R.trans_cw, f.trans_cw, sizeof R.trans_cw);
        cam_center(f.rot_cw, f.trans_cw, R.trans_wc);
        R.n = n, R.ray_cos_thr = 0.5f, R.num_levels = (unsigned)num_levels, R.log_scale_factor = log_scale_factor, R.margin = margin;
        for (int l = 0; l < num_levels; ++l) R.scale_factors[l] = scale_factors[l];
        R.dist_mode = 1, R.normal_mode = 1, R.center_mode = 0, R.window_mode = 0;
        R.visible = Y.visible, R.reproj = Y.reproj, R.x_right = Y.x_right;
        R.q_xy = Y.q_xy, R.q_margin = Y.q_margin, R.q_min_level = Y.q_min_level, R.q_max_level = Y.q_max_level;
        hipLaunchKernelGGL(k_fuse_reproject, dim3((n + 255) / 256), dim3(256), 0, C.s, R, T, pass_list(p), f.observer);
        ++Tl.launches;
        GridProblem G = grids[u];
        G.nq = n;
        Tl.add(sv_launch_grid_queries(C.s, G));
    };
    auto worth = [&](int p) { return pass_n(p) > 0 && keyframes[pass_slot(p)].n > 0 && L > 0; };
    auto count = [&](bool snapshot) -> int {  // one upload of everything, the grids, and (first time) the snapshot counts of every pass
        for (int u = 0; u <= K; ++u) {
            const svgpu_fuse_keyframe& f = keyframes[u];
            const size_t a = Y.first[u], n = (size_t)f.n;
            C.up(Y.desc.p + a * 32, f.desc, n * 32), C.up(Y.xy.p + a * 2, f.xy, n * 2), C.up(Y.octave.p + a, f.octave, n), C.up(Y.kp_lm.p + a, (const int32_t*)f.kp_lm, n);
            if (f.xright) C.up(Y.xright.p + Y.first_xr[u], f.xright, n);
        }
        C.up(Y.kf_tab, (const char*)kf_tab.data());
        C.up(Y.observer_rank, observer_rank, Y.observer_kf, (const int32_t*)observer_kf.data(), Y.observer_twc, observer_trans_wc);
        C.up(Y.pos_w, Tb.pos_w, Y.ref_twc, Tb.ref_trans_wc, Y.ref_sf, Tb.ref_scale_factor, Y.obs_off, Tb.obs_off, Y.obs_cap, Tb.obs_cap);
        C.up(Y.alive, (const uint8_t*)Tb.alive, Y.lm_desc, (const uint8_t*)Tb.descriptor, Y.mean_normal, (const double*)Tb.mean_normal);
        C.up(Y.min_d, (const float*)Tb.min_valid_dist, Y.max_d, (const float*)Tb.max_valid_dist, Y.has_desc, (const uint8_t*)Tb.has_descriptor);
        C.up(Y.has_geom, (const uint8_t*)Tb.has_geometry, Y.obs_cnt, (const int32_t*)Tb.obs_cnt, Y.obs_observer, (const int32_t*)Tb.obs_observer);
        C.up(Y.obs_kp, (const int32_t*)Tb.obs_kp, Y.obs_desc, (const uint8_t*)Tb.obs_desc, Y.obs_weight, (const int32_t*)Tb.obs_weight);
        C.up(Y.fwd_list, fwd_list, Y.bwd_list, bwd_list);
        int r = C.flush();
        if (r) return r;
        ++Tl.copies;
        const int g = (int)std::max<size_t>({(size_t)L, n_out, (size_t)passes, 1});
        hipLaunchKernelGGL(k_fuse_init, dim3((g + 255) / 256), dim3(256), 0, C.s, T, Y.best.p, Y.event.p, (int)n_out, Y.num_fused.p, Y.total0.p, passes);
        ++Tl.launches;
        for (int u = 0; u <= K; ++u)
            if (keyframes[u].n > 0) Tl.add(sv_launch_grid_frame(C.s, grids[u]));
        if (!snapshot) return SVGPU_OK;
        for (int p = 0; p < passes; ++p) {
            if (!worth(p)) continue;
            reproject(p);
            SV_HIP(ctx, hipMemcpyAsync(Y.total0.p + p, Y.cand_off.p + pass_n(p), sizeof(int32_t), hipMemcpyDeviceToDevice, C.s));
            ++Tl.copies;
        }
        return SVGPU_OK;
    };
    int rc = C.open(ctx, "svgpu_fuse_landmarks_batch: internal arena overflow", layout);
    if (!rc) rc = count(true);
    std::vector<int32_t> total0((size_t)passes, 0);
    if (!rc) {
        SV_HIP(ctx, hipMemcpyAsync(total0.data(), Y.total0.p, sizeof(int32_t) * (size_t)passes, hipMemcpyDeviceToHost, C.s));
        SV_HIP(ctx, hipStreamSynchronize(C.s));
        ++Tl.copies, ++Tl.syncs;
    }
    report();
    if (rc) return rc;
    for (int p = 0; p < passes; ++p)
        if (total0[p] < 0) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    cap = fuse_cand_capacity(total0.data(), (size_t)passes);
    lists = true;
    bool survived = false;
    if ((rc = C.reopen(layout, survived))) return rc;
    if (!survived && (rc = count(false))) return rc;
    {
        for (int p = 0; p < passes; ++p) {
            if (!worth(p)) continue;
            const int u = pass_slot(p), n = pass_n(p);
            reproject(p);
            GridProblem G = grids[u];
            G.nq = n;
            Tl.add(sv_launch_grid_fill(C.s, G));
            FusePass P{};
            P.kf = u, P.n = n, P.cap = (int)cap, P.chi_gate = do_reprojection_matching ? 1 : 0, P.list = pass_list(p);
            for (int l = 0; l < num_levels; ++l) P.inv_level_sigma_sq[l] = inv_level_sigma_sq[l];
            P.visible = Y.visible, P.reproj = Y.reproj, P.x_right = Y.x_right, P.cand_off = Y.cand_off, P.cand_idx = Y.cand_idx, P.dist = Y.dist;
            P.owner = Y.owner, P.match = Y.match, P.hit_lm = Y.hit_lm, P.touch = Y.touch;
            const size_t o = p < K ? (size_t)p * n_fwd : (size_t)K * n_fwd;
            P.best_out = Y.best.p + o, P.event_out = Y.event.p + o, P.num_fused_out = Y.num_fused.p + p;
            hipLaunchKernelGGL(k_fuse_dist, dim3((n + 3) / 4), dim3(256), 0, C.s, T, P);
            hipLaunchKernelGGL(k_fuse_replay, dim3(1), dim3(1024), 0, C.s, T, P);
            hipLaunchKernelGGL(k_fuse_update<false>, dim3(1), dim3(1024), 0, C.s, T, P);
            hipLaunchKernelGGL(k_fuse_update<true>, dim3(1), dim3(1024), 0, C.s, T, P);
            Tl.launches += 4;
        }
    }
    // everything comes back into the mirror; the caller's arrays are written only when the chain did not overflow
    C.keep(Y.kp_lm), C.keep(Y.alive), C.keep(Y.lm_desc), C.keep(Y.mean_normal), C.keep(Y.min_d), C.keep(Y.max_d), C.keep(Y.has_desc), C.keep(Y.has_geom);
    C.keep(Y.obs_cnt), C.keep(Y.replaced_by), C.keep(Y.obs_observer), C.keep(Y.obs_kp), C.keep(Y.obs_desc), C.keep(Y.obs_weight);
    C.keep(Y.flag), C.keep(Y.best), C.keep(Y.event), C.keep(Y.num_fused);
    {
        std::vector<Downloads::Item> items = C.D.items;
        Tl.copies += (int)sv_merge_ranges(items, 32768).size();
    }
    rc = C.finish();
    ++Tl.syncs;
    report();
    if (rc) return rc;
    if (*C.host(Y.flag.p)) return SVGPU_FUSE_OVERFLOW;
    auto out = [&](auto* dst, auto piece, size_t count) {
        if (count) std::memcpy(dst, C.host(piece.p), count * sizeof(*dst));
    };
    for (int u = 0; u <= K; ++u)
        if (keyframes[u].n > 0) std::memcpy(keyframes[u].kp_lm, C.host(Y.kp_lm.p) + Y.first[u], sizeof(int32_t) * (size_t)keyframes[u].n);
    out(Tb.alive, Y.alive, (size_t)L), out(Tb.descriptor, Y.lm_desc, (size_t)L * 32), out(Tb.mean_normal, Y.mean_normal, (size_t)L * 3);
    out(Tb.min_valid_dist, Y.min_d, (size_t)L), out(Tb.max_valid_dist, Y.max_d, (size_t)L), out(Tb.has_descriptor, Y.has_desc, (size_t)L);
    out(Tb.has_geometry, Y.has_geom, (size_t)L), out(Tb.obs_cnt, Y.obs_cnt, (size_t)L), out(Tb.replaced_by, Y.replaced_by, (size_t)L);
    out(Tb.obs_observer, Y.obs_observer, (size_t)E), out(Tb.obs_kp, Y.obs_kp, (size_t)E), out(Tb.obs_desc, Y.obs_desc, (size_t)E * 32);
    out(Tb.obs_weight, Y.obs_weight, (size_t)E);
    out(best_idx, Y.best, n_out), out(event, Y.event, n_out), out(num_fused, Y.num_fused, (size_t)passes);
    return SVGPU_OK;
}
