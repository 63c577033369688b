// Kernels of the keyframe BoW database (data/bow_database.cc:58-159): candidates of relocalisation and loop detection.
// The database is a FORWARD index (per keyframe its sorted word ids), not the reference's word -> keyframe lists: one query scans every
// keyframe, a wave per keyframe, and tests each of its ids for membership in the query, whose sorted ids the workgroup holds in LDS
// (binary search; a query longer than SV_BOWDB_STAGE ids is walked in chunks, the counts / sums of a keyframe carried in global memory
// between chunks by the one wave that owns it).  Counts are integers (wave reduction, atomicMax): order does not matter.  The score of a
// survivor is a floating-point sum and IS ordered: ascending word id, one addition after another, as the sequential merge of
// fbow::BoWVector::score / DBoW2's L1Scoring::score adds them -- matched lanes of each 64-entry chunk are found by ballot and added in lane
// order by every lane alike.  No floating-point atomics.  Both scoring forms are restated from the libraries' published sources (neither
// is in the reference checkout): parity unpinned.
#include "bowdb_kernels.h"

namespace {

// index of `key` in the ascending ids sq[0 .. n), or -1
__device__ __forceinline__ int bow_find(const uint32_t* sq, int n, uint32_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sq[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && sq[lo] == key) ? lo : -1;
}

// chunk c of query q into LDS (all threads of the workgroup); returns its length
__device__ __forceinline__ int bow_stage(uint32_t* sq, const uint32_t* __restrict__ q_ids, int qb, int qn, int c) {
    const int cn = min(SV_BOWDB_STAGE, qn - c * SV_BOWDB_STAGE);
    __syncthreads();  // the readers of the previous chunk are done
    for (int i = threadIdx.x; i < cn; i += SV_BOWDB_THREADS) sq[i] = q_ids[qb + c * SV_BOWDB_STAGE + i];
    __syncthreads();
    return cn > 0 ? cn : 0;
}

__global__ void __launch_bounds__(256) k_bowdb_reject(const int32_t* __restrict__ reject_slots, int n, uint8_t* __restrict__ reject, int num_slots) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t s = reject_slots[i];
    if (0 <= s && s < num_slots) reject[s] = 1;  // (a slot listed twice: the same byte, the same value)
}

// step 1 of acquire_keyframes (compute_num_common_words, :98-129) and the maximum of :72-77
__global__ void __launch_bounds__(SV_BOWDB_THREADS) k_bowdb_count(BowdbProblem P) {
    __shared__ uint32_t sq[SV_BOWDB_STAGE];
    const int q = blockIdx.y, qb = P.q_off[q], qn = P.q_off[q + 1] - qb;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, waves = SV_BOWDB_THREADS / 64;
    const int nchunks = max(1, (qn + SV_BOWDB_STAGE - 1) / SV_BOWDB_STAGE);  // an empty query still writes its zeros
    for (int c = 0; c < nchunks; ++c) {
        const int cn = bow_stage(sq, P.q_ids, qb, qn, c);
        const uint32_t id_lo = cn ? sq[0] : 1u, id_hi = cn ? sq[cn - 1] : 0u;
        for (int slot = blockIdx.x * waves + wave; slot < P.num_slots; slot += gridDim.x * waves) {  // wave-uniform
            const BowSlot s = P.slots[slot];
            unsigned cnt = 0;
            if (cn && s.live && !P.reject[slot]) {
                const uint32_t* ids = P.pool_ids + s.off;
                for (uint32_t e = lane; e < s.len; e += 64) {
                    const uint32_t id = ids[e];
                    if (id_lo <= id && id <= id_hi) cnt += bow_find(sq, cn, id) >= 0;
                }
            }
            for (int d = 32; d; d >>= 1) cnt += __shfl_xor(cnt, d);
            if (lane == 0) {
                const size_t idx = (size_t)q * P.num_slots + slot;
                const unsigned tot = (c ? P.common[idx] : 0u) + cnt;  // written by this very lane one chunk ago
                P.common[idx] = tot;
                if (c == nchunks - 1 && tot) atomicMax(&P.max_common[q], tot);
            }
        }
    }
}

// step 2 (compute_scores, :131-159): thr from the maximum the count pass left in device memory, the ordered sum of every survivor, the
// clamp / sqrt, the min_score gate.  Items are the slots, or -- svgpu_bowdb_score -- the entries of a list, each scored if live.
__global__ void __launch_bounds__(SV_BOWDB_THREADS) k_bowdb_score(BowdbProblem P) {
    __shared__ uint32_t sq[SV_BOWDB_STAGE];
    const int q = blockIdx.y, qb = P.q_off[q], qn = P.q_off[q + 1] - qb;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, waves = SV_BOWDB_THREADS / 64;
    const int items = P.list ? P.num_list : P.num_slots;
    // static_cast<unsigned int>(num_common_words_thr_ratio * max_num_common_words), :78: a float product, truncated
    const unsigned thr = P.list ? 0u : (unsigned)(P.ratio * (float)P.max_common[q]);
    auto slot_of = [&](int i, bool& ok) -> int {
        if (!P.list) {
            ok = thr < P.common[(size_t)q * P.num_slots + i];  // strict, :143 (common > 0 implies live and not rejected)
            return i;
        }
        const int32_t s = P.list[i];
        ok = 0 <= s && s < P.num_slots && P.slots[s].live;
        return ok ? s : 0;
    };
    // what does not survive is settled now; a workgroup without survivors stages nothing
    int any = 0;
    for (int i = blockIdx.x * waves + wave; i < items; i += gridDim.x * waves) {
        bool ok;
        slot_of(i, ok);
        any |= ok;
        if (!ok && lane == 0) {
            P.keep[(size_t)q * items + i] = 0;
            P.score[(size_t)q * items + i] = -1.0f;
        }
    }
    if (!__syncthreads_or(any)) return;
    const float min_score = P.min_score[q];
    const int nchunks = max(1, (qn + SV_BOWDB_STAGE - 1) / SV_BOWDB_STAGE);
    for (int c = 0; c < nchunks; ++c) {
        const int cn = bow_stage(sq, P.q_ids, qb, qn, c);
        const double* qw = P.q_w + qb + c * SV_BOWDB_STAGE;
        for (int i = blockIdx.x * waves + wave; i < items; i += gridDim.x * waves) {  // wave-uniform
            bool ok;
            const int slot = slot_of(i, ok);
            if (!ok) continue;
            const BowSlot sl = P.slots[slot];
            const size_t idx = (size_t)q * items + i;
            double s = c ? P.sum[idx] : 0.0;  // every lane carries the same sum
            for (uint32_t e0 = 0; e0 < sl.len; e0 += 64) {
                const uint32_t e = e0 + lane;
                int j = -1;
                if (e < sl.len && cn) j = bow_find(sq, cn, P.pool_ids[sl.off + e]);
                double term = 0.0;
                if (j >= 0) {
                    const double v = qw[j], w = P.pool_w[sl.off + e];  // v: the query's weight, w: the keyframe's
                    if (P.score_form == SVGPU_BOW_SCORE_FBOW_L2) term = (double)((float)v * (float)w);  // fp32 product
                    else term = fabs(v - w) - fabs(v) - fabs(w);
                }
                unsigned long long m = __ballot(j >= 0);
                while (m) {  // ascending lane = ascending word id
                    const int b = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    s += __shfl(term, b);
                }
            }
            if (lane) continue;
            if (c < nchunks - 1) {
                P.sum[idx] = s;
                continue;
            }
            float f;
            if (P.score_form == SVGPU_BOW_SCORE_FBOW_L2) f = (float)(s >= 1.0 ? 1.0 : 1.0 - sqrt(1.0 - s));
            else f = (float)(-s / 2.0);
            P.score[idx] = f;
            P.keep[idx] = !(min_score > f);  // :147: a score equal to min_score stays
        }
    }
}

// the kept keyframes of a query in ascending slot order: one workgroup per query walks the slots 256 at a time (ballot + prefix)
__global__ void __launch_bounds__(256) k_bowdb_emit(BowdbProblem P) {
    __shared__ int wsum[4];
    const int q = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int base = 0;
    for (int t = 0; t < P.num_slots; t += 256) {
        const int i = t + threadIdx.x;
        const size_t idx = (size_t)q * P.num_slots + i;
        const bool keep = i < P.num_slots && P.keep[idx];
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int pre = 0, tot = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) pre += wsum[w];
            tot += wsum[w];
        }
        const int pos = base + pre + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && pos < P.cap) {
            const size_t o = (size_t)q * P.cap + pos;
            P.out_slots[o] = i;
            P.out_common[o] = P.common[idx];
            P.out_score[o] = P.score[idx];
        }
        base += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) P.n_out[q] = (uint32_t)base;
}

__global__ void __launch_bounds__(256) k_bowdb_move(const uint32_t* __restrict__ ids_old, const double* __restrict__ w_old, uint32_t* __restrict__ ids_new,
                                                    double* __restrict__ w_new, const uint32_t* __restrict__ moves, int m) {
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= m) return;
    const uint32_t src = moves[3 * k], dst = moves[3 * k + 1], len = moves[3 * k + 2];
    for (uint32_t e = lane; e < len; e += 64) {
        ids_new[dst + e] = ids_old[src + e];
        w_new[dst + e] = w_old[src + e];
    }
}

dim3 scan_grid(int items, int queries) {
    const int gx = std::max(1, std::min((items + 3) / 4, SV_BOWDB_MAX_GRID));
    return dim3(gx, queries);
}

}  // namespace

void sv_launch_bowdb_reject(hipStream_t s, const int32_t* reject_slots, int n, uint8_t* reject, int num_slots) {
    if (n > 0) hipLaunchKernelGGL(k_bowdb_reject, dim3((n + 255) / 256), dim3(256), 0, s, reject_slots, n, reject, num_slots);
}
void sv_launch_bowdb_count(hipStream_t s, const BowdbProblem& P) {
    hipLaunchKernelGGL(k_bowdb_count, scan_grid(P.num_slots, P.num_queries), dim3(SV_BOWDB_THREADS), 0, s, P);
}
void sv_launch_bowdb_score(hipStream_t s, const BowdbProblem& P) {
    hipLaunchKernelGGL(k_bowdb_score, scan_grid(P.list ? P.num_list : P.num_slots, P.num_queries), dim3(SV_BOWDB_THREADS), 0, s, P);
}
void sv_launch_bowdb_emit(hipStream_t s, const BowdbProblem& P) {
    hipLaunchKernelGGL(k_bowdb_emit, dim3(P.num_queries), dim3(256), 0, s, P);
}
void sv_launch_bowdb_move(hipStream_t s, const uint32_t* ids_old, const double* w_old, uint32_t* ids_new, double* w_new, const uint32_t* moves, int m) {
    if (m > 0) hipLaunchKernelGGL(k_bowdb_move, dim3((m + 3) / 4), dim3(256), 0, s, ids_old, w_old, ids_new, w_new, moves, m);
}
