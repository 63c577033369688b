// Kernels of svgpu_bow_compute_batch (bow_compute_kernels.h): what bow_vocabulary_hip::compute_bow (host/camera.cpp) does with one
// std::map insertion per descriptor, for B frames at once.  The maps' iteration order becomes a sort: per frame the composite keys
// (word << 32 | feature index) ascend, so the features of one word lie next to one another in ascending feature index, and the words in
// ascending id.  Every floating-point sum is made by ONE lane, term after term in that order -- no tree, no wave reduction, no atomics: the
// order of the additions is part of the result.
#include "bow_compute_kernels.h"

namespace {

// (b) the frame of every descriptor: the last f with d_off[f] <= i (empty frames share their offset with the next one and own nothing)
__global__ void __launch_bounds__(256) k_bowc_owner(BowComputeProblem P) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.total) return;
    int lo = 0, hi = P.num_frames;  // d_off[lo] <= i < d_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (P.d_off[mid] <= i) lo = mid;
        else hi = mid;
    }
    P.frame[i] = lo;
}

__device__ __forceinline__ unsigned long long bowc_composite(const BowComputeProblem& P, int first, int i, int which) {
    if (P.dbow2 && !(P.weight[first + i] > 0.f)) return SV_BOWC_DROPPED;  // stop words take no part, in either map
    const unsigned k = (unsigned)(which ? P.node[first + i] : P.word[first + i]);
    return ((unsigned long long)k << 32) | (unsigned)i;
}

// (c) one workgroup per frame: bitonic network over the composites in LDS, first by word, then by node key.  The composites of a frame are
// distinct (the index is part of them) but for the dropped ones, which are all equal: the order is the same whatever network sorts them.
__global__ void __launch_bounds__(256) k_bowc_sort_lds(BowComputeProblem P) {
    extern __shared__ unsigned long long s_v[];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int first = P.d_off[f], n = P.d_off[f + 1] - first;
    if (n <= 0 || n > SV_BOWC_LDS_MAX) return;  // (uniform: before any barrier)
    int npow2 = 1;
    while (npow2 < n) npow2 <<= 1;
    for (int which = 0; which < 2; ++which) {
        for (int i = tid; i < npow2; i += 256) s_v[i] = i < n ? bowc_composite(P, first, i, which) : SV_BOWC_DROPPED;
        __syncthreads();
        for (int k = 2; k <= npow2; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (npow2 >> 1); t += 256) {  // one lane per PAIR: i has bit j clear, its partner has it set
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                    const unsigned long long a = s_v[i], b = s_v[l];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) {
                        s_v[i] = b;
                        s_v[l] = a;
                    }
                }
                __syncthreads();
            }
        unsigned long long* __restrict__ out = which ? P.fkey : P.vkey;
        for (int i = tid; i < n; i += 256) out[first + i] = s_v[i];
        __syncthreads();
    }
}

// (c) a frame beyond the workgroup path: the stable radix sort by the 32-bit key alone keeps the ascending feature index inside a key,
// which is the order of the composites.  A dropped feature carries the key 0xFFFFFFFF (word and node ids of the DBoW2 form are int32 >= 0).
__global__ void __launch_bounds__(256) k_bowc_big_init(BowComputeProblem P, int first, int n, int which, unsigned* __restrict__ keys,
                                                       unsigned long long* __restrict__ vals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long c = bowc_composite(P, first, i, which);
    keys[i] = (unsigned)(c >> 32);
    vals[i] = c == SV_BOWC_DROPPED ? SV_BOWC_DROPPED : (unsigned long long)i;
}
__global__ void __launch_bounds__(256) k_bowc_big_pack(BowComputeProblem P, int first, int n, int which, const unsigned* __restrict__ keys,
                                                       const unsigned long long* __restrict__ vals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsigned long long* __restrict__ out = which ? P.fkey : P.vkey;
    out[first + i] = vals[i] == SV_BOWC_DROPPED ? SV_BOWC_DROPPED : ((unsigned long long)keys[i] << 32) | (unsigned)vals[i];
}

__device__ __forceinline__ bool bowc_is_head(const BowComputeProblem& P, int p, unsigned long long a) {
    if (a == SV_BOWC_DROPPED) return false;
    return p == P.d_off[P.frame[p]] || (unsigned)(P.vkey[p - 1] >> 32) != (unsigned)(a >> 32);  // (a predecessor inside the frame is a kept one)
}

// (d) run heads by a compare with the predecessor, and the kept features of the node-key order; the scans make positions of both
__global__ void __launch_bounds__(256) k_bowc_heads(BowComputeProblem P) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P.total) return;
    P.head[p] = bowc_is_head(P, p, P.vkey[p]) ? 1 : 0;
    P.kept[p] = P.fkey[p] != SV_BOWC_DROPPED ? 1 : 0;
}

// (d) one lane per run: the word's weight is 0.0 + (double)weight[i0] + (double)weight[i1] + ... over its features in ascending index.
// The same launch writes the feature vector and, by its first B + 1 threads, the frame offsets of both results.
__global__ void __launch_bounds__(256) k_bowc_emit(BowComputeProblem P) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p <= P.num_frames) {
        const int o = P.d_off[p];  // <= total: the scans wrote their totals there
        P.vec_off[p] = P.head[o];
        P.feat_off[p] = P.kept[o];
    }
    if (p >= P.total) return;
    const unsigned long long b = P.fkey[p];
    if (b != SV_BOWC_DROPPED) {
        const int t = P.kept[p];
        P.feat_key[t] = (unsigned)(b >> 32);
        P.feat_index[t] = (int)(unsigned)b;
    }
    const unsigned long long a = P.vkey[p];
    if (!bowc_is_head(P, p, a)) return;
    const int f = P.frame[p], first = P.d_off[f], end = P.d_off[f + 1];
    const unsigned w = (unsigned)(a >> 32);
    double sum = 0.0;
    for (int q = p; q < end; ++q) {
        const unsigned long long c = P.vkey[q];
        if (c == SV_BOWC_DROPPED || (unsigned)(c >> 32) != w) break;
        sum += (double)P.weight[first + (int)(unsigned)c];
    }
    const int r = P.head[p];
    P.vec_word[r] = w;
    P.vec_weight[r] = sum;
}

// (e) one wave per frame.  The words are read 64 at a time, a lane each; the running sum takes them one after another through a
// lane-indexed read (every lane performs the same additions in the same order and ends with the same norm), then all lanes scale.
__global__ void __launch_bounds__(256) k_bowc_normalise(BowComputeProblem P) {
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (f >= P.num_frames) return;
    const int lo = P.vec_off[f], hi = P.vec_off[f + 1];
    double norm = 0.0;
    for (int base = lo; base < hi; base += 64) {
        const double v = base + lane < hi ? P.vec_weight[base + lane] : 0.0;
        const double t = P.dbow2 ? fabs(v) : v * v;  // (the product is rounded before it is added: no contraction in this build)
        const int m = min(64, hi - base);
        for (int i = 0; i < m; ++i) norm += __shfl(t, i, 64);
    }
    if (!(norm > 0.0)) return;
    if (P.dbow2) {
        for (int i = lo + lane; i < hi; i += 64) P.vec_weight[i] = P.vec_weight[i] / norm;
    }
    else {
        const double r = 1.0 / sqrt(norm);
        for (int i = lo + lane; i < hi; i += 64) P.vec_weight[i] = P.vec_weight[i] * r;
    }
}

inline dim3 blocks_of(int n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

void sv_launch_bowc_owner(hipStream_t s, const BowComputeProblem& P) { hipLaunchKernelGGL(k_bowc_owner, blocks_of(P.total), dim3(256), 0, s, P); }
void sv_launch_bowc_sort_lds(hipStream_t s, const BowComputeProblem& P, int max_lds_frame) {
    hipLaunchKernelGGL(k_bowc_sort_lds, dim3((unsigned)P.num_frames), dim3(256), bowc_lds_bytes((size_t)max_lds_frame), s, P);
}
void sv_launch_bowc_big_init(hipStream_t s, const BowComputeProblem& P, int first, int n, int which, unsigned* keys, unsigned long long* vals) {
    hipLaunchKernelGGL(k_bowc_big_init, blocks_of(n), dim3(256), 0, s, P, first, n, which, keys, vals);
}
void sv_launch_bowc_big_pack(hipStream_t s, const BowComputeProblem& P, int first, int n, int which, const unsigned* keys, const unsigned long long* vals) {
    hipLaunchKernelGGL(k_bowc_big_pack, blocks_of(n), dim3(256), 0, s, P, first, n, which, keys, vals);
}
void sv_launch_bowc_heads(hipStream_t s, const BowComputeProblem& P) { hipLaunchKernelGGL(k_bowc_heads, blocks_of(P.total), dim3(256), 0, s, P); }
void sv_launch_bowc_emit(hipStream_t s, const BowComputeProblem& P) {
    hipLaunchKernelGGL(k_bowc_emit, blocks_of(P.total > P.num_frames + 1 ? P.total : P.num_frames + 1), dim3(256), 0, s, P);
}
void sv_launch_bowc_normalise(hipStream_t s, const BowComputeProblem& P) {
    hipLaunchKernelGGL(k_bowc_normalise, dim3((unsigned)((P.num_frames + 3) / 4)), dim3(256), 0, s, P);
}
