// The scratch-arena layout of svgpu_bow_compute_batch (svgpu_bowcompute.hip): the concatenated descriptors with their frame offsets, the
// descent's three arrays, the two sorted composite-key arrays, the two flag arrays the scans turn into positions, the buffers of the general
// sort (only when a frame is longer than the workgroup path takes), and the results next to one another.  It places and does nothing else.
// Plain C++ (no HIP): tests/bow_compute_arena_check.cpp compiles this header with sv_arena.h alone.
#pragma once
#include <cstddef>
#include <cstdint>

#include "sv_arena.h"

// A frame of at most this many descriptors is ordered by ONE workgroup in LDS (k_bowc_sort_lds: 8 bytes per composite key, the count
// rounded up to a power of two: at most 32 KB, below what a workgroup gets without asking).  A longer frame takes the radix sort.
#define SV_BOWC_LDS_MAX 4096

inline bool bowc_lds_path(size_t n) { return n <= SV_BOWC_LDS_MAX; }
inline size_t bowc_pow2(size_t n) {
    size_t p = 1;
    while (p < n) p <<= 1;
    return p;
}
// LDS bytes of the sort workgroups of one call: the largest frame that takes the workgroup path decides
inline size_t bowc_lds_bytes(size_t max_lds_frame) { return bowc_pow2(max_lds_frame) * 8; }

struct BowComputeShape {
    size_t num_frames = 0;  // B
    size_t total = 0;       // N = d_off[B]
    size_t max_big = 0;     // descriptors of the longest frame beyond SV_BOWC_LDS_MAX (0: every frame takes the workgroup path)
    size_t scan_ints = 0;   // sv_scan_scratch_ints(N)
    size_t hist_ints = 0;   // sv_sort_hist_ints(max_big)
};
struct BowComputePieces {
    Piece<int32_t> d_off;              // B + 1
    Piece<uint32_t> desc;              // N x 8 words
    Piece<int32_t> frame;              // N: the frame of every descriptor
    Piece<unsigned long long> vkey;    // N: per frame (word << 32 | index) ascending, the dropped features (all ones) last
    Piece<unsigned long long> fkey;    // N: the same by (node key << 32 | index)
    Piece<int32_t> head, kept;         // N + 1 each: run-head / kept flags, then their exclusive scans with the totals
    Piece<int32_t> scan_scratch;
    Piece<uint32_t> sort_key[2];       // max_big each
    Piece<unsigned long long> sort_val[2];
    Piece<int32_t> sort_hist;
    // what is read back, side by side
    Piece<int32_t> word;               // N
    Piece<float> weight;               // N
    Piece<int32_t> node;               // N (the FBoW form's code as its bits)
    Piece<int32_t> vec_off, feat_off;  // B + 1 each
    Piece<uint32_t> vec_word;          // N (vec_off[B] used)
    Piece<double> vec_weight;          // N
    Piece<uint32_t> feat_key;          // N (feat_off[B] used)
    Piece<int32_t> feat_index;         // N
};

template <class A>
void bow_compute_layout(A& arena, const BowComputeShape& S, BowComputePieces& Y) {
    const size_t B = S.num_frames, N = S.total, big = S.max_big;
    Y.d_off = arena.template piece<int32_t>(B + 1);
    Y.desc = arena.template piece<uint32_t>(N * 8);
    Y.frame = arena.template piece<int32_t>(N);
    Y.vkey = arena.template piece<unsigned long long>(N);
    Y.fkey = arena.template piece<unsigned long long>(N);
    Y.head = arena.template piece<int32_t>(N + 1);
    Y.kept = arena.template piece<int32_t>(N + 1);
    Y.scan_scratch = optional_piece<int32_t>(arena, S.scan_ints > 0, S.scan_ints);
    for (int u = 0; u < 2; ++u) {
        Y.sort_key[u] = optional_piece<uint32_t>(arena, big > 0, big);
        Y.sort_val[u] = optional_piece<unsigned long long>(arena, big > 0, big);
    }
    Y.sort_hist = optional_piece<int32_t>(arena, big > 0, S.hist_ints);
    Y.word = arena.template piece<int32_t>(N);
    Y.weight = arena.template piece<float>(N);
    Y.node = arena.template piece<int32_t>(N);
    Y.vec_off = arena.template piece<int32_t>(B + 1);
    Y.feat_off = arena.template piece<int32_t>(B + 1);
    Y.vec_word = arena.template piece<uint32_t>(N);
    Y.vec_weight = arena.template piece<double>(N);
    Y.feat_key = arena.template piece<uint32_t>(N);
    Y.feat_index = arena.template piece<int32_t>(N);
}
