// The scratch-arena layout of svgpu_new_landmarks_batch (svgpu_newlm.hip): what the triangulator reads beyond the matcher's arrays, the
// chain's state and the results, and behind them the whole layout of the batched bucket matcher (bucket_batch_layout.h) for the ACTIVE
// neighbours with the current keyframe as the one shared side 1.  octave / bearings / xright of a keyframe are the matcher's pieces: the
// triangulator's views name them, nothing is placed twice.  It places and does nothing else, and it keeps the prefix invariant: the
// candidate lists are the LAST takes (bucket_batch_layout's), and nothing in front of them depends on `lists` or on their capacity.
// Plain C++ (no HIP): tests/newlm_arena_check.cpp compiles this header with sv_arena.h alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "bucket_batch_layout.h"

struct NewLmShape {
    BucketBatchShape match;        // shared1, side1 = {the current keyframe}, side2 = the active neighbours in neighbour order
    size_t num_neighbours = 0;     // K, inactive ones included: the results have a row per neighbour
    bool depth1 = false;           // the current keyframe has depths
    std::vector<uint8_t> depth2;   // per active neighbour
    size_t view_rec = 0;           // bytes of one TriView record
};
struct NewLmPieces {
    Piece<float> xy1, depth1, xy2, depth2;   // xy: n x 2; the neighbours' arrays one after another in problem order
    Piece<int32_t> octave2;
    std::vector<float*> depth2_at;           // per active neighbour (null = none)
    std::vector<size_t> first2;              // per active neighbour: its first keypoint inside xy2 / octave2
    Piece<char> view_tab;                    // K + 1 records: the neighbours, then the current keyframe
    Piece<int32_t> prob_of_nb;               // K
    Piece<uint8_t> taken;                    // n1
    // the results, next to one another: one read-back
    Piece<int32_t> match;                    // K x n1
    Piece<double> pos_w;                     // K x n1 x 3
    Piece<uint8_t> status;                   // K x n1
    Piece<int32_t> num_matches, num_accepted;  // K each
    Piece<int32_t> created_by;               // n1
    BucketBatchPieces B;
};

template <class A>
void newlm_layout(A& arena, const NewLmShape& S, bool lists, size_t total, NewLmPieces& Y) {
    const size_t K = S.num_neighbours, M = S.match.side2.size(), n1 = S.match.side1.empty() ? 0 : (size_t)S.match.side1[0].n;
    size_t N2 = 0, D2 = 0;
    Y.first2.assign(M, 0);
    std::vector<size_t> dfirst(M, ~size_t(0));
    for (size_t p = 0; p < M; ++p) {
        Y.first2[p] = N2;
        N2 += (size_t)S.match.side2[p].n;
        if (p < S.depth2.size() && S.depth2[p]) dfirst[p] = D2, D2 += (size_t)S.match.side2[p].n;
    }
    Y.xy1 = arena.template piece<float>(n1 * 2);
    Y.depth1 = optional_piece<float>(arena, S.depth1, n1);
    Y.xy2 = arena.template piece<float>(N2 * 2);
    Y.octave2 = arena.template piece<int32_t>(N2);
    Y.depth2 = optional_piece<float>(arena, D2 > 0, D2);
    Y.view_tab = arena.template piece<char>((K + 1) * S.view_rec);
    Y.prob_of_nb = arena.template piece<int32_t>(K);
    Y.taken = arena.template piece<uint8_t>(n1);
    Y.match = arena.template piece<int32_t>(K * n1);
    Y.pos_w = arena.template piece<double>(K * n1 * 3);
    Y.status = arena.template piece<uint8_t>(K * n1);
    Y.num_matches = arena.template piece<int32_t>(K);
    Y.num_accepted = arena.template piece<int32_t>(K);
    Y.created_by = arena.template piece<int32_t>(n1);
    Y.depth2_at.assign(M, nullptr);
    for (size_t p = 0; p < M; ++p) Y.depth2_at[p] = bucket_batch_detail::at(Y.depth2, dfirst[p]);
    bucket_batch_layout(arena, S.match, lists, total, Y.B);  // ... whose last takes are the lists
}
