// The scratch-arena layout of the batched bucket matcher (svgpu_bow_match_batch, svgpu_match_for_triangulation_batch): K problems in
// one staged call.  A side that all problems share is one entry of its side list and takes its pieces once.  Like bucket_layout
// (match_layout.h) it places and does nothing else, and it keeps the prefix invariant: the candidate lists are the LAST takes and
// nothing in front of them depends on `lists` or on their capacity.  Plain C++ (no HIP): tests/bucket_batch_arena_check.cpp compiles
// this header with sv_arena.h alone.
//
// Every array kind is ONE piece that holds the sides which have it, one after another in side order; a side without an optional array
// adds nothing to that piece and gets a null pointer.  Per-problem device arrays (rows, offsets, matches) are concatenated in problem
// order: problem p owns rows row_base[p] .. row_base[p + 1].
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "match_layout.h"

struct BucketBatchShape {
    std::vector<BucketSide> side1, side2;      // the DISTINCT sides: one entry when the side is shared, else one per problem
    std::vector<const uint8_t*> occupied2;     // per entry of side2 (nullable each)
    int num_problems = 0;
    bool shared1 = false, shared2 = false;
    std::vector<uint8_t> global_form;          // per problem: 1 = the replay keeps its tables in global memory (owner, match_of_row)
    size_t sortb = 0;                          // scratch of the general sort, for sides beyond the one-workgroup sort
    size_t scan_ints = 0;                      // scratch of the scan over all rows
    size_t side_rec = 0, gather_rec = 0, bucket_rec = 0, cand_rec = 0, replay_rec = 0;  // bytes of one record of the five device tables
    const BucketSide& s1(int p) const { return side1[shared1 ? 0 : (size_t)p]; }
    const BucketSide& s2(int p) const { return side2[shared2 ? 0 : (size_t)p]; }
};
// where one side's arrays lie inside the concatenated pieces (null = the side has none)
struct BucketSidePlace {
    uint8_t* desc = nullptr;
    float* angle = nullptr;
    uint8_t* valid = nullptr;
    int32_t* node = nullptr;
    int32_t* octave = nullptr;
    double* bearings = nullptr;
    float* xright = nullptr;
    uint8_t* occupied = nullptr;
    unsigned* key = nullptr;       // sorted node ids
    int* order = nullptr;          // position in (node, index) order -> keypoint
    uint32_t* desc_rows = nullptr; // side 1: descriptors gathered in row order
    size_t first = 0;              // element offset of the side inside the per-keypoint pieces of its side list
};
struct BucketBatchPieces {
    Piece<uint8_t> desc1, desc2, valid1, valid2, occupied2, q_valid;
    Piece<float> angle1, angle2, xright1, xright2;
    Piece<int32_t> node1, node2, octave1, row_base, side1_base, cand_off, match_rows, match, num, cand_idx;
    Piece<double> bearings1, bearings2;
    Piece<char> side_tab, gather_tab, bucket_tab, cand_tab, replay_tab, sort_scratch;
    Piece<unsigned> key1, key2;
    Piece<int> order1, order2, row_lo, row_hi, owner, match_of_row, scan_scratch;
    Piece<uint32_t> qdesc_rows, dist;
    std::vector<BucketSidePlace> at1, at2;     // per distinct side
    std::vector<size_t> row_first;             // per problem (+ the total): first row
    std::vector<size_t> owner_first, mrow_first;  // per problem: offset inside owner / match_of_row (global-form problems only)
};

namespace bucket_batch_detail {
template <class T, class A, class Has>
Piece<T> cat(A& arena, const std::vector<BucketSide>& sides, size_t per, Has&& has, std::vector<size_t>& first) {
    size_t total = 0;
    bool any = false;
    first.assign(sides.size(), ~size_t(0));
    for (size_t u = 0; u < sides.size(); ++u)
        if (has(u)) {
            any = true;
            first[u] = total;
            total += (size_t)sides[u].n * per;
        }
    return optional_piece<T>(arena, any, total);
}
template <class T>
T* at(const Piece<T>& piece, size_t first) { return piece.p && first != ~size_t(0) ? piece.p + first : nullptr; }
}  // namespace bucket_batch_detail

template <class A>
void bucket_batch_layout(A& arena, const BucketBatchShape& S, bool lists, size_t total, BucketBatchPieces& Y) {
    using namespace bucket_batch_detail;
    const size_t K = (size_t)S.num_problems, U1 = S.side1.size(), U2 = S.side2.size();
    size_t N1 = 0, N2 = 0, R = 0, G1 = 0, G2 = 0;
    for (const BucketSide& s : S.side1) N1 += (size_t)s.n;
    for (const BucketSide& s : S.side2) N2 += (size_t)s.n;
    Y.row_first.assign(K + 1, 0);
    Y.owner_first.assign(K, 0);
    Y.mrow_first.assign(K, 0);
    for (size_t p = 0; p < K; ++p) {
        Y.row_first[p] = R;
        R += (size_t)S.s1((int)p).n;
        if (p < S.global_form.size() && S.global_form[p]) {
            Y.owner_first[p] = G2, Y.mrow_first[p] = G1;
            G2 += (size_t)S.s2((int)p).n, G1 += (size_t)S.s1((int)p).n;
        }
    }
    Y.row_first[K] = R;
    // inputs: the first takes
    std::vector<size_t> f_desc1, f_desc2, f_angle1, f_angle2, f_valid1, f_valid2, f_node1, f_node2, f_oct1, f_bear1, f_bear2, f_xr1, f_xr2, f_occ2;
    Y.desc1 = cat<uint8_t>(arena, S.side1, 32, [&](size_t) { return true; }, f_desc1);
    Y.desc2 = cat<uint8_t>(arena, S.side2, 32, [&](size_t) { return true; }, f_desc2);
    Y.angle1 = cat<float>(arena, S.side1, 1, [&](size_t u) { return S.side1[u].angle != nullptr; }, f_angle1);
    Y.angle2 = cat<float>(arena, S.side2, 1, [&](size_t u) { return S.side2[u].angle != nullptr; }, f_angle2);
    Y.valid1 = cat<uint8_t>(arena, S.side1, 1, [&](size_t u) { return S.side1[u].valid != nullptr; }, f_valid1);
    Y.valid2 = cat<uint8_t>(arena, S.side2, 1, [&](size_t u) { return S.side2[u].valid != nullptr; }, f_valid2);
    Y.node1 = cat<int32_t>(arena, S.side1, 1, [&](size_t u) { return S.side1[u].node != nullptr; }, f_node1);
    Y.node2 = cat<int32_t>(arena, S.side2, 1, [&](size_t u) { return S.side2[u].node != nullptr; }, f_node2);
    Y.octave1 = cat<int32_t>(arena, S.side1, 1, [&](size_t u) { return S.side1[u].octave != nullptr; }, f_oct1);
    Y.bearings1 = cat<double>(arena, S.side1, 3, [&](size_t u) { return S.side1[u].bearings != nullptr; }, f_bear1);
    Y.bearings2 = cat<double>(arena, S.side2, 3, [&](size_t u) { return S.side2[u].bearings != nullptr; }, f_bear2);
    Y.xright1 = cat<float>(arena, S.side1, 1, [&](size_t u) { return S.side1[u].xright != nullptr; }, f_xr1);
    Y.xright2 = cat<float>(arena, S.side2, 1, [&](size_t u) { return S.side2[u].xright != nullptr; }, f_xr2);
    Y.occupied2 = cat<uint8_t>(arena, S.side2, 1, [&](size_t u) { return u < S.occupied2.size() && S.occupied2[u] != nullptr; }, f_occ2);
    // the device tables the host fills: sides, the two per-problem records, the replay's form, the row and side-1 bases
    Y.side_tab = arena.template piece<char>((U1 + U2) * S.side_rec);
    Y.gather_tab = arena.template piece<char>(U1 * S.gather_rec);
    Y.bucket_tab = arena.template piece<char>(K * S.bucket_rec);
    Y.cand_tab = arena.template piece<char>(K * S.cand_rec);
    Y.replay_tab = arena.template piece<char>(K * S.replay_rec);
    Y.row_base = arena.template piece<int32_t>(K + 1);
    Y.side1_base = arena.template piece<int32_t>(U1 + 1);
    // per distinct side: the (node, index) order, and side 1's descriptors in row order
    Y.key1 = arena.template piece<unsigned>(N1);
    Y.order1 = arena.template piece<int>(N1);
    Y.qdesc_rows = arena.template piece<uint32_t>(N1 * 8);
    Y.key2 = arena.template piece<unsigned>(N2);
    Y.order2 = arena.template piece<int>(N2);
    // per problem, concatenated in problem order
    Y.row_lo = arena.template piece<int>(R);
    Y.row_hi = arena.template piece<int>(R);
    Y.q_valid = arena.template piece<uint8_t>(R);
    Y.cand_off = arena.template piece<int32_t>(R + 1);
    Y.match_rows = arena.template piece<int32_t>(R);
    Y.match = arena.template piece<int32_t>(R);
    Y.num = arena.template piece<int32_t>(K);
    Y.owner = arena.template piece<int>(G2);
    Y.match_of_row = arena.template piece<int>(G1);
    Y.scan_scratch = arena.template piece<int>(S.scan_ints);
    Y.sort_scratch = arena.template piece<char>(S.sortb);
    Y.cand_idx = optional_piece<int32_t>(arena, lists, total);  // the lists: last
    Y.dist = optional_piece<uint32_t>(arena, lists, total);

    Y.at1.assign(U1, BucketSidePlace{});
    Y.at2.assign(U2, BucketSidePlace{});
    size_t first = 0;
    for (size_t u = 0; u < U1; ++u) {
        BucketSidePlace& P = Y.at1[u];
        P.desc = at(Y.desc1, f_desc1[u]), P.angle = at(Y.angle1, f_angle1[u]), P.valid = at(Y.valid1, f_valid1[u]), P.node = at(Y.node1, f_node1[u]);
        P.octave = at(Y.octave1, f_oct1[u]), P.bearings = at(Y.bearings1, f_bear1[u]), P.xright = at(Y.xright1, f_xr1[u]);
        P.key = at(Y.key1, first), P.order = at(Y.order1, first), P.desc_rows = at(Y.qdesc_rows, first * 8), P.first = first;
        first += (size_t)S.side1[u].n;
    }
    first = 0;
    for (size_t u = 0; u < U2; ++u) {
        BucketSidePlace& P = Y.at2[u];
        P.desc = at(Y.desc2, f_desc2[u]), P.angle = at(Y.angle2, f_angle2[u]), P.valid = at(Y.valid2, f_valid2[u]), P.node = at(Y.node2, f_node2[u]);
        P.bearings = at(Y.bearings2, f_bear2[u]), P.xright = at(Y.xright2, f_xr2[u]), P.occupied = at(Y.occupied2, f_occ2[u]);
        P.key = at(Y.key2, first), P.order = at(Y.order2, first), P.first = first;
        first += (size_t)S.side2[u].n;
    }
}
