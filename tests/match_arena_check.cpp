// Host-only check of the two-pass matchers' scratch layouts (stella_vslam_amd/csrc/match_layout.h), built and run by
// tests/test_arena_layouts.py: the checks of tests/layout_check.h for the smallest and the largest shape of the two-pass tests of
// tests/test_gpu_staged_call.py, every optional array present and absent, a resident frame or none -- and the prefix invariant a second
// pass without regrowth rests on: every piece in front of the candidate lists has the same offset with the lists off, with lists of
// capacity 1 and with lists past the 1 MiB scratch granule.
#include <cstdint>

#include "layout_check.h"
#include "match_layout.h"

static const size_t NCELL = 64 * 48;

// A host array that is passed, or not: the layouts only ask whether it is there, so any address will do.
static const double THERE[1] = {};
struct On {
    bool b;
    template <class T>
    operator const T*() const { return b ? reinterpret_cast<const T*>(THERE) : nullptr; }
};
static const On on{true}, off{false};
struct CellOpt {  // the optional arrays of the keypoint side
    bool occupied, t_angle, t_xright;
};

static Rows reproj_rows(const ReprojPieces& Q, size_t n, const ReprojQuery& h, bool windows) {
    const size_t w = windows ? n : 0;
    return Rows{{Q.desc, h.desc ? n * 32 : 0}, {Q.pos_w, n * 24}, {Q.mean_normal, h.mean_normal ? n * 24 : 0}, {Q.min_valid_dist, h.min_valid_dist ? n * 4 : 0},
                {Q.max_valid_dist, h.max_valid_dist ? n * 4 : 0}, {Q.skip, h.skip ? n : 0}, {Q.q_level, h.q_level ? n * 4 : 0}, {Q.q_angle, h.q_angle ? n * 4 : 0},
                {Q.q_blocks, h.q_blocks ? n : 0}, {Q.visible, n}, {Q.reproj, n * 16}, {Q.x_right, n * 4}, {Q.pred_level, n * 4}, {Q.q_xy, w * 8},
                {Q.q_margin, w * 4}, {Q.q_min_level, w * 4}, {Q.q_max_level, w * 4}};
}
static Rows query_rows(const CellQueryPieces& Q, size_t nq, const CellQuery& h) {
    return Rows{{Q.desc, nq * 32}, {Q.xy, nq * 8}, {Q.margin, nq * 4}, {Q.min_level, h.min_level ? nq * 4 : 0}, {Q.max_level, h.max_level ? nq * 4 : 0},
                {Q.valid, h.valid ? nq : 0}, {Q.angle, h.angle ? nq * 4 : 0}, {Q.xright, h.xright ? nq * 4 : 0}, {Q.xr_tol, h.xr_tol ? nq * 4 : 0},
                {Q.blocks, h.blocks ? nq : 0}};
}
static Rows cell_rows(const CellPieces& Y, size_t nq, size_t nt, const CellOpt& h, bool res, bool lists, size_t cap) {
    const size_t own = res ? 0 : nt, l = lists ? cap : 0;
    return Rows{{Y.tdesc, own * 32}, {Y.t_xy, own * 8}, {Y.t_octave, own * 4}, {Y.occupied, h.occupied ? nt : 0}, {Y.t_angle, h.t_angle ? own * 4 : 0},
                {Y.t_xright, h.t_xright ? own * 4 : 0}, {Y.cell_of, own * 4}, {Y.cell_off, res ? 0 : (NCELL + 1) * 4}, {Y.cell_items, own * 4},
                {Y.cand_off, (nq + 1) * 4}, {Y.match_q, nq * 4}, {Y.num, 4}, {Y.owner, nt * 4}, {Y.match, nq * 4}, {Y.mdist, nt * 4}, {Y.cand_idx, l * 4},
                {Y.dist, l * 4}};
}
static Rows bucket_rows(const BucketPieces& Y, const BucketSide& S1, const BucketSide& S2, bool occupied2, size_t sortb, bool lists, size_t total) {
    const size_t l = lists ? total : 0, n1 = (size_t)S1.n, n2 = (size_t)S2.n;
    return Rows{{Y.desc1, n1 * 32}, {Y.desc2, n2 * 32}, {Y.angle1, S1.angle ? n1 * 4 : 0}, {Y.angle2, S2.angle ? n2 * 4 : 0}, {Y.valid1, S1.valid ? n1 : 0},
                {Y.valid2, S2.valid ? n2 : 0}, {Y.node1, S1.node ? n1 * 4 : 0}, {Y.node2, S2.node ? n2 * 4 : 0}, {Y.octave1, S1.octave ? n1 * 4 : 0},
                {Y.bearings1, S1.bearings ? n1 * 24 : 0}, {Y.bearings2, S2.bearings ? n2 * 24 : 0}, {Y.xright1, S1.xright ? n1 * 4 : 0},
                {Y.xright2, S2.xright ? n2 * 4 : 0}, {Y.occupied2, occupied2 ? n2 : 0}, {Y.key1, n1 * 4}, {Y.q_idx, n1 * 4}, {Y.key2, n2 * 4},
                {Y.t_sorted, n2 * 4}, {Y.row_lo, n1 * 4}, {Y.row_hi, n1 * 4}, {Y.q_valid, n1}, {Y.cand_off, (n1 + 1) * 4}, {Y.qdesc_rows, n1 * 32},
                {Y.qangle_rows, n1 * 4}, {Y.match_rows, n1 * 4}, {Y.match, n1 * 4}, {Y.num, 4}, {Y.owner, n2 * 4}, {Y.match_of_row, n1 * 4},
                {Y.mdist, n2 * 4}, {Y.sort_scratch, sortb}, {Y.cand_idx, l * 4}, {Y.dist, l * 4}};
}

// the offsets of every piece in front of the lists, and where the lists begin
static std::vector<ptrdiff_t> offsets(Rows rows, const char* base) {
    std::vector<ptrdiff_t> o;
    for (size_t i = 0; i + 2 < rows.size(); ++i) o.push_back(rows[i].p ? rows[i].p - base : -1);
    return o;
}
// the prefix invariant: place(lists, cap, rows&) over one buffer, three times
template <class Place>
static void prefix_check(const char* name, Place&& place) {
    const size_t caps[3] = {0, 1, (size_t(1) << 20) / 4 + 4097};  // the last: each list alone is past 1 MiB
    std::vector<ptrdiff_t> first;
    for (int k = 0; k < 3; ++k) {
        const size_t need = arena_measure([&](Arena& A) { Rows r; place(A, k > 0, caps[k], r); });
        std::vector<char> buf(need + 1);
        Arena A(buf.data(), need);
        Rows rows;
        place(A, k > 0, caps[k], rows);
        CHECK(!A.overflow);
        const Row &idx = rows[rows.size() - 2], &dist = rows[rows.size() - 1];
        if (k > 0) CHECK(idx.p && dist.p && dist.p == idx.p + pad(caps[k] * 4) && dist.p + pad(caps[k] * 4) == buf.data() + need);  // the lists are last
        else CHECK(!idx.p && !dist.p);
        const std::vector<ptrdiff_t> o = offsets(rows, buf.data());
        for (size_t i = 0; k > 0 && i + 2 < rows.size(); ++i)  // (a zero-length piece may end where the lists begin)
            if (rows[i].p) CHECK(rows[i].p + rows[i].touched <= idx.p);
        if (k == 0) first = o;
        else CHECK(o == first);
    }
    std::printf("ok prefix %s: %zu pieces in front of the lists\n", name, first.size());
}

static void check_cells(size_t nq, size_t nt, const CellOpt& h, bool res, int query, unsigned opt) {
    // query 0: the caller's window arrays (svgpu_match_in_cells); 1: reprojected landmarks; `opt`: one bit per optional array of the query side
    auto bit = [&](unsigned b) { return On{(opt & b) != 0}; };
    const CellQuery qh{.desc = on, .xy = on, .margin = on, .min_level = bit(1), .max_level = bit(2), .valid = bit(4), .angle = bit(8), .xright = bit(16),
                       .xr_tol = bit(32), .blocks = bit(64)};
    const ReprojQuery rh{.desc = on, .pos_w = on, .mean_normal = bit(1), .min_valid_dist = bit(2), .max_valid_dist = bit(4), .skip = bit(8),
                         .q_level = bit(16), .q_angle = bit(32), .q_blocks = bit(64)};
    struct Both {
        CellPieces Y;
        CellQueryPieces Q;
        ReprojPieces R;
    };
    auto place = [&](Arena& A, bool lists, size_t cap, Both& B) {
        cell_layout(A, nq, nt, NCELL, On{h.occupied}, On{h.t_angle}, On{h.t_xright}, res, lists, cap, B.Y, [&](Arena& Aq) {
            if (query) reproj_layout(Aq, nq, rh, true, B.R);
            else cell_query_layout(Aq, nq, qh, B.Q);
        });
    };
    auto table = [&](const Both& B, bool lists, size_t cap) {
        Rows rows = query ? reproj_rows(B.R, nq, rh, true) : query_rows(B.Q, nq, qh);
        const Rows own = cell_rows(B.Y, nq, nt, h, res, lists, cap);
        rows.insert(rows.end(), own.begin(), own.end());  // (the lists stay the last two rows)
        return rows;
    };
    char name[128];
    std::snprintf(name, sizeof name, "cells nq %zu nt %zu occ %d ang %d xr %d resident %d query %d opt %#x", nq, nt, (int)h.occupied, (int)h.t_angle,
                  (int)h.t_xright, (int)res, query, opt);
    for (const size_t cap : {size_t(0), size_t(1), nq * 100})
        layout_check<Both>(name, [&](Arena& A, Both& B) { place(A, cap > 0, cap, B); }, [&](const Both& B) { return table(B, cap > 0, cap); },
                           [&](const Both& B, const char* base, size_t) {  // the keypoint side's inputs and the query side's lie in front of everything the kernels write
                               if (!res) CHECK((const char*)B.Y.tdesc.p == base);
                               CHECK((const char*)B.Y.cand_off.p > (query ? (const char*)B.R.pos_w.p : (const char*)B.Q.desc.p));
                           });
    prefix_check(name, [&](Arena& A, bool lists, size_t cap, Rows& rows) {
        Both B{};
        place(A, lists, cap, B);
        rows = table(B, lists, cap);
    });
}

static void check_bucket(const BucketSide& S1, const BucketSide& S2, bool occupied2, size_t sortb) {
    const size_t n1 = (size_t)S1.n, n2 = (size_t)S2.n;
    char name[128];
    std::snprintf(name, sizeof name, "bucket n1 %zu n2 %zu sort %zu node %d tri %d", n1, n2, sortb, S1.node != nullptr, S1.bearings != nullptr);
    for (const size_t total : {size_t(0), size_t(1), n1 * n2 / 10})
        layout_check<BucketPieces>(name, [&](Arena& A, BucketPieces& Y) { bucket_layout(A, S1, S2, On{occupied2}, sortb, total > 0, total, Y); },
                                   [&](const BucketPieces& Y) { return bucket_rows(Y, S1, S2, occupied2, sortb, total > 0, total); });
    prefix_check(name, [&](Arena& A, bool lists, size_t total, Rows& rows) {
        BucketPieces Y{};
        bucket_layout(A, S1, S2, On{occupied2}, sortb, lists, total, Y);
        rows = bucket_rows(Y, S1, S2, occupied2, sortb, lists, total);
    });
}

int main() {
    // svgpu_reproject_landmarks: the reprojection side alone, neither descriptors nor windows
    for (const size_t n : {size_t(1), size_t(2000)})
        for (const bool skip : {false, true}) {
            const ReprojQuery h{.desc = off, .pos_w = on, .mean_normal = on, .min_valid_dist = on, .max_valid_dist = on, .skip = On{skip},
                                .q_level = off, .q_angle = off, .q_blocks = off};
            layout_check<ReprojPieces>("reproject", [&](Arena& A, ReprojPieces& Y) { reproj_layout(A, n, h, false, Y); },
                                       [&](const ReprojPieces& Y) { return reproj_rows(Y, n, h, false); });
        }
    const size_t shapes[2][2] = {{3, 5}, {2000, 20000}};  // queries x keypoints: the small and the large call of the GPU tests
    for (const auto& sh : shapes)
        for (int query = 0; query < 2; ++query)
            for (const bool res : {false, true}) {
                check_cells(sh[0], sh[1], CellOpt{false, false, false}, res, query, 0);
                check_cells(sh[0], sh[1], CellOpt{true, true, true}, res, query, 0x7F);
                for (unsigned bit = 0; bit < 7; ++bit) check_cells(sh[0], sh[1], CellOpt{bit % 2 == 0, bit % 3 == 0, bit % 2 == 1}, res, query, 1u << bit);
                check_cells(sh[0], sh[1], CellOpt{true, false, false}, res, query, 0);
                check_cells(sh[0], sh[1], CellOpt{false, true, false}, res, query, 0);
                check_cells(sh[0], sh[1], CellOpt{false, false, true}, res, query, 0);
            }
    const int bshapes[2][3] = {{3, 5, 0}, {2000, 2000, 70001}};
    for (const auto& sh : bshapes) {
        const int n1 = sh[0], n2 = sh[1];
        const size_t sortb = (size_t)sh[2];
        const BucketSide bare1{.desc = on, .angle = off, .valid = off, .node = off, .octave = off, .bearings = off, .xright = off, .n = n1};
        const BucketSide bare2{.desc = on, .angle = off, .valid = off, .node = off, .octave = off, .bearings = off, .xright = off, .n = n2};
        check_bucket(bare1, bare2, false, sortb);
        // svgpu_bow_match: angles, validity and node ids on both sides, the occupied flags of side 2
        check_bucket({.desc = on, .angle = on, .valid = on, .node = on, .octave = off, .bearings = off, .xright = off, .n = n1},
                     {.desc = on, .angle = on, .valid = on, .node = on, .octave = off, .bearings = off, .xright = off, .n = n2}, true, sortb);
        // svgpu_match_for_triangulation in one bucket: octaves of side 1, bearings of both
        check_bucket({.desc = on, .angle = on, .valid = on, .node = off, .octave = on, .bearings = on, .xright = off, .n = n1},
                     {.desc = on, .angle = on, .valid = on, .node = off, .octave = off, .bearings = on, .xright = off, .n = n2}, false, sortb);
        // ... with node ids and stereo keypoints
        check_bucket({.desc = on, .angle = on, .valid = on, .node = on, .octave = on, .bearings = on, .xright = on, .n = n1},
                     {.desc = on, .angle = on, .valid = on, .node = on, .octave = off, .bearings = on, .xright = on, .n = n2}, false, sortb);
        for (unsigned bit = 0; bit < 12; ++bit) {  // each optional array alone: six of side 1, five of side 2, the occupied flags
            auto at = [&](unsigned b) { return On{bit == b}; };
            check_bucket({.desc = on, .angle = at(0), .valid = at(1), .node = at(2), .octave = at(3), .bearings = at(4), .xright = at(5), .n = n1},
                         {.desc = on, .angle = at(6), .valid = at(7), .node = at(8), .octave = off, .bearings = at(9), .xright = at(10), .n = n2}, bit == 11,
                         sortb);
        }
    }
    return layout_check_result("match arena ok");
}
