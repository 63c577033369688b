// Host-only check of newlm_layout (stella_vslam_amd/csrc/newlm_layout.h): the smallest and the largest shape of
// tests/test_gpu_new_landmarks.py, depths present and absent, inactive neighbours (result rows without a problem), and the prefix
// invariant across the two passes (lists off, of capacity 1, of a capacity past 1 MiB: every piece in front of the lists keeps its offset).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "layout_check.h"
#include "newlm_layout.h"

static const uint8_t one = 1;
struct On {  // a host array stands for "present"
    bool on;
    template <class T>
    operator const T*() const { return on ? reinterpret_cast<const T*>(&one) : nullptr; }
};
static BucketSide side(int n, bool node, bool xright, bool side1) {
    return BucketSide{On{true}, On{true}, On{true}, On{node}, On{side1}, On{true}, On{xright}, n};
}

static Rows rows_of(const NewLmPieces& Y, const NewLmShape& S, bool lists, size_t total) {
    const size_t K = S.num_neighbours, M = S.match.side2.size(), n1 = (size_t)S.match.side1[0].n, l = lists ? total : 0;
    size_t N2 = 0, D2 = 0;
    for (size_t p = 0; p < M; ++p) {
        N2 += (size_t)S.match.side2[p].n;
        if (S.depth2[p]) D2 += (size_t)S.match.side2[p].n;
    }
    const BucketBatchPieces& B = Y.B;
    // the new pieces in full; of the matcher's layout (checked piece by piece in bucket_batch_arena_check.cpp) the per-row state the chain
    // writes, and the lists, which must stay the last two rows
    return Rows{{Y.xy1, n1 * 8}, {Y.depth1, S.depth1 ? n1 * 4 : 0}, {Y.xy2, N2 * 8}, {Y.octave2, N2 * 4}, {Y.depth2, D2 * 4},
                {Y.view_tab, (K + 1) * S.view_rec}, {Y.prob_of_nb, K * 4}, {Y.taken, n1}, {Y.match, K * n1 * 4}, {Y.pos_w, K * n1 * 24},
                {Y.status, K * n1}, {Y.num_matches, K * 4}, {Y.num_accepted, K * 4}, {Y.created_by, n1 * 4},
                {B.q_valid, M * n1}, {B.cand_off, (M * n1 + 1) * 4}, {B.match_rows, M * n1 * 4}, {B.num, M * 4},
                {B.cand_idx, l * 4}, {B.dist, l * 4}};
}

static void check(const char* what, NewLmShape S) {
    S.view_rec = 320;
    BucketBatchShape& H = S.match;
    H.num_problems = (int)H.side2.size(), H.shared1 = true;
    H.occupied2.assign(H.side2.size(), nullptr);
    H.side_rec = 24, H.gather_rec = 24, H.bucket_rec = 336, H.cand_rec = 304, H.replay_rec = 24;
    if (H.global_form.empty()) H.global_form.assign(H.side2.size(), 0);
    size_t pairs = 0;
    for (const BucketSide& b : H.side2) pairs += (size_t)H.side1[0].n * (size_t)b.n;
    const size_t caps[3] = {0, 1, std::max<size_t>(pairs / 10, (size_t(1) << 18) + 1)};  // off, one entry, past 1 MiB
    std::vector<Rows> placed;
    for (const size_t total : caps) {
        char name[160];
        std::snprintf(name, sizeof name, "%s lists %zu", what, total);
        layout_check<NewLmPieces>(
            name, [&](Arena& A, NewLmPieces& Y) { newlm_layout(A, S, total > 0, total, Y); },
            [&](const NewLmPieces& Y) { return rows_of(Y, S, total > 0, total); },
            [&](const NewLmPieces& Y, const char* base, size_t) {
                // a neighbour's arrays lie inside the concatenated pieces in problem order; the results lie next to one another
                size_t first = 0, dfirst = 0;
                for (size_t p = 0; p < H.side2.size(); ++p) {
                    CHECK(Y.first2[p] == first);
                    CHECK((Y.depth2_at[p] != nullptr) == (S.depth2[p] != 0 && Y.depth2.p != nullptr));
                    if (Y.depth2_at[p]) {
                        CHECK(Y.depth2_at[p] == Y.depth2.p + dfirst);
                        dfirst += (size_t)H.side2[p].n;
                    }
                    first += (size_t)H.side2[p].n;
                }
                const char* r[7] = {(const char*)Y.match.p, (const char*)Y.pos_w.p, (const char*)Y.status.p, (const char*)Y.num_matches.p,
                                    (const char*)Y.num_accepted.p, (const char*)Y.created_by.p, (const char*)Y.created_by.p + pad(Y.created_by.bytes())};
                const size_t bytes[6] = {Y.match.bytes(), Y.pos_w.bytes(), Y.status.bytes(), Y.num_matches.bytes(), Y.num_accepted.bytes(), Y.created_by.bytes()};
                for (int i = 0; i < 6; ++i) CHECK(r[i] + pad(bytes[i]) == r[i + 1]);  // one range: one read-back
                CHECK((const char*)Y.B.desc1.p >= r[6]);                              // the matcher's layout lies behind everything new
                Rows rr = rows_of(Y, S, total > 0, total);
                for (Row& x : rr) x.p = x.p ? (const char*)(x.p - base) : nullptr;  // offsets: the buffers of the three runs differ
                placed.push_back(rr);
            });
    }
    // the prefix invariant: everything but the two lists (the last two rows) lies where it lay without them, and the lists come last
    for (size_t v = 1; v < placed.size(); ++v) {
        const Rows &a = placed[0], &b = placed[v];
        CHECK(a.size() == b.size());
        for (size_t i = 0; i + 2 < a.size(); ++i) CHECK(a[i].p == b[i].p && a[i].touched == b[i].touched);
        const Row &ci = b[b.size() - 2], &di = b[b.size() - 1];
        for (size_t i = 0; i + 2 < b.size(); ++i)
            if (b[i].touched) CHECK(b[i].p + b[i].touched <= ci.p);
        CHECK(ci.p + ci.touched <= di.p);
    }
}

int main() {
    {  // smallest: one neighbour, no stereo arrays, no node ids
        NewLmShape S;
        S.num_neighbours = 1, S.match.side1 = {side(150, false, false, true)}, S.match.side2 = {side(145, false, false, false)}, S.depth2 = {0};
        S.match.sortb = 4096;
        check("single", S);
    }
    {  // three neighbours of five active, depths on the current keyframe and on two neighbours, an empty neighbour
        NewLmShape S;
        S.num_neighbours = 5, S.depth1 = true, S.match.side1 = {side(238, true, true, true)};
        S.match.side2 = {side(225, true, true, false), side(0, true, false, false), side(225, true, true, false)}, S.depth2 = {1, 0, 1};
        S.match.sortb = 8192;
        check("stereo with inactive neighbours", S);
    }
    {  // largest: the spill -- the middle neighbour in the global-memory form
        NewLmShape S;
        S.num_neighbours = 3, S.match.side1 = {side(300, true, false, true)};
        S.match.side2 = {side(295, true, false, false), side(25500, true, false, false), side(295, true, false, false)}, S.depth2 = {0, 0, 0};
        S.match.global_form = {0, 1, 0}, S.match.sortb = 1 << 20, S.match.scan_ints = 0;
        check("spill", S);
    }
    return layout_check_result("new landmarks arena ok");
}
