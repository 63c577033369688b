// Host-only check of bucket_batch_layout (stella_vslam_amd/csrc/bucket_batch_layout.h): the smallest and the largest shape of
// tests/test_gpu_bucket_batch.py, every optional array present and absent, shared and unshared sides, and the prefix invariant (lists
// off, of capacity 1, of a capacity past 1 MiB: every piece in front of the lists keeps its offset).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bucket_batch_layout.h"
#include "layout_check.h"

static const uint8_t one = 1;
struct On {  // a host array stands for "present"
    bool on;
    template <class T>
    operator const T*() const { return on ? reinterpret_cast<const T*>(&one) : nullptr; }
};

static BucketSide side(int n, unsigned has) {  // bits: angle, valid, node, octave, bearings, xright
    return BucketSide{On{true}, On{(has & 1) != 0}, On{(has & 2) != 0}, On{(has & 4) != 0}, On{(has & 8) != 0}, On{(has & 16) != 0}, On{(has & 32) != 0}, n};
}
static size_t sum(const std::vector<BucketSide>& v, size_t per, bool (*has)(const BucketSide&)) {
    size_t t = 0;
    for (const BucketSide& s : v)
        if (has(s)) t += (size_t)s.n * per;
    return t;
}

static Rows rows_of(const BucketBatchPieces& Y, const BucketBatchShape& S, bool lists, size_t total) {
    const size_t K = (size_t)S.num_problems, U1 = S.side1.size(), U2 = S.side2.size(), l = lists ? total : 0;
    size_t N1 = 0, N2 = 0, R = 0, G1 = 0, G2 = 0, occ = 0;
    for (const BucketSide& s : S.side1) N1 += (size_t)s.n;
    for (const BucketSide& s : S.side2) N2 += (size_t)s.n;
    for (size_t p = 0; p < K; ++p) {
        R += (size_t)S.s1((int)p).n;
        if (S.global_form[p]) G1 += (size_t)S.s1((int)p).n, G2 += (size_t)S.s2((int)p).n;
    }
    for (size_t u = 0; u < U2; ++u)
        if (S.occupied2[u]) occ += (size_t)S.side2[u].n;
    auto all = [](const BucketSide&) { return true; };
    auto ang = [](const BucketSide& s) { return s.angle != nullptr; };
    auto val = [](const BucketSide& s) { return s.valid != nullptr; };
    auto nod = [](const BucketSide& s) { return s.node != nullptr; };
    auto oct = [](const BucketSide& s) { return s.octave != nullptr; };
    auto bea = [](const BucketSide& s) { return s.bearings != nullptr; };
    auto xr = [](const BucketSide& s) { return s.xright != nullptr; };
    return Rows{{Y.desc1, sum(S.side1, 32, all)}, {Y.desc2, sum(S.side2, 32, all)}, {Y.angle1, sum(S.side1, 4, ang)}, {Y.angle2, sum(S.side2, 4, ang)},
                {Y.valid1, sum(S.side1, 1, val)}, {Y.valid2, sum(S.side2, 1, val)}, {Y.node1, sum(S.side1, 4, nod)}, {Y.node2, sum(S.side2, 4, nod)},
                {Y.octave1, sum(S.side1, 4, oct)}, {Y.bearings1, sum(S.side1, 24, bea)}, {Y.bearings2, sum(S.side2, 24, bea)},
                {Y.xright1, sum(S.side1, 4, xr)}, {Y.xright2, sum(S.side2, 4, xr)}, {Y.occupied2, occ},
                {Y.side_tab, (U1 + U2) * S.side_rec}, {Y.gather_tab, U1 * S.gather_rec}, {Y.bucket_tab, K * S.bucket_rec}, {Y.cand_tab, K * S.cand_rec},
                {Y.replay_tab, K * S.replay_rec}, {Y.row_base, (K + 1) * 4}, {Y.side1_base, (U1 + 1) * 4},
                {Y.key1, N1 * 4}, {Y.order1, N1 * 4}, {Y.qdesc_rows, N1 * 32}, {Y.key2, N2 * 4}, {Y.order2, N2 * 4},
                {Y.row_lo, R * 4}, {Y.row_hi, R * 4}, {Y.q_valid, R}, {Y.cand_off, (R + 1) * 4}, {Y.match_rows, R * 4}, {Y.match, R * 4}, {Y.num, K * 4},
                {Y.owner, G2 * 4}, {Y.match_of_row, G1 * 4}, {Y.scan_scratch, S.scan_ints * 4}, {Y.sort_scratch, S.sortb},
                {Y.cand_idx, l * 4}, {Y.dist, l * 4}};
}

// what only this layout promises: a side's arrays lie inside their pieces, one after another in side order, and a shared side once
static void places(const BucketBatchPieces& Y, const BucketBatchShape& S) {
    CHECK(Y.at1.size() == S.side1.size() && Y.at2.size() == S.side2.size());
    CHECK(Y.row_first.size() == (size_t)S.num_problems + 1);
    size_t first = 0, adesc = 0, aangle = 0;
    for (size_t u = 0; u < S.side1.size(); ++u) {
        const BucketSidePlace& a = Y.at1[u];
        const size_t n = (size_t)S.side1[u].n;
        CHECK(a.first == first && a.desc == Y.desc1.p + adesc && a.key == Y.key1.p + first && a.order == Y.order1.p + first && a.desc_rows == Y.qdesc_rows.p + first * 8);
        CHECK((a.angle != nullptr) == (S.side1[u].angle != nullptr) && (a.valid != nullptr) == (S.side1[u].valid != nullptr)
              && (a.node != nullptr) == (S.side1[u].node != nullptr) && (a.octave != nullptr) == (S.side1[u].octave != nullptr)
              && (a.bearings != nullptr) == (S.side1[u].bearings != nullptr) && (a.xright != nullptr) == (S.side1[u].xright != nullptr) && !a.occupied);
        if (a.angle) {
            CHECK(a.angle == Y.angle1.p + aangle);
            aangle += n;
        }
        first += n, adesc += n * 32;
    }
    CHECK(aangle == Y.angle1.n && adesc == Y.desc1.n);
    first = 0;
    size_t occ = 0;
    for (size_t u = 0; u < S.side2.size(); ++u) {
        const BucketSidePlace& b = Y.at2[u];
        const size_t n = (size_t)S.side2[u].n;
        CHECK(b.first == first && b.desc == Y.desc2.p + first * 32 && b.key == Y.key2.p + first && b.order == Y.order2.p + first && !b.octave && !b.desc_rows);
        CHECK((b.occupied != nullptr) == (S.occupied2[u] != nullptr) && (b.bearings != nullptr) == (S.side2[u].bearings != nullptr)
              && (b.node != nullptr) == (S.side2[u].node != nullptr));
        if (b.occupied) {
            CHECK(b.occupied == Y.occupied2.p + occ);
            occ += n;
        }
        first += n;
    }
    size_t R = 0, G1 = 0, G2 = 0;
    for (int p = 0; p < S.num_problems; ++p) {
        CHECK(Y.row_first[(size_t)p] == R);
        if (S.global_form[(size_t)p]) {
            CHECK(Y.owner_first[(size_t)p] == G2 && Y.mrow_first[(size_t)p] == G1);
            G1 += (size_t)S.s1(p).n, G2 += (size_t)S.s2(p).n;
        }
        R += (size_t)S.s1(p).n;
    }
    CHECK(Y.row_first[(size_t)S.num_problems] == R && Y.owner.n == G2 && Y.match_of_row.n == G1);
}

static void check(const char* what, BucketBatchShape S) {
    S.side_rec = 24, S.gather_rec = 24, S.bucket_rec = 336, S.cand_rec = 304, S.replay_rec = 24;
    if (S.global_form.empty()) S.global_form.assign((size_t)S.num_problems, 0);
    size_t pairs = 0;
    for (int p = 0; p < S.num_problems; ++p) pairs += (size_t)S.s1(p).n * (size_t)S.s2(p).n;
    const size_t caps[3] = {0, 1, std::max<size_t>(pairs / 10, (size_t(1) << 18) + 1)};  // off, one entry, past 1 MiB
    std::vector<Rows> placed;
    for (const size_t total : caps) {
        char name[160];
        std::snprintf(name, sizeof name, "%s lists %zu", what, total);
        layout_check<BucketBatchPieces>(
            name, [&](Arena& A, BucketBatchPieces& Y) { bucket_batch_layout(A, S, total > 0, total, Y); },
            [&](const BucketBatchPieces& Y) { return rows_of(Y, S, total > 0, total); },
            [&](const BucketBatchPieces& Y, const char* base, size_t) {
                places(Y, S);
                Rows r = rows_of(Y, S, total > 0, total);
                for (Row& x : r) x.p = x.p ? (const char*)(x.p - base) : nullptr;  // offsets: the buffers of the three runs differ
                placed.push_back(r);
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
    const unsigned BOW = 1 | 2 | 4, TRI1 = 1 | 2 | 4 | 8 | 16 | 32, TRI2 = 1 | 2 | 4 | 16 | 32;
    {  // smallest of the GPU test: one problem, one keypoint a side (a batch of one of `unshared`)
        BucketBatchShape S;
        S.num_problems = 1, S.side1 = {side(1, BOW)}, S.side2 = {side(1, BOW)}, S.occupied2 = {nullptr}, S.sortb = 2048;
        check("one by one", S);
    }
    {  // reloc: side 2 shared with occupied flags, an empty keyframe among six
        BucketBatchShape S;
        S.num_problems = 6, S.shared2 = true, S.side2 = {side(1000, BOW & ~2u)}, S.occupied2 = {&one}, S.sortb = 70000;
        for (int n : {1000, 666, 666, 500, 0, 333}) S.side1.push_back(side(n, BOW));
        check("reloc", S);
    }
    {  // loop / triangulation: side 1 shared, neighbours of different sizes, some with x_right and some without
        BucketBatchShape S;
        S.num_problems = 4, S.shared1 = true, S.side1 = {side(1000, TRI1)}, S.sortb = 70000;
        for (int n : {1000, 750, 500, 1}) S.side2.push_back(side(n, n == 500 ? (TRI2 & ~32u) : TRI2)), S.occupied2.push_back(nullptr);
        check("triangulation shared side 1", S);
    }
    {  // largest: spill -- 11 000 x 11 000 in the global-memory form between two small problems, the scan beyond one workgroup
        BucketBatchShape S;
        S.num_problems = 3, S.sortb = 600000, S.scan_ints = 16, S.global_form = {0, 1, 0};
        for (int n : {64, 11000, 64}) S.side1.push_back(side(n, BOW)), S.side2.push_back(side(n, 1 | 4)), S.occupied2.push_back(nullptr);
        check("spill", S);
    }
    {  // many: 300 problems
        BucketBatchShape S;
        S.num_problems = 300, S.sortb = 4096;
        for (int p = 0; p < 300; ++p) S.side1.push_back(side(64, BOW)), S.side2.push_back(side(64, 1 | 4)), S.occupied2.push_back(nullptr);
        check("many", S);
    }
    for (unsigned bit = 0; bit < 13; ++bit) {  // each optional array alone on ONE of two unshared problems: six of side 1, six of side 2, occupied
        BucketBatchShape S;
        S.num_problems = 2, S.sortb = 4096;
        S.side1 = {side(70, bit < 6 ? 1u << bit : 0), side(30, 0)};
        S.side2 = {side(50, 0), side(90, bit >= 6 && bit < 12 ? 1u << (bit - 6) : 0)};
        S.side2[1].octave = nullptr;  // (side 2 has no octaves)
        S.occupied2 = {nullptr, bit == 12 ? &one : nullptr};
        check("one optional array", S);
    }
    return layout_check_result("bucket batch arena ok");
}
