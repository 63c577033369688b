// Host-only check of bow_compute_layout (stella_vslam_amd/csrc/bow_compute_layout.h): the shapes of tests/test_gpu_bow_compute.py -- one
// frame, 33 frames, a frame one descriptor beyond the workgroup path -- and a whole loaded map; counted pieces without overlap, the results
// as one range, the cap of the LDS path and the switch to the general sort.
#include <cstdint>
#include <cstdio>

#include "bow_compute_layout.h"
#include "layout_check.h"

static Rows rows_of(const BowComputePieces& Y, const BowComputeShape& S) {
    const size_t B = S.num_frames, N = S.total, big = S.max_big;
    return Rows{{Y.d_off, (B + 1) * 4}, {Y.desc, N * 32}, {Y.frame, N * 4}, {Y.vkey, N * 8}, {Y.fkey, N * 8}, {Y.head, (N + 1) * 4},
                {Y.kept, (N + 1) * 4}, {Y.scan_scratch, S.scan_ints * 4}, {Y.sort_key[0], big * 4}, {Y.sort_key[1], big * 4},
                {Y.sort_val[0], big * 8}, {Y.sort_val[1], big * 8}, {Y.sort_hist, big ? S.hist_ints * 4 : 0}, {Y.word, N * 4}, {Y.weight, N * 4},
                {Y.node, N * 4}, {Y.vec_off, (B + 1) * 4}, {Y.feat_off, (B + 1) * 4}, {Y.vec_word, N * 4}, {Y.vec_weight, N * 8},
                {Y.feat_key, N * 4}, {Y.feat_index, N * 4}};
}

static void check(const char* what, size_t B, size_t N, size_t max_big, size_t scan_ints) {
    BowComputeShape S;
    S.num_frames = B, S.total = N, S.max_big = max_big, S.scan_ints = scan_ints, S.hist_ints = max_big ? 64 * (max_big / 2048 + 2) + 4 : 0;
    layout_check<BowComputePieces>(
        what, [&](Arena& A, BowComputePieces& Y) { bow_compute_layout(A, S, Y); }, [&](const BowComputePieces& Y) { return rows_of(Y, S); },
        [&](const BowComputePieces& Y, const char*, size_t) {
            // the upload is one range: offsets, then descriptors
            CHECK((const char*)Y.desc.p == (const char*)Y.d_off.p + pad((B + 1) * 4));
            // the results lie next to one another, in the order they are requested: one read-back
            const char* at = (const char*)Y.word.p;
            const Row seq[] = {{Y.word, 0}, {Y.weight, 0}, {Y.node, 0}, {Y.vec_off, 0}, {Y.feat_off, 0}, {Y.vec_word, 0}, {Y.vec_weight, 0},
                               {Y.feat_key, 0}, {Y.feat_index, 0}};
            for (const Row& r : seq) {
                CHECK(r.p == at);
                at += pad(r.piece_bytes);
            }
            // the general sort's buffers exist exactly when a frame is beyond the workgroup path
            CHECK((Y.sort_key[0].p != nullptr) == (max_big > 0) && (Y.sort_hist.p != nullptr) == (max_big > 0));
            CHECK((Y.scan_scratch.p != nullptr) == (scan_ints > 0));
        });
}

int main() {
    // the cap of the workgroup path: 8 bytes per key, the count rounded up to a power of two, within the 48 KB a workgroup gets unasked
    CHECK(bowc_lds_path(0) && bowc_lds_path(1) && bowc_lds_path(SV_BOWC_LDS_MAX) && !bowc_lds_path(SV_BOWC_LDS_MAX + 1));
    CHECK(bowc_pow2(1) == 1 && bowc_pow2(63) == 64 && bowc_pow2(64) == 64 && bowc_pow2(65) == 128 && bowc_pow2(SV_BOWC_LDS_MAX) == SV_BOWC_LDS_MAX);
    CHECK(bowc_lds_bytes(SV_BOWC_LDS_MAX) == 32768 && bowc_lds_bytes(SV_BOWC_LDS_MAX) <= 48 * 1024 && bowc_lds_bytes(0) == 8);
    CHECK(bowc_lds_bytes(257) == 512 * 8);

    check("one frame", 1, 65, 0, 0);
    check("two frames, one empty", 2, 257, 0, 0);
    check("33 frames", 33, 1700, 0, 0);
    check("a frame beyond the cap", 3, 5 + (SV_BOWC_LDS_MAX + 1) + 66, SV_BOWC_LDS_MAX + 1, 0);
    check("a loaded map", 2000, 2000 * 2000, 0, 2000 * 2000 / 4096 + 9);
    check("a loaded map with one long frame", 2000, 1999 * 2000 + 5000, 5000, (1999 * 2000 + 5000) / 4096 + 9);
    return layout_check_result("bow compute arena ok");
}
