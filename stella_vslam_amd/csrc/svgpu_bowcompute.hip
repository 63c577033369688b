// svgpu_bow_compute_batch: bow_vocabulary_util::compute_bow (data/bow_vocabulary.cc:18-24) for B descriptor sets as one staged call -- one
// upload, the descent of bow_kernels.hip over the concatenated descriptors, the kernels of bow_compute_kernels.hip, one read-back -- and,
// when a database is given, the B vectors appended to its pools device to device behind the one small read-back of their offsets.
// DESIGN section 21.
#include <algorithm>
#include <cstring>
#include <vector>

#include "sv_staged_call.h"
#include "bow_compute_kernels.h"
#include "bow_compute_layout.h"
#include "sv_sort.h"

extern "C" int svgpu_bow_compute_lds_capacity(void) { return SV_BOWC_LDS_MAX; }

extern "C" int svgpu_bow_compute_batch(svgpu_ctx* ctx, const svgpu_vocabulary* vocab, int form, int level, int k, int num_frames, const int32_t* d_off,
                                       const uint8_t* desc, int32_t* word_id, float* weight, uint32_t* node, int32_t* vec_off, uint32_t* vec_word,
                                       double* vec_weight, int32_t* feat_off, uint32_t* feat_key, int32_t* feat_index, svgpu_bowdb* db, int32_t* slots,
                                       svgpu_call_stats* stats) {
    const char* who = "svgpu_bow_compute_batch: bad arguments";
    const int B = num_frames;
    if (!ctx || !vocab || B < 0 || sv_vocabulary_device(vocab) != ctx->device || (form != SVGPU_BOW_FORM_DBOW2 && form != SVGPU_BOW_FORM_FBOW) || level < 0
        || (form == SVGPU_BOW_FORM_FBOW && (k < 2 || k > 65536)) || (db && (!slots || sv_bowdb_device(db) != ctx->device)))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    if (B == 0) {
        if (stats) *stats = svgpu_call_stats{0, 0, 0};
        return SVGPU_OK;
    }
    if (!d_off || d_off[0] != 0 || !vec_off || !feat_off) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    size_t max_lds = 0, max_big = 0;
    for (int f = 0; f < B; ++f) {
        if (d_off[f + 1] < d_off[f]) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
        const size_t n = (size_t)(d_off[f + 1] - d_off[f]);
        if (bowc_lds_path(n)) max_lds = std::max(max_lds, n);
        else max_big = std::max(max_big, n);
    }
    const int N = d_off[B];
    if (N > (1 << 26) || (N > 0 && (!desc || !vec_word || !vec_weight || !feat_key || !feat_index))) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    // ---- nothing can fail on the arguments from here on
    struct Tally {
        int launches = 0, copies = 0, syncs = 0;
    } T;
    auto report = [&]() {
        if (stats) *stats = svgpu_call_stats{T.launches, T.copies, T.syncs};
    };
    if (N == 0) {  // every frame is empty: empty vectors, and B empty keyframes for the database
        if (db) {
            const std::vector<int32_t> zero((size_t)B + 1, 0);
            SvBowdbAppend app;
            const int rc = app.begin(ctx, db, B, zero.data(), nullptr, nullptr, true);
            if (rc) return rc;
            SV_HIP(ctx, hipStreamSynchronize(ctx->stream));
            app.commit(slots);
            T.copies = app.copies, T.syncs = app.syncs + 1;
        }
        for (int f = 0; f <= B; ++f) vec_off[f] = feat_off[f] = 0;
        report();
        return SVGPU_OK;
    }

    BowComputeShape S;
    S.num_frames = (size_t)B, S.total = (size_t)N, S.max_big = max_big;
    S.scan_ints = sv_scan_scratch_ints((size_t)N), S.hist_ints = max_big ? sv_sort_hist_ints(max_big) : 0;
    BowComputePieces Y;
    StagedCall C;
    int rc = C.open(ctx, "svgpu_bow_compute_batch: internal arena overflow", [&](UploadArena& A) { bow_compute_layout(A, S, Y); });
    if (rc) return rc;
    hipStream_t s = C.s;
    C.up(Y.d_off, d_off);
    C.up(Y.desc, (const uint32_t*)desc);
    if ((rc = C.flush())) return rc;
    ++T.copies;

    BowComputeProblem P{};
    P.num_frames = B, P.total = N, P.dbow2 = form == SVGPU_BOW_FORM_DBOW2;
    P.d_off = Y.d_off, P.frame = Y.frame, P.word = Y.word, P.weight = Y.weight, P.node = Y.node, P.vkey = Y.vkey, P.fkey = Y.fkey;
    P.head = Y.head, P.kept = Y.kept, P.vec_off = Y.vec_off, P.feat_off = Y.feat_off, P.vec_word = Y.vec_word, P.feat_key = Y.feat_key;
    P.vec_weight = Y.vec_weight, P.feat_index = Y.feat_index;
    {
        SvProfScope ps(ctx, s, form == SVGPU_BOW_FORM_FBOW ? "k_fbow_descend" : "k_bow_descend");
        sv_launch_bow_descend(s, vocab, Y.desc, N, level, form == SVGPU_BOW_FORM_FBOW ? k : 0, Y.word, Y.weight, Y.node);
        ++T.launches;
    }
    {
        SvProfScope ps(ctx, s, "k_bowc_sort");
        sv_launch_bowc_owner(s, P);
        ++T.launches;
        if (max_lds > 0) {
            sv_launch_bowc_sort_lds(s, P, (int)max_lds);
            ++T.launches;
        }
        // frames beyond the workgroup path, one after another (their launches depend on how many there are, and on their lengths)
        for (int f = 0; f < B && max_big; ++f) {
            const int first = d_off[f], n = d_off[f + 1] - first;
            if (bowc_lds_path((size_t)n)) continue;
            unsigned* const keys[2] = {Y.sort_key[0], Y.sort_key[1]};
            unsigned long long* const vals[2] = {Y.sort_val[0], Y.sort_val[1]};
            for (int which = 0; which < 2; ++which) {
                sv_launch_bowc_big_init(s, P, first, n, which, keys[0], vals[0]);
                const int at = sv_sort_pairs(s, keys, vals, 0, n, 32, Y.sort_hist);
                sv_launch_bowc_big_pack(s, P, first, n, which, keys[at], vals[at]);
                T.launches += 2;  // (the general sort's own launches are not counted, as in the other batched calls)
            }
        }
    }
    {
        SvProfScope ps(ctx, s, "k_bowc_emit");
        sv_launch_bowc_heads(s, P);
        T.launches += 1 + sv_scan_i32(s, Y.head, N, Y.scan_scratch);
        T.launches += sv_scan_i32(s, Y.kept, N, Y.scan_scratch);
        sv_launch_bowc_emit(s, P);
        sv_launch_bowc_normalise(s, P);
        T.launches += 2;
    }
    SvBowdbAppend app;
    if (db) {  // the host makes the slot records: it needs the B + 1 offsets, the call's first synchronisation
        C.keep(Y.vec_off);
        SV_HIP(ctx, hipGetLastError());
        if ((rc = C.D.fetch(ctx, s, C.A))) return rc;
        SV_HIP(ctx, hipStreamSynchronize(s));
        ++T.copies, ++T.syncs;
        C.D.items.clear();
        if ((rc = app.begin(ctx, db, B, C.host(Y.vec_off.p), Y.vec_word, Y.vec_weight, true))) return rc;
        T.copies += app.copies, T.syncs += app.syncs;
    }
    C.down(word_id, Y.word), C.down(weight, Y.weight), C.down((int32_t*)node, Y.node);
    C.down(vec_off, Y.vec_off), C.down(feat_off, Y.feat_off);
    // the vectors' lengths are known behind the synchronisation only: their pieces come back whole into the mirror, the used part goes on
    C.keep(Y.vec_word), C.keep(Y.vec_weight), C.keep(Y.feat_key), C.keep(Y.feat_index);
    {
        std::vector<Downloads::Item> items = C.D.items;
        T.copies += (int)sv_merge_ranges(items, 32768).size();  // the results lie next to one another: one read-back
    }
    rc = C.finish();
    ++T.syncs;
    if (rc) return rc;
    const size_t nv = (size_t)vec_off[B], nf = (size_t)feat_off[B];
    std::memcpy(vec_word, C.host(Y.vec_word.p), nv * sizeof(uint32_t));
    std::memcpy(vec_weight, C.host(Y.vec_weight.p), nv * sizeof(double));
    std::memcpy(feat_key, C.host(Y.feat_key.p), nf * sizeof(uint32_t));
    std::memcpy(feat_index, C.host(Y.feat_index.p), nf * sizeof(int32_t));
    if (db) app.commit(slots);
    report();
    return SVGPU_OK;
}
