// svgpu_bowdb_*: host glue of the keyframe BoW database (bowdb_kernels.hip).  The pools and the slot table are the database's own device
// allocations (grow by doubling; erased spans are reclaimed by compaction); everything a query needs besides comes from the context's
// measured arena.  A query is one upload, four launches and one read-back, with one synchronisation at its end.
#include <algorithm>
#include <mutex>

#include "sv_staged_call.h"
#include "bowdb_kernels.h"
#include "bow_compute_kernels.h"

struct svgpu_bowdb {
    int device = 0;
    int score_form = 0;
    std::mutex mtx;  // bow_database::mtx_
    uint32_t* d_ids = nullptr;
    double* d_w = nullptr;
    BowSlot* d_slots = nullptr;
    size_t pool_cap = 0, pool_used = 0, dead_entries = 0, slot_cap = 0;
    std::vector<BowSlot> slots;  // host mirror of the slot table
    int live_keyframes = 0;
    long long live_entries = 0;
    long long growths = 0, compactions = 0;
};

namespace {

constexpr size_t POOL_INITIAL = 4096, SLOTS_INITIAL = 256;

bool ascending(const uint32_t* words, int n) {
    for (int i = 1; i < n; ++i)
        if (words[i - 1] >= words[i]) return false;
    return true;
}

void release(svgpu_bowdb* db) {
    (void)hipFree(db->d_ids);
    (void)hipFree(db->d_w);
    (void)hipFree(db->d_slots);
    db->d_ids = nullptr, db->d_w = nullptr, db->d_slots = nullptr;
}

// room for `extra` more entries and `new_slots` more slots (pool and table double until they fit; the stream is idle: every call synchronises)
int reserve(svgpu_ctx* ctx, svgpu_bowdb* db, size_t extra, size_t new_slots = 1, int* syncs = nullptr) {
    hipStream_t s = ctx->stream;
    if (db->pool_used + extra > db->pool_cap) {
        size_t cap = std::max(db->pool_cap, POOL_INITIAL);
        while (db->pool_used + extra > cap) cap *= 2;
        if (cap > 0xFFFFFFFFull) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_bowdb_add: pool beyond 2^32 entries");
        uint32_t* ids = nullptr;
        double* w = nullptr;
        SV_HIP(ctx, hipMalloc(&ids, cap * sizeof(uint32_t)));
        if (hipError_t e = hipMalloc(&w, cap * sizeof(double)); e != hipSuccess) {
            (void)hipFree(ids);
            return sv_set_error(ctx, SVGPU_ERR_HIP, "hipMalloc (bowdb pool)", e);
        }
        if (db->pool_used) {
            SV_HIP(ctx, hipMemcpyAsync(ids, db->d_ids, db->pool_used * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
            SV_HIP(ctx, hipMemcpyAsync(w, db->d_w, db->pool_used * sizeof(double), hipMemcpyDeviceToDevice, s));
            SV_HIP(ctx, hipStreamSynchronize(s));
            if (syncs) ++*syncs;
        }
        if (db->pool_cap) ++db->growths;
        (void)hipFree(db->d_ids);
        (void)hipFree(db->d_w);
        db->d_ids = ids, db->d_w = w, db->pool_cap = cap;
    }
    if (db->slots.size() + new_slots > db->slot_cap) {
        size_t cap = std::max(db->slot_cap * 2, SLOTS_INITIAL);
        while (db->slots.size() + new_slots > cap) cap *= 2;
        BowSlot* t = nullptr;
        SV_HIP(ctx, hipMalloc(&t, cap * sizeof(BowSlot)));
        if (!db->slots.empty()) {
            SV_HIP(ctx, hipMemcpyAsync(t, db->slots.data(), db->slots.size() * sizeof(BowSlot), hipMemcpyHostToDevice, s));
            SV_HIP(ctx, hipStreamSynchronize(s));
            if (syncs) ++*syncs;
        }
        (void)hipFree(db->d_slots);
        db->d_slots = t, db->slot_cap = cap;
    }
    return SVGPU_OK;
}

// the live spans move to the front of fresh pools, in slot order
int compact(svgpu_ctx* ctx, svgpu_bowdb* db) {
    hipStream_t s = ctx->stream;
    std::vector<uint32_t> moves;
    std::vector<BowSlot> table = db->slots;
    uint32_t used = 0;
    for (BowSlot& sl : table) {
        if (!sl.live) {
            sl.off = 0, sl.len = 0;
            continue;
        }
        if (sl.len) moves.insert(moves.end(), {sl.off, used, sl.len});
        sl.off = used;
        used += sl.len;
    }
    uint32_t* ids = nullptr;
    double* w = nullptr;
    SV_HIP(ctx, hipMalloc(&ids, db->pool_cap * sizeof(uint32_t)));
    if (hipError_t e = hipMalloc(&w, db->pool_cap * sizeof(double)); e != hipSuccess) {
        (void)hipFree(ids);
        return sv_set_error(ctx, SVGPU_ERR_HIP, "hipMalloc (bowdb compaction)", e);
    }
    const int m = (int)(moves.size() / 3);
    int rc = SVGPU_OK;
    if (m) {
        uint32_t* d_moves = nullptr;
        rc = sv_scratch_layout(ctx, "svgpu_bowdb_erase: internal arena overflow", [&](Arena& A) { d_moves = A.take<uint32_t>(moves.size()); });
        if (!rc && hipMemcpyAsync(d_moves, moves.data(), moves.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s) != hipSuccess) rc = SVGPU_ERR_HIP;
        if (!rc) sv_launch_bowdb_move(s, db->d_ids, db->d_w, ids, w, d_moves, m);
    }
    if (!rc && hipMemcpyAsync(db->d_slots, table.data(), table.size() * sizeof(BowSlot), hipMemcpyHostToDevice, s) != hipSuccess) rc = SVGPU_ERR_HIP;
    if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = SVGPU_ERR_HIP;
    if (rc) {
        (void)hipFree(ids);
        (void)hipFree(w);
        return rc == SVGPU_ERR_HIP ? sv_set_error(ctx, SVGPU_ERR_HIP, "svgpu_bowdb_erase: compaction", hipGetLastError()) : rc;
    }
    (void)hipFree(db->d_ids);
    (void)hipFree(db->d_w);
    db->d_ids = ids, db->d_w = w;
    db->slots.swap(table);
    db->pool_used = used, db->dead_entries = 0;
    ++db->compactions;
    return SVGPU_OK;
}

// Q queries (or, with `list`, one query against listed slots) through the three passes
int query_core(svgpu_ctx* ctx, svgpu_bowdb* db, const char* who, int Q, const int32_t* q_off, const uint32_t* words, const double* weights,
               const float* min_score, float ratio, int n_reject, const int32_t* reject_slots, const int32_t* list, int n_list, int cap, int32_t* out_slots,
               uint32_t* out_common, float* out_score, int32_t* n_out, uint32_t* max_common) {
    if (!ctx || !db || Q < 1 || Q > 65535 || !q_off || q_off[0] != 0 || n_reject < 0 || (n_reject && !reject_slots) || cap < 0 || n_list < 0)
        return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    for (int q = 0; q < Q; ++q) {
        const int n = q_off[q + 1] - q_off[q];
        if (n < 0 || (n && (!words || !weights)) || !ascending(words + q_off[q], n)) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    }
    if (list ? (n_list && !out_score) : (!n_out || (cap && (!out_slots || !out_common || !out_score)))) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    std::lock_guard<std::mutex> lock(db->mtx);
    const int ns = (int)db->slots.size(), items = list ? n_list : ns;
    if (!list) {
        for (int q = 0; q < Q; ++q) n_out[q] = 0;
        if (max_common)
            for (int q = 0; q < Q; ++q) max_common[q] = 0;
    }
    if (items == 0) return SVGPU_OK;
    if (db->live_keyframes == 0) {  // nothing to scan (an empty database, or every keyframe erased)
        for (int i = 0; list && i < n_list; ++i) out_score[i] = -1.0f;
        return SVGPU_OK;
    }
    const size_t total = (size_t)q_off[Q], per = (size_t)Q * items;
    BowdbProblem P{};
    Piece<int32_t> d_off, d_rej_list, d_list;
    Piece<uint32_t> d_ids;
    Piece<double> d_w;
    Piece<float> d_min;
    uint8_t* zero_lo = nullptr;
    size_t zero_bytes = 0;
    StagedCall C;
    int rc = C.open(ctx, "svgpu_bowdb: internal arena overflow", [&](UploadArena& A) {
        P.q_off = d_off = A.piece<int32_t>((size_t)Q + 1);
        P.q_ids = d_ids = optional_piece<uint32_t>(A, words, total);
        P.q_w = d_w = optional_piece<double>(A, weights, total);
        P.min_score = d_min = optional_piece<float>(A, min_score, Q);
        d_rej_list = optional_piece<int32_t>(A, reject_slots, n_reject);
        P.list = d_list = optional_piece<int32_t>(A, list, n_list);
        // zeroed in one go: the reject bytes and the maxima
        uint8_t* rej = A.take<uint8_t>(ns);
        P.max_common = A.take<uint32_t>(Q);
        zero_lo = rej, zero_bytes = (size_t)((char*)(P.max_common + Q) - (char*)rej);
        P.reject = rej;
        P.common = A.take<uint32_t>((size_t)Q * ns);
        P.sum = A.take<double>(per);
        P.keep = A.take<uint8_t>(per);
        // what is read back, side by side
        P.score = A.take<float>(per);
        P.n_out = A.take<uint32_t>(Q);
        P.out_slots = A.take<int32_t>((size_t)Q * cap);
        P.out_common = A.take<uint32_t>((size_t)Q * cap);
        P.out_score = A.take<float>((size_t)Q * cap);
    });
    if (rc) return rc;
    hipStream_t s = C.s;
    C.up(d_off, q_off, d_ids, words, d_w, weights, d_min, min_score, d_rej_list, reject_slots, d_list, list);
    if ((rc = C.flush())) return rc;
    P.pool_ids = db->d_ids, P.pool_w = db->d_w, P.slots = db->d_slots;
    P.num_slots = ns, P.score_form = db->score_form, P.num_queries = Q, P.ratio = ratio, P.num_list = n_list, P.cap = cap;
    if (!list) {
        SV_HIP(ctx, hipMemsetAsync(zero_lo, 0, zero_bytes, s));
        sv_launch_bowdb_reject(s, d_rej_list, n_reject, const_cast<uint8_t*>(P.reject), ns);
        {
            SvProfScope prof(ctx, s, "k_bowdb_count");
            sv_launch_bowdb_count(s, P);
        }
        {
            SvProfScope prof(ctx, s, "k_bowdb_score");
            sv_launch_bowdb_score(s, P);
            sv_launch_bowdb_emit(s, P);
        }
        C.down((uint32_t*)n_out, P.n_out, Q);
        C.down(max_common, P.max_common, Q);
        C.down(out_slots, P.out_slots, (size_t)Q * cap);
        C.down(out_common, P.out_common, (size_t)Q * cap);
        C.down(out_score, P.out_score, (size_t)Q * cap);
    }
    else {
        SvProfScope prof(ctx, s, "k_bowdb_score");
        sv_launch_bowdb_score(s, P);
        C.down(out_score, P.score, n_list);
    }
    return C.finish();
}

}  // namespace

// ---- B keyframes as one submission (bow_compute_kernels.h): one growth check for the whole batch, one copy per pool span, one upload of
// the new slot records.  The pools end where B single adds leave them: both double from the same capacity until the same fill fits.
int sv_bowdb_device(const svgpu_bowdb* db) { return db->device; }
struct SvBowdbAppendState {
    std::unique_lock<std::mutex> lock;
    std::vector<BowSlot> recs;
    size_t entries = 0;
};
SvBowdbAppend::SvBowdbAppend() = default;
SvBowdbAppend::~SvBowdbAppend() = default;
int SvBowdbAppend::begin(svgpu_ctx* ctx, svgpu_bowdb* db_, int num, const int32_t* off, const uint32_t* words, const double* weights, bool on_device) {
    state.reset(new SvBowdbAppendState);
    SvBowdbAppendState* st = state.get();
    st->lock = std::unique_lock<std::mutex>(db_->mtx);
    db = db_;
    if (db->slots.size() + (size_t)num > 0x7FFFFFFFull) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_bowdb_add_batch: out of slot numbers");
    SV_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t total = (size_t)off[num];
    int rc;
    if ((rc = reserve(ctx, db, total, (size_t)num, &syncs))) return rc;
    st->recs.resize((size_t)num);
    for (int f = 0; f < num; ++f) st->recs[f] = BowSlot{(uint32_t)(db->pool_used + (size_t)off[f]), (uint32_t)(off[f + 1] - off[f]), 1u, 0u};
    st->entries = total;
    if (total) {
        const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        SV_HIP(ctx, hipMemcpyAsync(db->d_ids + db->pool_used, words, total * sizeof(uint32_t), kind, s));
        SV_HIP(ctx, hipMemcpyAsync(db->d_w + db->pool_used, weights, total * sizeof(double), kind, s));
        copies += 2;
    }
    if (num) {  // (the records live in `state` until the caller has synchronised)
        SV_HIP(ctx, hipMemcpyAsync(db->d_slots + db->slots.size(), st->recs.data(), (size_t)num * sizeof(BowSlot), hipMemcpyHostToDevice, s));
        ++copies;
    }
    return SVGPU_OK;
}
void SvBowdbAppend::commit(int32_t* slots) {
    SvBowdbAppendState* st = state.get();
    for (size_t f = 0; f < st->recs.size(); ++f) {
        slots[f] = (int32_t)db->slots.size();
        db->slots.push_back(st->recs[f]);
    }
    db->pool_used += st->entries;
    db->live_keyframes += (int)st->recs.size();
    db->live_entries += (long long)st->entries;
}

extern "C" {

int svgpu_bowdb_add_batch(svgpu_ctx* ctx, svgpu_bowdb* db, int num_frames, const int32_t* off, const uint32_t* words, const double* weights,
                          int32_t* slots) {
    const char* who = "svgpu_bowdb_add_batch: bad arguments (offsets must not descend, word ids must ascend strictly inside a frame)";
    if (!ctx || !db || num_frames < 0) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    if (num_frames == 0) return SVGPU_OK;
    if (!off || off[0] != 0 || !slots) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    for (int f = 0; f < num_frames; ++f) {
        const int n = off[f + 1] - off[f];
        if (off[f + 1] < off[f] || (n && (!words || !weights)) || !ascending(words + off[f], n)) return sv_set_error(ctx, SVGPU_ERR_INVALID, who);
    }
    SvBowdbAppend app;
    int rc = app.begin(ctx, db, num_frames, off, words, weights, false);
    if (rc) return rc;
    SV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    app.commit(slots);
    return SVGPU_OK;
}

int svgpu_bowdb_query_stage_capacity(void) { return SV_BOWDB_STAGE; }

int svgpu_bowdb_create(svgpu_ctx* ctx, int score_form, svgpu_bowdb** out) {
    if (!ctx || !out || (score_form != SVGPU_BOW_SCORE_FBOW_L2 && score_form != SVGPU_BOW_SCORE_DBOW2_L1))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_bowdb_create: bad arguments");
    svgpu_bowdb* db = new svgpu_bowdb;
    db->device = ctx->device;
    db->score_form = score_form;
    *out = db;
    return SVGPU_OK;
}

void svgpu_bowdb_destroy(svgpu_bowdb* db) {
    if (!db) return;
    (void)hipSetDevice(db->device);
    release(db);
    delete db;
}

int svgpu_bowdb_clear(svgpu_ctx* ctx, svgpu_bowdb* db) {
    if (!ctx || !db) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_bowdb_clear: bad arguments");
    std::lock_guard<std::mutex> lock(db->mtx);
    db->slots.clear();  // the allocations stay; slot numbers start again at 0
    db->pool_used = db->dead_entries = 0;
    db->live_keyframes = 0, db->live_entries = 0;
    return SVGPU_OK;
}

int svgpu_bowdb_add(svgpu_ctx* ctx, svgpu_bowdb* db, int n_words, const uint32_t* words, const double* weights, int32_t* slot) {
    if (!ctx || !db || n_words < 0 || (n_words && (!words || !weights)) || !slot || !ascending(words, n_words))
        return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_bowdb_add: bad arguments (word ids must ascend strictly)");
    std::lock_guard<std::mutex> lock(db->mtx);
    if (db->slots.size() >= 0x7FFFFFFFull) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_bowdb_add: out of slot numbers");
    SV_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = reserve(ctx, db, (size_t)n_words))) return rc;
    const BowSlot sl{(uint32_t)db->pool_used, (uint32_t)n_words, 1u, 0u};
    if (n_words) {
        SV_HIP(ctx, hipMemcpyAsync(db->d_ids + sl.off, words, (size_t)n_words * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        SV_HIP(ctx, hipMemcpyAsync(db->d_w + sl.off, weights, (size_t)n_words * sizeof(double), hipMemcpyHostToDevice, s));
    }
    SV_HIP(ctx, hipMemcpyAsync(db->d_slots + db->slots.size(), &sl, sizeof sl, hipMemcpyHostToDevice, s));
    SV_HIP(ctx, hipStreamSynchronize(s));
    *slot = (int32_t)db->slots.size();
    db->slots.push_back(sl);
    db->pool_used += (size_t)n_words;
    ++db->live_keyframes;
    db->live_entries += n_words;
    return SVGPU_OK;
}

int svgpu_bowdb_erase(svgpu_ctx* ctx, svgpu_bowdb* db, int32_t slot) {
    if (!ctx || !db) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_bowdb_erase: bad arguments");
    std::lock_guard<std::mutex> lock(db->mtx);
    if (slot < 0 || (size_t)slot >= db->slots.size() || !db->slots[slot].live) return SVGPU_OK;  // not held: ignored, as the reference does
    SV_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    BowSlot& sl = db->slots[slot];
    sl.live = 0;
    --db->live_keyframes;
    db->live_entries -= sl.len;
    db->dead_entries += sl.len;
    if (db->dead_entries * 2 > db->pool_used) return compact(ctx, db);  // more than half of what the pool holds is dead
    SV_HIP(ctx, hipMemcpyAsync(db->d_slots + slot, &sl, sizeof sl, hipMemcpyHostToDevice, s));
    SV_HIP(ctx, hipStreamSynchronize(s));
    return SVGPU_OK;
}

int svgpu_bowdb_size(svgpu_bowdb* db, int* live_keyframes, long long* live_entries) {
    if (!db) return SVGPU_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mtx);
    if (live_keyframes) *live_keyframes = db->live_keyframes;
    if (live_entries) *live_entries = db->live_entries;
    return SVGPU_OK;
}

int svgpu_bowdb_diagnostics(svgpu_bowdb* db, long long* num_slots, long long* pool_capacity, long long* pool_used, long long* num_growths,
                            long long* num_compactions) {
    if (!db) return SVGPU_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mtx);
    if (num_slots) *num_slots = (long long)db->slots.size();
    if (pool_capacity) *pool_capacity = (long long)db->pool_cap;
    if (pool_used) *pool_used = (long long)db->pool_used;
    if (num_growths) *num_growths = db->growths;
    if (num_compactions) *num_compactions = db->compactions;
    return SVGPU_OK;
}

int svgpu_bowdb_acquire(svgpu_ctx* ctx, svgpu_bowdb* db, int n_words, const uint32_t* words, const double* weights, float min_score, float ratio,
                        int n_reject, const int32_t* reject_slots, int cap, int32_t* out_slots, uint32_t* out_common, float* out_score, int32_t* n_out,
                        uint32_t* max_common) {
    const int32_t off[2] = {0, n_words};
    return query_core(ctx, db, "svgpu_bowdb_acquire: bad arguments", 1, off, words, weights, &min_score, ratio, n_reject, reject_slots, nullptr, 0, cap,
                      out_slots, out_common, out_score, n_out, max_common);
}

int svgpu_bowdb_acquire_batch(svgpu_ctx* ctx, svgpu_bowdb* db, int num_queries, const int32_t* q_off, const uint32_t* words, const double* weights,
                              const float* min_score, float ratio, int n_reject, const int32_t* reject_slots, int cap, int32_t* out_slots,
                              uint32_t* out_common, float* out_score, int32_t* n_out, uint32_t* max_common) {
    if (num_queries == 0) return ctx && db ? SVGPU_OK : sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_bowdb_acquire_batch: bad arguments");
    if (!min_score) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_bowdb_acquire_batch: bad arguments");
    return query_core(ctx, db, "svgpu_bowdb_acquire_batch: bad arguments", num_queries, q_off, words, weights, min_score, ratio, n_reject, reject_slots,
                      nullptr, 0, cap, out_slots, out_common, out_score, n_out, max_common);
}

int svgpu_bowdb_score(svgpu_ctx* ctx, svgpu_bowdb* db, int n_words, const uint32_t* words, const double* weights, int n, const int32_t* slots,
                      float* out_score) {
    if (n < 0 || (n && !slots)) return sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_bowdb_score: bad arguments");
    if (n == 0) return ctx && db ? SVGPU_OK : sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu_bowdb_score: bad arguments");
    const int32_t off[2] = {0, n_words};
    const float min_score = 0.0f;
    return query_core(ctx, db, "svgpu_bowdb_score: bad arguments", 1, off, words, weights, &min_score, 0.0f, 0, nullptr, slots, n, 0, nullptr, nullptr,
                      out_score, nullptr, nullptr);
}

}  // extern "C"
