// The call protocol of the entry points that take host arrays: one upload through the page-locked mirror of the scratch arena, the
// launches on the context's stream, one read-back through the mirror and one synchronisation.  UploadArena and Downloads are its two
// halves; StagedCall owns the sequence.
#pragma once
#include <algorithm>
#include <cassert>
#include <cstring>
#include <utility>
#include <vector>

#include "svgpu_internal.h"

// The scratch arena (sv_arena.h) with batched uploads: with a page-locked mirror of the arena (ctx->h_stage) every host array is copied to the
// mirror at its arena offset and ONE host-to-device copy of the touched range follows (flush) -- the runtime turns every small copy from
// pageable memory into a staging kernel of its own (~5 us each on the stream: ten of them per cell-matcher call were half of what the call
// waited for).  Device-only pieces inside the range receive stale bytes, harmlessly: the kernels that produce them run behind the copy.
// Without a mirror (the bucket matcher's calls) every upload is a copy of its own.  On a measuring arena upload / flush do nothing.
struct UploadArena : Arena {
    char* mirror = nullptr;
    size_t up_lo = ~size_t(0), up_hi = 0;
    UploadArena() = default;
    explicit UploadArena(svgpu_ctx* ctx, char* mirror_ = nullptr) : Arena(ctx->d_scratch, ctx->scratch_bytes), mirror(mirror_) {}
    int upload(svgpu_ctx* ctx, hipStream_t s, void* dst, const void* src, size_t bytes) {
        if (!dst || !bytes) return SVGPU_OK;
        if (!mirror) {
            SV_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
            return SVGPU_OK;
        }
        const size_t o = (size_t)((char*)dst - base);
        memcpy(mirror + o, src, bytes);
        up_lo = std::min(up_lo, o);
        up_hi = std::max(up_hi, o + bytes);
        return SVGPU_OK;
    }
    int flush(svgpu_ctx* ctx, hipStream_t s) {
        if (mirror && up_hi > up_lo) SV_HIP(ctx, hipMemcpyAsync(base + up_lo, mirror + up_lo, up_hi - up_lo, hipMemcpyHostToDevice, s));
        up_lo = ~size_t(0), up_hi = 0;
        return SVGPU_OK;
    }
};

// Batched read-backs, the counterpart of UploadArena::upload: results that live in the arena are requested with add(), fetch() copies the
// range(s) that cover them into the page-locked mirror (requests closer than 32 KB share one copy: sv_merge_ranges), and after the stream
// has been synchronised scatter() hands them to the caller's arrays (an item without a destination stays in the mirror).  Without a
// mirror fetch() copies every item straight to its destination, in request order, and scatter() has nothing left to do.
struct Downloads {
    struct Item {
        void* dst;
        size_t off, bytes;
    };
    std::vector<Item> items;
    // an optional output the caller did not ask for (no destination) is no request ...
    void add(const UploadArena& A, void* dst, const void* src, size_t bytes) {
        if (dst) keep(A, src, bytes, dst);
    }
    // ... while keep() fetches into the mirror whether or not scatter() has somewhere to hand the bytes
    void keep(const UploadArena& A, const void* src, size_t bytes, void* dst = nullptr) {
        if (bytes) items.push_back({dst, (size_t)((const char*)src - A.base), bytes});
    }
    int fetch(svgpu_ctx* ctx, hipStream_t s, const UploadArena& A) {
        if (!A.mirror) {
            for (const Item& it : items) SV_HIP(ctx, hipMemcpyAsync(it.dst, A.base + it.off, it.bytes, hipMemcpyDeviceToHost, s));
            return SVGPU_OK;
        }
        for (const auto& [lo, hi] : sv_merge_ranges(items, 32768))
            SV_HIP(ctx, hipMemcpyAsync(A.mirror + lo, A.base + lo, hi - lo, hipMemcpyDeviceToHost, s));
        return SVGPU_OK;
    }
    void scatter(const UploadArena& A) const {
        if (!A.mirror) return;
        for (const Item& it : items)
            if (it.dst) memcpy(it.dst, A.mirror + it.off, it.bytes);
    }
};

// One synchronous call on host arrays.  open() sizes both buffers from the layout and places it; up() copies host arrays to their pieces'
// places in the mirror and flush() sends the touched range; the caller launches on `s`; down() names the results and finish() brings them
// back.  A Piece (sv_arena.h) carries the count its layout gave it, so up / down / keep / stage on a piece move the whole of it; a transfer
// that is deliberately shorter names its count, in elements, and one longer than its piece fails the call instead of being copied.  The
// forms on plain pointers, with a count, serve the layouts that place their pieces straight into a kernel's problem struct.
struct StagedCall {
    svgpu_ctx* ctx = nullptr;
    hipStream_t s = nullptr;
    UploadArena A;
    Downloads D;
    int rc = SVGPU_OK;  // the first failure of an up(), or a count beyond its piece

    const char* overflow_msg = "";
    bool mirrored = true;

    // `mirrored == false`: no page-locked mirror is asked for; up() is a copy of its own per array and down() one per result, straight
    // to the caller's array (keep / stage assert a mirror: there is none to read them in)
    template <class Layout>
    int open(svgpu_ctx* ctx_, const char* overflow_msg_, Layout&& layout, bool mirrored_ = true) {
        ctx = ctx_;
        overflow_msg = overflow_msg_;
        mirrored = mirrored_;
        SV_HIP(ctx, hipSetDevice(ctx->device));
        s = ctx->stream;
        bool survived;
        return reopen(layout, survived);
    }
    // A further pass of the same call under another layout: measures, grows scratch and mirror, places.  `survived`: the scratch arena
    // did not regrow, so what the passes before left in it is still there (for the pieces the new layout places where the old one did).
    // Upload range and read-back requests start empty.
    template <class Layout>
    int reopen(Layout&& layout, bool& survived) {
        const size_t need = arena_measure<UploadArena>(layout);
        survived = need <= ctx->scratch_bytes;
        int r;
        if ((r = sv_ensure_scratch(ctx, need))) return r;
        if (mirrored && (r = sv_ensure_stage(ctx, need))) return r;
        A = UploadArena(ctx, mirrored ? ctx->h_stage : nullptr);
        D.items.clear();
        layout(A);
        return A.overflow ? sv_set_error(ctx, SVGPU_ERR_INVALID, overflow_msg) : SVGPU_OK;
    }
    // one small value in the middle of the call, with a synchronisation of its own (the candidate total of a two-pass matcher)
    template <class T>
    int read_now(T* dst, const T* src) {
        SV_HIP(ctx, hipMemcpyAsync(dst, src, sizeof(T), hipMemcpyDeviceToHost, s));
        SV_HIP(ctx, hipStreamSynchronize(s));
        return SVGPU_OK;
    }
    template <class T>
    void up(T* dst, const T* src, size_t count) {
        if (!rc && src) rc = A.upload(ctx, s, dst, src, count * sizeof(T));
    }
    template <class T>
    void up(Piece<T> dst, const T* src) { up(dst.p, src, dst.n); }
    template <class T>
    void up(Piece<T> dst, const T* src, size_t count) { if (fits(count, dst.n)) up(dst.p, src, count); }
    template <class T, class U, class... More>  // several whole pieces, as (piece, source) pairs, in the order written
    void up(Piece<T> dst, const T* src, Piece<U> dst2, const U* src2, More... more) { up(dst, src), up(dst2, src2, more...); }
    int flush() { return rc ? rc : A.flush(ctx, s); }
    // the place of an arena piece in the mirror
    template <class T>
    T* host(T* dev) const {
        return (T*)(A.mirror + ((char*)dev - A.base));
    }
    // the same for a piece the caller fills there itself: its bytes travel with the next flush
    template <class T>
    T* stage(T* dev, size_t count) {
        assert(mirrored);
        const size_t o = (size_t)((char*)dev - A.base);
        A.up_lo = std::min(A.up_lo, o);
        A.up_hi = std::max(A.up_hi, o + count * sizeof(T));
        return host(dev);
    }
    template <class T>
    T* stage(Piece<T> dev) { return stage(dev.p, dev.n); }
    template <class T>
    void down(T* dst, const T* src, size_t count) {
        D.add(A, dst, src, count * sizeof(T));
    }
    // a result wanted in the mirror only: after finish() the caller reads it at host(src)
    template <class T>
    void keep(const T* src, size_t count) {
        assert(mirrored);
        D.keep(A, src, count * sizeof(T));
    }
    template <class T>
    void down(T* dst, Piece<T> src) { down(dst, src.p, src.n); }
    template <class T>
    void down(T* dst, Piece<T> src, size_t count) { if (fits(count, src.n)) down(dst, src.p, count); }
    template <class T>
    void keep(Piece<T> src) { keep(src.p, src.n); }
    bool fits(size_t count, size_t n) {  // a count beside a piece may fall short of it, never exceed it: nothing is copied then and the call fails
        if (count > n && !rc) rc = sv_set_error(ctx, SVGPU_ERR_INVALID, "svgpu: internal count mismatch (a transfer longer than its arena piece)");
        return count <= n;
    }
    int finish() {
        SV_HIP(ctx, hipGetLastError());
        const int r = D.fetch(ctx, s, A);
        if (r) return r;
        SV_HIP(ctx, hipStreamSynchronize(s));
        D.scatter(A);
        return rc;
    }
};
