// The call protocol of the entry points that take host arrays: one upload through the page-locked mirror of the scratch arena, the
// launches on the context's stream, one read-back through the mirror and one synchronisation.  UploadArena and Downloads are its two
// halves; StagedCall owns the sequence.
#pragma once
#include <algorithm>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "svgpu_internal.h"

// The scratch arena (sv_arena.h) with batched uploads: with a page-locked mirror of the arena (ctx->h_stage) every host array is copied to the
// mirror at its arena offset and ONE host-to-device copy of the touched range follows (flush) -- the runtime turns every small copy from
// pageable memory into a staging kernel of its own (~5 us each on the stream: ten of them per cell-matcher call were half of what the call
// waited for).  Device-only pieces inside the range receive stale bytes, harmlessly: the kernels that produce them run behind the copy.
// On a measuring arena upload / put / flush do nothing.
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
    // take n elements for an optional host array and, when `fresh`, upload it; no source: no piece, null.  The first failure stays in `rc`.
    template <class T>
    T* put(svgpu_ctx* ctx, hipStream_t s, const T* src, size_t n, bool fresh, int& rc) {
        if (!src) return nullptr;
        T* dst = take<T>(n);
        if (fresh && !rc) rc = upload(ctx, s, dst, src, n * sizeof(T));
        return dst;
    }
    int flush(svgpu_ctx* ctx, hipStream_t s) {
        if (mirror && up_hi > up_lo) SV_HIP(ctx, hipMemcpyAsync(base + up_lo, mirror + up_lo, up_hi - up_lo, hipMemcpyHostToDevice, s));
        up_lo = ~size_t(0), up_hi = 0;
        return SVGPU_OK;
    }
};

// Batched read-backs, the counterpart of UploadArena::upload: results that live in the arena are requested with add(), fetch() copies the
// range(s) that cover them into the page-locked mirror (requests closer than 32 KB share one copy: sv_merge_ranges), and after the stream
// has been synchronised scatter() hands them to the caller's arrays (an item without a destination stays in the mirror).
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
        for (const auto& [lo, hi] : sv_merge_ranges(items, 32768))
            SV_HIP(ctx, hipMemcpyAsync(A.mirror + lo, A.base + lo, hi - lo, hipMemcpyDeviceToHost, s));
        return SVGPU_OK;
    }
    void scatter(const UploadArena& A) const {
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

    // `layout(UploadArena&)` returns void, or an int status (the layouts that upload as they take, through UploadArena::put): that of the
    // placing run is returned as it is
    template <class Layout>
    int open(svgpu_ctx* ctx_, const char* overflow_msg, Layout&& layout) {
        ctx = ctx_;
        SV_HIP(ctx, hipSetDevice(ctx->device));
        s = ctx->stream;
        const size_t need = arena_measure<UploadArena>(layout);
        int r;
        if ((r = sv_ensure_scratch(ctx, need))) return r;
        if ((r = sv_ensure_stage(ctx, need))) return r;
        A = UploadArena(ctx, ctx->h_stage);
        if constexpr (std::is_void_v<decltype(layout(A))>) layout(A);
        else if ((r = layout(A))) return r;
        return A.overflow ? sv_set_error(ctx, SVGPU_ERR_INVALID, overflow_msg) : SVGPU_OK;
    }
    template <class T>
    void up(T* dst, const T* src, size_t count) {
        if (!rc && src) rc = A.upload(ctx, s, dst, src, count * sizeof(T));
    }
    template <class T>
    void up(Piece<T> dst, const T* src) { up(dst.p, src, dst.n); }
    template <class T>
    void up(Piece<T> dst, const T* src, size_t count) { if (fits(count, dst.n)) up(dst.p, src, count); }
    int flush() { return rc ? rc : A.flush(ctx, s); }
    // the place of an arena piece in the mirror
    template <class T>
    T* host(T* dev) const {
        return (T*)(A.mirror + ((char*)dev - A.base));
    }
    // the same for a piece the caller fills there itself: its bytes travel with the next flush
    template <class T>
    T* stage(T* dev, size_t count) {
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
