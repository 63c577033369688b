// The scratch arena: a bump allocator of 256-byte aligned pieces.  A layout is described ONCE, as a function of an Arena&, and run twice:
// on a measuring arena (no base) whose `off` is then the byte count to ask sv_ensure_scratch / sv_ensure_stage for, and on the placing
// arena over the buffer that call returned.  Plain C++ (no HIP): the same header is compiled by the host-only tests.
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

inline size_t pad(size_t bytes) { return (bytes + 255) & ~size_t(255); }

// A piece of the arena with the element count its layout asked for: what a copy into or out of the piece may move.  Converts to its
// pointer, so it stands wherever the pointer did; an empty piece (a conditional one that was not taken) is null with n == 0.
template <class T>
struct Piece {
    T* p = nullptr;
    size_t n = 0;
    operator T*() const { return p; }
    size_t bytes() const { return n * sizeof(T); }
};

// an optional array the caller did not pass is no piece: its pointer stays null (A: Arena or a type layered on it)
template <class T, class A>
Piece<T> optional_piece(A& arena, bool present, size_t n) { return present ? arena.template piece<T>(n) : Piece<T>{}; }

struct Arena {
    char* base = nullptr;
    size_t cap = 0, off = 0;
    bool overflow = false;  // placing: a piece would have ended beyond `cap` (checked once, after the layout)
    Arena() = default;      // measuring: take() only advances `off`; what it returns is null and must not reach a launch or a copy
    Arena(void* p, size_t capacity) : base((char*)p), cap(capacity) {}
    bool measuring() const { return !base; }
    template <class T>
    T* take(size_t n) {
        const size_t o = off;
        off += pad(n * sizeof(T));
        if (!base) return nullptr;
        if (off > cap) {
            overflow = true;
            return nullptr;
        }
        return (T*)(base + o);
    }
    template <class T>
    Piece<T> piece(size_t n) { return {take<T>(n), n}; }  // take() that remembers its count, also where the pointer is null (measuring, overflow)
};

// bytes a layout takes: the layout run on a measuring arena (A: Arena or a type layered on it)
template <class A = Arena, class Layout>
size_t arena_measure(Layout&& layout) {
    A m;
    layout(m);
    return m.off;
}

// The copies that cover a set of spans of the arena (Span: anything with `off` and `bytes`).  The spans are sorted by offset, in place; one
// that starts no further than `gap` bytes behind the end of the range before it joins that range.  Returns the (lo, hi) byte ranges, ascending.
template <class Span>
std::vector<std::pair<size_t, size_t>> sv_merge_ranges(std::vector<Span>& spans, size_t gap) {
    std::sort(spans.begin(), spans.end(), [](const Span& a, const Span& b) { return a.off < b.off; });
    std::vector<std::pair<size_t, size_t>> ranges;
    for (const Span& sp : spans) {
        if (!ranges.empty() && sp.off <= ranges.back().second + gap) ranges.back().second = std::max(ranges.back().second, sp.off + sp.bytes);
        else ranges.push_back({sp.off, sp.off + sp.bytes});
    }
    return ranges;
}
