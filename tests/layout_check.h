// What the host-only layout checks (tests/*_arena_check.cpp) share: the CHECK macro with its failure count, and layout_check(), which runs
// one scratch layout (stella_vslam_amd/csrc/*_layout.h) the way an entry point does -- on a measuring arena, then on a placing arena -- over
// a host buffer (pointers compared, never dereferenced) and compares it with the program's own table of bytes per piece.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <functional>
#include <memory>
#include <vector>

#include "sv_arena.h"

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// one row of a program's table: a piece, and the bytes the kernels or the copies touch there, written out by hand
struct Row {
    const char* p;
    size_t piece_bytes, touched;
    template <class T>
    Row(Piece<T> piece, size_t bytes) : p((const char*)piece.p), piece_bytes(piece.bytes()), touched(bytes) {}
};
using Rows = std::vector<Row>;

// layout(Arena&, Pieces&) fills the pieces; table(const Pieces&) gives the rows; extra(const Pieces&, base, need) checks what only this
// layout promises, on the placed pieces.
//   measuring: every piece is null and still carries its count
//   placing over exactly the measured size: no overflow, the same final offset
//   every row: the hand-written byte count is the piece's own
//   the rows sorted by address: 256-byte aligned, no overlap, all inside the measured size
//   one byte less: overflow
template <class Pieces, class Layout, class Table, class Extra>
void layout_check(const char* name, Layout&& layout, Table&& table, Extra&& extra) {
    Pieces M{};
    const size_t need = arena_measure([&](Arena& A) { layout(A, M); });
    CHECK(need % 256 == 0);
    for (const Row& r : table(M)) CHECK(r.p == nullptr && r.piece_bytes == r.touched);

    const std::unique_ptr<char[]> buf(new char[need + 512]);  // (never touched: a global-BA sized arena costs address space only)
    const char* const base = buf.get();
    Pieces Y{};
    Arena A(buf.get(), need);
    layout(A, Y);
    CHECK(!A.overflow && A.off == need);
    Rows rows = table(Y);
    for (const Row& r : rows) CHECK(r.piece_bytes == r.touched);
    std::sort(rows.begin(), rows.end(), [](const Row& a, const Row& b) { return std::less<const char*>()(a.p, b.p); });
    const char* end = base;
    for (const Row& r : rows) {
        if (!r.touched) continue;  // (an empty piece, or a zero-length one: it may sit anywhere, the very end included)
        CHECK(r.p != nullptr && (r.p - base) % 256 == 0 && r.p >= end && r.p + r.touched <= base + need);
        if (r.p) end = r.p + r.touched;
    }
    extra(Y, base, need);
    if (need > 0) {
        Arena S(buf.get(), need - 1);
        Pieces Z{};
        layout(S, Z);
        CHECK(S.overflow && S.off == need);
        for (const Row& r : table(Z)) CHECK(r.piece_bytes == r.touched);  // the counts survive the overflow
    }
    std::printf("ok %s: %zu bytes, %zu pieces\n", name, need, rows.size());
}
template <class Pieces, class Layout, class Table>
void layout_check(const char* name, Layout&& layout, Table&& table) {
    layout_check<Pieces>(name, layout, table, [](const Pieces&, const char*, size_t) {});
}

// the end of main(): the marker the pytest side looks for, or the count of what failed
inline int layout_check_result(const char* marker) {
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("%s\n", marker);
    return 0;
}
