// Host-only check of the scratch arena (stella_vslam_amd/csrc/sv_arena.h) and of the shared argument checks (sv_validate.h): built and run
// by tests/test_arena_layouts.py.
// Every layout is run on a measuring arena and on placing arenas over a host buffer (the pointers are compared, never dereferenced).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <limits>
#include <utility>
#include <vector>

#include "layout_check.h"
#include "sv_arena.h"
#include "sv_validate.h"

// a layout records what every take returned
using Layout = std::function<void(Arena&, std::vector<void*>&)>;

static void check_layout(const char* name, const Layout& lay) {
    Arena M;
    std::vector<void*> got;
    lay(M, got);
    CHECK(M.measuring());
    CHECK(!M.overflow);
    for (void* p : got) CHECK(p == nullptr);  // measuring mode never hands out a pointer
    const size_t need = M.off;
    CHECK(need % 256 == 0);

    std::vector<char> buf(need + 512);
    char* const base = buf.data();
    {  // exactly the measured capacity: no overflow, same final offset, every piece inside [base, base + need)
        Arena A(base, need);
        std::vector<void*> p;
        lay(A, p);
        CHECK(!A.overflow);
        CHECK(A.off == need);
        CHECK(p.size() == got.size());
        for (void* q : p) CHECK(q != nullptr && (char*)q >= base && (char*)q <= base + need && ((char*)q - base) % 256 == 0);
    }
    if (need > 0) {  // one byte short: the flag latches, the offending take returns null, nothing points out of range
        Arena A(base, need - 1);
        std::vector<void*> p;
        lay(A, p);
        CHECK(A.overflow);
        CHECK(A.off == need);
        bool any_null = false;
        for (void* q : p) {
            if (!q) any_null = true;
            else CHECK((char*)q >= base && (char*)q < base + (need - 1));
        }
        CHECK(any_null);
    }
    std::printf("ok %s: %zu bytes, %zu takes\n", name, need, got.size());
}

// the read-back ranges of Downloads::fetch: spans (offset, bytes) closer than `gap` share one copy
struct Span {
    size_t off, bytes;
};
using Spans = std::vector<Span>;
using Ranges = std::vector<std::pair<size_t, size_t>>;
static Ranges merged(Spans spans) { return sv_merge_ranges(spans, 32768); }
static void check_merge_covers(const Spans& spans, const Ranges& ranges) {
    for (size_t k = 0; k < ranges.size(); ++k) {
        CHECK(ranges[k].first < ranges[k].second);                        // no empty range
        if (k) CHECK(ranges[k].first > ranges[k - 1].second + 32768);     // ascending, and really further apart than the gap
    }
    for (const auto& sp : spans) {
        bool inside = false;
        for (const auto& r : ranges) inside = inside || (r.first <= sp.off && sp.off + sp.bytes <= r.second);
        CHECK(inside);
    }
}
static void check_merge() {
    CHECK(merged({}).empty());
    CHECK((merged({{512, 100}}) == Ranges{{512, 612}}));
    {  // end to start exactly the gap: one copy; one byte more: two
        const Spans near{{0, 256}, {256 + 32768, 64}}, far{{0, 256}, {256 + 32769, 64}};
        CHECK((merged(near) == Ranges{{0, 256 + 32768 + 64}}));
        CHECK((merged(far) == Ranges{{0, 256}, {256 + 32769, 256 + 32769 + 64}}));
        check_merge_covers(near, merged(near));
        check_merge_covers(far, merged(far));
    }
    {  // unsorted input; the spans come back sorted
        Spans in{{200000, 16}, {0, 4}, {100000, 8}, {256, 1024}};
        check_merge_covers(in, merged(in));
        CHECK((sv_merge_ranges(in, 32768) == Ranges{{0, 1280}, {100000, 100008}, {200000, 200016}}));
        CHECK(in[0].off == 0 && in[1].off == 256 && in[2].off == 100000 && in[3].off == 200000);
    }
    {  // a span wholly inside an earlier one: the end does not shrink
        const Spans in{{1000, 5000}, {2000, 100}};
        CHECK((merged(in) == Ranges{{1000, 6000}}));
    }
    {  // a chain: each near the one before it, the first and the last far apart
        const Spans in{{0, 100}, {30000, 100}, {60000, 100}};
        CHECK((merged(in) == Ranges{{0, 60100}}));
        check_merge_covers(in, merged(in));
    }
}

static void check_validate() {
    {
        const int32_t a[] = {0}, b[] = {0, 0, 3}, c[] = {1, 2}, d[] = {0, 3, 2};
        CHECK(sv_offsets_ok(a, 0));
        CHECK(sv_offsets_ok(b, 2));
        CHECK(!sv_offsets_ok(c, 1));
        CHECK(!sv_offsets_ok(d, 2));
    }
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    CHECK(sv_positive_finite(1e-300) && !sv_positive_finite(0.0) && !sv_positive_finite(-1.0) && !sv_positive_finite(nan) && !sv_positive_finite(inf));
    const double id[8] = {0, 0, 0, 1, 1, 2, 3, 0.5};
    CHECK(sv_sim3_ok(id));
    for (const double off : {0.9e-9, -0.9e-9, 1.1e-9, -1.1e-9}) {  // squared norm 1 + off (w alone carries the quaternion)
        double p[8] = {0, 0, 0, std::sqrt(1.0 + off), 1, 2, 3, 0.5};
        const bool inside = std::fabs(p[3] * p[3] - 1.0) <= 1e-9;
        CHECK(inside == (std::fabs(off) < 1e-9));  // the rounding of the square root does not move the case across the bound
        CHECK(sv_sim3_ok(p) == (std::fabs(off) < 1e-9));
    }
    for (const double scale : {0.0, -1.0, -0.5}) {
        double p[8] = {0, 0, 0, 1, 1, 2, 3, scale};
        CHECK(!sv_sim3_ok(p));
    }
    for (int k = 0; k < 8; ++k)
        for (const double bad : {nan, inf}) {
            double p[8] = {0, 0, 0, 1, 1, 2, 3, 0.5};
            p[k] = bad;
            CHECK(!sv_sim3_ok(p));
        }
}

int main() {
    check_merge();
    check_validate();
    CHECK(pad(0) == 0 && pad(1) == 256 && pad(255) == 256 && pad(256) == 256 && pad(257) == 512);

    check_layout("plain", [](Arena& A, std::vector<void*>& p) {
        p.push_back(A.take<uint32_t>(8 * 100));
        p.push_back(A.take<float>(100));
        p.push_back(A.take<double>(3 * 100));
    });
    check_layout("odd sizes", [](Arena& A, std::vector<void*>& p) {
        p.push_back(A.take<uint8_t>(1));
        p.push_back(A.take<uint8_t>(255));
        p.push_back(A.take<uint8_t>(257));
        p.push_back(A.take<uint16_t>(333));
        p.push_back(A.take<double>(7));
    });
    check_layout("zero-length takes", [](Arena& A, std::vector<void*>& p) {
        const size_t before = A.off;
        A.take<int>(0);  // (takes nothing: may sit at the very end of the buffer)
        if (A.off != before) ++failures;
        p.push_back(A.take<int>(5));
        A.take<double>(0);
        p.push_back(A.take<char>(1000));
    });
    for (int on = 0; on < 2; ++on)
        for (int n : {1, 64, 1000}) {
            char name[64];
            std::snprintf(name, sizeof name, "conditional group %s, n %d", on ? "on" : "off", n);
            check_layout(name, [on, n](Arena& A, std::vector<void*>& p) {
                p.push_back(A.take<float>(n));
                if (on) {
                    p.push_back(A.take<int32_t>((size_t)n + 1));
                    p.push_back(A.take<uint8_t>(n));
                }
                p.push_back(A.take<double>(2 * (size_t)n));
            });
        }
    {  // the group really changes the size, and measuring twice gives the same answer
        auto lay = [](bool on) {
            return [on](Arena& A) {
                A.take<float>(1000);
                if (on) A.take<int>(1001);
            };
        };
        CHECK(arena_measure(lay(true)) == arena_measure(lay(false)) + pad(1001 * 4));
        CHECK(arena_measure(lay(true)) == arena_measure(lay(true)));
    }
    {  // after an overflow every later take is null too, and `off` keeps counting (it is still the size that would have been needed)
        std::vector<char> buf(1024);
        Arena A(buf.data(), 512);
        CHECK(A.take<char>(256) == buf.data());
        CHECK(A.take<char>(257) == nullptr);
        CHECK(A.overflow);
        CHECK(A.take<char>(1) == nullptr);
        CHECK(A.off == 256 + 512 + 256);
    }
    {  // a piece is its take with the count beside it, and stands where the pointer did
        std::vector<char> buf(1024);
        Arena A(buf.data(), 1024), T(buf.data(), 1024);
        const Piece<double> a = A.piece<double>(7);
        const Piece<uint8_t> b = A.piece<uint8_t>(3);
        CHECK(a.p == T.take<double>(7) && b.p == T.take<uint8_t>(3) && A.off == T.off);
        CHECK(a.n == 7 && a.bytes() == 56 && b.n == 3 && b.bytes() == 3);
        double* q = a;
        const void* v = b;
        CHECK(q == a.p && v == b.p && a + 2 == a.p + 2);
        Arena M;  // measuring: null, the count kept
        const Piece<double> m = M.piece<double>(7);
        CHECK(m.p == nullptr && m.n == 7 && m.bytes() == 56 && M.off == 256 && !M.overflow);
        const Piece<char> o = A.piece<char>(513);  // overflow: null, the count kept, and so in every later piece
        const Piece<int32_t> l = A.piece<int32_t>(1);
        CHECK(A.overflow && o.p == nullptr && o.n == 513 && l.p == nullptr && l.n == 1 && l.bytes() == 4);
        const Piece<float> none{};  // a conditional piece that was not taken
        float* f = none;
        CHECK(f == nullptr && none.n == 0 && none.bytes() == 0);
    }
    return layout_check_result("arena ok");
}
