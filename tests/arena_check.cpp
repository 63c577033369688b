// Host-only check of the scratch arena (stella_vslam_amd/csrc/sv_arena.h): built and run by tests/test_arena.py.
// Every layout is run on a measuring arena and on placing arenas over a host buffer (the pointers are compared, never dereferenced).
#include <cstdint>
#include <cstdio>
#include <functional>
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

int main() {
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
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("arena ok\n");
    return 0;
}
