// Argument checks that more than one entry point makes.  Plain C++ (no HIP): tests/arena_check.cpp compiles this header alone.
#pragma once
#include <cmath>
#include <cstdint>

inline bool sv_positive_finite(double v) { return std::isfinite(v) && v > 0.0; }

// p: quaternion (4), translation (3), scale -- all finite, the quaternion of unit norm within 1e-9, the scale positive
inline bool sv_sim3_ok(const double* p) {
    double n2 = 0.0;
    for (int k = 0; k < 8; ++k)
        if (!std::isfinite(p[k])) return false;
    for (int k = 0; k < 4; ++k) n2 += p[k] * p[k];
    return std::fabs(n2 - 1.0) <= 1e-9 && p[7] > 0.0;
}

// CSR offsets of n rows (n + 1 entries): the first is 0 and none is smaller than the one before it
inline bool sv_offsets_ok(const int32_t* off, int n) {
    if (off[0] != 0) return false;
    for (int k = 0; k < n; ++k)
        if (off[k + 1] < off[k]) return false;
    return true;
}
