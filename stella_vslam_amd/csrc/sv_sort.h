// Hand-written device sorts / scans shared by the BA structure builder (ba_pairs.hip), the grid and bucket candidate lists
// (match_kernels.hip, bucket_kernels.hip) and through them every matcher call.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

// in-place exclusive scan of data[0 .. n), total to data[n]; 0 <= n <= SV_SCAN_MAX, data 16-byte aligned (the start of an arena piece is).
// Returns the launches it issued.  scratch == nullptr: ONE launch of one workgroup that walks tiles of 16 k elements, correct for every n
// (~9 us per tile: for callers that must not add launches or have no scratch).  With `scratch` = sv_scan_scratch_ints(n) ints (0 up to
// 16 k elements, where the form is the same one launch): tile sums, their scan, and a scan of every tile behind its offset, 3 launches.
#define SV_SCAN_MAX (INT32_MAX - 16384)  // (the one-workgroup kernel steps its int index a tile beyond n)
size_t sv_scan_scratch_ints(size_t n);
int sv_scan_i32(hipStream_t s, int* data, int n, int* scratch);
// stable least-significant-digit radix sort (6-bit digits) of n (u32 key, u64 value) pairs by the low `bits` key bits, ping-ponging between
// the two buffer sets; `hist` = sv_sort_hist_ints(n) ints of scratch.  The data starts in set `start`; returns the set that holds the result
// (start ^ (passes & 1)).  Key bits above `bits` travel with the key and order nothing: the last digit is cut where `bits` ends.
int sv_sort_passes(int bits);
size_t sv_sort_hist_ints(size_t n);
// n_dev != null: the element count is read on the device (*n_dev <= n; n sizes the launches and the scratch)
int sv_sort_pairs(hipStream_t s, unsigned* const keys[2], unsigned long long* const vals[2], int start, int n, int bits, int* hist, const int* n_dev = nullptr);
// n <= SV_SORT_SMALL_MAX (key, index) pairs sorted by (key, index) in ONE workgroup's LDS (bitonic network on the 64-bit composites)
#define SV_SORT_SMALL_MAX 16384
bool sv_sort_small(hipStream_t s, const unsigned* keys_in, const int* idx_in, int n, unsigned* keys_out, int* idx_out);  // false: not available on this device
// the (node, index) order of several sides in ONE launch, one workgroup per side (the same network): side u sorts n keypoints by
// (node id, index), node < 0 behind every bucket, node == null = identity; sides beyond SV_SORT_SMALL_MAX are skipped (the caller sorts them)
struct SvSortSide {
    const int32_t* node;
    int n;
    unsigned* keys_out;
    int* idx_out;
};
bool sv_sort_small_sides(hipStream_t s, const SvSortSide* sides_dev, int count, int max_n);  // false: not available on this device
