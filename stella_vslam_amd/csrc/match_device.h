// Device functions shared by match_kernels.hip and track_kernels.hip (the tracked-frame chain runs the same steps fused).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_kernels.h"
#include "sv_wave.h"

namespace svmd {

constexpr unsigned HAMMING_DIST_THR_LOW = 50;   // match/base.h:15
constexpr unsigned MAX_HAMMING_DIST = 256;      // match/base.h:17

__device__ __forceinline__ unsigned hamming256(const uint32_t (&a)[8], const uint32_t* __restrict__ b) {
    unsigned d = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) d += __popc(a[i] ^ b[i]);
    return d;
}

__device__ __forceinline__ float angle_diff(float a1, float a2) {  // util/angle.cc:7-16
    float ret = a1 - a2;
    if (ret <= -180.0f) ret += 360.0f;
    if (ret > 180.0f) ret -= 360.0f;
    return ret;
}

#define GRID_ONE_CELLS 4096
#define GRID_ONE_KPT_ROUNDS 8  // keypoints per thread whose arrival numbers stay in registers (8 192 keypoints)
#define GRID_ONE_SMALL 24      // a cell of at most this many keypoints is ordered by one thread (insertion sort); a larger one by the workgroup
// (body of k_grid_frame_one; `nt` = the number of keypoints, which the fused tracked-frame kernel reads from device memory)
__device__ __forceinline__ void grid_frame_one(const GridProblem& G, const int nt) {
    __shared__ int s_cnt[GRID_ONE_CELLS + 1];
    __shared__ int s_wsum[16];
    __shared__ int s_items[1024 * GRID_ONE_KPT_ROUNDS];  // the items of one crowded cell
    __shared__ int s_big[1024 * GRID_ONE_KPT_ROUNDS / GRID_ONE_SMALL + 1], s_nbig;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nc = G.cols * G.rows;
    for (int c = tid; c <= nc; c += 1024) s_cnt[c] = 0;
    if (tid == 0) s_nbig = 0;
    __syncthreads();
    int cell[GRID_ONE_KPT_ROUNDS], pos[GRID_ONE_KPT_ROUNDS];
#pragma unroll
    for (int r = 0; r < GRID_ONE_KPT_ROUNDS; ++r) {
        const int i = tid + r * 1024;
        cell[r] = -1, pos[r] = 0;
        if (i < nt) {
            const int cx = (int)floor((double)(G.t_xy[2 * i] - G.min_x) * G.inv_w), cy = (int)floor((double)(G.t_xy[2 * i + 1] - G.min_y) * G.inv_h);
            if (0 <= cx && cx < G.cols && 0 <= cy && cy < G.rows) {
                cell[r] = cx * G.rows + cy;
                pos[r] = atomicAdd(&s_cnt[cell[r]], 1);  // arrival order inside the cell: arbitrary, put right at the end
            }
            G.cell_of[i] = cell[r];
        }
    }
    __syncthreads();
    // exclusive scan of the counters: every thread owns a contiguous run of cells, wave scan of the run sums, then the waves' totals
    const int per = (nc + 1023) / 1024, c0 = tid * per, c1 = min(c0 + per, nc);
    int run = 0;
    for (int c = c0; c < c1; ++c) run += s_cnt[c];
    int incl = run;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int base = incl - run;
    for (int w = 0; w < wave; ++w) base += s_wsum[w];
    __syncthreads();
    for (int c = c0; c < c1; ++c) {  // counters -> offsets, in place (a thread's own run only)
        const int k = s_cnt[c];
        s_cnt[c] = base;
        base += k;
    }
    if (tid == 1023) s_cnt[nc] = base;  // (the last thread's run ends at nc or is empty: its base is the total either way)
    __syncthreads();
    for (int c = tid; c <= nc; c += 1024) G.cell_off[c] = s_cnt[c];
#pragma unroll
    for (int r = 0; r < GRID_ONE_KPT_ROUNDS; ++r)
        if (cell[r] >= 0) G.cell_items[s_cnt[cell[r]] + pos[r]] = tid + r * 1024;
    __syncthreads();  // (workgroup-scope: the placements above are visible to the threads below)
    for (int c = tid; c < nc; c += 1024) {  // increasing keypoint index inside every cell (= the stable placement)
        const int lo = s_cnt[c], k = s_cnt[c + 1] - lo;
        if (k > GRID_ONE_SMALL) {  // crowded: left to the whole workgroup below (at most nt / GRID_ONE_SMALL such cells)
            s_big[atomicAdd(&s_nbig, 1)] = c;
            continue;
        }
        for (int a = 1; a < k; ++a) {  // insertion sort: cells hold a handful of keypoints
            const int v = G.cell_items[lo + a];
            int b = a - 1;
            while (b >= 0 && G.cell_items[lo + b] > v) {
                G.cell_items[lo + b + 1] = G.cell_items[lo + b];
                --b;
            }
            G.cell_items[lo + b + 1] = v;
        }
    }
    __syncthreads();
    // crowded cells (a dense patch under a coarse grid; in the limit every keypoint in one cell): rank sort by the workgroup -- the cell's
    // items staged in LDS, every thread counts the items below its own: k^2 / 1 024 LDS reads per thread, 16 k at the 8 192-keypoint limit
    // (one thread's insertion sort would be k^2 / 4 global round trips)
    const int nbig = s_nbig;
    for (int bi = 0; bi < nbig; ++bi) {
        const int c = s_big[bi], lo = s_cnt[c], k = s_cnt[c + 1] - lo;
        for (int a = tid; a < k; a += 1024) s_items[a] = G.cell_items[lo + a];
        __syncthreads();
        for (int a = tid; a < k; a += 1024) {
            const int v = s_items[a];
            int rank = 0;
            for (int j = 0; j < k; ++j) rank += s_items[j] < v;  // (indices are distinct)
            G.cell_items[lo + rank] = v;
        }
        __syncthreads();
    }
}

// ---- the grid lists of larger frames and of several keypoint sets at once: the bodies behind k_grid_assign / k_grid_place / k_grid_walk
// and their _batch forms (match_kernels.hip).  data::assign_keypoints_to_grid (data/common.cc:83-108) and data::get_keypoints_in_cell
// (:127-190): cells are x-major (col * rows + row), a cell lists its keypoints in index order, a query scans cells col-major inside its
// window and keeps keypoints of the wanted levels strictly inside the margin square -- the reference's candidate ORDER, which decides
// ties downstream.

// the cell of keypoint i is counted (counts in cell_off; scanned in place afterwards) and noted as id_base + cell, -1 outside the grid;
// id_base = 0 for one set, the set's first counter among all sets' for a batch
__device__ __forceinline__ void grid_assign_one(const GridProblem& G, const int i, const int id_base) {
    const int cx = (int)floor((double)(G.t_xy[2 * i] - G.min_x) * G.inv_w), cy = (int)floor((double)(G.t_xy[2 * i + 1] - G.min_y) * G.inv_h);
    int c = -1;
    if (0 <= cx && cx < G.cols && 0 <= cy && cy < G.rows) {
        c = cx * G.rows + cy;
        atomicAdd(&G.cell_off[c], 1);
        c += id_base;
    }
    G.cell_of[i] = c;
}
// stable placement: the rank of keypoint i inside its cell = the number of keypoints in [first, i) with the same cell id `c`; the ids
// stream through LDS tiles (whole workgroup of 256; n = the length of cell_of)
__device__ __forceinline__ int grid_rank_in_cell(const int32_t* __restrict__ cell_of, const int n, const int first, const int i, const int c) {
    __shared__ int s_cell[1024];
    const int last = min((int)blockIdx.x * 256 + 255, n - 1);  // tiles beyond the block's last keypoint hold no earlier keypoint
    int rank = 0;
    for (int base = first; base <= last; base += 1024) {
        __syncthreads();
        for (int k = threadIdx.x; k < 1024; k += 256) s_cell[k] = base + k < n ? cell_of[base + k] : -2;
        __syncthreads();
        const int m = min(1024, i - base);  // earlier keypoints only
        for (int k = 0; k < m; ++k) rank += s_cell[k] == c;
    }
    return rank;
}
// one wave per query q of G: the lanes take the cells of the window (column-major = the reference's scan order), count their keypoints
// that pass the level and margin tests, and a wave prefix sum gives every cell its place in the query's list.  FILL = false leaves the
// list's size in cand_off[q]; FILL = true writes the list behind cand_idx + cand_off[q]
template <bool FILL>
__device__ __forceinline__ void grid_walk_one(const GridProblem& G, const int q, const int lane) {
    int total = 0;
    const bool live = !G.q_valid || G.q_valid[q];
    if (live) {
        const float ref_x = G.q_xy[2 * q], ref_y = G.q_xy[2 * q + 1], margin = G.q_margin[q];
        const int min_level = G.q_min_level ? G.q_min_level[q] : -1, max_level = G.q_max_level ? G.q_max_level[q] : -1;
        int lo_x = (int)floor((double)(ref_x - G.min_x - margin) * G.inv_w), hi_x = (int)ceil((double)(ref_x - G.min_x + margin) * G.inv_w);
        int lo_y = (int)floor((double)(ref_y - G.min_y - margin) * G.inv_h), hi_y = (int)ceil((double)(ref_y - G.min_y + margin) * G.inv_h);
        lo_x = max(lo_x, 0);
        lo_y = max(lo_y, 0);
        hi_x = min(hi_x, G.cols - 1);
        hi_y = min(hi_y, G.rows - 1);
        if (lo_x < G.cols && 0 <= hi_x && lo_y < G.rows && 0 <= hi_y && lo_x <= hi_x && lo_y <= hi_y) {
            const int ny = hi_y - lo_y + 1, ncell = (hi_x - lo_x + 1) * ny;
            int32_t* out = FILL ? G.cand_idx + G.cand_off[q] : nullptr;
            for (int base = 0; base < ncell; base += 64) {
                const int k = base + lane;
                int n = 0, c = 0;
                if (k < ncell) {
                    c = (lo_x + k / ny) * G.rows + lo_y + k % ny;
                    for (int it = G.cell_off[c]; it < G.cell_off[c + 1]; ++it) {
                        const int idx = G.cell_items[it];
                        const int oct = G.t_octave[idx];
                        if (0 <= min_level && oct < min_level) continue;
                        if (0 <= max_level && max_level < oct) continue;
                        const float dx = G.t_xy[2 * idx] - ref_x, dy = G.t_xy[2 * idx + 1] - ref_y;
                        if (fabsf(dx) < margin && fabsf(dy) < margin) ++n;
                    }
                }
                const int incl = sv_wave_inclusive_sum(n);
                if (FILL && n > 0) {
                    int o = total + incl - n;
                    for (int it = G.cell_off[c]; it < G.cell_off[c + 1]; ++it) {
                        const int idx = G.cell_items[it];
                        const int oct = G.t_octave[idx];
                        if (0 <= min_level && oct < min_level) continue;
                        if (0 <= max_level && max_level < oct) continue;
                        const float dx = G.t_xy[2 * idx] - ref_x, dy = G.t_xy[2 * idx + 1] - ref_y;
                        if (fabsf(dx) < margin && fabsf(dy) < margin) out[o++] = idx;
                    }
                }
                total += __builtin_amdgcn_readlane(incl, 63);
            }
        }
    }
    if (!FILL && lane == 0) G.cand_off[q] = total;
}

}  // namespace svmd
