// Internal declarations shared by the svgpu translation units (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "svgpu.h"
#include "sv_arena.h"
#include "orb_plan.h"  // ORB constants, OrbLevel / FastCell / DescBand / OrbConfig, the host planner
#include "frame_layout.h"
#include "ba_plan.h"  // BaEnv

// Optional per-kernel timing with HIP events on the launch stream (svgpu_profile_select / _read / _read_class).
// One accumulator per kernel class; the selection "*" brackets EVERY class, so that one timed region yields the mean launch time of
// each kernel as it runs inside the caller's pipeline (bench.py: roofline.kernels[] comes from the timed region itself).
struct SvProfClass {
    std::vector<hipEvent_t> ev;  // start/stop pairs
    size_t used = 0;
    double total_ms = 0;
    long long launches = 0;
};
struct SvProf {
    std::string name;  // kernel class being bracketed; "*" = all; empty = off
    std::map<std::string, SvProfClass> cls;
    unsigned long long* d_counter = nullptr;  // device word a profiled k_bf_mfma adds its multiplied 64 x 32 patches to
};

// A frame observation resident on the device (include/svgpu.h svgpu_frame_*): what every projection-family matcher reads of a
// data::frame / data::keyframe -- descriptors, undistorted keypoints split into the arrays the kernels take, stereo x_right, and the
// keypoint grid of data::assign_keypoints_to_grid as CSR.  Plain device allocations (grow-only), usable from any context of the device.
struct svgpu_frame : FrameSlab {
    int device = 0;
    int n = 0, cap = 0;
    int grid_cols = 0, grid_rows = 0, cells_cap = 0;
    float min_x = 0, max_x = 0, min_y = 0, max_y = 0;  // image bounds the grid was binned over
    bool has_xright = false;
    // ONE device allocation (`slab`, `slab_bytes`) holds the pieces of FrameSlab, carved by frame_slab_layout (frame_layout.h): the
    // observation first, so that what the host wants back of a freshly extracted frame is one contiguous copy (svgpu_track_motion)
    char* slab = nullptr;
    size_t slab_bytes = 0;
    int32_t* cell_off = nullptr;        // grid_cols * grid_rows + 1 (own allocation: sized by the grid)
    int32_t* dummy = nullptr;           // 1 int (the query-side scan of a grid build without queries)
};

// The landmark table of the tracked-frame chain (include/svgpu.h svgpu_map_*): records indexed by data::landmark::id_.
// Writers (upsert / erase: the mapping thread after BA, the tracking thread's flush) and readers (the tracker's chains) may sit on
// different contexts = streams: `mtx` serialises the host side, ev_write / the pending read events order the streams (a reader's stream
// waits for the last write, a writer's for EVERY read since the previous writer), and a growth waits for both before the old table is freed.
struct svgpu_map {
    int device = 0;
    int cap = 0;                         // records allocated (ids < cap are addressable)
    svgpu_landmark_record* rec = nullptr;
    std::mutex mtx;
    hipEvent_t ev_write = nullptr;
    bool wrote = false;
    // one event PER READ that no writer has waited for yet: readers run on any number of streams (two trackers of a stereo rig, a
    // relocaliser beside the tracker, svgpu_map_download on another context), and a writer -- above all a growth, which frees the old
    // allocation -- has to wait for every one of them, not for whichever recorded last
    std::vector<hipEvent_t> reads_pending, reads_pool;
};
int sv_map_reader_begin(svgpu_ctx* ctx, svgpu_map* map, hipStream_t s);  // the reader's stream waits for the last write (call with map->mtx held)
int sv_map_reader_end(svgpu_ctx* ctx, svgpu_map* map, hipStream_t s);    // records this read for the next writer (mutex still held)
// Scope of a read of the table on stream s (constructed with map->mtx held, destroyed before it is released): whatever path leaves the
// scope -- every SV_HIP early return included -- the read is recorded for the writers; a path that did not reach end() also drains the stream,
// so nothing it enqueued still reads the table when the caller sees the error.
struct SvMapReadScope {
    svgpu_ctx* ctx;
    svgpu_map* map;
    hipStream_t s;
    bool open = false;
    SvMapReadScope(svgpu_ctx* c, svgpu_map* m, hipStream_t st) : ctx(c), map(m), s(st) {}
    int begin() {
        const int rc = sv_map_reader_begin(ctx, map, s);
        open = rc == 0;
        return rc;
    }
    int end() {
        open = false;
        return sv_map_reader_end(ctx, map, s);
    }
    ~SvMapReadScope() {
        if (open) {
            (void)sv_map_reader_end(ctx, map, s);
            (void)hipStreamSynchronize(s);
        }
    }
    SvMapReadScope(const SvMapReadScope&) = delete;
    SvMapReadScope& operator=(const SvMapReadScope&) = delete;
};

// Image ingest of one camera (include/svgpu.h svgpu_ingest_*): the raw frame format and, for a rectified camera, the compiled map.
struct svgpu_ingest {
    int device = 0;
    int width = 0, height = 0, channels = 0, color_order = 0;
    uint2* d_map = nullptr;  // height x map_pitch compiled entries (ingest_kernels.h); null: no rectification
    int map_pitch = 0;
};

struct svgpu_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream_aux = nullptr;  // blur of a batch runs here beside FAST + selection on `stream`
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_stage[2] = {nullptr, nullptr};  // recorded inside svgpu_orb_extract_batch_device: [0] before k_fast, [1] before k_describe (svgpu_orb_stream_wait_stage)
    bool stage_recorded = false;
    std::string last_error;
    SvProf prof;
    OrbConfig orb;
    // device resources of the ORB path
    OrbLevel* d_levels = nullptr;
    FastCell* d_cells = nullptr;
    short* d_xofs = nullptr;        // per level >= 1: source column
    short2* d_xa = nullptr;         // (a0, a1) 11-bit coefficients
    short2* d_yofs = nullptr;       // (row0, row1) clamped
    short2* d_yb = nullptr;         // (b0, b1)
    uint32_t* d_xg = nullptr;       // k_pyramid_lds: 8 words per group of 4 output columns (orb_plan.h orb_plan_pyramid_records)
    short4* d_yrow = nullptr;       // k_pyramid_lds: (row0, row1, b0, b1) per output row
    int2* d_band_rows = nullptr;    // [bands][levels]: rows of each level a pyramid band computes
    unsigned short* d_gtab = nullptr;
    uint8_t* d_pyr = nullptr;       // max_batch * pyr_frame_bytes
    uint8_t* d_blur = nullptr;      // max_batch * blur_frame_bytes
    unsigned long long* d_keys = nullptr;  // max_batch * total_grid
    int4* d_sel = nullptr;          // max_batch * total_grid  (x, y, level, response)
    int32_t* d_cellpos = nullptr;   // max_batch * (total_grid + 1): emission position of every selection-grid cell
    DescBand* d_dbands = nullptr;
    // staging for the host-buffer entry points
    uint8_t* d_img = nullptr;
    uint8_t* d_mask = nullptr;
    svgpu_keypoint* d_kps = nullptr;
    uint8_t* d_desc = nullptr;
    int32_t* d_counts = nullptr;
    int last_batch = 0;
    int last_extract_n = -1;             // keypoints of the last svgpu_orb_extract, still in d_kps / d_desc (svgpu_frame_adopt_extraction)
    const svgpu_frame* bound_frame = nullptr;  // svgpu_frame_bind: keypoint side of the NEXT matcher call (one-shot)
    size_t cand_cap_hint = 0;                  // cell matchers: candidate-list capacity that sufficed last time (0: unknown -> exact two-pass sizing)
    const uint8_t* next_q_blocks = nullptr;    // svgpu_match_set_query_blocks: per-query "an accepted match occupies its target" of the NEXT svgpu_match_in_cells
    const uint8_t* last_imgs = nullptr;  // level-0 of the last call (device)
    size_t last_frame_stride = 0;
    int last_row_stride = 0;
    // generic scratch (matchers, BA)
    void* d_scratch = nullptr;
    double* h_pinned = nullptr;     // page-locked read-back buffer of the BA loops (small per-trial partial sums)
    size_t pinned_doubles = 0;
    char* h_stage = nullptr;        // page-locked mirror of d_scratch (StagedCall, sv_staged_call.h; BA's own images): inputs are written here in device layout, one copy each way
    size_t stage_bytes = 0;
    size_t scratch_bytes = 0;
    // bundle adjustment
    hipStream_t ba_copy_stream = nullptr;  // second stream of a global-BA sized call: the measurements' upload runs beside the structure kernels
    hipEvent_t ev_ba_copy = nullptr;
    hipEvent_t ev_ba = nullptr;     // completion event the BA host loop polls (while mirroring the caller's stop flag)
    int ba_solver = 0;              // svgpu_ba_solver
    double pcg_tol = 1e-10;         // relative residual of the reduced-system PCG
    int pcg_max_it = 0;             // 0 = max(2000, 4 n)
    void* comm = nullptr;           // ncclComm_t of svgpu_comm_init (RCCL, loaded with dlopen)
    void* ba_sky = nullptr;         // plan + buffers of the envelope Cholesky (ba_skyline.hip)
    svgpu_allreduce_fn ba_ar_fn = nullptr;  // the all-reduce of the sharded solve in progress (the segmented envelope solve exchanges through it); else null
    void* ba_ar_user = nullptr;
    BaEnv ba_env;                   // the switches of the bundle-adjustment call in progress (ba_plan.h; local_ba_impl reads them at its entry)
    int ba_last_solver = -1;        // svgpu_ba_last_solver: the solver the last stage's structure resolved to (ba_plan_solver_final)
    long long ba_xch[10] = {0};    // svgpu_ba_last_exchange: what the last sharded solve all-reduced (mode | bytes by category | calls | trials | linearisations)
    int comm_rank = 0, comm_world = 1;
};
void sv_comm_release(svgpu_ctx* ctx);

int sv_set_error(svgpu_ctx* ctx, int status, const char* what, hipError_t e = hipSuccess);
void sv_prof_begin(svgpu_ctx* ctx, hipStream_t s, const char* name);
void sv_prof_end(svgpu_ctx* ctx, hipStream_t s, const char* name);
unsigned long long* sv_prof_counter(svgpu_ctx* ctx, const char* name);  // the device counter when `name` is being profiled, else null
struct SvProfScope {  // brackets the launches issued inside its lifetime when `name` is the selected kernel class
    svgpu_ctx* c;
    hipStream_t s;
    const char* n;
    SvProfScope(svgpu_ctx* ctx, hipStream_t st, const char* name) : c(ctx), s(st), n(name) {
        if (!c->prof.name.empty()) sv_prof_begin(c, s, n);
    }
    ~SvProfScope() {
        if (!c->prof.name.empty()) sv_prof_end(c, s, n);
    }
};
int sv_ensure_scratch(svgpu_ctx* ctx, size_t bytes);
void sv_sky_release(svgpu_ctx* ctx);  // plan + buffers of the envelope Cholesky (ba_skyline.hip)
int sv_ensure_stage(svgpu_ctx* ctx, size_t bytes);  // grow-only page-locked host buffer (ctx->h_stage)
// the plain scratch user: measure the layout, grow ctx->d_scratch to it, place it there (`overflow_msg`: the error text of a failed placement)
template <class Layout>
int sv_scratch_layout(svgpu_ctx* ctx, const char* overflow_msg, Layout&& layout) {
    const int rc = sv_ensure_scratch(ctx, arena_measure(layout));
    if (rc) return rc;
    Arena A(ctx->d_scratch, ctx->scratch_bytes);
    layout(A);
    return A.overflow ? sv_set_error(ctx, SVGPU_ERR_INVALID, overflow_msg) : SVGPU_OK;
}
hipError_t sv_allow_dynamic_lds(const void* kernel, size_t bytes);  // per (device, kernel), thread-safe
void sv_orb_release(svgpu_ctx* ctx);
int sv_frame_reserve(svgpu_ctx* ctx, svgpu_frame* f, int n, int ncell);  // grow-only slab of a resident frame (svgpu_frame.hip)

#define SV_HIP(ctx, call)                                                   \
    do {                                                                    \
        hipError_t _e = (call);                                             \
        if (_e != hipSuccess) return sv_set_error((ctx), SVGPU_ERR_HIP, #call, _e); \
    } while (0)

// ---- kernel launchers (orb_kernels.hip)
// The images of one extract call, as every ORB kernel takes them: the launchers expand it into the kernels' parameter lists.
struct OrbFrames {
    const OrbLevel* levels;
    int num_levels;
    const uint8_t* img0;  // level 0: the caller's frames
    size_t img0_frame_stride;
    int img0_pitch;
    uint8_t* pyr;         // levels >= 1
    size_t pyr_frame_bytes;
    uint8_t* blur;        // blurred copy of every level
    size_t blur_frame_bytes;
    int batch;
};
hipError_t sv_pyramid_prepare();
void sv_launch_pyramid(hipStream_t s, const OrbFrames& F, const OrbLaunch& plan, const int2* band_rows, int bands, size_t lds_bytes, const short* xofs,
                       const short2* xa, const short2* yofs, const short2* yb, const uint32_t* xg, const short4* yrow);
void sv_launch_blur(hipStream_t s, const OrbFrames& F, const OrbLaunch& plan, int total_tiles, int total_bands);
void sv_launch_fast(hipStream_t s, const OrbFrames& F, int cpw, const FastCell* cells, int num_cells, const unsigned short* gtab,
                    unsigned long long* keys, int total_grid, int ini_thr, int min_thr, const uint8_t* mask, size_t mask_frame_stride,
                    int mask_pitch, int mask_w, int mask_h);
void sv_launch_select(hipStream_t s, const OrbFrames& F, unsigned long long* keys, int total_grid, int4* sel, int32_t* counts, int32_t* cellpos);
hipError_t sv_describe_bands_prepare(size_t lds_bytes);
void sv_launch_describe_bands(hipStream_t s, const OrbFrames& F, const DescBand* bands, int num_bands, size_t lds_bytes, const int4* sel,
                              int total_grid, const int32_t* cellpos, const int32_t* counts, svgpu_keypoint* kps, uint8_t* desc, int cap,
                              float* angles);
void sv_launch_describe(hipStream_t s, const OrbFrames& F, const int4* sel, int total_grid, const int32_t* counts, svgpu_keypoint* kps,
                        uint8_t* desc, int cap, float* angles);
