/*
 * svgpu.h -- C ABI of the MI355X-native stella_vslam hot path (ORB front end, Hamming matchers,
 * local bundle adjustment).  Plain pointers and sizes only; no C++/torch/OpenCV types.
 *
 * The reference (stella-cv/stella_vslam v0.6.0) has no FFI layer: its boundary for this path is three
 * C++ class surfaces.  Every entry point below names the reference interface it stands behind; the
 * C++ adaptor classes in stella_vslam_amd/host/ (same names and signatures as the reference classes)
 * flatten the object graph, call this ABI and write the results back.  INTEGRATION.md shows the
 * binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - every function returns an svgpu_status (0 = OK); nothing throws, nothing aborts
 *   - "host" pointers are ordinary CPU memory; "dev" pointers are HIP device memory on the context's GPU
 *   - `stream` arguments are a hipStream_t passed as void* (NULL = the context's own stream)
 *   - one svgpu_ctx per (device, caller thread): two extractor instances (stereo: system.cc:427-434)
 *     use two contexts and run concurrently
 *   - all device entry points are asynchronous on their stream unless stated otherwise
 *   - a context owns ONE set of scratch buffers (pyramid, score maps, candidate lists, BA arenas), reused by every call without a
 *     fence of its own: all calls on one context must be ordered on ONE stream at a time (the context's, or one caller stream).
 *     To move a context to another stream, synchronise the old one first; for concurrent streams use one context per stream
 *     (bench.py: an extraction context and a matching context, ordered by events on the buffers they hand over)
 */
#ifndef SVGPU_H
#define SVGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVGPU_ABI_VERSION 1

typedef enum svgpu_status {
    SVGPU_OK = 0,
    SVGPU_ERR_INVALID = 1,     /* bad argument */
    SVGPU_ERR_HIP = 2,         /* a HIP runtime call failed; svgpu_last_error() has the text */
    SVGPU_ERR_CAPACITY = 3,    /* an output did not fit; counts are still the true totals */
    SVGPU_ERR_NOT_CONFIGURED = 4,
    SVGPU_ERR_NO_DEVICE = 5,
    SVGPU_ERR_NUMERIC = 6,     /* e.g. reduced camera system not positive definite at every damping */
    SVGPU_STOPPED = 7          /* the caller's stop flag was set before any work was done */
} svgpu_status;

typedef struct svgpu_ctx svgpu_ctx;

/* cv::KeyPoint layout (28 bytes): pt.x pt.y size angle response octave class_id */
typedef struct svgpu_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} svgpu_keypoint;

/* ------------------------------------------------------------------------------------------------ core */
int svgpu_abi_version(void);
int svgpu_device_count(void);
int svgpu_create(int device, svgpu_ctx** out);
/* Same with a stream priority hint: > 0 highest, < 0 lowest, 0 default.  A pipeline that runs extraction and matching of
 * consecutive batches on two streams gives the longer leg (extraction) the higher priority (bench.py). */
int svgpu_create_with_priority(int device, int priority, svgpu_ctx** out);
void svgpu_destroy(svgpu_ctx* ctx);
const char* svgpu_last_error(const svgpu_ctx* ctx);
const char* svgpu_status_string(int status);
int svgpu_synchronize(svgpu_ctx* ctx);
void* svgpu_stream(svgpu_ctx* ctx); /* the context's hipStream_t */

/* Per-kernel timing with HIP events recorded on the launch stream (measurement aid for bench.py's roofline
 * object).  svgpu_profile_select brackets every later launch of the named kernel class (NULL = off, "*" = every class: one timed
 * region then yields each kernel's mean launch time as it runs inside the caller's pipeline);
 * svgpu_profile_read synchronises and returns the accumulated device time and the number of launches of the selected class,
 * svgpu_profile_read_class the same for a named class (the way to read a "*" selection). */
const char* svgpu_profile_kernels(void); /* comma-separated class names */
int svgpu_profile_select(svgpu_ctx* ctx, const char* kernel_name);
int svgpu_profile_read(svgpu_ctx* ctx, double* total_ms, long long* launches);
int svgpu_profile_read_class(svgpu_ctx* ctx, const char* kernel_name, double* total_ms, long long* launches);
/* int8 multiply-add operations the matrix cores executed in the profiled launches of the brute-force distance kernel since the
 * last svgpu_profile_select (counted by the kernel itself: 2 x 64 x 32 x 256 per multiplied patch); 0 when it was not profiled */
int svgpu_profile_mfma_ops(svgpu_ctx* ctx, unsigned long long* int8_ops);

/* ------------------------------------------------------------------------------------------------ ORB front end
 * Stands behind  stella_vslam::feature::orb_extractor  (feature/orb_extractor.h:46-71):
 *   orb_extractor(const orb_params*, unsigned min_area, descriptor_type, mask_rects)   -> svgpu_orb_configure
 *   void extract(in_image, in_image_mask, std::vector<cv::KeyPoint>&, out_descriptors) -> svgpu_orb_extract
 *   public member image_pyramid_ (read by match::stereo, match/stereo.cc:20-114)       -> svgpu_orb_pyramid_download
 * and behind orb_params' scale tables (feature/orb_params.cc:41-71)                    -> svgpu_orb_scale_tables
 */

/* orb_params::calc_* : four tables of num_levels floats, computed by the reference's fp32 recurrences. */
int svgpu_orb_scale_tables(float scale_factor, int num_levels, float* scale_factors, float* inv_scale_factors,
                           float* level_sigma_sq, float* inv_level_sigma_sq);

/* Fix the image geometry and ORB parameters; (re)allocates device workspaces for up to max_batch frames
 * per launch.  min_area is the constructor argument (system.cc:95 default 800); its integer square
 * root is taken as in orb_extractor.cc:20. */
int svgpu_orb_configure(svgpu_ctx* ctx, int width, int height, int max_batch, float scale_factor, int num_levels,
                        int ini_fast_thr, int min_fast_thr, unsigned min_area);

/* Pipeline scheduling aid for callers that run other work beside a batch extraction on a second stream: `stream` waits until the LAST
 * svgpu_orb_extract_batch_device enqueued on `ctx` has reached a stage -- 0: pyramid and blur done, FAST about to start; 1: FAST and the
 * selection done, the descriptor kernel about to start.  bench.py holds the matcher of batch t back until the extraction of batch t+1 is
 * at its descriptor kernel: that kernel waits on patch fetches and leaves issue slots to the matcher, the pyramid does not.
 * No extraction enqueued yet: returns at once. */
int svgpu_orb_stream_wait_stage(svgpu_ctx* ctx, int stage, void* stream);

/* Upper bound on keypoints per frame for the configured geometry (= number of selection-grid cells). */
int svgpu_orb_max_keypoints(const svgpu_ctx* ctx);
/* Level geometry of the configured pyramid. */
int svgpu_orb_level_size(const svgpu_ctx* ctx, int level, int* width, int* height);

/* extract(): one frame, host in / host out, synchronous.
 *   img        8UC1, `stride` bytes per row, configured width x height
 *   mask       nullable 8UC1 of the same size (0 = masked), mask_stride bytes per row
 *   kps/desc   caller-owned, room for `cap` keypoints / cap*32 bytes
 *   n_out      number of keypoints (true total even when > cap -> SVGPU_ERR_CAPACITY)
 *   level_counts  nullable, num_levels ints
 * Output order = the reference's: level-major, selection-grid cell order within a level. */
int svgpu_orb_extract(svgpu_ctx* ctx, const uint8_t* img, int stride, const uint8_t* mask, int mask_stride,
                      svgpu_keypoint* kps, uint8_t* desc, int cap, int* n_out, int* level_counts);

/* Throughput path: `batch` frames already resident in HBM, results left in HBM, asynchronous.
 *   imgs_dev       batch frames, frame b at imgs_dev + b*frame_stride, rows `row_stride` bytes apart
 *   mask_dev       nullable; mask_frame_stride 0 = one mask shared by all frames
 *   kps_dev        batch * cap records;  desc_dev  batch * cap * 32 bytes
 *   counts_dev     batch * (1 + num_levels) int32: [total, per-level...]; total may exceed cap (then
 *                  only the first cap keypoints were written) */
int svgpu_orb_extract_batch_device(svgpu_ctx* ctx, const uint8_t* imgs_dev, int batch, size_t frame_stride,
                                   int row_stride, const uint8_t* mask_dev, size_t mask_frame_stride,
                                   int mask_row_stride, svgpu_keypoint* kps_dev, uint8_t* desc_dev, int cap,
                                   int32_t* counts_dev, void* stream);

/* The same, and the keypoint angles once more as a packed float array (batch * cap; nullable): what the angle-bin sort of the batched
 * matcher wants to read -- 4 bytes per keypoint instead of walking the 28-byte records (svgpu_match_consecutive_batch_device_angles). */
int svgpu_orb_extract_batch_device_angles(svgpu_ctx* ctx, const uint8_t* imgs_dev, int batch, size_t frame_stride,
                                          int row_stride, const uint8_t* mask_dev, size_t mask_frame_stride,
                                          int mask_row_stride, svgpu_keypoint* kps_dev, uint8_t* desc_dev, int cap,
                                          int32_t* counts_dev, float* angles_dev, void* stream);

/* image_pyramid_[level] of frame `frame` of the last extract call, copied to host (level 0 is the
 * caller's own image and is not stored).  Synchronous. */
int svgpu_orb_pyramid_download(svgpu_ctx* ctx, int frame, int level, uint8_t* dst, int dst_stride);
/* Gaussian-blurred level (the image descriptors are sampled from); debugging / tests. */
int svgpu_orb_blurred_download(svgpu_ctx* ctx, int frame, int level, uint8_t* dst, int dst_stride);

/* ------------------------------------------------------------------------------------------------ matchers
 * Stand behind  stella_vslam::match::*  (match/base.h:15-91 and the six matcher classes).
 * The reference walks frame/keyframe/landmark objects; the adaptors flatten them to descriptor rows
 * (N x 32 bytes), angles, octaves and CSR candidate lists in the reference's scan order.
 * Every matcher resolves the reference's SEQUENTIAL greedy bookkeeping exactly (same result as the
 * serial loops), see DESIGN.md "greedy replay".
 */

/* compute_descriptor_distance_32 (match/base.h:20-41) for n pairs of 32-byte rows; host in/out, synchronous. */
int svgpu_hamming_distance(svgpu_ctx* ctx, const uint8_t* a, const uint8_t* b, int n, uint32_t* dist);

/* Full n2 x n1 distance matrix (uint16) -- building block / diagnostics; host in/out, synchronous. */
int svgpu_hamming_matrix(svgpu_ctx* ctx, const uint8_t* desc1, int n1, const uint8_t* desc2, int n2, uint16_t* out);

/* robust::brute_force_match (match/robust.cc:232-328).
 *   index 1 = frame side (scanned, claimed once), index 2 = keyframe side (outer loop in index order)
 *   valid2      nullable; 0 = keyframe keypoint without a live landmark (skipped, :258-263)
 *   matched_2_in_1[n1]  keyframe index matched to each frame keypoint or -1; returns count in *num_matches
 * Host in/out, synchronous. */
int svgpu_match_bruteforce(svgpu_ctx* ctx, const uint8_t* desc1, const float* angle1, int n1, const uint8_t* desc2,
                           const float* angle2, const uint8_t* valid2, int n2, float lowe_ratio,
                           int check_orientation, int32_t* matched_2_in_1, int* num_matches);

/* Batched, device-resident brute force: `pairs` independent (frame, keyframe) problems.
 *   desc1_dev   pairs * cap1 * 32 bytes, angle via the keypoint records (kps1_dev, pairs*cap1) written by
 *               svgpu_orb_extract_batch_device; n1_dev[p*n_stride] = count of pair p; likewise side 2
 *   valid2_dev  nullable (pairs * cap2)
 *   matched_dev pairs * cap1 int32;  num_dev pairs int32
 * Asynchronous on `stream`. */
int svgpu_match_bruteforce_batch_device(svgpu_ctx* ctx, int pairs, const uint8_t* desc1_dev,
                                        const svgpu_keypoint* kps1_dev, const int32_t* n1_dev, int cap1,
                                        const uint8_t* desc2_dev, const svgpu_keypoint* kps2_dev,
                                        const int32_t* n2_dev, int cap2, int n_stride, const uint8_t* valid2_dev,
                                        float lowe_ratio, int check_orientation, int32_t* matched_dev,
                                        int32_t* num_dev, void* stream);

/* The same matcher over a RING of `frames` extractor outputs that already sit in one device batch (the layout
 * svgpu_orb_extract_batch_device writes): pair t = robust::brute_force_match(frame (t + 1) % frames, keyframe = frame t),
 * t = 0 .. frames-1, without copying any slot.  matched_dev: frames x cap, row t indexed by the keypoints of frame (t+1) % frames. */
int svgpu_match_consecutive_batch_device(svgpu_ctx* ctx, int frames, const uint8_t* desc_dev, const svgpu_keypoint* kps_dev,
                                         const int32_t* n_dev, int cap, int n_stride, const uint8_t* valid_dev, float lowe_ratio,
                                         int check_orientation, int32_t* matched_dev, int32_t* num_dev, void* stream);

/* The same with the keypoint angles as the packed array svgpu_orb_extract_batch_device_angles wrote (kps_dev is still what the orientation
 * check of robust.cc:283-287 is defined on: the two hold the same values; angles_dev == NULL reads the records). */
int svgpu_match_consecutive_batch_device_angles(svgpu_ctx* ctx, int frames, const uint8_t* desc_dev, const svgpu_keypoint* kps_dev,
                                                const float* angles_dev, const int32_t* n_dev, int cap, int n_stride, const uint8_t* valid_dev,
                                                float lowe_ratio, int check_orientation, int32_t* matched_dev, int32_t* num_dev, void* stream);

typedef enum svgpu_match_mode {
    SVGPU_MATCH_BEST_ONLY = 0,        /* projection::match_current_and_last_frames (match/projection.cc:95-207) */
    SVGPU_MATCH_RATIO_SAME_OCTAVE = 1,/* projection::match_frame_and_landmarks     (match/projection.cc:13-93)  */
    SVGPU_MATCH_RATIO = 2,            /* bow_tree::match_frame_and_keyframe / match_keyframes (match/bow_tree.cc:169-366) */
    SVGPU_MATCH_TRIANGULATION = 3,    /* bow_tree / robust ::match_for_triangulation (match/bow_tree.cc:11-167, robust.cc:14-146) */
    SVGPU_MATCH_AREA = 4              /* area::match_in_consistent_area (match/area.cc:8-98): ratio test; a closer later query takes
                                         the target from its holder (occupied / stereo inputs are not used) */
} svgpu_match_mode;

/* Candidate-list matcher: query q scans targets cand_idx[cand_off[q] .. cand_off[q+1]) in order.
 *   cand_skip    nullable, one byte per CSR entry: non-zero drops that (query, target) pair -- gates the caller evaluated
 *                on its object graph (epipolar constraint base.h:67-79, chi-square reprojection gate fuse.cc:92-119,
 *                "keypoint already has a landmark" bow_tree.cc:72-76)
 *   q_valid      nullable, 0 = query skipped
 *   occupied     nullable nt, 1 = target already holds an observed landmark (projection.cc:52-55)
 *   q_angle/t_angle + check_orientation : |angle::diff| > 30 gate (projection.cc:179-181)
 *   q_xright/t_xright/q_xr_tol : nullable stereo gate (projection.cc:57-62)
 *   thr, lowe_ratio, mode : acceptance rule
 *   match_q[nq]  target index or -1.  Host in/out, synchronous. */
int svgpu_match_candidates(svgpu_ctx* ctx, const uint8_t* qdesc, int nq, const uint8_t* tdesc, const int32_t* t_octave,
                           int nt, const int32_t* cand_off, const int32_t* cand_idx, const uint8_t* cand_skip,
                           const uint8_t* q_valid, const uint8_t* occupied, const float* q_angle, const float* t_angle, int check_orientation,
                           const float* q_xright, const float* t_xright, const float* q_xr_tol, unsigned thr,
                           float lowe_ratio, int mode, int32_t* match_q, int* num_matches);

/* The same matcher with the candidate lists built ON THE DEVICE: data::assign_keypoints_to_grid (data/common.cc:83-108)
 * bins the target keypoints, and query q gets the result of
 *     get_keypoints_in_cell(q_xy[q], q_margin[q], q_min_level[q], q_max_level[q])            (data/common.cc:127-190)
 * in the reference's order (cells column-major inside the window, keypoints of a cell in index order, level bounds < 0 =
 * unbounded, strictly inside the margin square).  This is the loop that dominates projection::* / fuse on the CPU.
 *   t_xy          nt x 2 undistorted keypoint positions; t_octave nt
 *   grid          image bounds min_x max_x min_y max_y (camera::base img_bounds) and num_grid_cols / rows (default 64 x 48)
 *   everything else as svgpu_match_candidates (no cand_skip: pair gates that need the object graph use the CSR entry point). */
int svgpu_match_in_cells(svgpu_ctx* ctx, const uint8_t* qdesc, int nq, const float* q_xy, const float* q_margin,
                         const int32_t* q_min_level, const int32_t* q_max_level, const uint8_t* q_valid, const float* q_angle,
                         const float* q_xright, const float* q_xr_tol, const uint8_t* tdesc, const float* t_xy,
                         const int32_t* t_octave, int nt, const uint8_t* occupied, const float* t_angle, const float* t_xright,
                         float min_x, float max_x, float min_y, float max_y, int grid_cols, int grid_rows,
                         int check_orientation, unsigned thr, float lowe_ratio, int mode, int32_t* match_q, int* num_matches);

/* ------------------------------------------------------------------------------ frame observation / reprojection
 * The host steps either side of extract and match, on the device so that a tracked frame
 * goes extractor -> undistort -> bearings -> grid -> landmark reprojection -> cell matcher without per-query host work. */
typedef enum svgpu_camera_model { /* camera/base.h:24-29 model_type_t, same values */
    SVGPU_CAM_PERSPECTIVE = 0,
    SVGPU_CAM_FISHEYE = 1,
    SVGPU_CAM_EQUIRECTANGULAR = 2,
    SVGPU_CAM_RADIAL_DIVISION = 3
} svgpu_camera_model;

/* camera::base + the model's parameters (camera/perspective.h:57-73, fisheye.h:51-67, radial_division.h:49-61,
 * equirectangular.h).  dist: perspective k1 k2 p1 p2 k3 | fisheye k1 k2 k3 k4 | radial_division distortion | unused.
 * min_x..max_y = img_bounds_ (camera/base.h image_bounds, floats); svgpu_camera_image_bounds fills them. */
typedef struct svgpu_camera {
    int32_t model;
    int32_t pad_;
    double cols, rows;
    double fx, fy, cx, cy;
    double dist[5];
    double focal_x_baseline;
    float min_x, max_x, min_y, max_y;
} svgpu_camera;

/* camera::*::compute_image_bounds (perspective.cc:70-96, fisheye.cc:68-134, radial_division.cc:57-81,
 * equirectangular.cc:32-36): undistorts the image corners on the device and writes cam->min_x .. max_y. */
int svgpu_camera_image_bounds(svgpu_ctx* ctx, svgpu_camera* cam);

/* data::frame_observation from the extractor's keypoints (system.cc:384-395):
 *   undist_kps   camera::*::undistort_keypoints   (cv::undistortPoints / cv::fisheye::undistortPoints restated with the
 *                reference's CV_32F camera matrix and criteria; radial_division closed form; equirectangular copy)
 *   bearings     camera::*::convert_keypoints_to_bearings, n x 3 doubles
 *   cell_off / cell_items   data::assign_keypoints_to_grid (data/common.cc:83-108) as CSR over cell = col * grid_rows + row:
 *                cell_off has grid_cols * grid_rows + 1 entries, cell_items cell_off[last] <= n keypoint indices (index order
 *                inside a cell, as the reference's push_back order)
 * Any output may be NULL.  Host in/out, synchronous. */
int svgpu_frame_observation(svgpu_ctx* ctx, const svgpu_camera* cam, const svgpu_keypoint* kps, int n, int grid_cols,
                            int grid_rows, svgpu_keypoint* undist_kps, double* bearings, int32_t* cell_off, int32_t* cell_items);

/* camera::*::convert_keypoints_to_bearings (camera/base.cc:160-164) alone, for callers that hold UNDISTORTED keypoints. */
int svgpu_keypoints_to_bearings(svgpu_ctx* ctx, const svgpu_camera* cam, const svgpu_keypoint* undist_kps, int n, double* bearings);

/* data::frame::can_observe (data/frame.cc:59-85) for n landmarks at once -- the loop of
 * tracking_module::search_local_landmarks (tracking_module.cc:554-594) and relocalizer.cc:345:
 * camera::*::reproject_to_image, landmark::is_inside_in_orb_scale (margins 1.3 and 1/1.3), the viewing-angle test
 * against ray_cos_thr and landmark::predict_scale_level (data/landmark.cc:336-353).
 *   rot_cw 9 doubles row-major, trans_cw 3, trans_wc 3 (the frame's camera centre, frame.cc:29)
 *   pos_w / mean_normal n x 3 doubles; min_valid_dist / max_valid_dist n floats
 *   skip     nullable n bytes: non-zero = landmark not offered (already tracked, will_be_erased, temporal-ratio rule)
 *   visible n bytes; reproj n x 2 doubles; x_right n floats; pred_scale_level n ints (-1 where not visible). */
int svgpu_reproject_landmarks(svgpu_ctx* ctx, const svgpu_camera* cam, const double* rot_cw, const double* trans_cw,
                              const double* trans_wc, int n, const double* pos_w, const double* mean_normal,
                              const float* min_valid_dist, const float* max_valid_dist, const uint8_t* skip, float ray_cos_thr,
                              int num_levels, float log_scale_factor, uint8_t* visible, double* reproj, float* x_right,
                              int32_t* pred_scale_level);

/* can_observe + projection::match_frame_and_landmarks (match/projection.cc:13-93) in one call, nothing returning to the
 * host in between: the visible landmarks become the queries of the cell matcher (window margin * scale_factors[pred level],
 * levels pred-1 .. pred+1, stereo gate against x_right when t_xright is given, SVGPU_MATCH_RATIO_SAME_OCTAVE rule with
 * thr = HAMMING_DIST_THR_HIGH) over the frame's keypoints binned on the device.
 *   lm_desc n x 32; scale_factors num_levels floats (orb_params::scale_factors_)
 *   frame side: tdesc nt x 32, t_xy nt x 2 undistorted positions, t_octave nt, occupied nullable (keypoint already holds an
 *   observed landmark, projection.cc:52-55), t_xright nullable (frm_obs.stereo_x_right_)
 *   match_lm n: keypoint index or -1 (the frm.add_landmark calls, in landmark order); visible / reproj / x_right /
 *   pred_scale_level as svgpu_reproject_landmarks (nullable). */
int svgpu_match_frame_and_landmarks(svgpu_ctx* ctx, const svgpu_camera* cam, const double* rot_cw, const double* trans_cw,
                                    const double* trans_wc, int n, const double* pos_w, const double* mean_normal,
                                    const float* min_valid_dist, const float* max_valid_dist, const uint8_t* skip,
                                    const uint8_t* lm_desc, float ray_cos_thr, int num_levels, const float* scale_factors,
                                    float log_scale_factor, float margin, const uint8_t* tdesc, const float* t_xy,
                                    const int32_t* t_octave, int nt, const uint8_t* occupied, const float* t_xright,
                                    int grid_cols, int grid_rows, unsigned thr, float lowe_ratio, int32_t* match_lm,
                                    int* num_matches, uint8_t* visible, double* reproj, float* x_right,
                                    int32_t* pred_scale_level);

/* ------------------------------------------------------------------------------ device-resident frame observations
 * data::frame_observation (data/frame_observation.h:12-38) of a frame or keyframe kept ON THE DEVICE: descriptors, undistorted keypoints,
 * stereo x_right, bearings and the keypoint grid of data::assign_keypoints_to_grid.  A tracked frame (tracking_module.cc:533-608) goes
 * extract -> match_current_and_last_frames -> pose optimizer -> match_frame_and_landmarks -> pose optimizer; with a resident frame its
 * descriptors cross PCIe once (down, for the host-side data::frame) and are never uploaded again.
 *   svgpu_frame_adopt_extraction  what system.cc:384-395 does after extract(): undistort_keypoints, convert_keypoints_to_bearings,
 *                                 assign_keypoints_to_grid -- on the keypoints / descriptors the context's LAST svgpu_orb_extract left on
 *                                 the device; undist_kps / bearings (nullable) return the host copies data::frame_observation holds
 *   svgpu_frame_upload            the same for an observation that exists on the host (keyframes of the map): undistorted keypoint
 *                                 records, descriptors, stereo x_right (nullable)
 *   svgpu_frame_set_stereo        stereo_x_right_ once match::stereo has produced it (NULL: monocular again)
 *   svgpu_frame_bind              ONE-SHOT: the next call of svgpu_match_in_cells / svgpu_match_frame_and_landmarks /
 *                                 svgpu_match_current_and_last_frames / svgpu_match_frame_and_keyframe_projection /
 *                                 svgpu_match_by_sim3_transform / svgpu_fuse_detect_duplication on `ctx` takes its keypoint side (tdesc, t_xy,
 *                                 t_octave, t_angle, t_xright, nt, image bounds, grid) from the frame: those arguments are then ignored (pass
 *                                 NULL / 0); `occupied` stays a host array of svgpu_frame_size bytes.  A frame may be bound on any context of
 *                                 its device.
 *   svgpu_match_set_query_blocks  ONE-SHOT for the next svgpu_match_in_cells: q_blocks[q] = 0 -> an accepted query q does NOT occupy its
 *                                 keypoint for later queries (the landmark it carries has no observation: `lm && lm->has_observation()`,
 *                                 projection.cc:52-55); NULL = every accepted query does */
typedef struct svgpu_frame svgpu_frame;
int svgpu_frame_create(svgpu_ctx* ctx, svgpu_frame** out);
void svgpu_frame_destroy(svgpu_frame* frame);
int svgpu_frame_size(const svgpu_frame* frame);
int svgpu_frame_adopt_extraction(svgpu_ctx* ctx, svgpu_frame* frame, const svgpu_camera* cam, int grid_cols, int grid_rows,
                                 svgpu_keypoint* undist_kps, double* bearings);
int svgpu_frame_upload(svgpu_ctx* ctx, svgpu_frame* frame, const svgpu_camera* cam, const svgpu_keypoint* undist_kps, const uint8_t* desc,
                       const float* x_right, int n, int grid_cols, int grid_rows);
int svgpu_frame_set_stereo(svgpu_ctx* ctx, svgpu_frame* frame, const float* x_right);
int svgpu_frame_bind(svgpu_ctx* ctx, const svgpu_frame* frame);
int svgpu_match_set_query_blocks(svgpu_ctx* ctx, const uint8_t* q_blocks);

/* ------------------------------------------------------------------------------ device-resident local map + tracked-frame chain
 * What tracking_module does per image between extract() and the keyframe decision (tracking_module.cc:253-275, 333-355, 533-608;
 * module/frame_tracker.cc:22-60) reads, of every landmark, five things: pos_w_, mean_normal_, the valid-distance range, the
 * representative descriptor and whether it has observations.  svgpu_map keeps exactly those ON THE DEVICE, indexed by
 * data::landmark::id_ (ids are dense: one atomic counter hands them out, data/landmark.cc:13), and is kept current by the few
 * mutators of data::landmark; a tracked frame then hands over landmark IDS -- of the last frame's
 * keypoints, of the local map -- instead of flattening thousands of records out of the shared_ptr graph, and the two halves of the
 * per-frame chain are ONE submission each with ONE synchronisation at the end:
 *   svgpu_track_motion     [extract -> undistort / bearings / grid ->] projection::match_current_and_last_frames -> pose_optimizer
 *   svgpu_track_local_map  frame::can_observe over the local landmarks -> projection::match_frame_and_landmarks -> pose_optimizer
 * (between the two the host runs update_local_map on the landmarks the first half matched: object-graph work, stays the reference's).
 * Results are identical to the separate entry points (svgpu_match_current_and_last_frames, svgpu_pose_optimize,
 * svgpu_reproject_landmarks, svgpu_match_in_cells) fed from host-flattened arrays: tests/test_gpu_track.py. */
typedef struct svgpu_map svgpu_map;
enum {
    SVGPU_LM_PRESENT = 1,          /* the landmark exists and !will_be_erased() */
    SVGPU_LM_HAS_OBSERVATION = 2,  /* landmark::has_observation() */
    SVGPU_LM_HAS_DESCRIPTOR = 4    /* !get_descriptor().empty() */
};
typedef struct svgpu_landmark_record { /* 96 bytes */
    double pos_w[3];                   /* landmark::pos_w_ */
    double mean_normal[3];             /* landmark::mean_normal_ */
    float min_valid_dist, max_valid_dist;
    uint8_t descriptor[32];
    uint32_t flags;                    /* SVGPU_LM_* */
    uint32_t reserved;
} svgpu_landmark_record;
int svgpu_map_create(svgpu_ctx* ctx, svgpu_map** out);
void svgpu_map_destroy(svgpu_map* map);
int svgpu_map_capacity(const svgpu_map* map); /* ids below this are addressable (grows with the largest id upserted) */
/* whole-record upsert of n landmarks (ids[i] -> records[i]; a later entry of the same id wins); synchronous */
int svgpu_map_upsert(svgpu_ctx* ctx, svgpu_map* map, int n, const uint32_t* ids, const svgpu_landmark_record* records);
/* landmark::prepare_for_erasing: flags -> 0 (ids beyond the capacity are ignored) */
int svgpu_map_erase(svgpu_ctx* ctx, svgpu_map* map, int n, const uint32_t* ids);
/* test hook: the records as the device holds them (flags 0 for ids it has never seen) */
int svgpu_map_download(svgpu_ctx* ctx, const svgpu_map* map, int n, const uint32_t* ids, svgpu_landmark_record* records);

typedef struct svgpu_tracker svgpu_tracker;
typedef struct svgpu_track_config {
    int num_levels;
    float scale_factors[16];         /* orb_params::scale_factors_ */
    float inv_level_sigma_sq[16];    /* orb_params::inv_level_sigma_sq_ */
    float log_scale_factor;          /* orb_params::log_scale_factor_ */
    int grid_cols, grid_rows;        /* frame_observation::num_grid_cols_ / rows_ */
    int is_monocular;                /* camera::setup_type_t::Monocular */
    float true_baseline;             /* camera::base::true_baseline_ */
    /* pose_optimizer_factory.h:18-26 (2 / 2 / 10) and the stop-flag reading of svgpu_pose_optimize */
    int po_num_trials_robust, po_num_trials, po_num_each_iter, po_reset_stop_flag_each_round;
} svgpu_track_config;
typedef struct svgpu_track_result {
    int n_keypoints;     /* of the current frame */
    int num_matches;     /* the matcher's return value */
    int num_valid;       /* pose optimizer: observations that are inliers at the end (0: fewer than 5 observations, pose unchanged) */
    int lm_iterations;
    int num_observations;/* edges the pose optimizer was given */
    int num_candidates;  /* entries of the candidate lists beyond their queries' own slots (diagnostics) */
    int replay_sweeps;   /* sweeps of the matcher's greedy replay, summed over its chunks (diagnostics) */
    int reserved;
    double pose_cw[12];  /* optimised [R|t], row-major 3x4 */
} svgpu_track_result;
/* One tracker per tracking thread: owns the chain's device and page-locked buffers.  `ctx` is the context its launches go to; for the
 * fused extraction of svgpu_track_motion it must be configured (svgpu_orb_configure). */
int svgpu_tracker_create(svgpu_ctx* ctx, svgpu_map* map, const svgpu_camera* cam, const svgpu_track_config* cfg, svgpu_tracker** out);
void svgpu_tracker_destroy(svgpu_tracker* tracker);
/* frame_tracker::motion_based_track (module/frame_tracker.cc:22-60) up to discard_outliers, as one submission.
 *   img != NULL   system::create_monocular_frame's device work comes first: ORB extraction of `img` (row stride `stride`), undistortion,
 *                 bearings and grid -> `cur` becomes the resident observation; kps / desc / undist_kps / bearings (each cap entries)
 *                 receive the host copies data::frame_observation holds (all four NULL: left in the tracker's own page-locked buffer,
 *                 svgpu_tracker_observation).  img == NULL: `cur` already holds the observation
 *                 (svgpu_frame_adopt_extraction / svgpu_frame_upload) and those four outputs are ignored.
 *   last, last_lm_ids   the last frame's resident observation and, per keypoint of it, the landmark id it holds (-1: none)
 *   pose_guess_cw / pose_last_cw   3x4 [R|t] row-major: velocity * last pose, and the last frame's pose (assume_forward / backward)
 *   match_last    svgpu_frame_size(last) entries: keypoint of `cur` the landmark of last keypoint i was matched to, or -1; the caller
 *                 replays curr_frm.add_landmark(lm, match_last[i]) in increasing i (projection.cc:202)
 *   outlier       per keypoint of `cur` (with an image: cap entries, cap >= svgpu_orb_max_keypoints covers every frame): the pose optimizer's flag
 * The caller compares result->num_matches with its threshold and, below it, calls again with img = NULL and twice the margin
 * (frame_tracker.cc:36-40): the optimisation that was enqueued behind the first matcher is then simply discarded. */
int svgpu_track_motion(svgpu_tracker* tracker, svgpu_frame* cur, const uint8_t* img, int stride, const svgpu_frame* last,
                       const int32_t* last_lm_ids, const double* pose_guess_cw, const double* pose_last_cw, float margin,
                       int check_orientation, svgpu_keypoint* kps, uint8_t* desc, svgpu_keypoint* undist_kps, double* bearings, int cap,
                       int32_t* match_last, uint8_t* outlier, svgpu_track_result* result);
/* The observation the last svgpu_track_motion with an image brought back, where the copy engine left it (page-locked memory of the tracker;
 * valid until the tracker's next call): pass NULL for kps / desc / undist_kps / bearings there and read it here without a second copy.
 * Each pointer is nullable; returns the keypoint count (0 when there is none). */
int svgpu_tracker_observation(const svgpu_tracker* tracker, const svgpu_keypoint** kps, const uint8_t** desc, const svgpu_keypoint** undist_kps,
                              const double** bearings);
/* The same for a STEREO frame (system::create_stereo_frame, system.cc:406-447, then the tracker): both images go down, the right one is
 * extracted on `ctx_right` (a second context of the tracker's device, configured like the tracker's) and its own stream beside the left
 * one's, match::stereo::compute (match/stereo.cc:20-114) runs behind both on the device-resident keypoints, descriptors and pyramids, the
 * left observation (undistortion, bearings, grid) follows, then the matcher and the optimiser with the stereo gates and edges -- still ONE
 * submission and ONE synchronisation.  The observation stays in the tracker's page-locked buffer: svgpu_tracker_observation for the
 * keypoints / descriptors / undistorted keypoints / bearings, svgpu_tracker_observation_stereo for stereo_x_right_ / depths_
 * (-1 where the left keypoint found no partner).  The tracker must have been created with is_monocular = 0. */
int svgpu_track_motion_stereo(svgpu_tracker* tracker, svgpu_ctx* ctx_right, svgpu_frame* cur, const uint8_t* img_left, int stride_left,
                              const uint8_t* img_right, int stride_right, const svgpu_frame* last, const int32_t* last_lm_ids,
                              const double* pose_guess_cw, const double* pose_last_cw, float margin, int check_orientation, int cap,
                              int32_t* match_last, uint8_t* outlier, svgpu_track_result* result);
int svgpu_tracker_observation_stereo(const svgpu_tracker* tracker, const float** stereo_x_right, const float** depths);
/* ... and for an RGB-D frame (system::create_RGBD_frame, system.cc:466-526): `depth` = the depth image in metres as CV_32F
 * (util::convert_to_true_depth already applied by the caller) with the SAME height and width as `img` (the library reads height rows of
 * width floats; it cannot check the size of the buffer behind the pointer), `depth_stride` in FLOATS per row (>= width).  The depth is sampled at the distorted
 * keypoint (img_depth.at<float>(y, x), coordinates truncated), stereo_x_right_ = undist.x - focal_x_baseline / depth (-1 where depth <= 0),
 * inside the frame-observation kernel of the same submission; read back with svgpu_tracker_observation_stereo. */
int svgpu_track_motion_rgbd(svgpu_tracker* tracker, svgpu_frame* cur, const uint8_t* img, int stride, const float* depth, int depth_stride,
                            const svgpu_frame* last, const int32_t* last_lm_ids, const double* pose_guess_cw, const double* pose_last_cw,
                            float margin, int check_orientation, int cap, int32_t* match_last, uint8_t* outlier, svgpu_track_result* result);
/* tracking_module::search_local_landmarks + optimize_current_frame_with_local_map's optimisation (tracking_module.cc:533-608, 441-446)
 * as one submission.
 *   cur_lm_ids    per keypoint of `cur`: the landmark id the frame holds now (-1: none) -- after discard_outliers and update_local_map's
 *                 clean-up, i.e. curr_frm.get_landmarks() as ids
 *   local_ids     n_local entries: landmark ids of local_landmarks_ in order; -1 = not offered to can_observe (already in the frame,
 *                 will_be_erased, temporal-ratio rule :565-580)
 *   pose_cw       nullable: NULL = the pose the tracker's last optimisation left on the device
 *   match_local   n_local: keypoint the landmark was matched to or -1 (replay frm.add_landmark in increasing order, projection.cc:88)
 *   visible       nullable, n_local: can_observe's verdict (increase_num_observable, tracking_module.cc:588)
 *   outlier       per keypoint of `cur` */
int svgpu_track_local_map(svgpu_tracker* tracker, const svgpu_frame* cur, const int32_t* cur_lm_ids, int n_local, const int32_t* local_ids,
                          const double* pose_cw, float margin, float lowe_ratio, float ray_cos_thr, int32_t* match_local, uint8_t* visible,
                          uint8_t* outlier, svgpu_track_result* result);
/* lm_to_reproj / lm_to_x_right / lm_to_scale of the last svgpu_track_local_map, fetched only when somebody wants them (each nullable) */
int svgpu_track_local_map_observability(svgpu_tracker* tracker, int n_local, double* reproj, float* x_right, int32_t* pred_scale_level);
/* diagnostics: kernel launches + runtime copies the tracker enqueued, and stream synchronisations it waited on, since creation */
int svgpu_tracker_counters(const svgpu_tracker* tracker, long long* launches, long long* host_syncs);
/* debug (SVGPU_TRACK_STAMPS set): 100 MHz wall-clock stamps of the last optimisation kernel's phases, [0] = how many follow; else NULL / zeros */
const unsigned long long* svgpu_tracker_debug_stamps(const svgpu_tracker* tracker);

/* ------------------------------------------------------------------------------------------------ image ingest
 * Stands behind what system::create_monocular_frame / create_stereo_frame / create_RGBD_frame do to an image before the extractor sees it:
 *   util::convert_to_grayscale(img, color_order)        (util/image_converter.cc:8-39)   cv::cvtColor COLOR_{RGB,BGR,RGBA,BGRA}2GRAY
 *   util::convert_to_true_depth(img, depthmap_factor)   (util/image_converter.cc:41-43)  img.convertTo(img, CV_32F, 1.0 / factor)
 *   util::stereo_rectifier::rectify                     (util/stereo_rectifier.cc:62-66) cv::remap(.., INTER_LINEAR), constant border 0
 * in OpenCV's 8-bit fixed-point arithmetic (tests/ingest_problems.py states it; DESIGN.md section 11: PARITY UNPINNED).  With maps the
 * order is the reference's: remap the image as read, per channel, then convert to grey.  The rectified colour image is never stored.
 * util::equalize_histogram and the construction of the maps (cv::initUndistortRectifyMap, once per session) stay with the caller. */
typedef struct svgpu_ingest svgpu_ingest;
typedef enum svgpu_color_order { SVGPU_COLOR_GRAY = 0, SVGPU_COLOR_RGB = 1, SVGPU_COLOR_BGR = 2 } svgpu_color_order; /* camera::color_order_t */
typedef enum svgpu_depth_type { SVGPU_DEPTH_NONE = 0, SVGPU_DEPTH_U16 = 1, SVGPU_DEPTH_F32 = 2 } svgpu_depth_type;   /* CV_16U / CV_32F */
/* One ingest per camera: `width` x `height` frames of `channels` interleaved 8-bit channels (1, 3 or 4; 4 = alpha last, ignored) in
 * `color_order` (Gray with 3 or 4 channels is refused).  map_x / map_y: both NULL (no rectification) or both set: CV_32FC1 maps of
 * width x height entries (the rectified image has the size of the image as read, as in the reference), rows `map_stride` BYTES apart,
 * host memory.  The float maps are compiled once, on the device, into 8 bytes per pixel (clamped integer source position + the two 5-bit
 * fractions); no frame reads a float again.  Map VALUES are never an error: outside, non-finite and huge entries give 0.  Synchronous. */
int svgpu_ingest_create(svgpu_ctx* ctx, int width, int height, int channels, int color_order, const float* map_x, const float* map_y,
                        int map_stride, svgpu_ingest** out);
void svgpu_ingest_destroy(svgpu_ingest* ingest);
/* One frame, host in / host out, synchronous (the counterpart of svgpu_orb_extract): src rows `src_stride` bytes apart
 * (>= width * channels), dst 8UC1 rows `dst_stride` bytes apart (>= width). */
int svgpu_ingest_gray(svgpu_ctx* ctx, const svgpu_ingest* ingest, const uint8_t* src, int src_stride, uint8_t* dst, int dst_stride);
/* Throughput path: `batch` raw frames resident in HBM -> `batch` grey frames in HBM, asynchronous, one launch.  The output layout
 * (frame b at dst_dev + b * dst_frame_stride, rows dst_row_stride apart) is what svgpu_orb_extract_batch_device takes as imgs_dev. */
int svgpu_ingest_gray_batch_device(svgpu_ctx* ctx, const svgpu_ingest* ingest, const uint8_t* src_dev, int batch, size_t src_frame_stride,
                                   int src_row_stride, uint8_t* dst_dev, size_t dst_frame_stride, int dst_row_stride, void* stream);
/* convert_to_true_depth: dst[y][x] = (float)src[y][x] * (float)(1.0 / depthmap_factor).  src_type: svgpu_depth_type (U16 or F32);
 * strides in BYTES; depthmap_factor must be finite and non-zero.  Host in / host out, synchronous ... */
int svgpu_ingest_depth(svgpu_ctx* ctx, const void* src, int src_type, int src_stride, int width, int height, double depthmap_factor, float* dst,
                       int dst_stride);
/* ... and device in / device out on a stream, asynchronous */
int svgpu_ingest_depth_device(svgpu_ctx* ctx, const void* src_dev, int src_type, int src_stride, int width, int height, double depthmap_factor,
                              float* dst_dev, int dst_stride, void* stream);
/* Switches the tracker's fused extraction to RAW frames.  Afterwards `img` / `img_left` of svgpu_track_motion / _stereo / _rgbd is a frame
 * in ingest_left's input format and `img_right` one in ingest_right's, `stride` in bytes of the raw row; with depth_type != 0 the `depth`
 * argument of svgpu_track_motion_rgbd points to raw CV_16U / CV_32F rows, `depth_stride` BYTES apart, and is multiplied by
 * (float)(1.0 / depthmap_factor) on the device.  The raw frames go down in the submission's own copies, the ingest kernels run on the
 * submission's own streams between the upload and the extraction (the right image's on the right context's stream): still one submission
 * and one synchronisation, one more launch per ingested image and one for the depth.  Every argument is nullable / 0 = that input stays
 * as before; all off restores the grey path.  The ingests' output size must be the configured extractor's (checked per call, before any
 * launch); a pair of ingests must agree on it.  The ingests must outlive the tracker or be switched off first. */
int svgpu_tracker_set_ingest(svgpu_tracker* tracker, const svgpu_ingest* ingest_left, const svgpu_ingest* ingest_right, int depth_type,
                             double depthmap_factor);

/* ------------------------------------------------------------------------------ function-specific matchers
 * One entry point per reference method: candidate generation (reprojection + grid cells, or BoW buckets), the method's own pair
 * gates and the exact sequential bookkeeping all run on the device; the adaptor classes of stella_vslam_amd/host/ flatten the
 * frame / keyframe / landmark objects into these arrays and write the results back.  Common conventions:
 *   landmarks (queries)  pos_w n x 3 doubles, `valid` 0 = not offered (null, will_be_erased, already matched ...: the method's own
 *                        `continue` tests on the object graph), min/max_valid_dist (landmark::get_min/max_valid_distance),
 *                        mean_normal n x 3 (get_obs_mean_normal), lm_desc n x 32 (get_descriptor)
 *   keypoint side        tdesc nt x 32, t_xy nt x 2 undistorted positions, t_octave, t_angle, t_xright (stereo_x_right_, nullable),
 *                        binned on the device by data::assign_keypoints_to_grid over cam->min_x .. max_y and grid_cols x grid_rows
 *   scale_factors / inv_level_sigma_sq   orb_params tables of num_levels floats, log_scale_factor = orb_params::log_scale_factor_
 *   outputs              per query the matched keypoint index or -1, in query order; the adaptor replays them onto the objects
 * All host in/out, synchronous. */

/* camera::*::reproject_to_bearing (perspective.cc:150-170, fisheye.cc:189-209, equirectangular.cc:75-80, radial_division.cc:135-156):
 * used by the triangulation matchers for the epipole of keyframe 1 in keyframe 2.  Pure host function. */
int svgpu_reproject_to_bearing(const svgpu_camera* cam, const double* rot_cw, const double* trans_cw, const double* pos_w, double* bearing,
                               int* valid);

/* projection::match_current_and_last_frames (match/projection.cc:95-207): the landmarks of the last frame's keypoints reprojected
 * with the current pose guess; level window from the keypoint's octave in the last frame and the forward / backward motion test
 * (:108-157; is_monocular = camera setup Monocular, true_baseline = camera::base::true_baseline_); gates: keypoint already holds an
 * observed landmark (`occupied`), stereo x_right, orientation; best <= HAMMING_DIST_THR_HIGH.
 *   lm_has_observation  nullable (all 1): 0 = the landmark carries no observation, so the keypoint it is attached to stays open for
 *                       later landmarks (`curr_lm && curr_lm->has_observation()`, :167-170) and a later match overwrites it
 *   match_last[i]       keypoint of the current frame matched to landmark i (curr_frm.add_landmark(lm, best_idx) in order) */
int svgpu_match_current_and_last_frames(svgpu_ctx* ctx, const svgpu_camera* cam, const double* rot_cw, const double* trans_cw, const double* rot_lw,
                                        const double* trans_lw, int is_monocular, float true_baseline, int n_last, const double* pos_w,
                                        const uint8_t* valid, const uint8_t* lm_desc, const int32_t* octave_last, const float* angle_last,
                                        const uint8_t* lm_has_observation, int num_levels, const float* scale_factors, float margin,
                                        const uint8_t* tdesc, const float* t_xy, const int32_t* t_octave, const float* t_angle, int nt,
                                        const uint8_t* occupied, const float* t_xright, int grid_cols, int grid_rows, int check_orientation,
                                        int32_t* match_last, int* num_matches);

/* projection::match_frame_and_keyframe (match/projection.cc:209-319; relocalisation): the keyframe's landmarks into the frame;
 * double-precision distance-range test (:233-241), landmark::predict_scale_level, window [l-1, l+1]; gates: frame keypoint already
 * holds a landmark (`occupied` = frm_landmarks non-null), orientation against the KEYFRAME keypoint's angle; best <= hamm_dist_thr.
 *   valid  = landmark non-null, not will_be_erased, not in already_matched_lms */
int svgpu_match_frame_and_keyframe_projection(svgpu_ctx* ctx, const svgpu_camera* cam, const double* rot_cw, const double* trans_cw, int n_kf,
                                              const double* pos_w, const uint8_t* valid, const float* min_valid_dist, const float* max_valid_dist,
                                              const uint8_t* lm_desc, const float* angle_kf, int num_levels, const float* scale_factors,
                                              float log_scale_factor, float margin, unsigned hamm_dist_thr, const uint8_t* tdesc, const float* t_xy,
                                              const int32_t* t_octave, const float* t_angle, int nt, const uint8_t* occupied, int grid_cols,
                                              int grid_rows, int check_orientation, int32_t* match_kf, int* num_matches);

/* projection::match_by_Sim3_transform (match/projection.cc:321-416; loop detection): sim3_cw 4x4 row-major; converted to SE3 as the
 * reference does (:326-330); distance range, viewing-angle test dot(v, normal) >= 0.5 |v|, predicted level; candidates skip keypoints
 * that already hold a landmark (`occupied` = matched_lms_in_keyfrm non-null); best <= HAMMING_DIST_THR_LOW, no orientation test.
 *   valid  = landmark not will_be_erased and not already in matched_lms_in_keyfrm */
int svgpu_match_by_sim3_transform(svgpu_ctx* ctx, const svgpu_camera* cam, const double* sim3_cw, int n, const double* pos_w, const uint8_t* valid,
                                  const float* min_valid_dist, const float* max_valid_dist, const double* mean_normal, const uint8_t* lm_desc,
                                  int num_levels, const float* scale_factors, float log_scale_factor, float margin, const uint8_t* tdesc,
                                  const float* t_xy, const int32_t* t_octave, int nt, const uint8_t* occupied, int grid_cols, int grid_rows,
                                  int32_t* match_lm, int* num_matches);

/* projection::match_keyframes_mutually (match/projection.cc:418-629): landmarks of keyframe 1 into keyframe 2 through the similarity
 * (s_12, rot_12, trans_12) and vice versa, two independent passes (no bookkeeping inside a pass), then the cross-check.
 *   valid1 / valid2   landmark non-null, not will_be_erased, not already matched between the two keyframes (:441-450, 466-468)
 *   desc*, xy*, octave*   the keyframes' own keypoints (the side that is searched in the other pass)
 *   matched_2_in_1 / matched_1_in_2   the two passes; mutual_2_in_1[i] = idx_2 where both agree (:598-610), num_matches counts those.
 * As in the reference, both passes test "inside the image" with keyframe 2's camera (:477, 550). */
int svgpu_match_keyframes_mutually(svgpu_ctx* ctx, const svgpu_camera* cam1, const svgpu_camera* cam2, const double* rot_1w, const double* trans_1w,
                                   const double* rot_2w, const double* trans_2w, float s_12, const double* rot_12, const double* trans_12,
                                   int n1, const double* pos_w1, const uint8_t* valid1, const float* min_valid1, const float* max_valid1,
                                   const uint8_t* lm_desc1, const uint8_t* desc1, const float* xy1, const int32_t* octave1,
                                   int n2, const double* pos_w2, const uint8_t* valid2, const float* min_valid2, const float* max_valid2,
                                   const uint8_t* lm_desc2, const uint8_t* desc2, const float* xy2, const int32_t* octave2,
                                   int num_levels, const float* scale_factors, float log_scale_factor, float margin, int grid_cols, int grid_rows,
                                   int32_t* matched_2_in_1, int32_t* matched_1_in_2, int32_t* mutual_2_in_1, int* num_matches);

/* fuse::detect_duplication<T> (match/fuse.cc:11-154): landmarks_to_check reprojected into a keyframe; distance range, viewing angle,
 * predicted level; per candidate the optional chi-square reprojection gate (do_reprojection_matching: 5.99146 / 7.81473 against the
 * squared error times inv_level_sigma_sq of the keypoint's octave, 3 dof when the keypoint has a stereo x_right, :92-119) and
 * `already_matched_idx_in_keyfrm`; best <= HAMMING_DIST_THR_LOW.
 *   valid     = landmark non-null, not will_be_erased, not observed in the keyframe (:27-35)
 *   best_idx  per landmark the keyframe keypoint it fuses with, or -1; the adaptor sorts them into duplicated_lms_in_keyfrm /
 *             new_connections by keyfrm->get_landmark(best_idx) (:130-147) */
int svgpu_fuse_detect_duplication(svgpu_ctx* ctx, const svgpu_camera* cam, const double* rot_cw, const double* trans_cw, int n, const double* pos_w,
                                  const uint8_t* valid, const float* min_valid_dist, const float* max_valid_dist, const double* mean_normal,
                                  const uint8_t* lm_desc, int num_levels, const float* scale_factors, const float* inv_level_sigma_sq,
                                  float log_scale_factor, float margin, int do_reprojection_matching, const uint8_t* tdesc, const float* t_xy,
                                  const int32_t* t_octave, const float* t_xright, int nt, int grid_cols, int grid_rows, int32_t* best_idx,
                                  int* num_fused);

/* robust::match_for_triangulation (match/robust.cc:14-146) and bow_tree::match_for_triangulation (match/bow_tree.cc:11-167).
 * Keypoints WITHOUT a landmark on both sides (has_lm* = 1 excludes); per pair: orientation, Hamming <= 50 and <= the running best,
 * the epipole test (cos > 0.99862953475 rejected unless one of the two is a stereo keypoint, xright* >= 0) and
 * check_epipolar_constraint(bearing_1, bearing_2, E_12, ...) in fp64 (match/base.h:67-79) with the threshold
 * residual_rad_thr * scale_factors[octave1]; strict '<' updates, Lowe ratio, a keypoint of keyframe 2 is taken once.
 *   node1 / node2   both NULL: robust (all keypoints of keyframe 2 are candidates, queries in index order);
 *                   both given: bow_tree -- the bow_feat_vec_ node of every keypoint (svgpu_bow_transform's node_id, < 0 = none); the
 *                   merge-join of the two maps (:37-40, 142-153) runs on the device: queries in (node, index) order, candidates = the
 *                   keypoints of keyframe 2 in the same node, index order
 *   epipole_in_2 / valid_epipole   svgpu_reproject_to_bearing(cam2, rot_2w, trans_2w, keyfrm_1 camera centre)   (:22-27)
 *   matched_2_in_1[i]   keypoint of keyframe 2 or -1 (the reference returns the pairs sorted by i). */
int svgpu_match_for_triangulation(svgpu_ctx* ctx, const uint8_t* desc1, const float* angle1, const int32_t* octave1, const double* bearings1,
                                  const uint8_t* has_lm1, const float* xright1, int n1, const uint8_t* desc2, const float* angle2,
                                  const double* bearings2, const uint8_t* has_lm2, const float* xright2, int n2, const int32_t* node1,
                                  const int32_t* node2, const double* E_12, const double* epipole_in_2, int valid_epipole, const float* scale_factors,
                                  int num_levels, float residual_rad_thr, float lowe_ratio, int check_orientation, int32_t* matched_2_in_1,
                                  int* num_matches);

/* module::two_view_triangulator::triangulate (module/two_view_triangulator.cc:19-96, .h:89-110) for a list of keypoint matches between
 * keyframe 1 and keyframe 2: the step between svgpu_match_for_triangulation and the landmark refresh in
 * mapping_module::triangulate_with_two_keyframes (mapping_module.cc:343-375).  One lane per match, fp64 except where the reference
 * computes in float.  Per match (idx1[m], idx2[m]):
 *   is_stereo_k = 0 <= xright_k[idx_k]; world rays and cos_rays_parallax; cos_stereo_parallax_k = cos(2 atan2(true_baseline_k / 2, depth_k))
 *   or 2.0 (:33-42); the three-way choice of :46-67 with its strict comparisons: solve::triangulator::triangulate(bearing_1, bearing_2,
 *   cam_pose_1w, cam_pose_2w) (solve/triangulator.h:76-88: null vector of the 4 x 4 A, here by a one-sided Jacobi on its columns), else
 *   data::triangulate_stereo of keyframe 1, else of keyframe 2 (data/common.cc:192-261, unproj_x / unproj_y rounded to float), else reject;
 *   check_depth_is_positive (always true for equirectangular); check_reprojection_error with camera::*::reproject_to_image and
 *   chi_sq_2D = 5.99146f / chi_sq_3D = 7.81473f times level_sigma_sq[octave] (:98-129); check_scale_factors with
 *   ratio_factor = 2.0f * max(scale_factor_1, scale_factor_2) (.h:94-110, .cc:16).
 *   pose_kw          12 doubles: rows 0..2 of cam_pose_kw, row-major ([rot_kw | trans_kw]); the camera centre is derived as
 *                    keyframe::set_pose_cw does (data/keyframe.cc:365-376)
 *   true_baseline_k  camera::base::true_baseline_ (svgpu_camera does not carry it)
 *   xy / octave / bearings   undist_keypts_[i].pt (n x 2 floats), .octave, bearings_ (n x 3 doubles)
 *   xright / depth   stereo_x_right_ / depths_, nullable = empty (-1 for every keypoint)
 *   scale_factors / level_sigma_sq   orb_params tables of num_levels floats; scale_factor_k = orb_params::scale_factor_
 *   idx2 == NULL     idx1 is matched_2_in_1 of length num_matches = n1, the output of svgpu_match_for_triangulation: entry i pairs keypoint i
 *                    of keyframe 1 with keypoint idx1[i] of keyframe 2; -1 = no match, status SVGPU_TRI_SKIPPED
 *   pos_w            num_matches x 3; meaningful where status is SVGPU_TRI_ACCEPTED (else the rejected candidate, or zeros)
 *   status           num_matches bytes: which gate rejected the match (the reference returns only a bool)
 *   num_accepted     nullable
 * An index or octave out of range, or a stereo keypoint of an equirectangular camera (the reference throws, data/common.cc:239-241),
 * is SVGPU_ERR_INVALID before anything is launched; num_matches == 0 is a success that launches nothing.  Host in/out, synchronous. */
#define SVGPU_TRI_ACCEPTED 0
#define SVGPU_TRI_NO_MODE 1       /* neither enough parallax for two cameras nor a usable stereo keypoint (:65-67) */
#define SVGPU_TRI_DEPTH 2         /* check_depth_is_positive (:70-73) */
#define SVGPU_TRI_REPROJECTION 3  /* check_reprojection_error (:76-82) */
#define SVGPU_TRI_SCALE 4         /* check_scale_factors (:85-90) */
#define SVGPU_TRI_SKIPPED 255     /* matched_2_in_1 form: keypoint without a match */
int svgpu_triangulate_two_views(svgpu_ctx* ctx, const svgpu_camera* cam1, const double* pose_1w, double true_baseline_1, const float* xy1, const int32_t* octave1,
                                const double* bearings1, const float* xright1, const float* depth1, int n1, const svgpu_camera* cam2, const double* pose_2w,
                                double true_baseline_2, const float* xy2, const int32_t* octave2, const double* bearings2, const float* xright2,
                                const float* depth2, int n2, const float* scale_factors, const float* level_sigma_sq, int num_levels, float scale_factor_1,
                                float scale_factor_2, float rays_parallax_deg_thr, const int32_t* idx1, const int32_t* idx2, int num_matches, double* pos_w,
                                uint8_t* status, int* num_accepted);

/* The loop of mapping_module::create_new_landmarks (mapping_module.cc:274-341) in ONE launch: the current keyframe (side 1 of every
 * match) against num_neighbours covisible keyframes.  A view is one side's arguments of svgpu_triangulate_two_views; the matches of
 * neighbour k are entries match_off[k] .. match_off[k + 1] of idx1 / idx2 / pos_w / status (match_off[0] = 0, a neighbour may have none).
 * idx2 == NULL: every non-empty range is a matched_2_in_1 of length view1->n.  num_accepted: nullable, num_neighbours ints.
 * Results equal num_neighbours single calls bit for bit. */
typedef struct svgpu_triangulate_view {
    const svgpu_camera* cam;
    const double* pose_cw; /* 12 doubles, as pose_kw above */
    double true_baseline;
    const float* xy;
    const int32_t* octave;
    const double* bearings;
    const float* xright; /* nullable */
    const float* depth;  /* nullable */
    int32_t n;
    float scale_factor;
} svgpu_triangulate_view;
int svgpu_triangulate_two_views_batch(svgpu_ctx* ctx, const svgpu_triangulate_view* view1, const svgpu_triangulate_view* neighbours, int num_neighbours,
                                      const int32_t* match_off, const float* scale_factors, const float* level_sigma_sq, int num_levels,
                                      float rays_parallax_deg_thr, const int32_t* idx1, const int32_t* idx2, double* pos_w, uint8_t* status, int* num_accepted);

/* ------------------------------------------------------------------------------ PnP pose from 2D-3D matches (EPnP + RANSAC)
 * solve::pnp_solver (solve/pnp_solver.cc): the pose step of module::relocalizer::relocalize_by_pnp_solver (module/relocalizer.cc:134-209)
 * and of module::loop_detector (module/loop_detector.cc:423-446), for every candidate keyframe in one call.  fp64, one wavefront per
 * correspondence set or RANSAC hypothesis; Eigen's JacobiSVD is replaced by Jacobi iterations of the project's own, so singular vectors
 * may differ from Eigen's in sign and, inside a null space, in basis.
 *
 * svgpu_pnp_compute_pose: pnp_solver::compute_pose (:155-206) for num_sets correspondence sets; set s is entries set_off[s] ..
 * set_off[s + 1] of bearings / pos_w (n x 3 doubles each; set_off[0] = 0, every set holds at least 4 correspondences).
 *   choose_control_points (:208-238), compute_barycentric_coordinates with the D(i) > 1e-6 pseudo-inverse rule (:240-275), M^T M and its
 *   singular vectors 11 - j, compute_L_6x10 / compute_rho (:502-548), find_initial_betas_2 / _3 / _4 with every sign rule (:386-500),
 *   gauss_newton with gauss_newton_num_iter Householder-QR steps (:550-579), compute_ccs / compute_pcs with the z-sign flip (:303-334),
 *   estimate_R_and_t with the det < 0 repair (:350-384), reprojection_error (:336-348) and the strict `<` choice over N = 2, 3, 4.
 *   pose_cw        num_sets x 12: rows 0..2 of [rot_cw | trans_cw], row-major (as svgpu_triangulate_view::pose_cw); NaN when no N
 *                  gave a comparable error (the reference leaves its outputs untouched)
 *   reproj_error   num_sets: the value compute_pose returns
 * Non-monotone offsets or a set of fewer than 4 are SVGPU_ERR_INVALID before anything is launched; num_sets == 0 is a success. */
int svgpu_pnp_compute_pose(svgpu_ctx* ctx, int num_sets, const int32_t* set_off, const double* bearings, const double* pos_w,
                           int gauss_newton_num_iter, double* pose_cw, double* reproj_error);

/* pnp_solver::find_via_ransac (:44-124) for num_problems problems (candidate keyframes) at once; problem p is entries match_off[p] ..
 * match_off[p + 1] of bearings / pos_w / octaves / is_inlier (match_off[0] = 0, a problem may be empty).
 *   scale_factors / num_levels   orb_params::scale_factors_; max_cos_errors_ is computed here, on the host, as the constructor does
 *                  (:27-32): util::cos(scale_factors[octave] * pi / 180), a float
 *   samples        num_problems x num_iter x 4 indices local to their problem: what util::create_random_array(4, 0, n - 1, engine)
 *                  (util/random_array.cc:26-63) returned for every iteration (:73).  The table is an input: the engine is host state,
 *                  and with the draws made elsewhere the device is deterministic.  Entries of a problem that does not run are not read.
 *   per hypothesis compute_pose of the four sampled correspondences, check_inliers (:126-153: max_cos_error < cos_angle, strict; the cost
 *                  adds 1 - cos_angle for an inlier and 1 - max_cos_error for an outlier)
 *   selection      in iteration order, num_inliers > min_num_inliers && min_cost > cost, both strict (:95): the first of equal costs
 *                  stays, a NaN cost never wins; valid = min_cost < DBL_MAX (:103)
 *   recompute      != 0: compute_pose over the winner's inliers, in ascending index order, replaces the pose of a valid problem (:109-123)
 *                  -- unless no N gave it a comparable error: the pose then stays the winning hypothesis', as the reference leaves it
 *   valid / pose_cw / best_iter   per problem; best_iter is the winning iteration or -1, pose_cw is zero when invalid
 *   is_inlier      one byte per match: the winner's flags, zero when invalid
 *   hyp_pose / hyp_num_inliers / hyp_cost   nullable diagnostics, num_problems x num_iter (x 12): what every hypothesis gave (zero for a
 *                  problem that did not run)
 * A problem with fewer than 4 or fewer than min_num_inliers matches is valid = 0 and launches nothing for itself (:49-52).
 * SVGPU_ERR_INVALID before anything is launched: an octave outside [0, num_levels), a sample index outside its problem, an index repeated
 * within one sample, non-monotone offsets.  num_problems == 0 is a success.  Host in/out, synchronous, one synchronisation per call. */
int svgpu_pnp_ransac_batch(svgpu_ctx* ctx, int num_problems, const int32_t* match_off, const double* bearings, const double* pos_w,
                           const int32_t* octaves, const float* scale_factors, int num_levels, int min_num_inliers, int num_iter,
                           const uint32_t* samples, int recompute, int gauss_newton_num_iter, uint8_t* valid, double* pose_cw,
                           uint8_t* is_inlier, int32_t* best_iter, double* hyp_pose, int32_t* hyp_num_inliers, double* hyp_cost);

/* One problem: the batch of one, bit for bit. */
int svgpu_pnp_ransac(svgpu_ctx* ctx, const double* bearings, const double* pos_w, const int32_t* octaves, int num_matches,
                     const float* scale_factors, int num_levels, int min_num_inliers, int num_iter, const uint32_t* samples, int recompute,
                     int gauss_newton_num_iter, uint8_t* valid, double* pose_cw, uint8_t* is_inlier, int32_t* best_iter, double* hyp_pose,
                     int32_t* hyp_num_inliers, double* hyp_cost);

/* ------------------------------------------------------------------------------ Sim3 pose-graph optimisation (loop correction)
 * optimize::graph_optimizer::optimize (optimize/graph_optimizer.cc:26-303), the step module::global_optimization_module::correct_loop runs
 * between loop validation and the global bundle adjustment.  Every vertex is a Sim3 (8 doubles: qx qy qz qw tx ty tz s, g2o's unit
 * quaternion, translation, scale), every edge the 7-vector log(Sim3_21 * v1 * v2^-1) with identity information and g2o's numeric Jacobian
 * (central differences, delta 1e-9, through exp(update) * estimate; with fix_scale coordinate 6 of every update is zero).  Levenberg-
 * Marquardt as svgpu_global_ba runs it (lambda0 = 1e-5 max diag H, at most 10 damping trials per iteration) with terminate_action on the
 * relative chi2 gain; no robust kernel.  The damped 7x7-block system is solved by block-Jacobi PCG to a relative residual of 1e-14, capped
 * at 10 iterations per unknown.  fp64 throughout, sums in a fixed order, no atomics: two calls on the same input are bit-equal.
 *   sim3 / fixed      num_vertices x 8 doubles, num_vertices bytes (non-zero: the vertex is fixed and comes back bit-equal)
 *   edge_v1 / edge_v2 / edge_sim3_21   num_edges vertex indices each, num_edges x 8 doubles.  Duplicate edges between one pair are allowed;
 *                     an edge between two fixed vertices contributes to chi2 only
 *   sim3_out          num_vertices x 8; pose_cw_out (nullable) num_vertices x 12: rows 0..2 of [R | t / s] as the reference writes the
 *                     pose back (:272-278, the scale rounded to a float first)
 * SVGPU_ERR_INVALID before anything is launched: num_vertices or num_edges < 1, max_iterations < 0, an index out of range, a self-edge, a
 * quaternion whose squared norm is further than 1e-9 from 1, a scale that is not positive and finite, a free vertex without an edge, no
 * fixed vertex.  Host in/out, synchronous: one upload, the launches on the context's stream, one read-back; the damping decisions are
 * taken on the device and the host only polls for the end of the run between batches of enqueued trials. */
typedef struct svgpu_pose_graph_stats {
    int32_t lm_iterations;    /* LM iterations run */
    int32_t lm_trials;        /* damping trials = linear solves */
    int32_t pcg_iterations;   /* PCG iterations over all solves */
    int32_t pcg_capped;       /* solves that ended at the iteration cap */
    int32_t stopped_by_gain;  /* terminate_action raised the stop flag */
    int32_t num_free;         /* free vertices */
    double initial_chi2;
    double final_chi2;
    double lambda;            /* damping after the last trial */
} svgpu_pose_graph_stats;
int svgpu_pose_graph_optimize(svgpu_ctx* ctx, int num_vertices, const double* sim3, const uint8_t* fixed, int num_edges, const int32_t* edge_v1,
                              const int32_t* edge_v2, const double* edge_sim3_21, int fix_scale, int max_iterations, double gain_threshold,
                              double* sim3_out, double* pose_cw_out, svgpu_pose_graph_stats* stats);

/* The same call with a choice of the linear solver of the damped system (options == NULL: PCG; svgpu_pose_graph_optimize IS this call
 * with PCG, bit for bit).  SVGPU_PG_SOLVER_ENVELOPE factors the system directly: a block envelope (skyline) LL^T with 7x7 blocks in one
 * workgroup, in the elimination order -- natural, interleaved from both ends, or reverse Cuthill-McKee -- whose lower envelope is the
 * smallest (planned on the host).  fp64, fixed summation order, bit-reproducible.  A pivot that is not positive and finite fails the
 * damping trial, which is then rejected as if chi2 had risen; when all 10 trials of an iteration fail the run ends and the call returns
 * SVGPU_ERR_NUMERIC (the outputs hold the last estimate).  With the envelope solver pcg_iterations and pcg_capped are 0.
 * SVGPU_ERR_INVALID before anything is launched, beyond the cases above: an unknown solver, a reserved field that is not 0, an envelope
 * whose value count (49 per block) does not fit 32-bit indexing.  solver_stats may be NULL. */
typedef enum svgpu_pose_graph_solver { SVGPU_PG_SOLVER_PCG = 0, SVGPU_PG_SOLVER_ENVELOPE = 1 } svgpu_pose_graph_solver;
typedef struct svgpu_pose_graph_options {
    int32_t solver;       /* svgpu_pose_graph_solver */
    int32_t reserved[3];  /* must be 0 */
} svgpu_pose_graph_options;
typedef struct svgpu_pose_graph_solver_stats {
    int32_t solver;           /* the solver that ran */
    int32_t ordering;         /* envelope: 0 natural, 1 interleaved, 2 reverse Cuthill-McKee */
    int32_t envelope_blocks;  /* envelope: 7x7 blocks of the lower envelope, diagonal included */
    int32_t max_column_rows;  /* envelope: most rows below the diagonal in one block column */
    int32_t failed_solves;    /* envelope: damping trials whose factorisation met a bad pivot */
} svgpu_pose_graph_solver_stats;
int svgpu_pose_graph_optimize_ex(svgpu_ctx* ctx, int num_vertices, const double* sim3, const uint8_t* fixed, int num_edges, const int32_t* edge_v1,
                                 const int32_t* edge_v2, const double* edge_sim3_21, int fix_scale, int max_iterations, double gain_threshold,
                                 double* sim3_out, double* pose_cw_out, svgpu_pose_graph_stats* stats, const svgpu_pose_graph_options* options,
                                 svgpu_pose_graph_solver_stats* solver_stats);

/* Device self-test of the envelope solver (NOT a product entry point; the LM loop is not run): plans, assembles, factors and solves the
 * block-sparse symmetric system with 7x7 blocks {diag_blocks nfree x 49 row-major, block (pair_a[k], pair_b[k]) = pair_blocks k x 49
 * row-major and its transpose at (pair_b[k], pair_a[k]); a pair given more than once is summed} x = rhs (7 nfree).  x_out 7 nfree.
 * SVGPU_ERR_NUMERIC with failed_solves = 1 and x_out untouched when the system is not positive definite. */
int svgpu_selftest_pose_graph_envelope_solve(svgpu_ctx* ctx, int nfree, int num_pairs, const int32_t* pair_a, const int32_t* pair_b,
                                             const double* diag_blocks, const double* pair_blocks, const double* rhs, double* x_out,
                                             svgpu_pose_graph_solver_stats* solver_stats);

/* Step 5 of the same function (:284-301): pos_out = sim3_after[ref]^-1 .map( sim3_before[ref] .map(pos_w) ) for num_landmarks landmarks,
 * ref_vertex being the landmark's reference vertex.  The output feeds svgpu_landmarks_update_geometry.  SVGPU_ERR_INVALID for a
 * reference out of range; num_landmarks == 0 is a success. */
int svgpu_pose_graph_correct_landmarks(svgpu_ctx* ctx, int num_vertices, const double* sim3_before, const double* sim3_after, int num_landmarks,
                                       const int32_t* ref_vertex, const double* pos_w, double* pos_w_out);

/* ------------------------------------------------------------------------------ pairwise Sim3 optimisation (loop validation), batched
 * optimize::transform_optimizer::optimize (optimize/transform_optimizer.cc:20-158), the step module::loop_detector runs between
 * match_keyframes_mutually and its inlier threshold (module/loop_detector.cc:581), for every loop candidate of a keyframe in one call.
 * Problem p is one 7-dof vertex Sim3_12 (8 doubles as in svgpu_pose_graph_optimize) and, per match, two unary reprojection edges:
 *   forward    e12 = obs1 - project1(S12.map(R_2w pos_w_2 + t_2w))      (optimize/internal/sim3/forward_reproj_edge.h:61-76)
 *   backward   e21 = obs2 - project2(S12^-1.map(R_1w pos_w_1 + t_1w))   (backward_reproj_edge.h:61-77)
 * project is fx x / z + cx, fy y / z + cy for perspective, fisheye and radial-division keyframes (their keypoints are undistorted;
 * mutual_reproj_edge_wrapper.h:64-158) and the atan2 / asin form of forward_reproj_edge.h:110-114 for equirectangular ones; the two views may
 * differ in model.  Information = inv_sigma_sq (a float, widened) times identity, chi2 = info |e|^2, Huber of width (double)sqrtf(chi_sq) on
 * every edge in both stages (first-order weighting), g2o's numeric Jacobian (central differences, delta 1e-9, through exp(update) *
 * estimate; with fix_scale coordinate 6 of every update is zero, transform_vertex.h:61-70), Levenberg-Marquardt as
 * svgpu_pose_graph_optimize states it but without terminate_action: lambda0 = 1e-5 max diag H at iteration 0 of each stage, at most 10
 * damping trials per iteration; a stage ends at its iteration count, after 10 rejected trials, on rho == 0 or on a non-finite lambda.
 *   stage 1     5 iterations over all edges (:98-99); a match survives if chi2_12 < chi_sq && chi2_21 < chi_sq, both strict (:109).  Fewer than
 *               10 survivors (:121-123): num_inliers = 0, sim3_12_out = the input bit for bit, the rejected matches stay rejected
 *   stage 2     num_iter iterations over the survivors' edges (:127-128); a survivor is rejected if chi_sq < chi2_12 || chi_sq < chi2_21 (:143)
 *   The chi2 a gate reads is g2o's cached error of the edge: that of the stage's last evaluation, i.e. its last damping trial, accepted or
 *   not; with num_iter == 0 the second gate reads stage 1's values.
 * One persistent workgroup per problem, fp64, sums in a fixed order, no atomics: a problem's result does not depend on the rest of the
 * batch or on its position in it, and two calls are bit-equal.  Host in/out, synchronous: one upload, one launch, one read-back.
 *   view1 / view2     camera and pose of keyframe 1 (the current keyframe) and keyframe 2 (the candidate); view2 holds num_problems entries,
 *                     view1 one entry shared by all problems when view1_shared != 0, else num_problems entries
 *   match_off         num_problems + 1 offsets into the per-match arrays (match_off[0] = 0; a problem may be empty: 0 inliers, Sim3 unchanged)
 *   obs1 / obs2       2 doubles per match: the undistorted keypoints; inv_sigma_sq1 / inv_sigma_sq2: inv_level_sigma_sq of their octaves
 *   pos_w_1 / pos_w_2 3 doubles per match: the landmark of keyframe 1 / of keyframe 2, each in its keyframe's world.  Matches in
 *                     ascending idx1 order, as the reference adds its edges (:64-94)
 *   sim3_12 / sim3_12_out   num_problems x 8
 *   chi_sq / fix_scale / num_iter   of the call (transform_optimizer.h:25,41-43)
 *   num_inliers       per problem: what optimize returns
 *   status            one byte per match: SVGPU_SIM3OPT_INLIER, _REJECTED_STAGE1, _REJECTED_STAGE2
 *   stats             nullable, per problem
 * SVGPU_ERR_INVALID before anything is launched: non-monotone offsets, a quaternion whose squared norm is further than 1e-9 from 1, a
 * scale, an inv_sigma_sq or chi_sq that is not positive and finite, num_iter < 0, a camera model outside svgpu_camera_model, a null
 * required pointer.  num_problems == 0 is a success whatever the other arguments hold. */
#define SVGPU_SIM3OPT_INLIER 0
#define SVGPU_SIM3OPT_REJECTED_STAGE1 1
#define SVGPU_SIM3OPT_REJECTED_STAGE2 2
typedef struct svgpu_sim3opt_view {
    svgpu_camera cam;
    double pose_cw[12]; /* rows 0..2 of [rot_cw | trans_cw], row-major */
} svgpu_sim3opt_view;
typedef struct svgpu_sim3opt_stats {
    int32_t lm_iterations[2]; /* per stage */
    int32_t lm_trials[2];     /* damping trials per stage */
    int32_t early_return;     /* fewer than 10 matches survived stage 1 */
    int32_t num_survivors;    /* matches that survived stage 1 */
    double first_chi2[2];     /* robust chi2 at the first linearisation of the stage (0 if the stage did not run) */
    double last_chi2[2];      /* robust chi2 of the estimate when the stage ended */
    double lambda;            /* damping after the last trial */
} svgpu_sim3opt_stats;
int svgpu_sim3_transform_optimize_batch(svgpu_ctx* ctx, int num_problems, const svgpu_sim3opt_view* view1, int view1_shared,
                                        const svgpu_sim3opt_view* view2, const int32_t* match_off, const double* obs1, const double* obs2,
                                        const float* inv_sigma_sq1, const float* inv_sigma_sq2, const double* pos_w_1, const double* pos_w_2,
                                        const double* sim3_12, float chi_sq, int fix_scale, int num_iter, double* sim3_12_out,
                                        int32_t* num_inliers, uint8_t* status, svgpu_sim3opt_stats* stats);

/* One problem: the batch of one, bit for bit. */
int svgpu_sim3_transform_optimize(svgpu_ctx* ctx, const svgpu_sim3opt_view* view1, const svgpu_sim3opt_view* view2, int num_matches,
                                  const double* obs1, const double* obs2, const float* inv_sigma_sq1, const float* inv_sigma_sq2,
                                  const double* pos_w_1, const double* pos_w_2, const double* sim3_12, float chi_sq, int fix_scale, int num_iter,
                                  double* sim3_12_out, int32_t* num_inliers, uint8_t* status, svgpu_sim3opt_stats* stats);

/* bow_tree::match_frame_and_keyframe (match/bow_tree.cc:169-256) and bow_tree::match_keyframes (:258-366).
 * Side 1 = the keyframe whose landmarks are handed over (queries: valid1 = keypoint holds a live landmark), side 2 = the frame /
 * the other keyframe (valid2 nullable = every keypoint, or "holds a live landmark" for match_keyframes; occupied2 nullable = keypoints
 * that must not be matched from the start).  Device-side merge-join of the node ids as above; per pair orientation; best / second
 * best with strict '<', best <= HAMMING_DIST_THR_LOW, Lowe ratio; a side-2 keypoint is taken once.
 *   match_1to2[i]   side-2 keypoint matched to side-1 keypoint i, or -1. */
int svgpu_bow_match(svgpu_ctx* ctx, const uint8_t* desc1, const float* angle1, const uint8_t* valid1, const int32_t* node1, int n1,
                    const uint8_t* desc2, const float* angle2, const uint8_t* valid2, const int32_t* node2, int n2, const uint8_t* occupied2,
                    float lowe_ratio, int check_orientation, int32_t* match_1to2, int* num_matches);

/* The bucketed matchers for ALL partners of a loop in one call: module::relocalizer's candidates (and their covisible neighbours) against
 * the frame (module/relocalizer.cc:134-188), module::loop_detector's candidates against the current keyframe (module/loop_detector.cc:377),
 * mapping_module::create_new_landmarks' neighbours against the current keyframe (mapping_module.cc:332-335).  A view is one side of
 * svgpu_bow_match / svgpu_match_for_triangulation as host arrays.  `side1` has num_problems views, or ONE view that every problem uses
 * when side1_shared != 0 (uploaded and ordered once); side2 likewise; both may be shared only when num_problems == 1.
 *   match_1to2 / matched_2_in_1   the problems' results one after another in problem order: n1 of problem p entries each (num_problems * n1
 *                                 with a shared side 1), a side-2 keypoint index of that problem's side 2 or -1
 *   num_matches                   num_problems counts
 * Problem p's result equals, element for element, what the single entry point returns for its two sides; it depends on nothing else in
 * the batch.  A problem with n1 == 0 or n2 == 0 has no match.  num_problems == 0 succeeds and touches nothing.
 * SVGPU_ERR_INVALID, before anything is staged or launched: a null required pointer; n < 0 or n2 >= 1 << 22; node ids on one side of a
 * problem only (svgpu_bow_match_batch: missing on side 1); check_orientation without angles; for triangulation missing bearings or
 * octaves, num_levels outside 1..16, an octave outside [0, num_levels); `occupied` on a side-1 view or on any view of the triangulation
 * matcher; both sides shared with num_problems > 1; totals (rows, keypoints x 8, sum of n1 x n2) beyond int32.  Host in/out, synchronous. */
typedef struct svgpu_match_view {
    const uint8_t* desc;     /* n x 32 */
    const float* angle;      /* n; required when check_orientation */
    const uint8_t* valid;    /* nullable = all.  bow: "holds a live landmark" (side 1 always; side 2 for match_keyframes);
                                triangulation: 1 = keypoint WITHOUT a landmark (robust.cc:47-50, 66-70) */
    const int32_t* node;     /* BoW node id per keypoint, < 0 = none; null on BOTH sides of a problem = one bucket (robust::) */
    const int32_t* octave;   /* side 1, triangulation only */
    const double* bearings;  /* n x 3, triangulation only */
    const float* xright;     /* nullable, triangulation only */
    const uint8_t* occupied; /* side 2 of svgpu_bow_match_batch only, nullable: not matchable from the start */
    int n;
} svgpu_match_view;
int svgpu_bow_match_batch(svgpu_ctx* ctx, int num_problems, const svgpu_match_view* side1, int side1_shared, const svgpu_match_view* side2,
                          int side2_shared, float lowe_ratio, int check_orientation, int32_t* match_1to2, int32_t* num_matches);
/* E_12: num_problems x 9, epipole_in_2: num_problems x 3, valid_epipole: num_problems; the remaining parameters as in
 * svgpu_match_for_triangulation, shared by all problems. */
int svgpu_match_for_triangulation_batch(svgpu_ctx* ctx, int num_problems, const svgpu_match_view* side1, int side1_shared,
                                        const svgpu_match_view* side2, int side2_shared, const double* E_12, const double* epipole_in_2,
                                        const int32_t* valid_epipole, const float* scale_factors, int num_levels, float residual_rad_thr,
                                        float lowe_ratio, int check_orientation, int32_t* matched_2_in_1, int32_t* num_matches);

/* ------------------------------------------------------------------------------ landmark refresh (batched)
 * data::landmark::compute_descriptor (data/landmark.cc:199-254) for n landmarks: the representative descriptor is the
 * observation whose row of the k x k Hamming matrix has the smallest lower median (sorted index (unsigned)(0.5 (k-1)); first
 * row wins ties).  obs_off: n + 1 CSR offsets (obs_off[0] = 0, every landmark >= 1 observation, in the iteration order of the
 * reference's observations_ map with will_be_erased keyframes already dropped), obs_desc: obs_off[n] x 32 descriptor rows.
 *   best_obs[l]  index inside landmark l's list;  descriptor  n x 32. */
int svgpu_landmarks_compute_descriptor(svgpu_ctx* ctx, int n, const int32_t* obs_off, const uint8_t* obs_desc, int32_t* best_obs,
                                       uint8_t* descriptor);

/* data::landmark::update_mean_normal_and_obs_scale_variance (data/landmark.cc:256-318) for n landmarks:
 *   mean_normal = normalized( sum over observations of normalized(pos_w - keyfrm->get_trans_wc()) )   (summed in list order)
 *   max_valid_dist = |pos_w - ref_trans_wc| * ref_scale_factor ;  min_valid_dist = max_valid_dist * inv_scale_factor_last
 * obs_trans_wc: obs_off[n] x 3 doubles (camera centre of each observing keyframe); ref_trans_wc n x 3 (the landmark's reference
 * keyframe); ref_scale_factor[l] = scale_factors_[octave of its keypoint there]; inv_scale_factor_last =
 * inv_scale_factors_[num_levels - 1]. */
int svgpu_landmarks_update_geometry(svgpu_ctx* ctx, int n, const int32_t* obs_off, const double* obs_trans_wc, const double* pos_w,
                                    const double* ref_trans_wc, const float* ref_scale_factor, float inv_scale_factor_last,
                                    double* mean_normal, float* max_valid_dist, float* min_valid_dist);

/* ------------------------------------------------------------------------------ BoW transform (tree descent)
 * data::bow_vocabulary_util::compute_bow (data/bow_vocabulary.cc:18-24): per descriptor, descend the vocabulary tree choosing the
 * child with the smallest Hamming distance (first child wins ties) down to a leaf; word_id / weight = the leaf's, node_id = the
 * node passed at depth `node_level` (DBoW2's transform(.., levelsup = 4) records depth L - levelsup, clamped at 0 = root; the
 * bucket key of match::bow_tree).  The binding accumulates bow_vec (word -> weight, then the vocabulary's normalisation) and
 * bow_feat_vec (node -> feature indices in order) from these arrays.
 * Flat tree: node 0 = root, children of node i = children[child_off[i] .. child_off[i+1]) (none => leaf), ids strictly > 0;
 * node_desc n_nodes x 32, node_weight / word_id per node.  The vocabulary stays resident on ctx's device until freed. */
typedef struct svgpu_vocabulary svgpu_vocabulary;
int svgpu_bow_vocabulary_upload(svgpu_ctx* ctx, int n_nodes, const int32_t* child_off, const int32_t* children, const uint8_t* node_desc,
                                const float* node_weight, const int32_t* word_id, svgpu_vocabulary** out);
void svgpu_bow_vocabulary_free(svgpu_vocabulary* vocab);
int svgpu_bow_transform(svgpu_ctx* ctx, const svgpu_vocabulary* vocab, const uint8_t* desc, int n, int node_level, int32_t* word_id,
                        float* weight, int32_t* node_id);
/* The reference's DEFAULT BoW build: fbow::Vocabulary::transform(features, level = 4, bow_vec, bow_feat_vec) (data/bow_vocabulary.cc:20-22; FBoW =
 * stella-cv/FBoW, restated from its published sources -- the submodule is empty in the reference checkout, so parity is unpinned).  Same
 * descent; differences to the DBoW2 form above: `store_level` counts DOWN from the root (DBoW2's levelsup counts up from the leaves), the
 * bow_feat_vec key is FBoW's PATH CODE of the node ((code << ceil(log2 k)) | child index per level), and a leaf met above the store level
 * files its feature under the code of the block it was found in.  k = the vocabulary's branching factor. */
int svgpu_fbow_transform(svgpu_ctx* ctx, const svgpu_vocabulary* vocab, const uint8_t* desc, int n, int store_level, int k,
                         int32_t* word_id, float* weight, uint32_t* node_code);
/* The WHOLE of compute_bow for num_frames descriptor sets in one call: the descent above and, built on the device, the two sparse maps of
 * every frame as flat arrays in the iteration order of the reference's std::map.  Frame f is rows d_off[f] .. d_off[f + 1] of desc
 * (d_off[0] = 0, offsets must not descend, empty frames anywhere).
 *   form   SVGPU_BOW_FORM_DBOW2: `level` = node_level of svgpu_bow_transform (k ignored); features whose weight is not > 0 take part in
 *          neither map; norm = the sum of fabs(v); if norm > 0 every weight is DIVIDED by it
 *          SVGPU_BOW_FORM_FBOW:  `level` = store_level, k as in svgpu_fbow_transform (2 .. 65536); every feature takes part; norm = the sum of
 *          v * v (the product rounded before the add); if norm > 0 every weight is MULTIPLIED by 1.0 / sqrt(norm), the reciprocal formed first
 *   word_id, weight, node (nullable): d_off[B] entries, equal to the single calls on the same rows
 *   vec_off (B + 1), vec_word / vec_weight: bow_vec of frame f at vec_off[f] .. vec_off[f + 1], word ids strictly ascending -- the form
 *          svgpu_bowdb_add and svgpu_bowdb_acquire* take.  A word's weight is 0.0 + (double)weight[i0] + (double)weight[i1] + ... over its
 *          features in ascending index; the norm adds the words one after another in ascending id.  No tree or wave reduction and no
 *          floating-point atomic anywhere: the results equal data::bow_vocabulary_hip::compute_bow (host/camera.cpp) bit for bit.
 *          (The Python bow_vocabulary.transform divides the FBoW form by sqrt(norm) instead, which differs in the last bit: this call
 *          follows the C++ class.)
 *   feat_off (B + 1), feat_key / feat_index: bow_feat_vec of frame f, entries in ascending key (node id, or FBoW path code), inside a key in
 *          ascending feature index (an index inside its frame)
 *   vec_* and feat_* arrays hold d_off[B] entries each (no frame has more words or kept features than descriptors); vec_off[B] and
 *          feat_off[B] of them are written.
 *   db (nullable) with slots (B): the B vectors are also appended to the database's pools, device to device and under its mutex, as
 *          svgpu_bowdb_add_batch would append the returned vectors; slots as that call returns them.
 * A frame of at most svgpu_bow_compute_lds_capacity() descriptors is ordered by one workgroup; longer ones take the radix sort, with the
 * same results.  While every frame fits, the launches do not depend on B (they do on whether d_off[B] exceeds one scan tile of 16384).
 * One synchronisation, two with a database (the B + 1 vector offsets come back first; a pool growth adds its own).  `stats` (nullable)
 * receives what the call issued.  SVGPU_ERR_INVALID before anything is launched or written: a null required pointer, d_off[0] != 0 or
 * descending offsets, num_frames < 0, level < 0, k out of range, an unknown form, d_off[B] > 1 << 26, a vocabulary or database of another
 * device.  num_frames == 0 succeeds.  Host in/out, synchronous.  FBoW / DBoW2 parity stays unpinned, as above. */
#define SVGPU_BOW_FORM_DBOW2 0
#define SVGPU_BOW_FORM_FBOW 1
struct svgpu_call_stats;
struct svgpu_bowdb;
int svgpu_bow_compute_batch(svgpu_ctx* ctx, const svgpu_vocabulary* vocab, int form, int level, int k, int num_frames, const int32_t* d_off,
                            const uint8_t* desc, int32_t* word_id, float* weight, uint32_t* node, int32_t* vec_off, uint32_t* vec_word,
                            double* vec_weight, int32_t* feat_off, uint32_t* feat_key, int32_t* feat_index, struct svgpu_bowdb* db, int32_t* slots,
                            struct svgpu_call_stats* stats);
int svgpu_bow_compute_lds_capacity(void);

/* ------------------------------------------------------------------------------ keyframe BoW database
 * data::bow_database (data/bow_database.h:20-100, data/bow_database.cc:21-159): the candidates of module::relocalizer::relocalize
 * (module/relocalizer.cc:58) and module::loop_detector::detect_loop_candidates (module/loop_detector.cc:83-129), resident on the device.
 * A BoW vector is n_words (word id, weight) pairs with STRICTLY ascending ids (the iteration order of the reference's std::map), weights
 * as doubles (what compute_bow hands out).  The database keeps a forward index -- per keyframe its ids and weights in two pools, and a slot
 * table -- and scans it per query; the reference's inverted index keyfrms_in_node_ has no device counterpart, by design.
 * acquire (data/bow_database.cc:58-96), per query:
 *   1. common = shared word ids with every live keyframe that is not rejected (compute_num_common_words, :98-129); keyframes with
 *      common == 0 do not exist for the rest of the query; none at all: empty result, max_common = 0
 *   2. max_common = the largest count (:72-77); thr = (unsigned)(ratio * max_common), a float product truncated (:78)
 *   3. survivors: thr < common, strict (:143); each is scored; dropped iff min_score > score (:147), a score equal to min_score stays
 *   4. the kept keyframes in ASCENDING SLOT order (the reference returns them in unordered_set order, which is unspecified), each with its
 *      common and score
 * score(query, keyframe) (data/bow_vocabulary.cc:9-16), chosen at creation like the build switch USE_DBOW2; v = the query's weight of a
 * shared word, w = the keyframe's, shared words added one after another in ascending word order:
 *   SVGPU_BOW_SCORE_FBOW_L2   the DEFAULT build, fbow::BoWVector::score: weights rounded to float, s += (double)(v * w) with the product
 *                             in fp32; score = s >= 1 ? 1 : 1 - sqrt(1 - s) in fp64, returned as float
 *   SVGPU_BOW_SCORE_DBOW2_L1  USE_DBOW2, DBoW2's L1Scoring::score: s += fabs(v - w) - fabs(v) - fabs(w) in fp64; score = -s / 2 as float
 * Both forms are restated from the libraries' published sources (neither is in the reference checkout): parity unpinned.
 * Against a sequential host loop of these definitions the counts, the candidate lists and the scores are equal bit for bit.
 * Every call is synchronous (one synchronisation at its end); calls on one database are serialised by a mutex, as bow_database::mtx_ does. */
#define SVGPU_BOW_SCORE_FBOW_L2 0
#define SVGPU_BOW_SCORE_DBOW2_L1 1
typedef struct svgpu_bowdb svgpu_bowdb;
int svgpu_bowdb_create(svgpu_ctx* ctx, int score_form, svgpu_bowdb** db);
void svgpu_bowdb_destroy(svgpu_bowdb* db);
/* bow_database::clear (data/bow_database.cc:52-56): every keyframe gone, slot numbers start again at 0 (the allocations are kept) */
int svgpu_bowdb_clear(svgpu_ctx* ctx, svgpu_bowdb* db);
/* bow_database::add_keyframe (data/bow_database.cc:21-28).  *slot: the keyframe's number; slots are handed out in increasing order and not
 * reused before clear, so ascending slot order is insertion order.  Ids that do not ascend strictly: SVGPU_ERR_INVALID. */
int svgpu_bowdb_add(svgpu_ctx* ctx, svgpu_bowdb* db, int n_words, const uint32_t* words, const double* weights, int32_t* slot);
/* num_frames svgpu_bowdb_add calls as one submission (a loaded map registering every keyframe): vector f is entries off[f] .. off[f + 1] of
 * words / weights (off[0] = 0); slots (num_frames) are handed out in order.  One pool growth check, one upload per pool span and one of
 * the new slot records.  Afterwards slot numbers, svgpu_bowdb_size, pool capacity and fill, and every later acquire, score, erase and
 * compaction are those after the single adds (num_growths counts one growth where the single adds may have doubled several times).  If
 * the ids of ANY frame do not ascend strictly: SVGPU_ERR_INVALID and the database is untouched. */
int svgpu_bowdb_add_batch(svgpu_ctx* ctx, svgpu_bowdb* db, int num_frames, const int32_t* off, const uint32_t* words, const double* weights,
                          int32_t* slots);
/* bow_database::erase_keyframe (data/bow_database.cc:30-50); an erased or unknown slot is ignored, as the reference ignores a keyframe it
 * does not hold.  Erased spans of the pools are reclaimed by a compaction once they exceed half of what the pools hold. */
int svgpu_bowdb_erase(svgpu_ctx* ctx, svgpu_bowdb* db, int32_t slot);
int svgpu_bowdb_size(svgpu_bowdb* db, int* live_keyframes, long long* live_entries);
/* slots handed out since the last clear, pool capacity / fill in entries, pool growths and compactions since creation (all nullable) */
int svgpu_bowdb_diagnostics(svgpu_bowdb* db, long long* num_slots, long long* pool_capacity, long long* pool_used, long long* num_growths,
                            long long* num_compactions);
/* word ids of a query a workgroup holds in LDS at a time; a longer query is processed in chunks, with the same results */
int svgpu_bowdb_query_stage_capacity(void);
/* bow_database::acquire_keyframes (data/bow_database.cc:58-96).  reject_slots: keyfrms_to_reject as slot numbers (unknown or erased ones
 * are ignored).  out_*: `cap` entries each; when more than cap keyframes pass, the first cap in slot order are written and *n_out is the
 * full count.  max_common: nullable. */
int svgpu_bowdb_acquire(svgpu_ctx* ctx, svgpu_bowdb* db, int n_words, const uint32_t* words, const double* weights, float min_score, float ratio,
                        int n_reject, const int32_t* reject_slots, int cap, int32_t* out_slots, uint32_t* out_common, float* out_score, int32_t* n_out,
                        uint32_t* max_common);
/* num_queries queries in one submission (a batch of lost frames; an offline loop search of a whole map): query q is entries
 * q_off[q] .. q_off[q + 1] of words / weights (q_off[0] = 0) with its own min_score[q]; ratio and the reject list are shared; results of
 * query q at q * cap, n_out / max_common per query.  Every query's outputs equal the single call's bit for bit. */
int svgpu_bowdb_acquire_batch(svgpu_ctx* ctx, svgpu_bowdb* db, int num_queries, const int32_t* q_off, const uint32_t* words, const double* weights,
                              const float* min_score, float ratio, int n_reject, const int32_t* reject_slots, int cap, int32_t* out_slots,
                              uint32_t* out_common, float* out_score, int32_t* n_out, uint32_t* max_common);
/* The score of the query against each of n listed slots, whatever they share (loop_detector::compute_min_score_in_covisibilities,
 * module/loop_detector.cc:278-297); an erased or unknown slot gives -1. */
int svgpu_bowdb_score(svgpu_ctx* ctx, svgpu_bowdb* db, int n_words, const uint32_t* words, const double* weights, int n, const int32_t* slots,
                      float* out_score);

/* match::stereo::compute (match/stereo.cc:20-114): for every left keypoint the closest right keypoint in its row band
 * (rows +-2*scale, octave +-1, disparity in [0, focal_x_baseline / true_baseline], Hamming < 75), then the 11x11 L1 patch
 * slide (+-5 px) on the keypoint's pyramid level with parabolic sub-pixel refinement, finally the 2x-median correlation
 * filter.  The two pyramids are those of the LAST extract call on ctx_left / ctx_right (both contexts on one device;
 * the reference reads extractor_left_->image_pyramid_ / extractor_right_->image_pyramid_, system.cc:443-447).
 * stereo_x_right / depths: n_left floats, -1 where no match.  Host in/out, synchronous. */
int svgpu_stereo_match(svgpu_ctx* ctx_left, svgpu_ctx* ctx_right, const svgpu_keypoint* kps_left, const uint8_t* desc_left,
                       int n_left, const svgpu_keypoint* kps_right, const uint8_t* desc_right, int n_right,
                       float focal_x_baseline, float true_baseline, float* stereo_x_right, float* depths);

/* The same for `pairs` stereo pairs at once, everything resident in HBM (BASELINE config 4: KITTI stereo batches): the keypoints /
 * descriptors / counts are the outputs of svgpu_orb_extract_batch_device on ctx_left and ctx_right (pair p at p * cap records,
 * count at n_*_dev[p * n_stride]), the pyramids those calls left in the two contexts.  The 2 x median correlation filter runs on the
 * device as well (rank-size/2 value by bisection).  stereo_x_right_dev / depths_dev: pairs * cap floats (-1 = no match).
 * Only the first min(n_left, cap) entries of a pair are written; the entries behind a pair's left count keep what the buffers held.
 * Asynchronous on `stream` (NULL = ctx_left's); the caller orders it behind both extractions. */
int svgpu_stereo_match_batch_device(svgpu_ctx* ctx_left, svgpu_ctx* ctx_right, int pairs, const svgpu_keypoint* kps_left_dev, const uint8_t* desc_left_dev,
                                    const int32_t* n_left_dev, const svgpu_keypoint* kps_right_dev, const uint8_t* desc_right_dev,
                                    const int32_t* n_right_dev, int cap, int n_stride, float focal_x_baseline, float true_baseline,
                                    float* stereo_x_right_dev, float* depths_dev, void* stream);

/* ------------------------------------------------------------------------------------------------ local BA
 * Stands behind  stella_vslam::optimize::local_bundle_adjuster::optimize(map_db, curr_keyfrm, force_stop_flag)
 * (optimize/local_bundle_adjuster.h:23; g2o implementation optimize/local_bundle_adjuster_g2o.cc:36-431).
 * The adaptor performs steps 1 (gather) and 7-8 (outlier list, write-back under mtx_database_) on the
 * host exactly as the g2o/gtsam backends do and hands steps 2-6 to this call.
 */
typedef struct svgpu_ba_problem {
    int32_t num_poses;               /* local + fixed keyframes */
    int32_t num_points;              /* local landmarks (+ marker corners) */
    int32_t num_obs;                 /* reprojection edges */
    const double* pose_cw;           /* num_poses x 12: rows of [R|t] (3x4, row-major), world -> camera */
    const uint8_t* pose_fixed;       /* num_poses: 1 = fixed keyframe vertex */
    const double* points;            /* num_points x 3 */
    const uint8_t* point_fixed;      /* nullable num_points: 1 = fixed vertex (kept-fixed marker corners) */
    const int32_t* obs_pose;         /* num_obs */
    const int32_t* obs_point;        /* num_obs */
    const float* obs_uvr;            /* num_obs x 3: undistorted u, v, u_right (< 0 => monocular edge) */
    const float* obs_inv_sigma_sq;   /* num_obs: orb_params::inv_level_sigma_sq_[octave] */
    const float* obs_huber_delta;    /* num_obs: sqrt(chi_sq) of the Huber kernel, <= 0 => no kernel; < 0 => a marker-corner edge (no kernel, and
                                      * outside the chi-square / depth gate and the outlier list: local_bundle_adjuster_g2o.cc:246-304) */
    const double* intrinsics;        /* num_poses x 5: fx fy cx cy focal_x_baseline (perspective / fisheye / radial-division cameras:
                                        all use the perspective edge on undistorted keypoints, reproj_edge_wrapper.h:64-201);
                                        {0, 0, cols, rows, 0} selects the equirectangular edge (equirectangular_reproj_edge.h:64-134,
                                        monocular only, no depth gate) */
    int32_t num_first_iter;          /* 5  (local_bundle_adjuster_factory.h) */
    int32_t num_second_iter;         /* 10 */
    double gain_threshold;           /* terminate_action gain, 1e-3 */
} svgpu_ba_problem;

typedef struct svgpu_ba_stats {
    double chi2_initial, chi2_final;
    int32_t iters_stage1, iters_stage2, stage2_entered, num_gated;
    int32_t lm_trials, cholesky_failures;
    double lambda_final;
    int32_t stopped_by_terminate_action; /* the gain rule (not the caller) raised the stop flag (global_bundle_adjuster.cc:341) */
    int32_t pcg_iterations;              /* total PCG iterations over all damping trials (0 with the Cholesky solvers) */
} svgpu_ba_stats;

/* Linear solver of the reduced camera system (BlockSolver_6_3 + LinearSolverEigen / LinearSolverCSparse in the reference,
 * optimize/local_bundle_adjuster_g2o.cc:151-164, optimize/global_bundle_adjuster.cc:66-85):
 *   AUTO      dense LL^T in one workgroup's LDS while it fits (6 * free poses <= ~135), the LDS-resident PCG while THAT fits, the
 *             block envelope Cholesky beyond (the one-launch-per-iteration PCG only when the envelope is too large)
 *   PCG       block-Jacobi PCG on the block-sparse Schur complement: inside ONE workgroup (blocks, block rows, vectors all in
 *             its LDS) while the kept 6x6 blocks fit ~150 KB and 6 * free poses <= 512, else one kernel launch per iteration
 *   CHOLESKY  the LDS LL^T (larger systems fall back to PCG): the register-tile LDL^T with 3x3 pivots
 *   CHOLESKY_MFMA  the same system by a blocked right-looking LL^T, 16-column panels, the trailing update on v_mfma_f64_16x16x4_f64
 *             (DESIGN section 5 has the measured comparison of the two)
 *   DENSE     dense image in global memory + the library's own one-workgroup LL^T (no vendor solver is loaded anywhere)
 *   ENVELOPE  direct block envelope (skyline) LL^T after a reverse Cuthill-McKee ordering of the keyframe graph -- what AUTO takes beyond
 *             the on-chip solvers while the envelope stays under 256 MB (the reference factors this system with a sparse Cholesky)
 * pcg_tolerance: relative residual |r| / |g| (<= 0: 1e-10); pcg_max_iterations <= 0: max(2000, 4 n).  A solve that hits the
 * cap is taken as an inexact step when the residual fell below 1e-6, else the damping trial counts as a solver failure. */
typedef enum svgpu_ba_solver {
    SVGPU_BA_SOLVER_AUTO = 0,
    SVGPU_BA_SOLVER_CHOLESKY = 1,
    SVGPU_BA_SOLVER_PCG = 2,
    SVGPU_BA_SOLVER_DENSE = 3,
    SVGPU_BA_SOLVER_PCG_MULTI = 4, /* PCG with one kernel launch per iteration even when the system would fit one workgroup's LDS */
    SVGPU_BA_SOLVER_CHOLESKY_MFMA = 7, /* CHOLESKY with the blocked LL^T whose trailing updates run on the matrix cores (up to 126 unknowns; the register-tile form beyond) */
    SVGPU_BA_SOLVER_ENVELOPE = 6   /* block envelope Cholesky at any size (falls back to the PCG when the envelope of the ordered block graph exceeds 256 MB) */
} svgpu_ba_solver;
int svgpu_ba_set_solver(svgpu_ctx* ctx, int solver, double pcg_tolerance, int pcg_max_iterations);

/* How the context's last envelope factorisation was planned (diagnostics for tests / bench.py): info[8] = {0 one-sided | 1 two-sided |
 * 2 segmented, block rows, widest column; segmented: cuts, jobs, jobs on this rank, separator rows, longest job (columns)}. */
int svgpu_ba_last_envelope_plan(svgpu_ctx* ctx, int* info);

/* Which solver factored the reduced system in the last stage of the context's last bundle adjustment (diagnostics for tests): *solver =
 * the svgpu_ba_solver value AUTO or the request resolved to -- CHOLESKY (both on-chip forms), DENSE, PCG_MULTI, ENVELOPE -- or 5, the PCG
 * inside one workgroup's LDS; -1 before the first call. */
int svgpu_ba_last_solver(svgpu_ctx* ctx, int* solver);

/* Planner self-test of the segmented envelope factorisation (host arithmetic only, runs without a device; NOT a solver path: the
 * bundle adjusters never call it).  Plans the elimination of the 6x6-block SPD system {blk_ab[NB] upper blocks a <= b, Sblk NB x 36
 * row-major, g 6 nP} exactly as the global / sharded bundle adjusters do (RCM order, `cuts` separators or the planner's choice when
 * <= 0, jobs spread over `world` ranks), walks the same plan arrays and maps the kernels walk and returns the solution x.
 * info[8] = {segmented, cuts, jobs, separator rows, longest job, separator banded, widest job column, widest column of the unsegmented
 * envelope}.  Returns 0, 1 = the system is not segmented (too short / not banded), 2 = not positive definite, < 0 = bad arguments. */
int svgpu_selftest_segmented_solve(int nP, int NB, const int* blk_ab, const double* Sblk, const double* g, int cuts, int world,
                                   double* x, int* info);

/* The same walk for ONE RANK of the distributed factorisation (tests/test_distributed_cpu.py drives it over gloo): the rank eliminates only
 * the jobs it owns; `allreduce(user, host_buf, count, NULL)` sums a HOST buffer of doubles in place across the ranks (the exchange of the
 * separator contributions and of the solution, as in the sharded bundle adjusters).  Every rank returns the single-rank solution, bit for
 * bit; info[5] = jobs this rank eliminated.  allreduce == NULL: svgpu_selftest_segmented_solve. */
int svgpu_selftest_segmented_solve_rank(int nP, int NB, const int* blk_ab, const double* Sblk, const double* g, int cuts, int rank, int world,
                                        int (*allreduce)(void* user, double* buf, size_t count, void* stream), void* allreduce_user, double* x,
                                        int* info);

/* Device self-test of the hand-written scan and radix sort the BA structure builder and the BoW merge-join run on (csrc/sv_sort.hip; NOT a
 * product entry point).  values[n] >= 0 are scanned in place semantics: scan_out[n + 1] receives the exclusive prefix sums and the total
 * (n above 16384 takes the many-workgroup path).  keys[n] (low `bits` bits significant) are sorted stably: sorted_idx[n] receives the
 * permutation.  Either half is skipped when its output pointer is NULL.  Host in / out, synchronous. */
int svgpu_selftest_scan_sort(svgpu_ctx* ctx, int n, const int32_t* values, int32_t* scan_out, const uint32_t* keys, int bits, int32_t* sorted_idx);
/* The same scan without scratch, as the grid and bucket candidate lists call it: ONE launch of one workgroup that walks tiles of 16384
 * elements, whatever n >= 0.  scan_out[n + 1].  Host in / out, synchronous. */
int svgpu_selftest_scan_one_launch(svgpu_ctx* ctx, int n, const int32_t* values, int32_t* scan_out);

/* Device self-test of the sort paths the entry above does not reach (csrc/sv_sort.hip, sv_bucket_sort of csrc/bucket_kernels.hip; NOT a
 * product entry point).  Host in / out, synchronous; arguments a path does not name are ignored.  info: 4 ints.
 *   SVGPU_SORT_PATH_RADIX_COUNT  sv_sort_pairs with the element count read ON THE DEVICE: keys[n] / idx[n] are the pairs (the 64-bit value
 *                        of pair i is idx[i] with its complement in the high word), the launches are sized for n, `count` (0 .. n) is
 *                        uploaded, the data starts in buffer set `start` (0 | 1).  keys_out / idx_out [count] = the sorted prefix, taken
 *                        from the set the function returned; info[0] = that set, info[1] = 1 when every value came back whole.
 *   SVGPU_SORT_PATH_SMALL        sv_sort_small on keys[n], idx[n] (any indices, 0 <= n <= 16384): keys_out / idx_out [n], info[0] = its bool.
 *   SVGPU_SORT_PATH_SIDES        sv_sort_small_sides, ONE launch over n sides: sides[2 u] = keypoints of side u, sides[2 u + 1] != 0 when it
 *                        has node ids; node = all sides' node ids one after another (a side without ids still occupies its stretch),
 *                        keys_out / idx_out likewise.  Both outputs are filled with the byte 0xA5 before the launch: a side the
 *                        launch skips keeps 0xA5A5A5A5.  info[0] = its bool, info[1] = the max_n passed (largest side <= 16384).
 *   SVGPU_SORT_PATH_BUCKET       sv_bucket_sort on node[n] (or node == NULL: identity), scratch from sv_bucket_sort_bytes(n):
 *                        keys_out / idx_out [n]; info[0] = 1 when n is beyond the one-workgroup sort (the radix fallback ran). */
#define SVGPU_SORT_PATH_RADIX_COUNT 0
#define SVGPU_SORT_PATH_SMALL 1
#define SVGPU_SORT_PATH_SIDES 2
#define SVGPU_SORT_PATH_BUCKET 3
int svgpu_selftest_sort_paths(svgpu_ctx* ctx, int path, int n, int count, int start, int bits, const uint32_t* keys, const int32_t* idx,
                              const int32_t* node, const int32_t* sides, uint32_t* keys_out, int32_t* idx_out, int32_t* info);

/* Which form the replay of the candidate matcher takes for nq queries and nt targets (csrc/match_kernels.hip; NOT a product entry point:
 * the launch code calls the same function, tests assert with it that a problem reaches the form it was built for).  Host only, needs
 * no context and no device.  with_cnt != 0: the lists carry explicit counts (the tracked-frame chain).
 *   modes BEST_ONLY .. TRIANGULATION: K >= 0 = tables in LDS with K staged entries per list, -1 = tables in global memory
 *   mode AREA: 1 = state in LDS, 0 = state in global memory.                                  -2 = bad arguments */
int svgpu_selftest_cand_replay_form(int nq, int nt, int with_cnt, int mode);

/* Host in/out, synchronous.  The Levenberg-Marquardt loop (damping trials, rho test, terminate_action) runs on the device; the
 * host enqueues the trials of a stage and reads the control block back once per stage (plus once per rejected trial).
 *   stop        nullable; the caller's force_stop_flag (mapping_module.h:232).  Polled at every damping-trial boundary
 *               (mirrored into page-locked memory while the host waits) and -- reference quirk, terminate_action.cc:36-76 --
 *               SET when the gain rule stops stage 1, so that stage 2 is skipped exactly as in the reference.
 *   pose_out    num_poses x 12, points_out num_points x 3, outlier_out num_obs (1 = outlier observation)
 * Limits: num_obs < 2^32 / 144 (29.8 M) and num_points < 2^32 / 48 per call -- per RANK of the sharded variants --: the record gathers of the
 * reduced-system kernel address their arrays with 32-bit byte offsets; beyond, SVGPU_ERR_INVALID (shard the landmarks over more ranks). */
int svgpu_local_ba(svgpu_ctx* ctx, const svgpu_ba_problem* problem, volatile uint8_t* stop, double* pose_out,
                   double* points_out, uint8_t* outlier_out, svgpu_ba_stats* stats);

/* ------------------------------------------------------------------------------------------------ pose optimizer
 * Stands behind  stella_vslam::optimize::pose_optimizer::optimize  (optimize/pose_optimizer.h; g2o implementation
 * optimize/pose_optimizer_g2o.cc:38-175; factory defaults 2 / 2 / 10, optimize/pose_optimizer_factory.h:18-26): motion-only
 * BA of one frame against its n observed landmarks -- (num_trials_robust + num_trials) rounds of <= num_each_iter LM
 * iterations, each followed by the chi-square (5.99146 / 7.81473) re-classification of every observation; Huber kernels
 * are dropped after round num_trials_robust.  Fewer than 5 observations => *num_valid = 0 and the pose is returned unchanged.
 *   pose_cw / pose_out   3x4 [R|t] row-major; pos_w n x 3; uvr n x 3 f32 (u_right < 0 => monocular edge)
 *   huber_delta          per observation (sqrt(5.99146) for monocular cameras else sqrt(7.81473)); <= 0 => no kernel
 *   reset_stop_flag_each_round  0 = literal g2o behaviour (the terminate action's flag, once raised by the gain rule, also
 *                        suppresses the LM iterations of the later rounds); 1 = reset it before every round
 * The whole optimisation is ONE single-workgroup kernel launch.  Host in/out, synchronous. */
int svgpu_pose_optimize(svgpu_ctx* ctx, const double* pose_cw, int n, const double* pos_w, const float* uvr,
                        const float* inv_sigma_sq, const float* huber_delta, const double* intrinsics /* fx fy cx cy fxb, or 0 0 cols rows 0 = equirectangular */,
                        int num_trials_robust, int num_trials, int num_each_iter, int reset_stop_flag_each_round,
                        double* pose_out, uint8_t* outlier_flags, int* num_valid, int* lm_iterations);

/* Same with the observations already on the context's device (pos_w_dev n x 3 f64, uvr_dev n x 3 f32, inv_sigma_sq_dev / huber_delta_dev n
 * f32), e.g. the gathered landmarks a projection matcher just worked on: no input copy; pose, intrinsics and the results stay host-side. */
int svgpu_pose_optimize_device(svgpu_ctx* ctx, const double* pose_cw, int n, const double* pos_w_dev, const float* uvr_dev,
                               const float* inv_sigma_sq_dev, const float* huber_delta_dev, const double* intrinsics, int num_trials_robust,
                               int num_trials, int num_each_iter, int reset_stop_flag_each_round, double* pose_out,
                               uint8_t* outlier_flags, int* num_valid, int* lm_iterations);

/* The same for several problems over ONE frame observation -- the candidates of relocalizer::reloc_by_candidates or
 * loop_detector::select_loop_candidate_via_Sim3 right behind svgpu_pnp_ransac_batch -- in one call: one upload, one launch (one workgroup
 * per problem), one read-back, one synchronisation.  Problem p is the entries obs_off[p] .. obs_off[p + 1] (obs_off[0] = 0; a problem may
 * be empty) of pos_w / uvr / inv_sigma_sq / huber_delta whose `select` byte is non-zero (select null: all of them), in entry order; the
 * device compacts them.  is_inlier, valid and pose_cw of svgpu_pnp_ransac_batch are a valid select, active and pose_cw (match_off = obs_off
 * when the match arrays are the same).  A problem with active[p] == 0 or fewer than 5 selected entries is skipped: num_valid 0,
 * lm_iterations 0, pose_out = its pose_cw, flags 0.  outlier_flags holds one byte per ENTRY, 0 for an unselected one (a keypoint without a
 * landmark).  Every problem's pose, flags, count and iteration count are bit for bit what svgpu_pose_optimize returns for its selected
 * entries, whatever else the batch holds.  The intrinsics are the current frame's and shared.  num_problems == 0 succeeds whatever else is
 * passed; lm_iterations may be null.  Host in/out, synchronous. */
int svgpu_pose_optimize_batch(svgpu_ctx* ctx, int num_problems, const int32_t* obs_off,
                              const double* pose_cw,      /* num_problems x 12 */
                              const uint8_t* active,      /* nullable, num_problems */
                              const double* pos_w, const float* uvr, const float* inv_sigma_sq, const float* huber_delta,
                              const uint8_t* select,      /* nullable, one byte per entry */
                              const double* intrinsics,   /* shared: the current (key)frame's camera, as svgpu_pose_optimize */
                              int num_trials_robust, int num_trials, int num_each_iter, int reset_stop_flag_each_round,
                              double* pose_out, uint8_t* outlier_flags, int32_t* num_valid, int32_t* lm_iterations);

/* module::relocalizer::refine_pose (module/relocalizer.cc:236-297) for ALL candidates that survived optimize_pose, in one call: per
 * candidate a chain of num_stages x (projection match of the candidate keyframe's landmarks into the frame from the current pose ->
 * count test -> pose optimisation over every keypoint that holds a landmark); the pose, the new matches and the landmark bookkeeping
 * move from step to step on the device.  The frame (keypoints, descriptors, grid) is uploaded and binned once and shared.
 *   frame (shared)       cam, tdesc / t_xy / t_octave / t_angle / nt / grid as svgpu_match_frame_and_keyframe_projection; t_xright
 *                        nullable (null = monocular camera: every edge monocular, Huber delta sqrt(5.99146); else the edge of keypoint t
 *                        is stereo where t_xright[t] >= 0 and the delta is sqrt(7.81473), pose_optimizer_g2o.cc:86-109);
 *                        inv_level_sigma_sq by octave; intrinsics and the trial counts as svgpu_pose_optimize_batch
 *   per candidate p      active[p] (nullable = all); pose_cw[p] 12 doubles (the pose after relocalizer::optimize_pose);
 *                        n_already_found[p] = already_found_landmarks.size(); frame_has_lm (K x nt bytes) and frame_lm_pos_w
 *                        (K x nt x 3) = the frame's landmarks after optimize_pose's outlier rejection; the keyframe's landmark entries
 *                        kf_off[p] .. kf_off[p + 1] of pos_w / valid / min_valid_dist / max_valid_dist / lm_desc / angle_kf with the
 *                        meaning of the single call (valid = 0: null, will_be_erased or in already_found_landmarks; null = all valid)
 *   stages               num_stages in 1..4, margin[s] and hamm_dist_thr[s] per stage (the relocaliser: {10, 3}, {100, 64}),
 *                        min_num_valid_obs (50)
 * Per candidate, with count = n_already_found, occupied = frame_has_lm, pose = pose_cw[p], for every stage s:
 *   1. the single call's projection match of the still-valid entries from `pose` against the keypoints that are not occupied ->
 *      num_found[p][s]; a matched entry is invalid for later stages, its keypoint becomes occupied and takes the entry's pos_w;
 *   2. count + num_found[p][s] < min_num_valid_obs: status 1 + s, the candidate stops;
 *   3. svgpu_pose_optimize over every keypoint that holds a landmark, in keypoint-index order -> pose, num_valid[p][s] = count
 *      (outliers are NOT removed between stages);
 *   after the last stage: count < min_num_valid_obs: status 1 + num_stages.
 * Outputs: status (0 accepted, -1 inactive on input), pose_out (the pose of the last optimisation that ran; the input bit for bit if none
 * ran), match_kf / match_stage per keyframe entry (frame keypoint and the stage that matched it, or -1), outlier (K x nt: the flags of
 * the last optimisation that ran; 0 where the keypoint holds no landmark), num_found / num_valid (K x num_stages, 0 for a stage that was
 * not reached), lm_iterations (K, of the last optimisation that ran; nullable).  Every output equals, bit for bit, the same chain made of
 * svgpu_match_frame_and_keyframe_projection and svgpu_pose_optimize calls for that candidate alone.
 * `stats` (nullable) receives what the call issued; none of the three depends on num_candidates.  One synchronisation per stage (the
 * stage's candidate-list total) and one at the end; a call whose lists outgrow their capacity starts again with longer ones.
 * SVGPU_ERR_INVALID before anything is launched or written: a null required pointer, kf_off[0] != 0 or non-monotone offsets, an octave
 * outside [0, num_levels), num_stages outside 1..4, num_levels outside 1..16, nt >= 1 << 22, totals beyond int32.  num_candidates == 0
 * succeeds whatever else is passed.  Host in/out, synchronous. */
typedef struct svgpu_call_stats {
    int32_t launches;          /* kernel launches */
    int32_t copies;            /* runtime copies and memsets */
    int32_t synchronisations;  /* stream synchronisations */
} svgpu_call_stats;
int svgpu_reloc_refine_batch(svgpu_ctx* ctx, const svgpu_camera* cam, const uint8_t* tdesc, const float* t_xy, const int32_t* t_octave,
                             const float* t_angle, const float* t_xright, int nt, int grid_cols, int grid_rows, int num_levels,
                             const float* scale_factors, const float* inv_level_sigma_sq, float log_scale_factor, const double* intrinsics,
                             int num_trials_robust, int num_trials, int num_each_iter, int reset_stop_flag_each_round, int check_orientation,
                             int num_candidates, const uint8_t* active, const double* pose_cw, const int32_t* n_already_found,
                             const uint8_t* frame_has_lm, const double* frame_lm_pos_w, const int32_t* kf_off, const double* pos_w,
                             const uint8_t* valid, const float* min_valid_dist, const float* max_valid_dist, const uint8_t* lm_desc,
                             const float* angle_kf, int num_stages, const float* margin, const int32_t* hamm_dist_thr, int min_num_valid_obs,
                             int32_t* status, double* pose_out, int32_t* match_kf, int32_t* match_stage, uint8_t* outlier, int32_t* num_found,
                             int32_t* num_valid, int32_t* lm_iterations, svgpu_call_stats* stats);

/* module::relocalizer::reloc_by_candidate (module/relocalizer.cc:93-132) behind the BoW matcher, for ALL candidates in one call: per
 * candidate relocalize_by_pnp_solver's RANSAC (:191-197; solve/pnp_solver.cc:44-124) -> relocalizer::optimize_pose (:211-234) -> the
 * bookkeeping of :103-123 -> refine_pose (:236-297), i.e. the chain svgpu_pnp_ransac -> svgpu_pose_optimize -> svgpu_reloc_refine_batch
 * with the host steps between them done on the device.  The frame, its bearings and the keyframe entries are uploaded once; which
 * problems PnP and the first optimisation run is decided on the device, from the flags the kernel before wrote.
 *   frame (shared)       as svgpu_reloc_refine_batch, plus t_bearings (nt x 3 doubles, frm_obs_.bearings_)
 *   per candidate p      active[p] (nullable = all) and its 2D-3D matches, the entries match_off[p] .. match_off[p + 1] of
 *     m_keypt            frame keypoint index, strictly ascending inside a candidate (extract_valid_indices order, :391-405)
 *     m_pos_w            3 doubles, the landmark's position
 *     m_kf_entry         index of the landmark among the candidate's keyframe entries (relative to kf_off[p]), or -1 when it is none of
 *                        them (it came from a neighbour keyframe); the values >= 0 are distinct inside a candidate
 *                        octave, observation, weight and Huber delta of a match are derived on the device from t_octave / t_xy /
 *                        t_xright / inv_level_sigma_sq as svgpu_reloc_refine_batch derives them (pose_optimizer_g2o.cc:86-109)
 *   PnP                  min_num_inliers, num_iter, samples (num_candidates x num_iter x 4, local indices), recompute,
 *                        gauss_newton_num_iter: as svgpu_pnp_ransac_batch
 *   min_num_opt_valid_obs   the threshold of optimize_pose: the reference tests its count against min_num_bow_matches_ / 2 (:220), a
 *                        number of its own beside the min_num_valid_obs of refine_pose
 *   keyframe entries, stages   kf_off, pos_w, valid, min_valid_dist, max_valid_dist, lm_desc, angle_kf, num_stages, margin, hamm_dist_thr,
 *                        min_num_valid_obs: as svgpu_reloc_refine_batch
 * Per candidate, in order:
 *   1. svgpu_pnp_ransac over its matches; not valid: status SVGPU_RELOC_PNP_FAILED, the candidate stops.  A candidate with fewer than 4 or
 *      fewer than min_num_inliers matches is not valid and launches nothing for itself.
 *   2. svgpu_pose_optimize from the PnP pose over the inlier matches, in entry order; the pose goes on whatever follows (:218);
 *      num_valid < min_num_opt_valid_obs: status SVGPU_RELOC_OPTIMIZE_FAILED, the candidate stops.
 *   3. a keypoint holds a landmark where its match is an inlier of 1 and no outlier of 2, frame_lm_pos_w is that match's m_pos_w,
 *      n_already_found the number of such matches, and every keyframe entry such a match names becomes invalid;
 *   4. the stages of svgpu_reloc_refine_batch from that state.
 * Outputs: status (0 accepted, -1 inactive on input, the two codes above, else the refine call's 1 + s unchanged); of step 1 pnp_valid /
 * pnp_pose_cw / best_iter per candidate and is_inlier per match entry, as svgpu_pnp_ransac returns them; of step 2 opt_pose,
 * opt_num_valid per candidate and opt_outlier per match entry (0 for a non-inlier); every output of svgpu_reloc_refine_batch.  Every
 * output of candidate p equals, bit for bit, that chain of calls for the candidate alone, whatever else the batch holds; outputs of a
 * step a candidate did not reach carry what the refine call documents for a stage not reached (pose = the last pose that exists -- zero
 * after an invalid PnP --, counts 0, flags 0, matches -1).
 * `stats` (nullable): launches, copies and synchronisations do not depend on num_candidates, and the synchronisations are those of
 * svgpu_reloc_refine_batch for the same num_stages.
 * SVGPU_ERR_INVALID before anything is launched or written: what svgpu_reloc_refine_batch refuses; offsets that do not start at 0 or are
 * not monotone; m_keypt outside [0, nt) or not strictly ascending; m_kf_entry outside [-1, kf_off[p + 1] - kf_off[p]) or repeated; a
 * sample index outside its problem or repeated within a sample (of a problem that runs).  num_candidates == 0 succeeds whatever else is
 * passed.  Host in/out, synchronous. */
#define SVGPU_RELOC_PNP_FAILED (-2)
#define SVGPU_RELOC_OPTIMIZE_FAILED (-3)
int svgpu_reloc_solve_batch(svgpu_ctx* ctx, const svgpu_camera* cam, const uint8_t* tdesc, const float* t_xy, const int32_t* t_octave,
                            const float* t_angle, const float* t_xright, const double* t_bearings, int nt, int grid_cols, int grid_rows,
                            int num_levels, const float* scale_factors, const float* inv_level_sigma_sq, float log_scale_factor,
                            const double* intrinsics, int num_trials_robust, int num_trials, int num_each_iter, int reset_stop_flag_each_round,
                            int check_orientation, int num_candidates, const uint8_t* active, const int32_t* match_off, const int32_t* m_keypt,
                            const double* m_pos_w, const int32_t* m_kf_entry, int min_num_inliers, int num_iter, const uint32_t* samples,
                            int recompute, int gauss_newton_num_iter, int min_num_opt_valid_obs, const int32_t* kf_off, const double* pos_w,
                            const uint8_t* valid, const float* min_valid_dist, const float* max_valid_dist, const uint8_t* lm_desc, const float* angle_kf,
                            int num_stages, const float* margin, const int32_t* hamm_dist_thr, int min_num_valid_obs, int32_t* status,
                            uint8_t* pnp_valid, double* pnp_pose_cw, uint8_t* is_inlier, int32_t* best_iter, double* opt_pose,
                            uint8_t* opt_outlier, int32_t* opt_num_valid, double* pose_out, int32_t* match_kf, int32_t* match_stage,
                            uint8_t* outlier, int32_t* num_found, int32_t* num_valid, int32_t* lm_iterations, svgpu_call_stats* stats);

/* The middle of module::loop_detector::select_loop_candidate_via_Sim3 (module/loop_detector.cc:537-587) for ALL candidates that survived
 * the pose refinement, in one call: per candidate the scale from the small-parallax landmark pairs (:540-573),
 * projection::match_keyframes_mutually (:577; match/projection.cc:418-629), the edge gather of optimize::transform_optimizer::optimize
 * (optimize/transform_optimizer.cc:64-94) and the optimisation itself (:581), with the decision of :585.  Keyframe 1 (the current
 * keyframe) is uploaded and binned once; the candidates' keypoints are binned in one pass; both matcher passes of all candidates are one
 * concatenation of queries; the edges go straight into the arrays the Sim3 optimiser reads.
 *   keyframe 1 (shared)  cam1, pose_1w (12 doubles, rows of [rot_cw | trans_cw]), n1 keypoints: desc1 / xy1 (undistorted) / octave1, and
 *                        one landmark slot per keypoint: pos_w1, has_lm1 (non-null and not will_be_erased), min_valid1 / max_valid1,
 *                        lm_desc1; the ORB tables and the grid as svgpu_match_keyframes_mutually takes them, inv_level_sigma_sq by octave
 *   per candidate p      cam2[p], pose_2w[p] (12), the entries kf2_off[p] .. kf2_off[p + 1] of desc2 / xy2 / octave2 / pos_w2 / has_lm2 /
 *                        min_valid2 / max_valid2 / lm_desc2 (a candidate may have none); pose_1w_in_cand[p] (12, optimized_pose2, :537);
 *                        rot_12[p] (9) and trans_12[p] (3) as :570-571 computes them; sim3_12[p] (8 doubles as
 *                        svgpu_sim3_transform_optimize takes them; the scale entry is ignored); active[p] (nullable = all)
 *   prior matches        curr_match_lms_observed_in_cand, each K x n1: prior_state 0 none, 1 present and alive, 2 present and
 *                        will_be_erased; prior_idx2 = lm->get_index_in_keyframe(keyfrm_2), or -1 when negative or >= n2; prior_pos_w x 3
 *   of the call          scale_12_in (nullable, K floats: the scale is taken from it and step 1 is skipped); margin (the reference: 7.5);
 *                        chi_sq, fix_scale, num_iter as svgpu_sim3_transform_optimize; min_num_inliers (num_optimized_inliers_thr_)
 * Per active candidate:
 *   1. scale (:540-573): for every idx1 with has_lm1 and prior_state 1, pos_1_in_cand = R prior_pos_w + t from pose_1w_in_cand and
 *      pos_1_in_curr from pose_1w and pos_w1; both norms in double, narrowed to float; cos_parallax = (float)(dot / (double)(n_cand *
 *      n_curr)) with the product in float; kept iff 0.99996192306f < cos_parallax; ratio n_curr / n_cand in float; scale_12 = element
 *      (count - 1) / 2 of the ratios in ascending order.  No ratio: status SVGPU_LOOP_NO_SCALE, nothing further runs for the candidate.
 *   2. mutual match (projection.cc:418-629): is_already_matched_in_keyfrm_1 / 2 from prior_state != 0 && prior_idx2 >= 0 (:440-450); both
 *      passes as svgpu_match_keyframes_mutually runs them (best only, HAMMING_DIST_THR_HIGH, level window +-1, the distance range with the
 *      1.3 margins in double, keyframe 2's camera for the in-image test in BOTH passes), then the cross-check (:613-626).
 *   3. edges (transform_optimizer.cc:64-94), idx1 ascending: has_lm1 and either a new mutual match (pos_w2[idx2]; it overwrites a prior
 *      entry, :623) or a prior with prior_state 1 and prior_idx2 >= 0 (prior_pos_w).
 *   4. svgpu_sim3_transform_optimize on those edges; status SVGPU_LOOP_FEW_INLIERS when num_inliers < min_num_inliers, else 0.
 * Outputs: status (K; -1 = inactive on input), scale_12 (K; 0 where none was estimated), matched_2_in_1 (K x n1), matched_1_in_2
 * (by kf2_off), mutual_2_in_1 (K x n1: the new mutual matches, else -1), num_mutual (K), edge_idx1 / edge_idx2 (K x n1, num_edges[p] valid
 * entries per row, -1 behind them), edge_status (K x n1: the optimiser's status byte per edge, 0 behind them), sim3_12_out (K x 8: the
 * input with the estimated scale if the optimiser returned early; the input itself for an inactive candidate or one without a scale),
 * num_inliers (K), opt_stats (nullable, K; zero where the optimiser had nothing to do).  Every output equals, bit for bit, the chain
 * of svgpu_match_keyframes_mutually and svgpu_sim3_transform_optimize for that candidate alone, whatever else the batch holds.
 * `stats` (nullable) receives what the call issued; none of the three depends on num_candidates.  Two synchronisations: the candidate-list
 * total and the end.  A call whose lists outgrow their first capacity (16 entries per row, at most 4 Mi entries) starts again with lists
 * of the exact size: `stats` then holds the launches, copies and synchronisations of both attempts (3 synchronisations).
 * SVGPU_ERR_INVALID before anything is launched or written: a null required pointer, kf2_off[0] != 0 or non-monotone offsets, an octave
 * outside [0, num_levels), num_levels outside 1..16, n1 or an n2 >= 1 << 22, a prior_idx2 >= that candidate's n2, a camera model the Sim3
 * edges do not cover, a non-unit quaternion, a non-positive chi_sq, inv_level_sigma_sq or scale_12_in, num_iter < 0, totals beyond int32.
 * num_candidates == 0 succeeds whatever else is passed.  Host in/out, synchronous. */
#define SVGPU_LOOP_NO_SCALE 1
#define SVGPU_LOOP_FEW_INLIERS 2
int svgpu_loop_sim3_batch(svgpu_ctx* ctx, const svgpu_camera* cam1, const double* pose_1w, int n1, const uint8_t* desc1, const float* xy1,
                          const int32_t* octave1, const double* pos_w1, const uint8_t* has_lm1, const float* min_valid1,
                          const float* max_valid1, const uint8_t* lm_desc1, int num_levels, const float* scale_factors,
                          const float* inv_level_sigma_sq, float log_scale_factor, int grid_cols, int grid_rows, int num_candidates,
                          const svgpu_camera* cam2, const double* pose_2w, const int32_t* kf2_off, const uint8_t* desc2, const float* xy2,
                          const int32_t* octave2, const double* pos_w2, const uint8_t* has_lm2, const float* min_valid2,
                          const float* max_valid2, const uint8_t* lm_desc2, const double* pose_1w_in_cand, const double* rot_12,
                          const double* trans_12, const double* sim3_12, const uint8_t* active, const uint8_t* prior_state,
                          const int32_t* prior_idx2, const double* prior_pos_w, const float* scale_12_in, float margin, float chi_sq,
                          int fix_scale, int num_iter, int min_num_inliers, int32_t* status, float* scale_12, int32_t* matched_2_in_1,
                          int32_t* matched_1_in_2, int32_t* mutual_2_in_1, int32_t* num_mutual, int32_t* edge_idx1, int32_t* edge_idx2,
                          int32_t* num_edges, uint8_t* edge_status, double* sim3_12_out, int32_t* num_inliers,
                          svgpu_sim3opt_stats* opt_stats, svgpu_call_stats* stats);

/* The loop of mapping_module::create_new_landmarks (mapping_module.cc:275-341) for ALL neighbours in one call: per neighbour
 * match_for_triangulation (:332-335), then two_view_triangulator::triangulate on its matches (:343-375).  The loop is sequential: a
 * keypoint of the current keyframe that got a landmark at neighbour p (:364-367) is no query for neighbour p + 1 (robust.cc:47-50,
 * bow_tree.cc likewise).  svgpu_match_for_triangulation_batch followed by svgpu_triangulate_two_views_batch treats the neighbours as
 * independent and hands a keypoint that matches in two neighbours to both; this call carries the landmark state from neighbour to
 * neighbour on the device.
 *   side1 / view1       the current keyframe as the matcher and as the triangulator see it; side2[k] / neighbours[k] likewise for
 *                       neighbour k.  The two views of a keyframe must agree in n and name the SAME octave / bearings / xright arrays
 *                       (a side-2 match view may leave octave null); every array is uploaded once.
 *   active              nullable = all; 0 = the neighbour is skipped (the baseline `continue` of :303-319, decided by the caller)
 *   E_12, epipole_in_2, valid_epipole   per neighbour, as in svgpu_match_for_triangulation_batch; the remaining parameters as in
 *                       svgpu_match_for_triangulation and svgpu_triangulate_two_views, shared by all neighbours
 * With taken_0 = !side1->valid (null: nothing taken), for p = 0 .. num_neighbours - 1 in order:
 *   inactive            row p of matched_2_in_1 is -1, of status SVGPU_TRI_SKIPPED, of pos_w zero, both counts 0; taken_{p+1} = taken_p
 *   active              row p of matched_2_in_1 (num_neighbours x n1) equals, element for element, svgpu_match_for_triangulation with
 *                       has_lm1 = taken_p against neighbour p; rows p of pos_w (x 3) and status equal, bit for bit,
 *                       svgpu_triangulate_two_views on that row in its idx2 == NULL form;
 *                       taken_{p+1} = taken_p | (status == SVGPU_TRI_ACCEPTED), and created_by[i] = p for those keypoints
 *   created_by          n1: the neighbour whose match gave keypoint i its landmark, or -1
 * `stats` (nullable) receives what the call issued.  Two synchronisations whatever num_neighbours is (the candidate-list total and
 * the end; one when no neighbour has a candidate); launches = a constant + 2 per active neighbour (a replay and a triangulation
 * launch, enqueued back to back); one read-back.
 * SVGPU_ERR_INVALID before anything is staged or launched, the outputs untouched: a null required pointer; n < 0 or an n2 >= 1 << 22;
 * node ids on one side only; check_orientation without angles; missing bearings, octaves or xy; num_levels outside 1..16; an octave of
 * any keyframe outside [0, num_levels); `occupied` set on any view; a camera model out of range; a stereo keypoint of an equirectangular
 * camera; the two views of a keyframe disagreeing; totals beyond int32.  num_neighbours == 0 succeeds and touches nothing.
 * Host in/out, synchronous. */
int svgpu_new_landmarks_batch(svgpu_ctx* ctx, const svgpu_match_view* side1, const svgpu_triangulate_view* view1, int num_neighbours,
                              const svgpu_match_view* side2, const svgpu_triangulate_view* neighbours, const uint8_t* active, const double* E_12,
                              const double* epipole_in_2, const int32_t* valid_epipole, const float* scale_factors, const float* level_sigma_sq,
                              int num_levels, float residual_rad_thr, float lowe_ratio, int check_orientation, float rays_parallax_deg_thr,
                              int32_t* matched_2_in_1, double* pos_w, uint8_t* status, int32_t* num_matches, int32_t* num_accepted,
                              int32_t* created_by, svgpu_call_stats* stats);

/* ------------------------------------------------------------------------------ landmark fusion of a new keyframe
 * mapping_module::fuse_landmark_duplication (mapping_module.cc:417-537) for all fuse targets in ONE staged call: per target
 * fuse::detect_duplication of the current keyframe's landmarks, then the replace / connect_to_keyframe / compute_descriptor /
 * update_mean_normal_and_obs_scale_variance bookkeeping (:436-467) that decides the next target's inputs, and at the end the
 * backward pass into the current keyframe (:471-536).  The landmark state travels from target to target on the device.
 *
 * keyframes   num_targets + 1 records: slot 0 the current keyframe, slots 1.. the targets in the caller's order.  desc / xy / octave /
 *             xright (nullable) as svgpu_fuse_detect_duplication takes them; `observer` = the keyframe's index in the observer table;
 *             kp_lm (in/out, n entries) = landmark slot per keypoint, -1 = none.  The ORB tables are the call's (one extractor per map).
 * observers   every keyframe that observes a landmark of the table: observer_rank = its place in the order of landmark::observations_t
 *             (data/landmark.h:29: id_less, i.e. ascending keyframe id; ranks are distinct), observer_trans_wc its camera centre.
 * table       num_landmarks slots.  pos_w, ref_trans_wc / ref_scale_factor (the reference keyframe's camera centre and
 *             scale_factors_[octave of its keypoint]; a survivor keeps its reference keyframe), obs_off / obs_cap are inputs; alive,
 *             descriptor, mean_normal, the distance limits, the two "has" flags, obs_cnt and the observation entries at
 *             obs_off[l] .. obs_off[l] + obs_cnt[l] (rank order; observer, keypoint, its 32-byte descriptor, and the weight the
 *             observation adds to num_observations(): 2 for a keypoint with stereo x_right >= 0, else 1, data/landmark.cc:116-121)
 *             are in/out; replaced_by (out) = the survivor a dead landmark was replaced by, -1 otherwise.
 * fwd_list    n_fwd slots (-1 allowed): cur_keyfrm_->get_landmarks() as copied before the loop (:426).
 * bwd_list    n_bwd distinct slots: the landmarks of the targets in the order the caller wants them checked (the reference iterates an
 *             unordered_set); entries that are dead after the forward loop are no candidates.
 * For k = 1 .. num_targets: valid = slot >= 0, alive, no observation by target k; gates, window, greedy claims in list order and
 * best <= HAMMING_DIST_THR_LOW as svgpu_fuse_detect_duplication on the CURRENT table; then the hits in ascending list index, the
 * duplicates (:436-456) before the new connections (:458-467):
 *   duplicate (the keypoint's kp_lm at detection time is alive)   same slot: SVGPU_FUSE_SAME_ID.  Otherwise the one with fewer
 *       num_observations() loses (the checked one at equality survives); its observations move to the survivor where the survivor
 *       has none by that observer, kp_lm of a table keyframe is rewritten (landmark::replace, prepare_for_erasing), the loser dies,
 *       replaced_by[loser] = survivor, and the survivor's descriptor / geometry are refreshed if their flag is down.
 *       SVGPU_FUSE_DUP_SURVIVED / SVGPU_FUSE_DUP_LOST speak of the checked landmark.  A pair one of whose members died earlier in the
 *       same target (possible only when kp_lm and the observation lists disagree on entry) is SVGPU_FUSE_SKIPPED.
 *   new connection (the keypoint holds no landmark)   replaced_by is followed from the checked landmark (:461-463), the observation is
 *       inserted (an existing one by that observer is overwritten and its weight added, as observations_[keyfrm] = idx does),
 *       kp_lm is set, both refreshes run.  SVGPU_FUSE_NEW_CONNECTION.
 * Then once for bwd_list into slot 0.  best (num_targets + 1 rows: fwd rows of n_fwd, then one row of n_bwd, concatenated) and event
 * per checked entry; num_fused per pass (num_targets + 1).
 * Every float output equals, bit for bit, the chain of svgpu_fuse_detect_duplication, svgpu_landmarks_compute_descriptor and
 * svgpu_landmarks_update_geometry calls with that bookkeeping done on the host between them.
 * SVGPU_ERR_INVALID before anything is staged or launched: a null required pointer, an index out of its range (kp_lm, lists, observation
 * entries, observers), obs_cnt > obs_cap, overlapping observation ranges, an octave outside [0, num_levels), duplicate ranks, two keyframe
 * slots with one observer, a keyframe of more than 8192 keypoints or a grid of more than 4096 cells, an obs_cap above 4096, an observation
 * weight outside {1, 2}, a list that is not in rank order, the same (observer, keypoint) held by two landmarks, a slot twice in bwd_list.
 * num_targets == 0 succeeds, reports zero stats and touches nothing else.
 * SVGPU_FUSE_OVERFLOW: an observation list would have outgrown obs_cap, or a candidate list the capacity sized from the snapshot
 * (fuse_layout.h); every in/out and output array is then untouched and the caller takes the chain of single calls.
 * `stats`: two synchronisations whatever num_targets is; launches and copies affine in num_targets (a call whose arena regrows for the
 * lists stages and bins a second time: a larger constant, the same slope).  Host in/out, synchronous. */
#define SVGPU_FUSE_OVERFLOW 100
#define SVGPU_FUSE_NONE 0
#define SVGPU_FUSE_NEW_CONNECTION 1
#define SVGPU_FUSE_DUP_SURVIVED 2
#define SVGPU_FUSE_DUP_LOST 3
#define SVGPU_FUSE_SAME_ID 4
#define SVGPU_FUSE_SKIPPED 5
typedef struct svgpu_fuse_keyframe {
    const svgpu_camera* cam;
    const double* rot_cw;   /* 9, row-major */
    const double* trans_cw; /* 3 */
    const uint8_t* desc;    /* n x 32 */
    const float* xy;        /* n x 2 undistorted */
    const int32_t* octave;  /* n */
    const float* xright;    /* n, nullable */
    int32_t* kp_lm;         /* n, in/out */
    int32_t n;
    int32_t observer;
    int32_t grid_cols, grid_rows;
} svgpu_fuse_keyframe;
typedef struct svgpu_fuse_table {
    int32_t num_landmarks;
    int32_t num_entries;     /* length of the observation arrays: every obs_off[l] + obs_cap[l] <= num_entries */
    const double* pos_w;     /* L x 3 */
    const double* ref_trans_wc;     /* L x 3 */
    const float* ref_scale_factor;  /* L */
    const int32_t* obs_off;  /* L */
    const int32_t* obs_cap;  /* L */
    uint8_t* alive;          /* L */
    uint8_t* descriptor;     /* L x 32 */
    double* mean_normal;     /* L x 3 */
    float* min_valid_dist;   /* L */
    float* max_valid_dist;   /* L */
    uint8_t* has_descriptor; /* L */
    uint8_t* has_geometry;   /* L */
    int32_t* obs_cnt;        /* L */
    int32_t* obs_observer;   /* num_entries */
    int32_t* obs_kp;         /* num_entries */
    uint8_t* obs_desc;       /* num_entries x 32 */
    int32_t* obs_weight;     /* num_entries */
    int32_t* replaced_by;    /* L, out */
} svgpu_fuse_table;
int svgpu_fuse_landmarks_batch(svgpu_ctx* ctx, int num_targets, const svgpu_fuse_keyframe* keyframes, int num_observers,
                               const int32_t* observer_rank, const double* observer_trans_wc, const svgpu_fuse_table* table, int n_fwd,
                               const int32_t* fwd_list, int n_bwd, const int32_t* bwd_list, int num_levels, const float* scale_factors,
                               const float* inv_level_sigma_sq, float log_scale_factor, float inv_scale_factor_last, float margin,
                               int do_reprojection_matching, int32_t* best_idx, uint8_t* event, int32_t* num_fused, svgpu_call_stats* stats);

/* Global BA core (optimize/global_bundle_adjuster.cc:26-192, 279-412): the same graph over ALL keyframes (spanning root
 * fixed), ONE Levenberg-Marquardt run of problem->num_first_iter iterations with the terminate rule, optional Huber
 * (obs_huber_delta), no outlier gate (num_second_iter is ignored).  The caller applies the reference's post-conditions
 * (`force_stop_flag && *force_stop_flag && !stats->stopped_by_terminate_action` => discard, :341-343).
 * Reduced systems beyond the on-chip solvers are factored by the block envelope Cholesky of the block-sparse Schur complement
 * (svgpu_ba_set_solver; the reference uses a sparse CSparse Cholesky there; the block-Jacobi PCG stays selectable).  Host in/out, synchronous. */
int svgpu_global_ba(svgpu_ctx* ctx, const svgpu_ba_problem* problem, volatile uint8_t* stop, double* pose_out,
                    double* points_out, svgpu_ba_stats* stats);

/* Multi-GPU variant.  Every rank passes the FULL pose / point arrays and ITS SHARD of the observations; the shard
 * must be BY LANDMARK (all observations of one landmark on one rank) so that the Schur complement of a landmark is formed
 * locally: either by keyframe segment (svgpu_ba_partition_keyframe_segments below: per damping trial only the separator blocks of the
 * reduced system cross ranks) or any other way, e.g. obs_point % world == rank -- then, per damping trial, the kept 6x6 blocks of the
 * partial reduced camera systems and their right-hand sides (36 * blocks + 6 * free poses doubles) are summed with ONE all-reduce.  The
 * factorisation of a large reduced system is distributed over the ranks (segmented envelope elimination), small ones are solved on every rank; per linearisation the pose blocks Hpp/bp (42 doubles per free pose) and per trial four scalars
 * (chi2, step scale, solver failure, stop votes) are summed as well.  All collectives are enqueued on the context's stream:
 * the damping loop never waits for the host.
 *   allreduce == NULL   the context's own RCCL communicator is used (svgpu_comm_init below: no Python, no callback)
 *   allreduce != NULL   `allreduce(user, dev_buf, count, stream)` must sum `count` doubles in place across ranks, ordered on
 *                       `stream` (stella_vslam_amd/distributed.py binds it to torch.distributed: RCCL, or gloo in CPU-side tests)
 * All ranks return identical poses and points; outlier_out covers the local shard.  A rank's stop flag is a VOTE: the votes are
 * summed inside the per-trial all-reduce and every rank acts on the sum only, so ranks never diverge between two collectives
 * however the callers' flags are raised.  Whether a stop POINTER was passed is agreed the same way: if any rank passes one, every rank
 * behaves as if it had (a NULL `stop` on some ranks only is allowed and cannot desynchronise the early return / skipped second stage). */
typedef int (*svgpu_allreduce_fn)(void* user, double* dev_buf, size_t count, void* stream);
int svgpu_local_ba_sharded(svgpu_ctx* ctx, const svgpu_ba_problem* shard, int rank, int world,
                           svgpu_allreduce_fn allreduce, void* allreduce_user, volatile uint8_t* stop, double* pose_out,
                           double* points_out, uint8_t* outlier_out, svgpu_ba_stats* stats);
/* svgpu_global_ba over the same sharding (BASELINE config 5: landmark-sharded global BA at 1/2/4/8 GPUs). */
int svgpu_global_ba_sharded(svgpu_ctx* ctx, const svgpu_ba_problem* shard, int rank, int world,
                            svgpu_allreduce_fn allreduce, void* allreduce_user, volatile uint8_t* stop, double* pose_out,
                            double* points_out, svgpu_ba_stats* stats);

/* Keyframe-segment partition of a global-BA problem over `world` ranks (optimize/global_bundle_adjuster.cc:26-192 is the workload):
 * the ordered keyframe graph is cut by the vertex separators of the segmented envelope solve (the cuts the solve itself will make for
 * `world` ranks), every piece between two cuts is a job owned by one rank, and a landmark goes to the rank that owns the piece its
 * keyframes lie in -- co-observation makes a landmark's keyframes a clique of the keyframe graph, so they all lie in ONE piece plus
 * separator keyframes.  Host only (no device is touched, ctx-free).
 *   landmark_rank   num_points entries: the rank whose shard gets every observation of that landmark (a valid BY-LANDMARK sharding)
 *   info            12 ints: [0] 1 = keyframe segments, 0 = no segmented plan for this problem: landmark_rank = l % world;
 *                   [1] jobs  [2] cuts  [3] separator keyframes  [4] landmarks seen from a separator keyframe (their blocks are what
 *                   crosses ranks)  [5] of those, seen from separator keyframes only  [6] free keyframes  [7] kept 6x6 blocks
 *                   [8] kept blocks between two separator keyframes  [9] doubles the jobs leave on the separators per trial  [10..11] 0
 * svgpu_global_ba_sharded / svgpu_local_ba_sharded RECOGNISE shards cut this way (every observation of a piece's keyframe on the
 * piece's rank; agreed between the ranks by one flag at set-up) and then exchange, per damping trial, only the separator-by-separator
 * blocks and separator rows of the reduced system + what the jobs leave on the separators + the solution, instead of the whole
 * reduced system; any other by-landmark sharding (l % world) keeps the full exchange.  SVGPU_BA_EXCHANGE=full forces the latter. */
int svgpu_ba_partition_keyframe_segments(const svgpu_ba_problem* problem, int world, int32_t* landmark_rank, int32_t* info);
/* What the last sharded solve on this context all-reduced, in bytes of payload per rank: info[0] 0 = not sharded, 1 = whole reduced
 * system per trial, 2 = keyframe-segment exchange; [1] set-up  [2] pose blocks (per linearisation)  [3] reduced system (per trial)
 * [4] separator contributions of the jobs (per trial)  [5] solution (per trial)  [6] trial sums / damping slots; [7] all-reduce calls
 * [8] damping trials  [9] linearisations. */
int svgpu_ba_last_exchange(svgpu_ctx* ctx, int64_t* info);

/* ------------------------------------------------------------------------------------------------ RCCL communicator
 * One communicator per context (= per GPU / process), RCCL over xGMI, loaded with dlopen on first use.  Rank 0 calls
 * svgpu_comm_unique_id and hands the 128 bytes (ncclUniqueId) to the other ranks through whatever channel the host
 * application has (the reference has none: a multi-process launcher passes it via its own rendezvous; bench.py and the tests
 * broadcast it with torch.distributed); every rank then calls svgpu_comm_init. */
int svgpu_comm_unique_id(uint8_t* id128);
int svgpu_comm_init(svgpu_ctx* ctx, int rank, int world, const uint8_t* id128);
void svgpu_comm_destroy(svgpu_ctx* ctx);
/* Sum of `count` doubles in place over the communicator, ordered on `stream` (NULL = the context's stream). */
int svgpu_comm_allreduce_f64(svgpu_ctx* ctx, double* dev_buf, size_t count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVGPU_H */
