/*
 * cvhip.h — C ABI of libcvhip.so, the MI355X (gfx950) backend for cybervision's hot path.
 *
 * This is the drop-in boundary: every entry point names the reference interface it replaces
 * (file:line into zlogic/cybervision v0.20.3, src/...).  Plain C types only; no HIP or torch
 * types cross the boundary.  INTEGRATION.md shows the Rust `extern "C"` block and the
 * `hip.rs` backend module a maintainer would add next to gpu/vulkan.rs and gpu/metal.rs.
 *
 * Conventions
 *  - Return value: 0 = CVHIP_OK, negative = error class; the message for the calling thread's
 *    last failure is cvhip_last_error() (maps to GpuError::Internal(&'static str),
 *    correlation/gpu/vulkan.rs:1204-1272).  Nothing throws or aborts across the ABI.
 *  - Ownership: the caller owns every host pointer and it only has to stay valid for the
 *    duration of the call; the library owns all device memory behind the opaque handles.
 *  - Image and output pointers may be HOST or DEVICE (HIP) pointers; the library detects
 *    which (hipPointerGetAttributes).  Device pointers must belong to the handle's GPU.
 *  - Grids are row-major, index = width*y + x (data.rs:22-64).  Option<Match> is encoded as
 *    int32 (x, y) with (-1, -1) = None plus a separate float score plane (NaN for None).
 *  - Threading: a handle is used by one thread at a time, as in the reference where every
 *    call goes through `&mut` (correlation/mod.rs:255).  Different handles are independent.
 *  - dir: 0 = CorrelationDirection::Forward, 1 = Reverse (correlation/mod.rs:77-81).  As in
 *    the reference, the caller swaps the images for Reverse (mod.rs:231-237) and the library
 *    transposes F (mod.rs:268-271).
 *  - projection: 0 = ProjectionMode::Affine, 1 = Perspective (correlation/mod.rs:43-47).
 */
#ifndef CVHIP_H
#define CVHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CVHIP_OK 0
#define CVHIP_ERR_INVALID (-1)     /* bad argument / call sequence */
#define CVHIP_ERR_DEVICE (-2)      /* HIP runtime error (message has hipGetErrorString) */
#define CVHIP_ERR_UNSUPPORTED (-3) /* valid in the reference, not supported here (documented) */
#define CVHIP_ERR_NOMEM (-4)
#define CVHIP_ERR_NO_MODEL (-5)    /* RANSAC: "Not enough matches" / "No reliable matches found" (RansacError) */
#define CVHIP_ERR_NO_SURFACE (-6)  /* perspective triangulation: the reference's TriangulationError messages */

typedef struct cvhip_device cvhip_device;
typedef struct cvhip_ctx cvhip_ctx;

/* Progress hook: replaces ProgressListener::report_status (correlation/mod.rs:56-61).
 * Invoked synchronously on the calling thread between kernel submissions; never retained. */
typedef void (*cvhip_progress_fn)(void *user, float pos);
/* fundamentalmatrix.rs:41-47: the RANSAC listener's second method, ProgressListener::report_matches(matches_count) -
 * the largest inlier count seen so far.  Same rules as cvhip_progress_fn. */
typedef void (*cvhip_matches_fn)(void *user, uint64_t matches_count);

/* Message of the calling thread's last error ("" if none). Static lifetime per thread. */
const char *cvhip_last_error(void);
/* ABI version, bumped on incompatible change. */
uint32_t cvhip_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Device — replaces GpuDevice::new / create_gpu_context (correlation/mod.rs:145-147) and
 * the DeviceContext trait (correlation/gpu/mod.rs:64-81).
 * ---------------------------------------------------------------------------------------- */

/* low_power mirrors HardwareMode::GpuLowPower (mod.rs:50-54); accepted and ignored (no
 * dispatch segmenting is needed on MI355X).  ordinal < 0 = HIP's current device. */
int cvhip_device_create(int low_power, int ordinal, cvhip_device **out);
/* Same, but all work is submitted to the caller's HIP stream (a hipStream_t passed as void*,
 * e.g. torch.cuda.current_stream().cuda_stream) so it is ordered with the caller's own work
 * (collectives between passes when row-sharding).  NULL means HIP's default (null) stream.  The
 * stream is not owned by the library. */
int cvhip_device_create_on_stream(int low_power, int ordinal, void *hip_stream, cvhip_device **out);
void cvhip_device_destroy(cvhip_device *dev);
/* DeviceContext::get_device_name (gpu/mod.rs:70). Valid until cvhip_device_destroy. */
const char *cvhip_device_name(const cvhip_device *dev);
/* Block until everything submitted on the device's stream has finished. */
int cvhip_device_synchronize(cvhip_device *dev);

/* ------------------------------------------------------------------------------------------
 * Dense correlation context — replaces GpuContext (correlation/gpu/mod.rs:106-362) as used by
 * PointCorrelations (correlation/mod.rs:150-245).
 * ---------------------------------------------------------------------------------------- */

/* GpuContext::new (gpu/mod.rs:125-163; called mod.rs:159-165).  dims are the FULL-RES image
 * dimensions, F is row-major 3x3 (nalgebra Matrix3 (r,c) -> F[3*r+c]). */
int cvhip_ctx_create(cvhip_device *dev, uint32_t w1, uint32_t h1, uint32_t w2, uint32_t h2, int projection,
                     const double *F, cvhip_ctx **out);
void cvhip_ctx_destroy(cvhip_ctx *ctx);

/* GpuContext::correlate_images (gpu/mod.rs:218-362; called mod.rs:255-259): one search pass
 * over level images img1 (searched) and img2 (target) at `scale`, results replace this
 * direction's level grid.  Results follow the reference's --mode=cpu semantics
 * (mod.rs:247-540), NOT the GLSL shaders' (SURVEY.md §8a N1).
 * Supported schedule (the only one the reference issues, reconstruction.rs:565-568):
 * scale = 2^-k exactly, k strictly decreasing from call to call per direction, level dims =
 * floor(full * scale); anything else returns CVHIP_ERR_UNSUPPORTED. */
int cvhip_correlate_images(cvhip_ctx *ctx, const uint8_t *img1, uint32_t w1, uint32_t h1, const uint8_t *img2,
                           uint32_t w2, uint32_t h2, float scale, int first_pass, int dir,
                           cvhip_progress_fn progress, void *user);

/* GpuContext::cross_check_filter (gpu/mod.rs:172-208; called mod.rs:557-560) with the CPU
 * semantics of mod.rs:552-624. */
int cvhip_cross_check_filter(cvhip_ctx *ctx, float scale, int dir);

/* One whole PointCorrelations::correlate_images (mod.rs:217-245) in a single call: forward
 * pass, reverse pass (images swapped, F transposed), cross-check forward, cross-check reverse.
 * Same results as the four calls above; uploads and window statistics are shared. */
int cvhip_correlate_level(cvhip_ctx *ctx, const uint8_t *img1, uint32_t w1, uint32_t h1, const uint8_t *img2,
                          uint32_t w2, uint32_t h2, float scale, int first_pass, cvhip_progress_fn progress,
                          void *user);

/* Result bands for host destinations.  With bands > 1 the last level (scale 1) of a pair whose geometry is row-local
 * (the same test as cvhip_plan_bands: affine models, near-horizontal epipolar lines) is searched and cross-checked in
 * `bands` row bands, and cvhip_complete_dir(dir 0) into HOST memory expands and copies band b out on the copy stream
 * while the bands behind it are still being searched - the 201 MB grid of a 4096^2 pair then costs ~1.5 ms beyond the
 * search instead of ~4.5.  The result is the one of bands == 1, bit for bit (tests/test_corr_gpu.py).  In the fused
 * four-call mode the last level's launches wait for its two cross_check_filter calls.  Under cvhip_ctx_set_async_readback
 * the level is not banded (the whole transfer runs under the next pair's search there).  Default 1 (off); at most 16;
 * 0 = the library chooses by size (bands of at least half a megapixel, six at most - what a binding whose grid always goes
 * to the host should pass).
 * Replaces nothing in the reference (its complete() maps one buffer after the last submission, gpu/mod.rs:321-349). */
int cvhip_ctx_set_result_bands(cvhip_ctx *ctx, uint32_t bands);
/* How many bands the grid now held went out in (1: not banded - the geometry, the size or the call order ruled it out). */
int cvhip_ctx_get_result_bands(cvhip_ctx *ctx, uint32_t *live);

/* The forward cross-check of the last level (scale 1) inside complete()'s expansion.  On (the default): that filter is
 * deferred, and cvhip_complete / cvhip_complete_dir(dir 0) / cvhip_complete_packed filter each cell while they write it out
 * - one pass over the grid and one launch instead of two.  Every other entry point that reads or hands out the forward
 * grid (cvhip_ctx_level_grid, cvhip_triangulate_affine, cvhip_extend_tracks) runs the plain filter first, so no result
 * changes, bit for bit (tests/test_fused_finish_gpu.py).  Row-sharded and band-mode contexts and levels that went out in
 * result bands never defer.  Off: the filter runs where the level's calls ask for it (a pending one is run at once). */
int cvhip_ctx_set_fused_finish(cvhip_ctx *ctx, int on);

/* GpuContext::complete_process (gpu/mod.rs:210-216; called mod.rs:208-215): write the forward
 * full-resolution grid.  out_xy: 2*w1*h1 int32, out_corr: w1*h1 float (may be NULL).
 * Host destinations are complete on return (synchronises); DEVICE destinations are written in
 * stream order on the context's stream without a host synchronisation (cvhip_device_synchronize,
 * or any later work on that stream, orders after them).  The context can be destroyed or reused
 * for cvhip_complete_dir afterwards. */
int cvhip_complete(cvhip_ctx *ctx, int32_t *out_xy, float *out_corr);
/* Asynchronous readback for pipelines that correlate pair after pair (reconstruction.rs:680-730): with enable = 1,
 * cvhip_complete into HOST destinations returns once the copies are enqueued - on the handle's own copy stream, behind
 * the grid expansion, from one of two device staging sets - so that the 12 B/px transfer of this pair runs under the
 * search of the next.  The destinations must be page-locked (hipHostMalloc / hipHostRegister; a pageable destination
 * makes the copy synchronous again) and are complete after cvhip_device_synchronize; at most two readbacks are in
 * flight per device handle (a third waits, on the device, for the first).  Default 0: complete on return. */
int cvhip_ctx_set_async_readback(cvhip_ctx *ctx, int enable);
/* Same for either direction (dir 1 = correlated_points_reverse, mod.rs:65); test hook. */
int cvhip_complete_dir(cvhip_ctx *ctx, int dir, int32_t *out_xy, float *out_corr);
/* The same grid in 8 instead of 12 bytes per cell, for host destinations behind PCIe: out_cells[y * w + x] =
 * y2 << 16 | x2 of the match (level dimensions are at most 65535), 0xFFFFFFFF = None; out_corr as above (may be NULL).
 * The binding unpacks in the loop in which it builds its Grid<Option<Match>> anyway (gpu/mod.rs:321-349 reads its own
 * [i32; 2] + f32 buffers cell by cell).  Everything else - result bands, asynchronous readback, device destinations - as
 * cvhip_complete_dir. */
int cvhip_complete_packed(cvhip_ctx *ctx, int dir, uint32_t *out_cells, float *out_corr);

/* All-gather hook for row sharding: called by cvhip_correlate_level after each sharded search
 * pass, on the calling thread.  `cells` is the device pointer of the level grid's match plane (4 bytes per level pixel)
 * of direction `dir`; shard r (0 <= r < n_shards) owns bytes [r*shard_bytes, (r+1)*shard_bytes).  The hook
 * must all-gather in place (e.g. ncclAllGather / torch.distributed.all_gather_into_tensor on
 * the stream given to cvhip_device_create_on_stream) and return 0, or non-zero to abort.  dir = 0 / 1: the match plane
 * of that direction (after each sharded search pass); dir = 2: the forward SCORE plane, once, after the forward pass at
 * scale 1 (same geometry; the only scores cvhip_complete reports).
 * Stream ordering: with a device handle created by cvhip_device_create_on_stream the hook MUST enqueue its collective
 * on that stream (the search pass before it and the cross-checks after it are submitted there).  With a handle that
 * owns a private stream (cvhip_device_create) the library fences both sides of the hook itself (stream synchronise
 * before, device synchronise after) - correct, but slower.  cvhip_ctx_set_row_shard_rccl needs neither. */
typedef int (*cvhip_allgather_fn)(void *user, void *cells, uint64_t shard_bytes, uint32_t n_shards, int dir);

/* Dense consumer — replaces AffineTriangulation::triangulate + triangulate_point
 * (triangulation.rs:268-330; reached from Triangulation::triangulate, :181-201, right after
 * PointCorrelations::complete()).  Straight from the device-resident forward grid, one track per
 * Some cell in scan order: out_points3d gets (x, y, sqrt(dx^2 + dy^2)) as 3 doubles per track,
 * out_p2 (may be NULL) the matched point (2 u32).  At most `cap` tracks are written; *out_n is
 * the number of Some cells (call with cap = 0 to size the buffers).  Host or device pointers. */
int cvhip_triangulate_affine(cvhip_ctx *ctx, double *out_points3d, uint32_t *out_p2, uint64_t cap, uint64_t *out_n);

/* Dense consumer, perspective pipeline — replaces Triangulation::extend_tracks (triangulation.rs:1330-1419; called
 * right after a pair's dense correlation, :638, :697) on the device-resident forward grid.
 *  - track_p1: the existing tracks' points in image 1, 2 int32 per track, (-1,-1) where a track has none.
 *  - out_track_p2[i]: the image-2 point `track.add(image2_index, ..)` is called with for track i - the match of the
 *    nearest Some cell within [p - r, p + r) (squared distance, first minimum in row-major order), r =
 *    3 * max_dimension2 / 1000 (3 when max_dimension2 <= 1000; max_dimension2 = max(width, height) of image 2) - or
 *    (-1,-1).  The caller applies Track::add's "only if the track has no point for this image yet" (:370-375).
 *  - The merged points are then cleared from the remaining grid AT THEIR OWN coordinates (the reference indexes the
 *    image-1 grid with the image-2 point, :1391-1393; out of bounds it panics - here CVHIP_ERR_INVALID), and every
 *    remaining Some cell becomes a new track: out_new_p1 = the cell, out_new_p2 = its match, scan order, at most
 *    `cap` written; *out_n_new = their number (call with cap = 0 to size the buffers).
 * Integer only, bit-exact.  Host or device pointers.  Uses the context's per-pass scratch: call it between pairs. */
int cvhip_extend_tracks(cvhip_ctx *ctx, const int32_t *track_p1, uint64_t n_tracks, uint32_t max_dimension2,
                        int32_t *out_track_p2, uint32_t *out_new_p1, uint32_t *out_new_p2, uint64_t cap,
                        uint64_t *out_n_new);

/* Dense consumer, perspective pipeline, last step - replaces PerspectiveTriangulation::triangulate_all (triangulation.rs:817-865)
 * with the cameras given by the caller (pose recovery, recover_pose / find_projection_matrix :1033-1278, and merge_tracks
 * :1421-1540 - cvhip_merge_tracks below - are not part of it):
 *  - triangulate_track (:867-911) for every track: the 2k x 4 DLT system of its k seen views in camera order, the right
 *    singular vector of the smallest singular value (nalgebra's `svd` sorts them in decreasing order, so the reference's
 *    `v_t.row(nrows - 1)`); rejected if k < 2 or |w| < 1e-4; the point is xyz / w.
 *  - filter_outliers (:1559-1593): dropped if a seen view has point_depth <= 0 (:492-500), if it has no pair of rays
 *    (rays shorter than f64::EPSILON skipped, min_ray_angle_cos :996-1031) or if the smallest |cos| between its rays is
 *    above cos(0.5 deg); the survivors keep their order (`retain`).
 *  - bundle_adjustment != 0 (the reference's default; --no-bundle-adjustment = 0): BundleAdjustment::optimize
 *    (:1675-2148) over all survivors and all cameras, with its Levenberg-Marquardt control as written, up to 100
 *    iterations; every reduction in a fixed order, so two calls give the same bits.
 * tracks: n x m x 2 int32 (x, y), (-1, -1) where the track has no point in that image.  K, R: m x 9 row-major, t: m x 3
 * (X_cam = R X + t).  As for the reference's initial pair (:727-740) the DLT projects with K [R | t] as given, while
 * filter_outliers and the bundle adjustment use the Camera that Camera::from_matrix (:414-466, including its 180 degree
 * branch) derives - whose angle is atan2(2 sin, cos) of R's as the reference writes it.
 * Out: out_points (n_kept x 3), out_index (n_kept: the row of each kept track in `tracks`) - both with room for n -,
 * per camera the refined r (3), t (3) and projection K [R | t] (12) (each may be NULL), *out_n = n_kept.  Optional
 * (NULL = not wanted): *out_iterations = the LM iterations run, out_history[100] = 1 accepted / 0 rejected step per
 * iteration (0xFF after the last), out_residual_norms[2] = |residual| before and after (NaN without bundle adjustment).
 * progress (may be NULL): iter / 100 before every iteration (:2054-2056), on the calling thread.
 * Errors: CVHIP_ERR_NO_SURFACE "Failed to compute delta vector" (the LU solve of S fails) / "Levenberg-Marquardt failed
 * to converge" (100 iterations); CVHIP_ERR_UNSUPPORTED above CVHIP_TRIANGULATE_MAX_CAMERAS cameras.  Tracks, outputs:
 * host or device pointers. */
#define CVHIP_TRIANGULATE_MAX_CAMERAS 8
int cvhip_triangulate_perspective(cvhip_device *dev, const int32_t *tracks, uint64_t n, uint32_t m, const double *K,
                                  const double *R, const double *t, int bundle_adjustment, double *out_points,
                                  uint64_t *out_index, double *out_r, double *out_t, double *out_projection,
                                  uint64_t *out_n, uint32_t *out_iterations, uint8_t *out_history,
                                  double *out_residual_norms, cvhip_progress_fn progress, void *user);

/* The same as cvhip_triangulate_perspective, with each camera given as the reference holds it after pose recovery
 * (PerspectiveTriangulation::{cameras, projections}, triangulation.rs:604-617, 727-752, 805-808): r (m x 3, the Camera's
 * axis-angle, as from_matrix made it), t (m x 3), K (m x 9) and projection (m x 12, what triangulate_tracks projects
 * with).  For a P3P camera the projection is K [matrix_r(from_matrix(R)) | t], not K [R | t], which the entry above
 * cannot express.  Outputs, limits and errors as above. */
int cvhip_triangulate_perspective_cameras(cvhip_device *dev, const int32_t *tracks, uint64_t n, uint32_t m,
                                          const double *K, const double *r, const double *t, const double *projection,
                                          int bundle_adjustment, double *out_points, uint64_t *out_index, double *out_r,
                                          double *out_t, double *out_projection, uint64_t *out_n,
                                          uint32_t *out_iterations, uint8_t *out_history, double *out_residual_norms,
                                          cvhip_progress_fn progress, void *user);

/* merge_tracks (triangulation.rs:1421-1540; reconstruct_dense runs it after each linked image's pairs, reconstruction.rs:726)
 * for image `image_index` of shape width x height, as the reference computes it: its AverageTrack folds
 * return the LAST element folded, so with r = 2 * md / 1000 and d^2 = 100 * md / 1000 (md = max(width, height) > 1000;
 * else 2 and 100), for every cell p of image i that holds tracks: A = the highest row in cell (x*, yhi - 1), yhi =
 * min(py + r, height), x* = the highest column of [px - r, min(px + r, width)) with a track in rows [py - r, yhi) (lower
 * bounds saturate at 0); the cell is kept iff every track in it can_merge with A (in every image where both have a point,
 * dx^2 + dy^2 <= d^2), and yields a copy of its highest row.  Tracks without a point in image i are dropped.
 * tracks: n x m x 2 int32, a point present iff x >= 0 and y >= 0.  Out (each with room for n, each may be NULL): out_rows
 * = the source row of each merged track, out_tracks = those rows (n_out x m x 2), in row-major order of their cells;
 * *out_n = n_out.  out_stats[4] (may be NULL): tracks with a point in image i, occupied cells, cells rejected by can_merge,
 * cells whose A has no point.  The trailing triangulate_tracks (:1538) is not part of it.  Integer only, bit-exact.
 * Errors (nothing written): CVHIP_ERR_INVALID for image_index >= m, a point with exactly one negative coordinate or an
 * image-i point outside width x height (the reference panics there, data.rs:61-64); CVHIP_ERR_UNSUPPORTED above
 * CVHIP_TRIANGULATE_MAX_CAMERAS images or with 2^32 - 1 or more tracks or cells.  tracks, out_rows, out_tracks: host or
 * device pointers; out_n and out_stats: host memory. */
int cvhip_merge_tracks(cvhip_device *dev, const int32_t *tracks, uint64_t n, uint32_t m, uint32_t image_index,
                       uint32_t width, uint32_t height, uint64_t *out_rows, int32_t *out_tracks, uint64_t *out_n,
                       uint64_t *out_stats);

/* max_points (triangulation.rs:837-843; the tail of triangulate_all, after filter_outliers and the bundle adjustment):
 * `if tracks.len() > max_points { tracks.shuffle(rng); tracks.truncate(max_points) }` with an OS-seeded generator.  Here, as
 * for the RANSAC samplers, a counter-based one: row i of the n rows has the key
 *   key(seed, i) = mix64(mix64(seed) + (i + 1) * 0x9E3779B97F4A7C15)   (mod 2^64; output i of splitmix64 started at mix64(seed);
 *                                                                        mix64 = splitmix64's finaliser)
 * - pairwise distinct for one seed - and the max_points rows with the smallest keys are kept; max_points >= n keeps every row
 * (no selection runs, the arrays are copied), max_points = 0 none.  Departure: the kept SET has the distribution of the
 * reference's shuffle + truncate, the ORDER does not - the kept rows come in ascending row order, where the reference's order
 * is random (nothing downstream reads it: polygons are sorted, the writers go by row).
 * points: n x 3 f64, tracks: n x m_cams x 2 int32; each may be NULL when its output is NULL.  Out (each with room for
 * min(n, max_points) rows, each may be NULL, none may alias an input): out_rows = the kept rows, out_points and out_tracks =
 * their points and track rows; *out_n = min(n, max_points).  The threshold key is found by a radix select on the device
 * (8 passes of 8 bits, the keys recomputed in every pass), the kept rows are compacted in row order: integer only, exact.
 * Errors (nothing written): CVHIP_ERR_INVALID for a NULL dev or out_n, an output whose input is NULL, tracks with m_cams = 0;
 * CVHIP_ERR_UNSUPPORTED above CVHIP_TRIANGULATE_MAX_CAMERAS cameras or with 2^32 - 1 or more rows.  points, tracks and the
 * three outputs: host or device pointers; out_n: host memory.
 * CVHIP_SUBSET_WG_ROWS: the rows a workgroup of the selection kernels handles per trip; CVHIP_SUBSET_GRID_ROWS: the rows of one
 * trip of their whole grid (more rows: the workgroups loop). */
#define CVHIP_SUBSET_WG_ROWS 1024
#define CVHIP_SUBSET_GRID_ROWS 524288
int cvhip_surface_subset(cvhip_device *dev, uint64_t n, uint64_t max_points, uint64_t seed, const double *points,
                         const int32_t *tracks, uint32_t m_cams, uint64_t *out_rows, double *out_points, int32_t *out_tracks,
                         uint64_t *out_n);

/* The same selection on keys given by the caller (n u64): out_rows = the m rows with the smallest (key, row) pairs - of equal
 * keys the lower row is taken - in ascending row order; m >= n: every row; *out_n = min(n, m).  out_rows (room for min(n, m),
 * may be NULL) and keys: host or device pointers.  Errors (nothing written): CVHIP_ERR_INVALID for a NULL dev or out_n, or
 * NULL keys with n > 0; CVHIP_ERR_UNSUPPORTED with 2^32 - 1 or more rows. */
int cvhip_select_smallest_u64(cvhip_device *dev, const uint64_t *keys, uint64_t n, uint64_t m, uint64_t *out_rows,
                              uint64_t *out_n);

/* ------------------------------------------------------------------------------------------
 * The dense track table in device memory: n x m x 2 int32, row-major, (-1, -1) = no point - what
 * cvhip_extend_tracks, cvhip_merge_tracks, cvhip_triangulate_perspective[_cameras], cvhip_surface_subset and the
 * cvhip_mesh_* entries take as `tracks` - owned by an opaque handle, so that the table never crosses to the host between
 * a pair's correlation grid and the surface.  A table belongs to one cvhip_device, does all its work on that handle's
 * stream, and is destroyed before it.  m <= CVHIP_TRIANGULATE_MAX_CAMERAS (CVHIP_ERR_UNSUPPORTED above), fewer than
 * 2^32 - 1 rows (CVHIP_ERR_UNSUPPORTED).  The capacity grows geometrically (at least doubling), keeps the rows, and is
 * never smaller than asked.
 * POINTER LIFETIME: the address cvhip_tracks_info gives out is valid until the next call that changes the table
 * (assign, extend, merge, destroy): any of them may move the rows.
 * UNCHANGED ON ERROR: an entry that returns an error leaves the table's rows, row count and contents as they were.
 * Integer only: every entry is bit-exact, and equal to the host-table path around the entries above. */
typedef struct cvhip_tracks cvhip_tracks;

/* An empty table of m images with room for reserve_rows rows.  CVHIP_ERR_INVALID for a NULL dev or out, or m = 0 (checked
 * before any device call). */
int cvhip_tracks_create(cvhip_device *dev, uint32_t m, uint64_t reserve_rows, cvhip_tracks **out);
void cvhip_tracks_destroy(cvhip_tracks *t); /* NULL: nothing */

/* *out_rows = n, *out_capacity (rows), *out_m, *out_device_rows = the device address of row 0 (see POINTER LIFETIME; NULL
 * while the capacity is 0).  Each may be NULL. */
int cvhip_tracks_info(const cvhip_tracks *t, uint64_t *out_rows, uint64_t *out_capacity, uint32_t *out_m,
                      const int32_t **out_device_rows);

/* assign: the table becomes the n rows at `rows` (n x m x 2 int32).  read: rows [first, first + n) into `out`;
 * CVHIP_ERR_INVALID when the range passes the end.  rows, out: host or device pointers. */
int cvhip_tracks_assign(cvhip_tracks *t, const int32_t *rows, uint64_t n);
int cvhip_tracks_read(const cvhip_tracks *t, uint64_t first, uint64_t n, int32_t *out);

/* extend_tracks (triangulation.rs:1330-1419) of the pair (image1, image2) on the table, from ctx's forward grid - what
 * cvhip_extend_tracks and its caller's bookkeeping do, in one call: the search of cvhip_extend_tracks runs ONCE, reading
 * column image1 of the table in place; a track's match fills slot image2 only where that slot is empty (x < 0; Track::add,
 * :370-375); the removal map is marked for every track that found a match, filled or not; every remaining Some cell is
 * appended as a new row in scan order - the cell in slot image1, its match in slot image2, (-1, -1) elsewhere.
 * out_counts[3] (may be NULL): tracks whose search found a match, slots filled, rows appended.  A ctx with nothing
 * correlated fills and appends nothing.  max_dimension2 as for cvhip_extend_tracks.
 * Errors (table unchanged: the matches go to a scratch column, and the table is written only once the flag is known to be
 * clear): CVHIP_ERR_INVALID for image1 == image2, an image index >= m, a ctx of another cvhip_device than the table's, and
 * "Index out of bounds" (a merged match lies outside the image-1 grid), as cvhip_extend_tracks has it.  Uses the context's
 * per-pass scratch: call it between pairs. */
int cvhip_tracks_extend(cvhip_tracks *t, cvhip_ctx *ctx, uint32_t image1, uint32_t image2, uint32_t max_dimension2,
                        uint64_t *out_counts);

/* cvhip_merge_tracks' out_tracks becomes the table (the same launches and rules; the result goes to a second device buffer
 * and the two are exchanged).  out_stats[4] (may be NULL) as there.  Errors as there, table unchanged. */
int cvhip_tracks_merge(cvhip_tracks *t, uint32_t image_index, uint32_t width, uint32_t height, uint64_t *out_stats);

/* prune_projections (triangulation.rs:913-938): *out = a new table (the caller destroys it) of the k listed columns of every
 * row of src, in that order.  columns: k u32 in host memory, strictly increasing and < m (CVHIP_ERR_INVALID otherwise, or
 * for k = 0).  The new table shares nothing with src. */
int cvhip_tracks_select_columns(const cvhip_tracks *src, const uint32_t *columns, uint32_t k, cvhip_tracks **out);

/* out[j] = row rows[j] for j < k (k x m x 2 int32).  rows (u64) and out: host or device pointers.  A row >= n is
 * CVHIP_ERR_INVALID and nothing is written: the rows are checked on the device before the copy. */
int cvhip_tracks_gather(const cvhip_tracks *t, const uint64_t *rows, uint64_t k, int32_t *out);

/* ------------------------------------------------------------------------------------------
 * Pose recovery, perspective pipeline (sparse stage).  All f64 on the device (csrc/pose_kernels.hip).
 * tracks: n x m x 2 int32, (-1, -1) = no point; m <= CVHIP_TRIANGULATE_MAX_CAMERAS.  projections: m x 12 row-major
 * (3 x 4, calibrated), used where has_projection[j] != 0.  Host pointers unless stated. */

/* extend_tracks (triangulation.rs:1330-1419) with the grid add_image_pair_sparse builds from a pair's inliers
 * (:620-638): inliers n_inliers x 4 uint32 (x1, y1, x2, y2); cell (x1, y1) of the w1 x h1 image-1 grid = (x2, y2), a later
 * duplicate overwriting an earlier one.  Then as cvhip_extend_tracks: out_track_p2 per existing track, the remaining
 * cells as new tracks in scan order (at most cap written, *out_n_new = their number).  Integer only, bit-exact.  The cells
 * pack (x2, y2) in 16 bits each: image-2 coordinates 0..65534 (CVHIP_ERR_INVALID otherwise). */
int cvhip_extend_tracks_matches(cvhip_device *dev, const uint32_t *inliers, uint64_t n_inliers, uint32_t w1, uint32_t h1,
                                const int32_t *track_p1, uint64_t n_tracks, uint32_t max_dimension2, int32_t *out_track_p2,
                                uint32_t *out_new_p1, uint32_t *out_new_p2, uint64_t cap, uint64_t *out_n_new);

/* triangulate_tracks (triangulation.rs:867-911) with the images that have a projection: per track the DLT of its seen
 * views among them; out_ok[i] = 0 (None) with fewer than 2 such views or |w| < 1e-4, else out_points[i] = xyz / w. */
int cvhip_triangulate_tracks(cvhip_device *dev, const int32_t *tracks, uint64_t n, uint32_t m, const double *projections,
                             const uint8_t *has_projection, double *out_points, uint8_t *out_ok);

/* find_projection_matrix (triangulation.rs:940-994): E = K2^T F K1 projected onto diag(1, 1, 0); the candidates
 * (r1, u3), (r1, -u3), (r2, u3), (r2, -u3) of its SVD (3 x 3 SVDs on the host); each scored by the short tracks (n x 2 x 2
 * int32: the points in images 1 and 2) that triangulate with K1 [I | 0], K2 [r | t], have z > 0 and lie in front of
 * Camera::from_matrix(K2, r, t) (cheirality, on the device).  out_P2 = [r | t] (12, uncalibrated) of the highest count -
 * the LAST of equal counts, as Rust's max_by; the candidates' order follows the SVD's sign choices, so a tie between
 * candidates is not pinned - and *out_score = that count.  out_r2 (3, may be NULL): the r of Camera::from_matrix(K2, r, t)
 * for the winner - recover_next_cameras' camera 2 of the initial pair (:729-736); out_KP2 (12, may be NULL): K2 [r | t], the
 * projection it stores for that camera (:737-740). */
int cvhip_find_projection_matrix(cvhip_device *dev, const double *F, const double *K1, const double *K2,
                                 const int32_t *short_tracks, uint64_t n, double *out_P2, double *out_score, double *out_r2,
                                 double *out_KP2);

/* recover_pose (triangulation.rs:1033-1144): the P3P RANSAC (Nakano, BMVC 2019) for image `image_index` over its linked
 * tracks - the rows with ok[i] != 0 (points[i], n x 3, from cvhip_triangulate_tracks) and a point in that image, in table
 * order.  K^-1 is pseudo_inverse(K).  Up to 100 batches of 1000 hypotheses; hypothesis h of batch b draws its 3 samples
 * from the counter-based generator of DESIGN.md 4.9 keyed on (seed, b, h); each root of solve_quartic gives a pose whose
 * camera Camera::from_matrix(K, R, t) is checked on the 3 samples (RANSAC_INLIERS_T * max_dimension) and scored on all
 * linked tracks (count below RANSAC_T * max_dimension, error = the largest such error / count).  Best: higher count,
 * then lower error; on an exact tie the lowest (hypothesis, root), and the result carried from earlier batches before
 * any of a later batch.  Early exit after a batch with count >= 95 % of the linked tracks.  Out: out_r (3, the Camera's
 * r), out_t (3), out_projection (12) = K [matrix_r(r) | t], *out_count, *out_error, *out_batches, out_winner (3: batch,
 * hypothesis, root slot of the winner; -1 while the initial result is carried) - each may be NULL.
 * progress (may be NULL): 0.02 + 0.98 * hypotheses done / 100000 after every batch.
 * Errors: CVHIP_ERR_NO_SURFACE "Unable to find projection matrix" with fewer than 3 linked tracks or a final count not
 * above 70 % of them (the outputs then hold the best found). */
int cvhip_recover_pose(cvhip_device *dev, const int32_t *tracks, uint64_t n, uint32_t m, const double *points,
                       const uint8_t *ok, const double *projections, const uint8_t *has_projection, uint32_t image_index,
                       const double *K, uint32_t max_dimension, uint64_t seed, double *out_r, double *out_t,
                       double *out_projection, uint32_t *out_count, double *out_error, uint32_t *out_batches,
                       int32_t *out_winner, cvhip_progress_fn progress, void *user);

/* Test hook of recover_pose's hot path: B caller-chosen sample triples (sample_idx: 3 linked-track indices each) through
 * the same kernels.  Per sample and root slot (B x 4, the quartic's root order): out_pose 27 doubles (R 9, t 3, the
 * Camera's r 3, projection 12; NaN where the slot has no pose), out_status 0 = no pose, 1 = rejected by the 3-sample
 * check, 2 = scored; out_count / out_error the score (0 / NaN unless scored). */
int cvhip_recover_pose_models(cvhip_device *dev, const int32_t *tracks, uint64_t n, uint32_t m, const double *points,
                              const uint8_t *ok, const double *projections, const uint8_t *has_projection,
                              uint32_t image_index, const double *K, uint32_t max_dimension, const uint32_t *sample_idx,
                              uint32_t B, double *out_pose, int8_t *out_status, uint32_t *out_count, double *out_error);

/* ------------------------------------------------------------------------------------------
 * Mesh stage (output::output, src/output.rs:567-611; csrc/mesh_kernels.hip).  All f64 on the device, each
 * operation one IEEE operation in the reference's order.
 * The SURFACE is passed the same way to every entry: points (n x 3 f64), tracks (n x m x 2 int32, (-1, -1) = no point) -
 * host or device pointers - and per camera projection (m x 12 row-major), r (m x 3, the Camera's axis-angle), t (m x 3) and
 * image_dims (m x 2 uint32, width then height) in host memory: what triangulation's Surface holds.  m <=
 * CVHIP_TRIANGULATE_MAX_CAMERAS (CVHIP_ERR_UNSUPPORTED above; m = 0, an affine surface, is CVHIP_ERR_INVALID: the reference
 * skips culling for it).  Polygons (n_poly x 3 uint32 track indices) and the outputs named so are host or device
 * pointers; counts and statistics are host memory.  CVHIP_ERR_UNSUPPORTED with 2^32 - 1 or more tracks, polygons or cells.
 * A track projects to P (X, Y, Z, 1) divided by its third component unless that is below f64::EPSILON in magnitude
 * (Surface::project_point, triangulation.rs:63-74); it is IN RANGE when the projection lies in [c - 4 size, c + 4 size) on
 * both axes, c = size / 2 (img_range, output.rs:613-624); its depth is Camera::point_depth (triangulation.rs:492-495).
 * The Delaunay construction is cvhip_mesh_delaunay below (a caller may still supply triangles of its own: the other entries
 * take any).  Not here: the colour table (an argument of cvhip_mesh_colour_map).  The PLY and OBJ writers, the colour
 * mapping and the PNG encoder (cvhip_png_encode) are the mesh OUTPUT entries below.
 * Two of the reference's results depend on its thread order, and are DEFINED here:
 *  - DepthBuffer::new folds a cell's points in par_bridge's order, keeping a new depth iff cur - new > f64::EPSILON; here
 *    the cell is the MINIMUM of its depths (one of the reference's outcomes unless two depths of a cell differ by a
 *    non-zero amount <= EPSILON).  The depth image's cells are the MAXIMUM likewise.
 *  - process_camera sorts with sort_unstable and de-duplicates by vertices alone, so the camera of a triple that two
 *    cameras produce is not determined; here the LOWEST camera keeps it. */

/* lanes of one grid-stride launch of the mesh kernels (1024 blocks of 256): more polygons or tracks than this take more
 * than one trip of the loops */
#define CVHIP_MESH_GRID_LANES 262144
/* cvhip_mesh_set_wide_threshold's default (DESIGN.md 4.11 has the sweep behind it) */
#define CVHIP_MESH_WIDE_THRESHOLD_DEFAULT 2048

/* A polygon whose bounding box inside the buffer (rows x columns of the scanline walk's bounds) holds `pixels` or more is
 * not walked by its lane but queued for a wave, whose lanes take consecutive x of a row.  0 sends every polygon through
 * the wave path, UINT32_MAX none.  Both paths give the same flags and maps. */
int cvhip_mesh_set_wide_threshold(cvhip_device *dev, uint32_t pixels);

/* The Delaunay input of camera_i (Mesh::process_camera, output.rs:401-423): the tracks with a point in camera_i whose
 * projection is in range, in TRACK ORDER (the reference collects them in par_bridge's order).  out_index (uint32 track
 * index) and out_xy (2 f64) get the first `cap` of them, *out_n their number: cap = 0 sizes the buffers. */
int cvhip_mesh_camera_points(cvhip_device *dev, const double *points, const int32_t *tracks, uint64_t n, uint32_t m,
                             const double *projection, const double *r, const double *t, const uint32_t *image_dims,
                             uint32_t camera_i, uint32_t *out_index, double *out_xy, uint64_t cap, uint64_t *out_n);

/* DepthBuffer::new for camera_j (output.rs:262-318): over the tracks with a point in camera_j and a projection in range,
 * the grid is (ceil(max x) + 1) x (ceil(max y) + 1) (0 x 0 without such a track); a track goes to cell (round(x) as usize,
 * round(y) as usize) - half away from zero, saturating, so negative coordinates land in column or row 0 -; the cell is the
 * minimum of its depths.  out_buffer (width x height f64, NaN = None) is written when cap_cells >= width x height;
 * cap_cells = 0 sizes it.  (cvhip_mesh_cull builds the same buffers itself; this entry shows them.) */
int cvhip_mesh_depth_buffer(cvhip_device *dev, const double *points, const int32_t *tracks, uint64_t n, uint32_t m,
                            const double *projection, const double *r, const double *t, const uint32_t *image_dims,
                            uint32_t camera_j, double *out_buffer, uint64_t cap_cells, uint64_t *out_width,
                            uint64_t *out_height);

/* The culling of camera_i's polygons (Mesh::process_camera, output.rs:457-508): out_keep[p] = 0 iff polygon p obstructs in
 * some camera j != camera_i (polygon_obstructs, :320-353): its three vertices are projected into j with their depths,
 * stably sorted by y (total_cmp) and walked by ProjectedPolygon's scanline iterator (:107-254, restated with its quirks:
 * DESIGN.md 4.11) with max_x, max_y = the buffer's width and height; it obstructs iff some emitted pixel's cell is
 * occupied and cell - depth > f64::EPSILON.  out_stats (m x 5 uint64, may be NULL; row camera_i is zero): the buffer's
 * width, height and occupied cells, the polygons that obstruct in that camera, and the polygons sent to the wave path.
 * A vertex >= n: CVHIP_ERR_INVALID with nothing written. */
int cvhip_mesh_cull(cvhip_device *dev, const double *points, const int32_t *tracks, uint64_t n, uint32_t m,
                    const double *projection, const double *r, const double *t, const uint32_t *image_dims,
                    uint32_t camera_i, const uint32_t *polygons, uint64_t n_poly, uint8_t *out_keep, uint64_t *out_stats);

/* The polygon list of Mesh::create (output.rs:50-105, 384, 510-516) from the cameras' kept polygons, concatenated, with
 * the camera of each: Polygon::new's rotation (the smallest vertex first, orientation kept), sorted by vertices and
 * de-duplicated by vertices alone - the lowest camera keeps a shared triple -, then grouped by camera (stable).  Host C++
 * inside the library (not a hot path).  out_polygons (n_poly x 3), out_camera (n_poly): room for n_poly; *out_n written. */
int cvhip_mesh_merge(cvhip_device *dev, const uint32_t *polygons, const uint32_t *camera, uint64_t n_poly,
                     uint32_t *out_polygons, uint32_t *out_camera, uint64_t *out_n);

/* ImageWriter (output.rs:1016-1143) without the colour table and the encoder: every track is projected to
 * project_to_image (visibility is not required; out of range = None); with min / max x / y over the rest, width =
 * (ceil(max_x) - floor(min_x)) as usize + 1, height likewise; each vertex is placed at (x - min_x, y - min_y, depth *
 * scale) (scale = +-1: out_scale.2.signum()) and splatted at its rounded position clamped into the map; each polygon
 * whose three vertices are Some is rasterised by the scanline iterator with max_x, max_y = width - 1, height - 1 (so the
 * last row and column never receive face pixels); a cell keeps the MAXIMUM.  out_map (width x height f64, NaN = None) is
 * written when cap_cells >= width x height; cap_cells = 0 sizes it (width, height and origin are returned either way).
 * out_origin[2] = (min_x, min_y), out_minmax[2] = the map's smallest and largest depth, *out_wide = polygons sent to the
 * wave path (each may be NULL).  Errors: CVHIP_ERR_NO_SURFACE "No point projections found" (:1046) when no projection is
 * in range; CVHIP_ERR_INVALID for a vertex >= n (nothing written). */
int cvhip_mesh_depth_image(cvhip_device *dev, const double *points, const int32_t *tracks, uint64_t n, uint32_t m,
                           const double *projection, const double *r, const double *t, const uint32_t *image_dims,
                           uint32_t project_to_image, double scale, const uint32_t *polygons, uint64_t n_poly,
                           double *out_map, uint64_t cap_cells, uint64_t *out_width, uint64_t *out_height,
                           double *out_origin, double *out_minmax, uint64_t *out_wide);

/* cvhip_mesh_delaunay_set_lane_cells' default: a GUESS until measured (tests/tools/bench_delaunay.py
 * sweeps it; on a jittered lattice a star visits about 85 cells, and about 1 star in 2000 - hull points - more than this) */
#define CVHIP_MESH_DELAUNAY_LANE_CELLS_DEFAULT 1024
/* out_stats of cvhip_mesh_delaunay: uint64 values */
#define CVHIP_DELAUNAY_STAT_GRID_WIDTH 0   /* cells of the uniform grid along x */
#define CVHIP_DELAUNAY_STAT_GRID_HEIGHT 1  /* and along y */
#define CVHIP_DELAUNAY_STAT_DEVICE_STARS 2 /* stars finished on the device */
#define CVHIP_DELAUNAY_STAT_HOST_STARS 3   /* stars finished on the exact host path */
#define CVHIP_DELAUNAY_STAT_DUPLICATES 4   /* points at the position of a lower index */
#define CVHIP_DELAUNAY_STAT_MOST_CELLS 5   /* the largest number of grid cells one device star visited */
#define CVHIP_DELAUNAY_STATS 6

/* The Delaunay triangulation of a camera's points (DelaunayTriangulation::bulk_load in Mesh::process_camera, output.rs:425;
 * DESIGN.md 4.13; csrc/delaunay_kernels.hip, csrc/delaunay_common.hpp).  xy: k points of 2 finite f64 - a camera's points
 * in track order, as cvhip_mesh_camera_points writes them.  out_faces: the faces of the Delaunay triangulation of the
 * DISTINCT positions, 3 uint32 positions in xy each, DEFINED as follows:
 *  - every decision is the sign of the EXACT orientation or in-circle determinant of the doubles as given (the device
 *    certifies a rounded determinant against its forward error bound; what it cannot certify is decided on the host with
 *    floating-point expansions), so without exact ties this is THE Delaunay triangulation, the reference's (spade's) too;
 *  - a face (a, b, c) is counter-clockwise, (xb - xa)(yc - ya) - (yb - ya)(xc - xa) > 0 (spade's vertices() order), and
 *    starts with its smallest index (Polygon::new's rotation);
 *  - exact ties: a maximal set of four or more points on one circle with no point strictly inside is a convex polygon; it
 *    is fanned from its vertex with the LOWEST index (the reference leaves this to spade's insertion order);
 *  - duplicates: of several indices at one position the lowest is the vertex, the others are in no face;
 *  - k < 3, or all points collinear: 0 faces, CVHIP_OK.
 * FACE ORDER: grouped by the face's first (lowest) index, ascending; within a group in the order of that point's star -
 * counter-clockwise from the point's nearest point (of equally near ones the lowest index) and, at a point of the convex
 * hull, then clockwise from it.  Deterministic: two calls on the same input give the same bytes.
 * xy and out_faces are host or device pointers; the counts and out_stats (CVHIP_DELAUNAY_STATS uint64, may be NULL: the
 * CVHIP_DELAUNAY_STAT_* values; which path finishes a star whose signs are near zero may depend on the order of the grid's
 * atomics, the faces do not) are host memory.  *out_n_faces is always written on success; cap_faces = 0 sizes the output
 * and writes no face; 0 < cap_faces < n_faces is CVHIP_ERR_INVALID with nothing written; 2 k is always enough.
 * Errors: CVHIP_ERR_INVALID for a coordinate that is not finite (nothing written); CVHIP_ERR_UNSUPPORTED for k >= 2^31
 * (the face count must stay below 2^32 - 1; so k >= 2^32 - 1 too).  The signs are exact while no product of coordinate
 * differences over- or underflows (differences within 2^-240 .. 2^240 in magnitude).
 * Integer lattices (the camera points of an affine surface): every star meets an exact tie, so with
 * cvhip_mesh_delaunay_set_lattice off every star runs on the host; with it on the device decides them in integers. */
int cvhip_mesh_delaunay(cvhip_device *dev, const double *xy, uint64_t k,
                        uint32_t *out_faces, uint64_t cap_faces, uint64_t *out_n_faces, uint64_t *out_stats);

/* A device star that would visit more than `cells` grid cells is left to the host path, so that one long star cannot hold
 * its wave: 0 sends every star to the host path, UINT32_MAX never leaves the device for size.  Every setting gives the same
 * faces. */
int cvhip_mesh_delaunay_set_lane_cells(cvhip_device *dev, uint32_t cells);

/* The lattice kernels: when `on` is not 0 and EVERY coordinate of a call is an integer with |v| <= 2^24
 * (decided per call, on the device, with the extent), the stars are built by kernels whose predicates go on, below the f64
 * filter, with the exact integer determinant (64-bit for orientation and distance, 128-bit for in-circle): ties are decided
 * on the device by the tie rule above, and only duplicates, stars past lane_cells and stars with more than 64 neighbours
 * still go to the host.  Any other input, and every input when off, runs the filtered kernels.  The faces are the same bytes
 * either way; only CVHIP_DELAUNAY_STAT_DEVICE_STARS / _HOST_STARS / _MOST_CELLS move (lattice stars count as device stars).
 * The default is CVHIP_MESH_DELAUNAY_LATTICE_DEFAULT: off, so that a call computes and reports what it did before this
 * switch existed; reconstruct_affine_mesh's triangulator switches it on. */
#define CVHIP_MESH_DELAUNAY_LATTICE_DEFAULT 0
int cvhip_mesh_delaunay_set_lattice(cvhip_device *dev, int on);
/* *out_on = 1 when the switch is on, 0 when off */
int cvhip_mesh_delaunay_get_lattice(cvhip_device *dev, int *out_on);
/* *out_stars = the stars of this device's last cvhip_mesh_delaunay call that its lattice kernels finished; 0 when that
 * call did not qualify (or failed before its stars were built) */
int cvhip_mesh_delaunay_get_lattice_stars(cvhip_device *dev, uint64_t *out_stars);

/* ------------------------------------------------------------------------------------------
 * Mesh output (csrc/mesh_output_kernels.hip): what output::output writes once the polygon list exists -
 * PlyWriter's binary file image (output.rs:648-772) and ImageWriter::complete's colour mapping (:1117-1229) -, pinned
 * byte for byte.  Neither touches the cameras: an affine surface works the same, and m is the number of images per track.
 * The OBJ writer, with its vt / UV tables, is cvhip_mesh_obj further below, the PNG encoder cvhip_png_encode. */

/* VertexMode (output.rs): what a vertex carries.  In a PLY, Texture writes what Plain writes; in an OBJ it adds the vt table. */
#define CVHIP_VERTEX_PLAIN 0
#define CVHIP_VERTEX_COLOR 1
#define CVHIP_VERTEX_TEXTURE 2

/* The binary PLY file image of Mesh::output with a PlyWriter (:521-559, :648-772): the header (:687-710; 198 + digits(n) +
 * digits(n_poly) bytes, 60 more in Color mode, composed on the host), one record per track in track order, one per polygon
 * in list order.
 *  - vertex (:712-750): x * sx, (-y) * sy, z * sz (out_scale[3]; the negation first, then one multiply: y = 0 gives -0.0)
 *    as 8 big-endian bytes each; NaN coordinates are written as their bytes.  In Color mode the pixel of the track's first
 *    present point - the lowest image c with tracks[i][c].x >= 0 - follows as 3 bytes IF get_pixel_checked finds it: a point
 *    with x >= width or y >= height of its image gets none, and its record is 24 bytes, not 27 (the reference's file).  A
 *    track without any point is the reference's error "Track has no images" in Color mode only.
 *  - face (:752-763): 0x03, then big-endian uint32 of vertices[2], vertices[1], vertices[0].
 * points (n x 3 f64), tracks (n x m x 2 int32; read in Color mode only), polygons (n_poly x 3 uint32), images and out are host
 * or device pointers; image_offsets, image_dims, out_scale and the counts are host memory.  images: the m RGB8 images
 * concatenated, row-major, 3 bytes per pixel; image_offsets: m + 1 byte offsets into it; image_dims: m x 2, width then height
 * (an image shorter than width x height x 3 bytes is CVHIP_ERR_INVALID).  They are read in Color mode only, where images =
 * NULL is CVHIP_ERR_INVALID.  vertex_mode: CVHIP_VERTEX_*; any other value is CVHIP_ERR_INVALID.
 * *out_size = the size of the file image, out_sections[3] (may be NULL) = the header's, the vertices' and the faces' bytes.
 * cap = 0 sizes the image and writes nothing (in Color mode it runs the counting pass, and reports a track without points);
 * 0 < cap < size is CVHIP_ERR_INVALID.  n = 0 and n_poly = 0 give the header alone.
 * Errors, each with nothing written: CVHIP_ERR_INVALID "Track has no images" (Color mode: a track without a point, or m = 0
 * with n > 0), CVHIP_ERR_INVALID for a vertex >= n, CVHIP_ERR_UNSUPPORTED for 2^32 - 1 or more tracks or polygons. */
int cvhip_mesh_ply(cvhip_device *dev, const double *points, const int32_t *tracks, uint64_t n, uint32_t m,
                   const uint8_t *images, const uint64_t *image_offsets, const uint32_t *image_dims,
                   uint32_t vertex_mode, const double *out_scale,
                   const uint32_t *polygons, uint64_t n_poly,
                   uint8_t *out, uint64_t cap, uint64_t *out_size, uint64_t *out_sections);

/* ImageWriter::complete's colour mapping (:1117-1143, map_depth / map_color :1146-1229) of a depth map as
 * cvhip_mesh_depth_image writes it (width x height f64, NaN = None) with its min_depth / max_depth: a None cell gives
 * (0, 0, 0, 0); otherwise value = (depth - min) / (max - min) and per channel table[255] if value >= 1, else with step =
 * 1 / 255: box = clamp(floor(value / step) as usize, 0, 254), ratio = (value - step * box) / step, round(c2 * ratio + c1 *
 * (1 - ratio)) as u8 (c1, c2 = table[box], table[box + 1]; half away from zero; the casts saturate, NaN -> 0), alpha 255.
 * All f64, one IEEE operation per written operation.  A constant map (max = min) gives (0, 0, 0, 255) in every Some cell.
 * table (host memory): 256 x 3 bytes, R, G, B per entry - the library ships none.  map and out_rgba (width x height x 4
 * bytes, 4-byte aligned) are host or device pointers; CVHIP_ERR_UNSUPPORTED with 2^32 - 1 or more cells. */
int cvhip_mesh_colour_map(cvhip_device *dev, const double *map, uint64_t width, uint64_t height,
                          double min_depth, double max_depth, const uint8_t *table, uint8_t *out_rgba);

/* ------------------------------------------------------------------------------------------
 * The Wavefront OBJ file image (csrc/mesh_obj_kernels.hip, csrc/f64_display.hpp): Mesh::output with an
 * ObjWriter (output.rs:521-559, 774-1007), byte for byte.  Every number is Rust's `{}`: an f64 as the shortest decimal digits
 * that read back as the same double, laid out without an exponent ("NaN", "inf", "-inf", "0", "-0"; 1e23 is 1 and 23 zeros,
 * 5e-324 is 326 characters).  Every line ends with '\n'; in this order:
 *  - header (:877-889): "mtllib {stem}.mtl" in Texture mode, nothing otherwise (composed on the host);
 *  - v (:891-936), one per track in track order: "v {x * sx} {(-y) * sy} {z * sz}" (the PLY's arithmetic: y = 0 prints -0); in
 *    Color mode " {r / 255} {g / 255} {b / 255}" of the track's first present point follows iff get_pixel_checked finds it;
 *  - vt (:938-969), Texture mode only: per track, and per present point in image order, "vt {x / width} {1 - y / height}" with x,
 *    y, width, height as u32 turned into f64.  No bounds test: a point past its image prints u above 1, a zero width inf or NaN;
 *  - f (:971-997), one per polygon in list order: "f" and for i in 2, 1, 0 " {vertices[i] + 1}", in Texture mode
 *    " {vertices[i] + 1}/{uv + 1}" with uv = (the present points of the tracks before vertices[i]) + (that track's present
 *    points among the images below the polygon's camera; a camera >= m counts all of them).  In Texture mode
 *    "usemtl Textured{camera}" goes before polygon 0 and before every polygon whose camera differs from its predecessor's.
 * Arguments as cvhip_mesh_ply's, plus polygon_cameras (n_poly x uint32, host or device; read in Texture mode, where NULL with
 * n_poly > 0 is CVHIP_ERR_INVALID) and stem (the output path's file stem; read in Texture mode, where NULL is
 * CVHIP_ERR_INVALID).  tracks are read in Color and Texture mode, images and image_offsets in Color mode only, image_dims in
 * both (Texture mode takes images = NULL).  out_sections[4] (may be NULL) = the header's, v, vt and f bytes.
 * cap = 0 sizes the image - it runs the length pass, whose per-block byte counts go through a 64-bit scan - and writes nothing;
 * 0 < cap < size is CVHIP_ERR_INVALID with nothing written.  n = 0 and n_poly = 0 give the header alone (an empty image
 * outside Texture mode).
 * Errors, each with nothing written: CVHIP_ERR_INVALID "Track has no images" (Color and Texture mode: a track without a point,
 * or m = 0 with n > 0; Plain mode accepts such a track), CVHIP_ERR_INVALID for a vertex >= n, CVHIP_ERR_UNSUPPORTED for 2^32 - 1
 * or more tracks or polygons, or n * m >= 2^32 - 1 in Color and Texture mode.  The {stem}-{i}.png images the .mtl names are
 * cvhip_png_encode's, one call per image. */
int cvhip_mesh_obj(cvhip_device *dev, const double *points, const int32_t *tracks, uint64_t n, uint32_t m,
                   const uint8_t *images, const uint64_t *image_offsets, const uint32_t *image_dims,
                   uint32_t vertex_mode, const double *out_scale,
                   const uint32_t *polygons, const uint32_t *polygon_cameras, uint64_t n_poly, const char *stem,
                   uint8_t *out, uint64_t cap, uint64_t *out_size, uint64_t *out_sections);

/* The {stem}.mtl text of ObjWriter::write_materials (:856-868) for m images: per image "newmtl Textured{i}", the five fixed
 * lines, "map_Ka {stem}-{i}.png", "map_Kd {stem}-{i}.png" and an empty line.  Host memory only, no device.  cap = 0 sizes;
 * 0 < cap < size is CVHIP_ERR_INVALID. */
int cvhip_mesh_obj_mtl(const char *stem, uint32_t m, char *out, uint64_t cap, uint64_t *out_size);

/* Rust's `{}` of each of n doubles, concatenated without separators, formatted on the device (the formatter of
 * cvhip_mesh_obj): value i's text is out[offsets[i] .. offsets[i + 1]).  values, out and offsets (n + 1 x uint64, may be NULL)
 * are host or device pointers.  cap = 0 sizes (*out_size) and writes nothing; 0 < cap < size is CVHIP_ERR_INVALID;
 * CVHIP_ERR_UNSUPPORTED with 2^32 - 1 or more values. */
int cvhip_f64_display(cvhip_device *dev, const double *values, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_size,
                      uint64_t *offsets);

/* ------------------------------------------------------------------------------------------
 * The PNG file image (csrc/png_kernels.hip, csrc/png_common.hpp): what the reference saves with img.save - the
 * {stem}-{i}.png textures of an OBJ (output.rs:845-875: 8-bit RGB, colour type 2) and ImageWriter's depth map (:1141: 8-bit
 * RGBA, colour type 6) - made on the device.  The reference's encoder is not restated: every decoder returns the same pixels,
 * the bytes are DEFINED here (tests/ref_png.py is the definition), deterministically:
 *  - the signature; IHDR: width, height, depth 8, colour type 0 / 4 / 2 / 6 for channels 1 / 2 / 3 / 4, compression 0,
 *    filter 0, interlace 0; ONE IDAT; IEND.  No other chunk;
 *  - the IDAT data: 78 01, one deflate block (BFINAL = 1, dynamic Huffman), the Adler-32 of the filtered bytes;
 *  - filtered bytes: per row the filter's number and width * channels bytes under that filter (bpp = channels).  filter 0 to 4
 *    (CVHIP_PNG_FILTER_NONE .. _PAETH): that filter on every row.  CVHIP_PNG_FILTER_ADAPTIVE: per row the filter with the
 *    least sum over its filtered bytes of (v < 128 ? v : 256 - v), the lowest number on equal sums;
 *  - tokens, per row (nothing crosses a row): byte 0 is a literal; position i >= 1 repeats iff it equals byte i - 1; of every
 *    maximal run of L repeating positions: while L >= 3 a match of min(L, 258) at distance 1, the remaining 0 to 2 literals;
 *    the end-of-block symbol behind the last row;
 *  - codes: lengths by package-merge over the whole image's literal/length counts, limit 15 (leaves sorted by (count,
 *    symbol); in the merges a leaf goes before a package of equal weight); canonical codes; HLIT = the highest used symbol + 1;
 *    HDIST = 1 with one distance code of one bit; the HLIT + 1 code lengths sent as themselves (no symbols 16 to 18), their
 *    code by the same routine with limit 7, HCLEN up to the last non-zero entry and at least 4.
 * pixels (height x width x channels bytes, rows packed) and out are host or device pointers, out of any alignment.
 * out_sections[3] (may be NULL) = the bytes before the IDAT data (41), the IDAT data, the bytes after it (16).
 * cap = 0 sizes the image - it filters, counts, gets the code from the host and scans the rows' bits - and writes nothing;
 * 0 < cap < size is CVHIP_ERR_INVALID with nothing written.  CVHIP_ERR_INVALID too: width or height 0, channels not 1 to 4,
 * filter above 5.  CVHIP_ERR_UNSUPPORTED: 2^32 - 1 or more filtered bytes, or IDAT data of 2^31 or more bytes.  There is no
 * stored-block fallback: noise grows by the code's overhead.  Not here: interlacing, 16-bit and palette images, ancillary
 * chunks, matches at other distances, decoding. */
#define CVHIP_PNG_FILTER_NONE 0u
#define CVHIP_PNG_FILTER_SUB 1u
#define CVHIP_PNG_FILTER_UP 2u
#define CVHIP_PNG_FILTER_AVERAGE 3u
#define CVHIP_PNG_FILTER_PAETH 4u
#define CVHIP_PNG_FILTER_ADAPTIVE 5u
int cvhip_png_encode(cvhip_device *dev, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels, uint32_t filter,
                     uint8_t *out, uint64_t cap, uint64_t *out_size, uint64_t *out_sections);

/* ------------------------------------------------------------------------------------------
 * JPEG files out (csrc/jpeg_encode_kernels.hip, csrc/jpeg_encode_common.hpp): the fourth kind of output file
 * of the reference - "if the filename ends with .jpg, this will save a JPEG depth map file" - which reaches every image format
 * through one img.save (src/output.rs:1141).  The file is DEFINED as libjpeg's (tests/ref_jpeg_out.py restates it and is pinned
 * to Pillow on libjpeg-turbo byte for byte): SOI, APP0 JFIF 1.01 (no units, 1:1), a DQT per table (the Annex K tables scaled by
 * the quality as jpeg_set_quality does, clamped to 1 .. 255), SOF0, a DHT per table (DC0, AC0, DC1, AC1), SOS, the data, EOI.
 *  - 1 channel is one component; 3 channels become Y, Cb, Cr by jccolor's fixed-point formulas; the second of 2 and the fourth
 *    of 4 channels (alpha) is dropped, so a depth-map cell without a depth, (0, 0, 0, 0), comes out black;
 *  - sampling: luma 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0) over 1x1 chroma; a one-component image ignores it (its SOF0
 *    says 1x1);  h2v1 is (a + b + bias) >> 1 with bias 0, 1, 0, 1, ..., h2v2 (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2, ...;
 *    the source row is replicated to the right before the downsampling, at the bottom the source is padded to a multiple of
 *    the vertical factor and the DOWNSAMPLED rows are replicated below that; a luma block of an edge MCU that lies beyond the
 *    component has no AC and the DC of the block before it;
 *  - jfdctint (CONST_BITS 13, PASS1_BITS 2) on samples minus 128, quantised by sign(c) * ((|c| + (8 q >> 1)) / (8 q));
 *  - one interleaved scan without restart markers, one-bits pad the last byte, a 00 follows every FF byte of the data;
 *  - optimize = 0: the Annex K Huffman tables.  optimize = 1: libjpeg's jpeg_gen_optimal_table per table from the scan's own
 *    counts (one round trip to the host); counts are not capped and code lengths of any depth are folded down to 16.
 * pixels (height x width x channels bytes, rows packed) and out are host or device pointers, out of any alignment.
 * out_sections[3] (may be NULL) = the bytes before the scan's data, the data, the bytes after it (2).
 * cap = 0 sizes the image - everything but the last copy runs, since the size is known only when the FF bytes are counted -
 * and writes nothing; 0 < cap < size is CVHIP_ERR_INVALID with nothing written.  CVHIP_ERR_INVALID too: width or height 0 or
 * above 65535, channels not 1 to 4, quality not 1 to 100, sampling above 2, optimize above 1.  CVHIP_ERR_UNSUPPORTED: more
 * than 2^25 blocks.  Not here: restart markers, progressive and arithmetic coding, 12 bits, EXIF; the OBJ writer's textures
 * stay PNG. */
#define CVHIP_JPEG_SAMPLING_444 0u /* Pillow's subsampling numbers */
#define CVHIP_JPEG_SAMPLING_422 1u
#define CVHIP_JPEG_SAMPLING_420 2u
int cvhip_jpeg_encode(cvhip_device *dev, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels, uint32_t quality,
                      uint32_t sampling, uint32_t optimize, uint8_t *out, uint64_t cap, uint64_t *out_size, uint64_t *out_sections);
/* Of the calling thread's last cvhip_jpeg_encode that sized or wrote a file: out_stats[4] = blocks, dummy blocks, the bits of
 * the data before padding and stuffing, the 00 bytes stuffed in. */
int cvhip_jpeg_encode_last_stats(uint64_t *out_stats);

/* ------------------------------------------------------------------------------------------
 * TIFF files out (csrc/tiff_encode_kernels.hip, csrc/tiff_encode_common.hpp): img.save (src/output.rs:1141)
 * of a depth map whose path ends in .tif, and the format of the SEM pairs cvhip_tiff_decode reads.  The file is DEFINED here
 * (tests/ref_tiff_out.py; the `image` crate's encoder is not restated): classic little-endian TIFF - II, 42, the one IFD at
 * offset 8 - with the entries 256 ImageWidth and 257 ImageLength (LONG), 258 BitsPerSample (`channels` SHORTs of 8), 259
 * Compression, 262 Photometric (1 for 1 or 2 channels, 2 for 3 or 4), 273 StripOffsets (LONG), 277 SamplesPerPixel, 278
 * RowsPerStrip (LONG), 279 StripByteCounts (LONG), 284 PlanarConfiguration 1, 317 Predictor only when it is 2, 338 ExtraSamples 2
 * (unassociated alpha) only for 2 or 4 channels; values of 4 bytes or less inline, the others behind the IFD in tag order;
 * then the strips in order, each at an even offset (a 0 byte pads the strip in front); nothing else.
 *  - rows_per_strip = 0 is max(1, 8192 / row_bytes) (TIFF 6.0's "about 8 KB"); any other value is clamped to height;
 *  - compression 1: the rows;  32773 PackBits: row by row, greedily - from the position the maximal run of equal bytes (at most
 *    128), 3 or more a run packet, otherwise a literal packet up to where three equal bytes begin, 128 bytes or the row's end
 *    (not libtiff's packets; any PackBits reader returns the rows);  5 LZW: TIFF 6.0's as libtiff writes it byte for byte -
 *    MSB-first codes, a Clear first, greedy longest match, the early change of the code width, a Clear after 3836 codes (also
 *    when that code is the strip's last, in front of EOI), EOI, zero bits to the byte's end;
 *  - predictor 2 (LZW only): each byte minus the byte `channels` before it in its row, modulo 256.
 * pixels (height x width x channels bytes, rows packed) and out are host or device pointers, out of any alignment.
 * out_sections[3] (may be NULL) = the bytes before the first strip, the strips with their padding, the bytes after (0).
 * cap = 0 sizes the file and writes nothing; 0 < cap < size is CVHIP_ERR_INVALID with nothing written.  CVHIP_ERR_INVALID too:
 * width or height 0, channels not 1 to 4, a compression other than 1, 5 or 32773, predictor not 1 or 2, predictor 2 without
 * LZW.  CVHIP_ERR_UNSUPPORTED: a dimension of 65536 or more, a file of 2^32 bytes or more, a strip of 2^31 bytes or more.
 * Not here: 16-bit samples, tiles, BigTIFF, Deflate, SEM metadata out, EXIF out. */
#define CVHIP_TIFF_COMPRESSION_NONE 1u
#define CVHIP_TIFF_COMPRESSION_LZW 5u
#define CVHIP_TIFF_COMPRESSION_PACKBITS 32773u
int cvhip_tiff_encode(cvhip_device *dev, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels,
                      uint32_t compression, uint32_t predictor, uint32_t rows_per_strip,
                      uint8_t *out, uint64_t cap, uint64_t *out_size, uint64_t *out_sections);
/* Of the calling thread's last cvhip_tiff_encode that sized or wrote a file: out_stats[4] = strips, LZW codes written (Clears
 * and EOIs included), Clear codes written, PackBits packets. */
int cvhip_tiff_encode_last_stats(uint64_t *out_stats);
/* Of the same call, for measurements (tests/tools/bench_tiff_out.py): out_ticks[3] = the ticks of the device's 100 MHz clock that
 * the LZW waves spent loading their strips' bytes, on the serial walk against the table, and packing the codes - each summed
 * over the strips, which run side by side, so the three give the shares of the LZW kernel's time, not its length.  0 without LZW. */
int cvhip_tiff_encode_last_phases(uint64_t *out_ticks);

/* ------------------------------------------------------------------------------------------
 * JPEG files in (csrc/jpeg_kernels.hip, csrc/jpeg_common.hpp): what the reference opens with
 * image::open(path)?.into_luma8() / into_rgb8() and crops by databar_height (src/reconstruction.rs:40-60), and the EXIF
 * FocalLengthIn35mmFilm it reads (:138-142).  The host walks the markers; the entropy decode and everything behind it runs on
 * the device.  The `image` crate's decoder is not restated: the pixels are DEFINED here (tests/ref_jpeg.py is the definition)
 * as libjpeg's default decode - sequential Huffman, jidctint (CONST_BITS 13, PASS1_BITS 2; here in 64-bit integers with a
 * clamp), fancy upsampling (replication where a chroma plane has at most 2 columns), the fixed-point YCbCr -> RGB - and are
 * what libjpeg-turbo returns for every file an encoder makes.  Luma8 of a colour file is (2126 r + 7152 g + 722 b) / 10000,
 * truncated, of that RGB (into_luma8 as remembered, not pinned to the crate); of a grey file its plane.  EXIF orientation is
 * not applied (image::open does not apply it).
 * Supported: SOF0, 8 bits, 1 component or 3 (YCbCr) in one interleaved scan, luma sampling 1x1, 2x1 or 2x2 over 1x1 chroma, any
 * DRI or none, any number of DQT / DHT segments before the scan, APPn and COM skipped, FF fill in front of a marker.
 * CVHIP_ERR_UNSUPPORTED: every other SOF, 12 bits, 2 or 4 components, an Adobe transform other than YCbCr, a second scan,
 * other sampling factors, DNL (a frame height of 0 announces it); a scan of 2^31 or more bytes, more than 2^25 blocks.
 * CVHIP_ERR_INVALID: anything malformed - a truncated segment, a missing table, a code that is not in its table, a run past
 * coefficient 63, a missing, surplus or misnumbered RSTn, data that ends before the last MCU, width 0, drop_rows >= height;
 * nothing is written then. */
#define CVHIP_IMAGE_LUMA8 0u
#define CVHIP_IMAGE_RGB8 1u
/* Host only, no device.  out_info[6] = width, height, components (1 or 3), the luma sampling factors h and v, and
 * FocalLengthIn35mmFilm (APP1 "Exif", either byte order, IFD0 -> 0x8769 -> 0xA405 as SHORT or LONG; 0 = none: a missing or
 * broken EXIF block is none, as get_metadata falls back, reconstruction.rs:62-73). */
int cvhip_jpeg_info(const uint8_t *file, uint64_t size, uint32_t *out_info);
/* file[0 .. size): the JPEG file in host memory.  out: width x (height - drop_rows) pixels of 1 (CVHIP_IMAGE_LUMA8) or 3
 * (CVHIP_IMAGE_RGB8: a grey file's plane three times) bytes, rows packed, in host or device memory at any alignment;
 * drop_rows rows are cut from the bottom (the reference's databar_height).  cap = 0 sizes (*out_size, from the header alone)
 * and writes nothing; 0 < cap < size is CVHIP_ERR_INVALID with nothing written. */
int cvhip_jpeg_decode(cvhip_device *dev, const uint8_t *file, uint64_t size, uint32_t format, uint32_t drop_rows, uint8_t *out,
                      uint64_t cap, uint64_t *out_size);
/* Of the calling thread's last cvhip_jpeg_decode that reached the device: out_stats[4] = restart intervals, subsequences,
 * launches of the synchronisation kernel, the most rounds a workgroup needed within a launch. */
int cvhip_jpeg_last_stats(uint64_t *out_stats);

/* ------------------------------------------------------------------------------------------
 * Progressive JPEG files in (csrc/jpeg_prog_kernels.hip, csrc/jpeg_prog_common.hpp): the SOF2 files that
 * cvhip_jpeg_decode refuses and image::open decodes - mozjpeg's and jpegtran's output, most of the web's photographs.  The pixels
 * are DEFINED (tests/ref_jpeg_prog.py is the definition, pinned to Pillow) as libjpeg's default decode of the whole file: the
 * coefficients accumulate over all scans as jdphuff.c does - DC first and refinement, AC first with EOB runs, AC refinement with
 * its correction bits - and go through the path above unchanged: dequantisation, jidctint, fancy upsampling, YCbCr -> RGB, luma.
 * The host walks the markers of the whole file and checks the progression; the cut of the scans at their RSTn markers, the
 * entropy decode of every scan and everything behind it run on the device.
 * Supported: SOF2, 8 bits, 1 or 3 components with the sampling factors above; Ss, Se, Ah, Al as T.81 G.1 allows (a DC scan
 * of 1 to 3 components with Ss = Se = 0, an AC scan of one component with 1 <= Ss <= Se <= 63, Ah = 0 in a first scan, in a
 * refinement Ah = the Al every coefficient of the band was last sent with and Al = Ah - 1, Al <= 13, a component's AC scans
 * behind a DC scan of it); any DRI, which may change between scans; DHT and DQT segments anywhere before or between scans (a
 * component keeps the quantisation table in force at its first scan); at most 256 scans.
 * CVHIP_ERR_UNSUPPORTED: a frame that is not SOF2 - a baseline file too: that is cvhip_jpeg_decode's, and a sequential file of
 * several scans is not built -; an incomplete progression, that is one that ends with one of a component's coefficients 0 .. 9
 * (zig-zag order) unsent or not refined down to Al = 0 (there libjpeg smooths between blocks, differently from version to
 * version; whatever is missing or unrefined of 10 .. 63 stays as sent); more than 256 scans; a file of 2^31 or more bytes, more
 * than 2^25 blocks; and what cvhip_jpeg_decode refuses of a frame (12 bits, DNL, 2 or 4 components, other sampling factors).
 * CVHIP_ERR_INVALID: anything malformed - a scan header outside the rules above, s > 1 in a refinement (libjpeg warns and
 * reads 1), a run past Se, a code that is not in its table, a missing, surplus or misnumbered RSTn, a scan whose data ends
 * before its last block, a truncated segment, a missing table; nothing is written then.  What follows a scan's last block is
 * ignored. */
/* Host only, no device.  out_info[7] = cvhip_jpeg_info's six words and the number of scans. */
int cvhip_jpeg_progressive_info(const uint8_t *file, uint64_t size, uint32_t *out_info);
/* cvhip_jpeg_decode's arguments and contract for a progressive file: cap = 0 sizes and writes nothing (the whole file is
 * walked and the progression checked, on the host), 0 < cap < size is CVHIP_ERR_INVALID with nothing written, out in host or
 * device memory at any alignment. */
int cvhip_jpeg_progressive_decode(cvhip_device *dev, const uint8_t *file, uint64_t size, uint32_t format, uint32_t drop_rows, uint8_t *out,
                                  uint64_t cap, uint64_t *out_size);
/* Of the calling thread's last cvhip_jpeg_progressive_decode that reached the device: out_stats[8] = scans, restart intervals
 * (of all scans), subsequences (the 1024-bit units of all scans' data, counted on the device), launches of the synchronisation
 * kernel that settles the DC-first and AC-first scans, the most rounds a workgroup needed within a launch, AC-refinement
 * scans, launches that hold one, the longest EOB run. */
int cvhip_jpeg_progressive_last_stats(uint64_t *out_stats);

/* ------------------------------------------------------------------------------------------
 * TIFF files in (csrc/tiff_kernels.hip, csrc/tiff_common.hpp): the reference's SEM pairs
 * (--projection=parallel), opened like every input with image::open(path)?.into_luma8() / into_rgb8() and cropped by the
 * DatabarHeight of the microscope's text block in tag 34683 or 34682 (src/reconstruction.rs:40-60, 80-144).  The host walks the
 * first IFD of a classic TIFF file (II or MM) and reads the block; decompression, Predictor 2 and the conversion run on the
 * device, a wave per strip.  The pixels are DEFINED by tests/ref_tiff.py: the decompressed samples are libtiff's (pinned to
 * Pillow); 16 -> 8 bits is (v + 128) / 257, Luma8 of RGB is (2126 r + 7152 g + 722 b) / 10000 truncated (of 16-bit samples
 * in 16 bits, then reduced), WhiteIsZero is inverted and a fourth sample dropped - into_luma8 / into_rgb8 as remembered, not
 * pinned to the `image` crate.
 * Supported: strips, PlanarConfiguration 1, 8 or 16 bits (unsigned integers), 1 sample (photometric 0 or 1), 3 or 4 samples
 * (photometric 2), compression 1, 5 (LZW) and 32773 (PackBits), Predictor 1 or 2, strips anywhere in the file in any order.
 * CVHIP_ERR_UNSUPPORTED: BigTIFF, tiles, PlanarConfiguration 2, other depths or sample formats, palette / CMYK / YCbCr / CIELab,
 * 2 or more than 4 samples, every other compression, Predictor 3, FillOrder 2, a dimension of 65536 or more, a strip of 2^31
 * or more bytes, old-style (bit-reversed) LZW.  CVHIP_ERR_INVALID: anything malformed - a truncated header or IFD, an entry or
 * strip past the file, width or height 0, a missing required tag, a wrong number of strip offsets or byte counts, byte counts
 * missing on a compressed file, an uncompressed strip shorter than its rows, PackBits input that ends before the strip's rows
 * are full, an LZW code above the next entry, an LZW EOI or end of input before the rows are full, drop_rows >= height;
 * nothing is written then. */
#define CVHIP_TIFF_DROP_DATABAR 0xFFFFFFFFu
/* Host only, no device.  out_info[12] = width, height, samples per pixel, bits per sample, compression, photometric,
 * predictor, strips, rows per strip, FocalLengthIn35mmFilm (IFD0 -> 34665 -> 0xA405 as SHORT or LONG; 0 = none),
 * databar_height, flags (bit 0: an SEM block was found, bit 1: tilt_angle is Some).  out_scale[3] = scale width, scale height
 * (1.0 each by default), tilt angle.  A missing or broken block gives the defaults, as get_metadata falls back. */
int cvhip_tiff_info(const uint8_t *file, uint64_t size, uint32_t *out_info, float *out_scale);
/* cvhip_jpeg_decode's arguments and contract for a TIFF file; drop_rows = CVHIP_TIFF_DROP_DATABAR cuts the file's own
 * DatabarHeight, as SourceImage::load does. */
int cvhip_tiff_decode(cvhip_device *dev, const uint8_t *file, uint64_t size, uint32_t format, uint32_t drop_rows, uint8_t *out,
                      uint64_t cap, uint64_t *out_size);
/* Of the calling thread's last cvhip_tiff_decode that reached the device: out_stats[4] = strips, LZW codes read, Clear codes
 * met, the longest string copied. */
int cvhip_tiff_last_stats(uint64_t *out_stats);

/* ------------------------------------------------------------------------------------------
 * TIFF files in, Deflate strips and tiled layout (csrc/tiff_ext_kernels.hip, csrc/tiff_common.hpp with
 * extended = true): the `image` crate behind image::open(path)?.into_luma8() / into_rgb8() (src/reconstruction.rs:40-60) also
 * reads Deflate and tiled TIFF files.  These entry points take a superset of what cvhip_tiff_info / cvhip_tiff_decode take -
 * those answer every file as they always did - and return the same pixels for a file both accept.  The pixels are DEFINED by
 * tests/ref_tiff_ext.py.  Newly accepted: compression 8 and 32946 (every strip or tile a whole zlib stream: header, stored,
 * fixed and dynamic blocks in any mix, the Adler-32 checked against the stream's own output; a workgroup per stream), and
 * tiles (tags 322 to 325) with compression 1, 5, 32773, 8 and 32946, Predictor 1 or 2 (it restarts at every tile's left
 * edge); edge tiles are stored whole, their padding is decoded and dropped.
 * CVHIP_ERR_UNSUPPORTED, beyond cvhip_tiff_decode's list without tiles and these two compressions: a tile width or length
 * that is 0 or no multiple of 16; a tile row, length or tile of 2^31 bytes or more; Deflate whose streams decompress (tiles
 * padded) to 2^31 bytes or more, or whose byte counts add up to more than the file (streams that share bytes).  CVHIP_ERR_INVALID: strip tags (273, 279) beside tile tags; TileOffsets or TileByteCounts that do not hold
 * tiles_across x tiles_down entries; a Deflate stream with a bad zlib header, block type 3, a stored block whose NLEN is not
 * ~LEN, bad code lengths, a code that does not exist, a copy that reaches in front of its own stream's first byte, an end
 * before the final block's end-of-block or inside the Adler-32, a wrong Adler-32, or output that is not exactly the bytes of
 * its strip or tile - fewer or more (libtiff stops when the rows are full and reads such a file; here the checksum is
 * always checked, so the stream has to end where the rows do).  Nothing is written on any refusal. */
/* Host only, as cvhip_tiff_info (src/reconstruction.rs:40-60, 80-144).  out_info[16]: slots 0 .. 11 as cvhip_tiff_info's - of a
 * tiled file slot 7 is the number of tiles and slot 8 TileLength -; 12 tile width, 13 tile length (both 0: strips), 14 tiles
 * across, 15 zero.  out_scale[3] as cvhip_tiff_info's. */
int cvhip_tiff_ext_info(const uint8_t *file, uint64_t size, uint32_t *out_info, float *out_scale);
/* cvhip_tiff_decode's arguments and contract, to the letter (src/reconstruction.rs:40-60): cap = 0 sizes without writing,
 * drop_rows = CVHIP_TIFF_DROP_DATABAR cuts the file's own DatabarHeight, out in host or device memory at any alignment. */
int cvhip_tiff_ext_decode(cvhip_device *dev, const uint8_t *file, uint64_t size, uint32_t format, uint32_t drop_rows, uint8_t *out,
                          uint64_t cap, uint64_t *out_size);
/* Of the calling thread's last cvhip_tiff_ext_decode that reached the device (the streams of src/reconstruction.rs:40-60's
 * image::open): out_stats[12] = streams (strips or tiles), LZW codes read, Clear codes met, the longest string copied, stored,
 * fixed and dynamic deflate blocks summed over the streams, subsequences, the most settle rounds one window needed, settle
 * windows, rounds of the copy resolution, zero. */
int cvhip_tiff_ext_last_stats(uint64_t *out_stats);

/* ------------------------------------------------------------------------------------------
 * PNG files in (csrc/png_decode_kernels.hip, csrc/png_decode_common.hpp): the third format the reference's
 * `image` crate is built with, and the one this library writes (cvhip_png_encode).  The host walks the chunks, checks the CRC
 * of every chunk that is not an IDAT and reads IHDR, PLTE and eXIf; inflate, the IDAT CRCs, the Adler-32, the five filters
 * and the conversion run on the device.  The pixels are DEFINED by tests/ref_png_in.py: the samples are what inflate and the
 * filters give (bpp = max(1, channels * bits / 8), Paeth's tie order a, b, c; pinned to Pillow); 16-bit samples are
 * big-endian and reduce by (v + 128) / 257, 1/2/4-bit grey scales by 255 / (2^bits - 1), a palette index becomes its PLTE
 * entry, alpha and tRNS are dropped (not blended), Luma8 of a colour pixel is (2126 r + 7152 g + 722 b) / 10000 truncated (of
 * 16-bit samples in 16 bits, then reduced), grey as RGB8 is the plane three times, gAMA / sRGB / iCCP are ignored -
 * into_luma8 / into_rgb8 as remembered, not pinned to the crate.  The SEM text tags are not read from a PNG file.
 * Supported: colour types 0, 2, 3, 4, 6 at every legal bit depth, no interlacing, any number of IDAT chunks split anywhere,
 * stored, fixed and dynamic deflate blocks in any mix; bytes behind the Adler-32 are ignored, distances up to 32 768 are
 * accepted whatever CINFO says; ancillary chunks (APNG's among them: the default image is decoded) are skipped.
 * CVHIP_ERR_UNSUPPORTED: Adam7 (cvhip_png_ext_decode below reads it), a dimension of 65 536 or more, a filtered image or IDAT data of 2^31 or more bytes.
 * CVHIP_ERR_INVALID: anything malformed - a bad signature, a first chunk that is not a 13-byte IHDR, a zero dimension, an
 * illegal colour type / bit depth pair, compression or filter method other than 0, interlace above 1, colour type 3 without
 * PLTE, a PLTE of a wrong length or out of place, a palette index beyond it, no IDAT, IDAT chunks that are not consecutive, a
 * chunk past the file, no IEND, an unknown critical chunk, a CRC mismatch, a bad zlib header, block type 3, NLEN that is not
 * ~LEN, over-subscribed code lengths, incomplete ones (unless no code is longer than one bit), HLIT above 286 or HDIST above
 * 30, a repeat with nothing before it or past HLIT + HDIST, no code for 256, a used symbol 286 / 287 or distance 30 / 31, a
 * distance before the first byte, a stream that ends early, output that is not height x (1 + row bytes) bytes, a wrong
 * Adler-32, a filter type above 4, drop_rows >= height; nothing is written then. */
/* Host only, no device (the IDAT CRCs and the stream are the device's).  out_info[8] = width, height, colour type, bit depth,
 * interlace method, IDAT chunks, FocalLengthIn35mmFilm (the eXIf chunk: IFD0 -> 0x8769 -> 0xA405 as SHORT or LONG, either
 * byte order; 0 = none, and a broken block is none), flags (bit 0: a PLTE was read, bit 1: a tRNS was read). */
int cvhip_png_info(const uint8_t *file, uint64_t size, uint32_t *out_info);
/* cvhip_jpeg_decode's arguments and contract for a PNG file. */
int cvhip_png_decode(cvhip_device *dev, const uint8_t *file, uint64_t size, uint32_t format, uint32_t drop_rows, uint8_t *out,
                     uint64_t cap, uint64_t *out_size);
/* Of the calling thread's last cvhip_png_decode that reached the device: out_stats[8] = stored, fixed and dynamic blocks,
 * subsequences (of the fixed and dynamic blocks), the most settle rounds one window needed, settle windows (of 256
 * subsequences; a stored block's 256 records count as one), rounds of the copy resolution (the one that changed nothing
 * included), row segments of the unfilter pass. */
int cvhip_png_last_stats(uint64_t *out_stats);

/* ------------------------------------------------------------------------------------------
 * PNG files in, Adam7 interlaced files too (csrc/png_decode_kernels.hip, csrc/png_decode_common.hpp with
 * adam7 = true): the `image` crate behind image::open(path)?.into_luma8() / into_rgb8() (src/reconstruction.rs:40-60) also
 * reads interlaced PNG files.  These entry points take a superset of what cvhip_png_info / cvhip_png_decode take - those
 * answer every file as they always did, an Adam7 file with CVHIP_ERR_UNSUPPORTED - and return the same bytes for a file both
 * accept.  The pixels are DEFINED by tests/ref_png_adam7.py: the stream holds seven reduced images one behind the other,
 * pass p = 0 .. 6 with x0 = 0,4,0,2,0,1,0, y0 = 0,0,4,0,2,0,1, dx = 8,8,4,4,2,2,1, dy = 8,8,8,4,4,2,2, of
 * ceil((W - x0) / dx) x ceil((H - y0) / dy) samples (a pass with no column or no row has no bytes at all); each is
 * filtered on its own with zeros above its first row and the image's bpp; sample (px, py) of pass p is pixel
 * (x0 + px dx, y0 + py dy); the padding bits at the end of a sub-byte row are nothing.  Conversion, eXIf and drop_rows are
 * cvhip_png_decode's.  CVHIP_ERR_UNSUPPORTED: a dimension of 65 536 or more, passes (rows with their filter bytes) or IDAT
 * data of 2^31 bytes or more.  CVHIP_ERR_INVALID: cvhip_png_decode's list, with "output that is not the passes' bytes" for
 * an interlaced file.  Nothing is written on any refusal. */
/* Host only, as cvhip_png_info (src/reconstruction.rs:40-60): out_info[8] has its slots; slot 4, the interlace method, is 0 or 1. */
int cvhip_png_ext_info(const uint8_t *file, uint64_t size, uint32_t *out_info);
/* cvhip_png_decode's arguments and contract, to the letter (src/reconstruction.rs:40-60): cap = 0 sizes without writing, out
 * in host or device memory at any alignment. */
int cvhip_png_ext_decode(cvhip_device *dev, const uint8_t *file, uint64_t size, uint32_t format, uint32_t drop_rows, uint8_t *out,
                         uint64_t cap, uint64_t *out_size);
/* Of the calling thread's last cvhip_png_ext_decode that reached the device (the files of src/reconstruction.rs:40-60's
 * image::open): out_stats[10] = slots 0 .. 7 as cvhip_png_last_stats' - the row segments counted over all passes, each of
 * which starts one -, 8 the non-empty passes (1 for a file that is not interlaced), 9 zero. */
int cvhip_png_ext_last_stats(uint64_t *out_stats);

/* Row sharding (multi-GPU): restrict the SEARCH passes of this context to shard `num` of `den`
 * equal row chunks of the searched level image: rows [num*rps, min((num+1)*rps, h_level)) with
 * rps = ceil(h_level / den).  Rows outside the band keep whatever the level grid holds until
 * the bands are all-gathered; the cross-checks then run on the whole grid on every rank, so
 * every rank ends with the complete, identical result (no reduction across ranks: N-GPU output
 * is bit-identical to 1-GPU output).  cvhip_correlate_level calls `gather` itself (levels with
 * fewer than 64 rows per shard are simply computed whole on every rank); with the per-pass
 * calls the host gathers between passes (cvhip_ctx_level_grid).  num = 0, den = 1 (default) =
 * all rows; den <= 64; gather may be NULL when only the per-pass calls are used. */
int cvhip_ctx_set_row_shard(cvhip_ctx *ctx, uint32_t num, uint32_t den, cvhip_allgather_fn gather, void *user);
/* Row sharding without collectives ("independent band" mode).  For row-local geometry — an affine F
 * whose epipolar lines stay within a few rows of the pixel's own row at every pyramid level — shard
 * `num` of `den` computes, at every level, only the rows its band of the FINAL forward grid depends
 * on: the band plus a halo (about 2*D + 20 rows per level, D = the corridor's row excursion) that is
 * recomputed redundantly instead of exchanged.  Uses the fact that the two cross-checks of a level
 * commute (any reverse match that supports a forward match is itself supported by it, mod.rs:588-624),
 * so no filtered grid has to be communicated between passes.  After the last level only rows
 * [num*rps, (num+1)*rps) of the forward level grid (cvhip_ctx_level_grid, dir 0) are meaningful; the
 * host gathers those bands once (the single RCCL gather of the north star) before cvhip_complete.
 * Returns CVHIP_ERR_UNSUPPORTED when the geometry is not row-local (perspective F, steep or
 * column-major lines): fall back to cvhip_ctx_set_row_shard + all-gather hook.  The context must be
 * driven with cvhip_correlate_level over the reference's schedule (scale = 2^-k, k = steps..0). */
int cvhip_ctx_set_row_band(cvhip_ctx *ctx, uint32_t num, uint32_t den);
/* ------------------------------------------------------------------------------------------
 * The collectives of row sharding on RCCL, inside the library (no torch, no host hook): one process per GPU, one
 * communicator per device handle, every collective enqueued on the handle's own stream - ordered with the kernels
 * around it by construction.  librccl.so.1 is opened on first use (CVHIP_ERR_UNSUPPORTED if it cannot be).
 * ---------------------------------------------------------------------------------------- */
typedef struct cvhip_rccl cvhip_rccl;
#define CVHIP_RCCL_ID_BYTES 128
/* ncclGetUniqueId: rank 0 calls this and hands the 128 bytes to every rank (launcher's store, MPI, a file). */
int cvhip_rccl_unique_id(uint8_t *id);
/* ncclCommInitRank on the handle's GPU; collective over all `world` ranks (<= 64). */
int cvhip_rccl_create(cvhip_device *dev, const uint8_t *id, uint32_t rank, uint32_t world, cvhip_rccl **out);
void cvhip_rccl_destroy(cvhip_rccl *comm);
/* In-place all-gather of `world` chunks of shard_bytes at `buf` (device memory; this rank's chunk already in place). */
int cvhip_rccl_allgather(cvhip_rccl *comm, void *buf, uint64_t shard_bytes);
/* In-place gather to `root` only: every other rank sends its chunk straight into the root's buffer (grouped
 * ncclSend/ncclRecv - on an 8-GPU xGMI node seven concurrent point-to-point transfers, not a ring). */
int cvhip_rccl_gather(cvhip_rccl *comm, void *buf, uint64_t shard_bytes, uint32_t root);
/* cvhip_ctx_set_row_shard(ctx, rank, world, <all-gather above>): bands + one all-gather per sharded search pass. */
int cvhip_ctx_set_row_shard_rccl(cvhip_ctx *ctx, cvhip_rccl *comm);
/* The single gather of independent-band mode (cvhip_ctx_set_row_band(ctx, rank, world)): after the last level, the
 * forward level grid's bands go to `root` (root < 0: to every rank) before cvhip_complete. */
int cvhip_ctx_gather_bands_rccl(cvhip_ctx *ctx, cvhip_rccl *comm, int root);

/* Device pointers + geometry of direction `dir`'s current level grid, for the host's collectives.  Two planes of one
 * 4-byte word per level pixel, row-major lw x lh: `cells` = the match plane, u32 x | y << 16 in LEVEL coordinates
 * (0xFFFFFFFF = None) - everything the search range and the cross-checks of other ranks read, i.e. all that has to
 * travel between passes; `scores` (may be NULL) = the f32 score plane, which only cvhip_complete reads (the single
 * final gather moves both).  Each plane always has room for den * rows_per_shard rows, so bands can be gathered in
 * equal chunks. */
int cvhip_ctx_level_grid(cvhip_ctx *ctx, int dir, void **cells, void **scores, uint32_t *lw, uint32_t *lh, uint32_t *row0,
                         uint32_t *row1, uint32_t *rows_per_shard);

/* Use device-resident level images where they are instead of copying them into the context's own padded
 * buffers first.  By enabling this the caller guarantees, for every DEVICE pointer it passes as a level image:
 * at least 64 readable bytes after the last pixel (the kernels read whole dwords at row ends), and that the
 * image stays unchanged until the work of the call has completed on the device's stream.  Under
 * cvhip_ctx_set_fuse_level_calls the work of a level's correlate calls is enqueued by LATER calls - both directions in
 * one launch at the reverse call, and with result bands (cvhip_ctx_set_result_bands != 1) the whole last level at its
 * second cvhip_cross_check_filter call - so borrowed images of a level must then stay unchanged until that level's
 * second cvhip_cross_check_filter call (or cvhip_complete) has completed on the stream.  Host images are still
 * copied.  Off by default. */
int cvhip_ctx_set_borrow_inputs(cvhip_ctx *ctx, int borrow);
/* The reference issues FOUR backend calls per pyramid level (PointCorrelations::correlate_images, correlation/mod.rs:
 * 217-245): correlate_images forward, correlate_images reverse with the SAME two images exchanged, cross_check_filter
 * forward, cross_check_filter reverse.  By enabling this the caller promises that order - the binding of
 * GpuContext::new does - and the library executes the four calls as cvhip_correlate_level would: the
 * forward call takes the images in (both images' window statistics, once per level), the reverse call - recognised by
 * the exchanged image pointers, dimensions, scale and first_pass - launches both search passes together, the second
 * cross-check call launches both filters.  Results are those of the independent calls, bit for bit; a call sequence
 * that departs from the order is executed call by call as without the promise (whatever was taken in runs first), and
 * every other entry point of the context first runs what is pending.  What the promise adds to the contract: between a
 * level's forward and reverse call the two images must not change (the reverse call does not read them again), and an
 * error of the forward pass is reported by the call that executes it.  Off by default. */
int cvhip_ctx_set_fuse_level_calls(cvhip_ctx *ctx, int enable);
/* Window statistics of a level (compute_image_point_data, mod.rs:632-694) on a stream of the library's own, ahead of
 * the level's turn: they depend on the level's images only, and the coarse levels' search is a chain of small
 * dependent launches that leaves the chip idle for ~0.4 ms of a 4096^2 pair - room for the 0.5 ms of full-chip work
 * the statistics of the two finest levels are.  Applies to cvhip_correlate_level calls with BORROWED device images
 * (cvhip_ctx_set_borrow_inputs) outside row-shard mode and outside per-kernel timing; the caller additionally
 * promises that a level image is complete in memory when it is passed (not merely ordered on the handle's stream:
 * the statistics kernel reads it on another stream, ordered behind the work enqueued before the pyramid run's FIRST
 * level only).  Same results bit for bit.  Off by default. */
int cvhip_ctx_set_stats_ahead(cvhip_ctx *ctx, int ahead);

/* Measurement hooks (bench.py).  time_kernels: 1 = every kernel launch is bracketed by HIP events on the
 * stream it is launched on, 2 = only the launches of the search class ([2] below), 0 = off.  Timing is
 * not free: with any timing event in flight the runtime profiles every dispatch of the step (~4 us per
 * kernel, 0.45 ms per 4096^2 step on this stack), however few events are recorded.  count_candidates:
 * evaluated candidates are counted on the device. */
int cvhip_ctx_set_profiling(cvhip_ctx *ctx, int time_kernels, int count_candidates);
/* Accumulated since the last reset: search-kernel launches, their summed duration (ms) and the
 * number of candidates that executed the 121-term sum (mod.rs:442-454).  Synchronises. */
int cvhip_ctx_get_profile(cvhip_ctx *ctx, uint32_t *launches, double *search_ms, uint64_t *candidates,
                          int reset);

/* Per-kernel-class device time since the last reset (needs time_kernels = 1), measured with HIP
 * events on the context's stream: [0] window statistics, [1] search-range estimation, [2] search
 * (version 3: the box filter; 1: the whole search), [3] fallback kernels (whole-corridor
 * exact re-evaluation; for version 3 also the candidate filter on the workgroups the box filter
 * declined), [4] cross-check, [5] grid expansion in complete(), [6] the candidate filter launched as a level's search
 * (the first pass, steep geometry, search version 2).  Synchronises. */
int cvhip_ctx_get_kernel_times(cvhip_ctx *ctx, double ms[7], uint32_t launches[7], int reset);
/* Device counters of the search kernel since the last reset (needs count_candidates = 1):
 * out[0] candidates that passed the reference's bounds/stdev tests (== candidates above),
 * out[1] exact 121-term f32 evaluations, out[2] pixels whose filter band held 2..4 contenders,
 * out[3] pixels that re-evaluated their whole corridor exactly (tile too large for LDS, or more
 * than 4 contenders).  reset clears these four only (cvhip_ctx_get_profile's reset clears every counter).
 * Synchronises. */
int cvhip_ctx_get_counters(cvhip_ctx *ctx, uint64_t out[4], int reset);
/* Diagnostics of the stepped box walk since the last reset (needs count_candidates = 1; kept apart from the
 * counters above, which they do not change): out[0] stepped waves of row-major tiles whose own displacement range
 * is 65 steps (one more than the walk's 64-lane step table), out[1] the same for transposed tiles, out[2] the
 * most steps any stepped wave walked, out[3] 0.  reset clears these four only.  Synchronises. */
int cvhip_ctx_get_box_counters(cvhip_ctx *ctx, uint64_t out[4], int reset);
/* The lean box walk (rectified pairs) folds the two ends of a wave's union of displacement ranges: where the ranges drift
 * along a wave's 53 pixels, the first steps of the union are searched only at one end of the wave and the last steps only
 * at the other, and one low and one high step then run as a single step, every lane at its own displacement (DESIGN.md
 * section 4.2).  Every candidate is still evaluated once, by the same instructions; results are identical either way.
 * on = 1 (default) / 0: every wave walks its whole union.  Takes effect with the next pass. */
int cvhip_ctx_set_box_fold(cvhip_ctx *ctx, int on);
/* Diagnostics of the fold since the last reset (needs count_candidates = 1; kept apart from the counters above), summed
 * over the lean box waves that walked: out[0] steps of their unions, out[1] steps walked after folding, out[2] pairs
 * folded with the low steps at the low lanes (ascending), out[3] pairs folded the other way (descending);
 * out[0] - out[1] == out[2] + out[3].  reset clears these four only.  Synchronises. */
int cvhip_ctx_get_box_fold_counters(cvhip_ctx *ctx, uint64_t out[4], int reset);
/* The lean box walk with lanes along x (exactly horizontal epipolar lines) takes its lines from a table with one entry per
 * image row, written by the search range kernel in front of it, where the line cannot differ along a row: an affine F whose
 * F[6] is +0.0 or -0.0.  Every other pass evaluates the line in every lane, as before; results are
 * identical either way.  on = 1 (default) / 0: never use the table.  Takes effect with the next pass. */
int cvhip_ctx_set_row_lines(cvhip_ctx *ctx, int on);
/* out[0] / out[1]: 1 if the last box launch of the forward / reverse direction took its lines from the row table. */
int cvhip_ctx_get_row_lines_used(cvhip_ctx *ctx, int out[2]);
/* Select the search kernel: 1 = every candidate through the exact serial f32 chain, 2 = exact-integer
 * filter per candidate + exact re-evaluation of the contenders, 3 (default) = the same filter evaluated
 * as displacement-plane box sums for whole row segments where the epipolar lines keep one major axis, with 2 for
 * every other geometry and as the per-workgroup fallback; 4 = 3 with the box kernel launched for every geometry
 * (testing); 5 = 3 with the rectified affine launches (exactly axis-parallel row-major lines, five stripes) as int8
 * matrix products on the matrix pipe (search4_mfma_kernel: the formulation the north star names; bit-exact, and
 * measured SLOWER than the box sums on MI355X - DESIGN.md section 4.7 - so it is not the default); 6 = 3 with the
 * rectified affine launches on TWO image columns per lane (search3_box2_kernel: one prefix sum and two permutes for two
 * pixels; bit-exact, 0.7-0.77 of the one-column group per pixel in isolation and SLOWER as a kernel - its 116-pixel waves walk
 * longer unions of displacement ranges - DESIGN.md section 4.2).  All give identical results. */
int cvhip_ctx_set_search_version(cvhip_ctx *ctx, int version);
/* Which passes write the reference's SCORES.  Match positions are the reference's in every pass, always.  Scores are
 * only observable for the forward grid of the last (full-resolution) level: the reference overwrites every cell a
 * coarser level wrote, None included (mod.rs:311-316), and complete() drops the reverse grid (mod.rs:208-215); nothing
 * else ever reads a score (estimate_search_range and cross_check_point look at positions only, mod.rs:468-540,
 * 588-624).  By default (all_passes = 0) the forward pass at scale 1 evaluates every recorded contender with the
 * reference's serial f32 chain, as before, and every other pass does so only where it decides something (several
 * contenders inside the filter's band, or one within the band of the threshold); a cell settled without it holds the
 * filter's estimate internally, its score plane is not written, and cvhip_complete_dir reports NaN scores for such a
 * grid.  all_passes = 1: the reference's bits in every cell of every pass - for tests that read coarser levels or the
 * reverse grid through cvhip_complete_dir. */
int cvhip_ctx_set_exact_scores(cvhip_ctx *ctx, int all_passes);
/* Test hook of the search-range kernel (estimate_search_range, mod.rs:468-540): 0 (default) = integer box sums with the
 * reference's f64 chain only where the rounding of `len` is open, 1 = the chain for every pixel, 2 / 3 = every third
 * block of a box-sum tile through the staged / the global-memory chain.  All give identical results. */
int cvhip_ctx_set_range_mode(cvhip_ctx *ctx, int mode);

/* ------------------------------------------------------------------------------------------
 * Pyramid level on the device.  The reference builds every level with
 * the `image` crate's Lanczos3 resize on the host (reconstruction.rs:146-162), upstream of the
 * boundary; its source is not available here, so this is the documented substitute used by the
 * benchmark: one 2x2 box-filter step with rounding, dst dims floor(w/2) x floor(h/2),
 * dst[y][x] = (s[2y][2x] + s[2y][2x+1] + s[2y+1][2x] + s[2y+1][2x+1] + 2) >> 2.  Keeps pyramids
 * resident in HBM for both the ORB and the dense stage.  Host or device pointers.
 * ---------------------------------------------------------------------------------------- */
int cvhip_downsample_box(cvhip_device *dev, const uint8_t *src, uint32_t w, uint32_t h, uint8_t *dst);

/* SourceImage::resize (reconstruction.rs:146-162) on the device: image::imageops::resize(.., FilterType::Lanczos3) of a
 * Luma8 image to nw x nh (the caller passes (w as f32 * scale) as u32, (h as f32 * scale) as u32, :149-150).  The
 * `image` crate (0.25.10) is not vendored with the reference; this is its published separable algorithm (vertical pass
 * to f32, horizontal pass, f32 weights normalised per output sample, clamp + round to nearest at the end; equal
 * dimensions are a copy).  Weights come from glibc's sinf on the host (what Rust's f32::sin resolves to on linux-gnu);
 * every other step is a single IEEE f32 operation in the crate's order, so the bytes equal the oracle's restatement
 * (oracle/cvref_resize.py, same sinf) exactly - tested with MAX_DIFF = 0.  Nothing pins either to the crate itself
 * ("parity unpinned").  Host or device pointers: with a host source or destination the call is complete on return; with
 * both on the device the two kernels are enqueued on the handle's stream and the call returns (stream order, like
 * cvhip_complete into device memory).  The resampling tables of every (source size, output size) met are kept in device
 * memory with the handle - a pipeline resizes equally sized images to the same scales pair after pair. */
int cvhip_resize_lanczos3(cvhip_device *dev, const uint8_t *src, uint32_t w, uint32_t h, uint8_t *dst, uint32_t nw,
                          uint32_t nh);

/* ------------------------------------------------------------------------------------------
 * ORB — replaces orb::extract_points (orb.rs:50-84).
 * out_xy: 2*cap u32 (x, y), out_desc: 8*cap u32, *out_n = keypoints written (<= cap).
 * Order = the reference's (Harris-descending stable, then BRIEF filter).  cap >= 10000 to
 * receive everything the reference returns (MAX_KEYPOINTS, orb.rs:41).
 * progress (may be NULL) replaces `Option<&PL>` (orb.rs:43-53): the reference reports from inside its parallel
 * loops, FAST rows 0 .. 0.20 (orb.rs:93-100), scores .. 0.25 (:112-118), non-maximum suppression .. 0.35 (:138-146),
 * Harris .. 0.70 (:60-66), BRIEF .. 1.0 (:358-363); here the same positions are reported on the calling thread as
 * the stages complete (0.25 and 1.0 after the stage's results have reached the host, the others at submission).
 * ---------------------------------------------------------------------------------------- */
int cvhip_orb_extract(cvhip_device *dev, const uint8_t *img, uint32_t w, uint32_t h, uint32_t cap,
                      uint32_t *out_xy, uint32_t *out_desc, uint32_t *out_n, cvhip_progress_fn progress, void *user);
/* The same for n_images independent images in one call - the pyramid levels of an image, as match_keypoints' per-image
 * loop extracts them (reconstruction.rs:418-458), or the images of a set.  An extraction has three host round trips
 * (corner counts; results - and, for an image with a keypoint inside the orientation guard band, patch moments out /
 * libm orientations in); the batch enqueues every image's work of a stage before it waits, so it pays them once.  Results per image are exactly cvhip_orb_extract's.  imgs / ws / hs / out_xy / out_desc: n_images entries
 * (each out_xy[i]: 2*cap u32, out_desc[i]: 8*cap u32); out_n: n_images counts. */
/* Test hook of the orientation step.  The reference computes atan2 / sin / cos with libm (orb.rs:337-341, 365-366); the
 * extraction uses the device's f64 functions wherever that provably gives the same rounded sample offsets - every
 * round(o_y cos - o_x sin) farther than `guard` from a half-integer - and redoes an image with the host's libm
 * otherwise.  Default 1e-9 (the functions agree to a few ulp: offsets move by < 1e-12).  A larger guard sends more
 * images down the host path, 0 switches the device orientation off (every image takes the host path).  Results are
 * identical for every setting. */
int cvhip_orb_set_orientation_guard(cvhip_device *dev, double guard);
int cvhip_orb_extract_batch(cvhip_device *dev, uint32_t n_images, const uint8_t *const *imgs, const uint32_t *ws,
                            const uint32_t *hs, uint32_t cap, uint32_t *const *out_xy, uint32_t *const *out_desc,
                            uint32_t *out_n, cvhip_progress_fn progress, void *user);

/* ------------------------------------------------------------------------------------------
 * Keypoint matcher — replaces KeypointMatching::match_points (pointmatching.rs:43-77).
 * xy: 2 u32 per keypoint, desc: 8 u32 per keypoint.  out_matches: 4*n1 u32 (x1,y1,x2,y2),
 * sorted by Hamming distance (stable); out_dist (n1, may be NULL).
 * ---------------------------------------------------------------------------------------- */
int cvhip_match_points(cvhip_device *dev, const uint32_t *xy1, const uint32_t *desc1, uint32_t n1,
                       const uint32_t *xy2, const uint32_t *desc2, uint32_t n2, uint32_t threshold,
                       uint32_t *out_matches, uint32_t *out_dist, uint32_t *out_n);

/* ------------------------------------------------------------------------------------------
 * RANSAC hypothesis scoring — replaces the all-matches fold of FundamentalMatrix::validate_f
 * (fundamentalmatrix.rs:210-216) with fits_model/reprojection_error (:452-471), for H
 * hypotheses at once.  F: 9*H doubles row-major, matches: 4*N u32 (x1,y1,x2,y2).
 * out_count[h] = inliers, out_err_sum[h] = sum of their errors in match order.
 * ---------------------------------------------------------------------------------------- */
int cvhip_ransac_score(cvhip_device *dev, const double *F, uint32_t H, const uint32_t *matches, uint32_t N,
                       double t, uint32_t *out_count, double *out_err_sum);

/* ------------------------------------------------------------------------------------------
 * Whole affine RANSAC on the device — replaces
 * FundamentalMatrix::new(Affine, _).find_ransac(matches) (fundamentalmatrix.rs:72-147, 155-286,
 * 231-239): sampling, the 4-point model fit and the sample checks run next to the scoring kernel;
 * the host only reads one early-exit word per 50 000-iteration round.  matches: 4*N u32
 * (x1,y1,x2,y2) sorted by descriptor distance as KeypointMatching returns them (the first 5000 are
 * sampled).  out_F: 9 doubles row-major; out_inlier_mask: N bytes (may be NULL).  The reference's RNG
 * is OS-seeded (not reproducible), so equality with it is statistical; `seed` makes this one
 * reproducible.  Returns CVHIP_ERR_NO_MODEL with the reference's RansacError messages.
 * ---------------------------------------------------------------------------------------- */
int cvhip_ransac_affine(cvhip_device *dev, const uint32_t *matches, uint32_t N, uint64_t seed, double *out_F,
                        uint32_t *out_inlier_count, uint8_t *out_inlier_mask);

/* The basis of the 7-point pencil in calculate_model_perspective (fundamentalmatrix.rs:309-322).
 * CVHIP_PENCIL_THIN_SVD (default) is the reference as written: `a.svd(false, true)` on the 7 x 9 system is nalgebra's
 * thin decomposition (v_t: 7 x 9, singular values descending), so `v_t.row(nrows - 2)` / `.row(nrows - 1)` are rows 5 and
 * 6 - the right singular vectors of the two SMALLEST of the seven singular values, not the null space.  Its hypotheses
 * do not fit their own sample until validate_f's optimize_perspective_f (:201-205) has run on EVERY root, which the
 * device does.  Sign convention of a singular vector (nalgebra's is not observable from its published interface): the
 * entry of largest magnitude is positive.  CVHIP_PENCIL_NULL_SPACE is the 7-point algorithm as published (the true
 * null space of A: rounds 2-3 of this build), kept as an option: better hypotheses, and ~3x cheaper - not the reference's. */
#define CVHIP_PENCIL_THIN_SVD 0
#define CVHIP_PENCIL_NULL_SPACE 1
int cvhip_ransac_set_pencil(cvhip_device *dev, int pencil);
/* Test hook: with the thin-SVD pencil validate_f's least_squares runs as two passes over the roots - up to the first
 * accepted step for all of them, then the accepting ones from their start - on persistent waves whose lanes take the next
 * root off the queue as they finish (enable = 2, default), as the same two passes with a root per thread (1), or as the
 * scalar loop itself in one kernel (0).  Same values, bit for bit. */
int cvhip_ransac_set_lm_pipeline(cvhip_device *dev, int enable);
/* The counting kernel's f32 screen over the head of the match list as [hypotheses x 12] x [12 x matches] products
 * (v_mfma_f32_16x16x4_f32; whoever is still alive behind the head continues in the vector kernel): enable = 1.  Default 0, the
 * vector kernel alone: in this form the matrix and the vector phase of every wave follow each other in lockstep
 * (SQ_VALU_MFMA_COEXEC_CYCLES = 0; within one wave the two pipes serialise), so it saves nothing - measured 47 against 45 ms for
 * config 5's RANSAC stage.  The counts are the f64 counts either way. */
int cvhip_ransac_set_count_mfma(cvhip_device *dev, int enable);
/* Test hook of the round scheduler: batches of rounds are normally scored as their generators finish (the host polls
 * their events, for at most 50 ms per decision); enable = 1 takes the branch that polling falls back to - the oldest
 * pending batch is enqueued behind its event, in order, no polling.  Same result (Ord's maximum does not depend on the
 * order; equal hypotheses are settled by their position in iteration order). */
int cvhip_ransac_set_in_order(cvhip_device *dev, int enable);

/* Perspective RANSAC on the device — FundamentalMatrix::new(Perspective, max_dimension).find_ransac
 * (fundamentalmatrix.rs:72-147, 155-229, 289-389): per sample the 7-point model (the pencil's basis as
 * cvhip_ransac_set_pencil says - default: rows 5 and 6 of the thin SVD, as the reference writes it -, the
 * determinant cubic, the reference's rank and sign-consistency checks, up to three roots),
 * every surviving root scored against ALL matches, best = most inliers then smallest mean error, early
 * exit above 50 000 inliers; t = 0.01 * max_dimension.  `rounds` = number of 50 000-sample rounds (0 or
 * more than 20 = the reference's 20).  validate_f's per-hypothesis optimize_perspective_f (:201-205: the LM
 * over the sample and the rank test on the re-parametrised matrix) runs on the device with the rest.  Not done
 * here: the final LM refit of optimize_result (:246-256): cvhip_optimize_perspective_f below, called by the
 * host layers.  out_F: the best hypothesis
 * (normalised by F[2][2]); mask/count: its inliers.  Statistical parity, as above. */
int cvhip_ransac_perspective(cvhip_device *dev, const uint32_t *matches, uint32_t N, double max_dimension,
                             uint64_t seed, uint32_t rounds, double *out_F, uint32_t *out_inlier_count,
                             uint8_t *out_inlier_mask);
/* Test hook of the generator above: the hypotheses of B caller-chosen samples (sample_idx: 7 match indices
 * each, host memory) exactly as they go on to the all-matches fold - i.e. after calculate_model_perspective
 * (:289-389) AND validate_f's finiteness test, optimize_perspective_f over the sample (LM + rank test on the
 * re-parametrised matrix, :201-205, :391-426) and sample-fit test (:206-209) -> out_F: B x 3 x 9 doubles, NaN
 * where a root does not exist or is rejected; t as in fits_model.  Compared with the oracle's numpy restatement
 * (oracle/cvref_fm.py) on identical samples. */
int cvhip_ransac_perspective_models(cvhip_device *dev, const uint32_t *matches, uint32_t N, const uint32_t *sample_idx,
                                    uint32_t B, double t, double *out_F);
/* Same for the affine generator (calculate_model_affine :260-286 + validate_f's checks): sample_idx holds 4
 * match indices per sample -> out_F: B x 9 doubles, NaN where the sample is rejected. */
int cvhip_ransac_affine_models(cvhip_device *dev, const uint32_t *matches, uint32_t N, const uint32_t *sample_idx,
                               uint32_t B, double t, double *out_F);
/* fits_model (fundamentalmatrix.rs:452-458) of one F for every match - the inlier filter of optimize_result
 * (:233-236, 248-254).  out_mask: N bytes, 1 = inlier.  Host or device pointers. */
int cvhip_fits_model(cvhip_device *dev, const double *F, const uint32_t *matches, uint32_t N, double t, uint8_t *out_mask);
/* Test hook: the scoring of ONE RANSAC round for caller-given hypotheses, as the device loops run it - inlier counts
 * from the counting kernel (one wave per hypothesis; pairs decided in packed f32 against rigorous error bounds, the
 * reference's f64 expression inside the guard band, so the counts are exact) and the reference's ordered error sum
 * for the hypotheses tied at the largest count (0 for all others: Ord, :623-649, never looks at theirs).  No pruning.
 * out_count must equal cvhip_ransac_score's counts; out_err_sum its sums where non-zero. */
int cvhip_ransac_round_score(cvhip_device *dev, const double *F, uint32_t H, const uint32_t *matches, uint32_t N, double t,
                             uint32_t *out_count, double *out_err_sum);
/* Test hook: the device loops' rounds on caller-given hypotheses: F is cut into `rounds` consecutive slices and every
 * slice is scored as cvhip_ransac_perspective / cvhip_find_ransac score a generated round - the counting kernel on its
 * own re-sorted copy of the match list, abandoning hypotheses against the best of the earlier slices and the running
 * maximum of the launch; the round's candidates; tie-break sums only where counts tie; the pick.  Out: the best
 * hypothesis after the last slice (its nine doubles, inlier count, mean error - NaN where no tie ever asked for it -
 * and its index in F, -1 if none reached min_count; the index needs F on the host).  Must be Ord's maximum
 * (fundamentalmatrix.rs:623-649) over cvhip_ransac_score's (count, err_sum / count), first of equals by index. */
int cvhip_ransac_rounds_pick(cvhip_device *dev, const double *F, uint32_t H, uint32_t rounds, const uint32_t *matches, uint32_t N,
                             double t, uint32_t min_count, double *out_F, uint32_t *out_count, double *out_mean_error,
                             int64_t *out_index);
/* FundamentalMatrix::new(projection, max_dimension).find_ransac(matches) in one call (fundamentalmatrix.rs:72-147
 * and optimize_result :231-257): cvhip_ransac_affine for projection 0 (max_dimension unused); for projection 1
 * cvhip_ransac_perspective, then the LM refit of the winner on its inliers (cvhip_optimize_perspective_f_device: the
 * reference's loop, values equal to the host function's) and the inliers of the refitted matrix.  This is what reconstruction.rs:502-526
 * calls.  out_F: 9 doubles row-major; out_inlier_mask: N bytes (may be NULL).
 * progress / report_matches (either may be NULL) replace `Option<&PL>` (fundamentalmatrix.rs:41-47, 103): the reference
 * reports iteration / ransac_k per iteration (:119-123) and the running maximum of the inlier counts (:126-131); here
 * both are reported once per 50 000-iteration round on the calling thread - pos = finished rounds / 20 - and, because
 * report_matches needs the round's best count on the host, a listener costs one 4-byte read per round that a call
 * without one only pays where the early exit (:135-141) can fire. */
int cvhip_find_ransac(cvhip_device *dev, int projection, const uint32_t *matches, uint32_t N, double max_dimension,
                      uint64_t seed, double *out_F, uint32_t *out_inlier_count, uint8_t *out_inlier_mask,
                      cvhip_progress_fn progress, cvhip_matches_fn report_matches, void *user);
/* optimize_perspective_f (fundamentalmatrix.rs:391-426) as optimize_result applies it to the winning model
 * (:246): the reference's own Levenberg-Marquardt loop (least_squares, :515-621) with its analytic Jacobian
 * (f_jacobian, :473-512) over the 7 free parameters of F (:429-449), then the rank test (:418-423).  Host
 * arithmetic, as in the reference (no device needed): matches = the n inliers, 4 x uint32 each.  out_F = the
 * refitted matrix and *out_refined = 1, or F itself and 0 where the reference's function returns None
 * (`.unwrap_or(res.f)`).  The loop is restated as written, including where it departs from the textbook
 * method (see the implementation's header); it is deterministic, so the oracle's restatement is compared
 * value for value. */
int cvhip_optimize_perspective_f(const double *F, const uint32_t *matches, uint32_t n, double *out_F, int *out_refined);
/* The same function on the device - what cvhip_find_ransac uses: one workgroup runs the loop's statements with the
 * per-observation work spread over its threads and every long dot product evaluated by eight threads, one per
 * partial sum of the reference's `dot`, so additions happen in the serial function's order and the result equals
 * cvhip_optimize_perspective_f's bit for bit (tested).  ~19 000 inliers: 12 ms on the host, well under 1 ms here.
 * F, matches: host or device pointers; out_F (9 doubles), out_refined: host. */
int cvhip_optimize_perspective_f_device(cvhip_device *dev, const double *F, const uint32_t *matches, uint32_t n,
                                        double *out_F, int *out_refined);

#ifdef __cplusplus
}
#endif
#endif
