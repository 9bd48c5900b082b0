/*
 * ndt_mi355x.h -- C ABI of the MI355X-native NDT scan-matching core (libndt_mi355x.so).
 *
 * Drop-in boundary.  The reference has no FFI: its hot path sits behind the
 * concrete C++ class PoseEstimator (include/ndt_slam/PoseEstimator.h:36-133), injected by
 * pointer (src/SlamLauncher.cpp:12 -> include/ndt_slam/FrontEnd.h:74-76 ->
 * include/ndt_slam/ScanMatcher.h:58-60) and called only from ScanMatcher::matchScan
 * (src/ScanMatcher.cpp:40,45).  A replacement PoseEstimator.{h,cpp} binds exactly the entry
 * points below; INTEGRATION.md shows that binding.  Each entry point names the reference
 * interface (file:line) it replaces.  Plain pointers and sizes only; never throws; every
 * function returns 0 on success or a negative ndt_status, with text in ndt_last_error().
 *
 * Threading: a context is bound to one device and one host thread; all GPU work runs on the
 * context's stream (or the stream passed to the *_dev calls).  Host-pointer calls are
 * synchronous on return; *_dev calls are asynchronous on their stream.  A context owns one set of
 * scratch buffers: *_dev calls of ONE context on different streams are serialised by the library (the
 * later call's stream waits for the earlier call's kernels); to have two batches in flight at the
 * same time use two contexts (a map may be read by any context of its device, from its own host thread: the
 * map's bookkeeping of who reads it is locked; a map is REBUILT from one thread at a time, that of its context).
 */
#ifndef NDT_MI355X_H_
#define NDT_MI355X_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum ndt_status {
  NDT_OK = 0,
  NDT_E_ARG = -1,        /* null / empty / inconsistent arguments                     */
  NDT_E_HIP = -2,        /* a HIP runtime call failed (text in ndt_last_error)        */
  NDT_E_NO_DEVICE = -3,  /* no gfx950 device: the library never falls back to the CPU */
  NDT_E_GRID = -4,       /* map extent / resolution needs more than 2^28 voxels       */
  NDT_E_NOMEM = -5
};

/* Parameters of the path.  The first four are the ROS parameters the reference's constructor
 * reads and hands to PCL (include/ndt_slam/PoseEstimator.h:63-84; values in
 * ndt_mapping.launch:32-36); the rest are PCL defaults and the version-sensitive switches of
 * SURVEY.md 8c; ndt_default_params = ndt_params_pcl110 (presets below). */
typedef struct ndt_params {
  float  resolution;        /* PoseEstimator.h:81  ndt.setResolution             */
  double step_size;         /* PoseEstimator.h:79  ndt.setStepSize               */
  double trans_eps;         /* PoseEstimator.h:77  ndt.setTransformationEpsilon  */
  int    max_iter;          /* PoseEstimator.h:83  ndt.setMaximumIterations      */
  double outlier_ratio;     /* 0.55 */
  int    min_pts;           /* 6    */
  double eig_mult;          /* 0.01 */
  int    cov_unbiased;      /* 0: (Sxx/n - mu mu^T)(n-1)/n ; 1: /(n-1)           */
  int    cov_init_identity; /* 1: per-voxel Sxx accumulator starts at I          */
  int    conv_ge;           /* 0: stop when iter > max_iter ; 1: >=              */
  int    radius_inclusive;  /* 0: d^2 < r^2 ; 1: <=                              */
  int    transform_sse;     /* 0: (m00 x + m01 y) + m03 ; 1: m00 x + (m01 y + m03) */
  int    stale_h_ang;       /* 0 (every preset): the Hessian after an inner line search uses the
                                  2nd-derivative angle terms of the LAST trial (PCL refreshes them on
                                  every computeDerivatives); 1: those of the line search's first trial */
  double snap_thresh;       /* 10e-5 */
  int    mt_max_iter;       /* 10    */
  double mt_mu;             /* 1e-4  */
  double mt_nu;             /* 0.9   */
  int    libm_f32;          /* float32 cos / sin of a trial's yaw, the entries of final_transformation_ (Eigen's
                               AngleAxisf::toRotationMatrix calls std::cos / std::sin on a float):
                               1: glibc >= 2.28's cosf / sinf (x86-64, FMA build: what Ubuntu 20.04 / 22.04 run), restated
                                  operation for operation and equal to libm on all 2.2e9 floats |x| < 120
                                  (tests/test_libm_f32.py); 0: correctly rounded (differs from glibc by one ulp in 1.3 % of
                                  the angles).  asinf / acosf / atan2f stay modelled as correctly rounded: DESIGN.md 2 */
  int    grid_margin;       /* 0 (every preset): the voxel grid is the one PCL's VoxelGridCovariance derives from the cloud's
                               bounding box, and a rebuild whose box has moved by a voxel is queued twice (NDT_REBUILT).
                               m > 0: a grid built or re-queued for this map is that box widened by m voxels on every side,
                               and ndt_map_rebuild_end accepts the grid queued ahead as long as it still contains the
                               cloud's box and is at most 2 m voxels wider on any side -- a sliding local map
                               (src/PointCloudMap.cpp:119-131) then pays the second build once per ~m voxels of travel
                               instead of once per voxel.  Matches, fitness scores and ndt_eval_at do not depend on it,
                               to the last bit (same voxels, same statistics, and the order of every sum follows the scan
                               and the pose, never the grid's extent: tests/test_gpu_parity.py); ndt_map_info and
                               ndt_map_export describe the widened grid */
} ndt_params;

/* Result of one scan-to-map match = everything src/PoseEstimator.cpp:28-64 reads back from
 * PCL after ndt.align(). */
typedef struct ndt_result {
  double pose[3];     /* x, y, yaw[rad] by the asin/acos branch logic of src/PoseEstimator.cpp:31-35
                         applied to the float32 matrix entries below                               */
  float  T00, T10, T03, T13; /* getFinalTransformation() entries (src/PoseEstimator.cpp:29)        */
  double fitness;     /* getFitnessScore() (src/PoseEstimator.cpp:43), m^2; the 1e7 sentinel of
                         :44-46 is applied by the shim, not here                                   */
  double trans_prob;  /* getTransformationProbability() (src/PoseEstimator.cpp:48)                 */
  double score;
  double H[9];        /* rows/cols {0,1,5} of getHessian()'s 6x6 (src/PoseEstimator.cpp:53-61),
                         row-major, before the sign flip of :61                                    */
  double p[3];        /* final fp64 parameter vector (tx, ty, yaw)                                 */
  int    iters;       /* outer Newton iterations                                                   */
  int    evals;       /* derivative passes this library executed                                   */
  int    ref_evals;   /* passes the reference executes on the same path: adds its Hessian-only passes and the
                         getHessian pass (fused here) and the trials of a line search that repeat the step length
                         of the pass before them (same pose, same totals: not run again here)      */
  int    converged;   /* hasConverged() (src/PoseEstimator.cpp:44)                                 */
  int    status;      /* ndt_status of this match                                                  */
  int    flags;       /* NDT_FLAG_* bits: which data path the match took (results do not depend on it)    */
  double kbar;        /* mean in-radius cells per point-evaluation (roofline accounting)           */
} ndt_result;

/* ndt_result.flags */
enum ndt_result_flags {
  NDT_FLAG_WINDOW_SPILL  = 1,  /* occupied voxels of the scan's window had no LDS record: points that reached
                                  them read the cell table from HBM                                          */
  NDT_FLAG_REGION_CLIPPED = 2, /* the scan's voxel bounding box exceeded the LDS window (16384 cells): points
                                  outside it read the cell table from HBM                                    */
  NDT_FLAG_UNSORTED      = 4   /* scan above 20000 points: passes read it in input order                     */
};

typedef struct ndt_map_info {
  int min_bx, min_by, div_x, div_y;
  int n_cells;   /* voxels with >= min_pts points */
  int n_valid;   /* of those, accepted covariances */
  size_t n_points;
} ndt_map_info;

typedef struct ndt_ctx ndt_ctx;
typedef struct ndt_map ndt_map;

/* include/ndt_slam/PoseEstimator.h:63-64 constructor defaults + the PCL-side values, as one of three
 * presets of the version-sensitive switches (PCL is un-vendored and unpinned, CMakeLists.txt:21; the
 * reference compiles only against PCL <= 1.10, include/ndt_slam/PoseEstimator.h:72-73):
 *   ndt_params_pcl110   PCL 1.9 / 1.10 (Ubuntu 20.04, the likely build): VoxelGridCovariance::Leaf() starts
 *                       cov_ at the identity (cov_init_identity = 1), (n-1)/n normalisation
 *                       (cov_unbiased = 0), SSE transformPointCloud (transform_sse = 1), glibc 2.31 (libm_f32 = 1)
 *   ndt_params_pcl18    PCL <= 1.8: the same voxel statistics, scalar transformPointCloud (transform_sse = 0); its
 *                       platform (Ubuntu 18.04, glibc 2.27) has an older sinf / cosf: modelled (libm_f32 = 0)
 *   ndt_params_pcl_new  PCL >= 1.11: cov_ starts at zero, /(n-1) (cov_unbiased = 1), SSE transform, libm_f32 = 1
 * ndt_default_params is ndt_params_pcl110. */
int ndt_default_params(ndt_params *p);
int ndt_params_pcl110(ndt_params *p);
int ndt_params_pcl18(ndt_params *p);
int ndt_params_pcl_new(ndt_params *p);

/* One context per process and device (one process per GPU).  device = HIP ordinal. */
int ndt_ctx_create(int device, ndt_ctx **out);
int ndt_ctx_destroy(ndt_ctx *ctx);               /* destroy the context's maps first */
const char *ndt_last_error(const ndt_ctx *ctx);   /* ctx may be NULL: last global error */
void *ndt_ctx_stream(ndt_ctx *ctx);               /* hipStream_t the context works on   */
/* Tuning of the match launch (defaults are right for whole-GPU batches):
 *   NDT_OPT_MAX_HELPERS  0..15  workgroups that may join the passes of one unfinished scan; 0 = no work sharing;
 *                               -1 = the default: 8, or 2 when the launch has a scan for every workgroup
 *   NDT_OPT_WORKGROUPS   0..#CU workgroups per match launch (0 = one per CU); a smaller value leaves CUs to
 *                               other streams
 * Results never depend on either (unit totals are summed in unit order whoever computed them).
 *   NDT_OPT_INJECT_FAULT k      test instrumentation for the error paths: the k-th next match launch of the context returns
 *                               NDT_E_HIP right behind the dispatch of its first kernel (0 = off, the default).  The call
 *                               leaves the context usable: the kernel that was queued is ordered in front of whatever any
 *                               stream does with the context next.
 *   NDT_OPT_DEFER_FITNESS 0 / 1 for callers with a stream of batches (ndt_align_batch_dev only; default 0).  1: the call queues the
 *                               match kernel on the caller's stream and the fitness kernels on a stream of the context's own
 *                               behind it, so the caller's NEXT launch starts its match kernel at once and the fitness
 *                               kernels fill the CUs its idle workgroups leave.  The records of a launch -- their `fitness`
 *                               field above all -- are then complete at the LAUNCH'S END, not at the caller's stream's
 *                               position behind the call: wait for it with ndt_ctx_wait_launch (or a device-wide
 *                               synchronisation) before reading them, keep scans / offsets / initial guesses alive until
 *                               then, and give two launches in a row different `out` arrays (a launch waits for the end of
 *                               the launch before last by itself).  Every other entry point of the context waits for a
 *                               deferred launch's end before it touches the context.  Same kernels, same records.
 *   NDT_OPT_SCORE_STAGE 0 / 1   the score sweep (ndt_score_*) copies a scan of up to 8000 points into LDS once per workgroup
 *                               (1, the default) or reads every scan from global memory (0), as it does for longer scans.
 *                               Same scores, bit for bit. */
enum ndt_option { NDT_OPT_MAX_HELPERS = 1, NDT_OPT_WORKGROUPS = 2, NDT_OPT_INJECT_FAULT = 3, NDT_OPT_DEFER_FITNESS = 4,
                  NDT_OPT_SCORE_STAGE = 5 };
int ndt_ctx_set_option(ndt_ctx *ctx, int option, long long value);
/* Make the context work on a caller-owned hipStream_t (e.g. the stream a host framework already
 * orders its copies on); NULL restores the context's own stream. */
int ndt_ctx_set_stream(ndt_ctx *ctx, void *stream);

/* Replaces ndt.setInputTarget(target_cloud) (src/PoseEstimator.cpp:19): voxel-grid
 * normal-distributions build plus the raw-point buckets the fitness
 * score searches (replaces the kd-tree Registration::initCompute builds, row a7).
 * xy: points at `stride_bytes` (8 = packed float2, 16 = pcl::PointXYZ).  If *map is non-NULL
 * it is rebuilt in place (the reference's target cloud is refilled every scan,
 * src/PointCloudMap.cpp:119-131).  Host-pointer form copies to the device first. */
int ndt_map_build(ndt_ctx *ctx, const float *xy_host, size_t n, size_t stride_bytes,
                  const ndt_params *prm, ndt_map **map);
int ndt_map_build_dev(ndt_ctx *ctx, const float *xy_dev, size_t n, size_t stride_bytes,
                      const ndt_params *prm, ndt_map **map);
/* The same rebuild in two halves for a pipeline that must not wait on the host: _begin queues the
 * bounding box of the new cloud and, ahead of its read-back, the whole build with the voxel grid of the map's previous
 * build, and returns; launches queued behind it see that build.  _end waits for the bounding box: NDT_OK if the grid
 * was the right one (a SLAM local map keeps its voxel bounding box for many scans, src/PointCloudMap.cpp:119-131),
 * NDT_REBUILT if it was not -- the build has been queued again (behind the launches of ANY context that read the map
 * since _begin: it rewrites the tables they read), and whatever was queued between _begin and _end ran on a stale grid
 * and has to be queued again by the caller.  One _begin may be open per context (other builds on that
 * context fail with NDT_E_ARG until _end); xy_dev must stay as it is until _end has returned.  The map must have been
 * built before at the same resolution. */
#define NDT_REBUILT 1
int ndt_map_rebuild_begin(ndt_ctx *ctx, const float *xy_dev, size_t n, size_t stride_bytes,
                          const ndt_params *prm, ndt_map *map);
int ndt_map_rebuild_end(ndt_ctx *ctx, ndt_map *map);
/* Many maps in one set of launches: replaces ndt.setInputTarget (src/PoseEstimator.cpp:19) for every session of a lockstep
 * step (one ndt_map_build_dev per session before).  Map s is built from n[s] points at xy[s] (stride_bytes as for
 * ndt_map_build) with parameters prm[s]; maps[s] == NULL: a new map is created and stored there, else maps[s] is rebuilt in
 * place.  xy, n, prm and maps are host arrays of n_maps entries; _dev takes device cloud pointers, the host form copies
 * the clouds to a staging buffer of the context first and is synchronous.
 *   Result: each map is what ndt_map_build_dev gives for that map with its history -- the same voxel grid (grid_margin's
 *     rule against the map's previous grid), ndt_map_info, ndt_map_export, raw-point buckets and match view -- so every
 *     other entry point treats it as before.
 *   The call reads back all the bounding boxes with one copy and waits for it once, then queues the rest of the build
 *     (each kernel once for all maps).  No two-phase form.  _dev returns before the build ends (stream order, as
 *     ndt_map_build_dev): xy[s] must stay valid until the build has run on the context's stream.
 *   Refusals (NDT_E_ARG, synchronous, no map changed or created; the text names the first offending index): a NULL
 *     context, n_maps < 1, NULL arrays, xy[s] == NULL, n[s] == 0 or > INT32_MAX, a bad stride, prm[s].resolution <= 0, a
 *     map of another context, the same map twice, an open ndt_map_rebuild_begin on the context.  Behind the box read-back,
 *     also changing nothing: a cloud with no finite point (NDT_E_ARG), a grid beyond 2^28 cells (NDT_E_GRID), grids that
 *     together need more than 2^32 work-items in one kernel (NDT_E_GRID).
 *   A HIP or allocation failure after that leaves the batch's existing maps unusable until they are rebuilt and destroys
 *     the maps the call created (as ndt_map_build_dev for one map).
 *   Ordering: as ndt_map_build_dev, per map (a deferred launch's fitness kernels that read it are waited for);
 *     ndt_last_timing reports the whole call as the build time. */
int ndt_map_build_batch_dev(ndt_ctx *ctx, const float *const *xy_dev, const size_t *n, size_t stride_bytes,
                            int n_maps, const ndt_params *prm, ndt_map **maps);
int ndt_map_build_batch(ndt_ctx *ctx, const float *const *xy_host, const size_t *n, size_t stride_bytes,
                        int n_maps, const ndt_params *prm, ndt_map **maps);
int ndt_map_destroy(ndt_map *map);
int ndt_map_info_get(const ndt_map *map, ndt_map_info *out);
/* Cell table in ascending voxel-index order, arrays sized n_cells (parity tests). */
int ndt_map_export(const ndt_map *map, int *cell_idx, float *cent_xy, double *mean_xy,
                   double *icov_xx_xy_yy, int *npts);

/* Replaces ndt.setInputSource + ndt.align + getFinalTransformation + getFitnessScore +
 * hasConverged + getTransformationProbability + getHessian for ONE scan
 * (src/PoseEstimator.cpp:17-56).  scan = the post-filter source cloud (row a1 stays with the
 * caller); init = (tx, ty, yaw[rad]) as src/PoseEstimator.cpp:22-24 builds the guess.
 * A match with nothing to match -- the guess is not finite, every point of the scan is NaN, or no point reaches a voxel --
 * is legal, here and in every batched form below: the first pass has score 0, a zero gradient and a zero Hessian; the
 * Newton step is then exactly zero and the match ends at once with status 0, iters = 0, converged = 1, p and the float32
 * matrix as the prologue forms them from the guess (NaN where the guess is), pose read from that matrix, and fitness
 * DBL_MAX when no point has a finite image.  Non-finite points are skipped by every pass and never binned: no float is
 * converted to an integer before it is known to be finite.  The checker (oracle/ndt_oracle.c) follows the same rule. */
int ndt_align(ndt_ctx *ctx, const ndt_map *map, const float *scan_xy_host, size_t n,
              size_t stride_bytes, const double init_xyyaw[3], ndt_result *out);

/* Batch of B independent matches against one map (BASELINE.json configs 3-5).  Scans are
 * packed float2, concatenated; offsets[B+1] in points.  shared_scan != 0: every match uses
 * scan 0 (offsets[0..1]) with its own init pose (multi-hypothesis relocalisation).  Such launches keep a scratch
 * slot of the scan's size PER MATCH (ordered copy 8 B, distance 4 B, far-query list 4 B per point: 16 B x n x B)
 * and score the seeds that end far from the map from the map's occupancy words (same `fitness`).
 * Each match with nothing to match ends as ndt_align says; it changes nothing for the other matches of the batch. */
int ndt_align_batch(ndt_ctx *ctx, const ndt_map *map, const float *scans_xy_host,
                    const uint64_t *offsets_host, int B, int shared_scan,
                    const double *inits_host /* B x 3 */, ndt_result *out_host /* B */);
/* Same with every buffer resident in device memory; asynchronous on `stream`
 * (NULL = the context's stream).  out_dev receives B ndt_result records.  total_points = number
 * of points in scans_xy_dev (offsets[B]; the host knows it, the offsets live on the device): it
 * sizes the context's scratch copy in which every scan is kept in the order its lanes walk it. */
int ndt_align_batch_dev(ndt_ctx *ctx, const ndt_map *map, const float *scans_xy_dev,
                        const uint64_t *offsets_dev, int B, size_t total_points, int shared_scan,
                        const double *inits_dev, ndt_result *out_dev, void *stream);
/* Optional first half of ndt_align_batch_dev for a caller with a STREAM of batches: what an alignment needs before its first
 * derivative pass -- the optimiser's start from the initial guess (src/PoseEstimator.cpp:22-24 and computeTransformation's
 * prologue), the window of the voxel grid the scan can reach, the scan's points in voxel order -- depends
 * on the scan, its guess, the grid of `map` and the map's parameters only.  This call queues that work for the whole batch on
 * `stream` (NULL: the context's) as a kernel of its own and returns; a later ndt_align_batch_dev(ctx, map, <the same scans,
 * offsets, B, total_points, shared_scan, inits>, ...) finds the prepared batch, orders its stream behind it and starts every
 * scan at the staging of its window.  Of `map` it uses, by value as they are at the time of the call, the voxel grid's geometry
 * (min_b, div_b, leaf size), transform_sse and the optimiser's parameters (step_size, trans_eps, max_iter, conv_ge,
 * stale_h_ang, snap_thresh, mt_max_iter, mt_mu, mt_nu, libm_f32), and reads nothing on the device, so it needs no ordering
 * against the map's builds: put it where the GPU has room while the previous batch's matches run out (bench.py: on a stream of
 * its own, queued before the step's rebuild).  Rules: the arrays must not change between the two calls -- a caller who
 * prepares, skips the launch and then rewrites the same arrays is not detected; if the map is rebuilt in between (in place,
 * or destroyed and another built at the same address) and any of the values above comes out different (another cloud with
 * another bounding box; a two-phase rebuild whose ndt_map_rebuild_end returns NDT_REBUILT; other parameters) the prepared
 * batch is simply not used, while a rebuild that keeps them all (another cloud, same grid) still finds it; one prepared batch
 * serves one launch; two batches may be prepared ahead per context, and a third prepare call takes the older set's place
 * behind that set's own kernel and its last launch.  Results are byte-identical with and without it (the same device
 * routines run, earlier).  One scan at a time (src/ScanMatcher.cpp:40,45 as the reference calls it) gains nothing from it. */
int ndt_align_batch_prepare_dev(ndt_ctx *ctx, const ndt_map *map, const float *scans_xy_dev,
                                const uint64_t *offsets_dev, int B, size_t total_points, int shared_scan,
                                const double *inits_dev, void *stream);
/* Duration (ms) of the kernel ndt_align_batch_prepare_dev queued for the batches the context's launches used; 0 when
 * none was used.  Blocks until that kernel has run. */
int ndt_prepare_timing(ndt_ctx *ctx, float *order_ms);

/* B independent matches, match b against maps[map_of[b]] (map_of == NULL: match b against maps[b], n_maps == B): one launch
 * for many SLAM sessions, each with its own local map (src/ScanMatcher.cpp:40, src/PointCloudMap.cpp:119-131), or one scan
 * against several candidate submaps.  Scans, offsets, inits, out, total_points and stream as for ndt_align_batch_dev;
 * map_of_dev holds B ints in device memory (ndt_align_batch_multi: map_of_host, host memory; the call is synchronous).
 *   Records: every record is byte-identical to the one ndt_align_batch_dev gives for the same scan, init and map -- flags,
 *     kbar, evals and ref_evals included -- whatever the other maps of the launch, the helper count or the work sharing.
 *   shared_scan != 0: scan 0 is matched from B seeds, each seed against its own map (relocalisation of one scan against K
 *     candidate submaps: B = K x seeds).
 *   Refusals (NDT_E_ARG, synchronous, nothing queued): n_maps < 1, a NULL maps array or map, a map that was never built, a map
 *     on another device than ctx, map_of == NULL with n_maps != B, maps whose match parameters differ -- the optimiser
 *     settings, transform_sse, radius_inclusive, resolution and the Gaussian constants d1 / d2 / e_hi, compared bit for bit
 *     (the launch's kernel instance depends on them); build-only fields such as grid_margin or the covariance switches may
 *     differ.  The error text names the first map that differs.
 *   A map_of[b] outside [0, n_maps): record b alone gets status = NDT_E_ARG, zeroed, converged = 0, fitness = DBL_MAX (as a
 *     failed shard's records, ndt_align_batch_sharded); no kernel reads through that index, the other records are unaffected.
 *   Maps may belong to other contexts of the same device.  The launch is entered as a reader of every distinct map it reads:
 *     a rebuild of any of them (re-queued by ndt_map_rebuild_end, or behind a deferred launch) waits for it; a map between
 *     ndt_map_rebuild_begin and _end is matched with the grid its view holds at the call.
 *   NDT_OPT_DEFER_FITNESS, NDT_OPT_MAX_HELPERS and NDT_OPT_WORKGROUPS apply as for ndt_align_batch_dev.  A multi-map call never
 *     uses a batch prepared by ndt_align_batch_prepare_dev and leaves the prepared batches as they are.
 *   The table of the maps' views is copied to the device once per call from pinned staging; the call waits on the host for
 *     the previous multi-map call's copy of it before it rewrites the staging. */
int ndt_align_batch_multi_dev(ndt_ctx *ctx, const ndt_map *const *maps, int n_maps, const int *map_of_dev,
                              const float *scans_xy_dev, const uint64_t *offsets_dev, int B, size_t total_points,
                              int shared_scan, const double *inits_dev, ndt_result *out_dev, void *stream);
int ndt_align_batch_multi(ndt_ctx *ctx, const ndt_map *const *maps, int n_maps, const int *map_of_host,
                          const float *scans_xy_host, const uint64_t *offsets_host, int B, int shared_scan,
                          const double *inits_host, ndt_result *out_host);

/* Many matches over several GPUs from ONE process (north_star: "batch across the 8 GPUs of one node"; SURVEY.md 8b's
 * indicative multi-device context): `ctxs[r]` / `maps[r]` are a context of device r and a map built there from the same
 * cloud.  The batch is cut into n_shards contiguous, balanced shards (matches [r B / n, (r + 1) B / n), the first B % n
 * one longer -- the partition of ndt_slam_amd/shard.py), every shard is uploaded straight to its device, all launches
 * run side by side, the records come back into results[0 .. B) in batch order.  No exchange between devices: the
 * matches are independent given the read-only map, so a batch that starts on the host needs no xGMI
 * traffic at all.  `shared_scan`: the one scan goes to every device, the B seed poses are sharded.  Synchronous; same
 * results as ndt_align_batch on one device, byte for byte.  (One process per GPU over torch.distributed / RCCL is the
 * other form: ndt_slam_amd/shard.py.)  Replaces a loop of src/ScanMatcher.cpp:40,45 over independent scans.
 * Errors: every shard is attempted; the call returns the FIRST shard's error code.  The records of a shard that failed
 * are all overwritten -- zeroed, `status` = that shard's error, `converged` = 0, `fitness` = DBL_MAX (the shim's 1e7
 * case, src/PoseEstimator.cpp:44-46) -- and the records of the shards that succeeded are complete, so `status` tells
 * per record what can be used (tests/test_gpu_parity.py::test_sharded_batch_marks_every_record_of_a_failed_shard). */
int ndt_align_batch_sharded(ndt_ctx *const *ctxs, const ndt_map *const *maps, int n_shards, const float *scans_xy_host,
                            const uint64_t *offsets, int B, int shared_scan, const double *inits_xyyaw,
                            ndt_result *results);
/* As ndt_align_batch, additionally recording per derivative pass of every match
 * 8 doubles {a_t, score, g0, g1, g2, p0, p1, p2} (parity tests: same step sequence as the
 * oracle).  trace_host: B x trace_cap x 8 doubles; trace_rows_host: B ints. */
int ndt_align_batch_trace(ndt_ctx *ctx, const ndt_map *map, const float *scans_xy_host,
                          const uint64_t *offsets_host, int B, int shared_scan,
                          const double *inits_host, ndt_result *out_host, double *trace_host,
                          int trace_cap, int *trace_rows_host);

/* One derivative pass at an explicit pose (rows a4+a5; parity tests and profiling):
 * score, gradient[3], Hessian[9] of d(score)/dp at p = (tx, ty, yaw). */
int ndt_eval_at(ndt_ctx *ctx, const ndt_map *map, const float *scan_xy_host, size_t n,
                size_t stride_bytes, const double p[3], double *score, double g[3], double H[9],
                double *pairs);
/* Fitness score alone at an explicit float32 transform (row a7). */
int ndt_fitness_at(ndt_ctx *ctx, const ndt_map *map, const float *scan_xy_host, size_t n,
                   size_t stride_bytes, float c, float s, float tx, float ty, double *fitness);

/* Replaces the source pre-filter pcl::ApproximateVoxelGrid::filter (src/PoseEstimator.cpp:6-10:
 * setLeafSize(LeafSize x3), setInputCloud(source_cloud), filter(*filtered_cloud); SURVEY.md 8a row
 * a1 / 8f row f1) on z = 0 clouds: 512-slot direct-mapped voxel history, flush on collision, the
 * rest flushed in slot order -- same centroids (float32 sums in cloud order), same output order.
 * Single scan, host pointers; out_xy_host needs room for n points; *n_out = points written.
 * A scan that holds a non-finite coordinate, or one with |x / leaf| >= 2^31, gets an unspecified
 * result (the reference's float -> int conversion is undefined there), but a deterministic one that
 * stays within the scan's bounds: 1..n points.  Every other scan of a batch is unaffected
 * (tests/test_gpu_prefilter_families.py::test_an_undefined_scan_is_isolated). */
int ndt_prefilter(ndt_ctx *ctx, const float *xy_host, size_t n, size_t stride_bytes, float leaf,
                  float *out_xy_host, size_t *n_out);
/* Batch of B raw scans resident in device memory (points at stride_bytes, raw_offsets[B+1] in
 * points).  Writes the filtered scans packed as float2 to out_xy_dev (capacity total_raw_points
 * points) and their offsets[B+1] to out_offsets_dev: exactly the inputs of ndt_align_batch_dev,
 * whose total_points may be given as total_raw_points (an upper bound).  Asynchronous on `stream`
 * (NULL = the context's stream). */
int ndt_prefilter_batch_dev(ndt_ctx *ctx, const float *raw_xy_dev, size_t stride_bytes,
                            const uint64_t *raw_offsets_dev, int B, size_t total_raw_points, float leaf,
                            float *out_xy_dev, uint64_t *out_offsets_dev, void *stream);

/* The two ends of ScanMatcher::matchScan for a batch: the resampler before the match and growMap's
 * transform after it (src/ScanMatcher.cpp:6, :92-107).  Raw scans are LPoint2D x, y doubles
 * (include/ndt_slam/LPoint2D.h:17-18) at stride_bytes (>= 16, a multiple of 8).
 *
 * Output bound of ndt_resample*: *capacity = total_points * k_max, where k_max = 1 if
 * space_thre <= space, else floor(space_thre / space) + 2 (the most points one input point can
 * emit).  Needs no context and no device.  NDT_E_ARG for a negative or non-finite parameter, for
 * space == 0 < space_thre (the reference interpolates at distance 0 forever there) and when the
 * product overflows. */
int ndt_resample_capacity(size_t total_points, double space, double space_thre, size_t *capacity);
/* Replaces ScanPointResampler::resamplePoints (src/ScanPointResampler.cpp:4-62, called at
 * src/ScanMatcher.cpp:6) for a batch of B raw scans in device memory (raw_offsets[B+1] in points),
 * bit for bit.  Writes the packed results: out_xy64_dev as double2 and/or out_xy32_dev as float2
 * (the double -> float32 conversion of setScanPair, include/ndt_slam/PoseEstimator.h:91-104: exactly
 * the input of ndt_prefilter_batch_dev); either may be NULL, not both; each needs room for
 * ndt_resample_capacity(total_raw_points) points.  out_offsets_dev[B+1] in points.  status_dev: B
 * ints or NULL; NDT_E_ARG marks a scan that holds a non-finite coordinate (its output range is then
 * empty), NDT_OK the others.  Parameters are checked as ndt_resample_capacity checks them.
 * growMap's ISOLATE skip (src/ScanMatcher.cpp:98) never fires on a resampled scan: every point is
 * created anew with type UNKNOWN (include/ndt_slam/LPoint2D.h:28-42), so no type array is taken.
 * Asynchronous on `stream` (NULL = the context's stream). */
int ndt_resample_batch_dev(ndt_ctx *ctx, const double *raw_xy_dev, size_t stride_bytes,
                           const uint64_t *raw_offsets_dev, int B, size_t total_raw_points, double space,
                           double space_thre, double *out_xy64_dev, float *out_xy32_dev,
                           uint64_t *out_offsets_dev, int *status_dev, void *stream);
/* The same for one scan of n points in host memory; out_xy_host needs room for
 * ndt_resample_capacity(n) points (double2); *n_out = points written.  Synchronous, like
 * ndt_prefilter.  NDT_E_ARG for a non-finite coordinate. */
int ndt_resample(ndt_ctx *ctx, const double *xy_host, size_t n, size_t stride_bytes, double space,
                 double space_thre, double *out_xy_host, size_t *n_out);
/* Replaces ScanMatcher::growMap's transform (src/ScanMatcher.cpp:96-101), followed by
 * PointCloudMap::addPoints' conversion to float32 with z = 0: the resampled scans (doubles at
 * stride_bytes, offsets_dev[B+1]) with B poses (tx, ty, th[deg]; Rmat as Pose2D::calRmat,
 * include/ndt_slam/Pose2D.h:43-47) -> map-frame float2 points at the same offsets in out_xy_dev,
 * ready for ndt_make_map_dev.  Asynchronous on `stream` (NULL = the context's stream). */
int ndt_scan_to_map_batch_dev(ndt_ctx *ctx, const double *xy_dev, size_t stride_bytes,
                              const uint64_t *offsets_dev, int B, size_t total_points,
                              const double *poses_dev, float *out_xy_dev, void *stream);

/* SURVEY.md 8f row f2 -- the steps either side of the match, for a batch resident in device
 * memory.  Poses are (tx, ty, th) triples of doubles with th in DEGREES (include/ndt_slam/Pose2D.h:14);
 * covariances are row-major 3x3 in (m, m, rad). */
typedef struct ndt_fuse_params {
  double coe_ndt_cov;  /* include/ndt_slam/PoseEstimator.h:63  coeNDTCov  (1.0) */
  double coe_vel;      /* include/ndt_slam/PoseFuser.h:19      coeVel     (0.1) */
  double coe_omega;    /* include/ndt_slam/PoseFuser.h:19      coeOmega   (0.1) */
  double del_time;     /* include/ndt_slam/PoseFuser.h:19      delTime    (0.5) */
  double score_thre;   /* include/ndt_slam/ScanMatcher.h:49-50 scthre     (0.0; launch file sets score_thre) */
} ndt_fuse_params;
int ndt_fuse_default_params(ndt_fuse_params *p);
/* Replaces Pose2D::calMotion (src/Pose2D.cpp:5-16) + Pose2D::calPredPose (:28-37) as
 * ScanMatcher::matchScan chains them (src/ScanMatcher.cpp:27-32): odometry motion in the robot
 * frame, predicted pose, and (if init_xyyaw_dev != NULL) the same pose as the (tx, ty, yaw[rad])
 * guess ndt_align_batch_dev takes.  All arrays B x 3 doubles in device memory; asynchronous. */
int ndt_predict_batch_dev(ndt_ctx *ctx, const double *odo_cur_dev, const double *odo_prev_dev,
                          const double *last_pose_dev, int B, double *odo_motion_dev, double *pred_pose_dev,
                          double *init_xyyaw_dev, void *stream);
/* Replaces, per match: cost with the 1e7 sentinel and Qmat = (-H)^-1 * coeNDTCov
 * (src/PoseEstimator.cpp:43-64), the accept test cost <= scthre (src/ScanMatcher.cpp:50), then
 * PoseFuser::fusePose (src/PoseFuser.cpp:3-37) or, for a rejected match, the predicted pose with
 * PoseFuser::calOdometryCovariance (src/PoseFuser.cpp:39-61; src/ScanMatcher.cpp:60-66).
 * results_dev: B records as written by ndt_align_batch_dev; last_cov_dev, cov_dev: B x 9;
 * successful_dev: B ints or NULL.  Asynchronous on `stream`. */
int ndt_fuse_batch_dev(ndt_ctx *ctx, const ndt_result *results_dev, const double *pred_pose_dev,
                       const double *odo_motion_dev, const double *last_pose_dev, const double *last_cov_dev,
                       int B, const ndt_fuse_params *prm, double *fused_pose_dev, double *cov_dev,
                       int *successful_dev, void *stream);

/* SURVEY.md 8f row f3 (the all-pairs step on its own) -- replaces PCFilter::remove_neighborPoint(cloud_base, point_list)
 * (include/ndt_slam/PCFilter.h:29-56, called from Submap::makeMap, src/PointCloudMap.cpp:27): the points
 * of `base` with no point of `list` closer than thre_neighbor (PCLUtil::distance_points' float32
 * distance, include/ndt_slam/PCLUtil.h:21-23, strict <), in input order, packed as float2.
 * out needs room for n_base points; n_list may be 0 (list_xy may then be NULL: every point is kept).
 * Refusals (NDT_E_ARG, nothing written): a NULL context, base_xy, out_xy or n_out, n_base == 0, n_base or n_list above
 * INT32_MAX, n_list > 0 with a NULL list, a stride below 8, not a multiple of 8, or above UINT32_MAX. */
int ndt_remove_neighbors(ndt_ctx *ctx, const float *base_xy_host, size_t base_stride_bytes, size_t n_base,
                         const float *list_xy_host, size_t list_stride_bytes, size_t n_list, double thre_neighbor,
                         float *out_xy_host, size_t *n_out);
/* Same with device pointers; *n_out_dev is a uint64 in device memory; asynchronous on `stream`. */
int ndt_remove_neighbors_dev(ndt_ctx *ctx, const float *base_xy_dev, size_t base_stride_bytes, size_t n_base,
                             const float *list_xy_dev, size_t list_stride_bytes, size_t n_list,
                             double thre_neighbor, float *out_xy_dev, uint64_t *n_out_dev, void *stream);

/* SURVEY.md 8f row f3 -- replaces PCFilter::difference_extraction(cloud_base, cloud_test)
 * (include/ndt_slam/PCFilter.h:58-94): the points of `test` that fall in leaf voxels (side `resol`) of
 * pcl::octree::OctreePointCloudChangeDetector which hold no point of `base`.  The voxel lattice is the
 * octree's own: anchored by the first point added (base first, then test) and carried through every
 * doubling of the bounding box with the keys computed in fp64 as PCL computes them.  z is taken as 0
 * (PointCloudMap::addPoints, src/PointCloudMap.cpp:71); non-finite points are skipped as PCL skips them.
 * The points come back in INPUT order, packed as float2; PCL returns the same set in the order of its
 * depth-first leaf walk, which nothing downstream depends on (the list only feeds remove_neighborPoint).
 * out needs room for n_test points; n_base may be 0.  NDT_E_ARG when the two clouds span more than 2^30
 * voxels per axis (PCL's own key width is 32 bits).
 * Refusals (NDT_E_ARG, nothing written): a NULL context or array, more than 2^30 points in all, a resol that is not
 * positive and finite, a stride below 8, not a multiple of 8, or above UINT32_MAX. */
int ndt_difference_extraction(ndt_ctx *ctx, const float *base_xy_host, size_t base_stride_bytes, size_t n_base,
                              const float *test_xy_host, size_t test_stride_bytes, size_t n_test, double resol,
                              float *out_xy_host, size_t *n_out);
/* Same with device pointers; *n_out_dev is a uint64 in device memory (UINT64_MAX on the span error);
 * asynchronous on `stream`. */
int ndt_difference_extraction_dev(ndt_ctx *ctx, const float *base_xy_dev, size_t base_stride_bytes, size_t n_base,
                                  const float *test_xy_dev, size_t test_stride_bytes, size_t n_test, double resol,
                                  float *out_xy_dev, uint64_t *n_out_dev, void *stream);
/* Replaces Submap::makeMap (src/PointCloudMap.cpp:15-39): the submap's cloud from its scans (already in the
 * map frame), scan i = points [offsets[i], offsets[i+1]) of scans_xy.  With remove_moving: scans[0] when
 * first_submap (cntS == 0), then for every triple (i, i+1, i+2) the points of scan i+1 that are not within
 * thre_neighbor of a point of difference_extraction(scan i ++ scan i+2, scan i+1), then the last scan when
 * `newest`; without: all scans (first submap) or scans 2.. (later ones).  All triples run side by side, one
 * workgroup each.  out needs room for every input point (twice that for n_scans == 1: the reference then
 * appends the lone scan as the first and again as the newest).  resol / thre_neighbor are PCFilter's `resol` (0.05) and `thre_neighbor` (0.1),
 * include/ndt_slam/PCFilter.h:20-23.
 * Refusals (NDT_E_ARG, nothing written): a NULL context or array, n_scans < 1 or above 2^20, offsets that decrease or a scan
 * above 2^29 points, remove_moving with a resol that is not positive and finite or a thre_neighbor that is not finite, a
 * stride below 8, not a multiple of 8, or above UINT32_MAX. */
int ndt_make_map(ndt_ctx *ctx, const float *scans_xy_host, size_t stride_bytes, const uint64_t *offsets, int n_scans,
                 int first_submap, int newest, int remove_moving, double resol, double thre_neighbor,
                 float *out_xy_host, size_t *n_out);
/* Same with the points in device memory (offsets stay on the host); *n_out_dev is a uint64 in device memory
 * (UINT64_MAX on the span error); asynchronous on `stream`.  The result can be handed to
 * ndt_prefilter_batch_dev / ndt_map_build_dev without leaving the device. */
int ndt_make_map_dev(ndt_ctx *ctx, const float *scans_xy_dev, size_t stride_bytes, const uint64_t *offsets,
                     int n_scans, int first_submap, int newest, int remove_moving, double resol,
                     double thre_neighbor, float *out_xy_dev, uint64_t *n_out_dev, void *stream);

/* The same pre-filter for B scans in host memory (scan b = points [raw_offsets[b], raw_offsets[b+1]) of raw_xy_host at
 * stride_bytes): one upload, one ndt_prefilter_batch_dev, the offsets read back, one copy of the result.  Scan b's filtered
 * points are [out_offsets_host[b], out_offsets_host[b+1]) of out_xy_host (packed float2; room for every input point), each
 * byte-identical to ndt_prefilter of that scan; an empty scan stays empty (a call whose scans are all empty is valid).
 * Synchronous.  NDT_E_ARG (nothing changed): a NULL context ("null context"), B < 1, a NULL array, a bad stride,
 * leaf <= 0, offsets that decrease (the text names the scan). */
int ndt_prefilter_batch(ndt_ctx *ctx, const float *raw_xy_host, size_t stride_bytes, const uint64_t *raw_offsets_host,
                        int B, float leaf, float *out_xy_host, uint64_t *out_offsets_host);

/* SURVEY.md 8f row f3 for many submaps at once -- Submap::makeMap (src/PointCloudMap.cpp:15-39) and the local map that
 * PointCloudMap::makeLocalMap (:119-134) makes of it, for n_subs independent submaps (one per SLAM session) in ONE set of
 * launches: the number of kernels, copies and host waits of a call does not depend on n_subs.
 *
 * One entry of the HOST array `subs` per submap: */
typedef struct ndt_submap_desc {
  const float    *scans_xy;      /* the submap's scans, already in the map frame (as ndt_make_map), points at stride_bytes */
  const uint64_t *offsets;       /* HOST array, n_scans + 1 entries, in points of scans_xy                                 */
  int             n_scans;
  int             first_submap, newest, remove_moving;   /* as ndt_make_map                                                */
  double          resol, thre_neighbor;                  /* PCFilter's, per submap                                         */
  const float    *prev_xy;       /* p_cloud of the submap before this one (makeLocalMap :123-126) at stride_bytes, or NULL */
  size_t          n_prev;
} ndt_submap_desc;
/* For submap s the call writes
 *   cloud[s]  = points [cloud_off[s], cloud_off[s+1]) of cloud_xy: what ndt_make_map_dev gives for that submap, byte for
 *               byte (Submap::p_cloud after makeMap);
 *   target[s] = points [target_off[s], target_off[s+1]) of target_xy: prev[s] (n_prev points) followed by
 *               Submap::filterPoints of cloud[s] at leaf size `leaf` -- makeLocalMap's localMap_cloud, and what
 *               ndt_map_build_batch_dev takes as xy[s] once target_off has been read back.  The part behind the first n_prev
 *               points is byte-identical to ndt_prefilter(cloud[s], leaf); an empty cloud[s] gives an empty filtered part;
 *   status[s] = NDT_OK, or NDT_E_ARG when one of the submap's scan triples spans more than 2^30 voxels: that submap alone
 *               gets empty ranges in both outputs (the single call reports this as *n_out = UINT64_MAX).
 * Both outputs are packed float2.  With target_xy_dev == NULL (then target_off_dev must be NULL too) the call is a batched
 * ndt_make_map_dev: leaf, prev_xy and n_prev are ignored.  One leaf per call; resol and thre_neighbor per submap.
 *
 * Buffer sizes, computable without a device:
 *   cloud capacity  (points) = the sum over the submaps of their input points, offsets[n_scans] - offsets[0], counting a
 *                              submap of a single scan TWICE (ndt_make_map appends a lone scan as the first and as the newest);
 *   target capacity (points) = the cloud capacity + the sum of n_prev;
 *   cloud_off, target_off: n_subs + 1 uint64 each; status: n_subs ints.
 * The inputs (scans and previous clouds; not `subs` and the offsets, which are read before the call returns) must stay
 * valid until the call has run on its stream; the outputs must not overlap the inputs.  Asynchronous on `stream`
 * (NULL = the context's stream).
 *
 * Refusals (NDT_E_ARG, synchronous, nothing written or queued; the text names the first offending submap): a NULL context
 * ("null context", checked first), n_subs < 1, a NULL array (subs, cloud_xy, cloud_off, status; target_xy without
 * target_off or the reverse), a submap with n_scans < 1 or NULL scans_xy / offsets, offsets that decrease or a scan above
 * 2^29 points, a bad stride (below 8, not a multiple of 8, or above UINT32_MAX), remove_moving with a resol that is not positive and finite, n_prev > 0 with NULL prev_xy, a
 * target with leaf <= 0.  A call in which every submap is empty is valid and gives all-zero offsets. */
int ndt_local_map_batch_dev(ndt_ctx *ctx, const ndt_submap_desc *subs, int n_subs, size_t stride_bytes, float leaf,
                            float *cloud_xy_dev, uint64_t *cloud_off_dev, float *target_xy_dev, uint64_t *target_off_dev,
                            int *status_dev, void *stream);
/* The same with every point pointer (scans_xy, prev_xy, cloud_xy, target_xy) and every result in HOST memory: one upload of
 * all scans and previous clouds, one ndt_local_map_batch_dev, one read-back of the offsets and status, one copy of each
 * result.  Synchronous; same capacities, same refusals. */
int ndt_local_map_batch(ndt_ctx *ctx, const ndt_submap_desc *subs, int n_subs, size_t stride_bytes, float leaf,
                        float *cloud_xy_host, uint64_t *cloud_off_host, float *target_xy_host, uint64_t *target_off_host,
                        int *status_host);

/* Device-resident lockstep sessions: replaces, for n_sessions independent SLAM sessions stepped together, the whole of
 * ScanMatcher::matchScan + growMap (src/ScanMatcher.cpp:4-116), PointCloudMap::addPose / addPoints / makeLocalMap /
 * makeGlobalMap (src/PointCloudMap.cpp:44-134) and the part of FrontEnd::process that drives them (src/FrontEnd.cpp), with
 * every session's scans, submap clouds, local map, NDT map, last pose and covariance kept in device memory from step to
 * step.  One ndt_sessions_step takes the new raw scans and odometry up and brings the fused poses down (DESIGN.md 4.10;
 * the call sequence in INTEGRATION.md 5.3).  A step is the step of the chain ndt_resample_batch_dev ->
 * ndt_prefilter_batch_dev -> ndt_predict_batch_dev -> ndt_align_batch_multi_dev -> ndt_fuse_batch_dev ->
 * ndt_scan_to_map_batch_dev -> ndt_local_map_batch_dev -> ndt_map_build_batch_dev with PointCloudMap's bookkeeping on the
 * host, byte for byte, except that of a submap's scan triples only the newest is computed (the survivors of the earlier ones
 * are kept), and that nothing but the records below crosses the bus.  The number of kernels, copies and host waits (three)
 * of a step does not depend on n_sessions or on the length of a submap. */
typedef struct ndt_session_params {   /* one set of parameters per session set; a sweep uses several sets */
  ndt_params      match;              /* PoseEstimator's (include/ndt_slam/PoseEstimator.h:63-84); grid_margin as given (the shims use 8) */
  ndt_fuse_params fuse;               /* coeNDTCov, coeVel, coeOmega, delTime, score_thre */
  double space, space_thre;           /* ScanPointResampler (src/ScanPointResampler.cpp:4-62) */
  float  leaf;                        /* LeafSize: source pre-filter (src/PoseEstimator.cpp:6-10) and Submap::filterPoints (src/PointCloudMap.cpp:4-13) */
  double resol, thre_neighbor;        /* PCFilter (include/ndt_slam/PCFilter.h:20-23) */
  double sep_thre;                    /* PointCloudMap sepThre (src/PointCloudMap.cpp:72) */
  int    remove_moving;
} ndt_session_params;
typedef struct ndt_sessions ndt_sessions;
typedef struct ndt_session_step {     /* one per session and step, HOST memory */
  double pose[3];                     /* fused pose (tx, ty, th[deg]) = what savePose stores (src/ScanMatcher.cpp:76-80) */
  double cov[9];
  double cost;                        /* fitness with the 1e7 sentinel (src/PoseEstimator.cpp:43-46); 0 for a first scan */
  int    stepped;                     /* 0: inactive or skipped this step, state untouched */
  int    matched;                     /* 0: first scan, taken as it is at its odometry pose (src/ScanMatcher.cpp:9-22) */
  int    successful;                  /* matchScan's return value (1 for a first scan) */
  int    status;                      /* NDT_OK, or NDT_E_ARG for a raw scan with a non-finite coordinate: that session alone
                                         skips the step; also NDT_E_ARG (stepped = 1) when the newest scan triple spans more
                                         than 2^30 voxels: that session's clouds of this step are empty and its map is kept;
                                         or the code ndt_map_build_batch_dev gives the session's new local map on its own
                                         (stepped = 1; NDT_E_GRID: a voxel grid beyond 2^28 cells, NDT_E_ARG: no finite
                                         point): pose, scans and clouds of the step are as computed, the session's map is
                                         left exactly as it was (a session without a map stays without one) until a later
                                         local map builds.  Either way that session alone is concerned: every other
                                         session steps as in a set without it, and the call returns NDT_OK */
  int    submap;                      /* index of the session's current submap after the step */
  int    split;                       /* 1: this step closed a submap (src/PointCloudMap.cpp:72-90) */
} ndt_session_step;
typedef struct ndt_sessions_stats {   /* of the most recent step, ndt_sessions_correct or ndt_sessions_remake_closed */
  uint64_t h2d_bytes, d2h_bytes;      /* bytes the step copied to and from the device */
  int host_waits;                     /* times the step waited for the device on the host */
  int triples_run;                    /* scan triples the step computed (at most one per stepped session) */
  int sessions_stepped;
} ndt_sessions_stats;

/* ndt_default_params (grid_margin 8, as the shims set it) + ndt_fuse_default_params + the values of ndt_mapping.launch:8-36. */
int ndt_session_default_params(ndt_session_params *p);
/* Refusals of every call below (NDT_E_ARG, synchronous, nothing changed, the text names the first offending index): a NULL
 * context or set, checked first ("null context" / "null session set"); n_sessions < 1; parameters the single entry points
 * refuse (leaf <= 0, resolution <= 0, del_time <= 0, a bad stride, resol not positive and finite with remove_moving, the
 * resampler's parameter rules, ndt_resample_capacity); NULL arrays; offsets that decrease; an open ndt_map_rebuild_begin on the
 * context.  A HIP failure inside a step leaves the SET unusable (every later call on it returns NDT_E_HIP; destroy it) and
 * the context usable.  The set works on the context's stream and is bound to the context's host thread; destroy it before
 * the context.  The maps are owned by the set and destroyed with it. */
int ndt_sessions_create(ndt_ctx *ctx, int n_sessions, const ndt_session_params *prm, ndt_sessions **out);
int ndt_sessions_destroy(ndt_sessions *s);
/* One lockstep step (src/FrontEnd.cpp:20-33 for every session at once).  raw scans: LPoint2D x, y doubles
 * (include/ndt_slam/LPoint2D.h:17-18) at stride_bytes (>= 16, a multiple of 8), session i's scan = points
 * [raw_offsets[i], raw_offsets[i+1]) (raw_offsets[S+1] in points; an empty range is legal: the scan then has no points, and
 * a matched session gets the not-converged cost as ndt_align_batch_multi's NDT_E_ARG record gives it).  odo: S x 3
 * (tx, ty, th[deg]), the scan's odometry pose.  active: S bytes or NULL (= all); a session with active[i] == 0 is not touched
 * (start_frame, end_frame, logs of different lengths).  out_host: S records.  Synchronous. */
int ndt_sessions_step(ndt_sessions *s, const double *raw_xy_host, size_t stride_bytes,
                      const uint64_t *raw_offsets_host, const double *odo_host,
                      const unsigned char *active, ndt_session_step *out_host);
/* the same with raw_xy and odo in DEVICE memory; offsets, active and out stay on the host */
int ndt_sessions_step_dev(ndt_sessions *s, const double *raw_xy_dev, size_t stride_bytes,
                          const uint64_t *raw_offsets_host, const double *odo_dev,
                          const unsigned char *active, ndt_session_step *out_host);
/* Views of the resident state of session i, valid until the next step or ndt_sessions_correct: the local map (PointCloudMap::localMap_cloud,
 * src/PointCloudMap.cpp:119-134; packed float2 in device memory) with the NDT map built from it, and the current submap's
 * cloud (Submap::p_cloud after makeMap, src/PointCloudMap.cpp:15-39).  Before the session's first step: no points, no map. */
int ndt_sessions_local_map(const ndt_sessions *s, int i, const float **xy_dev, size_t *n, const ndt_map **map);
int ndt_sessions_submap_cloud(const ndt_sessions *s, int i, const float **xy_dev, size_t *n);
/* makeGlobalMap as of now (src/PointCloudMap.cpp:101-117): every closed submap's p_cloud, then filterPoints of the current
 * one, to HOST memory (packed float2).  sub_offsets: n_submaps + 1 entries, in points.  A call with out_xy_host == NULL
 * returns the sizes (*n_out, *n_submaps); capacity in points. */
int ndt_sessions_global_map(ndt_sessions *s, int i, float *out_xy_host, size_t capacity, size_t *n_out,
                            uint64_t *sub_offsets, int *n_submaps);
int ndt_sessions_get_stats(const ndt_sessions *s, ndt_sessions_stats *out);

/* ---- Relocalisation: score a pose lattice, pick candidates, refine --------------------------------------------------------
 * The reference has NO counterpart.  Every match it runs starts from the odometry prediction (src/ScanMatcher.cpp:40,45 ->
 * src/PoseEstimator.cpp:22-28), and its answer to a failed match is src/ScanMatcher.cpp:60-66: the fused pose falls back to
 * the prediction and the session stays lost.  These calls are the coarse half of coarse-to-fine for a caller that has no
 * guess inside the NDT basin (about one voxel and a few degrees wide): the NDT score alone -- eq. 6.9's sum, what
 * computeDerivatives returns as `score` (src/PoseEstimator.cpp:28 -> ndt.align), without gradient or Hessian -- of one scan
 * at a very large number of poses in one launch, a deterministic pick of the few poses worth refining, and the existing
 * shared-scan match from those.  The score of a pose list is also what a particle filter takes as weights. */

/* A regular lattice of poses.  Index = (k * ny + j) * nx + i (yaw-major, x fastest); pose = (x0 + (double)i * step_x,
 * y0 + (double)j * step_y, yaw0 + (double)k * step_yaw), each component one rounded multiply and one rounded add (no fused
 * multiply-add).  Yaw in radians, not wrapped.  Steps may be negative or zero. */
typedef struct ndt_pose_lattice {
  double x0, y0, yaw0;
  double step_x, step_y, step_yaw;
  int nx, ny, nyaw;
} ndt_pose_lattice;
/* Number of poses / pose `index` of a lattice.  Host only: no context, no device.  ndt_lattice_pose IS the definition of a
 * lattice pose: the device forms the same bits.  NDT_E_ARG: a NULL pointer, a dimension below 1, a non-finite origin or
 * step, more than 2^31 - 1 poses, index out of range. */
int ndt_lattice_size(const ndt_pose_lattice *lattice, uint64_t *n_poses);
int ndt_lattice_pose(const ndt_pose_lattice *lattice, uint64_t index, double pose_xyyaw[3]);

/* The score sweep.  For pose p: score[p] = -d1 * (sum of e over every (point, voxel) pair), pairs[p] = the number of pairs --
 * the pairs and the e of ndt_eval_at at that pose, term for term the same doubles (the float32 transform of the map's
 * ndt_params, the 3 x 3 neighbourhood with the radius test on float32 centroids, updateDerivatives' check on e).  A
 * non-finite scan point adds nothing; a pose with a non-finite component gets score 0 and pairs 0.
 * A pose's score and pairs are a function of the map, the scan and the pose to the last bit: they do not depend on the
 * pose's place in the list, the other poses, P, lattice or list form, NDT_OPT_WORKGROUPS, NDT_OPT_SCORE_STAGE or the stride
 * (the order of summation is fixed per pose).
 * _dev: every pointer a device address (poses_dev: P x 3 doubles; pairs_dev may be NULL); asynchronous on `stream` (NULL = the
 * context's), behind the map's build; the call is entered among the map's readers as a match launch is, so a rebuild of the
 * map queued behind it -- on whatever stream -- waits for it.  ndt_score_poses: host pointers, synchronous.
 * Refusals (NDT_E_ARG, synchronous, nothing queued): a NULL context ("null context"), a NULL map, scan, poses or score, a map
 * never built or of another device, n == 0 or n > INT32_MAX, P < 1 or P > 2^31 - 1, stride_bytes < 8 or not a multiple of 8
 * (as ndt_eval_at), a lattice ndt_lattice_size refuses, an open ndt_map_rebuild_begin on the context. */
int ndt_score_poses_dev(ndt_ctx *ctx, const ndt_map *map, const float *scan_xy_dev, size_t n, size_t stride_bytes,
                        const double *poses_dev, uint64_t P, double *score_dev, uint32_t *pairs_dev, void *stream);
int ndt_score_lattice_dev(ndt_ctx *ctx, const ndt_map *map, const float *scan_xy_dev, size_t n, size_t stride_bytes,
                          const ndt_pose_lattice *lattice, double *score_dev, uint32_t *pairs_dev, void *stream);
int ndt_score_poses(ndt_ctx *ctx, const ndt_map *map, const float *scan_xy_host, size_t n, size_t stride_bytes,
                    const double *poses_host, uint64_t P, double *score_host, uint32_t *pairs_host);

/* The candidate pick over a lattice's score volume (device pointers, asynchronous on `stream`).  A pose is eligible when
 * pairs > 0 and, with local_max != 0, score > neighbour for each of its up to 26 lattice neighbours of LOWER index and
 * score >= neighbour for each of HIGHER index (neighbours outside the lattice do not exist, the yaw does not wrap: a plateau
 * yields exactly its lowest-index pose).  cand_index_dev[0 .. *n_cand_dev) = the min(top_k, eligible) eligible poses of
 * largest score, in descending score, ties to the lower index.  top_k in 1 .. 1024.  Refusals as above. */
int ndt_lattice_select_dev(ndt_ctx *ctx, const ndt_pose_lattice *lattice, const double *score_dev, const uint32_t *pairs_dev,
                           int top_k, int local_max, uint64_t *cand_index_dev, int *n_cand_dev, void *stream);

/* Sweep, pick, one read-back of the number of candidates (the call's one host wait before the match), then
 * ndt_align_batch_dev's launch with shared_scan = 1 and B = n_cand from the candidates' lattice poses (formed on the device),
 * and the records back.  Synchronous.  cand_index / cand_score / records need room for top_k entries; the first *n_cand are
 * written.  records[c] is byte-identical to what ndt_align_batch with shared_scan gives for the same scan, map and those
 * initial guesses.  A record's cost is `converged ? fitness : 1e7`, the reference shim's sentinel
 * (src/PoseEstimator.cpp:43-46); *best = the index of the lowest cost, ties to the lower index, or -1 when *n_cand == 0 (the
 * scan met no voxel anywhere on the lattice; the call still returns NDT_OK).  scores_host: P doubles for the whole volume,
 * or NULL.  _dev: the scan already in device memory, every other pointer host memory.
 * Where the reference falls back to odometry after a rejected match (src/ScanMatcher.cpp:60-66), a caller runs this
 * instead.  Refusals: those of the sweep and the pick, and a NULL params or output pointer. */
typedef struct ndt_reloc_params { ndt_pose_lattice lattice; int top_k; int local_max; } ndt_reloc_params;
int ndt_relocalize(ndt_ctx *ctx, const ndt_map *map, const float *scan_xy_host, size_t n, size_t stride_bytes,
                   const ndt_reloc_params *params, uint64_t *cand_index, double *cand_score, ndt_result *records,
                   int *n_cand, int *best, double *scores_host);
int ndt_relocalize_dev(ndt_ctx *ctx, const ndt_map *map, const float *scan_xy_dev, size_t n, size_t stride_bytes,
                       const ndt_reloc_params *params, uint64_t *cand_index, double *cand_score, ndt_result *records,
                       int *n_cand, int *best, double *scores_host);

/* Many independent (scan, map, lattice) jobs in one sweep launch and one pick launch: what a caller with many sessions to
 * relocalise -- a loop search over a session set -- would otherwise queue once per session.  Device forms only.
 *
 * A job names its map (an index into maps[]), its scan (points [offsets_dev[scan], offsets_dev[scan + 1]) of scans_xy_dev,
 * packed float2; offsets_dev has n_scans + 1 entries, total_points = the points in scans_xy_dev) and its lattice.  jobs and
 * vol_offsets_host are HOST arrays, read during the call; vol_offsets_host has n_jobs + 1 entries, in poses, the running sum of
 * the jobs' lattice sizes from 0.  Jobs may share a scan, a map or both.
 *
 * The sweep.  score_dev[vol_offsets[j] + p] and pairs_dev[vol_offsets[j] + p] of job j are the bits ndt_score_lattice_dev
 * writes for that map, scan and lattice pose: a function of those three alone, which does not depend on j, on the other jobs,
 * on n_jobs, on NDT_OPT_WORKGROUPS or on NDT_OPT_SCORE_STAGE.  An empty scan range is legal here (a pre-filter may leave
 * one): every pose of that job gets score 0 and pairs 0.  pairs_dev may be NULL.  Asynchronous on `stream` (NULL = the
 * context's), behind the maps' builds, one launch whatever n_jobs; the call is entered among the readers of every map of
 * maps[], as a match launch is.  The kernel instance and the float32 sin / cos are those of maps[0], so every map must have
 * the match parameters of maps[0] (ndt_align_batch_multi_dev's rule).
 *
 * The pick.  cand_index_dev[j * top_k + c], c < n_cand_dev[j], are exactly the list ndt_lattice_select_dev gives on job j's
 * volume with the same top_k and local_max, as indices inside the job's own lattice; entries from n_cand_dev[j] on are not
 * written.  One workgroup per job: top_k in 1 .. 16, lattices of at most 2^24 poses (a larger one stays with
 * ndt_lattice_select_dev).  One launch, no host wait.  A job's map and scan are not read.
 *
 * Refusals of both (NDT_E_ARG, synchronous, nothing queued, the text names the first offending job or map): a NULL context
 * ("null context"), a NULL array (pairs_dev of the sweep excepted), n_jobs < 1, n_scans < 1 or total_points > 2^31 - 1, a job's
 * map or scan index out of range, a lattice ndt_lattice_size refuses (for the pick: or of more than 2^24 poses), vol_offsets
 * that are not the running sum of the lattice sizes, more than 2^31 - 1 poses in all, a NULL map, a map never built or of
 * another device, a map with other match parameters than maps[0], an open ndt_map_rebuild_begin on the context, top_k
 * outside 1 .. 16. */
typedef struct ndt_score_job {
  int map;                            /* index into maps[] */
  int scan;                           /* index of the job's scan in offsets_dev */
  ndt_pose_lattice lattice;
} ndt_score_job;
int ndt_score_lattice_multi_dev(ndt_ctx *ctx, const ndt_map *const *maps, int n_maps, const float *scans_xy_dev,
                                const uint64_t *offsets_dev, int n_scans, size_t total_points, const ndt_score_job *jobs,
                                int n_jobs, double *score_dev, uint32_t *pairs_dev, const uint64_t *vol_offsets_host,
                                void *stream);
int ndt_lattice_select_multi_dev(ndt_ctx *ctx, const ndt_score_job *jobs, int n_jobs, const double *score_dev,
                                 const uint32_t *pairs_dev, const uint64_t *vol_offsets_host, int top_k, int local_max,
                                 uint64_t *cand_index_dev, int *n_cand_dev, void *stream);

/* ---- Per-point nearest distances and the ranged fitness ------------------------------------------------------------------
 * ndt_result.fitness is getFitnessScore() as src/PoseEstimator.cpp:43 calls it: PCL's getFitnessScore(max_range) with the
 * default max_range = DBL_MAX, the mean over EVERY scan point.  These calls give what that one number hides: the float32
 * squared distance of every point of a scan, at a given transform, to its nearest raw map point, in the caller's order, and
 * PCL's getFitnessScore(max_range) from them for any range.
 *
 * Inputs.  scans_xy / offsets / B / total_points / shared_scan as for ndt_align_batch_dev (packed float2; shared_scan: scan 0
 * with B transforms).  Transform b is four floats (c, s, tx, ty) at (const char *)tf + b * tf_stride_bytes: the T00, T10,
 * T03, T13 of an ndt_result, in that order; tf_stride_bytes is a multiple of 4 and at least 16, so sizeof(ndt_result) with
 * tf = &records[0].T00 takes the transforms straight from a launch's records, on the device, without a copy.  The point
 * transform is the map's ndt_params::transform_sse form, the one the launch's own fitness kernels apply.
 *
 * d2.  The value the launch's search returns: the minimum over all raw map points of F(ex * ex) + F(ey * ey), float32.  A point
 * without a distance -- a non-finite transformed point, or one every distance of which overflows -- gets +INFINITY.  Output
 * is in INPUT order, never the launch's internal voxel order: scans of their own, the point's index in scans_xy (d2 has
 * total_points floats); shared_scan, index b * n + i (d2 has B * n floats).  d2 may be NULL and stats may be NULL, not both.
 *
 * Stats.  max_d2 is compared with the SQUARED distance widened to double, `<=`, inclusive: what PCL's
 * getFitnessScore(max_range) does with its argument.  DBL_MAX reproduces the reference's call (src/PoseEstimator.cpp:43);
 * 0.0 is legal and counts the exact hits.
 *
 * Order of summation, stated once and kept.  Chunk k of a match is its points [64k, 64k + 64) in input order.  A chunk's two
 * sums (all / in range) are the wave butterfly over the 64 lanes' (double)d2, 0.0 where the predicate fails.  Lane l of ONE
 * wave adds the chunks l, l + 64, l + 128 ... in ascending order into one accumulator; the butterfly then adds the lanes.
 * Counts are integers.  fitness = n_in ? S_in / n_in : DBL_MAX, fitness_all likewise with n_dist.  (The launch's own scheme,
 * over input order instead of its ordered copy.)  A match's ndt_fit_stats and d2 are a function of (map, scan, transform,
 * max_d2) to the last bit: they do not depend on b, B, the other scans, shared_scan against the own-scan form, or
 * NDT_OPT_WORKGROUPS.  fitness_all equals ndt_result.fitness of a launch with the same transform within n * 2^-53 relative,
 * and bit for bit whenever the scan's sum is exact in fp64.
 * An empty scan: stats {DBL_MAX, DBL_MAX, 0, 0, 0, 0}, no d2 written.
 *
 * Ordering.  _dev is asynchronous on `stream` (NULL = the context's) and runs behind the map's build; it is entered among the
 * map's readers as the score sweep is, so a rebuild of the map queued behind it -- on whatever stream -- waits for it.  Its
 * scratch (one 32-byte {S_all, S_in, n_dist, n_in} per chunk) lies inside the context's scratch bracket.  ndt_fit_points_batch:
 * host pointers; one upload, the _dev call, one read-back each of d2 and stats; synchronous.
 *
 * Refusals (NDT_E_ARG, synchronous, nothing queued or written): a NULL context ("null context"); a NULL map, scans, offsets
 * or tf; both outputs NULL; B < 1; a map never built or of another device; tf_stride_bytes below 16 or not a multiple of 4;
 * max_d2 NaN or below 0; host form: offsets that decrease; an open ndt_map_rebuild_begin on the context. */
typedef struct ndt_fit_stats {
  double   fitness;      /* getFitnessScore(max_range) (PCL; src/PoseEstimator.cpp:43 passes none): mean of d2 over the
                            points with (double)d2 <= max_d2; DBL_MAX when there is none                       */
  double   fitness_all;  /* the same with no cut (src/PoseEstimator.cpp:43 as it stands): the quantity
                            ndt_result.fitness holds, summed in THIS call's order                                   */
  uint32_t n_in;         /* points with (double)d2 <= max_d2                                                        */
  uint32_t n_dist;       /* points that have a distance at all                                                      */
  uint32_t n_points;     /* points of the scan                                                                      */
  uint32_t reserved;     /* 0                                                                                       */
} ndt_fit_stats;         /* 32 bytes */
/* getFitnessScore(max_range) of PCL (src/PoseEstimator.cpp:43: without a range) and its per-point terms; device pointers. */
int ndt_fit_points_batch_dev(ndt_ctx *ctx, const ndt_map *map, const float *scans_xy_dev,
                             const uint64_t *offsets_dev, int B, size_t total_points, int shared_scan,
                             const float *tf_dev, size_t tf_stride_bytes, double max_d2,
                             float *d2_dev, ndt_fit_stats *stats_dev, void *stream);
/* The same from host memory (getFitnessScore(max_range) of PCL; src/PoseEstimator.cpp:43); synchronous. */
int ndt_fit_points_batch(ndt_ctx *ctx, const ndt_map *map, const float *scans_xy_host,
                         const uint64_t *offsets_host, int B, int shared_scan,
                         const float *tf_host, size_t tf_stride_bytes, double max_d2,
                         float *d2_host, ndt_fit_stats *stats_host);
/* One map per match.  Match b is searched in maps[map_of[b]]; with map_of == NULL, n_maps must equal B and match b uses
 * maps[b] (ndt_align_batch_multi_dev's rule).  Every other argument means what it means in ndt_fit_points_batch_dev.
 * Match b's d2 range and its ndt_fit_stats are, to the last bit, what ndt_fit_points_batch_dev writes for (that map, that
 * scan, that transform, max_d2), in the order of summation stated above: they do not depend on b, B, the other matches, the
 * other maps, n_maps, shared_scan against the own-scan form, or NDT_OPT_WORKGROUPS.  Resolutions, grids and every other
 * parameter but transform_sse may differ between the maps: the kernel reads a view per match, and a view carries its own grid.
 * A match without a map -- map_of[b] outside [0, n_maps) -- alone gets stats {DBL_MAX, DBL_MAX, 0, 0, n_points, 0} and
 * +INFINITY in every float of its d2 range; no kernel reads through the index.
 * One search launch and one close launch, whatever B and n_maps.  The table of the maps' views -- as they are at the call --
 * goes up once from pinned staging into a table of the call's own inside the context's scratch bracket (not the match
 * launch's: a match launch queued behind this call does not wait for it); the next ndt_fit_points_multi call waits for the
 * copy before it rewrites the staging.  The call is entered among the readers of every distinct map, so a rebuild of any of
 * them, on whatever stream, waits for it.
 * Refusals (NDT_E_ARG, synchronous, nothing queued or written; the text names the first offending map): maps == NULL or
 * n_maps < 1; a NULL map, a map never built or built on another device; the refusals of ndt_fit_points_batch_dev; map_of ==
 * NULL with n_maps != B; maps whose transform_sse differ (the kernel instance depends on it).
 * ndt_fit_points_multi: the same with host pointers (map_of_host too); one upload; synchronous. */
int ndt_fit_points_multi_dev(ndt_ctx *ctx, const ndt_map *const *maps, int n_maps, const int *map_of_dev,
                             const float *scans_xy_dev, const uint64_t *offsets_dev, int B, size_t total_points,
                             int shared_scan, const float *tf_dev, size_t tf_stride_bytes, double max_d2,
                             float *d2_dev, ndt_fit_stats *stats_dev, void *stream);
int ndt_fit_points_multi(ndt_ctx *ctx, const ndt_map *const *maps, int n_maps, const int *map_of_host,
                         const float *scans_xy_host, const uint64_t *offsets_host, int B, int shared_scan,
                         const float *tf_host, size_t tf_stride_bytes, double max_d2,
                         float *d2_host, ndt_fit_stats *stats_host);

/* ---- Occupancy grids, ray-cast from scans on the device -----------------------------------------------------------------
 * The reference writes poses and point clouds; it has no counterpart to these calls.  A grid holds, per cell, how many beams
 * ended in it (hit) and how many passed through it (pass).  Everything is integer addition, so a grid's counters and a
 * call's stats are a function of (geometry, beams) alone, to the last bit: they do not depend on the order of scans or beams,
 * on B, on how many calls the beams were spread over, or on NDT_OPT_WORKGROUPS.
 *
 * Geometry.  Cell (ix, iy) covers [x0 + ix res, x0 + (ix + 1) res) x [y0 + iy res, y0 + (iy + 1) res); cells are row-major,
 * index iy * nx + ix.  The cell of a point is ix = floor(((double)x - x0) / res): one rounded fp64 subtraction, one rounded
 * fp64 division, then floor; iy likewise.  ndt_occ_cell IS the definition (as ndt_lattice_pose is for lattices; host only, no
 * context): the device forms the same integers.  It saturates at +-2^62 and refuses a non-finite x or y.  Refusals of a
 * geometry: NDT_E_ARG for a res that is not positive and finite, a non-finite origin, nx or ny below 1; NDT_E_GRID for more
 * than 2^28 cells.
 *
 * Cells.  Two uint32_t counters {hit, pass}, interleaved, 8 bytes per cell; zero after create and after clear.  Counters wrap
 * modulo 2^32: nothing saturates.
 *
 * A beam runs from the origin o (two doubles) to an end point e (one float32 map-frame point, widened to double).  It is
 * SKIPPED -- nothing written, counted in n_skipped -- when a coordinate of o or e is not finite; when dx dx + dy dy >
 * max_range2, dx = (double)ex - ox (products and sum each rounded, no fma; max_range2 is the SQUARED range, as max_d2 is in
 * ndt_fit_points_batch; DBL_MAX = no limit); when a cell index of either endpoint lies outside [-2^30, 2^30]; when its length
 * in cells L exceeds 65536; when its scan's grid_of entry is out of range.
 *
 * The walk, in integers only.  (X0, Y0) = cell of o, (X1, Y1) = cell of e, dx = |X1 - X0|, dy = |Y1 - Y0|, sx, sy the signs,
 * L = max(dx, dy), m = min(dx, dy).  The beam visits k = 0 .. L - 1: the major coordinate is start + s k, the minor one
 * start + s floor((2 k m + L - 1) / (2 L)) in 64-bit integers; dx == dy counts as x-major.  Every visited cell inside the grid
 * gets pass += 1.  The end cell (X1, Y1) is not among the visits: it gets hit += 1 if it lies inside the grid.  L = 0 is a hit
 * only.  Cells outside the grid are not written; the beam is not otherwise clipped or dropped.  This closed form is the
 * all-octant integer Bresenham line from (X0, Y0) to (X1, Y1), end cell excluded: x-major, e = 2 dy - dx; dx times: visit;
 * if e > 0 { y += sy; e -= 2 dx; } e += 2 dy; x += sx (y-major: symmetric).
 *
 * Stats of one call (overwritten, not accumulated): n_beams seen, n_hit hits written, n_pass pass increments written,
 * n_skipped beams skipped.
 *
 * Render.  n = (uint64_t)hit + pass; the value is -1 when n < min_obs (min_obs >= 1), else (int8_t)((200 hit + n) / (2 n)):
 * 100 hit / n rounded half up, 0 .. 100, the convention of ROS's OccupancyGrid.
 *
 * ndt_occ_integrate_dev.  Scan b is the packed float2 map-frame points [offsets[b], offsets[b + 1]) -- what
 * ndt_scan_to_map_batch_dev writes -- and goes into occs[grid_of[b]] (grid_of_dev == NULL: all into occs[0]).  Origin b is two
 * doubles at (const char *)origins + b * origin_stride_bytes; the stride is a multiple of 8 and at least 16, so 24 takes the
 * (tx, ty, th) pose triples of ndt_scan_to_map_batch_dev, or a session set's last poses, where they lie.  An empty scan is
 * legal.  Asynchronous on `stream` (NULL = the context's), no host wait; one table upload (the grids, from pinned staging) and
 * two launches whatever B and n_occ are; the scratch (table, runs) lies inside the context's scratch bracket.
 * ndt_occ_integrate: the same from host memory, synchronous: one upload, the _dev call, the stats read back.
 *
 * Ordering.  A grid remembers the event behind its last writer (integrate, clear; create returns with the grid zeroed); any call that touches the grid on
 * another stream waits for that event first.  Calls of one context are otherwise serialised as all its calls are (the scratch
 * bracket).  Grids are destroyed before their context, like maps.
 *
 * Refusals (synchronous, nothing queued or written; the text names the first offender; NDT_E_ARG): a NULL context ("null
 * context", checked first); NULL arrays; n_occ < 1 or B < 1; a NULL grid, a grid of another context, the same grid twice; an
 * origin stride below 16 or not a multiple of 8; max_range2 NaN or negative; min_obs < 1; an open ndt_map_rebuild_begin on the
 * context; host form: offsets that decrease. */
typedef struct ndt_occ ndt_occ;
typedef struct ndt_occ_geometry { double x0, y0, res; int nx, ny; } ndt_occ_geometry;            /* 32 bytes */
typedef struct ndt_occ_stats { uint64_t n_beams, n_hit, n_pass, n_skipped; } ndt_occ_stats;    /* 32 bytes */
int ndt_occ_cell(const ndt_occ_geometry *geometry, double x, double y, int64_t *ix, int64_t *iy);
int ndt_occ_create(ndt_ctx *ctx, const ndt_occ_geometry *geometry, ndt_occ **out);
int ndt_occ_destroy(ndt_occ *occ);
/* Asynchronous memset on `stream` (NULL = the context's). */
int ndt_occ_clear(ndt_ctx *ctx, ndt_occ *occ, void *stream);
int ndt_occ_geometry_get(const ndt_occ *occ, ndt_occ_geometry *out);
/* The interleaved {hit, pass} device array, 2 * nx * ny uint32_t. */
int ndt_occ_view(const ndt_occ *occ, const uint32_t **cells_dev);
int ndt_occ_integrate_dev(ndt_ctx *ctx, ndt_occ *const *occs, int n_occ, const int *grid_of_dev, const float *xy_dev,
                          const uint64_t *offsets_dev, int B, size_t total_points, const double *origins_dev,
                          size_t origin_stride_bytes, double max_range2, ndt_occ_stats *stats_dev, void *stream);
int ndt_occ_integrate(ndt_ctx *ctx, ndt_occ *const *occs, int n_occ, const int *grid_of_host, const float *xy_host,
                      const uint64_t *offsets_host, int B, const double *origins_host, size_t origin_stride_bytes,
                      double max_range2, ndt_occ_stats *stats_host);
/* out: nx * ny int8_t, row-major.  _dev: asynchronous on `stream`; the host form is synchronous. */
int ndt_occ_render_dev(ndt_ctx *ctx, ndt_occ *occ, uint32_t min_obs, int8_t *out_dev, void *stream);
int ndt_occ_render(ndt_ctx *ctx, ndt_occ *occ, uint32_t min_obs, int8_t *out_host);
/* Synchronous read-back of the counters, nx * ny uint32_t each; either pointer may be NULL, not both. */
int ndt_occ_counts(ndt_ctx *ctx, ndt_occ *occ, uint32_t *hit_host, uint32_t *pass_host);
/* Session i is taken when (which == NULL or which[i] != 0) and it has started: its NEWEST scan -- the resampled scan in the
 * map frame as the last step that session took part in added it to the map -- goes into occs[i], from the origin at session
 * i's row of the set's resident last poses.  One table upload and the launches of ndt_occ_integrate_dev on the context's
 * stream; stats_host (may be NULL) is the call's one read-back, and with it the call waits.  Reads the set's state and
 * changes none of it.  Pass the step records' `stepped` flags as `which`: a session taken that did not step has its last
 * scan integrated AGAIN.  NDT_E_ARG: a NULL occs, a NULL or foreign entry of occs for a session that is taken, the same grid
 * for two of them, max_range2 NaN or negative.  NDT_E_HIP: a dead set. */
int ndt_sessions_occ_integrate(ndt_sessions *s, ndt_occ *const *occs, const unsigned char *which, double max_range2,
                               ndt_occ_stats *stats_host);

/* ---- Pose graphs: batched SE(2) optimisation and re-posing of stored clouds -------------------------------------------------
 * What the reference's commented-out loop closure was for: FrontEnd adds an odometry arc per scan and, on a detected loop, calls
 * backEnd->adjustPoses(), backEnd->remakeMaps() and smat.remakePoseArray(newPoses) (src/FrontEnd.cpp:21-44);
 * PointCloudMap::remakeMaps moves every map point from its old scan pose to its new one (src/PointCloudMap.cpp:136-170).  Its
 * back end (PoseGraph, SlamBackEnd) is absent from the reference tree; these calls are that step for S graphs at once.  Loop
 * DETECTION between independent maps is the caller's, with what exists (ndt_align_batch_multi_dev against old submaps' maps,
 * ndt_relocalize, ndt_fit_points_batch); inside a resident session it is ndt_sessions_find_loops, at the end of this section.
 * ndt_pg_optimize_batch and ndt_repose_points work on the caller's arrays; an ndt_sessions set's own
 * resident state takes an adjusted trajectory through ndt_sessions_correct (at the end of this section), and gives the
 * trajectory a graph is built from through ndt_sessions_trajectory.
 *
 * Conventions are those of the f2 rows: poses are (tx, ty, th[deg]) double triples, covariances and information matrices are
 * in (m, m, rad), output headings are wrapped into [-180, 180) as MyUtil::add_angle does (src/MyUtil.cpp:4-11).
 *
 * Model, in radians internally.  For an arc (i -> j, z, Omega): r_xy = R(th_i)^T (t_j - t_i) - z_xy,
 * r_th = wrap(th_j - th_i - z_th) into [-pi, pi), F = sum r^T Omega r.  Node 0 of every graph is held fixed: its three doubles
 * come back bit-identical.
 *
 * Method.  Gauss-Newton with analytic Jacobians.  The normal equations H d = -b, node 0's rows and columns removed, are solved
 * by conjugate gradients preconditioned with the CHAIN matrix T (J^T Omega J in full for every arc with |from - to| = 1, the two
 * diagonal blocks alone for every other arc: block-tridiagonal, factored once per Gauss-Newton step by a block-Thomas sweep) to
 * a relative preconditioned residual sqrt(r^T z / r0^T z0) <= cg_rtol, in at most cg_max_iter iterations (0: 6 N).  A step d is
 * taken only if F does not rise; otherwise it is halved, up to max_halvings times.  converged = 1 when max|d| of an accepted
 * step is below eps_step (metres and radians alike) -- and when the halving runs out at a step that is already below eps_step:
 * halving on could only accept a shorter one, so the poses stay (next to the minimiser the change of F along a step of 1e-9
 * is below the rounding of F itself, and the comparison decides nothing).  converged = 0 at max_iter, at any other step that
 * cannot be accepted, at a T that is not positive definite to working precision (a pivot of its factor below 1e-13 of its diagonal
 * entry: a node that nothing ties to node 0) and at a CG breakdown (p^T H p <= 0 or not finite); the poses are then the last accepted ones.
 * cost_final <= cost_initial always.  iterations counts accepted steps, cg_iterations is the total over the run.  A graph that
 * took no step keeps its poses' bytes.
 *
 * Per-graph faults are found on the device and do not disturb other graphs: an arc index outside the graph, from == to, a
 * non-finite number in the graph's poses or arcs, an info that is not positive definite (Sylvester's criterion).  Each gives
 * status = NDT_E_ARG, the other fields 0, that graph's poses untouched.  A graph without arcs: NDT_OK, converged = 1,
 * iterations = 0, untouched.  A graph in which some node has no path to node 0 is the caller's error: it ends through the
 * rules above with converged = 0 and finite poses.
 *
 * One 256-thread workgroup per graph, one launch for all iterations of all graphs (a batch of one graph uses one CU: the
 * product is the batch).  A graph's poses and record are a function of its own input alone, to the last bit: not of the
 * batch, its order, or the schedule.  Graph g's nodes are the pose triples [node_offsets[g], node_offsets[g + 1]), its arcs
 * edges[edge_offsets[g] .. edge_offsets[g + 1]); both offset arrays (n_graphs + 1 entries) are HOST arrays in either form: the
 * scratch is sized from them.  _dev is asynchronous on `stream` (NULL = the context's): one table upload, one launch, scratch
 * inside the context's scratch bracket.  ndt_pg_optimize_batch: host pointers; uploads, the _dev call, poses and records read
 * back; synchronous.
 *
 * Refusals (NDT_E_ARG, synchronous, nothing queued or written): a NULL context ("null context"); NULL arrays; n_graphs < 1;
 * offsets that decrease; a graph of 2^28 nodes or arcs or more; max_iter outside [1, 10000], eps_step negative or not finite,
 * cg_max_iter outside [0, 2^30], cg_rtol outside (0, 1), max_halvings outside [0, 60]; an open ndt_map_rebuild_begin on the
 * context. */
typedef struct ndt_pg_edge {      /* one arc; DEVICE or HOST memory by entry point; 80 bytes */
  int32_t from, to;               /* node indices inside the arc's own graph */
  double  rel[3];                 /* pose of `to` in `from`'s frame: Pose2D::calMotion(to, from) (src/Pose2D.cpp:5-14); th in deg */
  double  info[6];                /* xx xy xt yy yt tt of the 3x3 information matrix, (m, m, rad) */
} ndt_pg_edge;
typedef struct ndt_pg_params { int max_iter; double eps_step; int cg_max_iter; double cg_rtol; int max_halvings; } ndt_pg_params;
typedef struct ndt_pg_result {    /* one per graph; 32 bytes */
  double cost_initial, cost_final; int iterations, cg_iterations, converged, status;
} ndt_pg_result;
/* 20, 1e-9, 0 (= 6 N), 1e-10, 8: for the pose adjustment called at src/FrontEnd.cpp:37. */
int ndt_pg_default_params(ndt_pg_params *p);
/* Host helper, no context: edge->rel = Pose2D::calMotion(to_pose, from_pose) (src/Pose2D.cpp:5-14, the odometry arc of
 * src/FrontEnd.cpp:61-63); from, to and info are left as they are.  NDT_E_ARG: a NULL pointer, a non-finite pose. */
int ndt_pg_edge_between(const double from_pose[3], const double to_pose[3], ndt_pg_edge *edge);
/* Host helper, no context: the information matrix of a world-frame covariance (row-major 3 x 3, (m, m, rad)) seen from the frame
 * at heading th_deg: C' = R3^T C R3 with R3 = diag(R(th), 1) -- CovarianceCalculator::rotateCovariance(lastPose, fusedCov, cov,
 * true) of src/FrontEnd.cpp:69 --, then info = C'^-1 as xx xy xt yy yt tt.  The off-diagonal pairs of C are averaged.
 * NDT_E_ARG: a NULL pointer, a non-finite number, a pair that differs by more than 1e-9 sqrt(C_ii C_jj), a matrix that is not
 * positive definite by Sylvester's criterion to working precision: a pivot xx, m2 / xx, det / m2 of C' that is not above 1e-12
 * of the largest diagonal entry of its unit (m^2, rad^2).  A first scan's zero covariance is one, and so is the first matched
 * scan's, which has 1e-35 m^2 along the motion: give such an arc an information matrix of your own. */
int ndt_pg_info_from_cov(const double cov_world[9], double th_deg, double info[6]);
/* SlamBackEnd::adjustPoses (called at src/FrontEnd.cpp:37) for n_graphs graphs at once; device poses, arcs and records. */
int ndt_pg_optimize_batch_dev(ndt_ctx *ctx, double *poses_dev, const uint64_t *node_offsets_host, const ndt_pg_edge *edges_dev,
                              const uint64_t *edge_offsets_host, int n_graphs, const ndt_pg_params *params,
                              ndt_pg_result *out_dev, void *stream);
/* The same from host memory (src/FrontEnd.cpp:37); synchronous. */
int ndt_pg_optimize_batch(ndt_ctx *ctx, double *poses_host, const uint64_t *node_offsets_host, const ndt_pg_edge *edges_host,
                          const uint64_t *edge_offsets_host, int n_graphs, const ndt_pg_params *params,
                          ndt_pg_result *out_host);
/* ---- Pose graphs that reject false loop arcs: graduated non-convexity on Geman-McClure arcs ----
 * ndt_pg_optimize_batch takes every arc at face value; a loop search verifies that two clouds fit, not that the place is the
 * same, and one false arc bends a whole trajectory.  These calls are that optimiser with a robust cost on the arcs the caller
 * marks, by graduated non-convexity (Yang, Antonante, Tzoumas, Carlone: "Graduated Non-Convexity for Robust Spatial Perception",
 * RA-L 2020, the Geman-McClure form): a plain redescending kernel started at a drifted chain would reject the true loops too,
 * whose first chi-square is large precisely because of the drift they are meant to remove.
 *
 * Model.  Arcs, poses, the residual r_e, Omega_e and node 0 held fixed are exactly those of ndt_pg_optimize_batch.  Every arc
 * also carries phi_e >= 0 (phi[e], indexed like edges; phi == NULL: all 0).  phi_e == 0: a plain arc, never down-weighted
 * (odometry arcs).  phi_e > 0: a robust arc.  With c_e = r_e^T Omega_e r_e and a level mu >= 1: a plain arc has rho = c_e,
 * w_e = 1; a robust arc has sigma = mu phi_e, rho = sigma c_e / (sigma + c_e), w_e = (sigma / (sigma + c_e))^2;
 * F_mu = sum_e rho.  At mu = 1 an arc with c_e = phi_e has weight 1/4: phi is the chi-square beyond which an arc counts as
 * rejected.
 *
 * Method.  One TRIP at the current mu: linearise at x, every arc's w_e at x, (sum w_e J^T Omega J) d = -(sum w_e J^T Omega r)
 * by the same preconditioned conjugate gradients (the chain matrix T from the weighted blocks), then the same step rule on
 * F_mu: s = 1, 1/2, ..., the first trial whose F_mu is finite and does not rise, at most max_halvings halvings.  max_iter bounds
 * the TRIPS, accepted or not, over all levels; iterations counts accepted steps.  Levels: mu starts at mu0; mu0 = 0 in the
 * parameters means max(1, 2 max_e c_e(x0) / phi_e) over the graph's robust arcs, clipped to 1e12; a graph without a robust arc
 * starts at 1 whatever mu0 says.  A level with mu > 1 ends when an accepted step has max|s d| < eps_level, when the halving runs
 * out, or when the level has taken level_iter accepted steps; then mu = max(1, mu / factor) and F is evaluated again at the
 * same poses.  At mu == 1 the ending rules of ndt_pg_optimize_batch hold unchanged (eps_step, the run-out below eps_step, the
 * CG breakdown, the pivot floor, `converged`); converged can only become 1 at mu == 1.  A T that is not positive definite and a
 * CG breakdown end the run at any level, with converged = 0 and the last accepted poses: a component whose only tie to node 0
 * is a robust arc ends so once that arc's weight has fallen below the pivot floor.  cost_initial and cost_final are F_1 at the
 * first and the last poses; cost_final <= cost_initial is promised only for runs that spend every trip at mu == 1 (a level
 * above 1 lowers F_mu, not F_1).  factor = 1.4 is the paper's; level_iter = 3 and eps_level = 1e-3 come from a numpy prototype
 * on drifted figure-eights of 24 and 65 nodes (tests/pg_robust_helpers.py), not from a device measurement.
 *
 * Outputs per arc (optional arrays indexed like edges): weight_out[e] = w_e at mu = 1 at the final poses, 1.0 for a plain
 * arc; chi2_out[e] = c_e there.  An arc counts as REJECTED when it is robust and its final c_e > phi_e (weight below 1/4);
 * n_rejected counts them, n_robust the arcs with phi_e > 0.  mu0 in the record is the value the graph started at, levels the
 * number of levels visited (1 for a graph that starts at mu == 1).  For a graph that ends with status != NDT_OK the arc
 * outputs and the record's other fields are 0.  A graph without arcs: NDT_OK, converged = 1, mu0 = 1, levels = 1.
 *
 * Per-graph faults are those of ndt_pg_optimize_batch, found on the device in the same way, and a phi_e that is negative or
 * not finite: status = NDT_E_ARG for that graph alone.
 *
 * A graph with no robust arc (phi == NULL, or all zeros) comes back with poses and the `pg` part of its record byte-identical
 * to what ndt_pg_optimize_batch gives for the same input and ndt_pg_params; its weights are exactly 1.0.  Resources are those of
 * ndt_pg_optimize_batch: the same table and scratch, one launch; a graph's bytes are a function of its own input alone.
 *
 * Refusals (NDT_E_ARG, synchronous, nothing queued or written): those of ndt_pg_optimize_batch (on params->pg); mu0 that is
 * neither 0 nor in [1, 1e12]; factor outside [1.05, 1e6]; eps_level negative or not finite; level_iter outside [1, 10000]. */
typedef struct ndt_pg_robust_params { ndt_pg_params pg; double mu0, factor, eps_level; int level_iter; } ndt_pg_robust_params;
typedef struct ndt_pg_robust_result {   /* one per graph; 56 bytes */
  ndt_pg_result pg; double mu0; int levels, n_robust, n_rejected, pad;
} ndt_pg_robust_result;
/* pg as ndt_pg_default_params but max_iter = 200 (the trips of every level); mu0 = 0 (automatic), factor = 1.4,
 * eps_level = 1e-3, level_iter = 3. */
int ndt_pg_robust_default_params(ndt_pg_robust_params *p);
/* Device poses, arcs, phi (may be NULL), records and arc outputs (each may be NULL); HOST offset arrays; asynchronous on
 * `stream` (NULL = the context's). */
int ndt_pg_optimize_robust_batch_dev(ndt_ctx *ctx, double *poses_dev, const uint64_t *node_offsets_host, const ndt_pg_edge *edges_dev,
                                     const uint64_t *edge_offsets_host, int n_graphs, const double *phi_dev,
                                     const ndt_pg_robust_params *params, ndt_pg_robust_result *out_dev, double *weight_out_dev,
                                     double *chi2_out_dev, void *stream);
/* The same from host memory; synchronous. */
int ndt_pg_optimize_robust_batch(ndt_ctx *ctx, double *poses_host, const uint64_t *node_offsets_host, const ndt_pg_edge *edges_host,
                                 const uint64_t *edge_offsets_host, int n_graphs, const double *phi_host,
                                 const ndt_pg_robust_params *params, ndt_pg_robust_result *out_host, double *weight_out_host,
                                 double *chi2_out_host);
/* ---- Pose covariances from the pose graph: blocks of H^-1, and the consistency of a candidate loop arc ----
 * The optimisers above return poses and chi-squares; these calls answer how well pose b is known relative to pose a, and
 * whether a candidate loop arc agrees with the odometry in between -- a Mahalanobis distance on that answer, which needs no
 * true loop beside a false one and so belongs in front of ndt_pg_optimize_robust_batch.
 *
 * Model.  H = sum_e w_e J_e^T Omega_e J_e at the poses GIVEN (no step is taken, the poses are only read), node 0's rows and
 * columns removed, exactly as ndt_pg_optimize_robust_batch forms it; Sigma = H^-1 is the covariance relative to node 0, in
 * (m, m, rad).  weight (one double per arc, indexed like edges) may be NULL: every w_e = 1, and the result is byte-identical
 * to passing an array of 1.0.  It is meant to take weight_out of the robust call, so that a rejected arc does not count;
 * w_e >= 0 and finite is required, and an arc with w_e == 0 contributes nothing.
 *
 * Query (graph, a, b): Saa and Sbb are the diagonal blocks of the nodes a and b, each off-diagonal pair replaced by
 * 0.5 (upper + lower); Sab[3 r + c] = Sigma[3 a + r, 3 b + c], taken from the solves of node b's unit columns.  a == b is
 * legal: three columns are solved and Sab = Sbb = Saa.  A block that involves node 0 is exactly 0.0.
 *
 * Method.  For each unit column, H x = e by the conjugate gradients and the chain factor of the optimisers, to
 * sqrt(r^T z / r0^T z0) <= cg_rtol in at most cg_max_iter iterations (0: 6 N).  Of ndt_pg_params only cg_max_iter and cg_rtol
 * are used (the others are held to ndt_pg_optimize_batch's ranges and otherwise ignored).  The three or six columns of a query
 * share every walk over the arcs and every sweep of the factor, each with its own step lengths and its own stop.
 * cg_iterations is the largest count over the query's columns, converged = 1 when every column met the rule.  converged = 0
 * gives all three blocks as 0 -- nobody gets a half-solved covariance --: the iteration cap, a pivot of T below 1e-13 of its
 * diagonal entry (a node that nothing ties to node 0, also through arcs of weight 0), a CG breakdown.  On a graph that is a
 * pure chain T = H and a column takes one or two iterations.
 *
 * status = NDT_E_ARG with everything else 0, for that query alone: a per-graph fault as ndt_pg_optimize_batch defines it, a
 * weight of the graph that is negative or not finite, graph, a or b out of range, a graph without arcs when a or b is not 0.
 *
 * A column's solution is a function of (graph, weights, node, column) alone, to the last bit: not of the batch, the order of
 * the queries, the other node of the query or the place of the column in it.  Saa of (a, b), Saa of (a, a) and Sbb of (c, a)
 * are the same bytes.
 *
 * One 256-thread workgroup per query at a time, at most 1024 workgroups, one launch; the scratch is one slot per workgroup
 * for the largest queried graph, inside the context's scratch bracket: it does not grow with n_queries beyond that.  queries
 * and both offset arrays are HOST arrays in either form.  _dev is asynchronous on `stream` (NULL = the context's).
 *
 * Refusals (NDT_E_ARG, synchronous, nothing queued or written): those of ndt_pg_optimize_batch; NULL queries or out;
 * n_queries < 1. */
typedef struct ndt_pg_query    { int32_t graph, a, b, pad; } ndt_pg_query;
typedef struct ndt_pg_marginal {  /* one per query; 232 bytes */
  double Saa[9], Sab[9], Sbb[9];  /* row-major 3x3, (m, m, rad) */
  int cg_iterations, converged, status, pad;
} ndt_pg_marginal;
/* Device poses, arcs, weights (may be NULL) and records; HOST offsets and queries. */
int ndt_pg_marginals_batch_dev(ndt_ctx *ctx, const double *poses_dev, const uint64_t *node_offsets_host, const ndt_pg_edge *edges_dev,
                               const uint64_t *edge_offsets_host, int n_graphs, const double *weight_dev,
                               const ndt_pg_query *queries_host, int n_queries, const ndt_pg_params *params,
                               ndt_pg_marginal *out_dev, void *stream);
/* The same from host memory; synchronous. */
int ndt_pg_marginals_batch(ndt_ctx *ctx, const double *poses_host, const uint64_t *node_offsets_host, const ndt_pg_edge *edges_host,
                           const uint64_t *edge_offsets_host, int n_graphs, const double *weight_host,
                           const ndt_pg_query *queries_host, int n_queries, const ndt_pg_params *params,
                           ndt_pg_marginal *out_host);
/* Host helper, no context: the first-order covariance of "b in a's frame" (the arc residual's own variable), row-major 3 x 3 in
 * (m, m, rad): C = Ja Saa Ja^T + Ja Sab Jb^T + Jb Sab^T Ja^T + Jb Sbb Jb^T with Ja = d r / d x_a and Jb = d r / d x_b of the
 * residual above at (pose_a, pose_b), poses as (tx, ty, th[deg]).  NDT_E_ARG: a NULL pointer, a non-finite number, a C that is
 * not positive definite (Sylvester's criterion; the zero blocks of a query that did not converge end here). */
int ndt_pg_relative_cov(const double pose_a[3], const double pose_b[3], const ndt_pg_marginal *m, double cov[9]);
/* Host helper, no context: d2 = r^T (rel_cov + Omega^-1)^-1 r for an arc from pose_a to pose_b, r its residual at the two poses
 * and Omega its information (edge->from and edge->to are not read); rel_cov's off-diagonal pairs are averaged.  Under the model
 * d2 of a true arc follows chi-square with 3 degrees of freedom.  NDT_E_ARG: a NULL pointer, a non-finite number, an Omega or
 * a rel_cov + Omega^-1 that is not positive definite. */
int ndt_pg_edge_chi2(const double pose_a[3], const double pose_b[3], const ndt_pg_edge *edge, const double rel_cov[9], double *d2);
/* PointCloudMap::remakeMaps' point correction (src/PointCloudMap.cpp:147-154) for clouds stored in ranges.  Segment k covers the
 * points [seg_offsets[k], seg_offsets[k + 1]) of xy (two float32 at each stride) and has the pose triples old_poses[k] and
 * new_poses[k]: q = oldPose.relativePoint(p), p' = newPose.globalPoint(q) (src/Pose2D.cpp:46-59) with Rmat as Pose2D::calRmat
 * builds it, in fp64 without contraction as ndt_scan_to_map_batch_dev does it, rounded once to float32.  A segment whose old and
 * new pose are bit-equal is copied through unchanged: submaps that a correction does not reach keep their bytes.  out may be
 * xy itself at the same stride.  Segment ranges are those ndt_sessions_global_map returns in sub_offsets, or per-scan ranges of
 * a store.  Non-finite poses or points give non-finite points, nothing else.  _dev: asynchronous on `stream` (NULL = the
 * context's), one launch, no scratch.  Refusals (NDT_E_ARG): a NULL context or array, n_segs < 1, a stride below 8 or not a
 * multiple of 4, out == xy at another stride; host form: offsets that decrease. */
int ndt_repose_points_dev(ndt_ctx *ctx, const float *xy_dev, size_t stride_bytes, const uint64_t *seg_offsets_dev, int n_segs,
                          const double *old_poses_dev, const double *new_poses_dev, float *out_xy_dev, size_t out_stride_bytes,
                          void *stream);
/* The same from host memory (src/PointCloudMap.cpp:147-154); synchronous.  Only the points of the segments are read and written. */
int ndt_repose_points(ndt_ctx *ctx, const float *xy_host, size_t stride_bytes, const uint64_t *seg_offsets_host, int n_segs,
                      const double *old_poses_host, const double *new_poses_host, float *out_xy_host, size_t out_stride_bytes);

/* Session i's trajectory as of now (host only, no device work): poses_host[3 * k] = (tx, ty, th[deg]) of its k-th stepped scan
 * (the step records' `pose`; after ndt_sessions_correct, the corrected ones).  sub_first[m] = cntS of submap m
 * (src/PointCloudMap.cpp:72-90; n_submaps = closed + 1 entries, the last one the current submap's), sub_anchor[m] = the scan
 * whose pose pair moves submap m's closed cloud in ndt_sessions_correct: cntS + (cntE - cntS) / 2, with the newest scan as the
 * current submap's cntE, and cntS for a submap that closed without a scan of its own (cntE < cntS).  *store_first = index of
 * the first scan held in the current submap's scan store: the store's scans are the tail [store_first, n_scans) of the stepped
 * scans, the two carried-over scans of a split first (src/PointCloudMap.cpp:80-83).  A call with poses_host == NULL returns
 * the sizes (*n_scans, *n_submaps, *store_first).  Any other output may be NULL.  capacity in poses.  NDT_E_ARG: a NULL set,
 * an index outside it, a capacity below n_scans. */
int ndt_sessions_trajectory(const ndt_sessions *s, int i, double *poses_host, size_t capacity, size_t *n_scans,
                            int *sub_first, int *sub_anchor, int *n_submaps, size_t *store_first);
/* PointCloudMap::remakeMaps + ScanMatcher::remakePoseArray (src/PointCloudMap.cpp:136-170, src/FrontEnd.cpp:37-41) for
 * n_corr sessions of a resident set in one set of launches.  new_poses_host[c]: n_poses[c] x 3 doubles, the whole adjusted
 * trajectory of session which[c]; n_poses[c] must equal that session's n_scans (a stale trajectory is refused).  For each
 * of them, with old pose = the stored trajectory and new pose = the argument:
 *   - every scan of the current submap's store (the carried-over copies included) is moved in place by its own pair, every
 *     closed submap's cloud by the pair of its anchor scan (sub_anchor above: a closed cloud is a set of voxel centroids
 *     without a scan id, so it takes one rigid motion) -- ndt_repose_points' arithmetic to the bit, a bit-equal pair leaves
 *     the bytes alone;
 *   - the current submap's cloud is computed again from the moved scans, every triple of it, as ndt_local_map_batch_dev
 *     computes it; the local map is the previous closed cloud (moved) followed by the pre-filter of the new cloud, and the
 *     NDT map is rebuilt in place from it.  The state is then what the composed chain of ndt_sessions_step's comment holds
 *     after the same correction, and every later step equals that chain's, byte for byte;
 *   - the session's last pose becomes new_poses[last] and the stored trajectory the new one; the last covariance, the last
 *     odometry pose and the travelled distance (atd: the reference does not recompute it) are untouched.
 * status_host[c]: NDT_OK; NDT_E_GRID / NDT_E_ARG as ndt_map_build_batch_dev gives the new local map on its own (the map is
 * left as it was, as in a step); NDT_E_ARG when a recomputed triple spans more than 2^30 voxels: both views of that session
 * are empty, its map is kept, its points and trajectory are moved all the same, and no equality with the chain is claimed
 * for it afterwards.  Either way the call returns NDT_OK and no other session is concerned.  Sessions not named keep every
 * byte.  The views of ndt_sessions_local_map / _submap_cloud taken before the call are invalid after it, for every session.
 * The number of kernels, copies and host waits (two) depends neither on n_corr nor on a submap's length;
 * ndt_sessions_get_stats then describes this call (sessions_stepped = sessions corrected, triples_run = triples recomputed).
 * Refusals (NDT_E_ARG, synchronous, nothing changed, the text names the first offending entry): a NULL set ("null session
 * set"), NULL arrays, n_corr < 1, a session outside the set or one that has not started, the same session twice, a NULL
 * trajectory, n_poses[c] different from the session's scan count, a non-finite pose (the text names session and scan), an
 * open ndt_map_rebuild_begin.  NDT_E_HIP: a dead set; a HIP failure inside the call leaves the set dead, as in a step. */
int ndt_sessions_correct(ndt_sessions *s, const int *which, int n_corr, const double *const *new_poses_host,
                         const size_t *n_poses, int *status_host);

/* ---- Loop search on a session set: lpd.detectLoop of the chain the reference left commented out (src/FrontEnd.cpp:32-43) ----
 * For every session looked at: has its newest scan come back to a submap it closed long ago?  One call gates candidates on the
 * host, then sweeps a pose lattice around each candidate's last pose over the old submap's own NDT map, picks the best poses,
 * refines them with the match and returns a ready ndt_pg_edge per session -- with launches, copies and host waits that do not
 * grow with the number of sessions.  The edge goes into the graph made of ndt_sessions_trajectory, ndt_pg_optimize_batch
 * adjusts it and ndt_sessions_correct takes the result back.
 * Several candidate submaps per session and a ranged-fitness verification of a partial overlap: ndt_sessions_find_loops_multi
 * below; loops between the sessions of a set: ndt_sessions_find_cross_loops behind it.  Out of scope: keeping the loop maps
 * valid across calls; calling the optimiser or the correction for the caller.
 *
 * Gating (host only, no device work; ndt_sessions_loop_candidates gives exactly what ndt_sessions_find_loops will search).
 * This is the definition, on what ndt_sessions_trajectory returns (n poses, sub_first, sub_anchor) and the closed clouds'
 * sizes (ndt_sessions_global_map's sub_offsets):
 *   - session i is looked at when `which` is NULL or which[i] != 0, it has started and has n_closed >= 2 closed submaps;
 *   - submap m owns the scans [sub_first[m], sub_first[m + 1] - 1];
 *   - submap m is eligible when m <= n_closed - 2 (the newest closed submap is already in the local map every step matches
 *     against), its scan range is not empty, its closed cloud has points, path(m) >= min_path and dist(m) <= radius, where
 *     path(m) = the sum over k from the submap's last scan to n - 2, in ascending k, of sqrt(dx * dx + dy * dy) between poses
 *     k and k + 1, and dist(m) = the smallest sqrt(dx * dx + dy * dy) from the last pose (n - 1) to a pose of its scan range;
 *     fp64, every product, sum and root rounded once;
 *   - the session's candidate is the eligible submap of smallest dist, ties to the lower m; a session without one has no
 *     candidate;
 *   - anchor_scan = sub_anchor[m], the scan whose pose pair moves that cloud in ndt_sessions_correct: the edge made here and a
 *     correction applied there speak of the same rigid body; newest_scan = n - 1; nearest_scan = the scan of dist(m) (the
 *     lowest one);
 *   - the lattice is centred on the last pose (tx, ty, th[deg]): x0 = tx - (double)half_x * step_xy (one rounded multiply, one
 *     rounded subtraction), y0 likewise, yaw0 = DEG2RAD(th) - (double)half_yaw * step_yaw with DEG2RAD(x) = x * M_PI / 180
 *     (include/ndt_slam/MyUtil.h:22, as src/PoseEstimator.cpp:22 applies it to the guess); steps (step_xy, step_xy, step_yaw),
 *     2 half + 1 poses per axis.
 * Candidates come out in ascending session order; *n_out of them; `out` needs room for n_sessions.
 * Refusals (NDT_E_ARG, nothing queued): a NULL set ("null session set"), NULL params or outputs, a non-finite or negative
 * min_path, radius or step, a negative half extent, a lattice above 2^24 poses, top_k outside 1 .. NDT_LOOP_MAX_CAND, a NaN
 * max_cost.
 *
 * The search, for the J candidates (all on the context's stream; synchronous).  (1) One table upload.  (2) Each candidate's
 * newest stored scan (the one ndt_sessions_occ_integrate takes) goes into the robot frame by ndt_repose_points' arithmetic,
 * old pose = the session's last pose, new pose = (0, 0, 0), into scratch.  (3) ndt_prefilter_batch_dev's kernels with the set's
 * leaf: the source a step's match would see.  (4) The J closed clouds are built into NDT maps with the set's match parameters
 * by the batched build; the set owns these maps (one per session), reuses them from call to call and destroys them; host wait
 * 1, the bounding boxes.  (5) ndt_score_lattice_multi_dev's launch, (6) ndt_lattice_select_multi_dev's, (7) one kernel that
 * forms the J x top_k initial guesses and lays each filtered scan out top_k times, (8) ndt_align_batch_multi_dev's launch
 * with scans of their own, (9) records, candidate indices, scores and counts read back: host wait 2.
 * The host then takes, per candidate, the record of lowest cost = converged ? fitness : 1e7 (src/PoseEstimator.cpp:43-46), ties
 * to the lower index, as ndt_relocalize does.
 *
 * ndt_loop.  status: NDT_OK, or the code the build gave that candidate's map (NDT_E_GRID, NDT_E_ARG): that candidate alone
 * then has found = 0 and n_cand = 0.  n_cand records were made (cand_index inside the candidate's lattice, cand_score the
 * sweep's, cand_cost the rule above; entries from n_cand on are 0); best = the chosen one, -1 for n_cand == 0.  pose = the best
 * record's (pose[0], pose[1], RAD2DEG(pose[2])), RAD2DEG(x) = x * 180 / M_PI (src/PoseEstimator.cpp:36).  edge: from =
 * anchor_scan, to = newest_scan, info = params->info, rel by ndt_pg_edge_between(trajectory[anchor_scan], pose); with best == -1
 * pose and rel are 0.  found = best >= 0 and its cost <= max_cost.  records_host (or NULL): record c of candidate j at
 * [j * NDT_LOOP_MAX_CAND + c], byte-identical to ndt_align_batch_dev's for that filtered scan alone from that lattice pose;
 * the slots from n_cand on, and every slot behind the *n_out candidates, are not written.
 * A candidate's ndt_loop and records do not depend on which other sessions are named.
 * A candidate whose newest stored scan has no points (ndt_sessions_step stores a step whose scan is empty as a scan of length
 * 0) or filters to none, and one whose scan meets no voxel of its map at any lattice pose, is searched like every other and
 * picks nothing: status NDT_OK, found = 0, n_cand = 0, best = -1, pose and rel 0.  When EVERY candidate's newest scan is
 * empty the call returns before it builds a map or queues anything: every ndt_loop is that record, with status NDT_OK.
 *
 * The call changes nothing of the set's SLAM state: views taken before it stay valid, and the next step is the step of a set
 * that never searched.  ndt_sessions_get_stats afterwards describes this call: host_waits 2 (0 with no candidate: the call
 * then returns NDT_OK with *n_out = 0 and has queued nothing; 0 too when every candidate's newest scan is empty, 1 when no
 * map could be built: nobody is found), sessions_stepped = J, the bytes of its own tables and read-backs.
 * Refusals: those of the gating, an open ndt_map_rebuild_begin on the context, more than 2^31 - 1 lattice poses over all
 * candidates.  NDT_E_HIP on a dead set; a HIP failure inside the call kills the set as in a step. */
#define NDT_LOOP_MAX_CAND 8
typedef struct ndt_loop_params {
  double min_path;                    /* m of trajectory between the candidate submap's last scan and the newest scan */
  double radius;                      /* m: some scan pose of the candidate submap lies this close to the last pose */
  double step_xy, step_yaw;           /* m, rad */
  int    half_x, half_y, half_yaw;    /* lattice of (2 half + 1) per axis, centred on the last pose */
  int    top_k;                       /* 1 .. NDT_LOOP_MAX_CAND */
  int    local_max;
  double max_cost;                    /* found = best cost <= max_cost */
  double info[6];                     /* copied into every edge: xx xy xt yy yt tt, (m, m, rad) */
} ndt_loop_params;
/* min_path 10, radius 2, steps 0.1 m and 1 deg (in rad), halves 10, 10, 6, top_k 4, local_max 1, max_cost 0.02,
 * info diag(1e4, 1e4, 1e4). */
int ndt_loop_default_params(ndt_loop_params *p);
typedef struct ndt_loop_candidate {   /* HOST; what the search of one session will run on */
  int session, submap, anchor_scan, newest_scan, nearest_scan;
  double dist, path;
  ndt_pose_lattice lattice;
} ndt_loop_candidate;
/* The gating of ONE trajectory, host only, without a set or a context: the arrays are those ndt_sessions_trajectory (poses,
 * sub_first, sub_anchor, n_submaps) and ndt_sessions_global_map (sub_offsets, n_submaps + 1 entries) give for a session that has
 * started.  *has = 1 and *out written (session 0), or *has = 0.  ndt_sessions_loop_candidates is this rule on every session
 * looked at.  Refusals: those of the parameters, a NULL pointer, n_scans or n_submaps below 1, arrays that are not a set's
 * layout (sub_first[0] != 0 or decreasing, an index outside the trajectory, decreasing sub_offsets), a pose that is not finite. */
int ndt_loop_gate(const double *poses, size_t n_scans, const int *sub_first, const int *sub_anchor, const uint64_t *sub_offsets,
                  int n_submaps, const ndt_loop_params *p, ndt_loop_candidate *out, int *has);
int ndt_sessions_loop_candidates(const ndt_sessions *s, const unsigned char *which, const ndt_loop_params *p,
                                 ndt_loop_candidate *out, int *n_out);
typedef struct ndt_loop {             /* HOST; one per candidate, in candidate order */
  ndt_loop_candidate cand;
  int status, found, n_cand, best;
  uint64_t cand_index[NDT_LOOP_MAX_CAND];
  double cand_score[NDT_LOOP_MAX_CAND], cand_cost[NDT_LOOP_MAX_CAND];
  double pose[3];
  ndt_pg_edge edge;
} ndt_loop;
int ndt_sessions_find_loops(ndt_sessions *s, const unsigned char *which, const ndt_loop_params *p, ndt_loop *out,
                            int *n_out, ndt_result *records_host);

/* ---- Loop search over several old submaps per session, verified by ranged fitness --------------------------
 * A robot that re-enters a corridor passes several old submaps, and an old submap never covers the whole newest scan: the
 * points without a counterpart dominate PCL's full-cloud fitness, so ndt_sessions_find_loops rejects a correct pose in a
 * partly overlapping submap.  These calls search up to NDT_LOOP_MAX_SUBMAPS submaps per session and accept on the fitness of
 * the points within a range (ndt_fit_points' max_d2), given that enough of the scan lies within it.
 *
 * Gating.  Eligibility is exactly the rule above.  A session's candidates are its eligible submaps of smallest dist, at most
 * max_submaps of them, in ascending (dist, submap index); the sessions come in ascending order; every candidate of a session
 * has the same lattice, the one the rule above forms.  With max_submaps = 1 the output is byte-identical to
 * ndt_sessions_loop_candidates / ndt_loop_gate.  `out` needs room for n_sessions * max_submaps (ndt_loop_gate_multi:
 * max_submaps) candidates.  Refusals: those of the gating above, max_submaps outside 1 .. NDT_LOOP_MAX_SUBMAPS, max_d2 NaN or
 * negative, min_overlap NaN or outside [0, 1].
 *
 * The search is ndt_sessions_find_loops' list over the J candidates of all sessions, with two differences.  Every session's
 * newest scan is taken to the robot frame and filtered ONCE; all of that session's jobs name it.  Behind the multi-map match
 * comes one ndt_fit_points_multi_dev stage on the match's own device arrays (the laid-out scans, the slots' maps with -1 for a
 * dead slot, the records' transforms in place, max_d2; statistics only), whose J * top_k ndt_fit_stats travel back with the
 * records.  Two host waits; the number of launches, copies and waits depends neither on the number of sessions nor on
 * max_submaps.  The set owns up to NDT_LOOP_MAX_SUBMAPS loop maps per session, the slot is the candidate's rank, slot 0 is the
 * map ndt_sessions_find_loops keeps; all are destroyed with the set.  A slot is rebuilt in place by every search that has a
 * candidate of that rank for the session -- the three searches share the slots, and a cross search builds ANOTHER session's
 * cloud into the searcher's slot -- and no result depends on what a slot held before.  The call changes nothing of the SLAM
 * state.
 *
 * The decision, per candidate, on the host.  For slot c < n_cand, st = fit[c], r = record c:
 *   usable_c = r.converged && st.n_in >= 1 && (double)st.n_in >= min_overlap * (double)st.n_points (one rounded product);
 *   cand_cost[c] = usable_c ? st.fitness : 1e7;   ok_c = cand_cost[c] <= loop.max_cost;
 *   best = the slot that is first by: ok before not ok; then the larger (usable_c ? st.n_in : 0); then the lower cand_cost;
 *   then the lower c.  found = ok_best.  pose and edge come from the best record as ndt_sessions_find_loops forms them; with
 *   n_cand == 0: best = -1, pose and rel 0.  ok_c is the plain comparison also for a slot that is not usable: with
 *   loop.max_cost = +inf every candidate with a record is found (cost 1e7), with -inf none is; the caller that wants a
 *   verified loop keeps max_cost finite.
 * The inlier count ranks before the cost on purpose (ndt_relocalize's callers rank by ranged fitness alone): an alias that
 * overlaps less has fewer inliers, each of them tighter, and the lowest ranged fitness alone would pick it.
 *
 * Guarantees.  (a) A candidate's loop.cand, status, n_cand, cand_index, cand_score and records are byte-identical to what
 * ndt_sessions_find_loops gives for the same (session, submap, parameters); they do not depend on the other candidates or
 * sessions named, nor on max_submaps.  (b) fit[c] is byte-identical to ndt_fit_points_batch on that submap's map, the session's
 * filtered scan and record c's transform; fit is zero from n_cand on.  (c) A refused map (NDT_E_GRID or NDT_E_ARG from the
 * build) costs its candidate alone; a session whose newest scan is empty, or filters to nothing, gives the empty record for
 * each of its candidates; when every scan is empty the call queues nothing.  (d) ndt_sessions_get_stats: host_waits 2 (0 with
 * no candidate or with all scans empty, 1 when no map could be built), sessions_stepped = J.
 * Refusals: those of the gating, an open ndt_map_rebuild_begin on the context, more than 2^31 - 1 lattice poses over all
 * candidates.  NDT_E_HIP on a dead set; a HIP failure inside the call kills the set as in a step.
 * Out of scope: keeping the loop maps valid across calls; calling the optimiser for the caller.  (Loops between sessions:
 * the next section.) */
#define NDT_LOOP_MAX_SUBMAPS 4
typedef struct ndt_loop_multi_params {
  ndt_loop_params loop;     /* as for ndt_sessions_find_loops; loop.max_cost is compared with the RANGED cost above */
  int    max_submaps;       /* 1 .. NDT_LOOP_MAX_SUBMAPS candidate submaps per session */
  int    reserved;          /* 0 */
  double max_d2;            /* m^2, inclusive: the range of the verification (ndt_fit_points' max_d2) */
  double min_overlap;       /* 0 .. 1: share of the filtered scan that must lie within the range */
} ndt_loop_multi_params;
/* loop = ndt_loop_default_params, max_submaps 2, reserved 0, max_d2 0.09, min_overlap 0.5. */
int ndt_loop_multi_default_params(ndt_loop_multi_params *p);
/* ndt_loop_gate with up to p->max_submaps candidates (session 0) in (dist, submap) order; *n_out of them. */
int ndt_loop_gate_multi(const double *poses, size_t n_scans, const int *sub_first, const int *sub_anchor,
                        const uint64_t *sub_offsets, int n_submaps, const ndt_loop_multi_params *p,
                        ndt_loop_candidate *out, int *n_out);
int ndt_sessions_loop_candidates_multi(const ndt_sessions *s, const unsigned char *which, const ndt_loop_multi_params *p,
                                       ndt_loop_candidate *out, int *n_out);
typedef struct ndt_loop_multi {        /* HOST; one per candidate, in candidate order */
  ndt_loop      loop;                  /* every field as ndt_loop; cand_cost, best, found, pose, edge by the rule above */
  ndt_fit_stats fit[NDT_LOOP_MAX_CAND];/* slot c's ranged statistics at record c's transform; zero from n_cand on */
  int           rank;                  /* the candidate's place among its session's (0 = nearest) */
  int           reserved;
} ndt_loop_multi;
int ndt_sessions_find_loops_multi(ndt_sessions *s, const unsigned char *which, const ndt_loop_multi_params *p,
                                  ndt_loop_multi *out, int *n_out, ndt_result *records_host);

/* ---- Loops between the sessions of a set -------------------------------------------------------------------
 * Has session a just driven into a place that session b mapped -- several robots in one building, several logs of one site?
 * The sessions must share a map frame: a session's frame is its first odometry pose (src/ScanMatcher.cpp:9-22), so the caller
 * feeds odometry that starts at the robot's known pose.  An unknown offset between frames: the place section below.
 *
 * The cross gate.  Every searcher against every closed submap of every other track: a product, so it has a device form
 * (ndt_cross_gate_batch) beside the host definition (ndt_cross_gate); the two agree to the byte.  The rule is defined on the
 * SQUARED distance and takes no root.  For a searcher with last pose L = (x, y, th[deg]), track t and submap m of t:
 *   - t != own and m in 0 .. n_submaps - 2: every closed submap, the newest closed one included (the searcher's local map
 *     holds nothing of another session); own = -1: no track is the searcher's;
 *   - submap m owns the scans [sub_first[m], sub_first[m + 1] - 1];
 *   - d2(t, m) = the smallest, over the poses T[k] of that range, of dx * dx + dy * dy with dx = L.x - T[k].x, dy = L.y -
 *     T[k].y: fp64, each subtraction, product and the sum rounded once, no fused multiply-add; nearest_scan = the lowest k
 *     that attains it;
 *   - (t, m) is eligible when its scan range is not empty, its closed cloud has points (sub_offsets[m + 1] > sub_offsets[m])
 *     and d2 <= radius * radius (one rounded product);
 *   - the searcher's candidates are its max_submaps eligible (t, m) of smallest d2, in ascending (d2, t, m);
 *   - the lattice is the one ndt_loop_gate forms around L;
 *   - min_path is not read; every other field of ndt_loop_multi_params means what it means above.
 * ndt_cross_candidate: cand.session = the searcher (ndt_cross_gate: 0; the batch: its index), cand.submap = m, cand.anchor_scan
 * = sub_anchor[m] and cand.nearest_scan in track t's numbering, cand.newest_scan as given, cand.dist = sqrt(d2) (host), cand.path
 * = 0; map_session = t; rank = the candidate's place among its searcher's; padding bytes are 0.
 * Refusals (NDT_E_ARG): those of ndt_loop_gate_multi for every track, the text naming the track ("track 3: ..."); a NULL
 * pointer, n_tracks < 1; a last pose that is not finite; own outside [-1, n_tracks); more than 2^28 (searcher, closed submap)
 * pairs.
 * ndt_cross_gate_batch: n_search searchers (last_poses 3 doubles each) in one table upload, two launches and one read-back,
 * whatever n_search and n_tracks are; synchronous, on the context's stream.  out[i * max_submaps + r] is candidate r of
 * searcher i for r < n_out[i]; the records from n_out[i] on are zero.  out and n_out are byte-identical to n_search calls of
 * ndt_cross_gate (with cand.session = i).
 *
 * ndt_sessions_cross_candidates / ndt_sessions_find_cross_loops.  Searchers: the sessions with which[i] (NULL: all) that have
 * started.  Tracks: the sessions with against[i] (NULL: all) that have started and have at least one closed submap, in
 * ascending session order.  The candidates are what ndt_cross_gate gives for each searcher on the tracks' ndt_sessions_trajectory
 * and ndt_sessions_global_map arrays, own = the searcher's own place among the tracks (-1 when it is none), with cand.session
 * and map_session given as SESSION indices; the searchers in ascending order, each one's candidates in a row; *n_out of them;
 * `out` needs room for n_sessions * max_submaps.  They are computed by the device gate (one host wait).
 * The search is ndt_sessions_find_loops_multi's, stage for stage, with one difference: a candidate's closed cloud and anchor
 * pose are map_session's, not the searcher's.  The map slots are the searcher's loop maps (slot = rank); each searcher's newest
 * scan is taken to the robot frame and filtered once.  m is filled as ndt_sessions_find_loops_multi fills it: m.loop.edge.from =
 * the anchor scan in map_session's trajectory, edge.to = the searcher's newest scan, rel = ndt_pg_edge_between(trajectory of
 * map_session [anchor], pose) -- an arc between two trajectories, for a joint graph of both.
 * Guarantees.  (a) A candidate's status, n_cand, cand_index, cand_score, records and fit are byte-identical to the same search
 * made of public calls on that cloud and that scan.  (b) They depend neither on the other searchers, nor on the other tracks
 * beyond eligibility, nor on max_submaps.  (c) A refused map costs its candidate alone; an empty newest scan gives the empty
 * record; a set of one session, or no eligible pair, gives *n_out = 0 and NDT_OK with nothing queued behind the gate.  (d) The
 * SLAM state is untouched.  (e) ndt_sessions_get_stats: host_waits 3 (the gate, the boxes, the records), 1 when the gate finds
 * nothing (0 when there is no searcher or no track: the gate is not run), 1 also when every searcher that has a candidate has
 * an empty newest scan (the candidates are given, each with the empty record, and nothing is queued behind the gate), 2 when
 * no map could be built; sessions_stepped = J; launches, copies and waits do not depend on the number of sessions.
 * Refusals: those of ndt_sessions_find_loops_multi; NDT_E_HIP on a dead set.
 * Out of scope: keeping cross edges from one search to the next; loop maps that stay valid across calls; a robust back end.
 * (An unknown offset between the sessions' frames: ndt_sessions_place_candidates below.) */
typedef struct ndt_cross_track {        /* HOST: one trajectory whose closed submaps may be searched */
  const double   *poses;  size_t n_scans;               /* ndt_sessions_trajectory */
  const int      *sub_first, *sub_anchor;               /* n_submaps entries each */
  const uint64_t *sub_offsets;  int n_submaps;          /* ndt_sessions_global_map: n_submaps + 1 entries */
} ndt_cross_track;
typedef struct ndt_cross_candidate {
  ndt_loop_candidate cand;
  int map_session, rank;
  double d2;
} ndt_cross_candidate;
int ndt_cross_gate(const double last_pose[3], int newest_scan, int own, const ndt_cross_track *tracks, int n_tracks,
                   const ndt_loop_multi_params *p, ndt_cross_candidate *out, int *n_out);
int ndt_cross_gate_batch(ndt_ctx *ctx, const double *last_poses, const int *newest_scan, const int *own, int n_search,
                         const ndt_cross_track *tracks, int n_tracks, const ndt_loop_multi_params *p,
                         ndt_cross_candidate *out, int *n_out);
typedef struct ndt_cross_loop { ndt_loop_multi m; int map_session, reserved; } ndt_cross_loop;
int ndt_sessions_cross_candidates(ndt_sessions *s, const unsigned char *which, const unsigned char *against,
                                  const ndt_loop_multi_params *p, ndt_cross_candidate *out, int *n_out);
int ndt_sessions_find_cross_loops(ndt_sessions *s, const unsigned char *which, const unsigned char *against,
                                  const ndt_loop_multi_params *p, ndt_cross_loop *out, int *n_out, ndt_result *records_host);

/* ---- Place recognition: where two sessions overlap without a shared frame ---------------------------------
 * The gates above are distance gates around the last pose: they need the searcher and the map in one frame.  Two robots started
 * somewhere in one building, two logs of one site, or a session whose drift exceeds `radius` have none.  This section gives a
 * ROTATION-INVARIANT DESCRIPTOR of a cloud about a centre and an all-pairs match of descriptors that returns, per query, a few
 * candidates (item, descriptor, rotation) with no pose prior; the candidates then go through the verification that exists
 * (ndt_score_lattice_multi_dev .. ndt_fit_points_multi_dev).  Integer work throughout: every device result
 * is byte-identical to the host definition.
 *
 * THE DESCRIPTOR of a cloud about the centre (cx, cy) is n_rings uint64_t words: bit s of word r says that cell (ring r, sector
 * s) holds at least min_pts points.  The axes are the cloud's own: no heading, no trigonometry.  For a float32 point (x, y),
 * every operation fp64 and rounded once, no fused multiply-add:
 *   dx = (double)x - cx, dy = (double)y - cy, r2 = dx * dx + dy * dy;
 *   the point is skipped when r2 is not finite, r2 < r_min * r_min, or r2 >= edge2[n_rings], with
 *   edge2[j] = (j * ring_width) * (j * ring_width), j = 1 .. n_rings (two rounded products);
 *   ring = the number of j in 1 .. n_rings with r2 >= edge2[j];
 *   ax = |dx|, ay = |dy|, a = max(ax, ay), b = min(ax, ay); sub = the number of j in 1 .. 7 with b >= T[j] * a (one rounded
 *   product), T = NDT_PLACE_TAN below: the fp64 nearest to tan(j pi / 32); s16 = (ay > ax) ? 15 - sub : sub;
 *   sector = dx >= 0 ? (dy >= 0 ? s16 : 63 - s16) : (dy >= 0 ? 31 - s16 : 32 + s16).
 * The counts are integers: the descriptor does not depend on the order of the points.  An empty cloud gives zero words.
 * ndt_place_describe is the definition (host, no context, no device).  ndt_place_describe_batch_dev: n_desc descriptors in one
 * table upload and one launch, whatever n_desc; descriptor k is of cloud cloud_of[k] -- the points [offsets[c], offsets[c + 1]) of
 * xy_dev, stride_bytes apart (8 or 16) -- about centres[2k], centres[2k + 1]; several centres may name one cloud; desc_dev[k *
 * n_rings + r].  Every descriptor is byte-identical to ndt_place_describe and depends neither on the other descriptors, nor on
 * NDT_OPT_WORKGROUPS, nor on the stride.  ndt_place_describe_batch: the same with host pointers, synchronous.
 *
 * THE KEY of a query Q against an entry D (n_rings words each) at the shift s in 0 .. 63:
 *   c(s) = sum over r of popcount(Q_r & rotl64(D_r, s)), na = sum popcount(Q_r), nb = sum popcount(D_r), den = na + nb - c(s),
 *   key(s) = den == 0 ? 0 : (c(s) * 65536) / den (unsigned 32-bit division): the Jaccard overlap of the two cell sets in 1/65536.
 * A direction theta in the query's axes is the direction theta - s * 5.625 deg in the entry's axes.  The best shift of an entry
 * is the one of largest key, ties to the smallest s.  Entries are grouped into ITEMS: item i = the descriptors [item_first[i],
 * item_first[i + 1]) -- one submap described about several poses.  An item's hit = its descriptor of largest key, ties to the
 * lowest descriptor.  An item is skipped for a query when q_group >= 0 && q_group == item_group[i] (its own session) or when it
 * has no descriptor.  A query's result = its at most top_k items with key >= min_key, in descending key, ties to the lower item.
 * ndt_place_key: one (Q, D, s) (host).  ndt_place_match_host: the definition (host, no context).  ndt_place_match_dev: one table
 * upload and two launches (match, pick), no host wait.  out[q * top_k + j] is hit j of query q for j < n_out[q]; the records
 * from n_out[q] on are zero.  table (may be NULL): table[q * n_items + i] = (key << 32) | (0xFFFFFFFF - (desc << 6 | shift)) of
 * item i's hit, 0 when the item is skipped -- the ordering rules are one unsigned maximum.  out, n_out and table are
 * byte-identical to ndt_place_match_host; a query's bytes depend neither on the other queries nor on NDT_OPT_WORKGROUPS.
 * ndt_place_match: the same with host pointers, synchronous.  ndt_place_hit: desc counts from the first descriptor of the call;
 * overlap = c(shift), n_query = na, n_entry = nb; rank = j.
 *
 * Refusals (NDT_E_ARG, nothing queued or written): a NULL context ("null context") or pointer; a parameter outside the range
 * given beside it below, the text naming it ("ring_width", ...); a stride other than 8 or 16; n_clouds, n_desc, n_q or n_items
 * below 0; offsets that decrease; a cloud of more than 2^32 - 1 points; a non-finite centre; cloud_of outside [0, n_clouds);
 * item_first that does not start at 0 or decreases; more than 2^26 descriptors; n_q * n_items above 2^31 - 1.  Nothing to do
 * (n_desc, n_q == 0): NDT_OK.
 *
 * ndt_sessions_place_candidates.  Searchers and tracks are chosen as in ndt_sessions_cross_candidates.  A searcher's query is its
 * local map (the ndt_sessions_local_map points) about its last pose; its group is its session; a searcher without local-map
 * points gets no candidates.  Item (t, m) = closed submap m of track t with a non-empty cloud (as ndt_sessions_global_map returns
 * it) and a non-empty scan range, described about the trajectory poses of the scans sub_first[m] + j * centre_stride inside its
 * range; its group is the track's session; the items in ascending (t, m).  A candidate: session = the searcher, map_session and
 * submap = the item, centre_scan = the hit descriptor's scan in map_session's trajectory, shift .. rank as in ndt_place_hit,
 * guess = the searcher's newest pose in map_session's frame as the hit reads it: (centre.x, centre.y, last.th - shift * 5.625)
 * in (m, m, deg), not wrapped.  The searchers in ascending order, each one's candidates in a row; *n_out of them; `out` needs
 * room for n_sessions * top_k.  Guarantees: the candidates are byte-identical to ndt_place_describe_batch on those views followed
 * by ndt_place_match; they depend neither on the other searchers nor on top_k beyond truncation.  One table upload, one describe
 * launch for entries and queries together, the two match launches and one read-back as the only host wait (ndt_sessions_get_stats:
 * host_waits 1; 0 when there is no query or no item: nothing is queued), whatever the number of sessions.  The SLAM state is
 * untouched.  Descriptors are computed afresh on every call.  Refusals: a NULL set ("null session set"), a NULL pointer, a
 * parameter outside its range (the text names it), more descriptors or pairs than above, an open ndt_map_rebuild_begin on the
 * context.  NDT_E_HIP: a dead set.
 * Out of scope: descriptors kept across calls (ndt_sessions_correct and _remake_closed change the closed clouds); yaw finer
 * than a sector; mirrored maps. */
#define NDT_PLACE_SECTORS   64
#define NDT_PLACE_MAX_RINGS 32
#define NDT_PLACE_MAX_TOP_K 16
#define NDT_PLACE_TAN { 0x1.936bb8c5b2da2p-4, 0x1.975f5e0553158p-3, 0x1.36a08355c63dcp-2, 0x1.a827999fcef32p-2, 0x1.11ab7190834ebp-1, 0x1.561b82ab7f990p-1, 0x1.a43002ae4284fp-1 }
typedef struct ndt_place_params {
  double ring_width;    /* m, finite, > 0                          default 0.5  */
  double r_min;         /* m, finite, >= 0: nearer points skipped  default 0.25 */
  int    n_rings;       /* 1 .. 32                                 default 20   */
  int    min_pts;       /* >= 1: points a cell needs to count      default 1    */
  int    min_key;       /* 1 .. 65536: weaker hits are dropped     default 1    */
  int    top_k;         /* 1 .. 16                                 default 4    */
  int    centre_stride; /* >= 1 (ndt_sessions_place_candidates)    default 1    */
  int    reserved;      /* 0 */
} ndt_place_params;
typedef struct ndt_place_hit { int item, desc, shift, key, overlap, n_query, n_entry, rank; } ndt_place_hit;   /* 32 bytes */
typedef struct ndt_place_candidate {
  int session, map_session, submap, centre_scan, shift, key, overlap, n_query, n_entry, rank;
  double guess[3];
} ndt_place_candidate;
int ndt_place_default_params(ndt_place_params *p);
int ndt_place_describe(const float *xy_host, size_t n, size_t stride_bytes, double cx, double cy, const ndt_place_params *p,
                       uint64_t *desc_host);
int ndt_place_describe_batch_dev(ndt_ctx *ctx, const float *xy_dev, size_t stride_bytes, const uint64_t *offsets_host, int n_clouds,
                                 const double *centres_host, const int *cloud_of_host, int n_desc, const ndt_place_params *p,
                                 uint64_t *desc_dev, void *stream);
int ndt_place_describe_batch(ndt_ctx *ctx, const float *xy_host, size_t stride_bytes, const uint64_t *offsets_host, int n_clouds,
                             const double *centres_host, const int *cloud_of_host, int n_desc, const ndt_place_params *p,
                             uint64_t *desc_host);
int ndt_place_key(const uint64_t *q_desc, const uint64_t *d_desc, int n_rings, int shift, int *key, int *overlap);
int ndt_place_match_host(const uint64_t *q_desc, const int *q_group, int n_q, const uint64_t *d_desc, const int *item_first,
                         const int *item_group, int n_items, const ndt_place_params *p, uint64_t *table, ndt_place_hit *out,
                         int *n_out);
int ndt_place_match_dev(ndt_ctx *ctx, const uint64_t *q_desc_dev, const int *q_group_host, int n_q, const uint64_t *d_desc_dev,
                        const int *item_first_host, const int *item_group_host, int n_items, const ndt_place_params *p,
                        uint64_t *table_dev, ndt_place_hit *out_dev, int *n_out_dev, void *stream);
int ndt_place_match(ndt_ctx *ctx, const uint64_t *q_desc_host, const int *q_group_host, int n_q, const uint64_t *d_desc_host,
                    const int *item_first_host, const int *item_group_host, int n_items, const ndt_place_params *p,
                    uint64_t *table_host, ndt_place_hit *out_host, int *n_out_host);
int ndt_sessions_place_candidates(ndt_sessions *s, const unsigned char *which, const unsigned char *against,
                                  const ndt_place_params *p, ndt_place_candidate *out, int *n_out);

/* ---- The scan archive and ndt_sessions_occ_rebuild: occupancy grids that follow a correction -----------------
 * ndt_sessions_occ_integrate casts a session's newest scan at the pose it had at that step; after ndt_sessions_correct every beam
 * already in the grid lies where the uncorrected trajectory put it.  A set keeps only the current submap's scans (map frame,
 * float32), so nothing can be recast from it.  With an ARCHIVE a set keeps every stepped scan -- resampled, robot frame, fp64 --
 * on the device, and ndt_sessions_occ_rebuild casts the whole archive of any number of sessions into their grids at the poses
 * the trajectories hold NOW, before or after any number of corrections.
 *
 * ndt_sessions_archive_enable.  Off by default: a set without an archive behaves to the last byte and the last
 * ndt_sessions_stats field as it did before the archive existed.  Legal only while no session of the set has started (after
 * that NDT_E_ARG, the text names the first started session); idempotent.
 *
 * What is archived.  Exactly the scans a step records with stepped = 1: session i's archive always has the n_scans of
 * ndt_sessions_trajectory, and scan k of it belongs to pose k.  A scan refused with stepped = 0 is not archived; one whose
 * newest triple fails with the span error is; an empty scan is an empty range.  Stored are the bytes ndt_resample_batch_dev
 * wrote for the session at that step (double2), copied on the device by the step's own table of moves: with the archive on a
 * step has no further launch and no further host wait (host_waits stays 3), and uploads one more 24-byte move per session (the
 * only field of ndt_sessions_stats that differs is h2d_bytes).  Every step record, every view and every later
 * ndt_sessions_correct / ndt_sessions_find_loops result is byte-identical to a set without the archive.
 * ndt_sessions_correct does not touch the archive: robot-frame points do not move.  Cost: 16 bytes per resampled point (about
 * 16 KB per 1000-point scan), grown by doubling, never freed before the set; a failed growth ends the step as a failed growth
 * of a scan store does (NDT_E_HIP, the set is dead).
 *
 * Read-outs.  _info: host only.  _scans: scans [first, first + count) to the host, packed: xy_host takes *n_points double pairs,
 * offsets count + 1 entries relative to the first; xy_host == NULL returns the sizes (and the offsets).  _view: the device
 * address of the session's whole archive (NULL while it is empty), valid until the next step.  Refusals (NDT_E_ARG): a NULL
 * set ("null session set"), an index outside the set, a set without an archive, a range outside the archive, a capacity below
 * the range's points.
 *
 * ndt_sessions_occ_rebuild.  Session i is taken as in ndt_sessions_occ_integrate: (which == NULL or which[i] != 0) and it has
 * started.  clear != 0 zeroes a taken session's grid first, on the same stream.  Then, for every archived scan k of session i,
 * the beams of that scan go into occs[i]: a beam's end point is the float32 point ndt_scan_to_map_batch_dev writes for the
 * archived point and pose k of the trajectory as it is at the call (a = th * M_PI / 180, cos / sin, r00 * lx + r01 * ly + tx,
 * no contraction, rounded once to float32), its origin (tx, ty) of pose k.  Every other rule is ndt_occ_integrate's: the skips,
 * the walk, hit and pass, counters modulo 2^32, the stats.  DEFINITION: the grid after the call equals what
 * ndt_scan_to_map_batch_dev + ndt_occ_integrate_dev give for those scans and poses -- a function of archive, trajectory,
 * geometry and max_range2 alone; not of the other sessions named, of NDT_OPT_WORKGROUPS, or of anything a step or a correction
 * did in between.  One fused kernel reads each double2 once: there is no map-frame copy of the archive, the scratch is a table
 * of at most points / 256 + scans runs and 16 bytes per scan (the pose's cos and sin, computed once per scan).  One table upload (64 bytes per taken session, 32 per scan: the poses come from the
 * host's trajectory), the clears and two launches whatever the number of sessions and scans; stats_host (may be NULL) is the
 * one read-back and with it the call's only host wait.  Reads the set's state and changes none of it.  Grids are ordered as by
 * every ndt_occ_* call.  Refusals (NDT_E_ARG, nothing queued or written): those of ndt_sessions_occ_integrate, a set without an
 * archive, more than 2^31 - 1 scans or runs of 256 beams over the sessions taken.  NDT_E_HIP: a dead set. */
int ndt_sessions_archive_enable(ndt_sessions *s);
int ndt_sessions_archive_info(const ndt_sessions *s, int i, size_t *n_scans, size_t *n_points);
int ndt_sessions_archive_scans(ndt_sessions *s, int i, size_t first, size_t count, double *xy_host, size_t capacity_points,
                               uint64_t *offsets, size_t *n_points);
int ndt_sessions_archive_view(const ndt_sessions *s, int i, const double **xy_dev, size_t *n_points);
int ndt_sessions_occ_rebuild(ndt_sessions *s, ndt_occ *const *occs, const unsigned char *which, int clear, double max_range2,
                             ndt_occ_stats *stats_host);
/* ndt_sessions_remake_closed: PointCloudMap::remakeMaps for the CLOSED submaps, point by point.
 * ndt_sessions_correct moves a closed cloud as one rigid body by its anchor scan's pose pair; the reference moves every map
 * point by its own scan's pair (src/PointCloudMap.cpp:147-154), so the rigid move leaves the drift inside a closed submap where
 * it was.  With the archive, sessions which[0 .. n_named) get EVERY closed submap's cloud computed again from the archived
 * scans at the poses the trajectory holds now, and the local map and NDT map refreshed behind that.  Nothing of the
 * trajectory, of the current submap's scan store, cloud and prefix, or of the archive changes.  Meant to follow
 * ndt_sessions_correct; legal at any time.
 * DEFINITION.  Submap m owns the scans [sub_first[m], sub_last[m]], sub_last[m] = sub_first[m + 1] - 1 (ndt_sessions_trajectory).
 * Its scan list L_m is what its scan store held when it closed: L_0 = its own scans (none for the empty first submap of
 * sep_thre <= 0); for m >= 1 the last two scans of L_(m-1) -- none when L_(m-1) has fewer than two -- then its own
 * (src/PointCloudMap.cpp:72-90).  L_m is always a range of the archive, [sub_first[m] - carried_m, sub_last[m]].  Scan k in the
 * map frame is what ndt_scan_to_map_batch_dev writes for archived scan k and pose k of the trajectory (scan_to_map's
 * expressions, no contraction, rounded once to float32).  Closed cloud m is the TARGET range ndt_local_map_batch_dev gives one
 * descriptor with the scans of L_m, first_submap = (sub_first[m] == 0), newest = 1, the set's remove_moving, resol and
 * thre_neighbor, n_prev = 0, and the set's leaf: filterPoints(makeMap(L_m)), what a split stores.  An empty L_m gives an empty
 * cloud.  The closed block is rewritten with the new clouds back to back -- their sizes may change -- and
 * ndt_sessions_global_map's sub_offsets follow.  The local map becomes the new newest closed cloud followed by the filtered
 * tail of the present one, which keeps its bytes; the NDT map is rebuilt in place from it by the step's per-session refusal
 * rule.  A session without a local map at the moment gets its closed clouds remade and no local map.  A session without a
 * closed submap keeps every byte (NDT_OK).  A session's result is a function of its archive, its trajectory and the set's
 * parameters alone: not of who else is named, of NDT_OPT_WORKGROUPS, or of what steps, corrections or earlier remakes did; a
 * second call changes no byte.
 * status_host[c]: NDT_OK; NDT_E_ARG when a scan triple of any remade submap of the session spans more than 2^30 voxels: that
 * session keeps EVERY byte it had -- closed block, offsets, local map, NDT map (all or nothing per session); otherwise the code
 * ndt_map_build_batch_dev gives the new local map on its own (the closed clouds are remade, the map is left as it was, as in a
 * step).  Either way the call returns NDT_OK and no other session is concerned.  Sessions not named keep every byte.  Views
 * taken before the call are invalid after it, for every session.
 * Cost: one table upload (48 bytes per archived scan in use, 64 per named session), one kernel that writes each archived scan
 * in use ONCE into a map-frame scratch (consecutive submaps share it: a descriptor is a slice of the archive's offsets), the
 * assembly chain of ndt_local_map_batch_dev once over every closed submap of every named session, and TWO host waits (offsets
 * and status; the bounding boxes), whatever n_named, the number of closed submaps or their lengths.  The scratch holds every
 * scan in use (8 bytes per point) and every submap's cloud and target at capacity, all at once.  ndt_sessions_get_stats then
 * describes this call: host_waits 2, sessions_stepped = n_named, triples_run = triples recomputed, the bytes of its own tables
 * and read-backs.  When no named session has a closed submap that held a point there is nothing to compute: the call queues
 * nothing and host_waits is 0.
 * Refusals (NDT_E_ARG, synchronous, nothing changed, the text names the first offending entry): a NULL set ("null session
 * set"), NULL arrays, n_named < 1, a session outside the set or one that has not started, the same session twice, a set
 * without an archive, an open ndt_map_rebuild_begin on the context.  NDT_E_HIP: a dead set; a HIP failure inside the call
 * leaves the set dead, as in a step. */
int ndt_sessions_remake_closed(ndt_sessions *s, const int *which, int n_named, int *status_host);

/* Durations of the kernels of one of the context's last 64 match launches (`back` = 0: the most recent one):
 * the match kernel (rows a3-a6, a8, a9: start to stop of that kernel) and the fitness kernels behind it (row a7: stop of the
 * match kernel to stop of the last fitness kernel), from HIP events attached to the kernels' own dispatches on the launch's
 * stream.  Blocks until that launch has finished. */
int ndt_kernel_timing(ndt_ctx *ctx, int back, float *match_ms, float *fitness_ms);
/* Time from the start of the match kernel of launch `back + 1` to the start of the match kernel of launch `back` of
 * this context, from the same events: the step-to-step interval of a caller that issues launches back to back
 * (bench.py: ms_per_step_min / _max over the timed steps, without a further event record on the match stream).
 * Both launches must still be among the last 64.  Replaces the reference's per-scan "align time" log
 * (src/PoseEstimator.cpp:15,38-40). */
int ndt_launch_interval(ndt_ctx *ctx, int back, float *interval_ms);
/* Order another stream behind one of the context's last 64 match launches (`back` as above), fitness kernels included:
 * `stream` (hipStream_t; NULL = the context's stream) waits for the event attached to that launch's last kernel.  What a
 * caller would otherwise do with hipEventRecord on the launch's stream -- a packet of its own between two kernels
 * (6 us per launch on the stream that carries the matches) -- e.g. before the map the launch read is rebuilt on
 * another stream (the reference refills its target cloud every scan, src/ScanMatcher.cpp:40). */
int ndt_ctx_wait_launch(ndt_ctx *ctx, int back, void *stream);

/* Timing hooks used by bench.py (HIP events on the context's stream; milliseconds of the most
 * recent call of each kind, measured around the kernel launches only). */
int ndt_last_timing(const ndt_ctx *ctx, float *map_build_ms, float *align_ms);

/* Self-test of the device's float32 routines (ndt_params::libm_f32 = 1; ndt_slam_amd/csrc/ndt_libm_f32.hip.h): for n yaws
 * (host array, float32) the device's restatements of glibc's cosf / sinf and of the initial yaw computeTransformation reads
 * back from the guess matrix -- Eigen's Affine3f.rotation().eulerAngles(0,1,2)[2] with glibc's atan2f, from the cos / sin
 * just computed (src/PoseEstimator.cpp:22-24 -> the prologue of ndt.align, :28).  A caller on another platform checks them
 * against its own libm with this before trusting bit-level parity (tests/test_gpu_parity.py does, on 2e6 yaws).
 * Any output pointer may be NULL. */
int ndt_selftest_libm_f32(ndt_ctx *ctx, const float *yaw_host, size_t n, float *cos_out, float *sin_out, float *init_yaw_out);

/* Self-test of the optimiser's device functions (ndt_slam_amd/csrc/ndt_optimizer.hip.h), the functions the match kernel
 * calls, not copies: one lane per row, host arrays in and out, four independent parts.  A part whose input pointer is
 * NULL (or whose count is 0) is skipped; a part that runs needs its output pointer.
 *   solve3:     n x 9 doubles {Hxx, Hxy, Hxt, Hyy, Hyt, Htt, b0, b1, b2}          -> n x 3 doubles x (H x = b, pseudo-inverse)
 *   mt_trial:   n x 9 doubles {a_l, f_l, g_l, a_u, f_u, g_u, a_t, f_t, g_t}      -> n doubles, the trial value
 *   mt_update:  n x 9 doubles, the same layout                                   -> n x 7 doubles {a_l, f_l, g_l, a_u, f_u, g_u
 *               after the update, return value (1.0: interval converged)}, taken through the match kernel's state record
 *   yaw_from_T: n x 2 floats {T00, T10}                                           -> n doubles, the a9 yaw
 * NaN inputs are legal and give what the match gives: solve3 with a NaN entry of H returns NaN, a negative radicand in
 * mt_trial returns NaN.  (A whole match on non-finite input: see ndt_align.)
 * At most 2^26 rows per part.  NDT_E_ARG: no part to run, a missing output, too many rows. */
int ndt_selftest_optimizer(ndt_ctx *ctx, const double *solve3_in, size_t n_solve3, double *solve3_out,
                           const double *mt_trial_in, size_t n_mt_trial, double *mt_trial_out,
                           const double *mt_update_in, size_t n_mt_update, double *mt_update_out,
                           const float *yaw_in, size_t n_yaw, double *yaw_out);

#ifdef __cplusplus
}
#endif
#endif
