// ndt_common.hip.h -- device-side views of the map and small helpers shared by all kernels.
// Part of libndt_mi355x.so: included by ndt_mi355x.hip inside its anonymous namespace (one translation
// unit; the order of the includes matters).  Not a standalone header.

// ------------------------------------------------------------------------------------------
// device-side views
// ------------------------------------------------------------------------------------------

// Dense voxel grid padded by 2 cells on every side so that the 3x3 probe of any point whose
// voxel lies within one cell of the map's bounding box needs no bounds checks.
struct MapView {
  float inv_leaf, leaf, r2;
  int radius_inclusive, transform_sse;
  int min_bx, min_by, div_x, div_y;  // unpadded voxel grid (VoxelGridCovariance min_b_/div_b_)
  int gw, gh;                        // padded: div + 4
  const float2 *cent;                // gw*gh float32 centroids; +inf where the voxel is not in
                                     // the centroid search set (fewer than min_pts points)
  const double *rec;                 // gw*gh records of 8 doubles (64 B):
                                     // mean_x, mean_y, icov_xx, icov_xy, icov_yy, 3 pad
  const unsigned *occ;               // one bit per voxel of the unpadded grid: in the centroid search set
  const unsigned long long *tiles;   // which voxels hold raw points, 8 x 8 voxels per word (bit 8 (y & 7) + (x & 7)), tile
  int tiles_w;                       // (tx, ty) at [(ty + 1) tiles_w + tx + 1]: one tile of zeros all around (a7, far queries)
  const int *pt_start;               // div_x*div_y + 1 bucket offsets of the raw points
  const float2 *pts;                 // raw points bucketed by voxel, input order kept (a7)
  double d1, d2;                     // Gaussian constants (a3)
  double e_hi;                       // pairs with exp(..) > e_hi fail updateDerivatives' `d2 e in [0, 1]` check (ndt_point.hip.h)
};

struct OptParams {
  double step_size, trans_eps, snap_thresh, mt_mu, mt_nu;
  int max_iter, conv_ge, stale_h_ang, mt_max_iter;
  int libm_f32;                 // ndt_params::libm_f32: the float32 cos / sin of a trial as glibc computes them (ndt_libm_f32.hip.h)
};

struct Tf32 { float c, s, tx, ty; };

// eleven partial sums of one derivative pass
struct Acc {
  double e, g0, g1, g2, hxx, hxy, hxt, hyy, hyt, htt;
  unsigned pairs;
};
constexpr int kAcc = 11;

enum Phase : int { PH_INIT = 0, PH_LS_FIRST = 1, PH_LS_INNER = 2, PH_DONE = 3 };

// Resumable optimiser state of one match.  One lane advances it after every derivative pass;
// kept free of any per-workgroup assumption so a pass can be produced by any set of waves.
struct AlignState {
  int phase, iters, evals, ref_evals, converged, step_iterations, open_interval, interval_converged;
  Tf32 T;                       // final_transformation_ (float32)
  double cj, sj, ch, sh;        // angle terms of J_E and of the (yaw,yaw) block of H_E
  double p[3], dir[3], xt[3];
  double score, g[3], H[6];     // xx xy xt yy yt tt
  double phi0, dphi0, a_l, f_l, g_l, a_u, f_u, g_u, a_t;
  double pairs;
  double n_points;
  int need_tf;                  // set_trial: bit 0 = the trial's transforms are still to be formed (trial_transforms), bit 1 = with the Hessian angle terms
};

// ------------------------------------------------------------------------------------------
// small device helpers
// ------------------------------------------------------------------------------------------

// Loads through a pointer that is known to address device memory.  A pointer that reached a function through LDS
// (pass_units) has lost its address space: the compiler then emits flat_load, which counts on vmcnt AND lgkmcnt,
// so every LDS read behind it waits for the memory load as well (the software prefetch of the point loop was
// waited for at once).  These helpers put the address space back: global_load.
#define NDT_GLOBAL __attribute__((address_space(1)))
typedef float ndt_f2v __attribute__((ext_vector_type(2)));
typedef float ndt_f4v __attribute__((ext_vector_type(4)));
typedef double ndt_d2v __attribute__((ext_vector_type(2)));
typedef int ndt_i4v __attribute__((ext_vector_type(4)));
typedef int ndt_i2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2 gld_f2(const float2 *p) {
  const ndt_f2v v = *(const NDT_GLOBAL ndt_f2v *)p;
  return make_float2(v.x, v.y);
}
__device__ __forceinline__ float4 gld_f4(const float4 *p) {
  const ndt_f4v v = *(const NDT_GLOBAL ndt_f4v *)p;
  return make_float4(v.x, v.y, v.z, v.w);
}
// the same at a 32-bit byte offset from a wave-uniform base: global_load vdst, voffset, s[base] -- one VALU
// instruction per address instead of three (sign extension + 64-bit add) when a lane walks its own range
__device__ __forceinline__ float2 gld_f2_at(const void *base, unsigned byte_off) {
  const ndt_f2v v = *(const NDT_GLOBAL ndt_f2v *)((const NDT_GLOBAL char *)base + byte_off);
  return make_float2(v.x, v.y);
}
__device__ __forceinline__ float4 gld_f4_at(const void *base, unsigned byte_off) {
  const ndt_f4v v = *(const NDT_GLOBAL ndt_f4v *)((const NDT_GLOBAL char *)base + byte_off);
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ double2 gld_d2(const double *p) {
  const ndt_d2v v = *(const NDT_GLOBAL ndt_d2v *)p;
  return make_double2(v.x, v.y);
}
__device__ __forceinline__ double gld_d(const double *p) { return *(const NDT_GLOBAL double *)p; }
__device__ __forceinline__ int gld_i(const int *p) { return *(const NDT_GLOBAL int *)p; }
// Inclusive prefix sum over the 64 lanes of a wave with DPP moves only (row shifts with zero fill, then the row totals
// carried into the next rows): no LDS round trips.
__device__ __forceinline__ unsigned wave_incl_scan(unsigned x) {
#define NDT_DPP_ADD(CTRL, ROWS) x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROWS, 0xF, true)
  NDT_DPP_ADD(0x111, 0xF);     // row_shr:1
  NDT_DPP_ADD(0x112, 0xF);     // row_shr:2
  NDT_DPP_ADD(0x114, 0xF);     // row_shr:4
  NDT_DPP_ADD(0x118, 0xF);     // row_shr:8
  NDT_DPP_ADD(0x142, 0xA);     // row_bcast15: the total of rows 0 / 2 into rows 1 / 3
  NDT_DPP_ADD(0x143, 0xC);     // row_bcast31: the total of rows 0 + 1 into rows 2, 3
#undef NDT_DPP_ADD
  return x;
}

// min / max over the 64 lanes with DPP moves (row shifts, then the rows' results carried along): valid in lane 63
__device__ __forceinline__ int wave_min_dpp(int x) {
#define NDT_DPP_MIN(CTRL, ROWS) { const int t_ = __builtin_amdgcn_update_dpp(x, x, CTRL, ROWS, 0xF, false); x = t_ < x ? t_ : x; }
  NDT_DPP_MIN(0x111, 0xF) NDT_DPP_MIN(0x112, 0xF) NDT_DPP_MIN(0x114, 0xF) NDT_DPP_MIN(0x118, 0xF) NDT_DPP_MIN(0x142, 0xA) NDT_DPP_MIN(0x143, 0xC)
#undef NDT_DPP_MIN
  return x;
}
__device__ __forceinline__ int wave_max_dpp(int x) {
#define NDT_DPP_MAX(CTRL, ROWS) { const int t_ = __builtin_amdgcn_update_dpp(x, x, CTRL, ROWS, 0xF, false); x = t_ > x ? t_ : x; }
  NDT_DPP_MAX(0x111, 0xF) NDT_DPP_MAX(0x112, 0xF) NDT_DPP_MAX(0x114, 0xF) NDT_DPP_MAX(0x118, 0xF) NDT_DPP_MAX(0x142, 0xA) NDT_DPP_MAX(0x143, 0xC)
#undef NDT_DPP_MAX
  return x;
}
__device__ __forceinline__ unsigned long long gld_u64(const unsigned long long *p) { return *(const NDT_GLOBAL unsigned long long *)p; }

// ------------------------------------------------------------------------------------------
// wave and workgroup primitives
// ------------------------------------------------------------------------------------------

// 64-bit values: the __shfl_up form (DPP moves are 32 bits wide).  int: the DPP form.
__device__ __forceinline__ int wave_incl_scan(int x) { return (int)wave_incl_scan((unsigned)x); }
__device__ __forceinline__ unsigned long long wave_incl_scan(unsigned long long x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const unsigned long long u = __shfl_up(x, o, 64); if (lane >= o) x += u; }
  return x;
}

// Reductions over the 64 lanes, valid in lane 0.  The tree is fixed -- lane l takes lane l + 32, then + 16, ... + 1 -- and
// every floating-point sum that is compared bit for bit depends on it (the match, score and fitness sums, the pose graph).
template <typename T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
  return x;
}
__device__ __forceinline__ float wave_min(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fminf(x, __shfl_down(x, o));
  return x;
}
__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_down(x, o));
  return x;
}
__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_down(x, o));
  return x;
}
// The integer minimum with the result in every lane (butterfly).
__device__ __forceinline__ int wave_min_all(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o));
  return x;
}

// Inclusive sum over a workgroup of exactly kThreads threads (a multiple of 64, at most 1024), every thread calling it: the
// wave scan, the waves' totals through sh[kThreads / 64] and wave 0, three barriers.  *total: the sum of all threads'
// values.  T: unsigned, or unsigned long long.  sh may be used again as soon as the call returns.
template <int kThreads, typename T>
__device__ __forceinline__ T block_incl_scan(T v, T *sh, T *total) {
  constexpr int kWaves = kThreads / 64;
  static_assert(kThreads % 64 == 0 && kWaves >= 1 && kWaves <= 16, "whole waves, at most 1024 threads");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_incl_scan(v);
  if (lane == 63) sh[wave] = v;
  __syncthreads();
  if (wave == 0) {
    const T w = wave_incl_scan(lane < kWaves ? sh[lane] : (T)0);
    if (lane < kWaves) sh[lane] = w;
  }
  __syncthreads();
  const T r = v + (wave ? sh[wave - 1] : (T)0);
  *total = sh[kWaves - 1];
  __syncthreads();
  return r;
}

// Exclusive offsets of n items by ONE workgroup of kThreads threads, in rounds of kThreads items with a carry: thread t of
// round r has item i = r kThreads + t, v = load(i), and store(i, sum of the items in front of i, v); returns the sum of all
// items (in every thread).  load and store are called for i < n only, by the same thread, and all loads of a round come
// before its stores (a barrier lies between): a caller may keep what load found out in variables that store reads, and may
// store where it loaded.
template <int kThreads, typename T, typename I, typename Load, typename Store>
__device__ __forceinline__ T block_excl_offsets(I n, T *sh, Load load, Store store) {
  T carry = 0;
  for (I base = 0; base < n; base += (I)kThreads) {
    const I i = base + (I)threadIdx.x;
    const T v = i < n ? load(i) : (T)0;
    T sum;
    const T incl = block_incl_scan<kThreads>(v, sh, &sum);
    if (i < n) store(i, carry + incl - v, v);
    carry += sum;
  }
  return carry;
}

// Ballot compaction over a workgroup of kThreads threads: the number of flagged threads in front of this one (its place in a
// packed output that keeps the order) and, in *count, the number of flagged threads.  One barrier; wsum[kThreads / 64] must
// not be in use by a wave that is still in front of an earlier barrier.
template <int kThreads>
__device__ __forceinline__ int block_rank(bool flag, int *wsum, int *count) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long b = __ballot(flag);
  if (lane == 0) wsum[wave] = __builtin_popcountll(b);
  __syncthreads();
  int front = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) { const int c = wsum[w]; front += w < wave ? c : 0; all += c; }
  *count = all;
  return front + __builtin_popcountll(b & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ float2 load_pt(const float *xy, size_t stride, size_t i) {
  return *reinterpret_cast<const float2 *>(reinterpret_cast<const char *>(xy) + i * stride);
}

// The scan of match b in a launch's arrays: n points from point o0 of `scans`.  offsets holds B + 1 prefix offsets, or --
// shared_scan -- the one scan [offsets[0], offsets[1]) that every match uses.  slot: where match b's own elements start in the
// launch's per-point arrays (the ordered copies, fit, far_idx, d2): a scan of its own lies where it lies in `scans`, matches that
// share one have n elements each.  For the fitness kernels; ndt_align_kernel and ndt_order_kernel state the rule themselves
// (LOG R17.1: taking it out of the match kernel reschedules it).
struct ScanSpan {
  unsigned long long o0; int n;
  __device__ __forceinline__ size_t slot(int shared_scan, int b) const { return shared_scan ? (size_t)b * (size_t)n : (size_t)o0; }
};
__device__ __forceinline__ ScanSpan scan_span(const unsigned long long *__restrict__ offsets, int shared_scan, int b) {
  const unsigned long long o0 = shared_scan ? offsets[0] : offsets[b];
  const unsigned long long o1 = shared_scan ? offsets[1] : offsets[b + 1];
  return ScanSpan{o0, (int)(o1 - o0)};
}

// MULTI launches (ndt_align_batch_multi_dev): match b reads the map views[map_of[b]] (map_of null: views[b]); the index of a
// match is checked before anything is read through it.  -1: outside [0, n_maps), the match has no map.
__device__ __forceinline__ int map_index_of(const int *__restrict__ map_of, int n_maps, int b) {
  const int mi = map_of ? map_of[b] : b;
  return (mi >= 0 && mi < n_maps) ? mi : -1;
}

// float32 matrix of the fp64 parameter vector (a4): Translation3f(float(p0), float(p1), 0) *
// AngleAxisf(float(p2), Z); std::cos / std::sin(float): glibc's cosf / sinf (libm_f32) or modelled as correctly rounded.
__device__ __forceinline__ Tf32 tf_from_p(const double p[3], int libm_f32) {
  Tf32 t;
  float yaw = (float)p[2];
  if (libm_f32) {
    t.c = sincosf_glibc(yaw, 1);
    t.s = sincosf_glibc(yaw, 0);
  } else {
    double sd, cd;
    sincos_small((double)yaw, sd, cd);
    t.c = (float)cd;
    t.s = (float)sd;
  }
  t.tx = (float)p[0];
  t.ty = (float)p[1];
  return t;
}

// pcl::transformPointCloud on a z = 0 point, float32, no contraction.  SSE: the order of the additions of the map's build of PCL
// (MapView::transform_sse).
template <bool SSE>
__device__ __forceinline__ void tf_apply_t(const Tf32 &t, float x, float y, float &ox, float &oy) {
  const float ms = -t.s;
  const float a = t.c * x, b = ms * y, c = t.s * x, d = t.c * y;
  if (!SSE) { const float r = a + b; ox = r + t.tx; const float q = c + d; oy = q + t.ty; }
  else      { const float r = b + t.tx; ox = a + r; const float q = d + t.ty; oy = c + q; }
}
__device__ __forceinline__ void tf_apply(const Tf32 &t, int sse, float x, float y, float &ox, float &oy) {
  if (sse) tf_apply_t<true>(t, x, y, ox, oy); else tf_apply_t<false>(t, x, y, ox, oy);
}

// The voxel coordinate of a float: floor(x / leaf) as a float clamped to +-1e9, so that the conversion to int is defined for
// every input (NaN -> -1e9: outside every grid and window).  The build's grid (grid_of_box on the host, voxel_of) and every
// lookup of the match, score and fitness kernels go through this one definition: they must agree bit for bit.
__host__ __device__ __forceinline__ float voxel_coord(float x, float inv_leaf) {
  return fminf(fmaxf(floorf(x * inv_leaf), -1.0e9f), 1.0e9f);
}

__device__ __forceinline__ bool finite2(float x, float y) {
  return (fabsf(x) <= FLT_MAX) && (fabsf(y) <= FLT_MAX);
}

__device__ __forceinline__ void angle_cs(double snap, double yaw, double &c, double &s) {
  if (fabs(yaw) < snap) { c = 1.0; s = 0.0; }
  else { sincos_small(yaw, s, c); }
}
