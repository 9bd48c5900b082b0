// ndt_fit_points.hip.h -- ndt_fit_points_batch_dev: the distance of every scan point to its nearest raw map point, in the
// caller's order, and getFitnessScore(max_range) from them (row a7; src/PoseEstimator.cpp:43 calls it without a range);
// ndt_fit_points_multi_dev: the same with one map per match, through a table of views.
// Part of libndt_mi355x.so: included by ndt_mi355x.hip inside its anonymous namespace behind ndt_fitness.hip.h, whose
// search (lane_query -- nearest_prep / nearest_home / nearest_ring1_wave -- then nearest_far: path 2 of
// tests/test_gpu_fitness_geometry.py) it uses as it is.  Not a standalone header.

// ------------------------------------------------------------------------------------------
// The order of summation.  Chunk k of a match is its points [64k, 64k + 64) in INPUT order -- not the
// launch's voxel-ordered copy: the caller's indices are the only order that is the same for every way of calling.  A chunk's
// two sums (every point with a distance / those with (double)d2 <= max_d2) are the wave butterfly over the 64 lanes'
// (double)d2, 0.0 where the predicate fails; lane l of ONE wave adds the chunks l, l + 64, l + 128 ... in ascending order
// and the butterfly adds the lanes: chunk_part and close_chunks, which fitness_close_match uses too.  Counts are whole
// numbers however they are added.  So a match's d2 and ndt_fit_stats depend on (map, scan, transform, max_d2) alone, not
// on b, B, the other scans, the grid or shared_scan.  A chunk's part is 32 bytes of the context's scratch
// (ndt_ctx::d_fit_pts), first chunk of match b at fit_part_of: written by the wave that searched the chunk, read by the
// wave that closes the match.
// ------------------------------------------------------------------------------------------
struct FitPtsPart { double s_all, s_in, n_dist, n_in; };
static_assert(sizeof(FitPtsPart) == 32, "one 32-byte part per chunk");

// transform b of the call: four floats (c, s, tx, ty) at tf + b * stride bytes (the T00, T10, T03, T13 of an ndt_result)
__device__ __forceinline__ Tf32 fit_tf_of(const unsigned char *__restrict__ tf, size_t stride, int b) {
  const float *t = reinterpret_cast<const float *>(tf + (size_t)b * stride);
  return Tf32{t[0], t[1], t[2], t[3]};
}

// fitness_points_kernel<SSE, false> over the scan as the caller laid it out: the same waves (whole, a chunk each, lanes past
// the end without a query), the same search, the workgroups numbered by fit_block_of.  d2 (may be null): one float per
// point at the point's own index; parts (may be null): the chunk's sums and counts.
// MULTI (ndt_fit_points_multi_dev): match b is searched in views[match_map_index] instead of M_arg, the way
// fitness_points_kernel<.., MULTI> takes its table -- the view is this workgroup's only difference, so a match's d2 and
// parts are the single-map instance's.  A match without a map (index -1) reads nothing through the index: its workgroups
// write +INFINITY per point and empty parts (which close to {DBL_MAX, DBL_MAX, 0, 0, n, 0}) and return.
template <bool SSE, bool MULTI = false>
__global__ void __launch_bounds__(256, kFitOcc)
fit_points_kernel(MapView M_arg, const float2 *__restrict__ scans, const unsigned long long *__restrict__ offsets, int B,
                  int shared_scan, const unsigned char *__restrict__ tf, size_t tf_stride, double max_d2,
                  float *__restrict__ d2, FitPtsPart *__restrict__ parts, int gx, const MapView *__restrict__ views = nullptr,
                  const int *__restrict__ map_of = nullptr, int n_maps = 0) {
  __shared__ RingLds ring[256 / 64];
  int b, bx;
  if (!fit_block_of(gx, B, b, bx)) return;
  const int mi = match_map_index<MULTI>(map_of, n_maps, b);
  const ScanSpan sp = scan_span(offsets, shared_scan, b);
  const int n = sp.n;
  float *out = d2 ? d2 + sp.slot(shared_scan, b) : nullptr;
  FitPtsPart *part = parts ? parts + fit_part_of(sp, shared_scan, b) : nullptr;
  if (mi < 0) {                                                    // (workgroup-uniform; MULTI only)
    for (int i = bx * (int)blockDim.x + (int)threadIdx.x; i < n; i += gx * (int)blockDim.x) {
      if (out) out[i] = INFINITY;
      if (part && (i & 63) == 0) part[i >> 6] = FitPtsPart{0.0, 0.0, 0.0, 0.0};
    }
    return;
  }
  const MapView M = MULTI ? views[mi] : M_arg;
  const Tf32 T = fit_tf_of(tf, tf_stride, b);
  const float2 *pts = scans + sp.o0;
  for (int i0 = bx * (int)blockDim.x + (int)(threadIdx.x & ~63u); i0 < n; i0 += gx * (int)blockDim.x) {
    const int i = i0 + (int)(threadIdx.x & 63u);
    const LaneQuery Q = lane_query<SSE>(M, ring[threadIdx.x >> 6], T, pts, i, n);
    const float best = nearest_far(M, Q.qx, Q.qy, Q.S, Q.best);
    if (out && i < n) out[i] = Q.live ? best : INFINITY;
    if (part) {                                                  // (uniform) i0 is a multiple of 64: this wave's points are chunk i0 / 64
      const bool has = Q.live && best < INFINITY;
      const FitPart all = chunk_part(has, best), in = chunk_part(has && (double)best <= max_d2, best);
      if ((threadIdx.x & 63u) == 0u) part[i0 >> 6] = FitPtsPart{all.sum, in.sum, all.cnt, in.cnt};
    }
  }
}

// One wave per match: the match's ndt_fit_stats from its chunks, in the order stated above.
__global__ void __launch_bounds__(256)
fit_points_close_kernel(const unsigned long long *__restrict__ offsets, int B, int shared_scan,
                        const FitPtsPart *__restrict__ parts, ndt_fit_stats *__restrict__ stats) {
  const int lane = threadIdx.x & 63, b = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (b >= B) return;                                            // (whole waves)
  const ScanSpan sp = scan_span(offsets, shared_scan, b);
  double a[4];                                                   // s_all, s_in, n_dist, n_in
  close_chunks(parts + fit_part_of(sp, shared_scan, b), (sp.n + 63) >> 6, a);
  if (lane == 0) {
    ndt_fit_stats R;
    R.fitness = a[3] > 0.0 ? a[1] / a[3] : DBL_MAX;
    R.fitness_all = a[2] > 0.0 ? a[0] / a[2] : DBL_MAX;
    R.n_in = (uint32_t)a[3]; R.n_dist = (uint32_t)a[2]; R.n_points = (uint32_t)sp.n; R.reserved = 0u;
    stats[b] = R;
  }
}
