// ndt_resample.hip.h -- the two ends of ScanMatcher::matchScan for a batch on the device: the scan resampler
// (ScanPointResampler::resamplePoints, src/ScanPointResampler.cpp:4-62) and growMap's scan-to-map transform
// (src/ScanMatcher.cpp:96-101).  Part of libndt_mi355x.so: included by ndt_mi355x.hip inside its anonymous
// namespace (one translation unit, contraction off).  Not a standalone header.
//
// The resampler is a sequential walk, but it has two properties that split it:
//  * when the walk first looks at input point i, `prev` is the input point p[i-1] (after a drop or a keep prev
//    becomes the current point; after an interpolation the walk stays on i), so the first-look length
//    L_i = |p[i] - p[i-1]| does not depend on the walk: a parallel pre-pass computes it;
//  * the only state carried from one input point to the next is the accumulated distance dis in [0, space).
//    A point with L_i >= max(space, space_thre) is kept whatever dis is (dis + L >= L in IEEE arithmetic for
//    dis >= 0) and resets dis to 0.  Such "resync" points (and the first point of a scan) start independent
//    pieces, and one lane walks each piece in the reference's order, with its expressions.
// Every input point of a piece emits at most k_max points (the bound of ndt_resample_capacity): a lane writes
// the outputs of a piece starting at raw index s at s * k_max + t of the scratch, counts them, and one pass
// packs them after per-scan and batch prefix sums.  No input can make a lane loop longer than k_max turns at a
// point: reaching the cap (impossible for finite input) marks the scan as failed, like a non-finite coordinate.

constexpr int kRsGroup = 8;               // points a lane loads ahead of its walk (two groups in registers)
constexpr int kRsScanThreads = 1024;      // resample_segscan_kernel / resample_offsets_kernel
constexpr int kRsBadNonFinite = 1, kRsBadCap = 2;

__device__ __forceinline__ const double *rs_point(const double *xy, size_t stride, unsigned long long g) {
  return (const double *)((const char *)xy + g * stride);
}

// the scan that holds raw point g: the last b with offsets[b] <= g (empty scans are skipped)
__device__ __forceinline__ int rs_scan_of(const unsigned long long *__restrict__ offsets, int B, unsigned long long g) {
  int lo = 0, hi = B;                     // offsets[lo] <= g < offsets[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// Pre-pass, one thread per raw point: the first-look length L_i (+inf at the first point of a scan: a piece always
// starts there) and the non-finite check of the scan's coordinates.
__global__ void __launch_bounds__(256)
resample_prepass_kernel(const double *__restrict__ xy, size_t stride, const unsigned long long *__restrict__ offsets, int B,
                        unsigned long long total, double *__restrict__ L, int *__restrict__ bad) {
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const unsigned long long r0 = offsets[b], r1 = offsets[b + 1] < total ? offsets[b + 1] : total;
    bool nonfinite = false;
    for (unsigned long long g = r0 + blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; g < r1;
         g += (unsigned long long)gridDim.x * blockDim.x) {
      const double *p = rs_point(xy, stride, g);
      const double x = p[0], y = p[1];
      nonfinite |= !isfinite(x) || !isfinite(y);
      double l = INFINITY;
      if (g > r0) {
        const double *q = rs_point(xy, stride, g - 1);
        const double dx = x - q[0], dy = y - q[1];
        l = sqrt(dx * dx + dy * dy);
      }
      L[g] = l;
    }
    if (nonfinite) atomicOr(bad + b, kRsBadNonFinite);
  }
}

// The walk, one lane per piece: the thread of raw point g walks the piece that starts there (if one does).
// Points are loaded kRsGroup at a time, one group ahead of the walk.  A point at or past the piece's end reads as
// L = +inf, which ends the walk.
__global__ void __launch_bounds__(256)
resample_walk_kernel(const double *__restrict__ xy, size_t stride, const unsigned long long *__restrict__ offsets, int B,
                     unsigned long long total, const double *__restrict__ L, double space, double space_thre, double resync,
                     unsigned long long k_max, int *__restrict__ bad, double2 *__restrict__ scr,
                     unsigned long long *__restrict__ cnt, unsigned *__restrict__ dist) {
  const unsigned long long s = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x;
  if (s >= total || !(L[s] >= resync)) return;
  const int b = rs_scan_of(offsets, B, s);
  const unsigned long long e = offsets[b + 1] < total ? offsets[b + 1] : total;
  if (bad[b] || s < offsets[b] || s >= e) return;
  double2 *out = scr + s * k_max;
  unsigned long long t = 0;
  double px = rs_point(xy, stride, s)[0], py = rs_point(xy, stride, s)[1];
  out[t++] = make_double2(px, py);                      // the first point of a piece is the input point itself
  dist[s] = 0;
  double dis = 0.0;
  double cx[kRsGroup], cy[kRsGroup], cl[kRsGroup], nx[kRsGroup], ny[kRsGroup], nl[kRsGroup];
#pragma unroll
  for (int k = 0; k < kRsGroup; ++k) {                 // (loads without branches: a point past the end reads the last one)
    const unsigned long long i = s + 1 + k, j = i < e ? i : e - 1;
    const double l = L[j];
    cl[k] = i < e ? l : INFINITY;
    cx[k] = rs_point(xy, stride, j)[0];
    cy[k] = rs_point(xy, stride, j)[1];
  }
  for (unsigned long long i0 = s + 1;; i0 += kRsGroup) {
#pragma unroll
    for (int k = 0; k < kRsGroup; ++k) {               // the next group, in flight while this one is walked
      const unsigned long long i = i0 + kRsGroup + k, j = i < e ? i : e - 1;
      const double l = L[j];
      nl[k] = i < e ? l : INFINITY;
      nx[k] = rs_point(xy, stride, j)[0];
      ny[k] = rs_point(xy, stride, j)[1];
    }
#pragma unroll
    for (int k = 0; k < kRsGroup; ++k) {
      if (cl[k] >= resync) { cnt[s] = t; return; }    // the next piece (or the end of the scan) starts here
      const double x = cx[k], y = cy[k];
      double dx = x - px, dy = y - py, len = cl[k];     // first look: prev is p[i-1], L from the pre-pass
      unsigned long long here = 0;                      // points emitted at this input point
      for (;;) {
        const double acc = dis + len;
        if (acc < space) { dis = acc; break; }          // too close: dropped
        if (here == k_max) { atomicOr(bad + b, kRsBadCap); return; }
        if (acc >= space_thre) {                        // a gap: the point is kept as it is
          out[t++] = make_double2(x, y);
          dis = 0.0;
          break;
        }
        const double ratio = (space - dis) / len;       // interpolated at `space` along prev -> current
        const double qx = dx * ratio + px, qy = dy * ratio + py;
        out[t++] = make_double2(qx, qy);
        ++here;
        px = qx; py = qy; dis = 0.0;                    // ... and the same input point is looked at again
        dx = x - px; dy = y - py;
        len = sqrt(dx * dx + dy * dy);
      }
      px = x; py = y;
      dist[i0 + k] = (unsigned)(i0 + k - s);
    }
#pragma unroll
    for (int k = 0; k < kRsGroup; ++k) { cx[k] = nx[k]; cy[k] = ny[k]; cl[k] = nl[k]; }
  }
}

// Per scan, one workgroup: where each piece's points go inside the scan's output range (pos, at the piece's
// start) and the scan's output count (tot; 0 for a failed scan).
__global__ void __launch_bounds__(kRsScanThreads)
resample_segscan_kernel(const unsigned long long *__restrict__ offsets, int B, unsigned long long total,
                        const double *__restrict__ L, double resync, const int *__restrict__ bad,
                        const unsigned long long *__restrict__ cnt, unsigned long long *__restrict__ pos,
                        unsigned long long *__restrict__ tot) {
  __shared__ unsigned long long sh[kRsScanThreads / 64];
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    if (bad[b]) { if (threadIdx.x == 0) tot[b] = 0; continue; }
    const unsigned long long r0 = offsets[b], r1 = offsets[b + 1] < total ? offsets[b + 1] : total;
    // (the rounds of block_excl_offsets, over raw indices from r0 on: its items count from 0, which costs registers here)
    unsigned long long carry = 0;
    for (unsigned long long base = r0; base < r1; base += kRsScanThreads) {
      const unsigned long long g = base + threadIdx.x;
      const bool start = g < r1 && L[g] >= resync;
      const unsigned long long v = start ? cnt[g] : 0ull;
      unsigned long long sum;
      const unsigned long long incl = block_incl_scan<kRsScanThreads>(v, sh, &sum);
      if (start) pos[g] = carry + incl - v;
      carry += sum;
    }
    if (threadIdx.x == 0) tot[b] = carry;
  }
}

// One workgroup: the batch's output offsets (exclusive sum of the scans' counts) and the per-scan status.
__global__ void __launch_bounds__(kRsScanThreads)
resample_offsets_kernel(const unsigned long long *__restrict__ tot, const int *__restrict__ bad, int B,
                        unsigned long long *__restrict__ out_offsets, int *__restrict__ status) {
  __shared__ unsigned long long sh[kRsScanThreads / 64];
  const unsigned long long sum = block_excl_offsets<kRsScanThreads>(
      B, sh, [&](int b) { return tot[b]; },
      [&](int b, unsigned long long off, unsigned long long) {
        out_offsets[b] = off;
        if (status) status[b] = bad[b] ? NDT_E_ARG : NDT_OK;
      });
  if (threadIdx.x == 0) out_offsets[B] = sum;
}

// The pack, one thread per raw point: the scratch slots [d * k_max, (d + 1) * k_max) of the piece that holds the
// point (d = its distance from the piece's start) that carry outputs go to the packed results.
__global__ void __launch_bounds__(256)
resample_pack_kernel(const unsigned long long *__restrict__ offsets, int B, unsigned long long total,
                     const int *__restrict__ bad, const double2 *__restrict__ scr, unsigned long long k_max,
                     const unsigned long long *__restrict__ cnt, const unsigned long long *__restrict__ pos,
                     const unsigned *__restrict__ dist, const unsigned long long *__restrict__ out_offsets,
                     double2 *__restrict__ out64, float2 *__restrict__ out32) {
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    if (bad[b]) continue;
    const unsigned long long r0 = offsets[b], r1 = offsets[b + 1] < total ? offsets[b + 1] : total, q0 = out_offsets[b];
    for (unsigned long long g = r0 + blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; g < r1;
         g += (unsigned long long)gridDim.x * blockDim.x) {
      const unsigned long long d = dist[g];
      if (d > g - r0) continue;                          // (only with offsets that are not ascending)
      const unsigned long long s = g - d, c = cnt[s];
      const unsigned long long t0 = d * k_max, q = q0 + pos[s];
      const double2 *src = scr + s * k_max;
      for (unsigned long long t = t0; t < c && t < t0 + k_max; ++t) {
        const double2 v = src[t];
        if (out64) out64[q + t] = v;
        if (out32) out32[q + t] = make_float2((float)v.x, (float)v.y);
      }
    }
  }
}

// growMap's transform (src/ScanMatcher.cpp:96-101) with Rmat as Pose2D::calRmat builds it
// (include/ndt_slam/Pose2D.h:43-47), then PointCloudMap::addPoints' conversion to float32: one thread per point.
__global__ void __launch_bounds__(256)
scan_to_map_kernel(const double *__restrict__ xy, size_t stride, const unsigned long long *__restrict__ offsets, int B,
                   unsigned long long total, const double *__restrict__ poses, float2 *__restrict__ out) {
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const unsigned long long r0 = offsets[b], r1 = offsets[b + 1] < total ? offsets[b + 1] : total;
    if (r0 >= r1) continue;
    const double tx = poses[3 * b], ty = poses[3 * b + 1], a = poses[3 * b + 2] * M_PI / 180;
    const double c = cos(a), sn = sin(a);
    const double r00 = c, r01 = -sn, r10 = sn, r11 = c;
    for (unsigned long long g = r0 + blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; g < r1;
         g += (unsigned long long)gridDim.x * blockDim.x) {
      const double *p = rs_point(xy, stride, g);
      const double lx = p[0], ly = p[1];
      const double x = r00 * lx + r01 * ly + tx;
      const double y = r10 * lx + r11 * ly + ty;
      out[g] = make_float2((float)x, (float)y);
    }
  }
}
