// ndt_occupancy.hip.h -- ndt_occ_*: occupancy grids of {hit, pass} counters, ray-cast from map-frame scans on the device
// (the contract is the header's).  Part of libndt_mi355x.so: included by ndt_mi355x.hip inside its
// anonymous namespace behind ndt_common.hip.h.  Not a standalone header.  Nothing here reads or writes what the match,
// score or fitness kernels use.

// ------------------------------------------------------------------------------------------
// The cell of a coordinate: floor((v - o) / res), one rounded fp64 subtraction, one rounded fp64 division (the file is
// compiled without contraction and with IEEE division), then floor.  ndt_occ_cell on the host and occ_integrate_kernel on
// the device call this one function.
// ------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ double occ_axis(double v, double o, double res) { return floor((v - o) / res); }

constexpr double kOccIndexMax = 1073741824.0;      // 2^30: cell indices of a beam's endpoints lie in [-2^30, 2^30]
constexpr unsigned kOccLenMax = 65536u;            // a beam's length in cells
constexpr int kOccRun = 256;                       // beams of a run = threads of a workgroup

// One row of a call's table (64 bytes).  The batch forms: row g is grid g, the scans come from the call's packed points and
// offsets.  The sessions form: row b is scan b AND its grid -- pts / n say where the scan lies; cells == nullptr: not taken.
struct OccRow {
  unsigned *cells;                   // nx * ny interleaved {hit, pass}
  double x0, y0, res;
  int nx, ny;
  const float2 *pts;
  unsigned long long n;
  unsigned long long pad;
};
static_assert(sizeof(OccRow) == 64, "one 64-byte row per grid");

// A run: up to kOccRun consecutive beams of scan b, from beam `first` of the scan.
struct OccJob { int b; int pad; unsigned long long first; };
static_assert(sizeof(OccJob) == 16, "one 16-byte job per run");

__device__ __forceinline__ unsigned long long occ_scan_len(const OccRow *__restrict__ tab, const unsigned long long *__restrict__ offsets, int b) {
  if (!offsets) return tab[b].cells ? tab[b].n : 0ull;
  const unsigned long long o0 = offsets[b], o1 = offsets[b + 1];
  return o1 > o0 ? o1 - o0 : 0ull;                 // (offsets that decrease: an empty scan, never a wild length)
}

// One workgroup: the runs of every scan, one behind the other (scan 0's first), never more than job_cap of them; the
// call's stats start at zero.
__global__ void __launch_bounds__(256)
occ_jobs_kernel(const OccRow *__restrict__ tab, const unsigned long long *__restrict__ offsets, int B, OccJob *__restrict__ jobs,
                unsigned job_cap, unsigned *__restrict__ n_jobs, unsigned long long *__restrict__ stats) {
  __shared__ unsigned long long sh[256 / 64];
  if (stats && threadIdx.x < 4) stats[threadIdx.x] = 0ull;
  const unsigned long long total = block_excl_offsets<256>(
      B, sh,
      [&](int b) { return (occ_scan_len(tab, offsets, b) + (unsigned long long)kOccRun - 1ull) / (unsigned long long)kOccRun; },
      [&](int b, unsigned long long j0, unsigned long long runs) {
        for (unsigned long long r = 0; r < runs && j0 + r < (unsigned long long)job_cap; ++r)
          jobs[j0 + r] = OccJob{b, 0, r * (unsigned long long)kOccRun};
      });
  if (threadIdx.x == 0) *n_jobs = (unsigned)(total < (unsigned long long)job_cap ? total : (unsigned long long)job_cap);
}

// no-return relaxed agent-scope integer add; the pointer came out of the call's table and is known to address device
// memory (NDT_GLOBAL, ndt_common.hip.h: global_atomic_add instead of the flat form)
__device__ __forceinline__ void occ_add(unsigned *p, unsigned v) {
  (void)__hip_atomic_fetch_add((NDT_GLOBAL unsigned *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A workgroup per run, balanced over CELLS: every thread classifies one beam (skip, or end cell and length L), the L + 1
// items of the live beams are prefix-summed in LDS, and the threads take the run's items in consecutive order -- item j
// belongs to the beam found by a search in the prefix, is its visit k = j - (items in front of the beam), and the last
// item of a beam is its hit.  Visit 0 of every live beam with L >= 1 is the scan's origin cell: the run adds those with ONE
// atomic.  grid_of == nullptr: every scan into row 0 (batch forms) or scan b into row b (sessions form, xy == nullptr).
__global__ void __launch_bounds__(256)
occ_integrate_kernel(const OccRow *__restrict__ tab, int n_occ, const int *__restrict__ grid_of, const float2 *__restrict__ xy,
                     const unsigned long long *__restrict__ offsets, const unsigned char *__restrict__ origins, size_t origin_stride,
                     double max_range2, const OccJob *__restrict__ jobs, const unsigned *__restrict__ n_jobs,
                     unsigned long long *__restrict__ stats) {
  __shared__ unsigned s_pref[kOccRun];             // inclusive prefix of the beams' items
  __shared__ int s_x1[kOccRun], s_y1[kOccRun];     // end cells
  __shared__ unsigned s_wave[4], s_org[4];
  __shared__ unsigned long long s_stat[4][4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned nj = *n_jobs;
  unsigned long long c_beams = 0ull, c_hit = 0ull, c_pass = 0ull, c_skip = 0ull;
  for (unsigned j = blockIdx.x; j < nj; j += gridDim.x) {
    const OccJob J = jobs[j];
    const int b = J.b;
    const bool own = xy == nullptr;                // the sessions form
    const int g = own ? b : (grid_of ? grid_of[b] : 0);
    const bool scan_ok = g >= 0 && g < n_occ && (!own || tab[b].cells != nullptr);
    const OccRow G = tab[scan_ok ? g : 0];
    const float2 *pts = own ? tab[b].pts : xy + offsets[b];
    const unsigned long long n = occ_scan_len(tab, offsets, b);
    const double *op = reinterpret_cast<const double *>(origins + (size_t)b * origin_stride);
    const double ox = op[0], oy = op[1];
    // the origin's cell (the same for the whole run)
    const double fx0 = occ_axis(ox, G.x0, G.res), fy0 = occ_axis(oy, G.y0, G.res);
    const bool org_ok = scan_ok && fabs(ox) <= DBL_MAX && fabs(oy) <= DBL_MAX && fx0 >= -kOccIndexMax && fx0 <= kOccIndexMax &&
                        fy0 >= -kOccIndexMax && fy0 <= kOccIndexMax;
    const int X0 = org_ok ? (int)fx0 : 0, Y0 = org_ok ? (int)fy0 : 0;
    // ---- classify: one beam per thread ----
    const unsigned long long i = J.first + (unsigned long long)tid;
    bool live = false;
    int X1 = 0, Y1 = 0;
    unsigned L = 0u;
    if (i < n) {
      c_beams++;
      const float2 p = gld_f2(pts + i);
      const double ex = (double)p.x, ey = (double)p.y;
      bool ok = org_ok && fabs(ex) <= DBL_MAX && fabs(ey) <= DBL_MAX;
      if (ok) {
        const double dx = ex - ox, dy = ey - oy;
        const double xx = dx * dx, yy = dy * dy;
        if (xx + yy > max_range2) ok = false;
      }
      if (ok) {
        const double fx1 = occ_axis(ex, G.x0, G.res), fy1 = occ_axis(ey, G.y0, G.res);
        ok = fx1 >= -kOccIndexMax && fx1 <= kOccIndexMax && fy1 >= -kOccIndexMax && fy1 <= kOccIndexMax;
        if (ok) {
          X1 = (int)fx1; Y1 = (int)fy1;
          const long long ax = llabs((long long)X1 - (long long)X0), ay = llabs((long long)Y1 - (long long)Y0);
          const long long len = ax > ay ? ax : ay;
          if (len > (long long)kOccLenMax) ok = false; else L = (unsigned)len;
        }
      }
      if (ok) live = true; else c_skip++;
    }
    const unsigned items = live ? L + 1u : 0u;
    // ---- the prefix of the items and the run's origin-cell count ----
    const unsigned incl = wave_incl_scan(items);
    const unsigned norg = (unsigned)__popcll(__ballot(live && L >= 1u));
    if (lane == 63) s_wave[wave] = incl;
    if (lane == 0) s_org[wave] = norg;
    s_x1[tid] = X1; s_y1[tid] = Y1;
    __syncthreads();
    unsigned front = 0u;
    for (int w = 0; w < wave; ++w) front += s_wave[w];
    s_pref[tid] = incl + front;
    __syncthreads();
    const unsigned total = s_pref[kOccRun - 1];
    const bool x_in0 = X0 >= 0 && X0 < G.nx && Y0 >= 0 && Y0 < G.ny;
    if (tid == 0) {
      const unsigned k0 = s_org[0] + s_org[1] + s_org[2] + s_org[3];
      if (k0 && x_in0) { occ_add(G.cells + 2 * ((size_t)Y0 * (size_t)G.nx + (size_t)X0) + 1, k0); c_pass += k0; }
    }
    // ---- the items, in consecutive order ----
    for (unsigned it = (unsigned)tid; it < total; it += (unsigned)kOccRun) {
      int t = 0;
#pragma unroll
      for (int step = kOccRun / 2; step > 0; step >>= 1)
        if (s_pref[t + step - 1] <= it) t += step;           // beams whose items all lie in front of `it`
      const unsigned excl = t ? s_pref[t - 1] : 0u;
      const unsigned k = it - excl, len = s_pref[t] - excl - 1u;
      const int ex1 = s_x1[t], ey1 = s_y1[t];
      int cx, cy, which;
      if (k == len) { cx = ex1; cy = ey1; which = 0; }         // the hit
      else {
        if (k == 0u) continue;                                 // the origin cell: added once for the run, above
        const long long ddx = (long long)ex1 - X0, ddy = (long long)ey1 - Y0;
        const long long ax = ddx < 0 ? -ddx : ddx, ay = ddy < 0 ? -ddy : ddy;
        const int sx = ddx > 0 ? 1 : (ddx < 0 ? -1 : 0), sy = ddy > 0 ? 1 : (ddy < 0 ? -1 : 0);
        const bool xmajor = ax >= ay;
        const unsigned long long m = (unsigned long long)(xmajor ? ay : ax);
        const unsigned long long q = (2ull * k * m + (unsigned long long)len - 1ull) / (2ull * (unsigned long long)len);
        cx = X0 + sx * (int)(xmajor ? (unsigned long long)k : q);
        cy = Y0 + sy * (int)(xmajor ? q : (unsigned long long)k);
        which = 1;
      }
      if (cx >= 0 && cx < G.nx && cy >= 0 && cy < G.ny) {
        occ_add(G.cells + 2 * ((size_t)cy * (size_t)G.nx + (size_t)cx) + which, 1u);
        if (which) c_pass++; else c_hit++;
      }
    }
    __syncthreads();                                           // (the LDS is the next run's)
  }
  // ---- the call's stats: per-wave sums, then one atomic per counter and workgroup ----
  if (!stats) return;
  const unsigned long long v[4] = {wave_sum(c_beams), wave_sum(c_hit), wave_sum(c_pass), wave_sum(c_skip)};
  if (lane == 0) { s_stat[wave][0] = v[0]; s_stat[wave][1] = v[1]; s_stat[wave][2] = v[2]; s_stat[wave][3] = v[3]; }
  __syncthreads();
  if (tid < 4) {
    const unsigned long long t = s_stat[0][tid] + s_stat[1][tid] + s_stat[2][tid] + s_stat[3][tid];
    if (t) (void)__hip_atomic_fetch_add(stats + tid, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ------------------------------------------------------------------------------------------
// ndt_sessions_occ_rebuild: the whole scan archive of the taken sessions, robot frame and fp64, cast at
// the trajectory's poses.  Row t of the table is taken session t: its grid, pts = its archive (double2), n = its first
// scan among the call's, pad = the call's offset of its first point.  Scan b (OccScan) is a pose and the call's offset of
// its first point; entry n_scans holds the total.
// ------------------------------------------------------------------------------------------
struct OccScan { double tx, ty, th; unsigned long long off; };
static_assert(sizeof(OccScan) == 32, "24 bytes of pose and 8 of offset per scan");

// occ_jobs_kernel over the archive's scans: job = (scan, its row, first beam); and every scan's (cos, sin) of its pose's
// heading, scan_to_map_kernel's expressions, once per scan
__global__ void __launch_bounds__(256)
occ_rebuild_jobs_kernel(const OccRow *__restrict__ tab, int n_rows, const OccScan *__restrict__ scans, int n_scans,
                        OccJob *__restrict__ jobs, unsigned job_cap, double2 *__restrict__ cs, unsigned long long *__restrict__ stats) {
  __shared__ unsigned long long sh[256 / 64];
  if (stats && threadIdx.x < 4) stats[threadIdx.x] = 0ull;
  (void)block_excl_offsets<256>(
      n_scans, sh,
      [&](int b) {
        const double a = scans[b].th * M_PI / 180;
        cs[b] = make_double2(cos(a), sin(a));
        const unsigned long long o0 = scans[b].off, o1 = scans[b + 1].off;
        return o1 > o0 ? (o1 - o0 + (unsigned long long)kOccRun - 1ull) / (unsigned long long)kOccRun : 0ull;
      },
      [&](int b, unsigned long long j0, unsigned long long runs) {
        if (!runs) return;
        int lo = 0, hi = n_rows - 1;               // the last row whose first scan is not behind b
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (tab[mid].n <= (unsigned long long)b) lo = mid; else hi = mid - 1;
        }
        for (unsigned long long r = 0; r < runs && j0 + r < (unsigned long long)job_cap; ++r)
          jobs[j0 + r] = OccJob{b, lo, r * (unsigned long long)kOccRun};
      });
}

// occ_integrate_kernel's run (classify, prefix, origin cell, items) on beams that are made here: the end point of beam i is
// scan_to_map_kernel's float32 point (ndt_resample.hip.h: the same expressions, the pose's cos / sin from the runs kernel's
// table) of the archived double2, the origin the pose's (tx, ty).  The runs are dealt in the order v -> (v * stride) % nj,
// stride coprime to nj and about one session's runs: workgroups that run side by side walk different sessions' grids
// instead of one session's neighbouring scans, whose beams share their first cells.
__global__ void __launch_bounds__(256)
occ_rebuild_kernel(const OccRow *__restrict__ tab, const OccScan *__restrict__ scans, const double2 *__restrict__ cs, double max_range2,
                   const OccJob *__restrict__ jobs, unsigned nj, unsigned long long stride, unsigned long long *__restrict__ stats) {
  __shared__ unsigned s_pref[kOccRun];
  __shared__ int s_x1[kOccRun], s_y1[kOccRun];
  __shared__ unsigned s_wave[4], s_org[4];
  __shared__ unsigned long long s_stat[4][4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long c_beams = 0ull, c_hit = 0ull, c_pass = 0ull, c_skip = 0ull;
  for (unsigned v = blockIdx.x; v < nj; v += gridDim.x) {
    const OccJob J = jobs[(unsigned)(((unsigned long long)v * stride) % (unsigned long long)nj)];
    const OccRow G = tab[J.pad];
    const OccScan P = scans[J.b];
    const unsigned long long n = scans[J.b + 1].off - P.off;
    const double2 *pts = reinterpret_cast<const double2 *>(G.pts) + (P.off - G.pad);
    const double ox = P.tx, oy = P.ty;
    const double fx0 = occ_axis(ox, G.x0, G.res), fy0 = occ_axis(oy, G.y0, G.res);
    const bool org_ok = fabs(ox) <= DBL_MAX && fabs(oy) <= DBL_MAX && fx0 >= -kOccIndexMax && fx0 <= kOccIndexMax &&
                        fy0 >= -kOccIndexMax && fy0 <= kOccIndexMax;
    const int X0 = org_ok ? (int)fx0 : 0, Y0 = org_ok ? (int)fy0 : 0;
    const double c = cs[J.b].x, sn = cs[J.b].y;
    const double r00 = c, r01 = -sn, r10 = sn, r11 = c;
    // ---- classify: one beam per thread ----
    const unsigned long long i = J.first + (unsigned long long)tid;
    bool live = false;
    int X1 = 0, Y1 = 0;
    unsigned L = 0u;
    if (i < n) {
      c_beams++;
      const double2 q = gld_d2(reinterpret_cast<const double *>(pts + i));
      const double lx = q.x, ly = q.y;
      const double mx = r00 * lx + r01 * ly + P.tx;
      const double my = r10 * lx + r11 * ly + P.ty;
      const double ex = (double)(float)mx, ey = (double)(float)my;
      bool ok = org_ok && fabs(ex) <= DBL_MAX && fabs(ey) <= DBL_MAX;
      if (ok) {
        const double dx = ex - ox, dy = ey - oy;
        const double xx = dx * dx, yy = dy * dy;
        if (xx + yy > max_range2) ok = false;
      }
      if (ok) {
        const double fx1 = occ_axis(ex, G.x0, G.res), fy1 = occ_axis(ey, G.y0, G.res);
        ok = fx1 >= -kOccIndexMax && fx1 <= kOccIndexMax && fy1 >= -kOccIndexMax && fy1 <= kOccIndexMax;
        if (ok) {
          X1 = (int)fx1; Y1 = (int)fy1;
          const long long ax = llabs((long long)X1 - (long long)X0), ay = llabs((long long)Y1 - (long long)Y0);
          const long long len = ax > ay ? ax : ay;
          if (len > (long long)kOccLenMax) ok = false; else L = (unsigned)len;
        }
      }
      if (ok) live = true; else c_skip++;
    }
    const unsigned items = live ? L + 1u : 0u;
    // ---- the prefix of the items and the run's origin-cell count ----
    const unsigned incl = wave_incl_scan(items);
    const unsigned norg = (unsigned)__popcll(__ballot(live && L >= 1u));
    if (lane == 63) s_wave[wave] = incl;
    if (lane == 0) s_org[wave] = norg;
    s_x1[tid] = X1; s_y1[tid] = Y1;
    __syncthreads();
    unsigned front = 0u;
    for (int w = 0; w < wave; ++w) front += s_wave[w];
    s_pref[tid] = incl + front;
    __syncthreads();
    const unsigned total = s_pref[kOccRun - 1];
    const bool x_in0 = X0 >= 0 && X0 < G.nx && Y0 >= 0 && Y0 < G.ny;
    if (tid == 0) {
      const unsigned k0 = s_org[0] + s_org[1] + s_org[2] + s_org[3];
      if (k0 && x_in0) { occ_add(G.cells + 2 * ((size_t)Y0 * (size_t)G.nx + (size_t)X0) + 1, k0); c_pass += k0; }
    }
    // ---- the items, in consecutive order ----
    for (unsigned it = (unsigned)tid; it < total; it += (unsigned)kOccRun) {
      int t = 0;
#pragma unroll
      for (int step = kOccRun / 2; step > 0; step >>= 1)
        if (s_pref[t + step - 1] <= it) t += step;
      const unsigned excl = t ? s_pref[t - 1] : 0u;
      const unsigned k = it - excl, len = s_pref[t] - excl - 1u;
      const int ex1 = s_x1[t], ey1 = s_y1[t];
      int cx, cy, which;
      if (k == len) { cx = ex1; cy = ey1; which = 0; }         // the hit
      else {
        if (k == 0u) continue;                                 // the origin cell: added once for the run, above
        const long long ddx = (long long)ex1 - X0, ddy = (long long)ey1 - Y0;
        const long long ax = ddx < 0 ? -ddx : ddx, ay = ddy < 0 ? -ddy : ddy;
        const int sx = ddx > 0 ? 1 : (ddx < 0 ? -1 : 0), sy = ddy > 0 ? 1 : (ddy < 0 ? -1 : 0);
        const bool xmajor = ax >= ay;
        const unsigned long long m = (unsigned long long)(xmajor ? ay : ax);
        const unsigned long long q = (2ull * k * m + (unsigned long long)len - 1ull) / (2ull * (unsigned long long)len);
        cx = X0 + sx * (int)(xmajor ? (unsigned long long)k : q);
        cy = Y0 + sy * (int)(xmajor ? q : (unsigned long long)k);
        which = 1;
      }
      if (cx >= 0 && cx < G.nx && cy >= 0 && cy < G.ny) {
        occ_add(G.cells + 2 * ((size_t)cy * (size_t)G.nx + (size_t)cx) + which, 1u);
        if (which) c_pass++; else c_hit++;
      }
    }
    __syncthreads();                                           // (the LDS is the next run's)
  }
  if (!stats) return;
  const unsigned long long v[4] = {wave_sum(c_beams), wave_sum(c_hit), wave_sum(c_pass), wave_sum(c_skip)};
  if (lane == 0) { s_stat[wave][0] = v[0]; s_stat[wave][1] = v[1]; s_stat[wave][2] = v[2]; s_stat[wave][3] = v[3]; }
  __syncthreads();
  if (tid < 4) {
    const unsigned long long t = s_stat[0][tid] + s_stat[1][tid] + s_stat[2][tid] + s_stat[3][tid];
    if (t) (void)__hip_atomic_fetch_add(stats + tid, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One thread per cell: 100 hit / n rounded half up, -1 below min_obs observations (ROS OccupancyGrid).
__global__ void __launch_bounds__(256)
occ_render_kernel(const uint2 *__restrict__ cells, size_t n_cells, unsigned min_obs, signed char *__restrict__ out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n_cells; i += (size_t)gridDim.x * blockDim.x) {
    const uint2 c = cells[i];
    const unsigned long long n = (unsigned long long)c.x + (unsigned long long)c.y;
    out[i] = n < (unsigned long long)min_obs ? (signed char)-1 : (signed char)((200ull * c.x + n) / (2ull * n));
  }
}
