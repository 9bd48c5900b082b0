// ndt_score.hip.h -- the coarse half of relocalisation: the NDT score alone (no gradient, no Hessian) of one scan at a very
// large number of poses, the pick of the poses worth refining, and their lattice poses as initial guesses.
// Part of libndt_mi355x.so: included by ndt_mi355x.hip inside its anonymous namespace, behind ndt_point.hip.h (one
// translation unit; the order of the includes matters).  Not a standalone header.

// ------------------------------------------------------------------------------------------
// the pose lattice (ndt_pose_lattice): index = (k * ny + j) * nx + i, yaw-major, x fastest
// ------------------------------------------------------------------------------------------

struct Lattice {
  double x0, y0, yaw0, step_x, step_y, step_yaw;
  int nx, ny, nyaw;
};

// ndt_lattice_pose on the device: one rounded multiply and one rounded add per component, never contracted into an fma
// (hipcc contracts a * b + c by default; the host's definition does not).
__device__ __forceinline__ void lattice_pose(const Lattice &L, unsigned long long idx, double p[3]) {
  const unsigned nx = (unsigned)L.nx, ny = (unsigned)L.ny;
  const unsigned long long row = idx / nx;
  const unsigned i = (unsigned)(idx - row * nx);
  const unsigned k = (unsigned)(row / ny), j = (unsigned)(row - (unsigned long long)k * ny);
  p[0] = __dadd_rn(L.x0, __dmul_rn((double)i, L.step_x));
  p[1] = __dadd_rn(L.y0, __dmul_rn((double)j, L.step_y));
  p[2] = __dadd_rn(L.yaw0, __dmul_rn((double)k, L.step_yaw));
}

// ------------------------------------------------------------------------------------------
// the score sweep
// ------------------------------------------------------------------------------------------

constexpr int kScoreBlock = 256;                     // four waves, a pose each
constexpr int kScoreWaves = kScoreBlock / 64;
constexpr int kScoreTile = 16;                       // consecutive poses a workgroup takes at a time (four per wave)
constexpr int kScoreStagePts = 8000;                 // scans up to this many points are staged in LDS (8 B per point: 62.5 KiB,
                                                     // so that a CU's 160 KiB still holds two workgroups and their exp tables)

// One source point at one pose, the score alone: the pairs eval_point forms on its global path (global_pairs) -- float32
// transform in the map's order, 3 x 3 neighbourhood, radius test on the float32 centroids -- and accumulate_pair's e for each,
// in ascending neighbour order, added to S.se.  The other five sums of S are never read: the compiler drops them and what feeds only them.
template <bool SSE, bool INCL, bool CHK>
__device__ __forceinline__ void score_point(const MapView &M, const double *__restrict__ etab, const Tf32 &T, float x, float y,
                                            PointAcc &S, unsigned &pairs) {
  float xt, yt;
  tf_apply_t<SSE>(T, x, y, xt, yt);
  global_pairs<INCL, CHK>(M, etab, xt, yt, (int)voxel_coord(xt, M.inv_leaf) - M.min_bx, (int)voxel_coord(yt, M.inv_leaf) - M.min_by, S, pairs);
}

// Score and pair count of one scan at P poses: poses[3 p .. 3 p + 3), or (poses == nullptr) the poses of lattice L.
// Persistent workgroups over tiles of kScoreTile consecutive poses; wave w of the workgroup takes poses w, w + 4, ... of the
// tile, so the four poses in flight are neighbours in the list -- in a lattice: same yaw, neighbouring x -- and read the same
// centroid and record lines.
// The order of summation is fixed by the pose alone: lane l adds the e of points l, l + 64, ... in point order, a point's
// pairs in ascending neighbour order, into one accumulator; wave_sum's tree adds the 64 lanes.  Nothing depends on the
// tile, the workgroup, the grid size, P or the other poses.
template <bool SSE, bool INCL, bool CHK>
__global__ void __launch_bounds__(kScoreBlock)
ndt_score_kernel(MapView M, int libm_f32, const float *__restrict__ scan, size_t stride, int n, int staged,
                 const double *__restrict__ poses, Lattice L, unsigned long long P, double *__restrict__ score,
                 unsigned *__restrict__ pairs_out) {
  extern __shared__ float2 s_scan[];                 // n points when staged
  __shared__ double etab[64];
  if (threadIdx.x < 64) etab[threadIdx.x] = c_exp2_tab[threadIdx.x];
  if (staged)
    for (int i = threadIdx.x; i < n; i += kScoreBlock) s_scan[i] = load_pt(scan, stride, (size_t)i);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long tiles = (P + kScoreTile - 1) / kScoreTile;
  for (unsigned long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    for (int r = 0; r < kScoreTile / kScoreWaves; ++r) {
      const unsigned long long pi = t * kScoreTile + (unsigned)(r * kScoreWaves + wave);   // (wave-uniform)
      if (pi >= P) break;
      double p[3];
      if (poses) { p[0] = gld_d(poses + 3 * pi); p[1] = gld_d(poses + 3 * pi + 1); p[2] = gld_d(poses + 3 * pi + 2); }
      else lattice_pose(L, pi, p);
      PointAcc S = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      unsigned np = 0;
      // a pose with a non-finite component scores nothing (decided before any sin or cos)
      if ((fabs(p[0]) <= DBL_MAX) & (fabs(p[1]) <= DBL_MAX) & (fabs(p[2]) <= DBL_MAX)) {
        const Tf32 T = tf_from_p(p, libm_f32);
        if (staged) {
          for (int i = lane; i < n; i += 64) { const float2 pt = s_scan[i]; score_point<SSE, INCL, CHK>(M, etab, T, pt.x, pt.y, S, np); }
        } else {
          for (int i = lane; i < n; i += 64) { const float2 pt = load_pt(scan, stride, (size_t)i); score_point<SSE, INCL, CHK>(M, etab, T, pt.x, pt.y, S, np); }
        }
      }
      const double tot = wave_sum(S.se);
      np = wave_sum(np);
      if (lane == 0) {
        score[pi] = -M.d1 * tot;
        if (pairs_out) pairs_out[pi] = np;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// the candidate pick (ndt_lattice_select_dev)
// ------------------------------------------------------------------------------------------
// The result is defined by a strict total order on the eligible poses -- larger score first, equal scores by lower index --
// so any method gives the same list.  Two kernels: every run of kSelTile poses is reduced to the sorted list of its eligible
// poses (lattice_rank_kernel); one workgroup then merges the lists' heads top_k times (lattice_merge_kernel).

constexpr int kSelTile = 1024;                       // poses per list = threads per workgroup

__device__ __forceinline__ bool sel_beats(double sa, unsigned long long ia, double sb, unsigned long long ib) {
  return sa > sb || (sa == sb && ia < ib);
}

// Eligibility of pose idx: pairs > 0 and (local_max) no lattice neighbour beats it -- score > every neighbour of lower index,
// score >= every neighbour of higher index; neighbours outside the lattice do not exist, the yaw does not wrap.
__device__ __forceinline__ bool sel_eligible(const Lattice &L, const double *__restrict__ score, const unsigned *__restrict__ pairs,
                                             unsigned long long idx, int local_max, double s) {
  if (pairs[idx] == 0u) return false;
  if (!local_max) return true;
  const unsigned nx = (unsigned)L.nx, ny = (unsigned)L.ny, nk = (unsigned)L.nyaw;
  const unsigned long long row = idx / nx;
  const int i = (int)(idx - row * nx);
  const int k = (int)(row / ny), j = (int)(row - (unsigned long long)k * ny);
  bool ok = true;
  for (int dk = -1; dk <= 1; ++dk) {
    if ((unsigned)(k + dk) >= nk) continue;
    for (int dj = -1; dj <= 1; ++dj) {
      if ((unsigned)(j + dj) >= ny) continue;
      for (int di = -1; di <= 1; ++di) {
        if ((unsigned)(i + di) >= nx || (dk == 0 && dj == 0 && di == 0)) continue;
        const long long d = ((long long)dk * ny + dj) * (long long)nx + di;
        const double sn = gld_d(score + (idx + d));
        ok &= d < 0 ? (s > sn) : (s >= sn);
      }
    }
  }
  return ok;
}

// List t = the eligible poses of [t kSelTile, (t + 1) kSelTile), best first, as 16-bit offsets into the run: cnt[t] of them at
// sorted[t kSelTile ..]; head[t] = 0.  The eligible poses are gathered in LDS (in any order), each then counts those that beat
// it: its place.
__global__ void __launch_bounds__(kSelTile)
lattice_rank_kernel(Lattice L, unsigned long long P, const double *__restrict__ score, const unsigned *__restrict__ pairs,
                    int local_max, unsigned short *__restrict__ sorted, unsigned *__restrict__ cnt, unsigned *__restrict__ head) {
  __shared__ double es[kSelTile];
  __shared__ unsigned short ei[kSelTile];
  __shared__ unsigned m_sh;
  const unsigned long long tiles = (P + kSelTile - 1) / kSelTile;
  for (unsigned long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    if (threadIdx.x == 0) m_sh = 0u;
    __syncthreads();
    const unsigned long long idx = t * kSelTile + threadIdx.x;
    if (idx < P) {
      const double s = gld_d(score + idx);
      if (sel_eligible(L, score, pairs, idx, local_max, s)) {
        const unsigned at = atomicAdd(&m_sh, 1u);
        es[at] = s; ei[at] = (unsigned short)threadIdx.x;
      }
    }
    __syncthreads();
    const unsigned m = m_sh;
    if (threadIdx.x < m) {
      const double s = es[threadIdx.x]; const unsigned short id = ei[threadIdx.x];
      unsigned rank = 0;
      for (unsigned q = 0; q < m; ++q) rank += sel_beats(es[q], ei[q], s, id) ? 1u : 0u;
      sorted[t * kSelTile + rank] = id;
    }
    if (threadIdx.x == 0) { cnt[t] = m; head[t] = 0u; }
    __syncthreads();
  }
}

// The best head among the lists a thread owns (lists tid, tid + kSelTile, ...): its score and pose index, or index ~0.
__device__ __forceinline__ void sel_best_head(unsigned long long tiles, const double *__restrict__ score,
                                              const unsigned short *__restrict__ sorted, const unsigned *__restrict__ cnt,
                                              const unsigned *head, double &bs, unsigned long long &bi) {
  bs = 0.0; bi = ~0ull;
  for (unsigned long long t = threadIdx.x; t < tiles; t += kSelTile) {
    const unsigned h = head[t];
    if (h >= cnt[t]) continue;
    const unsigned long long idx = t * kSelTile + sorted[t * kSelTile + h];
    const double s = gld_d(score + idx);
    if (bi == ~0ull || sel_beats(s, idx, bs, bi)) { bs = s; bi = idx; }
  }
}

// One workgroup: top_k rounds of "the best of all heads", each thread keeping the best head of its own lists and looking
// again only after one of them was taken.  cand[0 .. *n_cand) in descending score, ties to the lower index.
__global__ void __launch_bounds__(kSelTile)
lattice_merge_kernel(unsigned long long P, const double *__restrict__ score, const unsigned short *__restrict__ sorted,
                     const unsigned *__restrict__ cnt, unsigned *head, int top_k, unsigned long long *__restrict__ cand,
                     int *__restrict__ n_cand) {
  __shared__ double ws[kSelTile / 64];
  __shared__ unsigned long long wi[kSelTile / 64];
  __shared__ unsigned long long win_sh;
  const unsigned long long tiles = (P + kSelTile - 1) / kSelTile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double bs; unsigned long long bi;
  sel_best_head(tiles, score, sorted, cnt, head, bs, bi);
  int r = 0;
  for (; r < top_k; ++r) {
    double s = bs; unsigned long long i = bi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double s2 = __shfl_down(s, o); const unsigned long long i2 = __shfl_down(i, o);
      if (i2 != ~0ull && (i == ~0ull || sel_beats(s2, i2, s, i))) { s = s2; i = i2; }
    }
    if (lane == 0) { ws[wave] = s; wi[wave] = i; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < kSelTile / 64; ++w)
        if (wi[w] != ~0ull && (i == ~0ull || sel_beats(ws[w], wi[w], s, i))) { s = ws[w]; i = wi[w]; }
      win_sh = i;
      if (i != ~0ull) cand[r] = i;
    }
    __syncthreads();
    const unsigned long long win = win_sh;
    if (win == ~0ull) break;                          // (uniform) no eligible pose left
    if (win == bi) {                                  // mine: the list moves on
      head[win / kSelTile] += 1u;
      sel_best_head(tiles, score, sorted, cnt, head, bs, bi);
    }
  }
  if (threadIdx.x == 0) *n_cand = r;
}

// The candidates' lattice poses as initial guesses (cap x 3 doubles) and their scores; entries from *n_cand on are zeroed.
__global__ void __launch_bounds__(256)
lattice_cand_kernel(Lattice L, const unsigned long long *__restrict__ cand, const int *__restrict__ n_cand, int cap,
                    const double *__restrict__ score, double *__restrict__ inits, double *__restrict__ cand_score) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cap) return;
  double p[3] = {0.0, 0.0, 0.0}, s = 0.0;
  if (c < *n_cand) { lattice_pose(L, cand[c], p); s = score[cand[c]]; }
  inits[3 * c] = p[0]; inits[3 * c + 1] = p[1]; inits[3 * c + 2] = p[2];
  cand_score[c] = s;
}
