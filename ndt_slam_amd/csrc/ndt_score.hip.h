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

// ------------------------------------------------------------------------------------------
// many jobs in one launch (ndt_score_lattice_multi_dev, ndt_lattice_select_multi_dev)
// ------------------------------------------------------------------------------------------
// A job is one (map, scan, lattice).  Its volume lies at vol_off of the call's score / pairs arrays.

struct ScoreJob {                                    // a row of the sweep's table
  MapView M;
  Lattice L;
  unsigned long long P, vol_off;                     // poses of the lattice; where its volume starts
  int scan;                                          // points [offsets[scan], offsets[scan + 1]) of the call's scans
};

// ndt_score_kernel for a table of jobs.  A unit is a tile of kScoreTile consecutive poses of one job; job j owns the units
// [tile0[j], tile0[j + 1]), every job at least one.  A workgroup takes a contiguous range of the units: it finds the job of its
// first unit by search in tile0, goes on to the next job when a unit lies behind its job's last, and stages a scan only then.
// A pose's sums are formed as ndt_score_kernel forms them -- wave w of the workgroup on poses w, w + 4, ... of the tile, lane l
// on points l, l + 64, ... -- so they depend on the map, the scan and the pose alone.  A scan is staged when it has at most
// stage_pts points (the call's dynamic LDS; 0: none is); an empty scan gives score 0 (-d1 * 0.0) and pairs 0 at every pose.
template <bool SSE, bool INCL, bool CHK>
__global__ void __launch_bounds__(kScoreBlock)
ndt_score_multi_kernel(const ScoreJob *__restrict__ jobs, const unsigned long long *__restrict__ tile0, int n_jobs, int libm_f32,
                       const float2 *__restrict__ scans, const unsigned long long *__restrict__ offsets, unsigned stage_pts,
                       double *__restrict__ score, unsigned *__restrict__ pairs_out) {
  extern __shared__ float2 s_scan[];                 // stage_pts points
  __shared__ double etab[64];
  if (threadIdx.x < 64) etab[threadIdx.x] = c_exp2_tab[threadIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long units = tile0[n_jobs];
  const unsigned long long per = units / gridDim.x, rem = units % gridDim.x;
  const unsigned long long u0 = blockIdx.x * per + (blockIdx.x < rem ? blockIdx.x : rem), u1 = u0 + per + (blockIdx.x < rem ? 1u : 0u);
  if (u0 >= u1) return;                              // (uniform)
  int j = 0;                                         // the last job whose first unit is not behind u0
  for (int hi = n_jobs - 1; j < hi;) { const int mid = (j + hi + 1) >> 1; if (tile0[mid] <= u0) j = mid; else hi = mid - 1; }
  j = __builtin_amdgcn_readfirstlane(j) - 1;         // (entered below)
  MapView M; Lattice L;
  unsigned long long P = 0, vol = 0, t_first = 0, t_end = 0;
  const float2 *scan = nullptr; unsigned n = 0; bool staged = false;
  for (unsigned long long u = u0; u < u1; ++u) {
    if (u >= t_end) {                                // (uniform) the next job
      ++j;
      M = jobs[j].M; L = jobs[j].L; P = jobs[j].P; vol = jobs[j].vol_off;
      t_first = tile0[j]; t_end = tile0[j + 1];
      const unsigned long long o0 = offsets[jobs[j].scan], o1 = offsets[jobs[j].scan + 1];
      scan = scans + o0; n = (unsigned)(o1 - o0);
      staged = n <= stage_pts;
      __syncthreads();                               // every wave has left the previous job's points
      if (staged)
        for (unsigned i = threadIdx.x; i < n; i += kScoreBlock) s_scan[i] = gld_f2(scan + i);
      __syncthreads();
    }
    const unsigned long long t = u - t_first;
    for (int r = 0; r < kScoreTile / kScoreWaves; ++r) {
      const unsigned long long pi = t * kScoreTile + (unsigned)(r * kScoreWaves + wave);   // (wave-uniform)
      if (pi >= P) break;
      double p[3];
      lattice_pose(L, pi, p);
      PointAcc S = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      unsigned np = 0;
      // a pose that overflowed to a non-finite component scores nothing (ndt_score_kernel's test)
      if ((fabs(p[0]) <= DBL_MAX) & (fabs(p[1]) <= DBL_MAX) & (fabs(p[2]) <= DBL_MAX)) {
        const Tf32 T = tf_from_p(p, libm_f32);
        if (staged) {
          for (unsigned i = lane; i < n; i += 64) { const float2 pt = s_scan[i]; score_point<SSE, INCL, CHK>(M, etab, T, pt.x, pt.y, S, np); }
        } else {
          for (unsigned i = lane; i < n; i += 64) { const float2 pt = gld_f2(scan + i); score_point<SSE, INCL, CHK>(M, etab, T, pt.x, pt.y, S, np); }
        }
      }
      const double tot = wave_sum(S.se);
      np = wave_sum(np);
      if (lane == 0) {
        score[vol + pi] = -M.d1 * tot;
        if (pairs_out) pairs_out[vol + pi] = np;
      }
    }
  }
}

// The pick of every job in one launch: workgroup j on job j's volume.  Every thread keeps the top_k best eligible poses among
// its own (idx = tid, tid + kPickBlock, ...: ascending, so an equal score never displaces an earlier one) as a sorted list in
// LDS, slot q of thread t at [q kPickBlock + t]; the workgroup then takes the best of the lists' heads top_k times, as
// lattice_merge_kernel does.  sel_eligible / sel_beats: the strict total order makes the result ndt_lattice_select_dev's.
constexpr int kPickBlock = 256;
constexpr int kPickMaxK = 16;                        // 256 lists x 16 x (8 + 4) B = 48 KiB of LDS
constexpr unsigned kPickMaxPoses = 1u << 24;

struct PickJob { Lattice L; unsigned long long P, vol_off; };

__global__ void __launch_bounds__(kPickBlock)
lattice_pick_multi_kernel(const PickJob *__restrict__ jobs, const double *__restrict__ score, const unsigned *__restrict__ pairs,
                          int top_k, int local_max, unsigned long long *__restrict__ cand, int *__restrict__ n_cand) {
  extern __shared__ double pk_s[];                   // top_k x kPickBlock scores, then as many pose indices
  unsigned *pk_i = reinterpret_cast<unsigned *>(pk_s + (size_t)top_k * kPickBlock);
  __shared__ double ws[kPickBlock / 64];
  __shared__ unsigned wi[kPickBlock / 64];
  __shared__ unsigned win_sh;
  const PickJob J = jobs[blockIdx.x];
  const double *sc = score + J.vol_off; const unsigned *pr = pairs + J.vol_off;
  const unsigned P = (unsigned)J.P, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  int m = 0;                                         // length of my list
  for (unsigned idx = tid; idx < P; idx += kPickBlock) {
    const double s = gld_d(sc + idx);
    if (!sel_eligible(J.L, sc, pr, idx, local_max, s)) continue;
    if (m == top_k && !sel_beats(s, idx, pk_s[(top_k - 1) * kPickBlock + tid], pk_i[(top_k - 1) * kPickBlock + tid])) continue;
    int at = m < top_k ? m++ : top_k - 1;
    for (; at > 0 && sel_beats(s, idx, pk_s[(at - 1) * kPickBlock + tid], pk_i[(at - 1) * kPickBlock + tid]); --at) {
      pk_s[at * kPickBlock + tid] = pk_s[(at - 1) * kPickBlock + tid]; pk_i[at * kPickBlock + tid] = pk_i[(at - 1) * kPickBlock + tid];
    }
    pk_s[at * kPickBlock + tid] = s; pk_i[at * kPickBlock + tid] = idx;
  }
  constexpr unsigned kNone = ~0u;                    // (P <= 2^24: no pose has this index)
  int h = 0, r = 0;
  for (; r < top_k; ++r) {
    double s = h < m ? pk_s[h * kPickBlock + tid] : 0.0; unsigned i = h < m ? pk_i[h * kPickBlock + tid] : kNone;
    const unsigned mine = i;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double s2 = __shfl_down(s, o); const unsigned i2 = __shfl_down(i, o);
      if (i2 != kNone && (i == kNone || sel_beats(s2, i2, s, i))) { s = s2; i = i2; }
    }
    if (lane == 0) { ws[wave] = s; wi[wave] = i; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < kPickBlock / 64; ++w)
        if (wi[w] != kNone && (i == kNone || sel_beats(ws[w], wi[w], s, i))) { s = ws[w]; i = wi[w]; }
      win_sh = i;
      if (i != kNone) cand[(size_t)blockIdx.x * top_k + r] = i;
    }
    __syncthreads();
    const unsigned win = win_sh;
    if (win == kNone) break;                         // (uniform) no eligible pose left
    if (win == mine) ++h;
    __syncthreads();                                 // (win_sh, ws, wi are rewritten in the next round)
  }
  if (tid == 0) n_cand[blockIdx.x] = r;
}
