// Device-resident lockstep sessions (ndt_sessions_*): the state of S independent SLAM sessions and the
// step that advances all of them -- ScanMatcher::matchScan + growMap (src/ScanMatcher.cpp:4-116), PointCloudMap's
// addPose / addPoints / makeLocalMap (src/PointCloudMap.cpp:44-134) as FrontEnd::process drives them (src/FrontEnd.cpp) --
// without a scan, a cloud or a map leaving the device.  Included at the end of ndt_mi355x.hip: the step is made of the
// launches of the batched entry points (resampler, pre-filter, prediction, multi-map match, fusion, local-map assembly
// kernels, target filter, batched map build) on the session set's own resident arrays, plus five small kernels of its own:
//   session_select_kernel     per session: the odometry pose (first scan), the fused pose (matched) or nothing; carries
//                             last_pose / last_cov / prev_odo forward and writes the step record
//   scan_to_map_dst_kernel    growMap's transform, scan b to its own destination (the session's scan store)
//   session_units_kernel      the 256-point units of every newest triple's middle scan, from one job per session
//   session_plan_kernel       per session: the cloud's length and offset, the append of the new survivors to the cached
//                             prefix, and the gather table of prefix ++ survivors ++ newest scan
//   seg_copy_kernel           every move of a step (carried-over scans, closed clouds, gathers): a table of (src, dst, n)
// and two for ndt_sessions_correct:
//   repose_rows_kernel        every stored scan and closed cloud of the corrected sessions moved in place from its old pose
//                             to its new one: a table of (points, n, old pose, new pose), repose_point's arithmetic
//   session_refill_kernel     per corrected session: the prefix length and its refill from the recomputed cloud (a segment
//                             for seg_copy_kernel), and the session's row of last_pose
// and two for ndt_sessions_remake_closed:
//   remake_scans_kernel       every archived scan a closed submap of the named sessions held, into the map frame at the pose
//                             the trajectory holds now: a table of (archive range, pose, destination), scan_to_map_kernel's
//                             arithmetic
//   remake_plan_kernel        per named session: the all-or-nothing status over its submaps, its new local map's place in the
//                             target arena, and the moves into the arenas as segments for seg_copy_kernel

namespace {

struct SsCopy { const float2 *src; float2 *dst; unsigned long long n; };
struct SsMove { float2 *p; unsigned long long n; double old_pose[3], new_pose[3]; };
static_assert(sizeof(SsMove) == 64, "one 64-byte row per moved range");
// one corrected session: its index in the set, where its prefix lies, what of its cloud is the newest scan, its new last pose
struct SsFix { int ses, with_newest; unsigned long long newest_n; float2 *prefix; double pose[3]; };

// what the host knows of one session's cloud at a step: Submap::makeMap's branches (src/PointCloudMap.cpp:15-39) with the
// prefix = [scans[0] of a first submap] ++ the survivors of every triple computed so far (remove_moving), or the scans
// before the newest (otherwise)
struct SsPlan {
  float2 *prefix;                  // the session's prefix store
  const float2 *piece;             // what this step appends to the prefix: a whole scan (tri < 0) ...
  unsigned long long piece_n;
  int tri;                         // ... or the survivors of triple `tri`: points [tri_off[tri], tri_off[tri + 1]) of tri_xy
  int stepped;                     // 0: no cloud this step
  int reset;                       // 1: a new submap, the prefix starts empty
  int with_newest;                 // the newest scan closes the cloud
  const float2 *newest;
  unsigned long long newest_n;
};

// one archived scan of a remade session: where it lies in the archive, its pose as the trajectory holds it, where it goes
struct SsRescan { const double2 *src; float2 *dst; unsigned long long n; double pose[3]; };
static_assert(sizeof(SsRescan) == 48, "one 48-byte row per archived scan");
// one named session of a remake: its submaps [d0, d1) among the call's, its present views (old_t: the local map, its first
// n_prev points the newest closed cloud, `tail` points behind them; old_c: the cloud, c_n points) and where the cloud goes
struct SsRemake { int d0, d1, has_target, pad; const float2 *old_t, *old_c; float2 *new_c; unsigned long long n_prev, tail, c_n; };

constexpr int kSsNone = 0, kSsFirst = 1, kSsMatch = 2;      // a session's part in a step (SsMode)

__global__ void __launch_bounds__(256)
seg_copy_kernel(const SsCopy *__restrict__ tab, int n_seg) {
  for (int s = blockIdx.y; s < n_seg; s += gridDim.y) {
    const SsCopy c = tab[s];
    for (unsigned long long j = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; j < c.n;
         j += (unsigned long long)gridDim.x * blockDim.x)
      c.dst[j] = c.src[j];
  }
}

// seg_copy_kernel's shape over rows that are moved in place (ndt_repose_points' arithmetic: repose_point,
// ndt_posegraph.hip.h): blockIdx.y strides over the rows, blockIdx.x over a row's points; one sincos pair per row and block.
// A row whose poses are bit-equal keeps its bytes.
__global__ void __launch_bounds__(256)
repose_rows_kernel(const SsMove *__restrict__ tab, int n_rows) {
  for (int r = blockIdx.y; r < n_rows; r += gridDim.y) {
    const SsMove m = tab[r];
    if (!m.n) continue;
    const ReposeMove M = repose_move(m.old_pose, m.new_pose);
    if (M.same) continue;
    for (unsigned long long j = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; j < m.n;
         j += (unsigned long long)gridDim.x * blockDim.x) {
      const float2 v = m.p[j];
      m.p[j] = repose_point(M, v.x, v.y);
    }
  }
}

// One lane per corrected session c (row c of the recomputed clouds): the cached prefix is the cloud without its newest scan
// (Submap::makeMap's branches, SsStep::book), empty when the session's triples failed.
__global__ void __launch_bounds__(256)
session_refill_kernel(const SsFix *__restrict__ fix, int n, const unsigned long long *__restrict__ cloud_off,
                      const int *__restrict__ status, const float2 *__restrict__ arena, unsigned long long *__restrict__ plen,
                      double *__restrict__ last_pose, SsCopy *__restrict__ seg) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const SsFix F = fix[c];
  const unsigned long long len = cloud_off[c + 1] - cloud_off[c], nn = F.with_newest ? F.newest_n : 0ull;
  const unsigned long long pl = status[c] == NDT_OK && len >= nn ? len - nn : 0ull;
  plen[F.ses] = pl;
  for (int k = 0; k < 3; ++k) last_pose[3 * F.ses + k] = F.pose[k];
  seg[c] = SsCopy{arena + cloud_off[c], F.prefix, pl};
}

// scan_to_map_kernel (ndt_resample.hip.h) over rows of packed double2 with a destination each, in repose_rows_kernel's shape:
// blockIdx.y strides over the rows, blockIdx.x over a row's points; one cos / sin pair per row and block; 16 bytes in and 8 out
// per point.
__global__ void __launch_bounds__(256)
remake_scans_kernel(const SsRescan *__restrict__ tab, int n_rows) {
  for (int r = blockIdx.y; r < n_rows; r += gridDim.y) {
    const SsRescan R = tab[r];
    if (!R.n) continue;
    const double tx = R.pose[0], ty = R.pose[1], a = R.pose[2] * M_PI / 180;
    const double c = cos(a), sn = sin(a);
    const double r00 = c, r01 = -sn, r10 = sn, r11 = c;
    for (unsigned long long g = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; g < R.n;
         g += (unsigned long long)gridDim.x * blockDim.x) {
      const double2 p = R.src[g];
      const double lx = p.x, ly = p.y;
      const double x = r00 * lx + r01 * ly + tx;
      const double y = r10 * lx + r11 * ly + ty;
      R.dst[g] = make_float2((float)x, (float)y);
    }
  }
}

// One workgroup; session c of the call owns the remade submaps [d0, d1): their filtered clouds lie back to back at
// scr_t + scr_toff[d0 .. d1].  A session is remade when it has a submap and none of them failed (a failed one: NDT_E_ARG, and
// the session keeps every byte).  Its local map in the target arena: the newest closed cloud -- the remade one, else the one it
// has -- then the tail it has; a session without a local map gets none.  Writes the exclusive scan of those lengths, the status
// per session and three segments per session for seg_copy_kernel: the two parts of the local map and the cloud.
__global__ void __launch_bounds__(1024)
remake_plan_kernel(const SsRemake *__restrict__ rows, int C, const float2 *__restrict__ scr_t,
                   const unsigned long long *__restrict__ scr_toff, const int *__restrict__ scr_status, float2 *__restrict__ arena_t,
                   unsigned long long *__restrict__ ses_toff, int *__restrict__ ses_status, SsCopy *__restrict__ seg) {
  __shared__ unsigned long long sh[1024 / 64];
  SsRemake R;
  const float2 *psrc = nullptr;
  unsigned long long pn = 0ull, tail = 0ull;
  int st = NDT_OK;
  const unsigned long long total = block_excl_offsets<1024>(
      C, sh,
      [&](int i) {
        R = rows[i];
        st = NDT_OK;
        for (int d = R.d0; d < R.d1; ++d)
          if (scr_status[d] != NDT_OK) st = NDT_E_ARG;
        const bool remade = st == NDT_OK && R.d1 > R.d0;
        psrc = remade ? scr_t + scr_toff[R.d1 - 1] : R.old_t;
        pn = remade ? scr_toff[R.d1] - scr_toff[R.d1 - 1] : R.n_prev;
        tail = R.tail;
        if (!R.has_target) { pn = 0ull; tail = 0ull; }
        return pn + tail;
      },
      [&](int i, unsigned long long off, unsigned long long) {
        ses_toff[i] = off;
        ses_status[i] = st;
        seg[3 * i + 0] = SsCopy{pn ? psrc : nullptr, arena_t + off, pn};
        seg[3 * i + 1] = SsCopy{tail ? R.old_t + R.n_prev : nullptr, arena_t + off + pn, tail};
        seg[3 * i + 2] = SsCopy{R.old_c, R.new_c, R.has_target ? R.c_n : 0ull};
      });
  if (threadIdx.x == 0) ses_toff[C] = total;
}

// One lane per session.  mode: kSsNone / kSsFirst / kSsMatch; rs_status: the resampler's (NDT_E_ARG: a non-finite coordinate).
__global__ void __launch_bounds__(256)
session_select_kernel(const int *__restrict__ mode, const int *__restrict__ rs_status, const double *__restrict__ odo_cur,
                      const ndt_result *__restrict__ res, const double *__restrict__ fused, const double *__restrict__ cov,
                      const int *__restrict__ successful, int S, double *__restrict__ last_pose,
                      double *__restrict__ last_cov, double *__restrict__ prev_odo, ndt_session_step *__restrict__ rec) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= S) return;
  ndt_session_step r;
  for (int i = 0; i < 3; ++i) r.pose[i] = 0.0;
  for (int i = 0; i < 9; ++i) r.cov[i] = 0.0;
  r.cost = 0.0; r.stepped = 0; r.matched = 0; r.successful = 0; r.status = NDT_OK; r.submap = 0; r.split = 0;
  const int m = mode[b];
  if (m != kSsNone && rs_status[b] != NDT_OK) r.status = NDT_E_ARG;
  else if (m == kSsFirst) {
    for (int i = 0; i < 3; ++i) r.pose[i] = odo_cur[3 * b + i];
    r.stepped = 1; r.successful = 1;
  } else if (m == kSsMatch) {
    const ndt_result q = res[b];
    for (int i = 0; i < 3; ++i) r.pose[i] = fused[3 * b + i];
    for (int i = 0; i < 9; ++i) r.cov[i] = cov[9 * b + i];
    r.cost = (q.status == NDT_OK && q.converged) ? q.fitness : 10000000.0;
    r.stepped = 1; r.matched = 1; r.successful = successful[b];
  }
  if (r.stepped) {
    for (int i = 0; i < 3; ++i) { last_pose[3 * b + i] = r.pose[i]; prev_odo[3 * b + i] = odo_cur[3 * b + i]; }
    for (int i = 0; i < 9; ++i) last_cov[9 * b + i] = r.cov[i];
  }
  rec[b] = r;
}

// scan_to_map_kernel (ndt_resample.hip.h) with a destination per scan: dst[b] == nullptr: scan b is not transformed
__global__ void __launch_bounds__(256)
scan_to_map_dst_kernel(const double *__restrict__ xy, size_t stride, const unsigned long long *__restrict__ offsets, int B,
                       const double *__restrict__ poses, float2 *const *__restrict__ dst) {
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    float2 *out = dst[b];
    const unsigned long long r0 = offsets[b], r1 = offsets[b + 1];
    if (!out || r0 >= r1) continue;
    const double tx = poses[3 * b], ty = poses[3 * b + 1], a = poses[3 * b + 2] * M_PI / 180;
    const double c = cos(a), sn = sin(a);
    const double r00 = c, r01 = -sn, r10 = sn, r11 = c;
    for (unsigned long long g = r0 + blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; g < r1;
         g += (unsigned long long)gridDim.x * blockDim.x) {
      const double *p = rs_point(xy, stride, g);
      const double lx = p[0], ly = p[1];
      const double x = r00 * lx + r01 * ly + tx;
      const double y = r10 * lx + r11 * ly + ty;
      out[g - r0] = make_float2((float)x, (float)y);
    }
  }
}

// the units of triple t's middle scan (MmUnit, ndt_localmap.hip.h): [subs[t].u0, subs[t].u1), job t, submap t
__global__ void __launch_bounds__(256)
session_units_kernel(const MmJob *__restrict__ jobs, const MmSub *__restrict__ subs, MmUnit *__restrict__ units) {
  const MmJob J = jobs[blockIdx.x];
  const MmSub U = subs[blockIdx.x];
  for (unsigned k = threadIdx.x; k < U.u1 - U.u0; k += blockDim.x) {
    const unsigned first = k * (unsigned)kMmUnit;
    MmUnit u;
    u.src = (const float *)((const char *)J.b + (size_t)first * J.sb);
    u.stride = J.sb;
    u.n = min((unsigned)kMmUnit, J.nb - first);
    u.job = (int)blockIdx.x;
    u.sub = blockIdx.x;
    units[U.u0 + k] = u;
  }
}

// One workgroup: cloud s = prefix s ++ piece s ++ newest scan s.  Writes the exclusive scan of the lengths to cloud_off,
// the status per session (NDT_E_ARG: its triple failed, the cloud is empty and the prefix is left as it was), the new
// prefix lengths, and four segments per session for seg_copy_kernel: the append of the piece to the prefix, and the three
// gathers into the arena.
__global__ void __launch_bounds__(1024)
session_plan_kernel(const SsPlan *__restrict__ plan, int S, const float2 *__restrict__ tri_xy,
                    const unsigned long long *__restrict__ tri_off, const int *__restrict__ tri_status,
                    unsigned long long *__restrict__ plen, float2 *__restrict__ arena,
                    unsigned long long *__restrict__ cloud_off, int *__restrict__ status, SsCopy *__restrict__ seg) {
  __shared__ unsigned long long sh[1024 / 64];
  // what the load of session i finds out, for its store
  SsPlan P;
  unsigned long long pl = 0ull, pn = 0ull, nn = 0ull;
  const float2 *piece = nullptr;
  int st = NDT_OK;
  bool live = false;
  const unsigned long long total = block_excl_offsets<1024>(
      S, sh,
      [&](int i) {
        unsigned long long len = 0ull;
        P = plan[i];
        pl = 0ull; pn = 0ull; nn = 0ull; piece = nullptr; st = NDT_OK;
        live = P.stepped != 0;
        if (live) {
          pl = P.reset ? 0ull : plen[i];
          piece = P.piece; pn = P.piece_n;
          if (P.tri >= 0) {
            if (tri_status[P.tri] != NDT_OK) st = NDT_E_ARG;
            piece = tri_xy + tri_off[P.tri];
            pn = tri_off[P.tri + 1] - tri_off[P.tri];
          }
          nn = P.with_newest ? P.newest_n : 0ull;
          if (st != NDT_OK) { pn = 0ull; nn = 0ull; len = 0ull; }
          else len = pl + pn + nn;
        }
        return len;
      },
      [&](int i, unsigned long long off, unsigned long long) {
        cloud_off[i] = off;
        status[i] = st;
        const bool ok = live && st == NDT_OK;
        seg[4 * i + 0] = SsCopy{piece, ok ? P.prefix + pl : nullptr, ok ? pn : 0ull};
        seg[4 * i + 1] = SsCopy{ok ? P.prefix : nullptr, arena + off, ok ? pl : 0ull};
        seg[4 * i + 2] = SsCopy{piece, arena + off + pl, ok ? pn : 0ull};
        seg[4 * i + 3] = SsCopy{ok ? P.newest : nullptr, arena + off + pl + pn, ok ? nn : 0ull};
        if (live) plen[i] = st == NDT_OK ? pl + pn : pl;
      });
  if (threadIdx.x == 0) cloud_off[S] = total;
}

}  // namespace

// ---- the host side ----

namespace {

// PointCloudMap's bookkeeping of one session (the logic of host/PointCloudMap.cpp addPose / addPoints) and where its
// resident arrays are
struct SsSession {
  // PointCloudMap
  int n_poses = 0;
  double atd = 0.0, last_tx = 0.0, last_ty = 0.0;
  double atdS = 0.0;                        // of the current submap
  bool first_submap = true;                 // cntS == 0
  int n_closed = 0;
  // the trajectory (ndt_sessions_trajectory / ndt_sessions_correct): every stepped scan's pose as its record gave it, and per
  // submap its first scan, per closed submap its last (cntS / cntE, src/PointCloudMap.cpp:72-90)
  std::vector<double> traj;                 // 3 x n_poses
  std::vector<int> sub_first{0}, sub_last;  // n_closed + 1, n_closed entries
  // the current submap's scans (map frame, float2), one behind the other in store[cur]; the other store takes the two
  // carried-over scans at a split
  DevBuf<float2> store[2];
  int cur = 0;
  std::vector<uint64_t> scan_off{0};        // n_scans + 1 entries
  DevBuf<float2> prefix;                    // the cached part of p_cloud
  uint64_t plen = 0;                        // its length as of the last step (read back at host wait 2)
  DevBuf<float2> closed;                    // every closed submap's p_cloud
  std::vector<uint64_t> closed_off{0};      // n_closed + 1 entries
  // the last step's results in the arenas: arena `buf`, p_cloud at [c_off, c_off + c_n) of the cloud arena, the local map at
  // [t_off, t_off + t_n) of the target arena, its first n_prev points the previous submap's cloud
  bool has_target = false;
  int buf = 0;
  uint64_t c_off = 0, c_n = 0, t_off = 0, t_n = 0, n_prev = 0;
  ndt_map *map = nullptr;
  // the scan archive (ndt_sessions_archive_enable): every booked scan as the resampler wrote it -- robot frame,
  // double2 -- one behind the other; scan k of it belongs to pose k of traj.  Never moved by a correction.
  DevBuf<double2> arch;
  std::vector<uint64_t> arch_off{0};        // n_poses + 1 entries
  // the loop searches (ndt_loops.hip.h): the map of the session's candidate of rank r, rebuilt by every search (rank 0: the one
  // ndt_sessions_find_loops keeps)
  ndt_map *loop_maps[NDT_LOOP_MAX_SUBMAPS] = {};
  bool started = false;
};

}  // namespace

struct ndt_sessions {
  ndt_ctx *ctx = nullptr;
  int S = 0;
  ndt_session_params prm{};
  bool dead = false;                        // a HIP failure inside a step: every later call returns NDT_E_HIP
  bool archive = false;                     // ndt_sessions_archive_enable: every booked scan is kept (SsSession::arch)
  std::vector<SsSession> ses;
  ndt_sessions_stats stats{};
  // resident per-session state
  DevBuf<double> last_pose, last_cov, prev_odo;      // S x 3, S x 9, S x 3
  DevBuf<unsigned long long> plen;                   // S
  // a step's arrays
  DevBuf<unsigned char> raw;                         // the raw scans' copy (host form)
  DevBuf<double> odo, motion, pred, init, fused, cov;
  DevBuf<double> rs64; DevBuf<float> rs32, src;      // resampled scans (double2 / float2), filtered source scans
  DevBuf<uint64_t> raw_off, rs_off, src_off;
  DevBuf<int> rs_status, mode, map_of, successful;
  DevBuf<ndt_result> res;
  DevBuf<ndt_session_step> rec;
  PinnedBuf<unsigned char> h_back;                   // read-backs
  StagedUpload<unsigned char> tab_a, tab_b, tab_c;   // the tables of the three phases of a step
  DevBuf<unsigned char> d_tab_a, d_tab_b, d_tab_c;
  DevBuf<unsigned char> mm;                          // newest triples: units, counts, keep bits, voxel sets, difference lists
  DevBuf<float2> tri_xy; DevBuf<uint64_t> tri_off; DevBuf<int> tri_status;
  DevBuf<float2> cloud[2], target[2];                // the arenas, in turn
  DevBuf<uint64_t> cloud_off, target_off;            // S + 1 each
  DevBuf<int> status;
  int cur = 0;                                       // arena of the most recent step
  // ndt_sessions_find_loops (ndt_loops.hip.h): its table and its scratch -- scans, volumes, candidates, guesses, records
  StagedUpload<unsigned char> lp_tab; DevBuf<unsigned char> d_lp_tab, lp;
  // ndt_sessions_remake_closed: the archived scans in the map frame, the remade clouds and their filtered forms, one range per
  // closed submap of the named sessions
  DevBuf<float2> rm_scan, rm_cloud, rm_target;
  DevBuf<uint64_t> rm_coff, rm_toff, rm_ses_toff;
  DevBuf<int> rm_status, rm_ses_status;
};

namespace {

#define SS_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

// at least `need` elements with the first `keep` preserved: a growth doubles, copies on the device on the context's stream
// and frees the old block behind that copy
template <typename T>
int ss_grow(ndt_ctx *ctx, DevBuf<T> &b, size_t need, size_t keep) {
  if (b.p && need <= b.cap()) return NDT_OK;
  DevBuf<T> nb;
  SS_TRY(nb.alloc(ctx, std::max(need * 2, (size_t)1024) * sizeof(T)));
  if (keep && b.p) {
    HIP_TRY(ctx, hipMemcpyAsync(nb.p, b.p, keep * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  b = std::move(nb);
  return NDT_OK;
}

// One read-back into the set's h_back and its host wait: add() registers n elements at a device address (the array's number),
// wait() lays the registered arrays out, queues their copies, waits and counts the wait and the bytes it copied; at(k) is array
// k's host copy, good until the set's next read-back.
struct SsBack {
  ndt_sessions *s;
  struct Part { const void *src; size_t bytes, off; };
  std::vector<Part> parts; Regions R;
  template <typename T> size_t add(const T *src, size_t n) { parts.push_back(Part{src, n * sizeof(T), R.take(n * sizeof(T))}); return parts.size() - 1; }
  template <typename T> const T *at(size_t k) const { return (const T *)(s->h_back.p + parts[k].off); }
  int reserve() { return s->h_back.ensure(s->ctx, R.end); }
  int wait(ndt_sessions_stats &stats) {
    ndt_ctx *ctx = s->ctx;
    SS_TRY(reserve());
    for (const Part &p : parts) {
      HIP_TRY(ctx, hipMemcpyAsync(s->h_back.p + p.off, p.src, p.bytes, hipMemcpyDeviceToHost, ctx->stream));
      stats.d2h_bytes += p.bytes;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    stats.host_waits++;
    return NDT_OK;
  }
};

int ss_check_params(ndt_ctx *ctx, const ndt_session_params &p) {
  size_t cap = 0;
  if (!(p.leaf > 0)) return fail(ctx, NDT_E_ARG, "ndt_sessions_create: leaf <= 0");
  if (!(p.match.resolution > 0)) return fail(ctx, NDT_E_ARG, "ndt_sessions_create: match.resolution <= 0");
  if (!(p.fuse.del_time > 0)) return fail(ctx, NDT_E_ARG, "ndt_sessions_create: fuse.del_time <= 0");
  if (ndt_resample_capacity(1, p.space, p.space_thre, &cap))
    return fail(ctx, NDT_E_ARG, "ndt_sessions_create: space / space_thre refused (negative, non-finite, or space == 0 < space_thre)");
  if (p.remove_moving && (!(p.resol > 0.0) || !std::isfinite(p.resol) || !std::isfinite(p.thre_neighbor)))
    return fail(ctx, NDT_E_ARG, "ndt_sessions_create: remove_moving needs a positive finite resol (and a finite thre_neighbor)");
  if (!std::isfinite(p.sep_thre)) return fail(ctx, NDT_E_ARG, "ndt_sessions_create: sep_thre is not finite");
  return NDT_OK;
}

unsigned ss_gx(size_t total, int B) { return (unsigned)std::min<size_t>(64, (total / (size_t)std::max(B, 1) + 255) / 256 + 1); }

// ---- what the end of a step, of a correction and of a remake share: the commit ----

// The commit of a call that fills the arenas `cur` and counts in `stats`: who is named (the sessions the call computes; everybody
// else keeps its views across the call -- a step it did not take part in, a correction that does not name it -- and is carried),
// the call's own moves that ride in the carried ranges' table, which new local maps want an NDT map, and the tail.  The call itself
// states the named sessions' new views.
struct SsCommit {
  ndt_sessions *s; const int cur = s->cur ^ 1; ndt_sessions_stats stats{};
  std::vector<unsigned char> named = std::vector<unsigned char>((size_t)s->S, 0);
  std::vector<SsCopy> moves;
  std::vector<const float *> bxy; std::vector<size_t> bn, bentry; std::vector<int> bwho;
  // the points everybody else carries into this call's arenas: part of the arenas' sizes
  void carried(size_t *cloud, size_t *target) const {
    for (int i = 0; i < s->S; ++i) {
      const SsSession &Q = s->ses[(size_t)i];
      if (!named[(size_t)i] && Q.has_target && Q.buf != cur) { *cloud += Q.c_n; *target += Q.t_n; }
    }
  }
  // Named session i behind the call's wait, range `entry` of the read-back offsets: its views and its wish for a map, or (ok
  // false: a triple of its cloud spans more than 2^30 voxels) no cloud and no local map; the map stays as it is.
  void view(int i, size_t entry, bool ok, const uint64_t *coff, const uint64_t *toff, uint64_t n_prev) {
    SsSession &Q = s->ses[(size_t)i];
    Q.buf = cur; Q.has_target = ok; Q.c_n = Q.t_n = Q.n_prev = 0;
    if (!ok) return;
    Q.c_off = coff[entry]; Q.c_n = coff[entry + 1] - coff[entry];
    Q.t_off = toff[entry]; Q.t_n = toff[entry + 1] - toff[entry];
    Q.n_prev = n_prev;
    wants_map(i, entry);
  }
  // session i's new local map (its view is set) wants an NDT map; a refused build's code goes to the caller's status `entry`
  void wants_map(int i, size_t entry) {
    const SsSession &Q = s->ses[(size_t)i];
    if (!Q.t_n) return;
    bxy.push_back((const float *)(s->target[cur].p + Q.t_off)); bn.push_back((size_t)Q.t_n); bwho.push_back(i); bentry.push_back(entry);
  }
  // The tail.  (1) Everybody else's ranges move behind the call's own, which end at (c_end, t_end): with the call's moves table C, the
  // same size at every call (two carried ranges per session at most), and the copies; `cur` is the set's from here.  (2) The NDT maps
  // of the new local maps, rebuilt in place in one batched build; a host wait: the bounding boxes (without a map to build, the stream).
  // A build refused for one session (NDT_E_GRID: its local map spans more than 2^28 cells) costs that session alone: status(entry) takes
  // the build's code, its map stays exactly as it was (none stays none), every other map is built all the same.  (3) The set's stats.
  template <typename Status> int finish(uint64_t c_end, uint64_t t_end, Status &&status) {
    ndt_ctx *ctx = s->ctx; hipStream_t st = ctx->stream;
    for (int i = 0; i < s->S; ++i) {
      SsSession &Q = s->ses[(size_t)i];
      if (named[(size_t)i] || !Q.has_target || Q.buf == cur) continue;
      if (Q.c_n) moves.push_back(SsCopy{s->cloud[Q.buf].p + Q.c_off, s->cloud[cur].p + c_end, Q.c_n});
      if (Q.t_n) moves.push_back(SsCopy{s->target[Q.buf].p + Q.t_off, s->target[cur].p + t_end, Q.t_n});
      Q.c_off = c_end; c_end += Q.c_n; Q.t_off = t_end; t_end += Q.t_n; Q.buf = cur;
    }
    const size_t c_bytes = 2 * (size_t)s->S * sizeof(SsCopy), nb = bwho.size();
    SS_TRY(s->tab_c.reserve(ctx, c_bytes)); SS_TRY(s->d_tab_c.ensure(ctx, c_bytes));
    memset(s->tab_c.h.p, 0, c_bytes);
    if (!moves.empty()) memcpy(s->tab_c.h.p, moves.data(), moves.size() * sizeof(SsCopy));
    HIP_TRY(ctx, s->tab_c.upload(s->d_tab_c.p, 0, c_bytes, st));
    stats.h2d_bytes += c_bytes;
    if (!moves.empty())
      seg_copy_kernel<<<dim3(16, (unsigned)std::min<size_t>(moves.size(), 65535)), 256, 0, st>>>((const SsCopy *)s->d_tab_c.p, (int)moves.size());
    HIP_TRY(ctx, hipGetLastError());
    s->cur = cur;
    if (nb) {
      std::vector<ndt_params> bp(nb, s->prm.match);
      std::vector<ndt_map *> maps;
      std::vector<int> code(nb, NDT_OK);
      for (int i : bwho) maps.push_back(s->ses[(size_t)i].map);
      SS_TRY(check_build_batch(ctx, bxy.data(), bn.data(), sizeof(float2), (int)nb, bp.data(), maps.data(), "ndt_map_build_batch_dev"));
      SS_TRY(build_batch(ctx, bxy.data(), bn.data(), sizeof(float2), (int)nb, bp.data(), maps.data(), "ndt_map_build_batch_dev", code.data()));
      for (size_t k = 0; k < nb; ++k)
        if (code[k] == NDT_OK) s->ses[(size_t)bwho[k]].map = maps[k]; else status(bentry[k]) = code[k];
    } else {
      HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    stats.host_waits++; stats.d2h_bytes += nb * 16 * sizeof(unsigned);
    s->stats = stats;
    return NDT_OK;
  }
};

// queue_local_map_batch over `subs` on the set's stream, in a call frame of its own (the assembly's and the filter's scratch are
// the context's); its upload and its triples go to the stats.
int ss_local_maps(ndt_sessions *s, const std::vector<ndt_submap_desc> &subs, float2 *cloud, DevBuf<uint64_t> &cloud_off, float2 *target,
                  DevBuf<uint64_t> &target_off, DevBuf<int> &status, ndt_sessions_stats &stats) {
  ndt_ctx *ctx = s->ctx;
  size_t up = 0, nt = 0;
  CallFrame fr(ctx);
  SS_TRY(fr.open(ctx->stream));
  SS_TRY(queue_local_map_batch(ctx, ctx->stream, subs.data(), (int)subs.size(), sizeof(float2), s->prm.leaf, (float *)cloud, cloud_off.p,
                               (float *)target, target_off.p, status.p, &up, &nt));
  SS_TRY(fr.close());
  stats.h2d_bytes += up; stats.triples_run = (int)nt;
  return NDT_OK;
}

// What passes between the parts of one step (DESIGN.md 4.10's list), in the order the parts fill it.
struct SsStep {
  // the call; raw_dev / odo_dev: the device form (then raw_host / odo_host are NULL)
  ndt_sessions *s; const double *raw_host, *raw_dev; size_t stride; const uint64_t *raw_offsets; const double *odo_host, *odo_dev;
  const unsigned char *active; ndt_session_step *out;
  ndt_ctx *ctx = s->ctx; hipStream_t st = ctx->stream; const int S = s->S; const ndt_session_params &P = s->prm;
  SsCommit commit{s}; ndt_sessions_stats &stats = commit.stats; const int cur = commit.cur;      // (named: who stepped; cur: this step's arenas)
  std::vector<int> mode, map_of; std::vector<const ndt_map *> maps;      // who steps
  std::vector<uint64_t> rs_off;                    // the front part: the resampled scans' offsets
  // the bookkeeping: table B's contents, the newest triples (unit_room: their units) and the submaps of one triple each
  std::vector<SsCopy> moves;                       // carried-over scans and closed clouds, the scan's copy into the archive
  std::vector<float2 *> dst; std::vector<SsPlan> plan; std::vector<PfPrev> prevs;
  MmPlan tri; std::vector<MmSub> subs; float cut = 0.f;      // (cut: rn_cutoff of the set's thre_neighbor)
  size_t cap_cloud = 0, total_prev = 0, carry_cloud = 0, carry_target = 0;
  SsBack back{s}; size_t b_toff = 0, b_coff = 0, b_plen = 0, b_stat = 0;      // the part behind it: wait 2's read-back
  bool who_steps(); int front(); int bookkeeping(); int behind(); int close(); int run();      // the parts, in this order, and the step
  int book(int i, size_t n_new);
};

// ---- who steps; false: nobody (the records and the stats are written) ----
bool SsStep::who_steps() {
  mode.assign((size_t)S, kSsNone); map_of.assign((size_t)S, -1);
  int n_active = 0;
  for (int i = 0; i < S; ++i) {
    if (active && !active[i]) continue;
    ++n_active;
    SsSession &Q = s->ses[(size_t)i];
    if (!Q.started) mode[(size_t)i] = kSsFirst;
    else {
      mode[(size_t)i] = kSsMatch;
      if (Q.map) { map_of[(size_t)i] = (int)maps.size(); maps.push_back(Q.map); }
    }
  }
  if (n_active) return true;
  for (int i = 0; i < S; ++i) { memset(&out[i], 0, sizeof(out[i])); out[i].submap = s->ses[(size_t)i].n_closed; }
  s->stats = stats;
  return false;
}

// ---- the front part: upload, resample -> pre-filter -> predict -> match -> fuse -> select, host wait 1 ----
int SsStep::front() {
  const size_t N = (size_t)(raw_offsets[S] - raw_offsets[0]), S1 = (size_t)S + 1;
  size_t cap_rs = 0;
  if (ndt_resample_capacity(std::max<size_t>(N, 1), P.space, P.space_thre, &cap_rs))
    return fail(ctx, NDT_E_ARG, "ndt_sessions_step: the resampled scans' capacity overflows");
  SS_TRY(s->raw_off.ensure(ctx, S1)); SS_TRY(s->rs_off.ensure(ctx, S1)); SS_TRY(s->src_off.ensure(ctx, S1));
  SS_TRY(s->rs64.ensure(ctx, 2 * cap_rs)); SS_TRY(s->rs32.ensure(ctx, 2 * cap_rs)); SS_TRY(s->src.ensure(ctx, 2 * cap_rs));
  // table A: raw offsets (relative) | mode | map_of | odometry (host form)
  Regions A;
  const size_t a_off = A.take(S1 * 8), a_mode = A.take((size_t)S * 4), a_mapof = A.take((size_t)S * 4),
               a_odo = A.take(odo_host ? (size_t)S * 24 : 0);
  SS_TRY(s->tab_a.reserve(ctx, A.end)); SS_TRY(s->d_tab_a.ensure(ctx, A.end));
  unsigned char *h = s->tab_a.h.p;
  rel_offsets(raw_offsets, (size_t)S, A.at<uint64_t>(h, a_off));
  memcpy(h + a_mode, mode.data(), (size_t)S * 4); memcpy(h + a_mapof, map_of.data(), (size_t)S * 4);
  if (odo_host) memcpy(h + a_odo, odo_host, (size_t)S * 24);
  HIP_TRY(ctx, s->tab_a.upload(s->d_tab_a.p, 0, A.end, st));
  stats.h2d_bytes += A.end;
  const unsigned long long *d_raw_off = (const unsigned long long *)(s->d_tab_a.p + a_off);
  const int *d_mode = (const int *)(s->d_tab_a.p + a_mode), *d_map_of = (const int *)(s->d_tab_a.p + a_mapof);
  const double *d_odo = odo_host ? (const double *)(s->d_tab_a.p + a_odo) : odo_dev;
  const double *d_raw = raw_dev ? (const double *)((const char *)raw_dev + (size_t)raw_offsets[0] * stride) : nullptr;
  if (raw_host && N) {
    SS_TRY(s->raw.ensure(ctx, N * stride));
    HIP_TRY(ctx, hipMemcpyAsync(s->raw.p, (const char *)raw_host + (size_t)raw_offsets[0] * stride, N * stride, hipMemcpyHostToDevice, st));
    stats.h2d_bytes += N * stride;
    d_raw = (const double *)s->raw.p;
  }
  if (N) {
    SS_TRY(ndt_resample_batch_dev(ctx, d_raw, stride, (const uint64_t *)d_raw_off, S, N, P.space, P.space_thre, s->rs64.p, s->rs32.p,
                                  s->rs_off.p, s->rs_status.p, st));
    SS_TRY(ndt_prefilter_batch_dev(ctx, s->rs32.p, sizeof(float2), s->rs_off.p, S, cap_rs, P.leaf, s->src.p, s->src_off.p, st));
  } else {
    HIP_TRY(ctx, hipMemsetAsync(s->rs_off.p, 0, S1 * 8, st)); HIP_TRY(ctx, hipMemsetAsync(s->src_off.p, 0, S1 * 8, st));
    HIP_TRY(ctx, hipMemsetAsync(s->rs_status.p, 0, (size_t)S * 4, st));
  }
  SS_TRY(ndt_predict_batch_dev(ctx, d_odo, s->prev_odo.p, s->last_pose.p, S, s->motion.p, s->pred.p, s->init.p, st));
  if (!maps.empty() && N) {
    SS_TRY(ndt_align_batch_multi_dev(ctx, maps.data(), (int)maps.size(), d_map_of, s->src.p, s->src_off.p, S, cap_rs, 0, s->init.p,
                                     s->res.p, st));
  } else {
    HIP_TRY(ctx, hipMemsetAsync(s->res.p, 0, (size_t)S * sizeof(ndt_result), st));      // (status 0, converged 0: the sentinel cost)
  }
  SS_TRY(ndt_fuse_batch_dev(ctx, s->res.p, s->pred.p, s->motion.p, s->last_pose.p, s->last_cov.p, S, &P.fuse, s->fused.p, s->cov.p,
                            s->successful.p, st));
  session_select_kernel<<<(S + 255) / 256, 256, 0, st>>>(d_mode, s->rs_status.p, d_odo, s->res.p, s->fused.p, s->cov.p, s->successful.p,
                                                         S, s->last_pose.p, s->last_cov.p, s->prev_odo.p, s->rec.p);
  HIP_TRY(ctx, hipGetLastError());
  // host wait 1: the resampled counts and the records
  SsBack B{s};
  const size_t b_rs = B.add(s->rs_off.p, S1), b_rec = B.add(s->rec.p, (size_t)S);
  SS_TRY(B.wait(stats));
  rs_off.assign(B.at<uint64_t>(b_rs), B.at<uint64_t>(b_rs) + S1);
  memcpy(out, B.at<ndt_session_step>(b_rec), (size_t)S * sizeof(ndt_session_step));
  return NDT_OK;
}

// The bookkeeping of session i, which stepped with record out[i] and a new scan of n_new points: addPose, the split, where
// the scan lands (PointCloudMap::addPose / addPoints) and Submap::makeMap's branches in their incremental form -- the
// whole-submap form is submap_pieces (ndt_mi355x.hip).  Gives the session's row of table B (plan, dst, prevs), its moves and
// its newest triple, if any.  The stores may move when they grow: every pointer is taken after the session's own growth,
// and no other session touches them.
int SsStep::book(int i, size_t n_new) {
  SsSession &Q = s->ses[(size_t)i]; SsPlan &L = plan[(size_t)i];
  stats.sessions_stepped++;
  const double tx = out[i].pose[0], ty = out[i].pose[1];
  if (Q.n_poses) Q.atd += std::sqrt((tx - Q.last_tx) * (tx - Q.last_tx) + (ty - Q.last_ty) * (ty - Q.last_ty));
  else Q.atd = 0.0;
  Q.n_poses++; Q.last_tx = tx; Q.last_ty = ty; Q.started = true;
  Q.traj.insert(Q.traj.end(), out[i].pose, out[i].pose + 3);
  if (s->archive) {
    // the step's rs64 range of the session, byte for byte: a move of 2 n_new float2
    SS_TRY(ss_grow(ctx, Q.arch, (size_t)Q.arch_off.back() + n_new, (size_t)Q.arch_off.back()));
    if (n_new)
      moves.push_back(SsCopy{(const float2 *)(s->rs64.p + 2 * (size_t)rs_off[(size_t)i]), (float2 *)(Q.arch.p + Q.arch_off.back()), 2ull * n_new});
    Q.arch_off.push_back(Q.arch_off.back() + n_new);
  }
  if (Q.atd - Q.atdS >= P.sep_thre) {
    Q.sub_last.push_back(Q.n_poses - 2); Q.sub_first.push_back(Q.n_poses - 1);      // cntE = size - 2, the new cntS = size - 1
    // the current submap closes (src/PointCloudMap.cpp:72-90): its cloud becomes the filtered part of the last local map
    const uint64_t n_tail = Q.has_target ? Q.t_n - Q.n_prev : 0;
    SS_TRY(ss_grow(ctx, Q.closed, (size_t)(Q.closed_off.back() + n_tail), (size_t)Q.closed_off.back()));
    if (n_tail) moves.push_back(SsCopy{s->target[Q.buf].p + Q.t_off + Q.n_prev, Q.closed.p + Q.closed_off.back(), n_tail});
    Q.closed_off.push_back(Q.closed_off.back() + n_tail);
    Q.n_closed++;
    Q.atdS = Q.atd; Q.first_submap = Q.n_poses - 1 == 0;
    const size_t ns = Q.scan_off.size() - 1;
    const int other = Q.cur ^ 1;
    std::vector<uint64_t> noff{0};
    if (ns >= 2) {
      const uint64_t a = Q.scan_off[ns - 2], n2 = Q.scan_off[ns] - a;
      SS_TRY(ss_grow(ctx, Q.store[other], (size_t)n2 + n_new, 0));
      if (n2) moves.push_back(SsCopy{Q.store[Q.cur].p + a, Q.store[other].p, n2});
      noff.push_back(Q.scan_off[ns - 1] - a); noff.push_back(n2);
    }
    Q.scan_off = noff; Q.cur = other;
    L.reset = 1; Q.plen = 0;
    out[i].split = 1;
  }
  out[i].submap = Q.n_closed;
  SS_TRY(ss_grow(ctx, Q.store[Q.cur], (size_t)Q.scan_off.back() + n_new, (size_t)Q.scan_off.back()));
  float2 *base = Q.store[Q.cur].p;
  dst[(size_t)i] = base + Q.scan_off.back();
  Q.scan_off.push_back(Q.scan_off.back() + n_new);
  // Submap::makeMap's branches
  const size_t n = Q.scan_off.size() - 1;
  auto scan_p = [&](size_t k) { return base + Q.scan_off[k]; };
  auto scan_n = [&](size_t k) { return (size_t)(Q.scan_off[k + 1] - Q.scan_off[k]); };
  L.stepped = 1;
  L.newest = scan_p(n - 1); L.newest_n = scan_n(n - 1);
  size_t piece_room = 0;
  if (P.remove_moving) {
    L.with_newest = 1;
    if (n == 1 && Q.first_submap) { L.piece = scan_p(0); L.piece_n = scan_n(0); piece_room = scan_n(0); }
    else if (n >= 3 && scan_n(n - 2)) {      // the newest triple (an empty middle scan contributes nothing)
      const size_t n0 = scan_n(n - 3), n1 = scan_n(n - 1), nb = scan_n(n - 2);
      if (n0 > ((size_t)1 << 29) || n1 > ((size_t)1 << 29) || nb > ((size_t)1 << 29))
        return fail(ctx, NDT_E_ARG, "ndt_sessions_step: session " + std::to_string(i) + ": a scan above 2^29 points");
      L.tri = (int)tri.jobs.size();
      tri.add((const float *)scan_p(n - 3), (const float *)scan_p(n - 1), (const float *)scan_p(n - 2), n0, n1, nb, P.resol, cut);
      const size_t u0 = tri.unit_room;
      tri.unit_room += (nb + kMmUnit - 1) / kMmUnit;
      subs.push_back(MmSub{(unsigned)u0, (unsigned)tri.unit_room});      // (the triple's own submap: its units)
      piece_room = nb;
    }
  } else {
    L.with_newest = Q.first_submap || n - 1 >= 2;
    if (n >= 2 && (Q.first_submap || n - 2 >= 2)) { L.piece = scan_p(n - 2); L.piece_n = scan_n(n - 2); piece_room = scan_n(n - 2); }
  }
  SS_TRY(ss_grow(ctx, Q.prefix, (size_t)Q.plen + piece_room, (size_t)Q.plen));
  L.prefix = Q.prefix.p;
  cap_cloud += (size_t)Q.plen + piece_room + (L.with_newest ? (size_t)L.newest_n : 0);
  if (Q.n_closed >= 1) {
    const uint64_t a = Q.closed_off[(size_t)Q.n_closed - 1], np = Q.closed_off[(size_t)Q.n_closed] - a;
    prevs[(size_t)i] = PfPrev{np ? (const float *)(Q.closed.p + a) : nullptr, np};
    total_prev += (size_t)np;
  }
  return NDT_OK;
}

// ---- the host bookkeeping: table B's rows, the moves and the newest triples of the sessions that stepped (book) ----
int SsStep::bookkeeping() {
  dst.assign((size_t)S, nullptr); prevs.assign((size_t)S, PfPrev{nullptr, 0ull});
  plan.assign((size_t)S, SsPlan{nullptr, nullptr, 0ull, -1, 0, 0, 0, nullptr, 0ull});
  tri.sa = tri.sb = sizeof(float2);
  cut = P.remove_moving ? rn_cutoff(P.thre_neighbor) : 0.f;
  for (int i = 0; i < S; ++i) {
    const SsSession &Q = s->ses[(size_t)i];
    out[i].submap = Q.n_closed;
    commit.named[(size_t)i] = out[i].stepped != 0;
    if (out[i].stepped) SS_TRY(book(i, (size_t)(rs_off[(size_t)i + 1] - rs_off[(size_t)i])));
  }
  commit.carried(&carry_cloud, &carry_target);
  stats.triples_run = (int)tri.jobs.size();
  return NDT_OK;
}

// ---- the part behind it: growMap's transform, the moves, the newest triples, the clouds, the targets, host wait 2 ----
int SsStep::behind() {
  const size_t S1 = (size_t)S + 1, nt = tri.jobs.size();
  SS_TRY(s->cloud[cur].ensure(ctx, cap_cloud + carry_cloud + 64)); SS_TRY(s->tri_xy.ensure(ctx, tri.list_pts + 64));
  SS_TRY(s->target[cur].ensure(ctx, cap_cloud + total_prev + carry_target + 64));
  // device scratch of the triples: the units (made on the device), then the assembly chain's own
  Regions M;
  const size_t m_units = M.take(tri.unit_room * sizeof(MmUnit));
  const MmScratch X(M, tri);
  SS_TRY(s->mm.ensure(ctx, M.end));
  char *dm = (char *)s->mm.p;
  mm_bind(tri.jobs.data(), nt, dm, X);
  // table B, the same size at every step: dst | plan | prevs | jobs | subs | moves (3 per session at most, 4 with the archive); the segments
  // of session_plan_kernel lie behind it on the device
  Regions B;
  const size_t o_dst = B.take((size_t)S * 8), o_plan = B.take((size_t)S * sizeof(SsPlan)), o_prev = B.take((size_t)S * sizeof(PfPrev)),
               o_jobs = B.take((size_t)S * sizeof(MmJob)), o_subs = B.take((size_t)S * sizeof(MmSub)),
               o_moves = B.take((s->archive ? 4 : 3) * (size_t)S * sizeof(SsCopy)), o_seg = B.take(4 * (size_t)S * sizeof(SsCopy)), b_bytes = o_seg;
  SS_TRY(s->tab_b.reserve(ctx, b_bytes)); SS_TRY(s->d_tab_b.ensure(ctx, B.end));
  unsigned char *h = s->tab_b.h.p;
  memset(h, 0, b_bytes);
  memcpy(h + o_dst, dst.data(), (size_t)S * 8);
  memcpy(h + o_plan, plan.data(), (size_t)S * sizeof(SsPlan));
  memcpy(h + o_prev, prevs.data(), (size_t)S * sizeof(PfPrev));
  if (nt) { memcpy(h + o_jobs, tri.jobs.data(), nt * sizeof(MmJob)); memcpy(h + o_subs, subs.data(), nt * sizeof(MmSub)); }
  if (!moves.empty()) memcpy(h + o_moves, moves.data(), moves.size() * sizeof(SsCopy));
  HIP_TRY(ctx, s->tab_b.upload(s->d_tab_b.p, 0, b_bytes, st));
  stats.h2d_bytes += b_bytes;
  unsigned char *db = s->d_tab_b.p;
  const size_t rs_total = (size_t)rs_off[(size_t)S];
  if (rs_total)
    scan_to_map_dst_kernel<<<dim3(ss_gx(rs_total, S), (unsigned)std::min(S, 65535)), 256, 0, st>>>(
        s->rs64.p, sizeof(double2), (const unsigned long long *)s->rs_off.p, S, s->last_pose.p, (float2 *const *)(db + o_dst));
  if (!moves.empty())
    seg_copy_kernel<<<dim3(16, (unsigned)std::min<size_t>(moves.size(), 65535)), 256, 0, st>>>((const SsCopy *)(db + o_moves), (int)moves.size());
  if (nt) {
    const MmJob *d_jobs = (const MmJob *)(db + o_jobs); const MmSub *d_subs = (const MmSub *)(db + o_subs);
    SS_TRY(s->tri_off.ensure(ctx, nt + 1)); SS_TRY(s->tri_status.ensure(ctx, nt));
    session_units_kernel<<<(unsigned)nt, 256, 0, st>>>(d_jobs, d_subs, (MmUnit *)(dm + m_units));
    SS_TRY(mm_queue(ctx, d_jobs, (const MmUnit *)(dm + m_units), d_subs, dm, X, nt, s->tri_xy.p,
                    (unsigned long long *)s->tri_off.p, s->tri_status.p, nullptr, st));
  }
  session_plan_kernel<<<1, 1024, 0, st>>>((const SsPlan *)(db + o_plan), S, s->tri_xy.p, (const unsigned long long *)s->tri_off.p,
                                          s->tri_status.p, s->plen.p, s->cloud[cur].p, (unsigned long long *)s->cloud_off.p,
                                          s->status.p, (SsCopy *)(db + o_seg));
  seg_copy_kernel<<<dim3(ss_gx(cap_cloud, S), (unsigned)std::min(4 * S, 65535)), 256, 0, st>>>((const SsCopy *)(db + o_seg), 4 * S);
  HIP_TRY(ctx, hipGetLastError());
  {
    CallFrame fr(ctx);                            // (the filter's scratch is the context's)
    SS_TRY(fr.open(st));
    SS_TRY(pf_run<true>(ctx, (const float *)s->cloud[cur].p, sizeof(float2), s->cloud_off.p, S, std::max<size_t>(cap_cloud, 1), P.leaf,
                        (float *)s->target[cur].p, s->target_off.p, (const PfPrev *)(db + o_prev), sizeof(float2), total_prev,
                        s->status.p, st));
    SS_TRY(fr.close());
  }
  // host wait 2: the target and cloud offsets, the prefix lengths, the status
  b_toff = back.add(s->target_off.p, S1); b_coff = back.add(s->cloud_off.p, S1); b_plen = back.add(s->plen.p, (size_t)S);
  b_stat = back.add(s->status.p, (size_t)S);
  return back.wait(stats);
}

// ---- the close: the new views of who stepped; the commit (table C; the NDT maps, host wait 3: a refused build's code goes into the record) ----
int SsStep::close() {
  const uint64_t *toff = back.at<uint64_t>(b_toff), *coff = back.at<uint64_t>(b_coff), *pl = back.at<uint64_t>(b_plen);
  const int *stt = back.at<int>(b_stat);
  for (int i = 0; i < S; ++i) {
    if (!out[i].stepped) continue;      // (it keeps its views and its last local map: they move to this step's arenas)
    s->ses[(size_t)i].plen = pl[i];
    if (stt[i] != NDT_OK) out[i].status = NDT_E_ARG;
    commit.view(i, (size_t)i, stt[i] == NDT_OK, coff, toff, prevs[(size_t)i].n);
  }
  return commit.finish(coff[S], toff[S], [&](size_t i) -> int & { return out[i].status; });
}

// The step: DESIGN.md 4.10's list.  Every return with a HIP error leaves the set dead (the caller marks it).
int SsStep::run() {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!who_steps()) return NDT_OK;
  SS_TRY(front());
  SS_TRY(bookkeeping());
  SS_TRY(behind());
  return close();
}

// ---- ndt_sessions_correct: PointCloudMap::remakeMaps for the sessions which[0 .. n_corr) ----

// The scan whose (old, new) pose pair moves submap m's closed cloud: the middle one of the submap's own scans [cntS, cntE].
// The current submap's cntE is the newest scan; a submap that closed without a scan of its own (cntE < cntS: the empty first
// submap of sep_thre <= 0) takes cntS.
int ss_anchor(const SsSession &Q, int m) {
  const int a = Q.sub_first[(size_t)m], e = m < Q.n_closed ? Q.sub_last[(size_t)m] : Q.n_poses - 1;
  return e > a ? a + (e - a) / 2 : a;
}

// The arguments have passed the entry point's refusals.  rows(): the rows of every stored scan and closed cloud moved in place, the
// current submaps as queue_local_map_batch takes them.  run(): the moves, the current submaps assembled again from the moved scans
// with the local maps behind them (every triple, as the composed chain computes them), the prefixes refilled from the clouds; wait
// 1: offsets and status; the corrected sessions' views, then SsCommit's tail (everybody else's ranges, the NDT maps; wait 2).
struct SsCorrect {
  ndt_sessions *s; const int *which; int n_corr; const double *const *new_poses; int *status_out;
  ndt_ctx *ctx = s->ctx; const ndt_session_params &P = s->prm; const size_t C = (size_t)n_corr;
  SsCommit commit{s}; ndt_sessions_stats &stats = commit.stats; const int cur = commit.cur;
  std::vector<SsMove> moved; std::vector<SsFix> fix; std::vector<ndt_submap_desc> subs;
  size_t cap_cloud = 0, total_prev = 0, most_pts = 0;
  int rows(); int run();
};

int SsCorrect::rows() {
  fix.resize(C); subs.resize(C);
  stats.sessions_stepped = n_corr;
  for (size_t c = 0; c < C; ++c) {
    SsSession &Q = s->ses[(size_t)which[c]];
    commit.named[(size_t)which[c]] = 1;
    const double *po = Q.traj.data(), *pn = new_poses[c];
    const size_t n = Q.scan_off.size() - 1, first = (size_t)Q.n_poses - n;
    auto row = [&](float2 *p, uint64_t cnt, size_t k) {
      moved.push_back(SsMove{p, cnt, {po[3 * k], po[3 * k + 1], po[3 * k + 2]}, {pn[3 * k], pn[3 * k + 1], pn[3 * k + 2]}});
      most_pts = std::max(most_pts, (size_t)cnt);
    };
    for (int m = 0; m < Q.n_closed; ++m)
      row(Q.closed.p + Q.closed_off[(size_t)m], Q.closed_off[(size_t)m + 1] - Q.closed_off[(size_t)m], (size_t)ss_anchor(Q, m));
    float2 *base = Q.store[Q.cur].p;
    for (size_t k = 0; k < n; ++k) row(base + Q.scan_off[k], Q.scan_off[k + 1] - Q.scan_off[k], first + k);
    ndt_submap_desc &D = subs[c];
    D.scans_xy = (const float *)base; D.offsets = Q.scan_off.data(); D.n_scans = (int)n;
    D.first_submap = Q.first_submap; D.newest = 1; D.remove_moving = P.remove_moving; D.resol = P.resol; D.thre_neighbor = P.thre_neighbor;
    D.prev_xy = nullptr; D.n_prev = 0;
    if (Q.n_closed >= 1) {
      const uint64_t a = Q.closed_off[(size_t)Q.n_closed - 1], np = Q.closed_off[(size_t)Q.n_closed] - a;
      if (np) { D.prev_xy = (const float *)(Q.closed.p + a); D.n_prev = (size_t)np; }
    }
    cap_cloud += submap_points(D); total_prev += D.n_prev;
    SS_TRY(ss_grow(ctx, Q.prefix, submap_points(D), 0));      // (refilled whole: nothing of it is kept)
    const int with_newest = P.remove_moving ? 1 : (Q.first_submap || n - 1 >= 2);
    const double *last = pn + 3 * ((size_t)Q.n_poses - 1);
    fix[c] = SsFix{which[c], with_newest, Q.scan_off[n] - Q.scan_off[n - 1], Q.prefix.p, {last[0], last[1], last[2]}};
  }
  return NDT_OK;
}

int SsCorrect::run() {
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  SS_TRY(rows());
  size_t carry_cloud = 0, carry_target = 0;
  commit.carried(&carry_cloud, &carry_target);
  SS_TRY(s->cloud[cur].ensure(ctx, cap_cloud + carry_cloud + 64));
  SS_TRY(s->target[cur].ensure(ctx, cap_cloud + total_prev + carry_target + 64));
  // table A: the rows | the fixes; the prefix segments of session_refill_kernel lie behind it on the device
  Regions A;
  const size_t o_rows = A.take(moved.size() * sizeof(SsMove)), o_fix = A.take(C * sizeof(SsFix)), a_bytes = A.end,
               o_seg = A.take(C * sizeof(SsCopy));
  SS_TRY(s->tab_a.reserve(ctx, a_bytes)); SS_TRY(s->d_tab_a.ensure(ctx, A.end));
  memcpy(s->tab_a.h.p + o_rows, moved.data(), moved.size() * sizeof(SsMove));
  memcpy(s->tab_a.h.p + o_fix, fix.data(), C * sizeof(SsFix));
  HIP_TRY(ctx, s->tab_a.upload(s->d_tab_a.p, 0, a_bytes, st));
  stats.h2d_bytes += a_bytes;
  unsigned char *da = s->d_tab_a.p;
  repose_rows_kernel<<<dim3((unsigned)std::min<size_t>(64, most_pts / 256 + 1), (unsigned)std::min<size_t>(moved.size(), 65535)), 256, 0, st>>>(
      (const SsMove *)(da + o_rows), (int)moved.size());
  HIP_TRY(ctx, hipGetLastError());
  SS_TRY(ss_local_maps(s, subs, s->cloud[cur].p, s->cloud_off, s->target[cur].p, s->target_off, s->status, stats));
  session_refill_kernel<<<(n_corr + 255) / 256, 256, 0, st>>>((const SsFix *)(da + o_fix), n_corr, (const unsigned long long *)s->cloud_off.p,
                                                             s->status.p, s->cloud[cur].p, s->plen.p, s->last_pose.p, (SsCopy *)(da + o_seg));
  seg_copy_kernel<<<dim3(ss_gx(cap_cloud, n_corr), (unsigned)std::min(n_corr, 65535)), 256, 0, st>>>((const SsCopy *)(da + o_seg), n_corr);
  HIP_TRY(ctx, hipGetLastError());
  // host wait 1: the cloud and target offsets, the status
  SsBack back{s};
  const size_t b_coff = back.add(s->cloud_off.p, C + 1), b_toff = back.add(s->target_off.p, C + 1), b_stat = back.add(s->status.p, C);
  SS_TRY(back.wait(stats));
  const uint64_t *coff = back.at<uint64_t>(b_coff), *toff = back.at<uint64_t>(b_toff);
  const int *stt = back.at<int>(b_stat);
  // the corrected sessions' host state and views; everybody else's ranges move to this call's arenas
  for (size_t c = 0; c < C; ++c) {
    SsSession &Q = s->ses[(size_t)which[c]];
    Q.traj.assign(new_poses[c], new_poses[c] + 3 * (size_t)Q.n_poses);
    Q.last_tx = fix[c].pose[0]; Q.last_ty = fix[c].pose[1];
    status_out[c] = stt[c];
    commit.view(which[c], c, stt[c] == NDT_OK, coff, toff, subs[c].n_prev);
    const uint64_t nn = fix[c].with_newest ? fix[c].newest_n : 0;      // (session_refill_kernel's rule; a failed cloud: an empty prefix)
    Q.plen = Q.c_n >= nn ? Q.c_n - nn : 0;
  }
  return commit.finish(coff[C], toff[C], [&](size_t c) -> int & { return status_out[c]; });
}

// ---- ndt_sessions_remake_closed: every closed submap's cloud again from the archive ----

// The archive range [first, first + count) of the scans submap m held when it closed, for every closed submap of Q
// (SsStep::book's split rule: the last two scans of the store that closed before it, when it held two, then its own).
void ss_closed_scan_ranges(const SsSession &Q, std::vector<int> *first, std::vector<int> *count) {
  first->assign((size_t)Q.n_closed, 0); count->assign((size_t)Q.n_closed, 0);
  int held = 0;
  for (int m = 0; m < Q.n_closed; ++m) {
    const int a = Q.sub_first[(size_t)m] - (m >= 1 && held >= 2 ? 2 : 0);
    held = Q.sub_last[(size_t)m] - a + 1;
    (*first)[(size_t)m] = a; (*count)[(size_t)m] = held;
  }
}

// The arguments have passed the entry point's refusals.  plan(): every closed submap of every named session as queue_local_map_batch
// takes it -- its scan list a slice of the archive's own offsets, the session's scans laid out in archive order; the arenas'
// sizes, a row per archived scan in use, a row per named session.  run(): the one table, remake_scans_kernel, the assembly
// over every submap, remake_plan_kernel; wait 1: the filtered clouds' offsets, the local maps' offsets, the status; the moves into
// the arenas (seg_copy_kernel), the closed blocks grown to what they need and their moves beside everybody else's ranges (SsCommit's
// tail; the NDT maps, wait 2).  Nothing is committed before wait 1: a session that failed keeps every byte.
struct SsRemakeCall {
  ndt_sessions *s; const int *which; int n_named; int *status_out;
  ndt_ctx *ctx = s->ctx; const ndt_session_params &P = s->prm; const size_t C = (size_t)n_named;
  SsCommit commit{s}; ndt_sessions_stats &stats = commit.stats; const int cur = commit.cur;
  std::vector<SsRescan> scans; std::vector<SsRemake> rows; std::vector<ndt_submap_desc> subs;
  std::vector<size_t> base;                            // where session c's scans start in rm_scan
  size_t scan_pts = 0, cap_cloud = 0, most_pts = 0, need_cloud = 0, need_target = 0, c_end = 0;
  int plan(); int run();
};

int SsRemakeCall::plan() {
  static const uint64_t no_scan[2] = {0, 0};
  stats.sessions_stepped = n_named;
  rows.resize(C); base.assign(C, 0);
  std::vector<int> first, count;
  for (size_t c = 0; c < C; ++c) {
    const SsSession &Q = s->ses[(size_t)which[c]];
    commit.named[(size_t)which[c]] = 1;
    rows[c].d0 = (int)subs.size();
    ss_closed_scan_ranges(Q, &first, &count);
    base[c] = scan_pts;
    if (Q.n_closed) scan_pts += (size_t)Q.arch_off[(size_t)(Q.sub_last[(size_t)Q.n_closed - 1] + 1)];
    for (int m = 0; m < Q.n_closed; ++m) {
      ndt_submap_desc D{};
      // (scans_xy: bound below, once rm_scan has its size; a submap that held no scan is one empty scan)
      D.offsets = count[(size_t)m] ? Q.arch_off.data() + first[(size_t)m] : no_scan;
      D.n_scans = std::max(count[(size_t)m], 1);
      D.first_submap = Q.sub_first[(size_t)m] == 0; D.newest = 1;
      D.remove_moving = P.remove_moving; D.resol = P.resol; D.thre_neighbor = P.thre_neighbor;
      D.prev_xy = nullptr; D.n_prev = 0;
      if (D.n_scans > (1 << 20))
        return fail(ctx, NDT_E_ARG, "ndt_sessions_remake_closed: session " + std::to_string(which[c]) + ": a submap of more than 2^20 scans");
      cap_cloud += submap_points(D);
      subs.push_back(D);
    }
    rows[c].d1 = (int)subs.size();
  }
  const size_t nd = subs.size();
  if (!cap_cloud) return NDT_OK;      // (nothing to compute)
  if (nd > (size_t)INT32_MAX / 4 || scan_pts > ((size_t)1 << 40))
    return fail(ctx, NDT_E_ARG, "ndt_sessions_remake_closed: more than 2^29 closed submaps or 2^40 archived points in one call");
  SS_TRY(s->rm_scan.ensure(ctx, scan_pts + 64)); SS_TRY(s->rm_cloud.ensure(ctx, cap_cloud + 64)); SS_TRY(s->rm_target.ensure(ctx, cap_cloud + 64));
  SS_TRY(s->rm_coff.ensure(ctx, nd + 1)); SS_TRY(s->rm_toff.ensure(ctx, nd + 1)); SS_TRY(s->rm_status.ensure(ctx, nd));
  SS_TRY(s->rm_ses_toff.ensure(ctx, C + 1)); SS_TRY(s->rm_ses_status.ensure(ctx, C));
  // the arenas: a named session's cloud as it is; its local map with the larger of the two newest closed clouds it may get
  size_t carry_cloud = 0, carry_target = 0;
  for (size_t c = 0; c < C; ++c) {
    const SsSession &Q = s->ses[(size_t)which[c]];
    if (!Q.has_target) continue;
    const size_t newest = rows[c].d1 > rows[c].d0 ? submap_points(subs[(size_t)rows[c].d1 - 1]) : 0;
    need_cloud += (size_t)Q.c_n; need_target += std::max(newest, (size_t)Q.n_prev) + (size_t)(Q.t_n - Q.n_prev);
  }
  commit.carried(&carry_cloud, &carry_target);
  SS_TRY(s->cloud[cur].ensure(ctx, need_cloud + carry_cloud + 64));
  SS_TRY(s->target[cur].ensure(ctx, need_target + carry_target + 64));
  for (size_t c = 0; c < C; ++c) {
    const SsSession &Q = s->ses[(size_t)which[c]];
    SsRemake &R = rows[c];
    for (int d = R.d0; d < R.d1; ++d) subs[(size_t)d].scans_xy = (const float *)(s->rm_scan.p + base[c]);
    if (Q.n_closed) {
      const int last = Q.sub_last[(size_t)Q.n_closed - 1];      // (-1: one closed submap, the empty first one of sep_thre <= 0)
      for (size_t k = 0; k < (size_t)(last + 1); ++k) {
        const uint64_t n = Q.arch_off[k + 1] - Q.arch_off[k];
        scans.push_back(SsRescan{Q.arch.p + Q.arch_off[k], s->rm_scan.p + base[c] + Q.arch_off[k], n,
                                 {Q.traj[3 * k], Q.traj[3 * k + 1], Q.traj[3 * k + 2]}});
        most_pts = std::max(most_pts, (size_t)n);
      }
    }
    R.has_target = Q.has_target; R.pad = 0;
    R.old_t = Q.has_target ? s->target[Q.buf].p + Q.t_off : nullptr; R.old_c = Q.has_target ? s->cloud[Q.buf].p + Q.c_off : nullptr;
    R.new_c = s->cloud[cur].p + c_end;
    R.n_prev = Q.has_target ? Q.n_prev : 0; R.tail = Q.has_target ? Q.t_n - Q.n_prev : 0; R.c_n = Q.has_target ? Q.c_n : 0;
    c_end += (size_t)R.c_n;
  }
  if (scans.size() > (size_t)INT32_MAX) return fail(ctx, NDT_E_ARG, "ndt_sessions_remake_closed: more than 2^31 - 1 archived scans in one call");
  return NDT_OK;
}

int SsRemakeCall::run() {
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  SS_TRY(plan());
  if (!cap_cloud) {
    // no named session has a closed submap that held a point: nothing to compute, nobody changes a byte, nothing is queued
    for (size_t c = 0; c < C; ++c) status_out[c] = NDT_OK;
    s->stats = stats;
    return NDT_OK;
  }
  // table A: the scans' rows | the sessions' rows; the segments of remake_plan_kernel lie behind it on the device
  Regions A;
  const size_t o_scans = A.take(scans.size() * sizeof(SsRescan)), o_rows = A.take(C * sizeof(SsRemake)), a_bytes = A.end,
               o_seg = A.take(3 * C * sizeof(SsCopy));
  SS_TRY(s->tab_a.reserve(ctx, a_bytes)); SS_TRY(s->d_tab_a.ensure(ctx, A.end));
  memcpy(s->tab_a.h.p + o_scans, scans.data(), scans.size() * sizeof(SsRescan));
  memcpy(s->tab_a.h.p + o_rows, rows.data(), C * sizeof(SsRemake));
  HIP_TRY(ctx, s->tab_a.upload(s->d_tab_a.p, 0, a_bytes, st));
  stats.h2d_bytes += a_bytes;
  unsigned char *da = s->d_tab_a.p;
  remake_scans_kernel<<<dim3((unsigned)std::min<size_t>(64, most_pts / 256 + 1), (unsigned)std::min<size_t>(scans.size(), 65535)), 256, 0, st>>>(
      (const SsRescan *)(da + o_scans), (int)scans.size());
  HIP_TRY(ctx, hipGetLastError());
  SS_TRY(ss_local_maps(s, subs, s->rm_cloud.p, s->rm_coff, s->rm_target.p, s->rm_toff, s->rm_status, stats));
  remake_plan_kernel<<<1, 1024, 0, st>>>((const SsRemake *)(da + o_rows), n_named, s->rm_target.p, (const unsigned long long *)s->rm_toff.p,
                                         s->rm_status.p, s->target[cur].p, (unsigned long long *)s->rm_ses_toff.p, s->rm_ses_status.p,
                                         (SsCopy *)(da + o_seg));
  HIP_TRY(ctx, hipGetLastError());
  // host wait 1: the filtered clouds' offsets, the local maps' offsets, the status
  SsBack back{s};
  const size_t b_doff = back.add(s->rm_toff.p, subs.size() + 1), b_toff = back.add(s->rm_ses_toff.p, C + 1), b_stat = back.add(s->rm_ses_status.p, C);
  SS_TRY(back.wait(stats));
  const uint64_t *doff = back.at<uint64_t>(b_doff), *toff = back.at<uint64_t>(b_toff);
  const int *stt = back.at<int>(b_stat);
  // the commit: the moves into the arenas, then the closed blocks (to their exact size) with everybody else's ranges
  seg_copy_kernel<<<dim3(ss_gx(need_cloud + need_target, 3 * n_named), (unsigned)std::min<size_t>(3 * C, 65535)), 256, 0, st>>>(
      (const SsCopy *)(da + o_seg), 3 * n_named);
  HIP_TRY(ctx, hipGetLastError());
  uint64_t c_at = 0;
  for (size_t c = 0; c < C; ++c) {
    SsSession &Q = s->ses[(size_t)which[c]];
    const SsRemake &W = rows[c];
    status_out[c] = stt[c];
    const bool remade = stt[c] == NDT_OK && W.d1 > W.d0;
    if (remade) {
      const uint64_t d0 = doff[W.d0], need = doff[W.d1] - d0;
      SS_TRY(ss_grow(ctx, Q.closed, (size_t)need, 0));      // (rewritten whole: nothing of it is kept)
      if (need) commit.moves.push_back(SsCopy{s->rm_target.p + d0, Q.closed.p, need});
      for (int m = 0; m <= Q.n_closed; ++m) Q.closed_off[(size_t)m] = doff[W.d0 + m] - d0;
    }
    Q.buf = cur;
    if (!Q.has_target) continue;
    Q.c_off = c_at; c_at += Q.c_n;
    Q.t_off = toff[c]; Q.t_n = toff[c + 1] - toff[c];
    if (remade) {
      Q.n_prev = doff[W.d1] - doff[W.d1 - 1];
      commit.wants_map(which[c], c);
    }
  }
  return commit.finish(c_end, toff[C], [&](size_t c) -> int & { return status_out[c]; });
}

#undef SS_TRY

}  // namespace
