// Loops between the sessions of a set (ndt_cross_gate, ndt_cross_gate_batch, ndt_sessions_cross_candidates,
// ndt_sessions_find_cross_loops): the cross gate -- every searcher against every closed submap of every other
// track -- as a host definition and as a device form that equals it to the bit, and the search of its candidates by
// LpSearch (ndt_loops.hip.h) with the candidate's cloud and anchor taken from the track.  Included behind ndt_loops.hip.h
// (one translation unit).  Two kernels of its own:
//   cross_dist_kernel    per (row, searcher): the smallest squared distance from the searcher's last pose to a pose of the row
//                        (a closed submap's scan range, staged in LDS), and the first scan that attains it
//   cross_pick_kernel    per searcher: its four rows of smallest (d2, row), by integer keys, merged through LDS in a fixed order
// d2 is formed by explicitly rounded operations (__dsub_rn, __dmul_rn, __dadd_rn) on the device and with contraction off on the
// host (the whole file is), so both round every subtraction, product and sum once.

namespace {

struct CgRow { unsigned long long off; unsigned n; int t; };      // a closed submap: its poses in the packed xy, how many (0: not eligible whoever asks), its track
struct CgSearch { double x, y; int own, pad; };                   // a searcher: its last position, its own track (-1: none)
struct CgPick { unsigned long long key; int row, k; };            // a pick: d2's bits (kCgNone: no pick), the row, the scan inside the row
constexpr unsigned long long kCgNone = ~0ull;                     // (no d2 has these bits: d2 is never NaN)
constexpr int kCgStage = 1024;                                    // poses of a row in LDS at a time: 16 KB per workgroup
constexpr int kCgBlock = 256;
constexpr uint64_t kCgMaxPairs = 1ull << 28;

// Workgroup (x, y): row x, the searchers y * 256 .. of every 256 * gridDim.y.  A thread is one searcher; every lane of a wave
// reads the same staged pose at a time (an LDS broadcast, no bank conflict).  key / near: [searcher * R + row].
__global__ void __launch_bounds__(kCgBlock)
cross_dist_kernel(const CgRow *__restrict__ rows, const double2 *__restrict__ xy, const CgSearch *__restrict__ se, int n_search, int R,
                  double r2, unsigned long long *__restrict__ key, int *__restrict__ near) {
  __shared__ double2 P[kCgStage];
  const int row = blockIdx.x;
  const CgRow r = rows[row];
  for (long long s0 = (long long)blockIdx.y * kCgBlock; s0 < n_search; s0 += (long long)gridDim.y * kCgBlock) {
    const long long i = s0 + threadIdx.x;
    const bool live = i < n_search;
    CgSearch s{0.0, 0.0, -1, 0};
    if (live) s = se[i];
    double best = __longlong_as_double(0x7ff0000000000000ll);      // (+inf: a first d2 of +inf keeps k = 0, as the host's start does)
    int bk = 0;
    for (unsigned base = 0; base < r.n; base += kCgStage) {
      const unsigned cnt = min((unsigned)kCgStage, r.n - base);
      __syncthreads();
      for (unsigned q = threadIdx.x; q < cnt; q += kCgBlock) P[q] = xy[r.off + base + q];
      __syncthreads();
      if (live)
        for (unsigned q = 0; q < cnt; ++q) {
          const double2 v = P[q];
          const double dx = __dsub_rn(s.x, v.x), dy = __dsub_rn(s.y, v.y);
          const double d = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
          if (d < best) { best = d; bk = (int)(base + q); }
        }
    }
    if (live) {
      const bool ok = r.n && r.t != s.own && best <= r2;
      key[(size_t)i * R + row] = ok ? (unsigned long long)__double_as_longlong(best) : kCgNone;
      near[(size_t)i * R + row] = bk;
    }
  }
}

// A sorted list of four (key, row), smallest first; an empty place is (kCgNone, INT_MAX).  put() keeps the four smallest of the
// list and the newcomer: four compare-exchanges, no indexed access (the list stays in registers).
struct CgBest {
  unsigned long long k0, k1, k2, k3; int r0, r1, r2, r3;
  __device__ static bool less(unsigned long long ka, int ra, unsigned long long kb, int rb) { return ka < kb || (ka == kb && ra < rb); }
  __device__ void put(unsigned long long k, int r) {
#define CG_CE(K, Rr) if (less(k, r, K, Rr)) { const unsigned long long tk = K; const int tr = Rr; K = k; Rr = r; k = tk; r = tr; }
    CG_CE(k0, r0) CG_CE(k1, r1) CG_CE(k2, r2) CG_CE(k3, r3)
#undef CG_CE
  }
};

// One workgroup per searcher.  Thread t walks the rows t, t + 256, ...; the 256 lists meet pairwise through LDS, thread t taking
// thread t + w's for w = 128, 64 .. 1: (key, row) is a total order (a row occurs once), so the four that remain are the four
// smallest whatever the order of the meetings -- which is fixed all the same.  Integer compares only.
__global__ void __launch_bounds__(kCgBlock)
cross_pick_kernel(const unsigned long long *__restrict__ key, const int *__restrict__ near, int R, CgPick *__restrict__ out) {
  __shared__ unsigned long long sk[4 * kCgBlock];
  __shared__ int sr[4 * kCgBlock];
  const size_t i = blockIdx.x;
  const int t = threadIdx.x;
  CgBest b{kCgNone, kCgNone, kCgNone, kCgNone, INT_MAX, INT_MAX, INT_MAX, INT_MAX};
  for (int row = t; row < R; row += kCgBlock) {
    const unsigned long long k = key[i * R + row];
    if (k != kCgNone) b.put(k, row);
  }
  sk[4 * t] = b.k0; sk[4 * t + 1] = b.k1; sk[4 * t + 2] = b.k2; sk[4 * t + 3] = b.k3;
  sr[4 * t] = b.r0; sr[4 * t + 1] = b.r1; sr[4 * t + 2] = b.r2; sr[4 * t + 3] = b.r3;
  __syncthreads();
  for (int w = kCgBlock / 2; w > 0; w >>= 1) {
    if (t < w)
      for (int q = 0; q < 4; ++q) {
        const unsigned long long k = sk[4 * (t + w) + q];
        if (k != kCgNone) b.put(k, sr[4 * (t + w) + q]);
      }
    __syncthreads();
    if (t < w) {
      sk[4 * t] = b.k0; sk[4 * t + 1] = b.k1; sk[4 * t + 2] = b.k2; sk[4 * t + 3] = b.k3;
      sr[4 * t] = b.r0; sr[4 * t + 1] = b.r1; sr[4 * t + 2] = b.r2; sr[4 * t + 3] = b.r3;
    }
    __syncthreads();
  }
  if (t < 4) {
    const unsigned long long k = sk[t];
    const int row = sr[t];
    out[4 * i + t] = CgPick{k, k != kCgNone ? row : -1, k != kCgNone ? near[i * R + row] : 0};
  }
}

#define CG_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

// The closed submaps of the tracks in ascending (t, m): the rows of the gate.
struct CgRowRef { int t, m; };
void cross_rows(const ndt_cross_track *tr, int n_tracks, std::vector<CgRowRef> *rows) {
  rows->clear();
  for (int t = 0; t < n_tracks; ++t)
    for (int m = 0; m <= tr[t].n_submaps - 2; ++m) rows->push_back(CgRowRef{t, m});
}

// A row's scan range as the rule reads it: [first, first + n), n = 0 for a row that nobody may pick (an empty range, an empty cloud).
void cross_range(const ndt_cross_track &T, int m, int *first, unsigned *n) {
  const int a = T.sub_first[m], e = T.sub_first[m + 1] - 1;
  *first = a;
  *n = (e < a || T.sub_offsets[m + 1] == T.sub_offsets[m]) ? 0u : (unsigned)(e - a + 1);
}

// The record of a pick (the rule's words, include/ndt_mi355x.h): both forms of the gate fill theirs here.
void cross_fill(ndt_cross_candidate *c, int session, int newest_scan, const ndt_cross_track *tr, const CgRowRef &row, double d2, int nearest,
                int rank, const ndt_pose_lattice &L) {
  memset(c, 0, sizeof(*c));
  c->cand.session = session; c->cand.submap = row.m; c->cand.anchor_scan = tr[row.t].sub_anchor[row.m]; c->cand.newest_scan = newest_scan;
  c->cand.nearest_scan = nearest; c->cand.dist = std::sqrt(d2); c->cand.path = 0.0; c->cand.lattice = L;
  c->map_session = row.t; c->rank = rank; c->d2 = d2;
}

// THE DEFINITION, for one searcher (the arguments checked by the caller): its candidates into out[0 .. max_submaps), how many.
int cross_gate_host(const double *last, int newest_scan, int own, const ndt_cross_track *tr, int n_tracks, const ndt_loop_multi_params &p,
                    int session, ndt_cross_candidate *out) {
  const double r2 = p.loop.radius * p.loop.radius;
  struct Hit { double d2; int t, m, near; } best[NDT_LOOP_MAX_SUBMAPS];
  int n = 0;
  for (int t = 0; t < n_tracks; ++t) {
    if (t == own) continue;
    const double *T = tr[t].poses;
    for (int m = 0; m <= tr[t].n_submaps - 2; ++m) {
      int first; unsigned cnt;
      cross_range(tr[t], m, &first, &cnt);
      if (!cnt) continue;
      double d2 = 0.0; int near = first;
      for (int k = first; k < first + (int)cnt; ++k) {
        const double dx = last[0] - T[3 * (size_t)k], dy = last[1] - T[3 * (size_t)k + 1];
        const double xx = dx * dx, yy = dy * dy, dk = xx + yy;
        if (k == first || dk < d2) { d2 = dk; near = k; }
      }
      if (!(d2 <= r2)) continue;
      // (the kept ones are in (d2, t, m) order and (t, m) ascends: this one goes behind every one that is not farther)
      int pos = n;
      while (pos > 0 && d2 < best[pos - 1].d2) --pos;
      if (pos >= p.max_submaps) continue;
      for (int q = std::min(n, p.max_submaps - 1); q > pos; --q) best[q] = best[q - 1];
      best[pos] = Hit{d2, t, m, near};
      n = std::min(n + 1, p.max_submaps);
    }
  }
  if (!n) return 0;
  const ndt_pose_lattice L = loop_lattice_around(p.loop, last);
  for (int r = 0; r < n; ++r) cross_fill(out + r, session, newest_scan, tr, CgRowRef{best[r].t, best[r].m}, best[r].d2, best[r].near, r, L);
  return n;
}

// The refusals both forms share, behind their NULL checks; *R: the rows.
int cross_check(ndt_ctx *ctx, const std::string &f, const double *last_poses, const int *own, int n_search, const ndt_cross_track *tr,
                int n_tracks, const ndt_loop_multi_params *p, uint64_t *R) {
  if (n_tracks < 1) return fail(ctx, NDT_E_ARG, f + ": n_tracks < 1");
  *R = 0;
  for (int t = 0; t < n_tracks; ++t) {
    const std::string ft = f + ": track " + std::to_string(t);
    if (!tr[t].poses || !tr[t].sub_first || !tr[t].sub_anchor || !tr[t].sub_offsets) return fail(ctx, NDT_E_ARG, ft + ": NULL pointer");
    CG_TRY(loop_check_arrays(ctx, ft, tr[t].poses, tr[t].n_scans, tr[t].sub_first, tr[t].sub_anchor, tr[t].sub_offsets, tr[t].n_submaps));
    *R += (uint64_t)(tr[t].n_submaps - 1);
  }
  uint64_t P = 0;
  CG_TRY(loop_check_multi_params(ctx, p, f, &P));
  for (int i = 0; i < n_search; ++i) {
    for (int c = 0; c < 3; ++c)
      if (!(std::fabs(last_poses[3 * (size_t)i + c]) <= DBL_MAX))
        return fail(ctx, NDT_E_ARG, f + ": searcher " + std::to_string(i) + ": the last pose is not finite");
    if (own[i] < -1 || own[i] >= n_tracks)
      return fail(ctx, NDT_E_ARG, f + ": searcher " + std::to_string(i) + ": own is outside [-1, n_tracks)");
  }
  if (*R > kCgMaxPairs || (uint64_t)n_search * *R > kCgMaxPairs)
    return fail(ctx, NDT_E_ARG, f + ": more than 2^28 (searcher, closed submap) pairs");
  return NDT_OK;
}

// The device gate behind the refusals (n_search >= 1; the tracks' sub_offsets are read up to entry n_submaps - 1 only): one table
// upload, the two launches, one read-back, one wait.  `session`: what cand.session says per searcher (nullptr: its index).
// out[i * max_submaps + r], n_out[i]; every record is written (zero behind a searcher's candidates).
int cross_gate_dev(ndt_ctx *ctx, const double *last_poses, const int *newest_scan, const int *own, const int *session, int n_search,
                   const ndt_cross_track *tr, int n_tracks, const ndt_loop_multi_params &p, ndt_cross_candidate *out, int *n_out,
                   const char *fn, size_t *h2d = nullptr, size_t *d2h = nullptr) {
  const size_t K = (size_t)p.max_submaps, S = (size_t)n_search;
  memset(out, 0, S * K * sizeof(ndt_cross_candidate));
  std::fill(n_out, n_out + S, 0);
  if (h2d) *h2d = 0;
  if (d2h) *d2h = 0;
  std::vector<CgRowRef> rows;
  cross_rows(tr, n_tracks, &rows);
  const size_t R = rows.size();
  if (!R) return NDT_OK;      // no closed submap anywhere: nothing to launch
  std::vector<int> first(R);
  std::vector<CgRow> tab(R);
  unsigned long long total = 0;
  for (size_t r = 0; r < R; ++r) {
    unsigned n;
    cross_range(tr[rows[r].t], rows[r].m, &first[r], &n);
    tab[r] = CgRow{total, n, rows[r].t};
    total += n;
  }
  CallFrame fr(ctx);
  CG_TRY(fr.open());
  hipStream_t st = fr.st;
  Regions U;      // the table, then the scratch behind it in the same block
  const size_t u_rows = U.take(R * sizeof(CgRow), 256), u_xy = U.take((size_t)total * sizeof(double2), 256),
               u_se = U.take(S * sizeof(CgSearch), 256), up = U.end;
  const size_t d_key = U.take(S * R * 8, 256), d_near = U.take(S * R * 4, 256), d_pick = U.take(S * 4 * sizeof(CgPick), 256);
  CG_TRY(ctx->cg_tab.reserve(ctx, up));
  CG_TRY(ctx->d_cg.ensure(ctx, U.end));
  CG_TRY(ctx->h_cg.ensure(ctx, S * 4 * sizeof(CgPick)));
  unsigned char *h = ctx->cg_tab.h.p, *d = ctx->d_cg.p;
  memcpy(h + u_rows, tab.data(), R * sizeof(CgRow));
  double *xy = Regions::at<double>(h, u_xy);
  for (size_t r = 0; r < R; ++r) {
    const double *T = tr[rows[r].t].poses + 3 * (size_t)first[r];
    for (unsigned k = 0; k < tab[r].n; ++k) { *xy++ = T[3 * (size_t)k]; *xy++ = T[3 * (size_t)k + 1]; }
  }
  CgSearch *se = Regions::at<CgSearch>(h, u_se);
  for (size_t i = 0; i < S; ++i) se[i] = CgSearch{last_poses[3 * i], last_poses[3 * i + 1], own[i], 0};
  HIP_TRY(ctx, ctx->cg_tab.upload(d, 0, up, st));
  const double r2 = p.loop.radius * p.loop.radius;
  cross_dist_kernel<<<dim3((unsigned)R, (unsigned)std::min<size_t>((S + kCgBlock - 1) / kCgBlock, 65535)), kCgBlock, 0, st>>>(
      (const CgRow *)(d + u_rows), (const double2 *)(d + u_xy), (const CgSearch *)(d + u_se), n_search, (int)R, r2,
      (unsigned long long *)(d + d_key), (int *)(d + d_near));
  HIP_TRY(ctx, hipGetLastError());
  cross_pick_kernel<<<(unsigned)S, kCgBlock, 0, st>>>((const unsigned long long *)(d + d_key), (const int *)(d + d_near), (int)R,
                                                      (CgPick *)(d + d_pick));
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_cg.p, d + d_pick, S * 4 * sizeof(CgPick), hipMemcpyDeviceToHost, st));
  CG_TRY(fr.close_and_wait());
  if (h2d) *h2d = up;
  if (d2h) *d2h = S * 4 * sizeof(CgPick);
  const CgPick *pick = (const CgPick *)ctx->h_cg.p;
  for (size_t i = 0; i < S; ++i) {
    const CgPick *pi = pick + 4 * i;
    int n = 0;
    while (n < (int)K && pi[n].key != kCgNone) ++n;
    if (!n) continue;
    for (int r = 0; r < n; ++r)
      if (pi[r].row < 0 || (size_t)pi[r].row >= R || pi[r].k < 0 || (unsigned)pi[r].k >= tab[(size_t)pi[r].row].n)
        return fail(ctx, NDT_E_HIP, std::string(fn) + ": the device gate returned a pick outside its table");
    const ndt_pose_lattice L = loop_lattice_around(p.loop, last_poses + 3 * i);
    for (int r = 0; r < n; ++r) {
      double d2;
      memcpy(&d2, &pi[r].key, 8);
      cross_fill(out + i * K + (size_t)r, session ? session[i] : (int)i, newest_scan[i], tr, rows[(size_t)pi[r].row], d2,
                 first[(size_t)pi[r].row] + pi[r].k, r, L);
    }
    n_out[i] = n;
  }
  return NDT_OK;
}

// Who searches and who is searched in a set (include/ndt_mi355x.h), and the device gate on them: the candidates of all
// searchers in a row, cand.session and map_session as session indices.  A gate that ran adds its one host wait to *stats.
int cross_gate_set(ndt_sessions *s, const unsigned char *which, const unsigned char *against, const ndt_loop_multi_params &p, const char *fn,
                   std::vector<ndt_cross_candidate> *C, ndt_sessions_stats *stats) {
  C->clear();
  std::vector<int> track_ses, track_of((size_t)s->S, -1);
  std::vector<std::vector<int>> anchors;
  std::vector<ndt_cross_track> tr;
  for (int i = 0; i < s->S; ++i) {
    const SsSession &Q = s->ses[(size_t)i];
    if ((against && !against[i]) || !Q.started || Q.n_poses < 1 || Q.n_closed < 1) continue;
    track_of[(size_t)i] = (int)track_ses.size();
    track_ses.push_back(i);
    anchors.emplace_back((size_t)Q.n_closed + 1);
    for (int m = 0; m <= Q.n_closed; ++m) anchors.back()[(size_t)m] = ss_anchor(Q, m);
  }
  for (size_t t = 0; t < track_ses.size(); ++t) {
    const SsSession &Q = s->ses[(size_t)track_ses[t]];
    tr.push_back(ndt_cross_track{Q.traj.data(), (size_t)Q.n_poses, Q.sub_first.data(), anchors[t].data(), Q.closed_off.data(), Q.n_closed + 1});
  }
  std::vector<double> last; std::vector<int> newest, own, who;
  for (int i = 0; i < s->S; ++i) {
    const SsSession &Q = s->ses[(size_t)i];
    if ((which && !which[i]) || !Q.started || Q.n_poses < 1) continue;
    const double *L = Q.traj.data() + 3 * ((size_t)Q.n_poses - 1);
    last.insert(last.end(), L, L + 3);
    newest.push_back(Q.n_poses - 1); own.push_back(track_of[(size_t)i]); who.push_back(i);
  }
  if (who.empty() || tr.empty()) return NDT_OK;
  uint64_t R = 0;
  for (const ndt_cross_track &T : tr) R += (uint64_t)(T.n_submaps - 1);
  if (R > kCgMaxPairs || (uint64_t)who.size() * R > kCgMaxPairs)
    return fail(s->ctx, NDT_E_ARG, std::string(fn) + ": more than 2^28 (searcher, closed submap) pairs");
  const size_t K = (size_t)p.max_submaps;
  std::vector<ndt_cross_candidate> all(who.size() * K);
  std::vector<int> n(who.size());
  size_t h2d = 0, d2h = 0;
  CG_TRY(cross_gate_dev(s->ctx, last.data(), newest.data(), own.data(), who.data(), (int)who.size(), tr.data(), (int)tr.size(), p, all.data(),
                        n.data(), fn, &h2d, &d2h));
  stats->host_waits++; stats->h2d_bytes += h2d; stats->d2h_bytes += d2h;
  for (size_t i = 0; i < who.size(); ++i)
    for (int r = 0; r < n[i]; ++r) {
      ndt_cross_candidate c = all[i * K + (size_t)r];
      c.map_session = track_ses[(size_t)c.map_session];
      C->push_back(c);
    }
  return NDT_OK;
}

// Both set calls: the bracket, the refusals, the gate, and for out_loops the search.  The set's stats -- the gate's part and
// the search's -- are written once; behind a search that failed they hold the gate's part alone.
int cross_set_entry(ndt_sessions *s, const unsigned char *which, const unsigned char *against, const ndt_loop_multi_params *p,
                    ndt_cross_candidate *out_cand, ndt_cross_loop *out_loops, int *n_out, ndt_result *records_host, const char *fn) {
  SetCall call{s, fn};
  uint64_t P = 0;
  int rc = call.enter();
  if (rc || (rc = loop_entry_checks(call.ctx, call.f, p ? &p->loop : nullptr, p, out_cand ? (void *)out_cand : (void *)out_loops, n_out, &P))) return rc;
  return call.run([&] {
    std::vector<ndt_cross_candidate> C;
    ndt_sessions_stats stats{};
    CG_TRY(cross_gate_set(s, which, against, *p, fn, &C, &stats));
    if (C.size() * P > (uint64_t)INT32_MAX)
      return call.refuse("more than 2^31 - 1 lattice poses over the " + std::to_string(C.size()) + " candidates");
    *n_out = (int)C.size();
    int found = NDT_OK;
    if (out_cand) give_candidates(C, out_cand, n_out);
    else if (!C.empty()) {
      const ndt_sessions_stats gate = stats;
      std::vector<ndt_loop_candidate> lc(C.size());
      std::vector<ndt_loop_multi> M(C.size());
      for (size_t j = 0; j < C.size(); ++j) lc[j] = C[j].cand;
      memset(out_loops, 0, C.size() * sizeof(ndt_cross_loop));
      LpSearch T{s, p->loop, lc, P, records_host, stats};
      T.ranged(p, M.data(), fn);
      for (size_t j = 0; j < C.size(); ++j) T.owner[j] = C[j].map_session;
      if ((found = T.run())) stats = gate;
      else for (size_t j = 0; j < C.size(); ++j) { out_loops[j].m = M[j]; out_loops[j].map_session = C[j].map_session; }
    }
    s->stats = stats;
    return found;
  });
}

#undef CG_TRY

}  // namespace

extern "C" {

int ndt_cross_gate(const double last_pose[3], int newest_scan, int own, const ndt_cross_track *tracks, int n_tracks,
                   const ndt_loop_multi_params *p, ndt_cross_candidate *out, int *n_out) {
  if (!last_pose || !tracks || !p || !out || !n_out) return fail(nullptr, NDT_E_ARG, "ndt_cross_gate: NULL pointer");
  uint64_t R = 0;
  const int rc = cross_check(nullptr, "ndt_cross_gate", last_pose, &own, 1, tracks, n_tracks, p, &R);
  if (rc) return rc;
  *n_out = cross_gate_host(last_pose, newest_scan, own, tracks, n_tracks, *p, 0, out);
  return NDT_OK;
}

int ndt_cross_gate_batch(ndt_ctx *ctx, const double *last_poses, const int *newest_scan, const int *own, int n_search,
                         const ndt_cross_track *tracks, int n_tracks, const ndt_loop_multi_params *p, ndt_cross_candidate *out, int *n_out) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  const std::string f("ndt_cross_gate_batch");
  if (n_search < 0) return fail(ctx, NDT_E_ARG, f + ": n_search < 0");
  if (!tracks || !p || (n_search && (!last_poses || !newest_scan || !own || !out || !n_out))) return fail(ctx, NDT_E_ARG, f + ": NULL pointer");
  uint64_t R = 0;
  const int rc = cross_check(ctx, f, last_poses, own, n_search, tracks, n_tracks, p, &R);
  if (rc) return rc;
  if (!n_search) return NDT_OK;
  return cross_gate_dev(ctx, last_poses, newest_scan, own, nullptr, n_search, tracks, n_tracks, *p, out, n_out, "ndt_cross_gate_batch");
}

int ndt_sessions_cross_candidates(ndt_sessions *s, const unsigned char *which, const unsigned char *against,
                                  const ndt_loop_multi_params *p, ndt_cross_candidate *out, int *n_out) {
  return cross_set_entry(s, which, against, p, out, nullptr, n_out, nullptr, "ndt_sessions_cross_candidates");
}

int ndt_sessions_find_cross_loops(ndt_sessions *s, const unsigned char *which, const unsigned char *against,
                                  const ndt_loop_multi_params *p, ndt_cross_loop *out, int *n_out, ndt_result *records_host) {
  return cross_set_entry(s, which, against, p, nullptr, out, n_out, records_host, "ndt_sessions_find_cross_loops");
}

}  // extern "C"
