// Loop search on a session set (ndt_sessions_loop_candidates, ndt_sessions_find_loops; their _multi forms:
// 4.19): the host gating of one candidate submap per session, or of several, and the search of all candidates in one set of
// launches -- the newest scans into the robot frame, the pre-filter, the batched build of the old submaps' maps, the multi-job
// sweep and pick (ndt_score.hip.h), the candidates' guesses, the multi-map match and, for the _multi form, the multi-map
// ranged verification (ndt_fit_points.hip.h).  The same search serves the loops between sessions (ndt_cross.hip.h, included
// behind this file): a candidate's cloud and anchor pose may be another session's.  Included at the end of ndt_mi355x.hip (one
// translation unit).  Two kernels of its own:
//   loop_scan_kernel     every candidate's newest stored scan from the map frame into the robot frame (repose_point)
//   loop_guess_kernel    per (candidate, slot): the lattice pose of the slot's pick as initial guess, the candidate's filtered
//                        scan laid out once more behind a device-built offset, and the slot's map (-1: no pick in that slot)

namespace {

struct LpScan { const float2 *src; unsigned long long n, off; double pose[3]; };      // a newest scan, its place in the scratch, the session's last pose
struct LpJob { Lattice L; unsigned long long vol; int scan, pad; };                   // a candidate's lattice, where its volume starts, its newest scan among the call's

// repose_rows_kernel's shape, out of place: new pose (0, 0, 0).  A last pose that is bit-equal to it keeps the points' bytes,
// as ndt_repose_points does.
__global__ void __launch_bounds__(256)
loop_scan_kernel(const LpScan *__restrict__ tab, int n_rows, float2 *__restrict__ out) {
  const double zero[3] = {0.0, 0.0, 0.0};
  for (int r = blockIdx.y; r < n_rows; r += gridDim.y) {
    const LpScan m = tab[r];
    if (!m.n) continue;
    const ReposeMove M = repose_move(m.pose, zero);
    for (unsigned long long j = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; j < m.n;
         j += (unsigned long long)gridDim.x * blockDim.x) {
      const float2 v = m.src[j];
      out[m.off + j] = M.same ? v : repose_point(M, v.x, v.y);
    }
  }
}

// Workgroup b = j K + c: slot c of candidate j.  Scan b of the match launch is candidate j's filtered scan -- scan jobs[j].scan
// of the filtered ones, which several candidates may name -- at rep_off[b] = K * (the lengths of the candidates before j) +
// c * len(j): the K copies of a scan lie one behind the other, the candidates in order.  (The lengths exist on the device
// only; every workgroup adds up those before its candidate -- whole numbers, in any order.)
__global__ void __launch_bounds__(256)
loop_guess_kernel(const LpJob *__restrict__ jobs, int J, int K, const float2 *__restrict__ flt, const unsigned long long *__restrict__ flt_off,
                  const unsigned long long *__restrict__ cand, const int *__restrict__ n_cand, const double *__restrict__ score,
                  float2 *__restrict__ rep, unsigned long long *__restrict__ rep_off, double *__restrict__ inits,
                  double *__restrict__ cand_score, int *__restrict__ map_of) {
  __shared__ unsigned long long before[256];
  const int b = blockIdx.x, j = b / K, c = b - j * K;
  unsigned long long mine = 0;
  for (int q = threadIdx.x; q < j; q += blockDim.x) { const int sq = jobs[q].scan; mine += flt_off[sq + 1] - flt_off[sq]; }
  before[threadIdx.x] = mine;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) before[threadIdx.x] += before[threadIdx.x + w];
    __syncthreads();
  }
  const int sj = jobs[j].scan;
  const unsigned long long o0 = flt_off[sj], len = flt_off[sj + 1] - o0, at = (unsigned long long)K * before[0] + (unsigned long long)c * len;
  if (threadIdx.x == 0) {
    const LpJob Jb = jobs[j];
    double p[3] = {0.0, 0.0, 0.0}, s = 0.0;
    const bool live = c < n_cand[j];
    if (live) { const unsigned long long idx = cand[(size_t)j * K + c]; lattice_pose(Jb.L, idx, p); s = score[Jb.vol + idx]; }
    inits[3 * b] = p[0]; inits[3 * b + 1] = p[1]; inits[3 * b + 2] = p[2];
    cand_score[b] = s;
    map_of[b] = live ? j : -1;
    rep_off[b] = at;
    if (b == J * K - 1) rep_off[b + 1] = at + len;
  }
  for (unsigned long long i = threadIdx.x; i < len; i += blockDim.x) rep[at + i] = flt[o0 + i];
}

#define LP_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

// The refusals of the gating's parameters; *P: the poses of every candidate's lattice.
int loop_check_params(ndt_ctx *ctx, const ndt_loop_params *p, const std::string &f, uint64_t *P) {
  for (double v : {p->min_path, p->radius, p->step_xy, p->step_yaw})
    if (!(v >= 0.0) || !std::isfinite(v)) return fail(ctx, NDT_E_ARG, f + ": min_path, radius, step_xy or step_yaw is negative or not finite");
  if (p->half_x < 0 || p->half_y < 0 || p->half_yaw < 0) return fail(ctx, NDT_E_ARG, f + ": a negative half extent");
  const uint64_t nx = 2 * (uint64_t)p->half_x + 1, ny = 2 * (uint64_t)p->half_y + 1, nk = 2 * (uint64_t)p->half_yaw + 1;      // < 2^32 each
  if (nx * ny > (uint64_t)kPickMaxPoses || nx * ny * nk > (uint64_t)kPickMaxPoses) return fail(ctx, NDT_E_ARG, f + ": a lattice of more than 2^24 poses");
  if (p->top_k < 1 || p->top_k > NDT_LOOP_MAX_CAND) return fail(ctx, NDT_E_ARG, f + ": top_k must be in 1 .. " + std::to_string(NDT_LOOP_MAX_CAND));
  if (p->max_cost != p->max_cost) return fail(ctx, NDT_E_ARG, f + ": max_cost is NaN");
  *P = nx * ny * nk;
  return NDT_OK;
}

// The refusals ndt_loop_multi_params adds to those of its `loop` part.
int loop_check_multi_params(ndt_ctx *ctx, const ndt_loop_multi_params *p, const std::string &f, uint64_t *P) {
  const int rc = loop_check_params(ctx, &p->loop, f, P);
  if (rc) return rc;
  if (p->max_submaps < 1 || p->max_submaps > NDT_LOOP_MAX_SUBMAPS)
    return fail(ctx, NDT_E_ARG, f + ": max_submaps must be in 1 .. " + std::to_string(NDT_LOOP_MAX_SUBMAPS));
  if (!(p->max_d2 >= 0.0)) return fail(ctx, NDT_E_ARG, f + ": max_d2 is NaN or negative");
  if (!(p->min_overlap >= 0.0 && p->min_overlap <= 1.0)) return fail(ctx, NDT_E_ARG, f + ": min_overlap is NaN or outside [0, 1]");
  return NDT_OK;
}

// The lattice of the gating rule around a last pose (tx, ty, th[deg]).
ndt_pose_lattice loop_lattice_around(const ndt_loop_params &p, const double *last) {
  const double tx = last[0], ty = last[1], yaw = last[2] * M_PI / 180;      // DEG2RAD
  ndt_pose_lattice L;
  memset(&L, 0, sizeof(L));
  L.x0 = tx - (double)p.half_x * p.step_xy; L.y0 = ty - (double)p.half_y * p.step_xy; L.yaw0 = yaw - (double)p.half_yaw * p.step_yaw;
  L.step_x = p.step_xy; L.step_y = p.step_xy; L.step_yaw = p.step_yaw;
  L.nx = 2 * p.half_x + 1; L.ny = 2 * p.half_y + 1; L.nyaw = 2 * p.half_yaw + 1;
  return L;
}

// The gating of one trajectory as include/ndt_mi355x.h defines it (ndt_loop_gate's arguments, checked by the caller): the
// eligible submaps of smallest dist, max_k of them at the most, in ascending (dist, submap), appended to *out as candidates of
// `session`, every one with the session's one lattice.  Returns how many.  The single-candidate gating is max_k = 1.
int loop_gate_k(const double *T, int n, const int *sub_first, const int *sub_anchor, const uint64_t *closed_off, int n_closed,
                const ndt_loop_params &p, int session, int max_k, std::vector<ndt_loop_candidate> *out) {
  if (n < 1 || n_closed < 2) return 0;
  auto dist = [&](int a, int b) {
    const double dx = T[3 * a] - T[3 * b], dy = T[3 * a + 1] - T[3 * b + 1];
    return std::sqrt(dx * dx + dy * dy);
  };
  const size_t at = out->size();
  for (int m = 0; m <= n_closed - 2; ++m) {
    const int first = sub_first[m], last = sub_first[m + 1] - 1;
    if (last < first || closed_off[m + 1] == closed_off[m]) continue;
    double path = 0.0;
    for (int k = last; k <= n - 2; ++k) path += dist(k + 1, k);
    if (!(path >= p.min_path)) continue;
    double d = dist(n - 1, first); int near = first;
    for (int k = first + 1; k <= last; ++k) { const double dk = dist(n - 1, k); if (dk < d) { d = dk; near = k; } }
    if (!(d <= p.radius)) continue;
    // (the eligible ones so far are in (dist, submap) order: this one goes behind every one that is not farther)
    size_t pos = out->size();
    while (pos > at && d < (*out)[pos - 1].dist) --pos;
    if (pos - at >= (size_t)max_k) continue;
    ndt_loop_candidate c;
    memset(&c, 0, sizeof(c));
    c.session = session; c.submap = m; c.anchor_scan = sub_anchor[m]; c.newest_scan = n - 1; c.nearest_scan = near;
    c.dist = d; c.path = path;
    out->insert(out->begin() + (ptrdiff_t)pos, c);
    if (out->size() - at > (size_t)max_k) out->pop_back();
  }
  if (out->size() == at) return 0;
  const ndt_pose_lattice L = loop_lattice_around(p, T + 3 * (size_t)(n - 1));
  for (size_t i = at; i < out->size(); ++i) (*out)[i].lattice = L;
  return (int)(out->size() - at);
}

// ... of the sessions of a set that `which` names; out: up to max_k candidates per session, the sessions in ascending order.
void loop_gate(const ndt_sessions *s, const unsigned char *which, const ndt_loop_params &p, std::vector<ndt_loop_candidate> *out,
               int max_k = 1) {
  out->clear();
  std::vector<int> anchor;
  for (int i = 0; i < s->S; ++i) {
    const SsSession &Q = s->ses[(size_t)i];
    if ((which && !which[i]) || !Q.started || Q.n_closed < 2) continue;
    anchor.resize((size_t)Q.n_closed);
    for (int m = 0; m < Q.n_closed; ++m) anchor[(size_t)m] = ss_anchor(Q, m);
    loop_gate_k(Q.traj.data(), Q.n_poses, Q.sub_first.data(), anchor.data(), Q.closed_off.data(), Q.n_closed, p, i, max_k, out);
  }
}

// The decision of ndt_sessions_find_loops_multi for one candidate whose records and ranged statistics are in (include/
// ndt_mi355x.h states the rule): cand_cost and best; returns ok_best.
bool loop_decide_ranged(const ndt_loop_multi_params &mp, const ndt_result *res, ndt_loop_multi *M) {
  ndt_loop &L = M->loop;
  bool best_ok = false; uint32_t best_in = 0;
  for (int c = 0; c < L.n_cand; ++c) {
    const ndt_fit_stats &st = M->fit[c];
    const bool usable = res[c].converged && st.n_in >= 1 && (double)st.n_in >= mp.min_overlap * (double)st.n_points;
    L.cand_cost[c] = usable ? st.fitness : 1e7;
    const bool ok = L.cand_cost[c] <= mp.loop.max_cost;
    const uint32_t in = usable ? st.n_in : 0;
    const bool first = L.best < 0 || (ok != best_ok ? ok : in != best_in ? in > best_in : L.cand_cost[c] < L.cand_cost[L.best]);
    if (first) { L.best = c; best_ok = ok; best_in = in; }
  }
  return best_ok;
}

// The search of the candidates C (DESIGN.md 4.15's list; 4.19: the ranged verification; 4.20: the loops between sessions); the
// arguments have passed the entry point's refusals.  What its three callers differ in is set up once, by single() or ranged()
// (and `owner`, which the cross search overwrites): the function's name in messages; where record j is written (loop[j], and
// multi[j] with its slots' ranged statistics); whether the ranged verification runs, and with it the rule that decides best and
// found (mp); the session whose closed cloud and trajectory candidate j's submap and anchor scan are numbered in (owner[j]).
// The parts add to `stats`, which the entry owns.
struct LpSearch {
  ndt_sessions *s; const ndt_loop_params &p; const std::vector<ndt_loop_candidate> &C; uint64_t P; ndt_result *records_host;
  ndt_sessions_stats &stats;
  const char *fn = "ndt_sessions_find_loops"; const ndt_loop_multi_params *mp = nullptr;
  std::vector<ndt_loop *> loop; std::vector<ndt_loop_multi *> multi; std::vector<int> owner;
  ndt_ctx *ctx = s->ctx; hipStream_t st = ctx->stream; const size_t J = C.size(), K = (size_t)p.top_k, B = J * K;
  std::vector<int> scan_of, rank;                  // candidate j's newest scan among the call's nS (one per session) and its rank
  size_t nS = 0, longest = 0, NJ = 0, N = 0;       // NJ: the points of every candidate's scan, a shared one counted once per candidate
  std::vector<LpScan> rows; std::vector<uint64_t> raw_off, vol; std::vector<ndt_score_job> jobs;
  Regions A, D;                                    // the table; the device scratch
  size_t a_rows = 0, a_off = 0, a_jobs = 0, d_robot = 0, d_flt = 0, d_foff = 0, d_score = 0, d_pairs = 0, d_cand = 0, d_ncand = 0, d_rep = 0,
         d_roff = 0, d_init = 0, d_cs = 0, d_mapof = 0, d_res = 0, d_fit = 0;
  SsBack back{s}; size_t r_res = 0, r_cand = 0, r_cs = 0, r_ncand = 0, r_fit = 0;      // host wait 2's read-back
  std::vector<const ndt_map *> rd; const ndt_map *first = nullptr;      // the map every candidate's slots read; the first one built
  template <typename T> T *dev(size_t o) const { return Regions::at<T>(s->lp.p, o); }

  void single(ndt_loop *out) { for (size_t j = 0; j < J; ++j) { loop.push_back(out + j); owner.push_back(C[j].session); } }
  void ranged(const ndt_loop_multi_params *m, ndt_loop_multi *mout, const char *name) {
    mp = m; fn = name;
    for (size_t j = 0; j < J; ++j) { loop.push_back(&mout[j].loop); multi.push_back(mout + j); owner.push_back(C[j].session); }
  }
  int plan(); int scans(); int maps(); int match(); void decide(); int run();      // the parts, in this order, and the search
};

// (1) the plan: the records' fixed part, every candidate's scan and rank (the candidates of a session lie in a row), the newest
// scans' rows with an empty scan nS behind them -- the scan of a candidate whose map is refused: its poses then score nothing and
// nothing is picked --, volume offsets and jobs (N = 0: every newest scan is empty, nothing to search with); (2) the table: the
// rows | their offsets in the scratch | lattices, volume offsets, scans; the layouts of the device scratch and of the read-back
int LpSearch::plan() {
  stats.sessions_stepped = (int)J;
  scan_of.resize(J); rank.resize(J); jobs.resize(J); vol.assign(J + 1, 0);
  for (size_t j = 0; j < J; ++j) {
    const bool same = j > 0 && C[j].session == C[j - 1].session;
    rank[j] = same ? rank[j - 1] + 1 : 0;
    scan_of[j] = same ? scan_of[j - 1] : (int)nS++;
    if (mp) { memset(multi[j], 0, sizeof(*multi[j])); multi[j]->rank = rank[j]; }
    ndt_loop &L = *loop[j];
    memset(&L, 0, sizeof(L));
    L.cand = C[j]; L.best = -1;
    L.edge.from = C[j].anchor_scan; L.edge.to = C[j].newest_scan;
    memcpy(L.edge.info, p.info, sizeof(p.info));
  }
  rows.resize(nS); raw_off.assign(nS + 2, 0);
  for (size_t j = 0; j < J; ++j) {
    const SsSession &Q = s->ses[(size_t)C[j].session];
    const size_t k = Q.scan_off.size() - 2, u = (size_t)scan_of[j];
    const uint64_t n = Q.scan_off[k + 1] - Q.scan_off[k];
    if (rank[j] == 0) {
      const double *last = Q.traj.data() + 3 * ((size_t)Q.n_poses - 1);
      rows[u] = LpScan{Q.store[Q.cur].p + Q.scan_off[k], n, raw_off[u], {last[0], last[1], last[2]}};
      raw_off[u + 1] = raw_off[u] + n;
      longest = std::max(longest, (size_t)n);
    }
    NJ += (size_t)n;
    vol[j + 1] = vol[j] + P;
    jobs[j] = ndt_score_job{(int)j, scan_of[j], C[j].lattice};
  }
  N = (size_t)raw_off[nS];
  raw_off[nS + 1] = raw_off[nS];
  if (!N) return NDT_OK;
  a_rows = A.take(nS * sizeof(LpScan), 256); a_off = A.take((nS + 2) * 8, 256); a_jobs = A.take(J * sizeof(LpJob), 256);
  d_robot = D.take(N * 8, 256); d_flt = D.take(N * 8, 256); d_foff = D.take((nS + 2) * 8, 256); d_score = D.take(J * P * 8, 256);
  d_pairs = D.take(J * P * 4, 256); d_cand = D.take(B * 8, 256); d_ncand = D.take(J * 4, 256); d_rep = D.take(K * NJ * 8, 256);
  d_roff = D.take((B + 1) * 8, 256); d_init = D.take(B * 24, 256); d_cs = D.take(B * 8, 256); d_mapof = D.take(B * 4, 256);
  d_res = D.take(B * sizeof(ndt_result), 256); d_fit = mp ? D.take(B * sizeof(ndt_fit_stats), 256) : 0;
  LP_TRY(s->lp_tab.reserve(ctx, A.end)); LP_TRY(s->d_lp_tab.ensure(ctx, A.end)); LP_TRY(s->lp.ensure(ctx, D.end));
  r_res = back.add(dev<ndt_result>(d_res), B); r_cand = back.add(dev<uint64_t>(d_cand), B); r_cs = back.add(dev<double>(d_cs), B);
  r_ncand = back.add(dev<int>(d_ncand), J);
  if (mp) r_fit = back.add(dev<ndt_fit_stats>(d_fit), B);
  LP_TRY(back.reserve());
  unsigned char *h = s->lp_tab.h.p;
  memcpy(h + a_rows, rows.data(), nS * sizeof(LpScan));
  memcpy(h + a_off, raw_off.data(), (nS + 2) * 8);
  for (size_t j = 0; j < J; ++j) A.at<LpJob>(h, a_jobs)[j] = LpJob{lattice_of(C[j].lattice), vol[j], scan_of[j], 0};
  HIP_TRY(ctx, s->lp_tab.upload(s->d_lp_tab.p, 0, A.end, st));
  stats.h2d_bytes += A.end;
  return NDT_OK;
}

// (3) the newest scans in the robot frame, filtered as a step filters its source -- each once, whoever names it
int LpSearch::scans() {
  const unsigned char *da = s->d_lp_tab.p;
  loop_scan_kernel<<<dim3((unsigned)std::min<size_t>(64, longest / 256 + 1), (unsigned)std::min<size_t>(nS, 65535)), 256, 0, st>>>(
      (const LpScan *)(da + a_rows), (int)nS, dev<float2>(d_robot));
  HIP_TRY(ctx, hipGetLastError());
  return ndt_prefilter_batch_dev(ctx, dev<float>(d_robot), sizeof(float2), (const uint64_t *)(da + a_off), (int)nS + 1, N, s->prm.leaf,
                                 dev<float>(d_flt), dev<uint64_t>(d_foff), st);
}

// (4) the old submaps' maps, each searcher's own from call to call, a slot per rank (host wait 1: the bounding boxes); a
// refused build costs its candidate alone.  first stays nullptr: no map at all -- nobody is found
int LpSearch::maps() {
  std::vector<const float *> bxy(J); std::vector<size_t> bn(J); std::vector<ndt_params> bp(J, s->prm.match);
  std::vector<ndt_map *> built(J); std::vector<int> code(J, NDT_OK);
  for (size_t j = 0; j < J; ++j) {
    const SsSession &Q = s->ses[(size_t)owner[j]];
    const uint64_t a = Q.closed_off[(size_t)C[j].submap];
    bxy[j] = (const float *)(Q.closed.p + a); bn[j] = (size_t)(Q.closed_off[(size_t)C[j].submap + 1] - a);
    built[j] = s->ses[(size_t)C[j].session].loop_maps[rank[j]];
  }
  LP_TRY(check_build_batch(ctx, bxy.data(), bn.data(), sizeof(float2), (int)J, bp.data(), built.data(), fn));
  LP_TRY(build_batch(ctx, bxy.data(), bn.data(), sizeof(float2), (int)J, bp.data(), built.data(), fn, code.data()));
  stats.host_waits++; stats.d2h_bytes += J * 16 * sizeof(unsigned);
  for (size_t j = 0; j < J; ++j) {
    loop[j]->status = code[j];
    if (code[j] != NDT_OK) continue;
    s->ses[(size_t)C[j].session].loop_maps[rank[j]] = built[j];
    if (!first) first = built[j];
  }
  rd.resize(J);
  for (size_t j = 0; j < J; ++j) {
    rd[j] = code[j] == NDT_OK ? built[j] : first;
    if (code[j] != NDT_OK) jobs[j].scan = (int)nS;      // (the empty scan)
  }
  return NDT_OK;
}

// (5) the sweep, (6) the pick, (7) the guesses and the scans' copies, (8) the match and, for the ranged search, the verification
// on the match's own arrays: every slot's statistics at its record's transform, no d2; a dead slot (map_of -1) reads no map
int LpSearch::match() {
  const float *flt = dev<float>(d_flt); const uint64_t *flt_off = dev<uint64_t>(d_foff);
  double *score = dev<double>(d_score); uint32_t *pairs = dev<uint32_t>(d_pairs);
  uint64_t *cand = dev<uint64_t>(d_cand); int *n_cand = dev<int>(d_ncand);
  LP_TRY(score_multi(ctx, rd.data(), (int)J, flt, flt_off, (int)nS + 1, N, longest, jobs.data(), (int)J, score, pairs, vol.data(), st));
  LP_TRY(ndt_lattice_select_multi_dev(ctx, jobs.data(), (int)J, score, pairs, vol.data(), p.top_k, p.local_max, cand, n_cand, st));
  stats.h2d_bytes += J * (sizeof(ScoreJob) + sizeof(PickJob)) + (J + 1) * 8;
  loop_guess_kernel<<<(unsigned)B, 256, 0, st>>>((const LpJob *)(s->d_lp_tab.p + a_jobs), (int)J, (int)K, (const float2 *)flt,
                                                (const unsigned long long *)flt_off, (const unsigned long long *)cand, n_cand, score,
                                                dev<float2>(d_rep), dev<unsigned long long>(d_roff), dev<double>(d_init), dev<double>(d_cs),
                                                dev<int>(d_mapof));
  HIP_TRY(ctx, hipGetLastError());
  LP_TRY(ndt_align_batch_multi_dev(ctx, rd.data(), (int)J, dev<int>(d_mapof), dev<float>(d_rep), dev<uint64_t>(d_roff), (int)B, K * NJ, 0,
                                   dev<double>(d_init), dev<ndt_result>(d_res), st));
  if (!mp) return NDT_OK;
  LP_TRY(ndt_fit_points_multi_dev(ctx, rd.data(), (int)J, dev<int>(d_mapof), dev<float>(d_rep), dev<uint64_t>(d_roff), (int)B, K * NJ, 0,
                                  &dev<ndt_result>(d_res)->T00, sizeof(ndt_result), mp->max_d2, nullptr, dev<ndt_fit_stats>(d_fit), st));
  stats.h2d_bytes += J * sizeof(MapView);
  return NDT_OK;
}

// (9) the decision, behind host wait 2: the slots' records, costs (ranged: statistics), best and found, the pose and the edge
void LpSearch::decide() {
  const ndt_result *res = back.at<ndt_result>(r_res);
  const uint64_t *h_cand = back.at<uint64_t>(r_cand); const double *h_cs = back.at<double>(r_cs); const int *h_n = back.at<int>(r_ncand);
  for (size_t j = 0; j < J; ++j) {
    ndt_loop &L = *loop[j];
    if (L.status != NDT_OK) continue;
    L.n_cand = h_n[j];
    for (int c = 0; c < L.n_cand; ++c) {
      const ndt_result &r = res[j * K + (size_t)c];
      L.cand_index[c] = h_cand[j * K + (size_t)c]; L.cand_score[c] = h_cs[j * K + (size_t)c];
      if (mp) multi[j]->fit[c] = back.at<ndt_fit_stats>(r_fit)[j * K + (size_t)c];
      else {
        L.cand_cost[c] = r.converged ? r.fitness : 1e7;      // (src/PoseEstimator.cpp:43-46, as relocalize_impl)
        if (L.best < 0 || L.cand_cost[c] < L.cand_cost[L.best]) L.best = c;
      }
      if (records_host) records_host[j * NDT_LOOP_MAX_CAND + (size_t)c] = r;
    }
    const bool ranged_ok = mp && loop_decide_ranged(*mp, res + j * K, multi[j]);
    if (L.best < 0) continue;
    const bool ok = mp ? ranged_ok : L.cand_cost[L.best] <= p.max_cost;
    const ndt_result &w = res[j * K + (size_t)L.best];
    L.pose[0] = w.pose[0]; L.pose[1] = w.pose[1]; L.pose[2] = w.pose[2] * 180 / M_PI;      // RAD2DEG
    // (a pose that is not finite leaves rel at 0: the cost rule keeps such a record from being found)
    const double *anchor = s->ses[(size_t)owner[j]].traj.data() + 3 * (size_t)C[j].anchor_scan;
    if (ndt_pg_edge_between(anchor, L.pose, &L.edge) == NDT_OK) L.found = ok;
  }
}

int LpSearch::run() {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  LP_TRY(plan());
  if (!N) return NDT_OK;
  LP_TRY(scans());
  LP_TRY(maps());
  if (!first) return NDT_OK;
  LP_TRY(match());
  LP_TRY(back.wait(stats));
  decide();
  return NDT_OK;
}

// The refusals of a set's loop calls behind check_set: the NULL arguments and the parameters -- p, or mp whose `loop` part p is
// (the _multi and the cross calls); *P: the poses of every candidate's lattice.
int loop_entry_checks(ndt_ctx *ctx, const std::string &f, const ndt_loop_params *p, const ndt_loop_multi_params *mp, const void *out,
                      const int *n_out, uint64_t *P) {
  if (!p || !out || !n_out) return fail(ctx, NDT_E_ARG, f + ": NULL params or outputs");
  return mp ? loop_check_multi_params(ctx, mp, f, P) : loop_check_params(ctx, p, f, P);
}

// The candidates of a gate into the caller's array.
template <typename T> int give_candidates(const std::vector<T> &C, T *out, int *n_out) {
  if (!C.empty()) memcpy(out, C.data(), C.size() * sizeof(T));
  *n_out = (int)C.size();
  return NDT_OK;
}

// The candidates of a set's host gate (mp: up to max_submaps per session).
int loop_candidates_entry(const ndt_sessions *s, const unsigned char *which, const ndt_loop_params *p, const ndt_loop_multi_params *mp,
                          ndt_loop_candidate *out, int *n_out, const char *fn) {
  uint64_t P = 0;
  int rc = check_set(s, 0, false, fn);
  if (rc || (rc = loop_entry_checks(s->ctx, fn, p, mp, out, n_out, &P))) return rc;
  std::vector<ndt_loop_candidate> C;
  loop_gate(s, which, *p, &C, mp ? mp->max_submaps : 1);
  return give_candidates(C, out, n_out);
}

// Both searches (mp and mout: the ranged one): the bracket, the refusals, the gating, the search, the set's stats.
int loop_search_entry(ndt_sessions *s, const unsigned char *which, const ndt_loop_params *p, const ndt_loop_multi_params *mp, ndt_loop *out,
                      ndt_loop_multi *mout, int *n_out, ndt_result *records_host, const char *fn) {
  SetCall call{s, fn};
  uint64_t P = 0;
  int rc = call.enter();
  if (rc || (rc = loop_entry_checks(call.ctx, call.f, p, mp, mp ? (const void *)mout : (const void *)out, n_out, &P))) return rc;
  return call.run([&] {
    std::vector<ndt_loop_candidate> C;
    loop_gate(s, which, *p, &C, mp ? mp->max_submaps : 1);
    if (C.size() * P > (uint64_t)INT32_MAX)
      return call.refuse("more than 2^31 - 1 lattice poses over the " + std::to_string(C.size()) + " candidates");
    *n_out = (int)C.size();
    ndt_sessions_stats stats{};
    LpSearch T{s, *p, C, P, records_host, stats};
    if (mp) T.ranged(mp, mout, fn); else T.single(out);
    const int found = C.empty() ? NDT_OK : T.run();
    if (!found) s->stats = stats;
    return found;
  });
}

// The refusals of one trajectory's arrays (f: the function, and for the cross gate the track).
int loop_check_arrays(ndt_ctx *ctx, const std::string &f, const double *poses, size_t n_scans, const int *sub_first, const int *sub_anchor,
                      const uint64_t *sub_offsets, int n_submaps) {
  if (n_scans < 1 || n_scans > (size_t)INT32_MAX || n_submaps < 1) return fail(ctx, NDT_E_ARG, f + ": need 1 <= n_scans <= 2^31 - 1 and n_submaps >= 1");
  for (int m = 0; m < n_submaps; ++m) {
    const bool ordered = m == 0 ? sub_first[0] == 0 : sub_first[m] >= sub_first[m - 1];
    if (!ordered || sub_first[m] < 0 || (size_t)sub_first[m] >= n_scans || sub_anchor[m] < 0 || (size_t)sub_anchor[m] >= n_scans ||
        sub_offsets[m + 1] < sub_offsets[m])
      return fail(ctx, NDT_E_ARG, f + ": submap " + std::to_string(m) + ": sub_first, sub_anchor or sub_offsets is not a set's layout");
  }
  for (size_t k = 0; k < 3 * n_scans; ++k)
    if (!(std::fabs(poses[k]) <= DBL_MAX)) return fail(ctx, NDT_E_ARG, f + ": scan " + std::to_string(k / 3) + ": a pose is not finite");
  return NDT_OK;
}

// The gating of one trajectory (ndt_loop_gate; mp: ndt_loop_gate_multi, whose `loop` part p is): the NULL checks, the refusals of
// the arrays, then of the parameters, then the candidates (session 0) into out[0 .. *n_out).
int loop_gate_arrays(const char *fn, const double *poses, size_t n_scans, const int *sub_first, const int *sub_anchor,
                     const uint64_t *sub_offsets, int n_submaps, const ndt_loop_params *p, const ndt_loop_multi_params *mp,
                     ndt_loop_candidate *out, int *n_out) {
  const std::string f(fn);
  if (!poses || !sub_first || !sub_anchor || !sub_offsets || !p || !out || !n_out) return fail(nullptr, NDT_E_ARG, f + ": NULL pointer");
  int rc = loop_check_arrays(nullptr, f, poses, n_scans, sub_first, sub_anchor, sub_offsets, n_submaps);
  if (rc) return rc;
  uint64_t P = 0;
  rc = mp ? loop_check_multi_params(nullptr, mp, f, &P) : loop_check_params(nullptr, p, f, &P);
  if (rc) return rc;
  std::vector<ndt_loop_candidate> C;
  loop_gate_k(poses, (int)n_scans, sub_first, sub_anchor, sub_offsets, n_submaps - 1, *p, 0, mp ? mp->max_submaps : 1, &C);
  return give_candidates(C, out, n_out);
}

#undef LP_TRY

}  // namespace

extern "C" {

int ndt_loop_default_params(ndt_loop_params *p) {
  if (!p) return NDT_E_ARG;
  memset(p, 0, sizeof(*p));
  p->min_path = 10.0; p->radius = 2.0; p->step_xy = 0.1; p->step_yaw = 1.0 * M_PI / 180;
  p->half_x = 10; p->half_y = 10; p->half_yaw = 6; p->top_k = 4; p->local_max = 1; p->max_cost = 0.02;
  p->info[0] = p->info[3] = p->info[5] = 1e4;
  return NDT_OK;
}

int ndt_loop_multi_default_params(ndt_loop_multi_params *p) {
  if (!p) return NDT_E_ARG;
  memset(p, 0, sizeof(*p));
  ndt_loop_default_params(&p->loop);
  p->max_submaps = 2; p->max_d2 = 0.09; p->min_overlap = 0.5;
  return NDT_OK;
}

int ndt_loop_gate(const double *poses, size_t n_scans, const int *sub_first, const int *sub_anchor, const uint64_t *sub_offsets,
                  int n_submaps, const ndt_loop_params *p, ndt_loop_candidate *out, int *has) {      // (*has: one candidate at the most)
  return loop_gate_arrays("ndt_loop_gate", poses, n_scans, sub_first, sub_anchor, sub_offsets, n_submaps, p, nullptr, out, has);
}

int ndt_loop_gate_multi(const double *poses, size_t n_scans, const int *sub_first, const int *sub_anchor, const uint64_t *sub_offsets,
                        int n_submaps, const ndt_loop_multi_params *p, ndt_loop_candidate *out, int *n_out) {
  return loop_gate_arrays("ndt_loop_gate_multi", poses, n_scans, sub_first, sub_anchor, sub_offsets, n_submaps, p ? &p->loop : nullptr, p, out, n_out);
}

int ndt_sessions_loop_candidates_multi(const ndt_sessions *s, const unsigned char *which, const ndt_loop_multi_params *p,
                                       ndt_loop_candidate *out, int *n_out) {
  return loop_candidates_entry(s, which, p ? &p->loop : nullptr, p, out, n_out, "ndt_sessions_loop_candidates_multi");
}

int ndt_sessions_loop_candidates(const ndt_sessions *s, const unsigned char *which, const ndt_loop_params *p, ndt_loop_candidate *out,
                                 int *n_out) {
  return loop_candidates_entry(s, which, p, nullptr, out, n_out, "ndt_sessions_loop_candidates");
}

int ndt_sessions_find_loops(ndt_sessions *s, const unsigned char *which, const ndt_loop_params *p, ndt_loop *out, int *n_out,
                            ndt_result *records_host) {
  return loop_search_entry(s, which, p, nullptr, out, nullptr, n_out, records_host, "ndt_sessions_find_loops");
}

int ndt_sessions_find_loops_multi(ndt_sessions *s, const unsigned char *which, const ndt_loop_multi_params *p, ndt_loop_multi *out,
                                  int *n_out, ndt_result *records_host) {
  return loop_search_entry(s, which, p ? &p->loop : nullptr, p, nullptr, out, n_out, records_host, "ndt_sessions_find_loops_multi");
}

}  // extern "C"
