// ndt_posegraph.hip.h -- ndt_pg_*: SE(2) pose-graph optimisation of many graphs in one launch, and ndt_repose_points: stored
// clouds moved from their old scan poses to their new ones (the contract is the header's).  Part of
// libndt_mi355x.so: included by ndt_mi355x.hip inside its anonymous namespace behind ndt_common.hip.h.  Not a standalone header.
//
// One 256-thread workgroup per graph runs every Gauss-Newton iteration of that graph; nothing is shared between workgroups.
// Node i of a graph belongs to thread i % 256 in every node loop, so the vector updates of the conjugate gradients need no
// barrier; only H p (reads the neighbours' p), the preconditioner (a serial block-Thomas sweep) and the dot products do.
// No floating-point atomics: a node sums its arcs' blocks in arc-index order (its list is cut out of a sorted key array),
// and a dot product is each thread's nodes in index order, a fixed wave tree, then the four waves in order.
// The solver (pg_solve_kernel, plain and robust) and the marginals (pg_marginal_kernel) share every step but
// their conjugate-gradient loops: pg_graph_bad, pg_arc_order, pg_radians, pg_node_blocks, pg_arc_hp, pg_factor, pg_apply<K>,
// pg_block_sum_cols<N>, and the tail of the scratch (PgTail, PgWork).

constexpr double kPgPi = 3.14159265358979323846;
constexpr int kPgChunk = 64;                       // nodes of one staged piece of a block-Thomas sweep
constexpr int kPgThreads = 256;

// One row of a call's table.  scratch: byte offset of the graph's own scratch in the call's block.
struct PgRow {
  unsigned long long node0, edge0, scratch;
  int n, m;                                        // nodes, arcs
  unsigned n2, pad;                                // length of the key array: a power of two >= 2 m
};
static_assert(sizeof(PgRow) == 40, "one 40-byte row per graph");

struct PgParams { int max_iter, cg_max_iter, max_halvings, pad; double eps_step, cg_rtol; };
// The level schedule of the robust form (ndt_pg_robust_params without its pg part); unread by the plain one.
struct PgRobust { double mu0, factor, eps_level; int level_iter, pad; };
constexpr double kPgMuMax = 1e12;

// An arc linearised at the current poses: cos / sin of the `from` heading, d r_xy / d theta_from = (a, b), the residual.
// wt: the arc's weight (the robust form: at those poses, 1.0 for a plain arc; the marginals: as given); the plain form leaves it 0
// and unread.
struct PgLin { double c, s, a, b, r0, r1, r2, wt; };

// What every scratch ends with, in doubles from the scratch's start: the linear system's blocks, the chain factor, the
// linearised arcs and the arc order.  `o`: where it starts, behind the vectors that a layout puts in front of it.
struct PgTail {
  size_t D, U, L, Si, W, lin, keys, ptr, end;
  __host__ __device__ static PgTail at(size_t o, size_t n, size_t m, size_t n2) {
    PgTail t;
    t.D = o; o += 6 * n; t.U = o; o += 9 * n; t.L = o; o += 9 * n; t.Si = o; o += 6 * n; t.W = o; o += 9 * n;
    t.lin = o; o += 8 * m; t.keys = o; o += n2; t.ptr = o; o += (n + 2) / 2 + 1;
    t.end = o;
    return t;
  }
};

// The regions of one graph's scratch (host and device agree by calling this one function).
struct PgLayout : PgTail {
  size_t x, xt, g, dl, r, z, p, q, y;
  __host__ __device__ PgLayout(size_t n, size_t m, size_t n2) {
    size_t o = 0;
    x = o; o += 3 * n; xt = o; o += 3 * n; g = o; o += 3 * n; dl = o; o += 3 * n; r = o; o += 3 * n; z = o; o += 3 * n;
    p = o; o += 3 * n; q = o; o += 3 * n; y = o; o += 3 * n;
    static_cast<PgTail &>(*this) = PgTail::at(o, n, m, n2);
  }
};

// The tail's regions of the scratch at `base` as pointers.
struct PgWork {
  double *D, *U, *L, *Si, *W;
  PgLin *lin;
  unsigned long long *keys;
  int *ptr;
  __device__ PgWork(double *base, const PgTail &T)
      : D(base + T.D), U(base + T.U), L(base + T.L), Si(base + T.Si), W(base + T.W), lin(reinterpret_cast<PgLin *>(base + T.lin)),
        keys(reinterpret_cast<unsigned long long *>(base + T.keys)), ptr(reinterpret_cast<int *>(base + T.ptr)) {}
};

__device__ __forceinline__ bool pg_finite(double v) { return fabs(v) <= DBL_MAX; }

// into [-pi, pi)
__host__ __device__ __forceinline__ double pg_wrap(double v) {
  double w = v - 2.0 * kPgPi * floor((v + kPgPi) / (2.0 * kPgPi));
  if (w >= kPgPi) w -= 2.0 * kPgPi;
  if (w < -kPgPi) w += 2.0 * kPgPi;
  return w;
}
// degrees into [-180, 180) (MyUtil::add_angle's range, src/MyUtil.cpp:4-11)
__device__ __forceinline__ double pg_wrap_deg(double v) {
  double w = v - 360.0 * floor((v + 180.0) / 360.0);
  if (w >= 180.0) w -= 360.0;
  if (w < -180.0) w += 360.0;
  return w;
}

// Sums over the workgroup in a fixed shape, N values at once (s_w: 4 N doubles of LDS): each value goes through the wave tree,
// then the four waves in order.  Every thread gets the same bits.  Two barriers: called under block-uniform conditions only.
template <int N>
__device__ __forceinline__ void pg_block_sum_cols(double v[N], double *s_w) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double t = wave_sum(v[k]);
    if ((threadIdx.x & 63) == 0) s_w[(threadIdx.x >> 6) * N + k] = t;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = ((s_w[k] + s_w[N + k]) + s_w[2 * N + k]) + s_w[3 * N + k];
  __syncthreads();
}
__device__ __forceinline__ double pg_block_sum(double v, double *s_w) {
  pg_block_sum_cols<1>(&v, s_w);
  return v;
}
__device__ __forceinline__ double pg_block_max(double v, double *s_w) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  const double t = fmax(fmax(s_w[0], s_w[1]), fmax(s_w[2], s_w[3]));
  __syncthreads();
  return t;
}

// r = (R(th_i)^T (t_j - t_i) - z_xy, wrap(th_j - th_i - z_th)) of one arc at the poses X (radians)
__device__ __forceinline__ PgLin pg_linearise(const double *__restrict__ X, const ndt_pg_edge &E) {
  const double *xi = X + 3 * (size_t)E.from, *xj = X + 3 * (size_t)E.to;
  PgLin l;
  l.c = cos(xi[2]); l.s = sin(xi[2]);
  const double dx = xj[0] - xi[0], dy = xj[1] - xi[1];
  l.a = -l.s * dx + l.c * dy;
  l.b = -l.c * dx - l.s * dy;
  l.r0 = l.c * dx + l.s * dy - E.rel[0];
  l.r1 = l.a - E.rel[1];
  l.r2 = pg_wrap(xj[2] - xi[2] - E.rel[2] * (kPgPi / 180.0));
  l.wt = 0.0;
  return l;
}

// w = Omega v, Omega as xx xy xt yy yt tt
__device__ __forceinline__ void pg_info_mul(const double *__restrict__ I, const double v[3], double w[3]) {
  w[0] = I[0] * v[0] + I[1] * v[1] + I[2] * v[2];
  w[1] = I[1] * v[0] + I[3] * v[1] + I[4] * v[2];
  w[2] = I[2] * v[0] + I[4] * v[1] + I[5] * v[2];
}

// The Jacobian block of an arc's residual, row-major: side 0 = d r / d x_from, side 1 = d r / d x_to.
__device__ __forceinline__ void pg_jac(const PgLin &l, int side, double J[9]) {
  if (side == 0) {
    J[0] = -l.c; J[1] = -l.s; J[2] = l.a;
    J[3] = l.s;  J[4] = -l.c; J[5] = l.b;
    J[6] = 0.0;  J[7] = 0.0;  J[8] = -1.0;
  } else {
    J[0] = l.c;  J[1] = l.s;  J[2] = 0.0;
    J[3] = -l.s; J[4] = l.c;  J[5] = 0.0;
    J[6] = 0.0;  J[7] = 0.0;  J[8] = 1.0;
  }
}
// out = J^T w
__device__ __forceinline__ void pg_jt_mul(const double J[9], const double w[3], double out[3]) {
  out[0] = J[0] * w[0] + J[3] * w[1] + J[6] * w[2];
  out[1] = J[1] * w[0] + J[4] * w[1] + J[7] * w[2];
  out[2] = J[2] * w[0] + J[5] * w[1] + J[8] * w[2];
}
// out = J v
__device__ __forceinline__ void pg_j_mul(const double J[9], const double v[3], double out[3]) {
  out[0] = J[0] * v[0] + J[1] * v[1] + J[2] * v[2];
  out[1] = J[3] * v[0] + J[4] * v[1] + J[5] * v[2];
  out[2] = J[6] * v[0] + J[7] * v[1] + J[8] * v[2];
}
// M += Ja^T Omega Jb (row-major 3 x 3); ROBUST: M += wt Ja^T Omega Jb, and a wt of exactly 1.0 adds the same bits
template <bool ROBUST>
__device__ __forceinline__ void pg_block_add(const double Ja[9], const double *__restrict__ I, const double Jb[9], double wt, double M[9]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double v[3] = {Jb[c], Jb[3 + c], Jb[6 + c]};
    double w[3], o[3];
    pg_info_mul(I, v, w);
    pg_jt_mul(Ja, w, o);
    if constexpr (ROBUST) { M[c] += wt * o[0]; M[3 + c] += wt * o[1]; M[6 + c] += wt * o[2]; }
    else { M[c] += o[0]; M[3 + c] += o[1]; M[6 + c] += o[2]; }
  }
}

// c = r^T Omega r of a linearised arc
__device__ __forceinline__ double pg_chi2(const PgLin &l, const double *__restrict__ I) {
  const double r[3] = {l.r0, l.r1, l.r2};
  double w[3];
  pg_info_mul(I, r, w);
  return (r[0] * w[0] + r[1] * w[1]) + r[2] * w[2];
}
// Geman-McClure at sigma = mu phi, written with q = c / sigma so that a huge sigma gives the plain arc and not inf / inf:
// rho = sigma c / (sigma + c) = c / (1 + q), w = (sigma / (sigma + c))^2 = (1 / (1 + q))^2
__device__ __forceinline__ double pg_rho(double c, double sigma) { return c / (1.0 + c / sigma); }
__device__ __forceinline__ double pg_weight(double c, double sigma) { const double t = 1.0 / (1.0 + c / sigma); return t * t; }

// F = sum r^T Omega r at the poses X: each thread its arcs in index order, then the fixed block sum.  ROBUST: F_mu, an arc with
// phi[e] > 0 adds rho at sigma = mu phi[e] in place of c (phi: the graph's own, or NULL for none).
template <bool ROBUST>
__device__ double pg_cost(const double *__restrict__ X, const ndt_pg_edge *__restrict__ ed, int m, double *s_w, const double *__restrict__ phi,
                          double mu) {
  double acc = 0.0;
  for (int e = (int)threadIdx.x; e < m; e += kPgThreads) {
    const PgLin l = pg_linearise(X, ed[e]);
    const double r[3] = {l.r0, l.r1, l.r2};
    double w[3];
    pg_info_mul(ed[e].info, r, w);
    if constexpr (ROBUST) {
      const double c = (r[0] * w[0] + r[1] * w[1]) + r[2] * w[2], ph = phi ? phi[e] : 0.0;
      acc += ph > 0.0 ? pg_rho(c, mu * ph) : c;
    } else {
      acc += (r[0] * w[0] + r[1] * w[1]) + r[2] * w[2];
    }
  }
  return pg_block_sum(acc, s_w);
}

// A pivot of the chain factor counts as positive when it is above this part of its diagonal entry of T: a part of the graph
// that nothing ties to node 0 leaves pivots at the rounding of the subtraction (1e-16 of the entry, either sign), while the
// pivots of a connected graph keep a good part of it (0.14 and more on figure-eights up to N = 2000, stars, shuffled numbering).
constexpr double kPgPivotFloor = 1e-13;

// inverse of a symmetric 3 x 3 (full row-major in, full row-major out); false unless it is finite and positive definite with
// every pivot S00, m2 / S00, det / m2 above kPgPivotFloor times d0, d1, d2
__device__ __forceinline__ bool pg_spd_inverse(const double S[9], double d0, double d1, double d2, double Inv[9]) {
  const double c00 = S[4] * S[8] - S[5] * S[5], c01 = S[5] * S[2] - S[1] * S[8], c02 = S[1] * S[5] - S[4] * S[2];
  const double m2 = S[0] * S[4] - S[1] * S[1];
  const double det = (S[0] * c00 + S[1] * c01) + S[2] * c02;
  if (!(S[0] > kPgPivotFloor * d0) || !(m2 > kPgPivotFloor * d1 * S[0]) || !(det > kPgPivotFloor * d2 * m2) || !(S[0] > 0.0) || !(m2 > 0.0) ||
      !(det > 0.0) || !pg_finite(det))
    return false;
  const double id = 1.0 / det;
  Inv[0] = c00 * id; Inv[1] = c01 * id; Inv[2] = c02 * id;
  Inv[4] = (S[0] * S[8] - S[2] * S[2]) * id; Inv[5] = (S[1] * S[2] - S[0] * S[5]) * id;
  Inv[8] = m2 * id;
  Inv[3] = Inv[1]; Inv[6] = Inv[2]; Inv[7] = Inv[5];
  return pg_finite(Inv[0]) && pg_finite(Inv[4]) && pg_finite(Inv[8]);
}

// Block-Thomas factor of the chain preconditioner T (block-tridiagonal over the nodes 1 .. n-1: D_i on the diagonal, U_i at
// (i, i + 1)): S_1 = D_1, L_i = U_{i-1}^T S_{i-1}^-1, S_i = D_i - L_i U_{i-1}; kept are L_i, S_i^-1 (six entries) and
// W_i = S_i^-1 U_i.  The sweep is one lane's; the workgroup stages its input and output through LDS in pieces of kPgChunk
// nodes so that the lane never waits for global memory.  false: some S_i is not positive definite (pg_spd_inverse).
__device__ bool pg_factor(const double *__restrict__ D, const double *__restrict__ U, double *__restrict__ L, double *__restrict__ Si,
                          double *__restrict__ W, int n, double *sh, int *s_ok) {
  const int tid = (int)threadIdx.x;
  if (tid == 0) *s_ok = 1;
  double Sp[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i0 = 1; i0 < n; i0 += kPgChunk) {
    const int cn = n - i0 < kPgChunk ? n - i0 : kPgChunk;
    for (int idx = tid; idx < cn * 15; idx += kPgThreads) {
      const int a = idx / 15, k = idx % 15, i = i0 + a;
      sh[a * 30 + k] = k < 6 ? D[6 * (size_t)i + k] : (i > 1 ? U[9 * (size_t)(i - 1) + (k - 6)] : 0.0);
    }
    __syncthreads();
    if (tid == 0 && *s_ok) {
      for (int a = 0; a < cn; ++a) {
        const double *d = sh + a * 30, *u = d + 6;
        double *o = sh + a * 30 + 15;
        double Lm[9], S[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) Lm[3 * r + c] = (u[r] * Sp[c] + u[3 + r] * Sp[3 + c]) + u[6 + r] * Sp[6 + c];
        const double Dm[9] = {d[0], d[1], d[2], d[1], d[3], d[4], d[2], d[4], d[5]};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = r; c < 3; ++c) {
            S[3 * r + c] = Dm[3 * r + c] - ((Lm[3 * r] * u[c] + Lm[3 * r + 1] * u[3 + c]) + Lm[3 * r + 2] * u[6 + c]);
            S[3 * c + r] = S[3 * r + c];
          }
        if (!pg_spd_inverse(S, d[0], d[3], d[5], Sp)) { *s_ok = 0; break; }
#pragma unroll
        for (int k = 0; k < 9; ++k) o[k] = Lm[k];
        o[9] = Sp[0]; o[10] = Sp[1]; o[11] = Sp[2]; o[12] = Sp[4]; o[13] = Sp[5]; o[14] = Sp[8];
      }
    }
    __syncthreads();
    if (!*s_ok) return false;
    for (int idx = tid; idx < cn * 15; idx += kPgThreads) {
      const int a = idx / 15, k = idx % 15, i = i0 + a;
      const double v = sh[a * 30 + 15 + k];
      if (k < 9) L[9 * (size_t)i + k] = v; else Si[6 * (size_t)i + (k - 9)] = v;
    }
    __syncthreads();
  }
  for (int i = 1 + tid; i < n; i += kPgThreads) {
    const double *s = Si + 6 * (size_t)i, *u = U + 9 * (size_t)i;
    const double Sm[9] = {s[0], s[1], s[2], s[1], s[3], s[4], s[2], s[4], s[5]};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        W[9 * (size_t)i + 3 * r + c] = i + 1 < n ? (Sm[3 * r] * u[c] + Sm[3 * r + 1] * u[3 + c]) + Sm[3 * r + 2] * u[6 + c] : 0.0;
  }
  __syncthreads();
  return true;
}

// One staged piece of a sweep of pg_apply: the nodes i0 .. i0 + cn - 1 of M (L or W) and of `in` into LDS, lane k of wave 0
// takes column k through them (upwards, or downwards for DOWN) as v_i = in_i - M_i c with c the value before, `out` from LDS.
template <int K, bool DOWN>
__device__ __forceinline__ void pg_sweep_chunk(const double *__restrict__ M, const double *in, double *out, int i0, int cn, double c[3],
                                               double *sh) {
  constexpr int K3 = 3 * K, per = 9 + K3;          // doubles of one staged node: M_i, then K triples
  static_assert(per <= 30, "staged in the LDS that pg_factor uses");
  const int tid = (int)threadIdx.x;
  for (int idx = tid; idx < cn * per; idx += kPgThreads) {
    const int k = idx % per, i = i0 + idx / per;
    sh[idx] = k < 9 ? M[9 * (size_t)i + k] : in[(size_t)K3 * i + (k - 9)];
  }
  __syncthreads();
  if (tid < K) {
    for (int t = 0; t < cn; ++t) {
      const double *q = sh + (DOWN ? cn - 1 - t : t) * per;
      double *v = sh + (DOWN ? cn - 1 - t : t) * per + 9 + 3 * tid;
      const double v0 = v[0] - ((q[0] * c[0] + q[1] * c[1]) + q[2] * c[2]);
      const double v1 = v[1] - ((q[3] * c[0] + q[4] * c[1]) + q[5] * c[2]);
      const double v2 = v[2] - ((q[6] * c[0] + q[7] * c[1]) + q[8] * c[2]);
      v[0] = v0; v[1] = v1; v[2] = v2;
      c[0] = v0; c[1] = v1; c[2] = v2;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < cn * K3; idx += kPgThreads) out[(size_t)K3 * (i0 + idx / K3) + idx % K3] = sh[(idx / K3) * per + 9 + idx % K3];
  __syncthreads();
}

// z = T^-1 r with the factor above for K right-hand sides, laid out [node][column][3] (K = 1: the solver's [node][3]):
// y_i = r_i - L_i y_{i-1} upwards, v_i = S_i^-1 y_i, z_i = v_i - W_i z_{i+1} downwards.  Lane k of wave 0 carries column k; every
// lane reads the same L_i / W_i from LDS (a broadcast), so one trip up and one trip down serve all K columns, and a column's
// arithmetic is the same at every K.  Contains barriers: called under block-uniform conditions only.  Ends behind a barrier:
// every thread may read z.
template <int K>
__device__ void pg_apply(const PgWork &Wk, const double *__restrict__ r, double *__restrict__ y, double *__restrict__ z, int n, double *sh) {
  const int tid = (int)threadIdx.x;
  double c[3] = {0.0, 0.0, 0.0};                   // the lane's carry: y_{i-1} of its column, then z_{i+1}
  for (int i0 = 1; i0 < n; i0 += kPgChunk) pg_sweep_chunk<K, false>(Wk.L, r, y, i0, n - i0 < kPgChunk ? n - i0 : kPgChunk, c, sh);
  for (int idx = tid; idx < (n - 1) * K; idx += kPgThreads) {
    const double *s = Wk.Si + 6 * (size_t)(1 + idx / K);
    double *v = y + 3 * ((size_t)K + idx);         // (node 1 + idx / K, column idx % K)
    const double a = v[0], b = v[1], d = v[2];
    v[0] = (s[0] * a + s[1] * b) + s[2] * d;
    v[1] = (s[1] * a + s[3] * b) + s[4] * d;
    v[2] = (s[2] * a + s[4] * b) + s[5] * d;
  }
  __syncthreads();
  c[0] = c[1] = c[2] = 0.0;
  for (int i0 = 1 + (n - 2) / kPgChunk * kPgChunk; i0 >= 1; i0 -= kPgChunk)
    pg_sweep_chunk<K, true>(Wk.W, y, z, i0, n - i0 < kPgChunk ? n - i0 : kPgChunk, c, sh);
}

// ---- what the solver and the marginals share of a graph's set-up and of H p.  The functions that contain a barrier are called
// under block-uniform conditions only: every decision of either kernel comes from the launch's arguments or from block sums
// that all threads hold with the same bits. ----

// The graph's own faults: a pose, rel or info that is not finite, an arc end out of range or a loop on one node, an info that is
// not positive definite, an entry of arc_scalar (the graph's phi or weight, indexed like ed; NULL: none) that is negative or
// not finite.  Nonzero in every thread if any thread found one.  Contains a barrier.
__device__ __forceinline__ int pg_graph_bad(const double *__restrict__ pose, const ndt_pg_edge *__restrict__ ed, int n, int m,
                                            const double *__restrict__ arc_scalar) {
  const int tid = (int)threadIdx.x;
  int bad = 0;
  for (int i = tid; i < n; i += kPgThreads)
    if (!pg_finite(pose[3 * (size_t)i]) || !pg_finite(pose[3 * (size_t)i + 1]) || !pg_finite(pose[3 * (size_t)i + 2])) bad = 1;
  for (int e = tid; e < m; e += kPgThreads) {
    const ndt_pg_edge E = ed[e];
    if (E.from < 0 || E.from >= n || E.to < 0 || E.to >= n || E.from == E.to) bad = 1;
    bool fin = pg_finite(E.rel[0]) && pg_finite(E.rel[1]) && pg_finite(E.rel[2]);
#pragma unroll
    for (int k = 0; k < 6; ++k) fin = fin && pg_finite(E.info[k]);
    const double *I = E.info;
    const double m2 = I[0] * I[3] - I[1] * I[1];
    const double det = (I[0] * (I[3] * I[5] - I[4] * I[4]) + I[1] * (I[4] * I[2] - I[1] * I[5])) + I[2] * (I[1] * I[4] - I[3] * I[2]);
    if (!fin || !(I[0] > 0.0) || !(m2 > 0.0) || !(det > 0.0)) bad = 1;
    if (arc_scalar && (!(arc_scalar[e] >= 0.0) || !pg_finite(arc_scalar[e]))) bad = 1;
  }
  return __syncthreads_or(bad);
}

// Every node's arcs in arc-index order: the keys (node, 2 e + side) of the 2 m arc ends, padded to n2, sorted, then cut at the
// nodes -- node i's arc ends are keys[ptr[i] .. ptr[i + 1]).  Contains barriers (the sort's).  Ends behind none: ptr is written
// last, and the barrier behind the caller's pg_radians is the one that lets every thread read it.
__device__ __forceinline__ void pg_arc_order(const ndt_pg_edge *__restrict__ ed, int n, int m, unsigned n2, unsigned long long *keys, int *ptr) {
  const unsigned tid = threadIdx.x, m2e = 2u * (unsigned)m;
  for (unsigned k = tid; k < n2; k += kPgThreads) {
    unsigned long long key = ~0ull;
    if (k < m2e) { const ndt_pg_edge &E = ed[k >> 1]; key = ((unsigned long long)(unsigned)((k & 1u) ? E.to : E.from) << 32) | k; }
    keys[k] = key;
  }
  __syncthreads();
  for (unsigned kk = 2; kk <= n2; kk <<= 1)
    for (unsigned j = kk >> 1; j > 0; j >>= 1) {
      for (unsigned i = tid; i < n2; i += kPgThreads) {
        const unsigned l = i ^ j;
        if (l > i) {
          const unsigned long long a = keys[i], b = keys[l];
          if ((a > b) == ((i & kk) == 0)) { keys[i] = b; keys[l] = a; }
        }
      }
      __syncthreads();
    }
  for (unsigned k = tid; k <= m2e; k += kPgThreads) {
    const int node = k < m2e ? (int)(keys[k] >> 32) : n;
    const int prev = k > 0 ? (int)(keys[k - 1] >> 32) : -1;
    for (int v = prev + 1; v <= node; ++v) ptr[v] = (int)k;
  }
}

// x = the poses with the heading in radians.  No barrier: the caller's follows.
__device__ __forceinline__ void pg_radians(const double *__restrict__ pose, double *__restrict__ x, int n) {
  for (int i = (int)threadIdx.x; i < n; i += kPgThreads) {
    x[3 * (size_t)i] = pose[3 * (size_t)i]; x[3 * (size_t)i + 1] = pose[3 * (size_t)i + 1];
    x[3 * (size_t)i + 2] = pose[3 * (size_t)i + 2] * (kPgPi / 180.0);
  }
}

// Node i's diagonal block D_i (six entries) and chain block U_i of H from its arc list, the arcs as linearised in Wk.lin; GRAD:
// g3 = its entries of the gradient, summed in the same walk.  ROBUST: every term times the arc's weight (pg_block_add).
template <bool ROBUST, bool GRAD>
__device__ __forceinline__ void pg_node_blocks(const PgWork &Wk, const ndt_pg_edge *__restrict__ ed, int i, double g3[3]) {
  double Dm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Um[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if constexpr (GRAD) { g3[0] = 0.0; g3[1] = 0.0; g3[2] = 0.0; }
  for (int k = Wk.ptr[i]; k < Wk.ptr[i + 1]; ++k) {
    const unsigned slot = (unsigned)Wk.keys[k];
    const int e = (int)(slot >> 1), side = (int)(slot & 1u);
    const PgLin l = Wk.lin[e];
    const double *I = ed[e].info;
    const int other = side ? ed[e].from : ed[e].to;
    double Js[9], Jo[9];
    pg_jac(l, side, Js);
    if constexpr (GRAD) {
      const double rr[3] = {l.r0, l.r1, l.r2};
      double w[3], o[3];
      pg_info_mul(I, rr, w);
      pg_jt_mul(Js, w, o);
      if constexpr (ROBUST) { g3[0] += l.wt * o[0]; g3[1] += l.wt * o[1]; g3[2] += l.wt * o[2]; }
      else { g3[0] += o[0]; g3[1] += o[1]; g3[2] += o[2]; }
    }
    pg_block_add<ROBUST>(Js, I, Js, l.wt, Dm);
    if (other == i + 1) { pg_jac(l, side ^ 1, Jo); pg_block_add<ROBUST>(Js, I, Jo, l.wt, Um); }
  }
  double *d = Wk.D + 6 * (size_t)i;
  d[0] = Dm[0]; d[1] = Dm[1]; d[2] = Dm[2]; d[3] = Dm[4]; d[4] = Dm[5]; d[5] = Dm[8];
  for (int k = 0; k < 9; ++k) Wk.U[9 * (size_t)i + k] = Um[k];
}

// One arc's term of H p at the node whose Jacobian block is Js: q += [wt] Js^T Omega (Js p_i + Jo p_other)
template <bool ROBUST>
__device__ __forceinline__ void pg_arc_hp(const double Js[9], const double Jo[9], const double *__restrict__ I, double wt, const double pi3[3],
                                          const double po3[3], double q[3]) {
  double u1[3], u2[3], w[3], o[3];
  pg_j_mul(Js, pi3, u1); pg_j_mul(Jo, po3, u2);
  const double u[3] = {u1[0] + u2[0], u1[1] + u2[1], u1[2] + u2[2]};
  pg_info_mul(I, u, w);
  pg_jt_mul(Js, w, o);
  if constexpr (ROBUST) { q[0] += wt * o[0]; q[1] += wt * o[1]; q[2] += wt * o[2]; }
  else { q[0] += o[0]; q[1] += o[1]; q[2] += o[2]; }
}

// The record of one graph; the robust record nests it.
__device__ __forceinline__ ndt_pg_result pg_record(double cost_initial, double cost_final, int iterations, int cg_iterations, int converged,
                                                   int status) {
  ndt_pg_result res;
  res.cost_initial = cost_initial; res.cost_final = cost_final; res.iterations = iterations; res.cg_iterations = cg_iterations;
  res.converged = converged; res.status = status;
  return res;
}
__device__ __forceinline__ ndt_pg_robust_result pg_robust_record(const ndt_pg_result &pg, double mu0, int levels, int n_robust, int n_rejected) {
  ndt_pg_robust_result res;
  res.pg = pg; res.mu0 = mu0; res.levels = levels; res.n_robust = n_robust; res.n_rejected = n_rejected; res.pad = 0;
  return res;
}

// What the robust form's launch carries beside the plain one's arguments, and the record either form writes.
template <bool ROBUST> struct PgExtra;
template <> struct PgExtra<false> { typedef ndt_pg_result Record; };
template <> struct PgExtra<true> {
  typedef ndt_pg_robust_result Record;
  PgRobust RP;
  const double *phi;                               // indexed like edges, as the two outputs; each may be NULL
  double *weight_out, *chi2_out;
};

// All Gauss-Newton iterations of every graph of the call: workgroup w takes the graphs w, w + gridDim.x, ...  One body for both
// forms.  ROBUST = false is ndt_pg_optimize_batch: no extra argument, X is empty and out holds ndt_pg_result.  ROBUST = true is
// ndt_pg_optimize_robust_batch (graduated non-convexity, the header's contract): out holds ndt_pg_robust_result.  Every level decision is taken from
// block sums and maxima, which every thread holds with the same bits: control flow stays uniform around the barriers.
template <bool ROBUST, typename... Extra>
__global__ void __launch_bounds__(kPgThreads)
pg_solve_kernel(double *__restrict__ poses, const ndt_pg_edge *__restrict__ edges, const PgRow *__restrict__ rows, int n_graphs,
                PgParams P, unsigned char *__restrict__ scratch, typename PgExtra<ROBUST>::Record *__restrict__ out, Extra... extra) {
  static_assert(sizeof...(Extra) == (ROBUST ? 1 : 0), "the robust form takes one PgExtra<true>, the plain form nothing");
  const PgExtra<ROBUST> X{extra...};                 // (the plain form's argument list is ndt_pg_optimize_batch's own, unchanged)
  __shared__ double sh[kPgChunk * 30];
  __shared__ double s_w[4];
  __shared__ int s_ok;
  const int tid = (int)threadIdx.x;
  for (int gi = (int)blockIdx.x; gi < n_graphs; gi += (int)gridDim.x) {
    const PgRow R = rows[gi];
    const int n = R.n, m = R.m;
    double *pose = poses + 3 * R.node0;
    const ndt_pg_edge *ed = edges + R.edge0;
    const double *gphi = nullptr;                              // the graph's own phi, as ed its arcs
    double *weight_out = nullptr, *chi2_out = nullptr;
    if constexpr (ROBUST) { gphi = X.phi ? X.phi + R.edge0 : nullptr; weight_out = X.weight_out; chi2_out = X.chi2_out; }
    // ---- the graph's own faults: found here, the poses stay as they are ----
    const int bad = pg_graph_bad(pose, ed, n, m, gphi);
    if (bad || m == 0) {
      if constexpr (ROBUST)
        for (int e = tid; e < m; e += kPgThreads) {              // (a faulted graph's arc outputs are 0)
          if (weight_out) weight_out[R.edge0 + e] = 0.0;
          if (chi2_out) chi2_out[R.edge0 + e] = 0.0;
        }
      if (tid == 0) {
        const ndt_pg_result res = pg_record(0.0, 0.0, 0, 0, bad ? 0 : 1, bad ? NDT_E_ARG : NDT_OK);
        if constexpr (ROBUST) out[gi] = pg_robust_record(res, bad ? 0.0 : 1.0, bad ? 0 : 1, 0, 0);
        else out[gi] = res;
      }
      continue;
    }
    double *base = reinterpret_cast<double *>(scratch + R.scratch);
    const PgLayout Y((size_t)n, (size_t)m, (size_t)R.n2);
    double *x = base + Y.x, *xt = base + Y.xt, *g = base + Y.g, *dl = base + Y.dl, *r = base + Y.r, *z = base + Y.z, *p = base + Y.p,
           *q = base + Y.q, *y = base + Y.y;
    const PgWork Wk(base, Y);
    const unsigned long long *keys = Wk.keys;
    const int *ptr = Wk.ptr;
    PgLin *lin = Wk.lin;
    // ---- every node's arcs in arc-index order, the poses in radians; node 0's entries of the solver's vectors stay zero ----
    pg_arc_order(ed, n, m, R.n2, Wk.keys, Wk.ptr);
    pg_radians(pose, x, n);
    if (tid < 3) { g[tid] = 0.0; dl[tid] = 0.0; r[tid] = 0.0; z[tid] = 0.0; p[tid] = 0.0; q[tid] = 0.0; y[tid] = 0.0; }
    __syncthreads();
    // ---- the robust form's start: the robust arcs counted, mu0 = max(1, 2 max c_e / phi_e) over them unless it is given ----
    double mu = 1.0, mu_start = 1.0;
    int levels = 1, in_level = 0, n_robust = 0;
    if constexpr (ROBUST) {
      double cnt = 0.0, mx = 0.0;
      if (gphi)
        for (int e = tid; e < m; e += kPgThreads) {
          const double ph = gphi[e];
          if (ph > 0.0) { cnt += 1.0; mx = fmax(mx, pg_chi2(pg_linearise(x, ed[e]), ed[e].info) / ph); }
        }
      n_robust = (int)pg_block_sum(cnt, s_w);                    // (a sum of small whole numbers: exact in any order)
      mx = pg_block_max(mx, s_w);
      if (n_robust > 0) mu_start = X.RP.mu0 != 0.0 ? X.RP.mu0 : fmin(kPgMuMax, fmax(1.0, 2.0 * mx));
      mu = mu_start;
    }
    double F = pg_cost<ROBUST>(x, ed, m, s_w, gphi, 1.0);
    const double F0 = F;
    if constexpr (ROBUST)
      if (mu > 1.0) F = pg_cost<true>(x, ed, m, s_w, gphi, mu);
    int iters = 0, cg_total = 0, conv = 0;
    const int cg_cap = P.cg_max_iter > 0 ? P.cg_max_iter : 6 * n;
    for (int it = 0; it < P.max_iter; ++it) {
      // ---- linearise: the arcs, then every node's gradient, diagonal block and chain block ----
      for (int e = tid; e < m; e += kPgThreads) {
        PgLin l = pg_linearise(x, ed[e]);
        if constexpr (ROBUST) {
          const double ph = gphi ? gphi[e] : 0.0;
          l.wt = ph > 0.0 ? pg_weight(pg_chi2(l, ed[e].info), mu * ph) : 1.0;
        }
        lin[e] = l;
      }
      __syncthreads();
      for (int i = 1 + tid; i < n; i += kPgThreads) {
        double gi3[3];
        pg_node_blocks<ROBUST, true>(Wk, ed, i, gi3);
        for (int k = 0; k < 3; ++k) { g[3 * (size_t)i + k] = gi3[k]; dl[3 * (size_t)i + k] = 0.0; r[3 * (size_t)i + k] = -gi3[k]; }
      }
      __syncthreads();
      if (!pg_factor(Wk.D, Wk.U, Wk.L, Wk.Si, Wk.W, n, sh, &s_ok)) break;
      pg_apply<1>(Wk, r, y, z, n, sh);
      double acc = 0.0;
      for (int i = 1 + tid; i < n; i += kPgThreads)
        for (int k = 0; k < 3; ++k) { const double zv = z[3 * (size_t)i + k]; p[3 * (size_t)i + k] = zv; acc += r[3 * (size_t)i + k] * zv; }
      double rz = pg_block_sum(acc, s_w);
      if (!(rz >= 0.0) || !pg_finite(rz)) break;
      bool cg_bad = false;
      if (rz > 0.0) {
        const double rz0 = rz;
        for (int k = 0; k < cg_cap; ++k) {
          // q = H p, a node's arcs in arc-index order (p of node 0 is zero: its columns are removed)
          acc = 0.0;
          for (int i = 1 + tid; i < n; i += kPgThreads) {
            double qi[3] = {0, 0, 0};
            const double pi3[3] = {p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]};
            for (int kk = ptr[i]; kk < ptr[i + 1]; ++kk) {
              const unsigned slot = (unsigned)keys[kk];
              const int e = (int)(slot >> 1), side = (int)(slot & 1u);
              const PgLin l = lin[e];
              const int other = side ? ed[e].from : ed[e].to;
              const double po[3] = {p[3 * (size_t)other], p[3 * (size_t)other + 1], p[3 * (size_t)other + 2]};
              double Js[9], Jo[9];
              pg_jac(l, side, Js); pg_jac(l, side ^ 1, Jo);
              pg_arc_hp<ROBUST>(Js, Jo, ed[e].info, l.wt, pi3, po, qi);
            }
            for (int c = 0; c < 3; ++c) { q[3 * (size_t)i + c] = qi[c]; acc += pi3[c] * qi[c]; }
          }
          const double pq = pg_block_sum(acc, s_w);
          cg_total++;
          if (!(pq > 0.0) || !pg_finite(pq)) { cg_bad = true; break; }
          const double alpha = rz / pq;
          for (int i = 1 + tid; i < n; i += kPgThreads)
            for (int c = 0; c < 3; ++c) { dl[3 * (size_t)i + c] += alpha * p[3 * (size_t)i + c]; r[3 * (size_t)i + c] -= alpha * q[3 * (size_t)i + c]; }
          __syncthreads();
          pg_apply<1>(Wk, r, y, z, n, sh);
          acc = 0.0;
          for (int i = 1 + tid; i < n; i += kPgThreads)
            for (int c = 0; c < 3; ++c) acc += r[3 * (size_t)i + c] * z[3 * (size_t)i + c];
          const double rzn = pg_block_sum(acc, s_w);
          if (!(rzn >= 0.0) || !pg_finite(rzn)) { cg_bad = true; break; }
          if (sqrt(rzn) <= P.cg_rtol * sqrt(rz0)) break;
          const double beta = rzn / rz;
          rz = rzn;
          for (int i = 1 + tid; i < n; i += kPgThreads)
            for (int c = 0; c < 3; ++c) p[3 * (size_t)i + c] = z[3 * (size_t)i + c] + beta * p[3 * (size_t)i + c];
          __syncthreads();
        }
      }
      if (cg_bad) break;
      // ---- the step: taken only if F does not rise, halved otherwise ----
      double dmax = 0.0;
      for (int i = 1 + tid; i < n; i += kPgThreads)
        for (int c = 0; c < 3; ++c) dmax = fmax(dmax, fabs(dl[3 * (size_t)i + c]));
      dmax = pg_block_max(dmax, s_w);                            // (NaN entries of d drop out here and fail the cost test)
      double s = 1.0, Ft = F;
      bool accepted = false;
      for (int h = 0; h <= P.max_halvings; ++h) {
        if (h) s *= 0.5;
        for (int i = tid; i < n; i += kPgThreads)
          for (int c = 0; c < 3; ++c) xt[3 * (size_t)i + c] = x[3 * (size_t)i + c] + s * dl[3 * (size_t)i + c];
        __syncthreads();
        Ft = pg_cost<ROBUST>(xt, ed, m, s_w, gphi, mu);
        if (pg_finite(Ft) && Ft <= F) { accepted = true; break; }
      }
      dmax *= s;                                                 // the step taken, or the last one tried
      if constexpr (ROBUST)
        if (mu > 1.0) {
          // a level above 1 never ends the run: it ends on a short accepted step, on level_iter of them, or where the halving
          // runs out; the next level starts from the same poses with F evaluated again at its own mu
          bool end_level = true;
          if (accepted) {
            for (int i = 1 + tid; i < n; i += kPgThreads)
              for (int c = 0; c < 3; ++c) x[3 * (size_t)i + c] = xt[3 * (size_t)i + c];
            __syncthreads();
            F = Ft;
            iters++;
            in_level++;
            end_level = dmax < X.RP.eps_level || in_level >= X.RP.level_iter;
          }
          if (end_level) {
            mu = fmax(1.0, mu / X.RP.factor);
            levels++;
            in_level = 0;
            F = pg_cost<true>(x, ed, m, s_w, gphi, mu);
          }
          continue;
        }
      if (!accepted) {
        // the halving ran out below eps_step: halving on could only give a step that is shorter still -- the poses stay
        if (pg_finite(dmax) && dmax < P.eps_step) conv = 1;
        break;
      }
      for (int i = 1 + tid; i < n; i += kPgThreads)
        for (int c = 0; c < 3; ++c) x[3 * (size_t)i + c] = xt[3 * (size_t)i + c];
      __syncthreads();                                           // (the next linearisation reads every node's x)
      F = Ft;
      iters++;
      if (dmax < P.eps_step) { conv = 1; break; }
    }
    __syncthreads();
    // ---- out: the last accepted poses (node 0 and an unmoved graph keep their bytes), the record ----
    if (iters > 0)
      for (int i = 1 + tid; i < n; i += kPgThreads) {
        pose[3 * (size_t)i] = x[3 * (size_t)i]; pose[3 * (size_t)i + 1] = x[3 * (size_t)i + 1];
        pose[3 * (size_t)i + 2] = pg_wrap_deg(x[3 * (size_t)i + 2] * (180.0 / kPgPi));
      }
    if constexpr (ROBUST) {
      // ---- the final pass: every arc's c and weight at mu = 1 at the last poses, the rejected arcs counted, F_1 there ----
      double cnt = 0.0;
      for (int e = tid; e < m; e += kPgThreads) {
        const double c = pg_chi2(pg_linearise(x, ed[e]), ed[e].info), ph = gphi ? gphi[e] : 0.0;
        if (ph > 0.0 && c > ph) cnt += 1.0;
        if (weight_out) weight_out[R.edge0 + e] = ph > 0.0 ? pg_weight(c, ph) : 1.0;
        if (chi2_out) chi2_out[R.edge0 + e] = c;
      }
      const int n_rejected = (int)pg_block_sum(cnt, s_w);
      if (mu > 1.0) F = pg_cost<true>(x, ed, m, s_w, gphi, 1.0);     // (the run ended inside a level)
      if (tid == 0) out[gi] = pg_robust_record(pg_record(F0, F, iters, cg_total, conv, NDT_OK), mu_start, levels, n_robust, n_rejected);
    } else if (tid == 0) {
      out[gi] = pg_record(F0, F, iters, cg_total, conv, NDT_OK);
    }
    __syncthreads();
  }
}

// ---- ndt_pg_marginals_batch: blocks of H^-1 at the poses given (the contract is the header's) ----
// A query (graph, a, b) is the three unit columns of each of its free nodes solved against the one factor: K = 3 or 6
// right-hand sides that share every H p walk and every block-Thomas sweep (pg_apply<K>).  The vectors are laid out
// [node][column][3]; a column's arithmetic is the same instructions in every slot and touches no other column's numbers, so its
// solution is a function of (graph, weights, node, column) alone.

constexpr int kPgCols = 6;                         // columns of one query at the most: two free nodes

// The regions of one workgroup's scratch slot: the vectors are sized for kPgCols columns.
struct PgMLayout : PgTail {
  size_t xr, r, z, p, q, y, x;
  __host__ __device__ PgMLayout(size_t n, size_t m, size_t n2) {
    const size_t v = 3 * (size_t)kPgCols * n;
    size_t o = 0;
    xr = o; o += 3 * n; r = o; o += v; z = o; o += v; p = o; o += v; q = o; o += v; y = o; o += v; x = o; o += v;
    static_cast<PgTail &>(*this) = PgTail::at(o, n, m, n2);
  }
};

// pg_apply at the query's column count (block-uniform).
__device__ __forceinline__ void pg_apply_cols(int K, const PgWork &Wk, const double *r, double *y, double *z, int n, double *sh) {
  if (K == 3) pg_apply<3>(Wk, r, y, z, n, sh); else pg_apply<kPgCols>(Wk, r, y, z, n, sh);
}

// One query's record: the blocks as given (NULL: zeros), the counters.
__device__ void pg_marginal_write(ndt_pg_marginal *__restrict__ o, const double *Saa, const double *Sab, const double *Sbb, int cg_iterations,
                                  int converged, int status) {
  for (int k = 0; k < 9; ++k) { o->Saa[k] = Saa ? Saa[k] : 0.0; o->Sab[k] = Sab ? Sab[k] : 0.0; o->Sbb[k] = Sbb ? Sbb[k] : 0.0; }
  o->cg_iterations = cg_iterations; o->converged = converged; o->status = status; o->pad = 0;
}
// The diagonal block of node `node` from the solves of its own columns (slot: its first column): every pair averaged.
__device__ void pg_marginal_diag(const double *__restrict__ x, int K, int node, int slot, double S[9]) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) S[3 * r + c] = x[((size_t)node * K + slot + c) * 3 + r];
  S[1] = S[3] = 0.5 * (S[1] + S[3]); S[2] = S[6] = 0.5 * (S[2] + S[6]); S[5] = S[7] = 0.5 * (S[5] + S[7]);
}

// Workgroup w takes the queries w, w + gridDim.x, ... in its own scratch slot (slot_bytes each, for the largest queried graph).
// The set-up of a query is the solver's own functions at the poses given (pg_graph_bad, pg_arc_order, pg_radians,
// pg_node_blocks<true, no gradient>), the arc weights as given in PgLin::wt; the conjugate gradients are the solver's loop
// around pg_arc_hp and pg_apply<K> with one alpha, beta, r^T z and stop flag per column.  A column that has stopped is frozen; every decision is
// taken from block sums, which every thread holds with the same bits: control flow stays uniform around the barriers.
__global__ void __launch_bounds__(kPgThreads)
pg_marginal_kernel(const double *__restrict__ poses, const ndt_pg_edge *__restrict__ edges, const PgRow *__restrict__ rows, int n_graphs,
                   const double *__restrict__ weight, const ndt_pg_query *__restrict__ queries, int n_queries, int cg_max_iter, double cg_rtol,
                   unsigned char *__restrict__ scratch, unsigned long long slot_bytes, ndt_pg_marginal *__restrict__ out) {
  __shared__ double sh[kPgChunk * 30];
  __shared__ double s_wk[4 * kPgCols];
  __shared__ int s_ok;
  const int tid = (int)threadIdx.x;
  double *base = reinterpret_cast<double *>(scratch + (unsigned long long)blockIdx.x * slot_bytes);
  for (int qi = (int)blockIdx.x; qi < n_queries; qi += (int)gridDim.x) {
    const ndt_pg_query Q = queries[qi];
    if (Q.graph < 0 || Q.graph >= n_graphs) {
      if (tid == 0) pg_marginal_write(out + qi, nullptr, nullptr, nullptr, 0, 0, NDT_E_ARG);
      continue;
    }
    const PgRow R = rows[Q.graph];
    const int n = R.n, m = R.m;
    const double *pose = poses + 3 * R.node0;
    const ndt_pg_edge *ed = edges + R.edge0;
    const double *gw = weight ? weight + R.edge0 : nullptr;
    // ---- the query's own faults and the graph's (a weight that is negative or not finite among them) ----
    int bad = pg_graph_bad(pose, ed, n, m, gw);
    if (Q.a < 0 || Q.a >= n || Q.b < 0 || Q.b >= n) bad = 1;
    if (!bad && m == 0 && (Q.a != 0 || Q.b != 0)) bad = 1;       // (nothing ties the node to node 0)
    // ---- the free nodes whose columns are solved: a, then b unless it is a again; a block with node 0 is exactly 0 ----
    const int na = Q.a != 0 ? 1 : 0, nb = (Q.b != 0 && Q.b != Q.a) ? 1 : 0;
    const int K = 3 * (na + nb);
    if (bad || K == 0) {
      if (tid == 0) pg_marginal_write(out + qi, nullptr, nullptr, nullptr, 0, bad ? 0 : 1, bad ? NDT_E_ARG : NDT_OK);
      continue;
    }
    const int node0 = na ? Q.a : Q.b, node1 = Q.b;             // the node of the columns 0 .. 2, of the columns 3 .. 5
    const int K3 = 3 * K;
    const PgMLayout Y((size_t)n, (size_t)m, (size_t)R.n2);
    double *xr = base + Y.xr, *r = base + Y.r, *z = base + Y.z, *p = base + Y.p, *q = base + Y.q, *y = base + Y.y, *x = base + Y.x;
    const PgWork Wk(base, Y);
    const unsigned long long *keys = Wk.keys;
    const int *ptr = Wk.ptr;
    PgLin *lin = Wk.lin;
    // ---- the arc order, the poses in radians (read only), the arcs linearised there with their weights, every node's D and U ----
    pg_arc_order(ed, n, m, R.n2, Wk.keys, Wk.ptr);
    pg_radians(pose, xr, n);
    __syncthreads();
    for (int e = tid; e < m; e += kPgThreads) {
      PgLin l = pg_linearise(xr, ed[e]);
      l.wt = gw ? gw[e] : 1.0;
      lin[e] = l;
    }
    __syncthreads();
    for (int i = 1 + tid; i < n; i += kPgThreads) pg_node_blocks<true, false>(Wk, ed, i, nullptr);
    __syncthreads();
    if (!pg_factor(Wk.D, Wk.U, Wk.L, Wk.Si, Wk.W, n, sh, &s_ok)) {
      if (tid == 0) pg_marginal_write(out + qi, nullptr, nullptr, nullptr, 0, 0, NDT_OK);
      __syncthreads();
      continue;
    }
    // ---- the right-hand sides: column k is the unit vector of entry k % 3 of its node; node 0's entries stay zero ----
    for (int i = tid; i < n; i += kPgThreads)
      for (int k = 0; k < K; ++k) {
        const int node = k < 3 ? node0 : node1;
        for (int c = 0; c < 3; ++c) {
          const size_t at = ((size_t)i * K + k) * 3 + c;
          r[at] = (i == node && c == k % 3) ? 1.0 : 0.0;
          x[at] = 0.0;
          if (i == 0) { z[at] = 0.0; p[at] = 0.0; q[at] = 0.0; y[at] = 0.0; }
        }
      }
    __syncthreads();
    pg_apply_cols(K, Wk, r, y, z, n, sh);
    double rz[kPgCols], rz0[kPgCols], coef[kPgCols], acc[kPgCols];
    bool act[kPgCols], ok[kPgCols];
    int its[kPgCols];
#pragma unroll
    for (int k = 0; k < kPgCols; ++k) acc[k] = 0.0;
    for (int i = 1 + tid; i < n; i += kPgThreads)
#pragma unroll
      for (int k = 0; k < kPgCols; ++k)
        if (k < K)
          for (int c = 0; c < 3; ++c) {
            const size_t at = ((size_t)i * K + k) * 3 + c;
            const double zv = z[at];
            p[at] = zv; acc[k] += r[at] * zv;
          }
    pg_block_sum_cols<kPgCols>(acc, s_wk);
    bool any = false;
#pragma unroll
    for (int k = 0; k < kPgCols; ++k) {
      rz[k] = acc[k]; rz0[k] = acc[k]; coef[k] = 0.0; its[k] = 0;
      ok[k] = k >= K || (rz[k] > 0.0 && pg_finite(rz[k]));      // (T is positive definite: r0^T z0 of a unit column is above 0)
      act[k] = k < K && ok[k];
      any = any || act[k];
    }
    const int cg_cap = cg_max_iter > 0 ? cg_max_iter : 6 * n;
    for (int it = 0; it < cg_cap && any; ++it) {
      // q = H p of the columns still running: a node's arcs in arc-index order, each arc's Jacobians applied to every column
#pragma unroll
      for (int k = 0; k < kPgCols; ++k) acc[k] = 0.0;
      for (int i = 1 + tid; i < n; i += kPgThreads) {
        double qv[kPgCols][3];
#pragma unroll
        for (int k = 0; k < kPgCols; ++k) { qv[k][0] = 0.0; qv[k][1] = 0.0; qv[k][2] = 0.0; }
        const double *pi = p + (size_t)i * K3;
        for (int kk = ptr[i]; kk < ptr[i + 1]; ++kk) {
          const unsigned slot = (unsigned)keys[kk];
          const int e = (int)(slot >> 1), side = (int)(slot & 1u);
          const PgLin l = lin[e];
          const double *I = ed[e].info;
          const int other = side ? ed[e].from : ed[e].to;
          const double *po = p + (size_t)other * K3;
          double Js[9], Jo[9];
          pg_jac(l, side, Js); pg_jac(l, side ^ 1, Jo);
#pragma unroll
          for (int k = 0; k < kPgCols; ++k)
            if (act[k]) {
              const double pi3[3] = {pi[3 * k], pi[3 * k + 1], pi[3 * k + 2]}, po3[3] = {po[3 * k], po[3 * k + 1], po[3 * k + 2]};
              pg_arc_hp<true>(Js, Jo, I, l.wt, pi3, po3, qv[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < kPgCols; ++k)
          if (act[k])
            for (int c = 0; c < 3; ++c) { q[(size_t)i * K3 + 3 * k + c] = qv[k][c]; acc[k] += pi[3 * k + c] * qv[k][c]; }
      }
      pg_block_sum_cols<kPgCols>(acc, s_wk);
#pragma unroll
      for (int k = 0; k < kPgCols; ++k)
        if (act[k]) {
          its[k]++;
          if (!(acc[k] > 0.0) || !pg_finite(acc[k])) { act[k] = false; ok[k] = false; }     // (a CG breakdown)
          else coef[k] = rz[k] / acc[k];
        }
      for (int i = 1 + tid; i < n; i += kPgThreads)
#pragma unroll
        for (int k = 0; k < kPgCols; ++k)
          if (act[k])
            for (int c = 0; c < 3; ++c) {
              const size_t at = (size_t)i * K3 + 3 * k + c;
              x[at] += coef[k] * p[at]; r[at] -= coef[k] * q[at];
            }
      __syncthreads();
      pg_apply_cols(K, Wk, r, y, z, n, sh);
#pragma unroll
      for (int k = 0; k < kPgCols; ++k) acc[k] = 0.0;
      for (int i = 1 + tid; i < n; i += kPgThreads)
#pragma unroll
        for (int k = 0; k < kPgCols; ++k)
          if (act[k])
            for (int c = 0; c < 3; ++c) { const size_t at = (size_t)i * K3 + 3 * k + c; acc[k] += r[at] * z[at]; }
      pg_block_sum_cols<kPgCols>(acc, s_wk);
      any = false;
#pragma unroll
      for (int k = 0; k < kPgCols; ++k)
        if (act[k]) {
          if (!(acc[k] >= 0.0) || !pg_finite(acc[k])) { act[k] = false; ok[k] = false; }
          else if (sqrt(acc[k]) <= cg_rtol * sqrt(rz0[k])) act[k] = false;                    // (the column has met the rule)
          else { coef[k] = acc[k] / rz[k]; rz[k] = acc[k]; any = true; }
        }
      for (int i = 1 + tid; i < n; i += kPgThreads)
#pragma unroll
        for (int k = 0; k < kPgCols; ++k)
          if (act[k])
            for (int c = 0; c < 3; ++c) { const size_t at = (size_t)i * K3 + 3 * k + c; p[at] = z[at] + coef[k] * p[at]; }
      __syncthreads();
    }
    // ---- out: all three blocks or none -- every column has to have met the rule ----
    int conv = 1, cg_most = 0;
#pragma unroll
    for (int k = 0; k < kPgCols; ++k) {
      if (!ok[k] || act[k]) conv = 0;
      cg_most = its[k] > cg_most ? its[k] : cg_most;
    }
    if (tid == 0) {
      if (!conv) {
        pg_marginal_write(out + qi, nullptr, nullptr, nullptr, cg_most, 0, NDT_OK);
      } else {
        double Saa[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Sab[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Sbb[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        const int slot_b = (na && nb) ? 3 : 0;                   // b's first column (a's is 0)
        if (na) pg_marginal_diag(x, K, Q.a, 0, Saa);
        if (Q.b != 0) pg_marginal_diag(x, K, Q.b, slot_b, Sbb);
        if (na && Q.b != 0)
          for (int rr = 0; rr < 3; ++rr)
            for (int c = 0; c < 3; ++c) Sab[3 * rr + c] = Q.a == Q.b ? Saa[3 * rr + c] : x[((size_t)Q.a * K + slot_b + c) * 3 + rr];
        pg_marginal_write(out + qi, Saa, Sab, Sbb, cg_most, 1, NDT_OK);
      }
    }
    __syncthreads();
  }
}

// remakeMaps' point correction (src/PointCloudMap.cpp:147-154): q = oldPose.relativePoint(p), p' = newPose.globalPoint(q)
// (src/Pose2D.cpp:46-59) with Rmat as Pose2D::calRmat builds it, fp64 without contraction, rounded once to float32.
// ReposeMove: what one (old, new) pose pair gives every point of its segment; repose_point: the per-point body -- the one
// statement of the arithmetic, for repose_points_kernel and the session set's repose_rows_kernel (ndt_sessions.hip.h).
struct ReposeMove {
  double tx1, ty1, o00, o01, o10, o11;             // oldPose and its Rmat
  double tx2, ty2, n00, n01, n10, n11;             // newPose and its Rmat
  bool same;                                       // the pair is bit-equal: the segment keeps its bytes
};

__device__ __forceinline__ ReposeMove repose_move(const double *po, const double *pn) {
  ReposeMove M;
  M.same = __double_as_longlong(po[0]) == __double_as_longlong(pn[0]) && __double_as_longlong(po[1]) == __double_as_longlong(pn[1]) &&
           __double_as_longlong(po[2]) == __double_as_longlong(pn[2]);
  const double a1 = po[2] * M_PI / 180, a2 = pn[2] * M_PI / 180;
  const double c1 = cos(a1), s1 = sin(a1), c2 = cos(a2), s2 = sin(a2);
  M.tx1 = po[0]; M.ty1 = po[1]; M.tx2 = pn[0]; M.ty2 = pn[1];
  M.o00 = c1; M.o01 = -s1; M.o10 = s1; M.o11 = c1;
  M.n00 = c2; M.n01 = -s2; M.n10 = s2; M.n11 = c2;
  return M;
}

__device__ __forceinline__ float2 repose_point(const ReposeMove &M, float fx, float fy) {
  const double dx = (double)fx - M.tx1, dy = (double)fy - M.ty1;
  const double lx = dx * M.o00 + dy * M.o10;
  const double ly = dx * M.o01 + dy * M.o11;
  const double gx = M.n00 * lx + M.n01 * ly + M.tx2;
  const double gy = M.n10 * lx + M.n11 * ly + M.ty2;
  return make_float2((float)gx, (float)gy);
}

// One thread per point; a segment per blockIdx.y, as scan_to_map_kernel takes its scans.  A segment whose poses are bit-equal
// is copied through (left alone when out is xy itself).
__global__ void __launch_bounds__(256)
repose_points_kernel(const unsigned char *__restrict__ xy, size_t stride, const unsigned long long *__restrict__ offsets, int n_segs,
                     const double *__restrict__ old_poses, const double *__restrict__ new_poses, unsigned char *__restrict__ out,
                     size_t out_stride) {
  for (int b = blockIdx.y; b < n_segs; b += gridDim.y) {
    const unsigned long long r0 = offsets[b], r1 = offsets[b + 1];
    if (r0 >= r1) continue;
    const ReposeMove M = repose_move(old_poses + 3 * (size_t)b, new_poses + 3 * (size_t)b);
    if (M.same && out == xy && out_stride == stride) continue;
    for (unsigned long long i = r0 + blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < r1;
         i += (unsigned long long)gridDim.x * blockDim.x) {
      const float *src = reinterpret_cast<const float *>(xy + i * stride);
      float *dst = reinterpret_cast<float *>(out + i * out_stride);
      const float fx = src[0], fy = src[1];
      if (M.same) { dst[0] = fx; dst[1] = fy; continue; }
      const float2 g = repose_point(M, fx, fy);
      dst[0] = g.x; dst[1] = g.y;
    }
  }
}
