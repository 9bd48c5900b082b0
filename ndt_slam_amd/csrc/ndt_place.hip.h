// Place recognition (ndt_place_*, ndt_sessions_place_candidates): a rotation-invariant descriptor of a cloud
// about a centre -- n_rings words of 64 sector bits -- and the all-pairs match of descriptors over the 64 rotations, each as a
// host definition and as a device form that equals it to the byte.  Included behind ndt_cross.hip.h (one translation unit).
// Three kernels:
//   place_describe_kernel   per descriptor: the cloud streamed once, n_rings x 64 counters in LDS, a ring's word = one ballot
//   place_match_kernel      per (four queries, a tile of items): lane = shift; a wave holds ITS query rotated right by its lane in
//                           registers, so an entry staged in LDS costs an AND and a popcount per half word; an item's hit = one
//                           wave maximum of (key << 32 | ~(desc << 6 | shift))
//   place_pick_kernel       per query: its top_k items, by top_k workgroup maxima over the query's row of the table
// A point's r2 is formed by explicitly rounded operations on the device and with contraction off on the host (the whole file
// is); everything behind the cell of a point is integer work.

namespace {

__host__ __device__ inline double pl_sub(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsub_rn(a, b);
#else
  return a - b;
#endif
}
__host__ __device__ inline double pl_mul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dmul_rn(a, b);
#else
  return a * b;
#endif
}
__host__ __device__ inline double pl_add(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dadd_rn(a, b);
#else
  return a + b;
#endif
}

struct PlGeom { double rmin2; double e2[NDT_PLACE_MAX_RINGS]; };      // r_min^2; e2[j - 1] = edge2[j] (0 behind n_rings)
struct PlRow { unsigned long long addr, n; double cx, cy; };           // a descriptor: its cloud's first point (a device address), how many, its centre
constexpr int kPlBlock = 256;
constexpr int kPlTileItems = 64;                                       // items of one match job
constexpr int kPlStage = 128;                                          // entries in LDS at a time
constexpr uint64_t kPlMaxDesc = 1ull << 26, kPlMaxPairs = (1ull << 31) - 1;

// THE DEFINITION of a point's offsets and r2, and whether the point counts (include/ndt_mi355x.h); outer2 = edge2[n_rings].
__host__ __device__ inline bool pl_point(float x, float y, double cx, double cy, double rmin2, double outer2, double *dx, double *dy, double *r2) {
  *dx = pl_sub((double)x, cx); *dy = pl_sub((double)y, cy);
  *r2 = pl_add(pl_mul(*dx, *dx), pl_mul(*dy, *dy));
  return fabs(*r2) <= DBL_MAX && !(*r2 < rmin2) && !(*r2 >= outer2);
}

// ... and of its sector: comparisons only.
__host__ __device__ inline int pl_sector(double dx, double dy) {
  constexpr double T[7] = NDT_PLACE_TAN;
  const double ax = fabs(dx), ay = fabs(dy), a = ax > ay ? ax : ay, b = ax > ay ? ay : ax;
  int sub = 0;
#pragma unroll
  for (int j = 0; j < 7; ++j) sub += b >= pl_mul(T[j], a) ? 1 : 0;
  const int s16 = ay > ax ? 15 - sub : sub;
  return dx >= 0 ? (dy >= 0 ? s16 : 63 - s16) : (dy >= 0 ? 31 - s16 : 32 + s16);
}

// Workgroup k, k + gridDim.x, ...: descriptor k.  The ring of a point is the first j with r2 < e2[j] (the edges ascend): found from
// a float estimate by steps that end exactly there whatever the estimate was.
__global__ void __launch_bounds__(kPlBlock)
place_describe_kernel(const PlGeom *__restrict__ geom, const PlRow *__restrict__ rows, int n_desc, unsigned stride, int n_rings, unsigned min_pts,
                      float inv_w, unsigned long long *__restrict__ desc) {
  __shared__ unsigned cnt[NDT_PLACE_MAX_RINGS * NDT_PLACE_SECTORS];
  __shared__ double e2[NDT_PLACE_MAX_RINGS];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t < n_rings) e2[t] = geom->e2[t];
  const double rmin2 = geom->rmin2;
  for (int k = blockIdx.x; k < n_desc; k += gridDim.x) {
    const PlRow R = rows[k];
    for (int c = t; c < n_rings * NDT_PLACE_SECTORS; c += kPlBlock) cnt[c] = 0;
    __syncthreads();
    const double outer2 = e2[n_rings - 1];
    for (unsigned long long i = t; i < R.n; i += kPlBlock) {
      const float *p = reinterpret_cast<const float *>(R.addr + i * stride);
      double dx, dy, r2;
      if (!pl_point(p[0], p[1], R.cx, R.cy, rmin2, outer2, &dx, &dy, &r2)) continue;
      int j = (int)fminf(fmaxf(sqrtf((float)r2) * inv_w, 0.f), (float)(n_rings - 1));
      while (j > 0 && r2 < e2[j - 1]) --j;
      while (j < n_rings - 1 && r2 >= e2[j]) ++j;
      atomicAdd(&cnt[j * NDT_PLACE_SECTORS + pl_sector(dx, dy)], 1u);
    }
    __syncthreads();
    for (int r = wave; r < n_rings; r += kPlBlock / 64) {
      const unsigned long long w = __ballot(cnt[r * NDT_PLACE_SECTORS + lane] >= min_pts);
      if (lane == 0) desc[(size_t)k * n_rings + r] = w;
    }
    __syncthreads();
  }
}

// num / den for num <= 2^27 and 1 <= den <= 2^12: a float estimate (within one of the quotient), then the exact remainder decides.
__device__ __forceinline__ unsigned pl_div(unsigned num, unsigned den) {
  unsigned k = (unsigned)((float)num * __builtin_amdgcn_rcpf((float)den));
  int r = (int)num - (int)(k * den);
  while (r < 0) { --k; r += (int)den; }
  while (r >= (int)den) { ++k; r -= (int)den; }
  return k;
}

__device__ __forceinline__ unsigned long long pl_wave_max(unsigned long long x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long y = __shfl_xor(x, o); x = y > x ? y : x; }
  return x;
}

// Job j = (query group j / n_tiles, item tile j % n_tiles); workgroup b takes the jobs b, b + gridDim.x, ...  Wave w of the
// workgroup is query 4 * group + w: lane s keeps rotr64(Q_r, s) -- popcount(Q_r & rotl64(D_r, s)) = popcount(rotr64(Q_r, s) & D_r)
// -- for r < NR (zero from n_rings on), so the four waves share the staged entries and nothing crosses a wave but an item's
// maximum.  For one entry the key rises strictly with c (a step of c moves it by 65536 / den >= 16), so a lane's running
// (key, lowest descriptor) is the lane's maximum of the composite over the item's entries.
template <int NR>
__global__ void __launch_bounds__(kPlBlock)
place_match_kernel(const unsigned long long *__restrict__ qd, const int *__restrict__ qg, int n_q, const unsigned long long *__restrict__ dd,
                   const int *__restrict__ item_first, const int *__restrict__ item_group, int n_items, int n_rings, unsigned n_tiles,
                   unsigned long long n_jobs, unsigned long long *__restrict__ table) {
  constexpr int NRP = NR + 1;                                          // (a row's pitch in words: thread e sums row e without bank conflicts)
  __shared__ unsigned long long sd[kPlStage * NRP];
  __shared__ int snb[kPlStage];
  __shared__ int sfirst[kPlTileItems + 1], sgroup[kPlTileItems];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (unsigned long long job = blockIdx.x; job < n_jobs; job += gridDim.x) {
    const int i0 = (int)(job % n_tiles) * kPlTileItems, ni = min(kPlTileItems, n_items - i0);
    const long long q = (long long)(job / n_tiles) * (kPlBlock / 64) + wave;
    const bool live = q < n_q;
    unsigned qlo[NR], qhi[NR];
    int na = 0;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const unsigned long long w = live && r < n_rings ? qd[(size_t)q * n_rings + r] : 0ull;
      na += __popcll(w);
      const unsigned long long v = (w >> lane) | (w << ((64 - lane) & 63));
      qlo[r] = (unsigned)v; qhi[r] = (unsigned)(v >> 32);
    }
    const int own = live ? qg[q] : -1;
    __syncthreads();
    for (int i = t; i <= ni; i += kPlBlock) sfirst[i] = item_first[i0 + i];
    for (int i = t; i < ni; i += kPlBlock) sgroup[i] = item_group[i0 + i];
    __syncthreads();
    const int D0 = sfirst[0], D1 = sfirst[ni];
    int cur = 0, bd = D0;
    unsigned bkey = 0;
    // item `cur` of the tile is complete: its maximum to the table, the next item's start
    auto flush = [&]() {
      unsigned long long comp = 0;
      if (sfirst[cur + 1] > sfirst[cur] && !(own >= 0 && own == sgroup[cur]))
        comp = pl_wave_max(((unsigned long long)bkey << 32) | (0xFFFFFFFFu - (((unsigned)bd << 6) | (unsigned)lane)));
      if (live && lane == 0) table[(size_t)q * n_items + i0 + cur] = comp;
      ++cur; bkey = 0; bd = sfirst[cur];
    };
    for (int base = D0; base < D1; base += kPlStage) {
      const int cnt = min(kPlStage, D1 - base);
      __syncthreads();
      for (int idx = t; idx < cnt * NR; idx += kPlBlock) {
        const int e = idx / NR, r = idx - e * NR;
        sd[e * NRP + r] = r < n_rings ? dd[(size_t)(base + e) * n_rings + r] : 0ull;
      }
      __syncthreads();
      if (t < cnt) {
        int nb = 0;
#pragma unroll
        for (int r = 0; r < NR; ++r) nb += __popcll(sd[t * NRP + r]);
        snb[t] = nb;
      }
      __syncthreads();
      for (int e = 0; e < cnt; ++e) {
        const int d = base + e;
        while (d >= sfirst[cur + 1]) flush();                          // (d < D1 = sfirst[ni]: ends with cur < ni)
        if (own >= 0 && own == sgroup[cur]) continue;
        const unsigned long long *row = sd + e * NRP;
        int c = 0;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const unsigned long long w = row[r];
          c += __popc((unsigned)w & qlo[r]) + __popc((unsigned)(w >> 32) & qhi[r]);
        }
        const int den = na + snb[e] - c;
        const unsigned key = den ? pl_div((unsigned)c << 16, (unsigned)den) : 0u;
        if (key > bkey) { bkey = key; bd = d; }
      }
    }
    while (cur < ni) flush();
  }
}

// Workgroup q, q + gridDim.x, ...: query q.  Round j takes the largest composite below round j - 1's among the row's entries
// with key >= min_key -- the composites of a row differ (an item's descriptors are its own) --, and the one thread that holds it
// writes the hit, with the three counts formed again for that (entry, shift).
__global__ void __launch_bounds__(kPlBlock)
place_pick_kernel(const unsigned long long *__restrict__ table, const unsigned long long *__restrict__ qd, const unsigned long long *__restrict__ dd,
                  int n_q, int n_items, int n_rings, unsigned min_key, int top_k, ndt_place_hit *__restrict__ out, int *__restrict__ n_out) {
  __shared__ unsigned long long swin[kPlBlock / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int q = blockIdx.x; q < n_q; q += gridDim.x) {
    const unsigned long long *row = table + (size_t)q * n_items;
    unsigned long long prev = ~0ull;
    int n = 0;
    for (; n < top_k; ++n) {
      unsigned long long best = 0;
      int bi = -1;
      for (int i = t; i < n_items; i += kPlBlock) {
        const unsigned long long v = row[i];
        if (v < prev && v > best && (unsigned)(v >> 32) >= min_key) { best = v; bi = i; }
      }
      const unsigned long long w = pl_wave_max(best);
      if (lane == 0) swin[wave] = w;
      __syncthreads();
      unsigned long long win = swin[0];
#pragma unroll
      for (int k = 1; k < kPlBlock / 64; ++k) win = swin[k] > win ? swin[k] : win;
      __syncthreads();
      if (!win) break;
      if (bi >= 0 && best == win) {
        const unsigned low = 0xFFFFFFFFu - (unsigned)win;
        const int d = (int)(low >> 6), s = (int)(low & 63u);
        int c = 0, na = 0, nb = 0;
        for (int r = 0; r < n_rings; ++r) {
          const unsigned long long Q = qd[(size_t)q * n_rings + r], D = dd[(size_t)d * n_rings + r];
          c += __popcll(Q & ((D << s) | (D >> ((64 - s) & 63)))); na += __popcll(Q); nb += __popcll(D);
        }
        out[(size_t)q * top_k + n] = ndt_place_hit{bi, d, s, (int)(win >> 32), c, na, nb, n};
      }
      prev = win;
    }
    if (t >= n && t < top_k) out[(size_t)q * top_k + t] = ndt_place_hit{0, 0, 0, 0, 0, 0, 0, 0};
    if (t == 0) n_out[q] = n;
  }
}

#define PL_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

bool pl_finite(double v) { return std::fabs(v) <= DBL_MAX; }

// A parameter outside its range: the refusal names it.
int place_check_params(ndt_ctx *ctx, const std::string &f, const ndt_place_params &p) {
  const char *bad = !(pl_finite(p.ring_width) && p.ring_width > 0) ? "ring_width (finite, > 0)"
                  : !(pl_finite(p.r_min) && p.r_min >= 0) ? "r_min (finite, >= 0)"
                  : p.n_rings < 1 || p.n_rings > NDT_PLACE_MAX_RINGS ? "n_rings (1 .. 32)"
                  : p.min_pts < 1 ? "min_pts (>= 1)"
                  : p.min_key < 1 || p.min_key > 65536 ? "min_key (1 .. 65536)"
                  : p.top_k < 1 || p.top_k > NDT_PLACE_MAX_TOP_K ? "top_k (1 .. 16)"
                  : p.centre_stride < 1 ? "centre_stride (>= 1)"
                  : p.reserved ? "reserved (0)" : nullptr;
  return bad ? fail(ctx, NDT_E_ARG, f + ": " + bad) : NDT_OK;
}

PlGeom place_geom(const ndt_place_params &p) {
  PlGeom g{};
  g.rmin2 = p.r_min * p.r_min;
  for (int j = 1; j <= p.n_rings; ++j) { const double e = (double)j * p.ring_width; g.e2[j - 1] = e * e; }
  return g;
}

// THE DEFINITION of the descriptor (the arguments checked by the caller).
void place_describe_host(const unsigned char *xy, size_t n, size_t stride, double cx, double cy, const ndt_place_params &p, uint64_t *desc) {
  const PlGeom g = place_geom(p);
  std::vector<uint32_t> cnt((size_t)p.n_rings * NDT_PLACE_SECTORS, 0u);
  for (size_t i = 0; i < n; ++i) {
    float v[2];
    memcpy(v, xy + i * stride, sizeof(v));
    double dx, dy, r2;
    if (!pl_point(v[0], v[1], cx, cy, g.rmin2, g.e2[p.n_rings - 1], &dx, &dy, &r2)) continue;
    int ring = 0;
    for (int j = 0; j < p.n_rings; ++j) ring += r2 >= g.e2[j] ? 1 : 0;
    cnt[(size_t)ring * NDT_PLACE_SECTORS + (size_t)pl_sector(dx, dy)]++;
  }
  for (int r = 0; r < p.n_rings; ++r) {
    uint64_t w = 0;
    for (int s = 0; s < NDT_PLACE_SECTORS; ++s) w |= (uint64_t)(cnt[(size_t)r * NDT_PLACE_SECTORS + (size_t)s] >= (uint32_t)p.min_pts) << s;
    desc[r] = w;
  }
}

// THE DEFINITION of the key.
struct PlKey { int key, c, na, nb; };
PlKey place_key_host(const uint64_t *Q, const uint64_t *D, int n_rings, int s) {
  PlKey k{0, 0, 0, 0};
  for (int r = 0; r < n_rings; ++r) {
    const uint64_t rot = s ? (D[r] << s) | (D[r] >> (64 - s)) : D[r];
    k.c += __builtin_popcountll(Q[r] & rot); k.na += __builtin_popcountll(Q[r]); k.nb += __builtin_popcountll(D[r]);
  }
  const uint32_t den = (uint32_t)(k.na + k.nb - k.c);
  k.key = den ? (int)(((uint32_t)k.c * 65536u) / den) : 0;
  return k;
}

// THE DEFINITION of the match (the arguments checked by the caller); table may be NULL.
void place_match_host(const uint64_t *qd, const int *qg, int n_q, const uint64_t *dd, const int *item_first, const int *item_group, int n_items,
                      const ndt_place_params &p, uint64_t *table, ndt_place_hit *out, int *n_out) {
  const size_t R = (size_t)p.n_rings, K = (size_t)p.top_k;
  std::vector<uint64_t> row((size_t)n_items);
  for (int q = 0; q < n_q; ++q) {
    const uint64_t *Q = qd + (size_t)q * R;
    for (int i = 0; i < n_items; ++i) {
      uint64_t best = 0;
      if (!(qg[q] >= 0 && qg[q] == item_group[i]))
        for (int d = item_first[i]; d < item_first[i + 1]; ++d)
          for (int s = 0; s < NDT_PLACE_SECTORS; ++s) {
            const uint64_t comp = ((uint64_t)place_key_host(Q, dd + (size_t)d * R, p.n_rings, s).key << 32) | (0xFFFFFFFFu - (((uint32_t)d << 6) | (uint32_t)s));
            best = std::max(best, comp);
          }
      row[(size_t)i] = best;
    }
    if (table) std::copy(row.begin(), row.end(), table + (size_t)q * (size_t)n_items);
    ndt_place_hit *o = out + (size_t)q * K;
    memset(o, 0, K * sizeof(ndt_place_hit));
    uint64_t prev = ~0ull;
    int n = 0;
    for (; n < p.top_k; ++n) {
      uint64_t win = 0; int wi = -1;
      for (int i = 0; i < n_items; ++i)
        if (row[(size_t)i] < prev && row[(size_t)i] > win && (row[(size_t)i] >> 32) >= (uint64_t)p.min_key) { win = row[(size_t)i]; wi = i; }
      if (wi < 0) break;
      const uint32_t low = 0xFFFFFFFFu - (uint32_t)win;
      const int d = (int)(low >> 6), s = (int)(low & 63u);
      const PlKey k = place_key_host(Q, dd + (size_t)d * R, p.n_rings, s);
      o[n] = ndt_place_hit{wi, d, s, k.key, k.c, k.na, k.nb, n};
      prev = win;
    }
    n_out[q] = n;
  }
}

// The refusals of the describe forms behind their NULL checks.
int place_describe_check(ndt_ctx *ctx, const std::string &f, size_t stride, const uint64_t *offsets, int n_clouds, const double *centres,
                         const int *cloud_of, int n_desc, const ndt_place_params &p) {
  PL_TRY(place_check_params(ctx, f, p));
  if (stride != 8 && stride != 16) return fail(ctx, NDT_E_ARG, f + ": stride_bytes must be 8 or 16");
  if (n_clouds < 0 || n_desc < 0) return fail(ctx, NDT_E_ARG, f + ": n_clouds or n_desc < 0");
  if ((uint64_t)n_desc > kPlMaxDesc) return fail(ctx, NDT_E_ARG, f + ": more than 2^26 descriptors");
  for (int c = 0; c < n_clouds; ++c) {
    if (offsets[c + 1] < offsets[c]) return fail(ctx, NDT_E_ARG, f + ": cloud " + std::to_string(c) + ": offsets decrease");
    if (offsets[c + 1] - offsets[c] > 0xFFFFFFFFull) return fail(ctx, NDT_E_ARG, f + ": cloud " + std::to_string(c) + ": more than 2^32 - 1 points");
  }
  for (int k = 0; k < n_desc; ++k) {
    if (!pl_finite(centres[2 * (size_t)k]) || !pl_finite(centres[2 * (size_t)k + 1]))
      return fail(ctx, NDT_E_ARG, f + ": descriptor " + std::to_string(k) + ": the centre is not finite");
    if (cloud_of[k] < 0 || cloud_of[k] >= n_clouds)
      return fail(ctx, NDT_E_ARG, f + ": descriptor " + std::to_string(k) + ": cloud_of is outside [0, n_clouds)");
  }
  return NDT_OK;
}

// ... and of the match forms.
int place_match_check(ndt_ctx *ctx, const std::string &f, int n_q, const int *item_first, int n_items, const ndt_place_params &p) {
  PL_TRY(place_check_params(ctx, f, p));
  if (n_q < 0 || n_items < 0) return fail(ctx, NDT_E_ARG, f + ": n_q or n_items < 0");
  if (item_first[0] != 0) return fail(ctx, NDT_E_ARG, f + ": item_first[0] is not 0");
  for (int i = 0; i < n_items; ++i)
    if (item_first[i + 1] < item_first[i]) return fail(ctx, NDT_E_ARG, f + ": item " + std::to_string(i) + ": item_first decreases");
  if ((uint64_t)item_first[n_items] > kPlMaxDesc) return fail(ctx, NDT_E_ARG, f + ": more than 2^26 descriptors");
  if ((uint64_t)n_q * (uint64_t)n_items > kPlMaxPairs) return fail(ctx, NDT_E_ARG, f + ": more than 2^31 - 1 (query, item) pairs");
  return NDT_OK;
}

unsigned place_grid(const ndt_ctx *ctx, uint64_t jobs) {
  return (unsigned)std::min<uint64_t>(jobs, ctx->workgroups > 0 ? (uint64_t)ctx->workgroups : 0x7fffffffull);
}

// The describe launch (n_desc >= 1): geom and rows are in device memory.
int place_queue_describe(ndt_ctx *ctx, hipStream_t st, const PlGeom *geom, const PlRow *rows, int n_desc, size_t stride, const ndt_place_params &p,
                         uint64_t *desc) {
  place_describe_kernel<<<place_grid(ctx, (uint64_t)n_desc), kPlBlock, 0, st>>>(geom, rows, n_desc, (unsigned)stride, p.n_rings, (unsigned)p.min_pts,
                                                                                (float)(1.0 / p.ring_width), (unsigned long long *)desc);
  HIP_TRY(ctx, hipGetLastError());
  return NDT_OK;
}

// The two match launches (n_q >= 1): the groups and items are in device memory, `table` has n_q x n_items words.
int place_queue_match(ndt_ctx *ctx, hipStream_t st, const uint64_t *qd, const int *qg, int n_q, const uint64_t *dd, const int *item_first,
                      const int *item_group, int n_items, const ndt_place_params &p, uint64_t *table, ndt_place_hit *out, int *n_out) {
  const unsigned n_tiles = (unsigned)(((size_t)n_items + kPlTileItems - 1) / kPlTileItems);
  const unsigned long long n_jobs = (unsigned long long)n_tiles * (unsigned long long)(((size_t)n_q + kPlBlock / 64 - 1) / (kPlBlock / 64));
  if (n_jobs) {
    const dim3 grid(place_grid(ctx, n_jobs));
#define PL_LAUNCH(NR) place_match_kernel<NR><<<grid, kPlBlock, 0, st>>>((const unsigned long long *)qd, qg, n_q, (const unsigned long long *)dd, item_first, \
                                                                       item_group, n_items, p.n_rings, n_tiles, n_jobs, (unsigned long long *)table)
    switch ((p.n_rings + 7) / 8) {
      case 1: PL_LAUNCH(8); break;
      case 2: PL_LAUNCH(16); break;
      case 3: PL_LAUNCH(24); break;
      default: PL_LAUNCH(32); break;
    }
#undef PL_LAUNCH
    HIP_TRY(ctx, hipGetLastError());
  }
  place_pick_kernel<<<place_grid(ctx, (uint64_t)n_q), kPlBlock, 0, st>>>((const unsigned long long *)table, (const unsigned long long *)qd,
                                                                        (const unsigned long long *)dd, n_q, n_items, p.n_rings, (unsigned)p.min_key,
                                                                        p.top_k, out, n_out);
  HIP_TRY(ctx, hipGetLastError());
  return NDT_OK;
}

// ndt_place_describe_batch_dev behind its refusals (n_desc >= 1), inside the caller's frame: the table, its upload, the launch.
int place_describe_dev(ndt_ctx *ctx, hipStream_t st, const float *xy_dev, size_t stride, const uint64_t *offsets, const double *centres,
                       const int *cloud_of, int n_desc, const ndt_place_params &p, uint64_t *desc_dev) {
  Regions U;
  const size_t o_geom = U.take(sizeof(PlGeom), 256), o_rows = U.take((size_t)n_desc * sizeof(PlRow), 256);
  PL_TRY(ctx->pld_tab.reserve(ctx, U.end));
  PL_TRY(ctx->d_pld.ensure(ctx, U.end));
  unsigned char *h = ctx->pld_tab.h.p, *d = ctx->d_pld.p;
  *Regions::at<PlGeom>(h, o_geom) = place_geom(p);
  PlRow *rows = Regions::at<PlRow>(h, o_rows);
  for (int k = 0; k < n_desc; ++k) {
    const uint64_t a = offsets[cloud_of[k]], e = offsets[cloud_of[k] + 1];
    rows[k] = PlRow{(unsigned long long)(uintptr_t)xy_dev + a * stride, e - a, centres[2 * (size_t)k], centres[2 * (size_t)k + 1]};
  }
  HIP_TRY(ctx, ctx->pld_tab.upload(d, 0, U.end, st));
  return place_queue_describe(ctx, st, Regions::at<PlGeom>(d, o_geom), Regions::at<PlRow>(d, o_rows), n_desc, stride, p, desc_dev);
}

// ndt_place_match_dev behind its refusals (n_q >= 1), inside the caller's frame: the table, its upload, the two launches.
int place_match_dev(ndt_ctx *ctx, hipStream_t st, const uint64_t *qd, const int *q_group, int n_q, const uint64_t *dd, const int *item_first,
                    const int *item_group, int n_items, const ndt_place_params &p, uint64_t *table_dev, ndt_place_hit *out_dev, int *n_out_dev) {
  Regions U;
  const size_t o_qg = U.take((size_t)n_q * sizeof(int), 256), o_first = U.take(((size_t)n_items + 1) * sizeof(int), 256),
               o_group = U.take((size_t)n_items * sizeof(int), 256), up = U.end;
  const size_t o_table = table_dev ? 0 : U.take((size_t)n_q * (size_t)n_items * 8, 256);
  PL_TRY(ctx->plm_tab.reserve(ctx, up));
  PL_TRY(ctx->d_plm.ensure(ctx, U.end));
  unsigned char *h = ctx->plm_tab.h.p, *d = ctx->d_plm.p;
  memcpy(h + o_qg, q_group, (size_t)n_q * sizeof(int));
  memcpy(h + o_first, item_first, ((size_t)n_items + 1) * sizeof(int));
  if (n_items) memcpy(h + o_group, item_group, (size_t)n_items * sizeof(int));
  HIP_TRY(ctx, ctx->plm_tab.upload(d, 0, up, st));
  return place_queue_match(ctx, st, qd, Regions::at<int>(d, o_qg), n_q, dd, Regions::at<int>(d, o_first), Regions::at<int>(d, o_group), n_items, p,
                           table_dev ? table_dev : Regions::at<uint64_t>(d, o_table), out_dev, n_out_dev);
}

// ndt_sessions_place_candidates behind the set's bracket and the refusals.
int place_set_candidates(ndt_sessions *s, const SetCall &call, const unsigned char *which, const unsigned char *against, const ndt_place_params &p,
                         ndt_place_candidate *out, int *n_out) {
  ndt_ctx *ctx = s->ctx;
  *n_out = 0;
  ndt_sessions_stats stats{};
  struct Item { int ses, m; };
  struct Centre { int scan; };
  std::vector<Item> items;
  std::vector<int> item_first{0}, item_group, q_group, who;
  std::vector<Centre> centres;
  std::vector<PlRow> rows;
  for (int i = 0; i < s->S; ++i) {
    const SsSession &Q = s->ses[(size_t)i];
    if ((against && !against[i]) || !Q.started || Q.n_poses < 1 || Q.n_closed < 1) continue;
    for (int m = 0; m < Q.n_closed; ++m) {
      const int first = Q.sub_first[(size_t)m], last = Q.sub_first[(size_t)m + 1] - 1;
      const uint64_t a = Q.closed_off[(size_t)m], n = Q.closed_off[(size_t)m + 1] - a;
      if (!n || last < first) continue;
      for (long long k = first; k <= last; k += p.centre_stride) {
        rows.push_back(PlRow{(unsigned long long)(uintptr_t)(Q.closed.p + a), n, Q.traj[3 * (size_t)k], Q.traj[3 * (size_t)k + 1]});
        centres.push_back(Centre{(int)k});
      }
      items.push_back(Item{i, m}); item_group.push_back(i); item_first.push_back((int)rows.size());
      if (rows.size() > kPlMaxDesc) return call.refuse("more than 2^26 descriptors");
    }
  }
  const size_t nD = rows.size(), nI = items.size();
  for (int i = 0; i < s->S; ++i) {
    const SsSession &Q = s->ses[(size_t)i];
    if ((which && !which[i]) || !Q.started || Q.n_poses < 1 || !Q.has_target || !Q.t_n) continue;
    const double *L = Q.traj.data() + 3 * ((size_t)Q.n_poses - 1);
    rows.push_back(PlRow{(unsigned long long)(uintptr_t)(s->target[Q.buf].p + Q.t_off), Q.t_n, L[0], L[1]});
    q_group.push_back(i); who.push_back(i);
  }
  const size_t nQ = who.size(), K = (size_t)p.top_k, R = (size_t)p.n_rings;
  if (!nQ || !nI) { s->stats = stats; return NDT_OK; }
  if ((uint64_t)nQ * nI > kPlMaxPairs) return call.refuse("more than 2^31 - 1 (query, item) pairs");
  CallFrame fr(ctx);
  PL_TRY(fr.open());
  hipStream_t st = fr.st;
  Regions U;      // the table, then the scratch behind it in the same block
  const size_t o_geom = U.take(sizeof(PlGeom), 256), o_rows = U.take(rows.size() * sizeof(PlRow), 256), o_qg = U.take(nQ * sizeof(int), 256),
               o_first = U.take((nI + 1) * sizeof(int), 256), o_group = U.take(nI * sizeof(int), 256), up = U.end;
  const size_t o_desc = U.take(rows.size() * R * 8, 256), o_table = U.take(nQ * nI * 8, 256), o_out = U.take(nQ * K * sizeof(ndt_place_hit), 256),
               o_nout = U.take(nQ * sizeof(int), 4), back = U.end - o_out;
  PL_TRY(ctx->plm_tab.reserve(ctx, up));
  PL_TRY(ctx->d_plm.ensure(ctx, U.end));
  PL_TRY(ctx->h_pl.ensure(ctx, back));
  unsigned char *h = ctx->plm_tab.h.p, *d = ctx->d_plm.p;
  *Regions::at<PlGeom>(h, o_geom) = place_geom(p);
  memcpy(h + o_rows, rows.data(), rows.size() * sizeof(PlRow));
  memcpy(h + o_qg, q_group.data(), nQ * sizeof(int));
  memcpy(h + o_first, item_first.data(), (nI + 1) * sizeof(int));
  memcpy(h + o_group, item_group.data(), nI * sizeof(int));
  HIP_TRY(ctx, ctx->plm_tab.upload(d, 0, up, st));
  uint64_t *desc = Regions::at<uint64_t>(d, o_desc);
  PL_TRY(place_queue_describe(ctx, st, Regions::at<PlGeom>(d, o_geom), Regions::at<PlRow>(d, o_rows), (int)rows.size(), sizeof(float2), p, desc));
  PL_TRY(place_queue_match(ctx, st, desc + nD * R, Regions::at<int>(d, o_qg), (int)nQ, desc, Regions::at<int>(d, o_first), Regions::at<int>(d, o_group),
                           (int)nI, p, Regions::at<uint64_t>(d, o_table), Regions::at<ndt_place_hit>(d, o_out), Regions::at<int>(d, o_nout)));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_pl.p, d + o_out, back, hipMemcpyDeviceToHost, st));
  PL_TRY(fr.close_and_wait());
  stats.host_waits = 1; stats.h2d_bytes = up; stats.d2h_bytes = back;
  const ndt_place_hit *hits = (const ndt_place_hit *)ctx->h_pl.p;
  const int *cnt = (const int *)(ctx->h_pl.p + (o_nout - o_out));
  int n = 0;
  for (size_t j = 0; j < nQ; ++j) {
    if (cnt[j] < 0 || cnt[j] > p.top_k) return fail(ctx, NDT_E_HIP, call.f + ": the device match returned a count outside its range");
    const SsSession &Q = s->ses[(size_t)who[j]];
    const double th = Q.traj[3 * ((size_t)Q.n_poses - 1) + 2];
    for (int r = 0; r < cnt[j]; ++r) {
      const ndt_place_hit &H = hits[j * K + (size_t)r];
      if (H.item < 0 || (size_t)H.item >= nI || H.desc < item_first[(size_t)H.item] || H.desc >= item_first[(size_t)H.item + 1])
        return fail(ctx, NDT_E_HIP, call.f + ": the device match returned a hit outside its table");
      const Item &I = items[(size_t)H.item];
      const int scan = centres[(size_t)H.desc].scan;
      const SsSession &T = s->ses[(size_t)I.ses];
      ndt_place_candidate c;
      memset(&c, 0, sizeof(c));
      c.session = who[j]; c.map_session = I.ses; c.submap = I.m; c.centre_scan = scan; c.shift = H.shift; c.key = H.key; c.overlap = H.overlap;
      c.n_query = H.n_query; c.n_entry = H.n_entry; c.rank = H.rank;
      c.guess[0] = T.traj[3 * (size_t)scan]; c.guess[1] = T.traj[3 * (size_t)scan + 1]; c.guess[2] = th - (double)H.shift * 5.625;
      out[n++] = c;
    }
  }
  *n_out = n;
  s->stats = stats;
  return NDT_OK;
}

// The host forms' device copies: regions of d_pl_host.
int place_host_block(ndt_ctx *ctx, const Regions &U) { return ctx->d_pl_host.ensure(ctx, U.end); }

}  // namespace

extern "C" {

int ndt_place_default_params(ndt_place_params *p) {
  if (!p) return fail(nullptr, NDT_E_ARG, "ndt_place_default_params: NULL pointer");
  memset(p, 0, sizeof(*p));
  p->ring_width = 0.5; p->r_min = 0.25; p->n_rings = 20; p->min_pts = 1; p->min_key = 1; p->top_k = 4; p->centre_stride = 1;
  return NDT_OK;
}

int ndt_place_describe(const float *xy_host, size_t n, size_t stride_bytes, double cx, double cy, const ndt_place_params *p, uint64_t *desc_host) {
  const std::string f("ndt_place_describe");
  if (!p || !desc_host || (n && !xy_host)) return fail(nullptr, NDT_E_ARG, f + ": NULL pointer");
  const uint64_t off[2] = {0, (uint64_t)n};
  const double centre[2] = {cx, cy};
  const int cloud_of = 0;
  PL_TRY(place_describe_check(nullptr, f, stride_bytes, off, 1, centre, &cloud_of, 1, *p));
  place_describe_host((const unsigned char *)xy_host, n, stride_bytes, cx, cy, *p, desc_host);
  return NDT_OK;
}

int ndt_place_describe_batch_dev(ndt_ctx *ctx, const float *xy_dev, size_t stride_bytes, const uint64_t *offsets_host, int n_clouds,
                                 const double *centres_host, const int *cloud_of_host, int n_desc, const ndt_place_params *p,
                                 uint64_t *desc_dev, void *stream) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  const std::string f("ndt_place_describe_batch_dev");
  if (!p || !offsets_host || (n_desc > 0 && (!centres_host || !cloud_of_host || !desc_dev))) return fail(ctx, NDT_E_ARG, f + ": NULL pointer");
  PL_TRY(place_describe_check(ctx, f, stride_bytes, offsets_host, n_clouds, centres_host, cloud_of_host, n_desc, *p));
  if (n_clouds > 0 && offsets_host[n_clouds] > offsets_host[0] && !xy_dev) return fail(ctx, NDT_E_ARG, f + ": NULL pointer");
  if (ctx->pending_map) return refuse_pending(ctx, f);
  if (!n_desc) return NDT_OK;
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {
    return place_describe_dev(ctx, st, xy_dev, stride_bytes, offsets_host, centres_host, cloud_of_host, n_desc, *p, desc_dev);
  });
}

int ndt_place_describe_batch(ndt_ctx *ctx, const float *xy_host, size_t stride_bytes, const uint64_t *offsets_host, int n_clouds,
                             const double *centres_host, const int *cloud_of_host, int n_desc, const ndt_place_params *p,
                             uint64_t *desc_host) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  const std::string f("ndt_place_describe_batch");
  if (!p || !offsets_host || (n_desc > 0 && (!centres_host || !cloud_of_host || !desc_host))) return fail(ctx, NDT_E_ARG, f + ": NULL pointer");
  PL_TRY(place_describe_check(ctx, f, stride_bytes, offsets_host, n_clouds, centres_host, cloud_of_host, n_desc, *p));
  const uint64_t a = n_clouds > 0 ? offsets_host[0] : 0, e = n_clouds > 0 ? offsets_host[n_clouds] : 0;
  if (e > a && !xy_host) return fail(ctx, NDT_E_ARG, f + ": NULL pointer");
  if (ctx->pending_map) return refuse_pending(ctx, f);
  if (!n_desc) return NDT_OK;
  CallFrame fr(ctx);
  PL_TRY(fr.open());
  Regions U;
  const size_t o_xy = U.take((size_t)(e - a) * stride_bytes, 256), words = (size_t)n_desc * (size_t)p->n_rings, o_desc = U.take(words * 8, 256);
  PL_TRY(place_host_block(ctx, U));
  unsigned char *d = ctx->d_pl_host.p;
  if (e > a) HIP_TRY(ctx, hipMemcpyAsync(d + o_xy, (const unsigned char *)xy_host + a * stride_bytes, (size_t)(e - a) * stride_bytes, hipMemcpyHostToDevice, fr.st));
  const std::vector<uint64_t> rel = rel_offsets(offsets_host, (size_t)n_clouds);
  PL_TRY(place_describe_dev(ctx, fr.st, (const float *)(d + o_xy), stride_bytes, rel.data(), centres_host, cloud_of_host, n_desc, *p,
                            Regions::at<uint64_t>(d, o_desc)));
  HIP_TRY(ctx, hipMemcpyAsync(desc_host, d + o_desc, words * 8, hipMemcpyDeviceToHost, fr.st));
  return fr.close_and_wait();
}

int ndt_place_key(const uint64_t *q_desc, const uint64_t *d_desc, int n_rings, int shift, int *key, int *overlap) {
  const std::string f("ndt_place_key");
  if (!q_desc || !d_desc || !key) return fail(nullptr, NDT_E_ARG, f + ": NULL pointer");
  if (n_rings < 1 || n_rings > NDT_PLACE_MAX_RINGS) return fail(nullptr, NDT_E_ARG, f + ": n_rings (1 .. 32)");
  if (shift < 0 || shift >= NDT_PLACE_SECTORS) return fail(nullptr, NDT_E_ARG, f + ": shift (0 .. 63)");
  const PlKey k = place_key_host(q_desc, d_desc, n_rings, shift);
  *key = k.key;
  if (overlap) *overlap = k.c;
  return NDT_OK;
}

int ndt_place_match_host(const uint64_t *q_desc, const int *q_group, int n_q, const uint64_t *d_desc, const int *item_first,
                         const int *item_group, int n_items, const ndt_place_params *p, uint64_t *table, ndt_place_hit *out, int *n_out) {
  const std::string f("ndt_place_match_host");
  if (!p || !item_first || (n_q > 0 && (!q_desc || !q_group || !out || !n_out)) || (n_items > 0 && !item_group))
    return fail(nullptr, NDT_E_ARG, f + ": NULL pointer");
  PL_TRY(place_match_check(nullptr, f, n_q, item_first, n_items, *p));
  if (n_items > 0 && item_first[n_items] > 0 && !d_desc) return fail(nullptr, NDT_E_ARG, f + ": NULL pointer");
  place_match_host(q_desc, q_group, n_q, d_desc, item_first, item_group, n_items, *p, table, out, n_out);
  return NDT_OK;
}

int ndt_place_match_dev(ndt_ctx *ctx, const uint64_t *q_desc_dev, const int *q_group_host, int n_q, const uint64_t *d_desc_dev,
                        const int *item_first_host, const int *item_group_host, int n_items, const ndt_place_params *p,
                        uint64_t *table_dev, ndt_place_hit *out_dev, int *n_out_dev, void *stream) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  const std::string f("ndt_place_match_dev");
  if (!p || !item_first_host || (n_q > 0 && (!q_desc_dev || !q_group_host || !out_dev || !n_out_dev)) || (n_items > 0 && !item_group_host))
    return fail(ctx, NDT_E_ARG, f + ": NULL pointer");
  PL_TRY(place_match_check(ctx, f, n_q, item_first_host, n_items, *p));
  if (n_items > 0 && item_first_host[n_items] > 0 && !d_desc_dev) return fail(ctx, NDT_E_ARG, f + ": NULL pointer");
  if (ctx->pending_map) return refuse_pending(ctx, f);
  if (!n_q) return NDT_OK;
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {
    return place_match_dev(ctx, st, q_desc_dev, q_group_host, n_q, d_desc_dev, item_first_host, item_group_host, n_items, *p, table_dev, out_dev, n_out_dev);
  });
}

int ndt_place_match(ndt_ctx *ctx, const uint64_t *q_desc_host, const int *q_group_host, int n_q, const uint64_t *d_desc_host,
                    const int *item_first_host, const int *item_group_host, int n_items, const ndt_place_params *p, uint64_t *table_host,
                    ndt_place_hit *out_host, int *n_out_host) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  const std::string f("ndt_place_match");
  if (!p || !item_first_host || (n_q > 0 && (!q_desc_host || !q_group_host || !out_host || !n_out_host)) || (n_items > 0 && !item_group_host))
    return fail(ctx, NDT_E_ARG, f + ": NULL pointer");
  PL_TRY(place_match_check(ctx, f, n_q, item_first_host, n_items, *p));
  const size_t nD = n_items > 0 ? (size_t)item_first_host[n_items] : 0;
  if (nD && !d_desc_host) return fail(ctx, NDT_E_ARG, f + ": NULL pointer");
  if (ctx->pending_map) return refuse_pending(ctx, f);
  if (!n_q) return NDT_OK;
  const size_t R = (size_t)p->n_rings, K = (size_t)p->top_k, Q = (size_t)n_q, I = (size_t)n_items;
  CallFrame fr(ctx);
  PL_TRY(fr.open());
  Regions U;
  const size_t o_q = U.take(Q * R * 8, 256), o_d = U.take(nD * R * 8, 256), o_table = U.take(Q * I * 8, 256),
               o_out = U.take(Q * K * sizeof(ndt_place_hit), 256), o_n = U.take(Q * sizeof(int), 256);
  PL_TRY(place_host_block(ctx, U));
  unsigned char *d = ctx->d_pl_host.p;
  HIP_TRY(ctx, hipMemcpyAsync(d + o_q, q_desc_host, Q * R * 8, hipMemcpyHostToDevice, fr.st));
  if (nD) HIP_TRY(ctx, hipMemcpyAsync(d + o_d, d_desc_host, nD * R * 8, hipMemcpyHostToDevice, fr.st));
  PL_TRY(place_match_dev(ctx, fr.st, Regions::at<uint64_t>(d, o_q), q_group_host, n_q, Regions::at<uint64_t>(d, o_d), item_first_host, item_group_host,
                         n_items, *p, Regions::at<uint64_t>(d, o_table), Regions::at<ndt_place_hit>(d, o_out), Regions::at<int>(d, o_n)));
  if (table_host && I) HIP_TRY(ctx, hipMemcpyAsync(table_host, d + o_table, Q * I * 8, hipMemcpyDeviceToHost, fr.st));
  HIP_TRY(ctx, hipMemcpyAsync(out_host, d + o_out, Q * K * sizeof(ndt_place_hit), hipMemcpyDeviceToHost, fr.st));
  HIP_TRY(ctx, hipMemcpyAsync(n_out_host, d + o_n, Q * sizeof(int), hipMemcpyDeviceToHost, fr.st));
  return fr.close_and_wait();
}

int ndt_sessions_place_candidates(ndt_sessions *s, const unsigned char *which, const unsigned char *against, const ndt_place_params *p,
                                  ndt_place_candidate *out, int *n_out) {
  SetCall call{s, "ndt_sessions_place_candidates"};
  PL_TRY(call.enter());
  if (!p || !out || !n_out) return call.refuse("NULL pointer");
  PL_TRY(place_check_params(call.ctx, call.f, *p));
  return call.run([&] { return place_set_candidates(s, call, which, against, *p, out, n_out); });
}

}  // extern "C"

#undef PL_TRY
