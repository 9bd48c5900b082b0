// ndt_mi355x.hip -- MI355X (gfx950 / CDNA4) NDT scan-matching core + its C ABI.
//
// Replaces what the reference delegates to PCL behind PoseEstimator::estimatePose
// (/root/reference/src/PoseEstimator.cpp:17-56): voxel normal-distributions build (SURVEY.md
// 8a row a2), SE(2) transform + radius lookup + score/gradient/Hessian accumulation (a4, a5),
// Newton + More-Thuente pose update (a3, a6), fitness score (a7), final Hessian (a8) and the
// pose extraction (a9).  Written for 64-wide wavefronts; no MFMA (there is no dense
// contraction on this path); fp64 accumulation with fixed-order reductions so a run is
// deterministic and takes the same line-search branches as the CPU oracle.
//
// Floating-point contraction is OFF for the whole file (voxel statistics, float32 transform and
// the optimiser must round like the scalar reference code); the hot accumulation loop asks for
// fused multiply-adds explicitly with __builtin_fma.
//
// This file never includes or calls anything under oracle/.  Without a HIP device every entry
// point fails with NDT_E_NO_DEVICE: there is no CPU fallback.

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <type_traits>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

#include "ndt_mi355x.h"

#pragma clang fp contract(off)

namespace {

thread_local std::string g_last_error;

#include "ndt_libm_f32.hip.h"
#include "ndt_common.hip.h"
#include "ndt_point.hip.h"
#include "ndt_optimizer.hip.h"
#include "ndt_fitness.hip.h"
#include "ndt_fit_points.hip.h"
#include "ndt_match.hip.h"
#include "ndt_map_build.hip.h"
#include "ndt_front.hip.h"
#include "ndt_localmap.hip.h"
#include "ndt_resample.hip.h"
#include "ndt_score.hip.h"
#include "ndt_occupancy.hip.h"
#include "ndt_posegraph.hip.h"

}  // namespace

// ==========================================================================================
// host side
// ==========================================================================================

namespace {

std::set<ndt_ctx *> g_live_ctx;                // contexts that exist (a map may outlive a context that only READ it)
std::mutex g_live_mu;                          // (contexts may be created / destroyed from different host threads)

int fail(ndt_ctx *ctx, int code, const std::string &msg);

#define HIP_TRY(ctx, expr)                                                                   \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return fail((ctx), NDT_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));      \
  } while (0)

// A device (or pinned host) allocation of T, freed by its owner's destructor: a context or map frees its buffers when it is
// deleted (after it has drained its streams and made its device current).
template <typename T, bool Pinned = false>
struct DevBuf {
  T *p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept { *this = std::move(o); }
  DevBuf &operator=(DevBuf &&o) noexcept { release(); std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }
  ~DevBuf() { release(); }
  size_t cap() const { return bytes / sizeof(T); }
  void release() { if (p) { hipError_t e = Pinned ? hipHostFree(p) : hipFree(p); (void)e; } p = nullptr; bytes = 0; }
  // exactly `want` bytes; the old allocation is freed first (no two at once)
  int alloc(ndt_ctx *ctx, size_t want) {
    release();
    void *q = nullptr;
    const hipError_t e = Pinned ? hipHostMalloc(&q, want, hipHostMallocDefault) : hipMalloc(&q, want);
    if (e != hipSuccess) return fail(ctx, NDT_E_HIP, std::string(Pinned ? "hipHostMalloc: " : "hipMalloc: ") + hipGetErrorString(e));
    p = static_cast<T *>(q); bytes = want;
    return NDT_OK;
  }
  // at least n elements, grow-only (need + need / 4 + 256 bytes); *grown: a new allocation was made (contents undefined)
  int ensure(ndt_ctx *ctx, size_t n, bool *grown = nullptr) {
    const bool grow = !p || n > cap();
    if (grown) *grown = grow;
    return grow ? alloc(ctx, n * sizeof(T) + n * sizeof(T) / 4 + 256) : NDT_OK;
  }
};
template <typename T> using PinnedBuf = DevBuf<T, true>;

// An event or a stream that its owner's destructor destroys, as DevBuf frees: the owner has drained its work first.
template <typename H, hipError_t (*Destroy)(H)>
struct Handle {
  H h = nullptr;
  Handle() = default;
  Handle(Handle &&o) noexcept { std::swap(h, o.h); }
  Handle &operator=(Handle &&o) noexcept { release(); std::swap(h, o.h); return *this; }
  ~Handle() { release(); }
  void release() { if (h) { hipError_t e = Destroy(h); (void)e; } h = nullptr; }
  H get() const { return h; }
  operator H() const { return h; }
};
struct Event : Handle<hipEvent_t, hipEventDestroy> {
  int create(ndt_ctx *ctx, unsigned flags = hipEventDefault) { release(); HIP_TRY(ctx, hipEventCreateWithFlags(&h, flags)); return NDT_OK; }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {
  int create(ndt_ctx *ctx, unsigned flags) { release(); HIP_TRY(ctx, hipStreamCreateWithFlags(&h, flags)); return NDT_OK; }
  int create(ndt_ctx *ctx, unsigned flags, int priority) { release(); HIP_TRY(ctx, hipStreamCreateWithPriority(&h, flags, priority)); return NDT_OK; }
};

// A table that the host writes into pinned memory and one copy per call uploads: the previous call's copy may still be reading
// the staging when the next call comes to rewrite (or reallocate) it.
template <typename T>
struct StagedUpload {
  PinnedBuf<T> h;
  Event ev;                           // behind the last upload (created on first use)
  bool pending = false;               // ... which has not been waited for yet
  // the staging is the host's to rewrite, with room for n elements
  int reserve(ndt_ctx *ctx, size_t n) {
    if (!ev) { const int rc = ev.create(ctx, hipEventDisableTiming); if (rc) return rc; }
    if (pending) { HIP_TRY(ctx, hipEventSynchronize(ev)); pending = false; }
    return h.ensure(ctx, n);
  }
  // elements [first, first + n) of the staging to dst, on st
  hipError_t upload(void *dst, size_t first, size_t n, hipStream_t st) {
    hipError_t e = hipMemcpyAsync(dst, h.p + first, n * sizeof(T), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(ev, st);
    if (e == hipSuccess) pending = true;
    return e;
  }
};

constexpr size_t align_up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }      // a: a power of two

// Consecutive regions of one block (a DevBuf of bytes, a pinned staging, or both with the same layout): take() gives the next
// one's offset, at a multiple of `align` bytes (tables that kernels read as a whole: 256), `end` is the block's size -- what
// ensure() / reserve() get --, at() a region's typed pointer in a block.  Size and pointers come from the one object.
struct Regions {
  size_t end = 0;
  size_t take(size_t bytes, size_t align = 64) { const size_t o = align_up(end, align); end = o + bytes; return o; }
  template <typename T, typename B> static T *at(B *base, size_t o) {
    using Byte = std::conditional_t<std::is_const<B>::value, const char, char>;
    return reinterpret_cast<T *>(reinterpret_cast<Byte *>(base) + o);
  }
};

// offsets[0 .. n] relative to offsets[0]: what a host form uploads beside the points [offsets[0], offsets[n]) alone
void rel_offsets(const uint64_t *offsets, size_t n, uint64_t *out) { for (size_t i = 0; i <= n; ++i) out[i] = offsets[i] - offsets[0]; }
std::vector<uint64_t> rel_offsets(const uint64_t *offsets, size_t n) { std::vector<uint64_t> r(n + 1); rel_offsets(offsets, n, r.data()); return r; }

// Run-time booleans as compile-time ones, to pick a kernel's template instance: f(std::true_type / std::false_type).
template <typename F> void with_bool(bool b, F &&f) { if (b) f(std::true_type{}); else f(std::false_type{}); }

// Timing events of the last kLen match launches of a context, attached to the dispatches: match kernel start / stop, end of
// the launch (fitness_reduce_kernel stop).  Launch k of the context is entry k % kLen.
struct LaunchRing {
  static constexpr int kLen = 64;
  Event ev[3 * kLen];
  bool deferred_[kLen] = {};           // NDT_OPT_DEFER_FITNESS: the launch's fitness kernels are on the context's own stream
  unsigned long long launches = 0;     // launches entered so far (read and written under g_live_mu)

  Event *events(unsigned long long k) { return ev + 3 * (k % kLen); }
  // A launch that has left the ring is covered by the latest one: a context queues its launches in order (its fitness stream
  // is in order, a launch that leaves the deferred mode waits for the last deferred one, the scratch bracket orders a call
  // on another stream behind the previous one), so the latest launch's end is reached after every earlier one's.
  unsigned long long covering(unsigned long long k) const { return launches - 1 - k >= (unsigned long long)kLen ? launches - 1 : k; }
  hipEvent_t end(unsigned long long k) { return events(covering(k))[2]; }
  bool deferred(unsigned long long k) const { return deferred_[covering(k) % kLen]; }
  // the events of the launch `b` launches before the latest (0: the latest); nullptr if it is not in the ring
  Event *back(int b) { return b < 0 || b >= kLen || (unsigned long long)b >= launches ? nullptr : events(launches - 1 - b); }
  // Enters the next launch of context `self` as the latest one of that context that reads maps[0 .. n) (each map once), in
  // their lists of readers (ndt_map::readers).
  // Under g_live_mu: launches and builds on several contexts may come from several host threads.
  void enter(ndt_ctx *self, const ndt_map *const *maps, int n, bool deferred);
};

}  // namespace

struct ndt_ctx {
  int device = 0;
  hipStream_t stream = nullptr;       // the stream all work is ordered on (own_stream, or the caller's: not owned)
  ndt_map *pending_map = nullptr;            // ndt_map_rebuild_begin without its _end (one at a time: the read-back buffer is the context's)
  bool map_ms_pending = false;
  PinnedBuf<unsigned> h_bounds;              // bounding box read-back of the map build
  std::string err;
  float map_ms = 0.f, align_ms = 0.f;
  // grow-only staging for the host-pointer entry points
  DevBuf<unsigned char> d_scan, d_tmp;
  DevBuf<uint64_t> d_off;
  DevBuf<double> d_init, d_trace;
  DevBuf<ndt_result> d_res;
  DevBuf<int> d_rows;
  DevBuf<int> d_map_of;                                // ndt_align_batch_multi: the host map_of's copy
  DevBuf<float> d_fit;                                 // squared distance to the nearest map point, per scan point (shared_scan launches)
  DevBuf<FitPart> d_fit_part;                          // FitPart per chunk of 64 scan points (ndt_fitness.hip.h)
  DevBuf<FitPtsPart> d_fit_pts;                        // ndt_fit_points_batch_dev: FitPtsPart per chunk of 64 scan points in input order (ndt_fit_points.hip.h)
  StagedUpload<unsigned char> fp_tab;                  // ndt_fit_points_batch: offsets, transforms and scans of the call, one upload
  DevBuf<unsigned char> d_occ;                         // ndt_occ_integrate_dev: the call's table of grids, its count of runs and the runs (ndt_occupancy.hip.h)
  StagedUpload<unsigned char> occ_tab, occ_up;         // ... the table's staging; ndt_occ_integrate: offsets, grid_of, origins and scans of the call, one upload
  DevBuf<unsigned char> d_pg;                          // ndt_pg_*_batch_dev: the call's table of graphs (and queries), then every graph's or workgroup's scratch (ndt_posegraph.hip.h)
  StagedUpload<unsigned char> pg_tab;                  // ... the table's staging
  DevBuf<unsigned char> d_far;                         // deferred far phase of the fitness search: per match two counts, then the lists
  DevBuf<unsigned char> d_pf;                          // pre-filter: filtered points at the raw offsets + counts
  DevBuf<unsigned char> d_rs;                          // resampler: walk outputs at k_max slots per raw point, lengths, piece counts
  DevBuf<unsigned char> d_mm;                          // local-map assembly (and the neighbour removal on its own): jobs, units, voxel sets, lists
  StagedUpload<unsigned char> mm_tab;                  // its job table
  StagedUpload<MapView> views_tab;                     // ndt_align_batch_multi_dev: the launch's table of map views
  DevBuf<MapView> d_fp_views;                          // ndt_fit_points_multi_dev: the call's table of map views ...
  StagedUpload<MapView> fpv_tab;                       // ... and its staging
  // ndt_map_build_batch_dev: the scan's ticket (word 0) and 16 words per map from word 16 (map_minmax's running box, result and
  // done-counter, set to their start values when the table grows), their read-back, the job table and its staging
  DevBuf<unsigned> d_boxes;
  PinnedBuf<unsigned> h_boxes;
  DevBuf<unsigned char> d_bb;
  StagedUpload<unsigned char> bb_tab;
  DevBuf<unsigned char> d_bstage;                      // ndt_map_build_batch: the host clouds' copies
  DevBuf<unsigned char> d_sel;                         // candidate pick: the sorted lists of the runs, their lengths and heads
  DevBuf<unsigned char> d_rl;                          // score sweep / relocalisation: poses or score volume, pair counts, candidates, guesses, records
  DevBuf<unsigned char> d_sj, d_pk;                    // multi-job sweep: the call's job table and prefix table of tiles; multi-job pick: its job table
  StagedUpload<unsigned char> sj_tab, pk_tab;          // ... their stagings (one each: a pick queued behind a sweep does not wait for the sweep's upload)
  DevBuf<unsigned char> d_cg;                          // ndt_cross_gate_batch: the call's table (rows, packed poses, searchers), the (searcher x row) minima, the picks (ndt_cross.hip.h)
  StagedUpload<unsigned char> cg_tab;                  // ... the table's staging
  PinnedBuf<unsigned char> h_cg;                       // ... the picks' read-back
  DevBuf<unsigned char> d_pld, d_plm;                  // ndt_place_describe_batch_dev: the call's table (edges, rows); ndt_place_match_dev: its table (groups, items) and scratch (ndt_place.hip.h)
  StagedUpload<unsigned char> pld_tab, plm_tab;        // ... their stagings (one each: a match queued behind a describe does not wait for the describe's upload)
  DevBuf<unsigned char> d_pl_host;                     // the host forms' copies of clouds, descriptors and results
  PinnedBuf<unsigned char> h_pl;                       // ndt_sessions_place_candidates: the hits' read-back
  int num_cus = 0;
  int helpers = -1;                                    // NDT_OPT_MAX_HELPERS: helper workgroups per scan (0: no work sharing; -1: by the size of the launch)
  int workgroups = 0;                                  // NDT_OPT_WORKGROUPS: workgroups of a match launch (0: one per CU)
  int inject_fault = 0;                                // NDT_OPT_INJECT_FAULT (tests): the k-th next match launch fails behind its first kernel
  int score_stage = 1;                                 // NDT_OPT_SCORE_STAGE: the score sweep stages scans that fit in LDS (0: every scan is read from global memory)
  // Batches prepared ahead (ndt_align_batch_prepare_dev): two sets of buffers in turn -- ordered copies, records, bitmaps -- that
  // belong to no scratch bracket: set s is written by the prepare call for batch i + 1 while the launch of batch i, which reads
  // the other set, is still running; the prepare call orders itself behind the last launch that read ITS set and behind the
  // set's own previous ndt_order_kernel (which may still run on another stream).
  struct PrepSet {
    DevBuf<float2> sorted;
    DevBuf<PrepRec> recs;
    DevBuf<unsigned char> maps;
    Event ev0, ready;                                  // around ndt_order_kernel (on its dispatch)
    bool valid = false, timed = false;
    // what the set was prepared for: the batch, and by value everything of the map ndt_order_kernel reads -- the optimiser's
    // parameters (init_state: libm_f32, snap_thresh), the kernel instance (transform_sse) and the grid's origin and leaf
    // (the cells at the first pose; div_x / div_y besides: the grid as a whole)
    const void *scans = nullptr, *offsets = nullptr, *inits = nullptr, *map = nullptr;
    int B = 0, shared_scan = 0; size_t total_points = 0;
    int min_bx = 0, min_by = 0, div_x = 0, div_y = 0; float inv_leaf = 0.f;
    OptParams P{}; int transform_sse = 0;
    long long reader = -1;                             // number of the last launch of this context that read the set (-1: none)
  } prep[2];
  int prep_last = 1;                                   // set of the most recent prepare call
  float order_ms = 0.f;                                // ndt_order_kernel of the prepared batch the last launch used
  // The grow-only scratch above belongs to the context, not to a stream: a call on another stream than the
  // previous one first waits for the previous user (ev_scratch).
  hipStream_t scratch_stream = nullptr; bool scratch_used = false, scratch_recorded = false;
  // A match launch's WsHeader + ScanCtl[B] + chunk totals + bitmaps (ws), cell-ordered copy of the scans (sorted) and leading
  // bytes of ws known to be zero (cleared by the previous launch's last kernel).  Set 0 is the one every entry point uses;
  // NDT_OPT_DEFER_FITNESS launches take turns on all of them (the fitness kernels of the launches in between read theirs).
  struct LaunchSet { DevBuf<unsigned char> ws; DevBuf<float2> sorted; size_t ws_clean = 0; };
  static constexpr int kDeferSets = 2;                 // launches whose fitness kernels may be outstanding behind a new launch's match kernel, + 1
  LaunchSet sets[kDeferSets];
  // NDT_OPT_DEFER_FITNESS: the fitness kernels of ndt_align_batch_dev on a stream of the context's own, beside whatever the
  // caller's stream runs next (the next launch's match kernel: its idle workgroups' CUs)
  int defer_fitness = 0;
  struct FitJob {                                      // the fitness kernels of one launch: what queue_fitness needs
    MapView V; const float *scans = nullptr; const unsigned long long *offsets = nullptr; int B = 0, shared_scan = 0;
    size_t total_points = 0; float2 *sorted = nullptr; ndt_result *out = nullptr; unsigned char *ws = nullptr;
    size_t zero_bytes = 0, far_cnt_bytes = 0; bool sse = false; hipEvent_t end = nullptr;
    const MapView *views = nullptr; const int *map_of = nullptr; int n_maps = 0;   // multi-map launch: the device table (else V)
  };
  bool deferred_pending = false;                       // the last launch's fitness kernels may still be running beside the caller's stream
  // The events and streams the context owns, declared behind the buffers above: `delete` destroys them first, the buffers after
  // them (ndt_ctx_destroy has drained every stream before; a staged table's and a prepared set's events go with their buffers).
  Stream own_stream;                  // created by ndt_ctx_create
  Event ev0, ev1;                     // around the last match launch
  Event evm0, evm1;                   // around the last map build
  Event evb;                          // bounding box of the map build read back
  Stream side;                        // map build: bounding box + centroid fill beside the bucketing chain
  Event ev_fork, ev_join;
  Event ev_scratch;                   // the scratch bracket (CallFrame)
  Stream fit_stream;                  // NDT_OPT_DEFER_FITNESS (created on first use)
  LaunchRing ring;
  // Occupancy grids: the event behind each of the last kOccEv calls that wrote a grid (integrate, clear, create), recorded on
  // that call's stream; call k's is occ_ev[k % kOccEv].  A grid remembers the number of its last writer (ndt_occ::wseq).
  static constexpr int kOccEv = 8;
  Event occ_ev[kOccEv];
  unsigned long long occ_seq = 0;
};

struct ndt_map {
  ndt_ctx *ctx = nullptr;
  int device = 0;                             // ctx->device, kept for a destroy after the context's (ndt_map_destroy)
  ndt_params prm;
  ndt_map_info info;
  bool info_valid = false;
  MapView view;
  size_t n = 0, ng = 0, npad = 0;
  // device buffers (grow-only across rebuilds)
  DevBuf<int> count, start, npts_grid;
  DevBuf<unsigned long long> scan_state;      // scan_onepass_kernel: two tagged words per tile
  unsigned scan_seq = 0;                      // tag of the last build's words
  bool count_clean = false;                   // count is all zero (a complete build leaves it so: the scatter takes back what the count added)
  DevBuf<int> perm;
  DevBuf<float2> pts, cent;
  DevBuf<double> rec;
  DevBuf<unsigned> bounds; DevBuf<int> counters;   // counters: n_cells, n_valid, n_big
  DevBuf<int> big;
  DevBuf<unsigned> occ;
  DevBuf<unsigned long long> tiles;           // MapView::tiles
  bool pending = false, pend_queued = false;  // between ndt_map_rebuild_begin and _end
  const float *pend_xy = nullptr; size_t pend_stride = 0;
  GridDims grid; bool have_grid = false;      // voxel grid of the last build (queued ahead of the next one's bounding box)
  DevBuf<unsigned char> xy_stage;             // ndt_map_build: the host cloud's copy
  // Launches that read this map since its last build_begin, one entry per reading context: (context, number of that launch
  // in the context's ring).  A build that has to be queued AGAIN (build_end: the speculative grid was wrong) rewrites
  // the tables those launches read -- on another stream when the caller builds and matches on different contexts -- and
  // must wait for them first (round 4: a fitness kernel walking bucket offsets that were being rebuilt ran 236 ms); so must
  // every build for the deferred ones (build_begin).
  std::vector<std::pair<ndt_ctx *, unsigned long long>> readers;
};

namespace {

int fail(ndt_ctx *ctx, int code, const std::string &msg) {
  g_last_error = msg;
  if (ctx) ctx->err = msg;
  return code;
}

// The refusal of a call `f` that would use the context while an ndt_map_rebuild_begin waits for its _end (the one sentence).
int refuse_pending(ndt_ctx *ctx, const std::string &f) { return fail(ctx, NDT_E_ARG, f + ": an ndt_map_rebuild_begin is open on the context"); }

// The call frame of every entry point that uses the context's scratch or queues one of its launches, opened behind the
// entry point's refusals and early returns: open() makes the context's device current, picks the stream (the caller's, or the
// context's for NULL) and opens the scratch bracket on it (ndt_ctx::ev_scratch) before the first use of the scratch; close()
// closes it after the last.  Everything the call queues lies in between -- a host form's uploads into d_scan / d_off / d_tmp
// and its read-backs too -- and a host form waits behind close() (close_and_wait).
// (An event record is a barrier packet between kernels: a call on the context's own / registered stream -- which lives
// as long as the registration -- records nothing; the event is recorded on that stream when a call on ANOTHER stream
// arrives.  A call on a foreign stream records at once: the stream may be gone by the time the next call comes.)
// The bracket is closed on EVERY way out of an entry point once it is open: an error return behind the first queued kernel or
// copy still leaves work on `st` that uses the context's scratch, and a later call on another stream must be ordered behind it
// (round 5; VERDICT r04: launch_align failing after the match kernel was queued returned without it).  The quiet form (the
// destructor) keeps the error message of the failure that is being returned.
struct CallFrame {
  ndt_ctx *ctx; hipStream_t st = nullptr; bool is_open = false;
  explicit CallFrame(ndt_ctx *c) : ctx(c) {}
  CallFrame(const CallFrame &) = delete;
  CallFrame &operator=(const CallFrame &) = delete;
  int open(void *stream = nullptr, bool deferred_launch = false) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    st = stream ? (hipStream_t)stream : ctx->stream;
    // (NDT_OPT_DEFER_FITNESS) whatever uses the context's scratch next waits for the fitness kernels still running on the
    // context's own stream -- except the next deferred launch, which orders itself (launch_align)
    if (ctx->deferred_pending && !deferred_launch && ctx->ring.launches > 0) {
      HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ring.end(ctx->ring.launches - 1), 0));
      ctx->deferred_pending = false;
    }
    if (ctx->scratch_used && st != ctx->scratch_stream) {
      if (!ctx->scratch_recorded) HIP_TRY(ctx, hipEventRecord(ctx->ev_scratch, ctx->scratch_stream));
      HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_scratch, 0));
    }
    is_open = true;
    return NDT_OK;
  }
  int close() {
    is_open = false; ctx->scratch_recorded = false;
    if (st != ctx->stream) { HIP_TRY(ctx, hipEventRecord(ctx->ev_scratch, st)); ctx->scratch_recorded = true; }
    ctx->scratch_stream = st; ctx->scratch_used = true;
    return NDT_OK;
  }
  int close_and_wait() {
    const int rc = close();
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return NDT_OK;
  }
  ~CallFrame() {
    if (!is_open) return;
    const std::string keep = ctx->err, keep_tl = g_last_error;
    (void)close();
    ctx->err = keep; g_last_error = keep_tl;
  }
  // the whole frame of a device form: open, body(st), close
  template <typename Body> static int run(ndt_ctx *ctx, void *stream, Body &&body, bool deferred_launch = false) {
    CallFrame fr(ctx);
    int rc = fr.open(stream, deferred_launch);
    if (rc == NDT_OK) rc = body(fr.st);
    return rc ? rc : fr.close();
  }
};

void LaunchRing::enter(ndt_ctx *self, const ndt_map *const *maps, int n, bool deferred) {
  std::lock_guard<std::mutex> lk(g_live_mu);
  deferred_[launches % kLen] = deferred;
  for (int i = 0; i < n; ++i) {
    auto &readers = const_cast<ndt_map *>(maps[i])->readers;
    auto it = std::find_if(readers.begin(), readers.end(), [&](const auto &r) { return r.first == self; });
    if (it != readers.end()) it->second = launches; else readers.emplace_back(self, launches);
  }
  launches++;
}

// The map-read bracket of a call of `ctx` that queues kernels on st which read maps[0 .. n) (each map once).
// begin(): st waits for the build of every map built on another stream (once per building context); ev[0 .. 2] are the ring's
// events for the launch.  entered(code, ...), on EVERY way out once a kernel is queued: the launch has its end event (recorded
// here unless a dispatch carried it) and its place in the context's ring and in each map's readers, so that a later call on
// another stream and a build that must wait for it are ordered behind it; returns code (for NDT_OK: the record's failure, as
// `who`'s).  deferred: work that the stream order of the map's builds does not cover (take_over_from_readers waits for it).
struct MapRead {
  ndt_ctx *ctx; hipStream_t st; const ndt_map *const *maps; int n;
  Event *ev = nullptr;
  int begin() {
    std::vector<const ndt_ctx *> waited;
    for (int i = 0; i < n; ++i) {
      const ndt_ctx *b = maps[i]->ctx;
      if (st == b->stream || std::find(waited.begin(), waited.end(), b) != waited.end()) continue;
      HIP_TRY(ctx, hipStreamWaitEvent(st, b->evm1, 0));
      waited.push_back(b);
    }
    ev = ctx->ring.events(ctx->ring.launches);
    return NDT_OK;
  }
  int entered(int code, bool end_carried, bool deferred, const char *who) {
    const hipError_t e = end_carried ? hipSuccess : hipEventRecord(ev[2], st);
    ctx->ring.enter(ctx, maps, n, deferred);
    if (e != hipSuccess && code == NDT_OK) return fail(ctx, NDT_E_HIP, std::string(who) + ": hipEventRecord: " + hipGetErrorString(e));
    return code;
  }
};

OptParams opt_of(const ndt_params &p) {
  OptParams o;
  o.step_size = p.step_size; o.trans_eps = p.trans_eps; o.snap_thresh = p.snap_thresh;
  o.mt_mu = p.mt_mu; o.mt_nu = p.mt_nu; o.max_iter = p.max_iter; o.conv_ge = p.conv_ge;
  o.stale_h_ang = p.stale_h_ang; o.mt_max_iter = p.mt_max_iter; o.libm_f32 = p.libm_f32;
  return o;
}

bool same_bits(const void *a, const void *b, size_t n) { return memcmp(a, b, n) == 0; }

// Every field of two OptParams, the doubles bit for bit (not the struct as a whole: its padding is not defined).
bool same_opt(const OptParams &o, const OptParams &o0) {
  return same_bits(&o.step_size, &o0.step_size, sizeof(double)) && same_bits(&o.trans_eps, &o0.trans_eps, sizeof(double)) &&
         same_bits(&o.snap_thresh, &o0.snap_thresh, sizeof(double)) && same_bits(&o.mt_mu, &o0.mt_mu, sizeof(double)) &&
         same_bits(&o.mt_nu, &o0.mt_nu, sizeof(double)) && o.max_iter == o0.max_iter && o.conv_ge == o0.conv_ge &&
         o.stale_h_ang == o0.stale_h_ang && o.mt_max_iter == o0.mt_max_iter && o.libm_f32 == o0.libm_f32;
}

// a3: Gaussian constants (Magnusson 2009 eq 6.8), host libm, once per map.
void gauss_constants(const ndt_params &p, double *d1, double *d2) {
  double res = (double)p.resolution;
  double c1 = 10.0 * (1.0 - p.outlier_ratio);
  double c2 = p.outlier_ratio / std::pow(res, 3);
  double d3 = -std::log(c2);
  *d1 = -std::log(c1 + c2) - d3;
  *d2 = -2.0 * std::log((-std::log(c1 * std::exp(-0.5) + c2) - d3) / *d1);
}

// Largest double e with fl(d2 * e) <= 1 (d2 > 0): updateDerivatives drops a pair when d2 e > 1, d2 e < 0 or NaN; e = exp(..)
// is never negative, so the check is `e > e_hi` (ndt_point.hip.h).  Plain fp64 products, as the device would form them.
double pair_check_threshold(double d2) {
  if (d2 != d2 || d2 == 0.0) return INFINITY;
  if (d2 < 0.0) return -1.0;                       // every e > 0 gives d2 e < 0; e == 0 adds nothing either way
  volatile double e = 1.0 / d2, pr;
  for (int i = 0; i < 64; ++i) { pr = d2 * e; if (pr <= 1.0) break; e = std::nextafter((double)e, 0.0); }
  for (int i = 0; i < 64; ++i) { const double up = std::nextafter((double)e, INFINITY); pr = d2 * up; if (!(pr <= 1.0)) break; e = up; }
  return e;
}

// exp table 2^(j/64), correctly rounded, uploaded once per device
int upload_exp_table(ndt_ctx *ctx);

int grid_for(size_t n, int block, int cap = 2048) {
  size_t g = (n + block - 1) / block;
  if (g < 1) g = 1;
  if (g > (size_t)cap) g = cap;
  return (int)g;
}

// The grid of the kernels that search a launch's scans (fitness_points_kernel, fitness_far_kernel, fit_points_kernel): gx
// workgroups of 256 queries per match, a block per 256 points of the average scan and 64 at the most, for B rounded up to
// whole rounds of the eight XCDs.  One-dimensional, XCD-aware: workgroup w -> (match, block of the match) in fit_block_of
// (ndt_fitness.hip.h).  workgroup_bound > 0 (NDT_OPT_WORKGROUPS): no more workgroups than that, while every match keeps one.
struct FitGrid { unsigned gx, workgroups; };
FitGrid fit_grid(size_t total_points, int B, int shared_scan, int workgroup_bound = 0) {
  const size_t avg = shared_scan ? total_points : (total_points + (size_t)B - 1) / (size_t)B;
  const size_t b8 = ((size_t)B + 7) / 8 * 8;
  size_t gx = std::min<size_t>(64, std::max<size_t>(1, (avg + 255) / 256));
  if (workgroup_bound > 0) gx = std::max<size_t>(1, std::min<size_t>(gx, (size_t)workgroup_bound / b8));
  return FitGrid{(unsigned)gx, (unsigned)(gx * b8)};
}

// The fitness kernels of one launch on stream fs (behind its match kernel there: stream order, or the caller has made fs wait).
int queue_fitness(ndt_ctx *ctx, const ndt_ctx::FitJob &J, hipStream_t fs) {
  const MapView &V = J.V;
  const float *scans = J.scans; const unsigned long long *offsets = J.offsets;
  const int B = J.B, shared_scan = J.shared_scan; const size_t total_points = J.total_points;
  float2 *sorted = J.sorted; ndt_result *out = J.out; unsigned char *ws = J.ws;
  const size_t zero_bytes = J.zero_bytes, far_cnt_bytes = J.far_cnt_bytes;
  float *fit = ctx->d_fit.p;
  FitPart *parts = ctx->d_fit_part.p;
  const FitGrid G = fit_grid(total_points, B, shared_scan);
  const unsigned gx = G.gx;
  const dim3 grid(G.workgroups);
  // hypothesis scoring (shared_scan): most seeds end far from the map -- the far phase of the search as a pass of its own over
  // the queries that need it (ndt_fitness.hip.h); scans of their own: the search kernel leaves a {sum, count} per chunk of 64
  // points instead of a distance per point
  unsigned *far_n = shared_scan ? (unsigned *)ctx->d_far.p : nullptr, *far_idx = shared_scan ? (unsigned *)(ctx->d_far.p + far_cnt_bytes) : nullptr;
  if (shared_scan) { hipError_t e = hipMemsetAsync(far_n, 0, far_cnt_bytes, fs); if (e != hipSuccess) return fail(ctx, NDT_E_HIP, std::string("queue_fitness: hipMemsetAsync: ") + hipGetErrorString(e)); }
  // the closing kernel, shared_scan: a workgroup per match; else a wave per match, and at least as many workgroups as clear the
  // control words with one store per thread, a CU each at most
  const size_t close_wgs = shared_scan ? (size_t)std::min(B, 4 * ctx->num_cus)
                                       : std::max<size_t>(((size_t)B + kFitBlock / 64 - 1) / (kFitBlock / 64),
                                                          std::min<size_t>((size_t)ctx->num_cus, (zero_bytes / 16 + kFitBlock - 1) / kFitBlock));
  // (a single-map launch: views, map_of null and n_maps 0, the kernels' defaults)
  with_bool(J.sse, [&](auto S) { with_bool(J.views != nullptr, [&](auto M) { with_bool(shared_scan != 0, [&](auto D) {
    constexpr bool sse = decltype(S)::value, multi = decltype(M)::value, shared = decltype(D)::value;
    fitness_points_kernel<sse, shared, multi><<<grid, 256, 0, fs>>>(V, scans, offsets, B, shared_scan, sorted, out, fit, far_idx, far_n, (int)gx,
                                                                    shared ? nullptr : parts, J.views, J.map_of, J.n_maps);
    if constexpr (shared)
      fitness_far_kernel<sse, multi><<<grid, 256, 0, fs>>>(V, scans, offsets, B, shared_scan, sorted, out, fit, far_idx, far_n, (int)gx, J.views, J.map_of, J.n_maps);
    hipExtLaunchKernelGGL((fitness_reduce_kernel<shared, multi>), dim3((unsigned)close_wgs), dim3(kFitBlock), 0, fs, nullptr, J.end, 0,
                          offsets, B, shared_scan, shared ? (const float *)fit : (const float *)nullptr, out, parts, (uint4 *)ws,
                          (unsigned)(zero_bytes / 16), J.map_of, J.n_maps);
  }); }); });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(ctx, NDT_E_HIP, std::string("queue_fitness: ") + hipGetErrorString(e));
  return NDT_OK;
}

// The maps of a multi-map launch (ndt_align_batch_multi_dev): match b reads maps[map_of[b]] (map_of null: maps[b]).
// The launch's parameters and template instance are those of maps[0] -- every map has the same ones (checked by the caller).
struct MultiMaps {
  const ndt_map *const *maps; int n_maps;
  const int *map_of;                          // device, B entries, or null
  std::vector<const ndt_map *> distinct;      // each map once: the launch enters itself in the readers of every one
};

int launch_align(ndt_ctx *ctx, const ndt_map *map, hipStream_t st, const float *scans,
                 const unsigned long long *offsets, int B, int shared_scan, size_t total_points, const double *inits,
                 ndt_result *out, double *trace, int trace_cap, int *trace_rows, unsigned long long *prof,
                 ndt_ctx::PrepSet *pset = nullptr, bool defer = false, const MultiMaps *mm = nullptr) {
  const bool sse = map->prm.transform_sse != 0, incl = map->prm.radius_inclusive != 0;
  LaunchRing &R = ctx->ring;
  const unsigned long long L = R.launches;
  const ndt_map *const *maps = mm ? mm->distinct.data() : &map;
  MapRead rd{ctx, st, maps, mm ? (int)mm->distinct.size() : 1};
  { const int rc = rd.begin(); if (rc) return rc; }
  // NDT_OPT_DEFER_FITNESS: launches take turns on the sets -- the fitness kernels of launch i (the context's own stream) read
  // set i & 1 while the match kernel of launch i + 1 (the caller's stream) fills the other
  ndt_ctx::LaunchSet &set = ctx->sets[defer ? L % ndt_ctx::kDeferSets : 0];
  // leaving the deferred mode: behind the last launch's fitness kernels; in it: behind those of the launch before last (whose
  // control words, ordered copies -- and, the caller alternating two of them, result records -- this launch takes over)
  if (!defer && L >= 1 && R.deferred(L - 1)) HIP_TRY(ctx, hipStreamWaitEvent(st, R.end(L - 1), 0));   // (the fitness stream is in order: the last launch's end is everybody's)
  if (defer && L >= (unsigned long long)ndt_ctx::kDeferSets && R.deferred(L - ndt_ctx::kDeferSets)) HIP_TRY(ctx, hipStreamWaitEvent(st, R.end(L - ndt_ctx::kDeferSets), 0));
  // (the caller's priority class: below it these kernels starve behind every match kernel -- 0.49 against 0.37 ms per bench step)
  if (defer && !ctx->fit_stream) { const int rc = ctx->fit_stream.create(ctx, hipStreamNonBlocking); if (rc) return rc; }
  const MapView &V = map->view;
  const OptParams O = opt_of(map->prm);
  // workspace (layout: ws_bytes, ndt_match.hip.h): what lies in front of the marked-cell bitmaps is zero at kernel start
  const size_t zero_bytes = ws_bitmap_off((size_t)B);
  // a multi-map launch: its table of MapViews behind the bitmaps, outside the zeroed part -- in the launch's own set, so that
  // it lives as long as the launch's fitness kernels, which read it (NDT_OPT_DEFER_FITNESS: the set is not taken over before
  // they have finished; see below)
  const size_t tab_off = ws_views_off((size_t)B);
  bool grown = false;
  int rc = set.ws.ensure(ctx, ws_bytes((size_t)B, mm ? (size_t)mm->n_maps : 0), &grown);
  if (rc) return rc;
  if (grown) set.ws_clean = 0;
  // ordered copy of every scan (what the passes and the fitness kernel read) and one float per point for the
  // fitness score; when every match uses scan 0 each match has its own slot of the scan's size
  const size_t slots = (shared_scan ? (size_t)B : (size_t)1) * total_points;
  if ((rc = set.sorted.ensure(ctx, slots + 2))) return rc;
  if (shared_scan && (rc = ctx->d_fit.ensure(ctx, slots + 4))) return rc;   // (scans of their own: chunk sums only, d_fit_part)
  float2 *sorted = pset ? pset->sorted.p : set.sorted.p;      // (a prepared batch: its ordered copies are in its own set)
  const PrepRec *prep = pset ? pset->recs.p : nullptr;
  const unsigned *prep_map = pset ? (const unsigned *)pset->maps.p : nullptr;
  // (every allocation of the launch in front of its first kernel: nothing below can fail for want of memory once work is queued)
  Regions far;                                     // d_far: two counts per match, then the lists (FitJob::far_cnt_bytes: where they start)
  far.take((size_t)B * 2 * sizeof(unsigned), 16);
  const size_t far_cnt_bytes = far.take(slots * sizeof(unsigned) + 16, 16);
  if (shared_scan && (rc = ctx->d_far.ensure(ctx, far.end))) return rc;
  // the chunk sums of the fitness kernels (FitPart, a chunk = 64 points; a match's chunks start at fit_part_of)
  if ((rc = ctx->d_fit_part.ensure(ctx, fit_parts_needed(total_points, (size_t)B, shared_scan)))) return rc;
  // control words: zero before every launch -- by the last kernel of the previous launch of this context
  // (fitness_reduce_kernel), or by a memset when that did not cover enough
  if (mm && (rc = ctx->views_tab.reserve(ctx, (size_t)mm->n_maps))) return rc;   // (waits for the previous multi-map launch's copy)
  if (set.ws_clean < zero_bytes) HIP_TRY(ctx, hipMemsetAsync(set.ws.p, 0, zero_bytes, st));
  set.ws_clean = 0;
  unsigned char *ws = set.ws.p;
  // The table: the views as they are now (a map between ndt_map_rebuild_begin and _end is matched with the grid its view
  // holds at the call), staged in pinned memory, then one copy
  const MapView *views = nullptr;
  if (mm) {
    for (int i = 0; i < mm->n_maps; ++i) ctx->views_tab.h.p[i] = mm->maps[i]->view;
    HIP_TRY(ctx, ctx->views_tab.upload(ws + tab_off, 0, (size_t)mm->n_maps, st));
    views = reinterpret_cast<const MapView *>(ws + tab_off);
  }
  // helper limit: 8 while a launch has fewer scans than workgroups (one scan at a time: everybody helps), 2 for whole-GPU
  // batches -- there the match kernel is as fast with 2 as with 15, and workgroups that find nothing to join leave their
  // CUs to the next step's map build earlier (round 4, after the repeated line-search passes went: LOG R4.9)
  const int helpers = ctx->helpers >= 0 ? ctx->helpers : (B >= (ctx->workgroups > 0 ? ctx->workgroups : ctx->num_cus) ? kBatchHelpers : kDefaultHelpers);
  // one workgroup per CU (the LDS window allows no more); idle workgroups help unfinished scans
  const int ncu = ctx->workgroups > 0 ? ctx->workgroups : ctx->num_cus;
  const int grid = helpers ? ncu : (B < ncu ? B : ncu);
  // timing: the events ride on the kernels' own dispatch packets (hipExtLaunchKernelGGL: start / stop of that kernel) -- an
  // event RECORD is a packet of its own between two kernels, three of them per launch cost the stream 6-10 us
  Event *evr = rd.ev;
  // (the pair check left out where it cannot fire -- accumulate_pair -- in the preset's own instantiation only)
  const bool chk = !(V.e_hi > 1.0 + 1e-6);
  // The kernel exists in five <SSE, INCL, CHK> instances per MULTI (not eight: it is the largest in the object); a single-map
  // launch has no table (views, map_of null), a multi-map one no prepared set (prep, prep_map null).
  const int *map_of = mm ? mm->map_of : nullptr; const int n_maps = mm ? mm->n_maps : 0;
  auto match = [&](auto S, auto I, auto C) {
    with_bool(mm != nullptr, [&](auto M) {
      hipExtLaunchKernelGGL((ndt_align_kernel<decltype(S)::value, decltype(I)::value, decltype(C)::value, decltype(M)::value>), dim3(grid),
                            dim3(kBlock), 0, st, evr[0], evr[1], 0, V, O, scans, offsets, B, shared_scan, inits, out, trace, trace_cap,
                            trace_rows, sorted, ws, helpers, prof, prep, prep_map, views, map_of, n_maps);
    });
  };
  const std::true_type yes; const std::false_type no;
  if (sse && incl)      match(yes, yes, yes);
  else if (sse && !chk) match(yes, no, no);
  else if (sse)         match(yes, no, yes);
  else if (incl)        match(no, yes, yes);
  else                  match(no, no, yes);
  // From here on a kernel that reads the map and the context's scratch is queued (MapRead::entered).  A match launch on a
  // foreign stream is deferred, to a build, only under NDT_OPT_DEFER_FITNESS: ordering it before a build is the caller's job
  // (take_over_from_readers).  Its end event rides on fitness_reduce_kernel's dispatch unless that was not made.
  auto entered = [&](int code) {
    if (pset) pset->reader = (long long)L;
    return rd.entered(code, /*end_carried=*/code == NDT_OK, defer, "launch_align");
  };
  if (ctx->inject_fault > 0 && --ctx->inject_fault == 0)      // NDT_OPT_INJECT_FAULT (tests): fail with the match kernel queued
    return entered(fail(ctx, NDT_E_HIP, "launch_align: injected fault behind the match kernel's dispatch (NDT_OPT_INJECT_FAULT)"));
  // a7: fitness scores, behind the matches: on the same stream, or (NDT_OPT_DEFER_FITNESS) on the context's own stream behind the
  // match kernel's event -- the caller's stream is free for the next launch's match kernel, whose idle workgroups' CUs these
  // kernels then fill
  hipStream_t fs = st;
  if (defer) {
    fs = ctx->fit_stream;
    hipError_t e = hipStreamWaitEvent(fs, evr[1], 0);
    if (e != hipSuccess) return entered(fail(ctx, NDT_E_HIP, std::string("launch_align: hipStreamWaitEvent: ") + hipGetErrorString(e)));
  }
  const int qrc = queue_fitness(ctx, {V, scans, offsets, B, shared_scan, total_points, sorted, out, ws, zero_bytes, far_cnt_bytes, sse, evr[2],
                                      views, map_of, n_maps}, fs);
  if (qrc != NDT_OK) return entered(qrc);
  {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return entered(fail(ctx, NDT_E_HIP, std::string("launch_align: ") + hipGetErrorString(e)));
  }
  set.ws_clean = zero_bytes;
  if (defer) ctx->deferred_pending = true;
  return entered(NDT_OK);
}

int upload_exp_table(ndt_ctx *ctx) {
  double tab[64];
  for (int j = 0; j < 64; ++j) tab[j] = (double)exp2l((long double)j / 64.0L);
  HIP_TRY(ctx, hipMemcpyToSymbol(HIP_SYMBOL(c_exp2_tab), tab, sizeof(tab)));
  return NDT_OK;
}

}  // namespace

extern "C" {

// Presets of the version-sensitive PCL behaviour.  The reference compiles only
// against PCL <= 1.10 (boost::shared_ptr clouds, include/ndt_slam/PoseEstimator.h:72-73), most likely 1.10.0.
static void params_common(ndt_params *p) {
  memset(p, 0, sizeof(*p));
  p->resolution = 1.0f; p->step_size = 0.1; p->trans_eps = 0.01; p->max_iter = 35;   // PoseEstimator.h:63-64
  p->outlier_ratio = 0.55; p->min_pts = 6; p->eig_mult = 0.01;
  p->conv_ge = 0; p->radius_inclusive = 0; p->stale_h_ang = 0;
  p->snap_thresh = 10e-5; p->mt_max_iter = 10; p->mt_mu = 1.e-4; p->mt_nu = 0.9; p->grid_margin = 0;
}

int ndt_params_pcl110(ndt_params *p) {      // PCL 1.9 / 1.10: Leaf() starts cov_ at the identity, biased
  if (!p) return NDT_E_ARG;                 // normalisation, SSE transformPointCloud
  params_common(p);
  p->cov_unbiased = 0; p->cov_init_identity = 1; p->transform_sse = 1; p->libm_f32 = 1;
  return NDT_OK;
}

int ndt_params_pcl18(ndt_params *p) {       // PCL <= 1.8: the same voxel statistics, scalar transformPointCloud
  if (!p) return NDT_E_ARG;
  params_common(p);
  p->cov_unbiased = 0; p->cov_init_identity = 1; p->transform_sse = 0; p->libm_f32 = 0;   // (Ubuntu 18.04's glibc 2.27 has another sinf)
  return NDT_OK;
}

int ndt_params_pcl_new(ndt_params *p) {     // PCL >= 1.11: cov_ starts at zero, unbiased /(n-1)
  if (!p) return NDT_E_ARG;
  params_common(p);
  p->cov_unbiased = 1; p->cov_init_identity = 0; p->transform_sse = 1; p->libm_f32 = 1;
  return NDT_OK;
}

int ndt_default_params(ndt_params *p) { return ndt_params_pcl110(p); }

const char *ndt_last_error(const ndt_ctx *ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

static int ctx_init(ndt_ctx *c, int device) {
  c->device = device;
  HIP_TRY(c, hipSetDevice(device));
  int rc;
  if ((rc = c->own_stream.create(c, hipStreamNonBlocking))) return rc;
  c->stream = c->own_stream.get();
  for (Event *e : {&c->ev0, &c->ev1, &c->evm0, &c->evm1}) if ((rc = e->create(c))) return rc;
  {
    int lo = 0, hi = 0;
    HIP_TRY(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
    if ((rc = c->side.create(c, hipStreamNonBlocking, hi))) return rc;
  }
  for (Event *e : {&c->evb, &c->ev_fork, &c->ev_join, &c->ev_scratch}) if ((rc = e->create(c, hipEventDisableTiming))) return rc;
  for (Event &e : c->ring.ev) if ((rc = e.create(c))) return rc;
  if ((rc = c->h_bounds.alloc(c, 64))) return rc;
  if ((rc = upload_exp_table(c))) return rc;
  hipDeviceProp_t prop;
  HIP_TRY(c, hipGetDeviceProperties(&prop, device));
  c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1;
  c->helpers = -1;                          // automatic (launch_align)
  return NDT_OK;
}

int ndt_ctx_create(int device, ndt_ctx **out) {
  if (!out) return NDT_E_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, NDT_E_NO_DEVICE, "no HIP device visible: libndt_mi355x has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(nullptr, NDT_E_ARG, "device ordinal out of range");
  ndt_ctx *c = new (std::nothrow) ndt_ctx();
  if (!c) return NDT_E_NOMEM;
  const int rc = ctx_init(c, device);
  if (rc) { ndt_ctx_destroy(c); return rc; }      // (the error text stays in ndt_last_error(NULL))
  { std::lock_guard<std::mutex> lk(g_live_mu); g_live_ctx.insert(c); }
  *out = c;
  return NDT_OK;
}

int ndt_ctx_set_option(ndt_ctx *c, int option, long long value) {
  if (!c) return NDT_E_ARG;
  switch (option) {
    case NDT_OPT_MAX_HELPERS:
      if (value < -1 || value > kMaxHelpers) return fail(c, NDT_E_ARG, "NDT_OPT_MAX_HELPERS: 0 .. 15, or -1 for the default");
      c->helpers = (int)value; return NDT_OK;
    case NDT_OPT_WORKGROUPS:
      if (value < 0 || value > c->num_cus) return fail(c, NDT_E_ARG, "NDT_OPT_WORKGROUPS: 0 (one per CU) .. number of CUs");
      c->workgroups = (int)value; return NDT_OK;
    case NDT_OPT_INJECT_FAULT:
      if (value < 0 || value > 1000000) return fail(c, NDT_E_ARG, "NDT_OPT_INJECT_FAULT: 0 (off) or the number of the launch that fails");
      c->inject_fault = (int)value; return NDT_OK;
    case NDT_OPT_DEFER_FITNESS:
      if (value != 0 && value != 1) return fail(c, NDT_E_ARG, "NDT_OPT_DEFER_FITNESS: 0 or 1");
      c->defer_fitness = (int)value; return NDT_OK;
    case NDT_OPT_SCORE_STAGE:
      if (value != 0 && value != 1) return fail(c, NDT_E_ARG, "NDT_OPT_SCORE_STAGE: 0 or 1");
      c->score_stage = (int)value; return NDT_OK;
    default: return fail(c, NDT_E_ARG, "ndt_ctx_set_option: unknown option");
  }
}

int ndt_ctx_destroy(ndt_ctx *c) {
  if (!c) return NDT_E_ARG;
  { std::lock_guard<std::mutex> lk(g_live_mu); g_live_ctx.erase(c); }
  hipError_t e;
  e = hipSetDevice(c->device);
  // Ordering, not ownership: everything the context queued has finished before any of its events, streams and buffers goes.
  if (c->stream) e = hipStreamSynchronize(c->stream);
  if (c->fit_stream) e = hipStreamSynchronize(c->fit_stream);
  if (c->side) e = hipStreamSynchronize(c->side);
  for (ndt_ctx::PrepSet &S : c->prep)
    if (S.ready && S.scans) e = hipEventSynchronize(S.ready);      // (its kernel may have been queued on another stream than the context's)
  (void)e;
  delete c;                                     // (its events and streams, then its buffers: on this device, after the work above has drained)
  return NDT_OK;
}

void *ndt_ctx_stream(ndt_ctx *c) { return c ? (void *)c->stream : nullptr; }

int ndt_ctx_set_stream(ndt_ctx *c, void *stream) {
  if (!c) return NDT_E_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // the last user of the scratch may have been a *_dev call on a foreign stream (its event was recorded then)
  if (c->scratch_used && c->scratch_recorded) HIP_TRY(c, hipEventSynchronize(c->ev_scratch));
  c->scratch_used = false; c->scratch_recorded = false;   // (everything queued so far has finished)
  c->stream = stream ? (hipStream_t)stream : c->own_stream.get();
  return NDT_OK;
}

int ndt_last_timing(const ndt_ctx *cc, float *map_ms, float *align_ms) {
  if (!cc) return NDT_E_ARG;
  ndt_ctx *c = const_cast<ndt_ctx *>(cc);
  if (c->map_ms_pending) {                     // the device-pointer build returns before its last kernels end
    HIP_TRY(c, hipEventSynchronize(c->evm1));
    HIP_TRY(c, hipEventElapsedTime(&c->map_ms, c->evm0, c->evm1));
    c->map_ms_pending = false;
  }
  if (map_ms) *map_ms = c->map_ms;
  if (align_ms) *align_ms = c->align_ms;
  return NDT_OK;
}

int ndt_kernel_timing(ndt_ctx *c, int back, float *match_ms, float *fitness_ms) {
  Event *evr = c ? c->ring.back(back) : nullptr;
  if (!evr) return fail(c, NDT_E_ARG, "ndt_kernel_timing: no such launch in the ring");
  HIP_TRY(c, hipEventSynchronize(evr[2]));
  float a = 0.f, f = 0.f;
  HIP_TRY(c, hipEventElapsedTime(&a, evr[0], evr[1]));
  HIP_TRY(c, hipEventElapsedTime(&f, evr[1], evr[2]));
  if (match_ms) *match_ms = a;
  if (fitness_ms) *fitness_ms = f;
  return NDT_OK;
}

int ndt_launch_interval(ndt_ctx *c, int back, float *interval_ms) {
  Event *e1 = c && interval_ms ? c->ring.back(back) : nullptr, *e0 = e1 ? c->ring.back(back + 1) : nullptr;
  if (!e0) return fail(c, NDT_E_ARG, "ndt_launch_interval: no such pair of launches in the ring");
  HIP_TRY(c, hipEventSynchronize(e1[0]));
  HIP_TRY(c, hipEventElapsedTime(interval_ms, e0[0], e1[0]));
  return NDT_OK;
}

int ndt_ctx_wait_launch(ndt_ctx *c, int back, void *stream) {
  Event *evr = c ? c->ring.back(back) : nullptr;
  if (!evr) return fail(c, NDT_E_ARG, "ndt_ctx_wait_launch: no such launch in the ring");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamWaitEvent(stream ? (hipStream_t)stream : c->stream, evr[2], 0));
  return NDT_OK;
}

int ndt_map_destroy(ndt_map *m) {
  if (!m) return NDT_E_ARG;
  bool ctx_live;
  { std::lock_guard<std::mutex> lk(g_live_mu); ctx_live = g_live_ctx.count(m->ctx) != 0; }
  hipError_t e = hipSetDevice(m->device);
  // A context destroyed before its map (the header asks for the other order; a garbage collector that frees both
  // together, such as Python's for objects on a reference cycle, may not keep it) has drained its streams already and
  // is gone: nothing of it is touched then.
  if (ctx_live) {
    if (m->ctx->pending_map == m) {             // an open ndt_map_rebuild_begin dies with its map
      if (m->ctx->side) e = hipStreamSynchronize(m->ctx->side);
      m->ctx->pending_map = nullptr;
    }
    e = hipStreamSynchronize(m->ctx->stream);
    if (m->ctx->side) e = hipStreamSynchronize(m->ctx->side);
  }
  (void)e;
  delete m;                                     // (its buffers: on this device, after the work above has drained)
  return NDT_OK;
}

// The launch geometry of a build of n points on grid G -- the rule of both build paths: queue_build launches with it,
// build_batch puts it into its BuildJobs and prefix sums.  (tiles: MapView::tiles, 8 x 8 voxels per word, a border of one word.)
struct BuildGeom {
  size_t ng, npad, ntile8;            // voxels, voxels with the border, occupancy words
  int tiles_w, ntiles, big_cap;       // occupancy words per row; tiles of the scan; room for voxels with > kBigVoxel points
  unsigned small_blocks, finalize_blocks;   // map_order's blocks of small voxels; map_finalize
  BuildGeom(size_t n, const GridDims &G)
      : ng((size_t)G.div_x * G.div_y), npad((size_t)G.gw * G.gh), ntile8((size_t)((G.div_x + 7) / 8 + 2) * ((G.div_y + 7) / 8 + 2)),
        tiles_w((G.div_x + 7) / 8 + 2), ntiles((int)((ng + kScanTile - 1) / kScanTile)), big_cap((int)(n / kBigVoxel + 1)),
        small_blocks((unsigned)((ng + kOrderVoxPerBlock - 1) / kOrderVoxPerBlock)),
        finalize_blocks((unsigned)((ng + 255) / 256)) {}
};
// ... and of the kernels over the points alone (map_minmax_kernel; map_count_kernel and map_scatter_kernel)
static int minmax_blocks(size_t n) { return grid_for(n, 256 * 32, 128); }
static int point_blocks(size_t n) { return grid_for(n, 256); }

// Step 2 of the map build: the map's buffers for n points on a grid of ng voxels (npad with the border), grow-only across
// rebuilds.  A grown count buffer is marked not clean; *state_grown: the scan's words were reallocated -- the caller clears
// them (no word may carry a tag by accident).
static int ensure_build_buffers(ndt_ctx *ctx, ndt_map *m, size_t n, const BuildGeom &g, bool *state_grown) {
  int rc; bool grown = false;
  if ((rc = m->count.ensure(ctx, g.ng + 1, &grown))) return rc;
  if (grown) m->count_clean = false;
  if ((rc = m->start.ensure(ctx, g.ng + 1 + 8))) return rc;   // 4 readable ints before, 3 after (nearest_sq)
  if ((rc = m->npts_grid.ensure(ctx, g.ng + 1))) return rc;
  if ((rc = m->scan_state.ensure(ctx, 2 * (size_t)g.ntiles + 2, state_grown))) return rc;
  if ((rc = m->perm.ensure(ctx, n + 4))) return rc;       // + 4: map_order_kernel reads four numbers at a time
  if ((rc = m->big.ensure(ctx, (size_t)g.big_cap))) return rc;   // voxels with > kBigVoxel points
  if ((rc = m->occ.ensure(ctx, (g.ng + 31) / 32 + 2))) return rc;
  if ((rc = m->tiles.ensure(ctx, g.ntile8))) return rc;
  if ((rc = m->pts.ensure(ctx, n))) return rc;
  if ((rc = m->cent.ensure(ctx, g.npad))) return rc;
  if ((rc = m->rec.ensure(ctx, g.npad * 8))) return rc;
  return NDT_OK;
}

// The tag of a build's scan words (never 0: cleared words carry no tag).
static unsigned next_scan_tag(ndt_map *m) {
  m->scan_seq = (m->scan_seq + 1u) & 0x3fffffffu;
  if (m->scan_seq == 0u) m->scan_seq = 1u;
  return m->scan_seq;
}

static LeafParams leaf_of(const ndt_params *prm) {
  LeafParams L;
  L.min_pts = prm->min_pts; L.cov_unbiased = prm->cov_unbiased; L.cov_init_identity = prm->cov_init_identity;
  L.eig_mult = prm->eig_mult;
  return L;
}

// The host side of a build, in two steps -- the rule of both build paths.  build_requested: what is to be built, before
// anything is queued (the two-phase build's second half reads it back).  build_queued: what the build's kernels, once queued
// on grid G, leave -- the map's view (what the match and fitness kernels read), its info and the grid kept for the next build.
static void build_requested(ndt_map *m, const float *xy, size_t n, size_t stride, const ndt_params *prm) {
  m->prm = *prm; m->n = n; m->info_valid = false;
  m->pend_xy = xy; m->pend_stride = stride; m->pend_queued = false;
}
static void build_queued(ndt_map *m, const GridDims &G) {
  const BuildGeom g(m->n, G);
  const ndt_params *prm = &m->prm;
  m->ng = g.ng; m->npad = g.npad;
  MapView &V = m->view;
  V.inv_leaf = G.inv_leaf; V.leaf = prm->resolution;
  V.r2 = (float)((double)prm->resolution * (double)prm->resolution);
  V.radius_inclusive = prm->radius_inclusive; V.transform_sse = prm->transform_sse;
  V.min_bx = G.min_bx; V.min_by = G.min_by; V.div_x = G.div_x; V.div_y = G.div_y; V.gw = G.gw; V.gh = G.gh;
  V.cent = m->cent.p; V.rec = m->rec.p; V.occ = m->occ.p; V.tiles = m->tiles.p; V.tiles_w = g.tiles_w; V.pt_start = m->start.p + 4;
  V.pts = m->pts.p;
  gauss_constants(*prm, &V.d1, &V.d2);
  V.e_hi = pair_check_threshold(V.d2);
  m->info.min_bx = G.min_bx; m->info.min_by = G.min_by; m->info.div_x = G.div_x; m->info.div_y = G.div_y;
  m->info.n_points = m->n;
  m->grid = G; m->have_grid = true;
  m->count_clean = true;                // (a complete build: map_scatter_kernel takes back what map_count_kernel added)
}

// Steps 2-4 of the map build for a given voxel grid: everything after the bounding box, queued on
// the context's stream.  The cloud, its parameters and n are the map's (build_requested).
static int queue_build(ndt_ctx *ctx, ndt_map *m, const GridDims &G, bool requeue = false) {
  hipStream_t st = ctx->stream;
  const float *xy = m->pend_xy; const size_t n = m->n, stride = m->pend_stride;
  const BuildGeom g(n, G);

  // 2. buffers (grow-only across rebuilds)
  {
    bool grown = false;
    const int rc = ensure_build_buffers(ctx, m, n, g, &grown);
    if (rc) return rc;
    if (grown)      // no word may carry a tag by accident
      HIP_TRY(ctx, hipMemsetAsync(m->scan_state.p, 0, m->scan_state.cap() * sizeof(unsigned long long), st));
  }
  // No clearing in the steady state (every memset is a kernel of its own between the build's kernels): the per-voxel
  // counters are zero again after a complete build (map_scatter_kernel takes back what map_count_kernel added), the
  // four small counters are cleared by map_count_kernel, the scan's words carry the build's tag, the readable ints in
  // front of `start` are written by scan_onepass_kernel.
  if (!m->count_clean) HIP_TRY(ctx, hipMemsetAsync(m->count.p, 0, m->count.cap() * sizeof(int), st));
  m->count_clean = false;
  // (records of voxels outside the search set are never read: no clearing of m->rec)
  // (the centroid grid is reset on the side stream, beside the bucketing chain; joined in front of the statistics)
  // A build queued AGAIN (build_end found the speculative grid wrong) must not reset the grid before the speculative
  // build's statistics kernel -- on the main stream, writing centroids at the stale grid's indices -- has finished:
  // the side stream was forked only once, in build_begin.  Its centroids would otherwise survive the reset as phantom
  // voxels (the slow path of ndt_point.hip.h reads the grid without an occupancy test).
  if (requeue) {
    HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, st));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
  }
  fill_f2_kernel<<<grid_for(g.npad, 256), 256, 0, ctx->side>>>(m->cent.p, g.npad, INFINITY, m->tiles.p, g.ntile8);
  HIP_TRY(ctx, hipEventRecord(ctx->ev_join, ctx->side));

  // 3. bucket the points by voxel, cloud order kept inside a bucket
  map_count_kernel<<<point_blocks(n), 256, 0, st>>>(xy, stride, n, G, m->count.p, m->counters.p);
  int *const start = m->start.p + 4;
  const unsigned tag = next_scan_tag(m);
  scan_onepass_kernel<<<g.ntiles, kScanBlock, 0, st>>>(m->count.p, g.ng, m->scan_state.p, tag, g.ntiles, m->counters.p + 3, start,
                                                       m->big.p, m->counters.p + 2, g.big_cap);
  map_scatter_kernel<<<point_blocks(n), 256, 0, st>>>(xy, stride, n, G, start, m->count.p, m->perm.p);
  HIP_TRY(ctx, hipGetLastError());
  m->count_clean = true;
  map_order_kernel<<<g.small_blocks + kBigBlocks, 256, 0, st>>>(start, g.ng, g.small_blocks, m->big.p, m->counters.p + 2, g.big_cap, m->perm.p, xy, stride, m->pts.p);
  HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_join, 0));

  // 4. per-voxel statistics -> centroid grid + cell records + bucketed raw points
  const LeafParams L = leaf_of(&m->prm);
  // evm1 -- the end of the build, for ndt_kernel timing and for launches on other streams -- rides on this kernel's own
  // dispatch (an hipEventRecord is a packet of its own: ~6 us between two kernels, tools/launch_gap.py)
  hipExtLaunchKernelGGL(map_finalize_kernel<false>, dim3(g.finalize_blocks), dim3(256), 0, st, nullptr, ctx->evm1, 0, G, L, start,
                        m->pts.p, m->cent.p, m->rec.p, m->npts_grid.p, m->counters.p, m->occ.p, m->tiles.p, g.tiles_w,
                        (const BuildBatch *)nullptr);
  HIP_TRY(ctx, hipGetLastError());
  build_queued(m, G);
  return NDT_OK;
}

// Makes `st` wait for the ends of the launches that read map m (ndt_map::readers): all, or only the unfinished deferred ones.
// The alive check, the read of the reader's ring and the wait happen under ONE hold of the registry's mutex: a concurrent
// ndt_ctx_destroy or launch on another host thread cannot slip in between.  (A launch that has left its ring is waited for
// through the latest one, LaunchRing::end: skipping it would let the build rewrite tables under a launch still running.)
static int wait_for_readers(ndt_ctx *ctx, const ndt_map *m, hipStream_t st, bool deferred_only) {
  std::lock_guard<std::mutex> lk(g_live_mu);
  for (const auto &r : m->readers) {
    if (g_live_ctx.count(r.first) == 0 || r.first->ring.launches <= r.second) continue;   // gone (it synchronised on the way out) / never launched
    LaunchRing &R = r.first->ring;
    const hipEvent_t end = R.end(r.second);
    if (deferred_only) {
      if (!R.deferred(r.second) || hipEventQuery(end) == hipSuccess) continue;            // not deferred / finished: no barrier packet
      (void)hipGetLastError();                     // (hipErrorNotReady is no failure: not left behind for the build's launch checks)
    }
    HIP_TRY(ctx, hipStreamWaitEvent(st, end, 0));
  }
  return NDT_OK;
}

// A build takes the map over from the launches that read its previous one.  Those are the caller's to order before the build
// (stream order / ndt_ctx_wait_launch), except for deferred fitness kernels (NDT_OPT_DEFER_FITNESS, their context's own stream):
// waited for here.  The list starts again with the launches that read the new build.
static int take_over_from_readers(ndt_ctx *ctx, ndt_map *m, hipStream_t st) {
  const int rc = wait_for_readers(ctx, m, st, /*deferred_only=*/true);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(g_live_mu);
  m->readers.clear();
  return NDT_OK;
}

// The build in two halves.  build_begin queues everything: the bounding box of the cloud (getMinMax3D) with its
// read-back on the side stream, and -- instead of idling the GPU during that round trip -- the rest of the build with
// the voxel grid of the previous build of this map (a SLAM local map keeps its voxel bounding box for many scans).
// build_end waits for the read-back, derives the grid on the host and queues the build again only if it differs.
// Any failure leaves the map without a speculative grid.
static int build_begin(ndt_ctx *ctx, ndt_map *m, const float *xy, size_t n, size_t stride, const ndt_params *prm) {
  hipStream_t st = ctx->stream;
  build_requested(m, xy, n, stride, prm);
  { const int rc = take_over_from_readers(ctx, m, st); if (rc) return rc; }      // (ahead of the fork below)
  // The bounding box (and the reset of the centroid grid, queue_build) run on a side stream beside the bucketing
  // chain -- a dozen dependent kernels whose launch latencies add up -- and are joined in front of the statistics.
  // (One record serves as the start of the build's timing and as the fork.)
  HIP_TRY(ctx, hipEventRecord(ctx->evm0, st));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->side, ctx->evm0, 0));
  map_minmax_kernel<<<minmax_blocks(n), 256, 0, ctx->side>>>(xy, stride, n, m->bounds.p, m->bounds.p + 4);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_bounds.p, m->bounds.p + 4, 4 * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->side));
  HIP_TRY(ctx, hipEventRecord(ctx->evb, ctx->side));
  const float inv_leaf = 1.0f / prm->resolution;
  if (m->have_grid && m->grid.inv_leaf == inv_leaf) {
    int rc = queue_build(ctx, m, m->grid);
    if (rc) return rc;
    m->pend_queued = true;                                 // (evm1, what launches queued before build_end wait for: queue_build)
  }
  m->pending = true;
  ctx->pending_map = m;
  return NDT_OK;
}

// The voxel grid of a build from its cloud's bounding box hb (min x, min y, max x, max y, order-encoded: map_minmax_kernel)
// -- the rule of both build paths.  prev: the grid of the map's previous build at this leaf size (what ndt_map_rebuild_begin
// queued ahead), or nullptr.  ndt_params::grid_margin: prev is kept (*same) if it contains the cloud's box and is not much
// wider; otherwise the grid is the box widened by the margin.  NDT_E_GRID (text: `who`: ...) beyond 2^28 cells.
static int grid_of_box(ndt_ctx *ctx, const unsigned *hb, const ndt_params *prm, const GridDims *prev, GridDims *out, bool *same_out,
                       const std::string &who) {
  const float inv_leaf = 1.0f / prm->resolution;
  const float mnx = ord2f(hb[0]), mny = ord2f(hb[1]), mxx = ord2f(hb[2]), mxy = ord2f(hb[3]);
  GridDims G;
  G.inv_leaf = inv_leaf;
  auto vox = [&](float x) { return (int)voxel_coord(x, inv_leaf); };   // (voxel_of's own rule: the device's function)
  G.min_bx = vox(mnx); G.min_by = vox(mny);
  long long dx = (long long)vox(mxx) - G.min_bx + 1;
  long long dy = (long long)vox(mxy) - G.min_by + 1;
  // ndt_params::grid_margin: the grid queued ahead is good if it contains the cloud's box and is not much wider
  const int mg = prm->grid_margin > 0 ? (prm->grid_margin < 4096 ? prm->grid_margin : 4096) : 0;
  bool same = false;
  if (prev) {
    const GridDims &S = *prev;
    const long long lo_x = (long long)G.min_bx - S.min_bx, lo_y = (long long)G.min_by - S.min_by;       // slack on the low sides
    const long long hi_x = ((long long)S.min_bx + S.div_x) - ((long long)G.min_bx + dx);
    const long long hi_y = ((long long)S.min_by + S.div_y) - ((long long)G.min_by + dy);
    same = lo_x >= 0 && lo_y >= 0 && hi_x >= 0 && hi_y >= 0 && lo_x <= 2 * mg && lo_y <= 2 * mg && hi_x <= 2 * mg && hi_y <= 2 * mg;
  }
  if (same) G = *prev;
  else {
    G.min_bx -= mg; G.min_by -= mg; dx += 2 * mg; dy += 2 * mg;
    if (dx > (1LL << 28) || dy > (1LL << 28) || dx * dy > (1LL << 28))      // (each factor first: the product of two 2^32s overflows)
      return fail(ctx, NDT_E_GRID, who + ": voxel grid larger than 2^28 cells");
    G.div_x = (int)dx; G.div_y = (int)dy; G.gw = G.div_x + 4; G.gh = G.div_y + 4;
  }
  *out = G; *same_out = same;
  return NDT_OK;
}

// Returns NDT_OK, or 1 if a build queued by build_begin used a grid that turned out wrong and has been queued again.
static int build_end(ndt_ctx *ctx, ndt_map *m) {
  hipStream_t st = ctx->stream;
  const ndt_params *prm = &m->prm;
  m->pending = false;
  ctx->pending_map = nullptr;
  const unsigned *hb = ctx->h_bounds.p;          // pinned
  HIP_TRY(ctx, hipEventSynchronize(ctx->evb));
  if (hb[0] == 0xffffffffu) return fail(ctx, NDT_E_ARG, "ndt_map_build: no finite points");
  GridDims G; bool same = false;
  { const int rc = grid_of_box(ctx, hb, prm, m->pend_queued ? &m->grid : nullptr, &G, &same, "ndt_map_build"); if (rc) return rc; }
  int redone = 0;
  if (!same) {
    if (m->pend_queued) {
      // the launches queued since build_begin read the speculative build's tables: the build that replaces them waits
      // for the last of them on every context that issued any (the event on that launch's last kernel)
      int rc = wait_for_readers(ctx, m, st, /*deferred_only=*/false);
      if (rc) return rc;
    }
    int rc = queue_build(ctx, m, G, /*requeue=*/m->pend_queued);
    if (rc) return rc;
    redone = m->pend_queued ? 1 : 0;
  }
  m->grid = G; m->have_grid = true;            // (again: a refused build between begin and end has withdrawn the grid, ndt_map_build_dev)
  ctx->map_ms_pending = true;
  return redone;                               // asynchronous from here on (stream order)
}

static int map_build_impl(ndt_ctx *ctx, ndt_map *m, const float *xy, size_t n, size_t stride, const ndt_params *prm) {
  if (ctx->pending_map) return fail(ctx, NDT_E_ARG, "ndt_map_build: ndt_map_rebuild_end is still owed for a map of this context");
  int rc = build_begin(ctx, m, xy, n, stride, prm);
  if (rc) { m->pending = false; ctx->pending_map = nullptr; return rc; }
  rc = build_end(ctx, m);
  return rc < 0 ? rc : NDT_OK;
}

// A new map of ctx with the buffers every build path expects: map_minmax_kernel's running box at its start values, the
// build's small counters.
static int new_map(ndt_ctx *ctx, ndt_map **out) {
  ndt_map *m = new (std::nothrow) ndt_map();
  if (!m) return NDT_E_NOMEM;
  m->ctx = ctx;
  m->device = ctx->device;
  const unsigned init_b[16] = {0xffffffffu, 0xffffffffu, 0u, 0u};     // running bounding box, result, done-counter (map_minmax_kernel)
  int rc = m->bounds.alloc(ctx, sizeof(init_b));
  const hipError_t e = rc ? hipSuccess : hipMemcpy(m->bounds.p, init_b, sizeof(init_b), hipMemcpyHostToDevice);
  if (e != hipSuccess) rc = fail(ctx, NDT_E_HIP, std::string("ndt_map_build: hipMemcpy: ") + hipGetErrorString(e));
  if (rc == NDT_OK) rc = m->counters.alloc(ctx, 4 * sizeof(int));
  if (rc) { ndt_map_destroy(m); return rc; }
  *out = m;
  return NDT_OK;
}

int ndt_map_build_dev(ndt_ctx *ctx, const float *xy, size_t n, size_t stride, const ndt_params *prm,
                      ndt_map **pmap) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!xy || n == 0 || !prm || !pmap || !(prm->resolution > 0) || stride < 8 || (stride & 7))
    return fail(ctx, NDT_E_ARG, "ndt_map_build: bad arguments (need n > 0, resolution > 0, stride % 8 == 0)");
  if (n > (size_t)INT32_MAX) return fail(ctx, NDT_E_ARG, "ndt_map_build: more than 2^31 points");
  if (*pmap && (*pmap)->ctx != ctx) return fail(ctx, NDT_E_ARG, "ndt_map_build: the map belongs to another context");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ndt_map *m = *pmap;
  const bool fresh = (m == nullptr);
  if (fresh) {
    const int rc = new_map(ctx, &m);
    if (rc) return rc;
  }
  const int rc = map_build_impl(ctx, m, xy, n, stride, prm);
  if (rc) {
    m->have_grid = false;                      // a half-queued speculative build must not be trusted next time
    if (fresh) ndt_map_destroy(m);             // (an existing map stays with its owner, unusable until rebuilt)
    return rc;
  }
  *pmap = m;
  return NDT_OK;
}


int ndt_map_rebuild_begin(ndt_ctx *ctx, const float *xy, size_t n, size_t stride, const ndt_params *prm, ndt_map *m) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!xy || n == 0 || !prm || !m || !(prm->resolution > 0) || stride < 8 || (stride & 7) || n > (size_t)INT32_MAX)
    return fail(ctx, NDT_E_ARG, "ndt_map_rebuild_begin: bad arguments");
  if (m->ctx != ctx) return fail(ctx, NDT_E_ARG, "ndt_map_rebuild_begin: the map belongs to another context");
  if (ctx->pending_map) return fail(ctx, NDT_E_ARG, "ndt_map_rebuild_begin: ndt_map_rebuild_end is still owed for a map of this context");
  if (!m->have_grid || m->grid.inv_leaf != 1.0f / prm->resolution)
    return fail(ctx, NDT_E_ARG, "ndt_map_rebuild_begin: the map has no earlier build at this resolution (use ndt_map_build_dev)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int rc = build_begin(ctx, m, xy, n, stride, prm);
  if (rc) { m->have_grid = false; m->pending = false; ctx->pending_map = nullptr; }
  return rc;
}

int ndt_map_rebuild_end(ndt_ctx *ctx, ndt_map *m) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!m || m->ctx != ctx || !m->pending || ctx->pending_map != m)
    return fail(ctx, NDT_E_ARG, "ndt_map_rebuild_end: no ndt_map_rebuild_begin is open for this map");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int rc = build_end(ctx, m);
  if (rc < 0) m->have_grid = false;
  return rc;
}

int ndt_map_build(ndt_ctx *ctx, const float *xy_host, size_t n, size_t stride, const ndt_params *prm,
                  ndt_map **pmap) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!xy_host || n == 0 || !pmap || stride < 8 || (stride & 7)) return fail(ctx, NDT_E_ARG, "ndt_map_build: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // stage through a buffer owned by the map once it exists; first build uses a temporary
  DevBuf<unsigned char> stage;
  if (*pmap) stage = std::move((*pmap)->xy_stage);
  int rc = stage.ensure(ctx, n * stride);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(stage.p, xy_host, n * stride, hipMemcpyHostToDevice, ctx->stream));
  rc = ndt_map_build_dev(ctx, (const float *)stage.p, n, stride, prm, pmap);
  if (rc == NDT_OK) { hipError_t e = hipStreamSynchronize(ctx->stream); if (e != hipSuccess) rc = fail(ctx, NDT_E_HIP, hipGetErrorString(e)); }   // host-pointer form: synchronous
  if (*pmap) (*pmap)->xy_stage = std::move(stage);
  return rc;
}

// ---- batched builds (ndt_map_build_batch_dev / ndt_map_build_batch) ----

// The synchronous refusals of a batched build: nothing changed, nothing created, nothing queued.
static int check_build_batch(ndt_ctx *ctx, const float *const *xy, const size_t *n, size_t stride, int n_maps, const ndt_params *prm,
                             ndt_map **maps, const std::string &fn) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (n_maps < 1) return fail(ctx, NDT_E_ARG, fn + ": n_maps < 1");
  if (!xy || !n || !prm || !maps) return fail(ctx, NDT_E_ARG, fn + ": NULL array (xy, n, prm or maps)");
  if (stride < 8 || (stride & 7)) return fail(ctx, NDT_E_ARG, fn + ": bad stride (need stride_bytes >= 8 and % 8 == 0)");
  if (ctx->pending_map) return fail(ctx, NDT_E_ARG, fn + ": ndt_map_rebuild_end is still owed for a map of this context");
  std::vector<std::pair<const ndt_map *, int>> seen;
  for (int s = 0; s < n_maps; ++s) {
    const std::string which = fn + ": map " + std::to_string(s);
    if (!xy[s]) return fail(ctx, NDT_E_ARG, which + ": NULL cloud");
    if (n[s] == 0) return fail(ctx, NDT_E_ARG, which + ": no points (n == 0)");
    if (n[s] > (size_t)INT32_MAX) return fail(ctx, NDT_E_ARG, which + ": more than 2^31 points");
    if (!(prm[s].resolution > 0)) return fail(ctx, NDT_E_ARG, which + ": resolution <= 0");
    if (!maps[s]) continue;
    if (maps[s]->ctx != ctx) return fail(ctx, NDT_E_ARG, which + " belongs to another context");
    seen.emplace_back(maps[s], s);
  }
  std::sort(seen.begin(), seen.end());
  int dup = -1, first = -1;                             // the first index that repeats an earlier map, and that map's first index
  for (size_t k = 1; k < seen.size(); ++k)             // (sorted: a map's indices in ascending order; k the second of its map)
    if (seen[k].first == seen[k - 1].first && (k < 2 || seen[k - 2].first != seen[k].first) && (dup < 0 || seen[k].second < dup)) {
      dup = seen[k].second;
      first = seen[k - 1].second;
    }
  if (dup >= 0)
    return fail(ctx, NDT_E_ARG, fn + ": map " + std::to_string(dup) + " is map " + std::to_string(first) + " again");
  return NDT_OK;
}

// One set of launches for every map: the bounding boxes (one kernel, ONE read-back and host wait), the grids by the rule of
// the single-map path (grid_of_box, with each map's previous grid), one job-table upload, then each kernel of the chain once.
// Each map comes out as ndt_map_build_dev would leave it.
// map_status == nullptr (the public entry points): all or nothing -- the first map whose box refuses fails the call with
// nothing built.  map_status != nullptr (the sessions step): n_maps codes; a map whose box refuses (no finite points, a grid
// beyond 2^28 cells) gets its code, is left exactly as it was (a NULL maps[s] stays NULL) and owns no workgroup of any kernel
// behind the boxes; every other map is built in the same launches and the call returns NDT_OK.
static int build_batch(ndt_ctx *ctx, const float *const *xy, const size_t *n, size_t stride, int n_maps, const ndt_params *prm,
                       ndt_map **maps, const std::string &fn, int *map_status = nullptr) {
  hipStream_t st = ctx->stream;
  const size_t S = (size_t)n_maps, npre = S + 1;
  // staging / device table: [BuildBatch | BoxJob x S | minmax prefixes] [BuildJob x S | prefixes of the other kernels]; the
  // first part goes up ahead of the boxes, the second (the job table proper) once the grids are known
  Regions T;
  T.take(sizeof(BuildBatch), 256);
  const size_t o_box = T.take(S * sizeof(BoxJob), 256), o_pre0 = T.take(npre * sizeof(unsigned), alignof(unsigned)),
               o_jobs = T.take(S * sizeof(BuildJob), 256), o_pre = T.take((kBbKernels - 1) * npre * sizeof(unsigned), 256), bytes = T.end;
  int rc;
  if ((rc = ctx->bb_tab.reserve(ctx, bytes))) return rc;           // (waits for the previous batched build's upload)
  if ((rc = ctx->d_bb.ensure(ctx, bytes))) return rc;
  if ((rc = ctx->h_boxes.ensure(ctx, 16 * S))) return rc;
  {
    bool grown = false;
    if ((rc = ctx->d_boxes.ensure(ctx, 16 * (S + 1), &grown))) return rc;
    if (grown) {                                       // every map's running box at its start values (map_minmax_kernel)
      std::vector<unsigned> init(ctx->d_boxes.cap(), 0u);
      for (size_t w = 16; w + 16 <= init.size(); w += 16) init[w] = init[w + 1] = 0xffffffffu;
      HIP_TRY(ctx, hipMemcpy(ctx->d_boxes.p, init.data(), init.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    }
  }
  unsigned char *h = ctx->bb_tab.h.p, *d = ctx->d_bb.p;
  BuildBatch &BB = *(BuildBatch *)h;
  const BuildBatch *dbb = (const BuildBatch *)d;
  BoxJob *hbox = (BoxJob *)(h + o_box);
  BuildJob *hjob = (BuildJob *)(h + o_jobs);
  unsigned *hpre[kBbKernels];
  BB.box_jobs = (const BoxJob *)(d + o_box); BB.jobs = (const BuildJob *)(d + o_jobs);
  hpre[kBbMinmax] = (unsigned *)(h + o_pre0); BB.pre[kBbMinmax] = (const unsigned *)(d + o_pre0);
  for (int k = 1; k < kBbKernels; ++k) {
    hpre[k] = (unsigned *)(h + o_pre) + (k - 1) * npre;
    BB.pre[k] = (const unsigned *)(d + o_pre) + (k - 1) * npre;
  }
  BB.boxes = ctx->d_boxes.p + 16; BB.ticket = (int *)ctx->d_boxes.p; BB.n_maps = n_maps;
  // a launch's work-items fit in 32 bits (blocks x block size, summed over the maps)
  auto prefixes = [&](int k, int block, auto &&blocks_of) -> int {
    unsigned long long tot = 0;
    for (size_t s = 0; s < S; ++s) {
      hpre[k][s] = (unsigned)tot;
      tot += (unsigned long long)blocks_of(s);
      if (tot * (unsigned long long)block > 0xffffffffull)
        return fail(ctx, k <= kBbCount || k == kBbScatter ? NDT_E_ARG : NDT_E_GRID, fn + ": the maps of the call need more than 2^32 work-items in one kernel");
    }
    hpre[k][S] = (unsigned)tot;
    return NDT_OK;
  };
  std::vector<char> refused(S, 0);                    // (map_status alone: the maps that take no part behind the boxes)
  size_t n_refused = 0;
  if ((rc = prefixes(kBbMinmax, 256, [&](size_t s) { return minmax_blocks(n[s]); }))) return rc;
  if ((rc = prefixes(kBbCount, 256, [&](size_t s) { return point_blocks(n[s]); }))) return rc;
  if ((rc = prefixes(kBbScatter, 256, [&](size_t s) { return point_blocks(n[s]); }))) return rc;

  // 1. the bounding boxes of all clouds, read back with one copy and one wait
  for (size_t s = 0; s < S; ++s) { hbox[s].xy = xy[s]; hbox[s].n = n[s]; }
  HIP_TRY(ctx, hipEventRecord(ctx->evm0, st));
  HIP_TRY(ctx, hipMemcpyAsync(d, h, o_jobs, hipMemcpyHostToDevice, st));
  map_minmax_kernel<true><<<hpre[kBbMinmax][S], 256, 0, st>>>(nullptr, stride, 0, nullptr, nullptr, dbb);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_boxes.p, ctx->d_boxes.p + 16, 16 * S * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipEventRecord(ctx->evb, st));
  HIP_TRY(ctx, hipEventSynchronize(ctx->evb));

  // 2. the grids; the refusals that need the boxes change nothing either
  std::vector<GridDims> grids(S);
  std::vector<BuildGeom> geom;
  geom.reserve(S);
  for (size_t s = 0; s < S; ++s) {
    const std::string which = fn + ": map " + std::to_string(s);
    const unsigned *hb = ctx->h_boxes.p + 16 * s + 4;
    const ndt_map *m = maps[s];
    const bool prev = m && m->have_grid && m->grid.inv_leaf == 1.0f / prm[s].resolution;   // (what ndt_map_rebuild_begin would queue ahead)
    bool same = false;
    rc = hb[0] == 0xffffffffu ? fail(ctx, NDT_E_ARG, which + ": no finite points")
                              : grid_of_box(ctx, hb, &prm[s], prev ? &m->grid : nullptr, &grids[s], &same, which);
    if (map_status) map_status[s] = rc;
    if (rc) {
      if (!map_status) return rc;
      refused[s] = 1; ++n_refused; grids[s] = GridDims{};
    }
    geom.emplace_back(n[s], grids[s]);
  }
  if (n_refused == S) return NDT_OK;                   // (map_status: nothing to build, nothing queued)
  if (n_refused) {                                     // a refused map owns no workgroup: zero-width rows of the prefixes
    if ((rc = prefixes(kBbCount, 256, [&](size_t s) { return refused[s] ? 0 : point_blocks(n[s]); }))) return rc;
    if ((rc = prefixes(kBbScatter, 256, [&](size_t s) { return refused[s] ? 0 : point_blocks(n[s]); }))) return rc;
  }
  if ((rc = prefixes(kBbScan, kScanBlock, [&](size_t s) { return refused[s] ? 0 : geom[s].ntiles; }))) return rc;
  if ((rc = prefixes(kBbOrder, 256, [&](size_t s) {      // (the big voxels' blocks: no more than the map can need, not kBigBlocks for each)
         return refused[s] ? (size_t)0
                           : (size_t)geom[s].small_blocks + std::min<size_t>(kBigBlocks, ((size_t)geom[s].big_cap + kBigWavesPerBlock - 1) / kBigWavesPerBlock); })))
    return rc;
  if ((rc = prefixes(kBbFinalize, 256, [&](size_t s) { return refused[s] ? 0u : geom[s].finalize_blocks; }))) return rc;

  // 3. the maps: new ones created, every one's readers waited for as build_begin does, buffers, jobs
  std::vector<ndt_map *> mp(S, nullptr), made;
  auto failed = [&](int code) {                        // a HIP / allocation failure from here on: as ndt_map_build_dev
    for (size_t s = 0; s < S; ++s)
      if (maps[s] && !refused[s]) { maps[s]->have_grid = false; maps[s]->count_clean = false; }
    for (ndt_map *m : made) ndt_map_destroy(m);
    return code;
  };
  for (size_t s = 0; s < S; ++s) {
    if (refused[s]) continue;
    if (maps[s]) { mp[s] = maps[s]; continue; }
    if ((rc = new_map(ctx, &mp[s]))) return failed(rc);
    made.push_back(mp[s]);
  }
  for (size_t s = 0; s < S; ++s) {
    if (refused[s]) continue;
    ndt_map *m = mp[s];
    const BuildGeom &g = geom[s];
    if ((rc = take_over_from_readers(ctx, m, st))) return failed(rc);
    bool state_grown = false;
    if ((rc = ensure_build_buffers(ctx, m, n[s], g, &state_grown))) return failed(rc);
    BuildJob &J = hjob[s];
    J.xy = xy[s]; J.n = n[s]; J.G = grids[s]; J.L = leaf_of(&prm[s]);
    J.count = m->count.p; J.start = m->start.p + 4; J.perm = m->perm.p; J.big = m->big.p; J.npts_grid = m->npts_grid.p;
    J.counters = m->counters.p; J.scan_state = m->scan_state.p; J.tag = next_scan_tag(m);
    J.ntiles = g.ntiles; J.big_cap = g.big_cap; J.small_blocks = g.small_blocks;
    J.pts = m->pts.p; J.cent = m->cent.p; J.rec = m->rec.p; J.occ = m->occ.p; J.tiles = m->tiles.p; J.tiles_w = g.tiles_w;
    J.ng = g.ng; J.npad = g.npad; J.ntile8 = g.ntile8;
    J.zero_count = m->count_clean ? 0 : m->count.cap();
    J.zero_state = state_grown ? m->scan_state.cap() : 0;
    m->count_clean = false;
  }
  if ((rc = prefixes(kBbFill, 256, [&](size_t s) {
         if (refused[s]) return 0;
         const BuildJob &J = hjob[s];
         return grid_for(std::max(std::max(J.npad, J.ntile8), std::max(J.zero_count, J.zero_state)), 256); })))
    return failed(rc);

  // 4. one upload of the jobs, then each kernel of the chain once (evm1 on the last one's dispatch, as queue_build)
  {
    const hipError_t e = ctx->bb_tab.upload(d + o_jobs, o_jobs, bytes - o_jobs, st);
    if (e != hipSuccess) return failed(fail(ctx, NDT_E_HIP, fn + ": job table upload: " + hipGetErrorString(e)));
  }
  // (the batched instances take every other argument from their map's job)
  const GridDims G0{}; const LeafParams L0{};
  fill_f2_kernel<true><<<hpre[kBbFill][S], 256, 0, st>>>(nullptr, 0, INFINITY, nullptr, 0, dbb);
  map_count_kernel<true><<<hpre[kBbCount][S], 256, 0, st>>>(nullptr, stride, 0, G0, nullptr, nullptr, dbb);
  scan_onepass_kernel<true><<<hpre[kBbScan][S], kScanBlock, 0, st>>>(nullptr, 0, nullptr, 0u, 0, nullptr, nullptr, nullptr, nullptr, 0, dbb);
  map_scatter_kernel<true><<<hpre[kBbScatter][S], 256, 0, st>>>(nullptr, stride, 0, G0, nullptr, nullptr, nullptr, dbb);
  map_order_kernel<true><<<hpre[kBbOrder][S], 256, 0, st>>>(nullptr, 0, 0u, nullptr, nullptr, 0, nullptr, nullptr, stride, nullptr, dbb);
  hipExtLaunchKernelGGL(map_finalize_kernel<true>, dim3(hpre[kBbFinalize][S]), dim3(256), 0, st, nullptr, ctx->evm1, 0, G0, L0,
                        (const int *)nullptr, (const float2 *)nullptr, (float2 *)nullptr, (double *)nullptr, (int *)nullptr, (int *)nullptr,
                        (unsigned *)nullptr, (u64 *)nullptr, 0, dbb);
  { const hipError_t e = hipGetLastError(); if (e != hipSuccess) return failed(fail(ctx, NDT_E_HIP, fn + ": launch: " + hipGetErrorString(e))); }

  // 5. the host side of every map
  for (size_t s = 0; s < S; ++s) {
    if (refused[s]) continue;
    build_requested(mp[s], xy[s], n[s], stride, &prm[s]);
    build_queued(mp[s], grids[s]);
    maps[s] = mp[s];
  }
  ctx->map_ms_pending = true;
  return NDT_OK;
}

int ndt_map_build_batch_dev(ndt_ctx *ctx, const float *const *xy_dev, const size_t *n, size_t stride, int n_maps,
                            const ndt_params *prm, ndt_map **maps) {
  int rc = check_build_batch(ctx, xy_dev, n, stride, n_maps, prm, maps, "ndt_map_build_batch_dev");
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return build_batch(ctx, xy_dev, n, stride, n_maps, prm, maps, "ndt_map_build_batch_dev");
}

int ndt_map_build_batch(ndt_ctx *ctx, const float *const *xy_host, const size_t *n, size_t stride, int n_maps,
                        const ndt_params *prm, ndt_map **maps) {
  int rc = check_build_batch(ctx, xy_host, n, stride, n_maps, prm, maps, "ndt_map_build_batch");
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // the clouds, one after another in the context's staging (each at a 256-byte boundary)
  std::vector<size_t> off((size_t)n_maps);
  Regions C;
  for (int s = 0; s < n_maps; ++s) off[s] = C.take(n[s] * stride, 256);
  if ((rc = ctx->d_bstage.ensure(ctx, C.end))) return rc;
  std::vector<const float *> dxy((size_t)n_maps);
  for (int s = 0; s < n_maps; ++s) {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_bstage.p + off[s], xy_host[s], n[s] * stride, hipMemcpyHostToDevice, ctx->stream));
    dxy[s] = (const float *)(ctx->d_bstage.p + off[s]);
  }
  rc = build_batch(ctx, dxy.data(), n, stride, n_maps, prm, maps, "ndt_map_build_batch");
  if (rc == NDT_OK) { const hipError_t e = hipStreamSynchronize(ctx->stream); if (e != hipSuccess) rc = fail(ctx, NDT_E_HIP, hipGetErrorString(e)); }
  return rc;
}

int ndt_map_info_get(const ndt_map *cm, ndt_map_info *out) {
  if (!cm || !out) return NDT_E_ARG;
  ndt_map *m = const_cast<ndt_map *>(cm);
  if (!m->info_valid) {
    // per-voxel flags: 0 not in the search set, n accepted, -n rejected covariance
    std::vector<int> flags(m->ng);
    HIP_TRY(m->ctx, hipSetDevice(m->ctx->device));
    HIP_TRY(m->ctx, hipMemcpyAsync(flags.data(), m->npts_grid.p, m->ng * sizeof(int), hipMemcpyDeviceToHost, m->ctx->stream));
    HIP_TRY(m->ctx, hipStreamSynchronize(m->ctx->stream));
    int cells = 0, valid = 0;
    for (int f : flags) { cells += f != 0; valid += f > 0; }
    m->info.n_cells = cells; m->info.n_valid = valid;
    m->info_valid = true;
  }
  *out = m->info;
  return NDT_OK;
}

int ndt_map_export(const ndt_map *cm, int *cell_idx, float *cent_xy, double *mean_xy, double *icov,
                   int *npts) {
  if (!cm || !cell_idx || !cent_xy || !mean_xy || !icov || !npts) return NDT_E_ARG;
  ndt_map *m = const_cast<ndt_map *>(cm);
  ndt_ctx *ctx = m->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t ng = m->ng, npad = m->npad;
  std::vector<int> hn(ng);
  std::vector<float2> hc(npad);
  std::vector<double> hr(npad * 8);
  hipError_t e1 = hipMemcpyAsync(hn.data(), m->npts_grid.p, ng * sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
  hipError_t e2 = hipMemcpyAsync(hc.data(), m->cent.p, npad * sizeof(float2), hipMemcpyDeviceToHost, ctx->stream);
  hipError_t e3 = hipMemcpyAsync(hr.data(), m->rec.p, npad * 8 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  hipError_t e4 = hipStreamSynchronize(ctx->stream);
  if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess)
    return fail(ctx, NDT_E_HIP, "ndt_map_export: copy failed");
  size_t k = 0;
  const int gw = m->view.gw, dx = m->view.div_x;
  for (size_t g = 0; g < ng; ++g) {
    if (hn[g] == 0) continue;
    size_t pg = (size_t)(g / dx + 2) * gw + (g % dx + 2);
    cell_idx[k] = (int)g; npts[k] = hn[g];
    cent_xy[2 * k] = hc[pg].x; cent_xy[2 * k + 1] = hc[pg].y;
    mean_xy[2 * k] = hr[pg * 8]; mean_xy[2 * k + 1] = hr[pg * 8 + 1];
    icov[3 * k] = hr[pg * 8 + 2]; icov[3 * k + 1] = hr[pg * 8 + 3]; icov[3 * k + 2] = hr[pg * 8 + 4];
    ++k;
  }
  return NDT_OK;
}

// A batch prepared ahead of its launch (see PrepRec, ndt_match.hip.h).  Asynchronous, on `stream` (NULL: the context's): the
// caller of a stream of batches puts it where the GPU has room -- e.g. behind the map's rebuild on the stream that carries the
// builds -- and issues ndt_align_batch_dev with the SAME arguments later; that call finds the prepared set, makes its stream
// wait for it and starts every scan at the window's staging.
int ndt_align_batch_prepare_dev(ndt_ctx *ctx, const ndt_map *map, const float *scans, const uint64_t *offsets,
                                int B, size_t total_points, int shared_scan, const double *inits, void *stream) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!map || !scans || !offsets || !inits || B <= 0 || total_points == 0)
    return fail(ctx, NDT_E_ARG, "ndt_align_batch_prepare_dev: bad arguments");
  if (map->ctx->device != ctx->device) return fail(ctx, NDT_E_ARG, "ndt_align_batch_prepare_dev: the map was built on another device");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  ndt_ctx::PrepSet &S = ctx->prep[ctx->prep_last ^ 1];
  S.valid = false;
  const size_t slots = (shared_scan ? (size_t)B : (size_t)1) * total_points;
  int rc;
  if ((rc = S.sorted.ensure(ctx, slots + 2))) return rc;
  if ((rc = S.recs.ensure(ctx, (size_t)B))) return rc;
  if ((rc = S.maps.ensure(ctx, (size_t)B * kBitmapBytes))) return rc;
  if (!S.ready && ((rc = S.ev0.create(ctx)) || (rc = S.ready.create(ctx)))) return rc;
  // Of the map it takes the grid's geometry (by value, now) and reads nothing on the device: no wait for a build that may be
  // queued or running -- a two-phase rebuild that ends with another grid simply leaves this set unused.  It is ordered behind
  // the last launch that read this set (its fitness kernels walk the set's ordered copies).
  if (S.reader >= 0 && (unsigned long long)S.reader < ctx->ring.launches)
    HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ring.end((unsigned long long)S.reader), 0));
  // ... and behind the set's own previous order kernel, which no launch may have read (a third prepare call before any launch,
  // the earlier one on another stream)
  if (S.scans) HIP_TRY(ctx, hipStreamWaitEvent(st, S.ready, 0));
  const MapView &V = map->view;
  const OptParams O = opt_of(map->prm);
  const int ncu = ctx->workgroups > 0 ? ctx->workgroups : ctx->num_cus;
  const int grid = B < ncu ? B : ncu;
  with_bool(map->prm.transform_sse != 0, [&](auto Sse) {
    hipExtLaunchKernelGGL((ndt_order_kernel<decltype(Sse)::value>), dim3(grid), dim3(kBlock), 0, st, S.ev0, S.ready, 0, V, O, scans,
                          (const unsigned long long *)offsets, B, shared_scan, inits, S.sorted.p, S.recs.p, (unsigned *)S.maps.p);
  });
  HIP_TRY(ctx, hipGetLastError());
  S.scans = scans; S.offsets = offsets; S.inits = inits; S.map = map; S.B = B; S.shared_scan = shared_scan; S.total_points = total_points;
  S.min_bx = V.min_bx; S.min_by = V.min_by; S.div_x = V.div_x; S.div_y = V.div_y; S.inv_leaf = V.inv_leaf;
  S.P = O; S.transform_sse = map->prm.transform_sse;
  S.valid = true; S.timed = false;
  ctx->prep_last ^= 1;
  return NDT_OK;
}

int ndt_align_batch_dev(ndt_ctx *ctx, const ndt_map *map, const float *scans, const uint64_t *offsets,
                        int B, size_t total_points, int shared_scan, const double *inits, ndt_result *out,
                        void *stream) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!map || !scans || !offsets || !inits || !out || B <= 0) return fail(ctx, NDT_E_ARG, "ndt_align_batch: bad arguments");
  if (map->ctx->device != ctx->device) return fail(ctx, NDT_E_ARG, "ndt_align_batch: the map was built on another device");
  if (total_points == 0) return fail(ctx, NDT_E_ARG, "ndt_align_batch: total_points = 0");
  int rc;
  const bool defer = ctx->defer_fitness != 0;
  CallFrame fr(ctx);
  if ((rc = fr.open(stream, defer))) return rc;
  hipStream_t st = fr.st;
  // a set prepared for exactly this batch against exactly this grid and these parameters?  (A map whose speculative grid turned
  // out wrong has been queued again with another origin -- ndt_map_rebuild_end: NDT_REBUILT --, or a rebuild changed the
  // parameters, or another map took the old one's address, and the set no longer fits: the owners order their scans
  // themselves, as without it.)
  ndt_ctx::PrepSet *pset = nullptr;
  const OptParams O = opt_of(map->prm);
  for (ndt_ctx::PrepSet &S : ctx->prep) {
    const MapView &V = map->view;
    if (S.valid && S.scans == scans && S.offsets == offsets && S.inits == inits && S.map == map && S.B == B &&
        S.shared_scan == shared_scan && S.total_points == total_points && S.min_bx == V.min_bx && S.min_by == V.min_by &&
        S.div_x == V.div_x && S.div_y == V.div_y && same_bits(&S.inv_leaf, &V.inv_leaf, sizeof(float)) &&
        S.transform_sse == map->prm.transform_sse && same_opt(S.P, O))
      pset = &S;
  }
  if (pset) {
    HIP_TRY(ctx, hipStreamWaitEvent(st, pset->ready, 0));
    pset->valid = false;                           // one launch per prepared set (the caller prepares the next batch)
  }
  if ((rc = launch_align(ctx, map, st, scans, (const unsigned long long *)offsets, B, shared_scan, total_points, inits,
                         out, nullptr, 0, nullptr, nullptr, pset, defer)))
    return rc;
  return fr.close();
}

// ms of the order kernel of the prepared set the context's most recent launches used (0 when none); blocks until it has run
int ndt_prepare_timing(ndt_ctx *ctx, float *order_ms) {
  if (!ctx || !order_ms) return NDT_E_ARG;
  *order_ms = 0.f;
  for (ndt_ctx::PrepSet &S : ctx->prep) {
    if (!S.ready || S.reader < 0) continue;
    HIP_TRY(ctx, hipEventSynchronize(S.ready));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, S.ev0, S.ready));
    if (ms > *order_ms) *order_ms = ms;
  }
  return NDT_OK;
}

}  // extern "C"

namespace {

__global__ void __launch_bounds__(256)
repack_f2_kernel(const float *__restrict__ in, size_t stride, size_t n, float2 *__restrict__ out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = load_pt(in, stride, i);
}

// A scan of n points (records of `stride` bytes) as packed float2 on the device, inside the caller's frame: from host memory
// (src_host: uploaded to d_scan, through d_tmp and repacked on the device when stride != 8, e.g. pcl::PointXYZ) or from device
// memory (src_dev: used in place when stride == 8, else repacked into d_scan).
int stage_scan_f2(ndt_ctx *ctx, hipStream_t st, const float *src_host, const float *src_dev, size_t n, size_t stride, const float **packed) {
  if (!src_host && stride == 8) { *packed = src_dev; return NDT_OK; }
  int rc;
  if ((rc = ctx->d_scan.ensure(ctx, n * 8))) return rc;
  if (stride == 8) {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_scan.p, src_host, n * 8, hipMemcpyHostToDevice, st));
  } else {
    if (src_host) {
      if ((rc = ctx->d_tmp.ensure(ctx, n * stride))) return rc;
      HIP_TRY(ctx, hipMemcpyAsync(ctx->d_tmp.p, src_host, n * stride, hipMemcpyHostToDevice, st));
      src_dev = (const float *)ctx->d_tmp.p;
    }
    repack_f2_kernel<<<grid_for(n, 256), 256, 0, st>>>(src_dev, stride, n, (float2 *)ctx->d_scan.p);
  }
  *packed = (const float *)ctx->d_scan.p;
  return NDT_OK;
}

#ifdef NDT_DIAG
// Diagnostic builds only (-DNDT_DIAG, tools/prof_phases.py): per-scan phase timers of the match kernel, printed
// to stderr when NDT_PROF is set.  Release builds contain neither the environment look-up nor the report.
void prof_report(const unsigned long long *hp, int B) {
  double te = 0, ta = 0, tw = 0, ev = 0, sh = 0, hc = 0, worst = 0;
  std::vector<unsigned long long> seen((size_t)B, 0ull);
  auto word = [&](int b, ProfScan k) { return hp[prof_scan_at(b) + k]; };
  auto ticks = [&](int b) { return (word(b, kPsEval) + (word(b, kPsAdv) & 0xFFFFFFFFull)) * 0.01; };
  for (int b = 0; b < B; ++b) {
    te += word(b, kPsEval) * 0.01; ta += (word(b, kPsAdv) & 0xFFFFFFFFull) * 0.01; tw += word(b, kPsWait) * 0.01;
    ev += (double)(word(b, kPsCounts) & 0xFFFF); sh += (double)((word(b, kPsCounts) >> 16) & 0xFFFF); hc += (double)(word(b, kPsCounts) >> 32);
    if (ticks(b) > worst) worst = ticks(b);
  }
  for (int rep = 0; rep < 6 && rep < B; ++rep) {      // the longest scans
    int best = -1; double bt = -1;
    for (int b = 0; b < B; ++b) if (ticks(b) > bt && !seen[b]) { bt = ticks(b); best = b; }
    if (best < 0) break;
    fprintf(stderr, "[NDT_PROF]   scan %3d: %.0f us (fitness pass %.0f us, window spilled %d), passes %llu, shared %llu, helper units %llu, first shared pass at %.0f us (scan started %.0f, first helper attached %.0f, its window ready %.0f)\n", best, bt,
            (double)((word(best, kPsAdv) >> 32) & 0x7FFFFFFFull) * 0.01, (int)(word(best, kPsAdv) >> 63),
            word(best, kPsCounts) & 0xFFFF, (word(best, kPsCounts) >> 16) & 0xFFFF, (word(best, kPsCounts) >> 32) & 0x7FFFFFFF,
            (double)(word(best, kPsStart) >> 32) * 0.01, (double)(word(best, kPsStart) & 0xFFFFFFFFull) * 0.01,
            (double)word(best, kPsAttached) * 0.01, (double)word(best, kPsHelperReady) * 0.01);
    seen[best] = 1;
  }
  fprintf(stderr, "[NDT_PROF] B=%d passes=%.0f (+fitness) | per pass: compute+combine %.2f us, advance %.2f us | shared passes %.0f, helper chunks %.0f, owner wait %.2f us per shared pass | slowest scan %.1f us\n",
          B, ev, te / (ev + B), ta / ev, sh, hc, sh > 0 ? tw / sh : 0.0, worst);
  if (const char *dump = getenv("NDT_PROF_DUMP")) { FILE *f = fopen(dump, "wb"); if (f) { fwrite(hp, prof_scan_bytes(), (size_t)B, f); fclose(f); } }
}
#endif

// The staged part of a host-pointer match call, its frame on the context's stream -- the same for one map and for many:
// scans (stage_scan_f2), offsets, initial guesses and (multi-map calls) map_of go up, `launch(st, d_scans, d_map_of, d_trace,
// d_rows, d_prof)` queues the batch between ev0 and ev1, the records and the trace come back.  Asynchronous:
// align_host_finish waits.
template <typename Launch>
int align_host_staged(ndt_ctx *ctx, const float *scans, size_t stride, const uint64_t *offsets, int B,
                      int shared_scan, const double *inits, const int *map_of, ndt_result *out, double *trace, int trace_cap,
                      int *trace_rows, Launch &&launch) {
  int rc;
  CallFrame fr(ctx);
  if ((rc = fr.open())) return rc;
  hipStream_t st = fr.st;
  const size_t nscan = shared_scan ? 1 : (size_t)B, ntot = (size_t)offsets[nscan];
  if ((rc = ctx->d_off.ensure(ctx, nscan + 1))) return rc;
  if ((rc = ctx->d_init.ensure(ctx, (size_t)B * 3))) return rc;
  if ((rc = ctx->d_res.ensure(ctx, (size_t)B))) return rc;
  double *d_trace = nullptr; int *d_rows = nullptr;
  if (trace && trace_cap > 0 && trace_rows) {
    if ((rc = ctx->d_trace.ensure(ctx, (size_t)B * trace_cap * 8))) return rc;
    if ((rc = ctx->d_rows.ensure(ctx, (size_t)B))) return rc;
    d_trace = ctx->d_trace.p; d_rows = ctx->d_rows.p;
    HIP_TRY(ctx, hipMemsetAsync(d_trace, 0, (size_t)B * trace_cap * 64, st));
  }
  if (map_of && (rc = ctx->d_map_of.ensure(ctx, (size_t)B))) return rc;
  const float *d_scans = nullptr;
  if ((rc = stage_scan_f2(ctx, st, scans, nullptr, ntot, stride, &d_scans))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_off.p, offsets, (nscan + 1) * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_init.p, inits, (size_t)B * 24, hipMemcpyHostToDevice, st));
  if (map_of) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_map_of.p, map_of, (size_t)B * sizeof(int), hipMemcpyHostToDevice, st));
  unsigned long long *d_prof = nullptr;
#ifdef NDT_DIAG
  const bool want_prof = getenv("NDT_PROF") != nullptr;
  const size_t prof_bytes = (size_t)B * prof_scan_bytes();
  DevBuf<unsigned long long> prof_buf;
  if (want_prof && (rc = prof_buf.alloc(ctx, prof_bytes))) return rc;
  if (want_prof) { d_prof = prof_buf.p; HIP_TRY(ctx, hipMemsetAsync(d_prof, 0, prof_bytes, st)); }
#endif
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, st));
  if ((rc = launch(st, d_scans, map_of ? ctx->d_map_of.p : nullptr, d_trace, d_rows, d_prof))) return rc;
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, st));
#ifdef NDT_DIAG
  if (want_prof) {
    std::vector<unsigned long long> hp(prof_bytes / 8);
    HIP_TRY(ctx, hipStreamSynchronize(st));
    HIP_TRY(ctx, hipMemcpy(hp.data(), d_prof, prof_bytes, hipMemcpyDeviceToHost));
    prof_report(hp.data(), B);
  }
#endif
  HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_res.p, (size_t)B * sizeof(ndt_result), hipMemcpyDeviceToHost, st));
  if (d_trace) {
    HIP_TRY(ctx, hipMemcpyAsync(trace, d_trace, (size_t)B * trace_cap * 64, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(trace_rows, d_rows, (size_t)B * 4, hipMemcpyDeviceToHost, st));
  }
  return fr.close();
}

// Host-pointer matches against one map: the refusals, then the staged part.
int align_host_queue(ndt_ctx *ctx, const ndt_map *map, const float *scans, size_t stride, const uint64_t *offsets, int B,
                     int shared_scan, const double *inits, ndt_result *out, double *trace, int trace_cap, int *trace_rows) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!map || !scans || !offsets || !inits || !out || B <= 0 || stride < 8 || (stride & 3))
    return fail(ctx, NDT_E_ARG, "ndt_align_batch: bad arguments");
  if (map->ctx->device != ctx->device) return fail(ctx, NDT_E_ARG, "ndt_align_batch: the map was built on another device");
  const size_t nscan = shared_scan ? 1 : (size_t)B;
  const size_t npts = (size_t)(offsets[nscan] - offsets[0]);
  if (npts == 0) return fail(ctx, NDT_E_ARG, "ndt_align_batch: empty scans");
  for (size_t b = 0; b < nscan; ++b)
    if (offsets[b + 1] < offsets[b]) return fail(ctx, NDT_E_ARG, "ndt_align_batch: offsets not monotone");
  return align_host_staged(ctx, scans, stride, offsets, B, shared_scan, inits, nullptr, out, trace, trace_cap, trace_rows,
                           [&](hipStream_t st, const float *d_scans, const int *, double *d_trace, int *d_rows, unsigned long long *d_prof) {
                             return launch_align(ctx, map, st, d_scans, (const unsigned long long *)ctx->d_off.p, B,
                                                 shared_scan, (size_t)offsets[nscan], ctx->d_init.p, ctx->d_res.p, d_trace, trace_cap,
                                                 d_rows, d_prof);
                           });
}

// The end of a host form whose result has a length only the device knows, inside the form's frame: W words come back (w[1]:
// the count when W > 1, else w[0]) and are waited for, `check(w)` -- the form's own refusal, an NDT code -- looks at them, then
// that many elements of `elem` bytes are copied, the frame is closed and the stream waited for.
template <size_t W, typename Check>
int read_back_counted(CallFrame &fr, const uint64_t *d_words, const void *d_out, size_t elem, void *out_host, size_t *n_out, Check &&check) {
  ndt_ctx *ctx = fr.ctx;
  uint64_t w[W] = {};
  HIP_TRY(ctx, hipMemcpyAsync(w, d_words, sizeof(w), hipMemcpyDeviceToHost, fr.st));
  HIP_TRY(ctx, hipStreamSynchronize(fr.st));
  if (const int rc = check(w)) return rc;
  const size_t cnt = (size_t)w[W > 1];
  *n_out = cnt;
  if (cnt) HIP_TRY(ctx, hipMemcpyAsync(out_host, d_out, cnt * elem, hipMemcpyDeviceToHost, fr.st));
  return fr.close_and_wait();
}
int no_check(const uint64_t *) { return NDT_OK; }

int align_host_finish(ndt_ctx *ctx) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipEventElapsedTime(&ctx->align_ms, ctx->ev0, ctx->ev1));
  return NDT_OK;
}

int align_host(ndt_ctx *ctx, const ndt_map *map, const float *scans, size_t stride, const uint64_t *offsets, int B,
               int shared_scan, const double *inits, ndt_result *out, double *trace, int trace_cap, int *trace_rows) {
  const int rc = align_host_queue(ctx, map, scans, stride, offsets, B, shared_scan, inits, out, trace, trace_cap, trace_rows);
  return rc ? rc : align_host_finish(ctx);
}

// ---- multi-map launches (ndt_align_batch_multi_dev / ndt_align_batch_multi) ----

// The refusals of a multi-map call (synchronous, nothing queued); fills mm on success.  The launch's template instance and
// optimiser parameters are those of maps[0], so every field a match reads besides the grid must be the same in every map.
int check_multi(ndt_ctx *ctx, const ndt_map *const *maps, int n_maps, bool have_map_of, int B, const char *fn, MultiMaps *mm) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!maps || n_maps < 1) return fail(ctx, NDT_E_ARG, std::string(fn) + ": no maps (maps == NULL or n_maps < 1)");
  if (!have_map_of && n_maps != B) return fail(ctx, NDT_E_ARG, std::string(fn) + ": map_of == NULL needs n_maps == B");
  for (int i = 0; i < n_maps; ++i) {
    const ndt_map *m = maps[i];
    const std::string which = std::string(fn) + ": map " + std::to_string(i);
    if (!m) return fail(ctx, NDT_E_ARG, which + " is NULL");
    if (!m->ctx || !m->view.cent) return fail(ctx, NDT_E_ARG, which + " was never built");
    if (m->ctx->device != ctx->device) return fail(ctx, NDT_E_ARG, which + " was built on another device");
  }
  const ndt_map *m0 = maps[0];
  const OptParams o0 = opt_of(m0->prm);
  for (int i = 1; i < n_maps; ++i) {
    const ndt_map *m = maps[i];
    const OptParams o = opt_of(m->prm);
    const bool same = same_opt(o, o0) && m->prm.transform_sse == m0->prm.transform_sse && m->prm.radius_inclusive == m0->prm.radius_inclusive &&
                      same_bits(&m->prm.resolution, &m0->prm.resolution, sizeof(m0->prm.resolution)) &&
                      same_bits(&m->view.d1, &m0->view.d1, sizeof(double)) && same_bits(&m->view.d2, &m0->view.d2, sizeof(double)) &&
                      same_bits(&m->view.e_hi, &m0->view.e_hi, sizeof(double));
    if (!same)
      return fail(ctx, NDT_E_ARG, std::string(fn) + ": map " + std::to_string(i) +
                  " has other match parameters than map 0 (optimiser settings, transform_sse, radius_inclusive, resolution or the Gaussian constants)");
  }
  mm->maps = maps; mm->n_maps = n_maps;
  mm->distinct.assign(maps, maps + n_maps);
  std::sort(mm->distinct.begin(), mm->distinct.end());
  mm->distinct.erase(std::unique(mm->distinct.begin(), mm->distinct.end()), mm->distinct.end());
  return NDT_OK;
}

}  // namespace

extern "C" {

int ndt_align_batch_multi_dev(ndt_ctx *ctx, const ndt_map *const *maps, int n_maps, const int *map_of_dev,
                              const float *scans, const uint64_t *offsets, int B, size_t total_points, int shared_scan,
                              const double *inits, ndt_result *out, void *stream) {
  MultiMaps mm;
  int rc = check_multi(ctx, maps, n_maps, map_of_dev != nullptr, B, "ndt_align_batch_multi_dev", &mm);
  if (rc) return rc;
  if (!scans || !offsets || !inits || !out || B <= 0) return fail(ctx, NDT_E_ARG, "ndt_align_batch_multi_dev: bad arguments");
  if (total_points == 0) return fail(ctx, NDT_E_ARG, "ndt_align_batch_multi_dev: total_points = 0");
  mm.map_of = map_of_dev;
  const bool defer = ctx->defer_fitness != 0;
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {
    return launch_align(ctx, maps[0], st, scans, (const unsigned long long *)offsets, B, shared_scan, total_points, inits, out, nullptr, 0,
                        nullptr, nullptr, nullptr, defer, &mm);
  }, defer);
}

int ndt_align_batch_multi(ndt_ctx *ctx, const ndt_map *const *maps, int n_maps, const int *map_of_host,
                          const float *scans, const uint64_t *offsets, int B, int shared_scan, const double *inits,
                          ndt_result *out) {
  MultiMaps mm;
  int rc = check_multi(ctx, maps, n_maps, map_of_host != nullptr, B, "ndt_align_batch_multi", &mm);
  if (rc) return rc;
  if (!scans || !offsets || !inits || !out || B <= 0) return fail(ctx, NDT_E_ARG, "ndt_align_batch_multi: bad arguments");
  const size_t nscan = shared_scan ? 1 : (size_t)B;
  for (size_t b = 0; b < nscan; ++b)
    if (offsets[b + 1] < offsets[b]) return fail(ctx, NDT_E_ARG, "ndt_align_batch_multi: offsets not monotone");
  const size_t ntot = (size_t)offsets[nscan];
  if (offsets[nscan] == offsets[0]) return fail(ctx, NDT_E_ARG, "ndt_align_batch_multi: empty scans");
  rc = align_host_staged(ctx, scans, 8, offsets, B, shared_scan, inits, map_of_host, out, nullptr, 0, nullptr,
                         [&](hipStream_t st, const float *d_scans, const int *d_map_of, double *, int *, unsigned long long *d_prof) {
                           mm.map_of = d_map_of;
                           return launch_align(ctx, maps[0], st, d_scans, (const unsigned long long *)ctx->d_off.p, B, shared_scan, ntot,
                                               ctx->d_init.p, ctx->d_res.p, nullptr, 0, nullptr, d_prof, nullptr, false, &mm);
                         });
  return rc ? rc : align_host_finish(ctx);
}

int ndt_align_batch_trace(ndt_ctx *ctx, const ndt_map *map, const float *scans, const uint64_t *offsets,
                          int B, int shared_scan, const double *inits, ndt_result *out, double *trace,
                          int trace_cap, int *trace_rows) {
  return align_host(ctx, map, scans, 8, offsets, B, shared_scan, inits, out, trace, trace_cap, trace_rows);
}

int ndt_align_batch(ndt_ctx *ctx, const ndt_map *map, const float *scans, const uint64_t *offsets, int B,
                    int shared_scan, const double *inits, ndt_result *out) {
  return align_host(ctx, map, scans, 8, offsets, B, shared_scan, inits, out, nullptr, 0, nullptr);
}

int ndt_align_batch_sharded(ndt_ctx *const *ctxs, const ndt_map *const *maps, int n_shards, const float *scans,
                            const uint64_t *offsets, int B, int shared_scan, const double *inits, ndt_result *out) {
  if (!ctxs || !maps || n_shards <= 0 || !scans || !offsets || !inits || !out || B <= 0)
    return fail(nullptr, NDT_E_ARG, "ndt_align_batch_sharded: bad arguments");
  for (int r = 0; r < n_shards; ++r)
    if (!ctxs[r] || !maps[r]) return fail(nullptr, NDT_E_ARG, "ndt_align_batch_sharded: null context or map");
  // contiguous, balanced shards: the first B % n_shards get one match more (ndt_slam_amd/shard.py: shard_bounds)
  const int base = B / n_shards, extra = B % n_shards;
  std::vector<std::vector<uint64_t>> offs((size_t)n_shards);
  std::vector<int> queued((size_t)n_shards, 0), shard_rc((size_t)n_shards, NDT_OK);
  int rc_first = NDT_OK;
  for (int r = 0; r < n_shards; ++r) {            // queue every shard on its own device: uploads, launch, read-back
    const int lo = r * base + std::min(r, extra), n = base + (r < extra ? 1 : 0);
    if (n == 0) continue;
    int rc;
    if (shared_scan) {
      rc = align_host_queue(ctxs[r], maps[r], scans, 8, offsets, n, 1, inits + 3 * (size_t)lo, out + lo, nullptr, 0, nullptr);
    } else {
      offs[r] = rel_offsets(offsets + lo, (size_t)n);
      rc = align_host_queue(ctxs[r], maps[r], scans + 2 * (size_t)offsets[lo], 8, offs[r].data(), n, 0, inits + 3 * (size_t)lo,
                            out + lo, nullptr, 0, nullptr);
    }
    if (rc) { shard_rc[r] = rc; if (!rc_first) rc_first = rc; } else queued[r] = 1;
  }
  for (int r = 0; r < n_shards; ++r) {            // ... then wait for all of them
    if (!queued[r]) continue;
    const int rc = align_host_finish(ctxs[r]);
    if (rc) { shard_rc[r] = rc; if (!rc_first) rc_first = rc; }
  }
  // A failed shard must not leave its part of `results` as the caller handed it over: every record of it says so
  // (status = the shard's error, not converged, fitness DBL_MAX -- what a caller maps to the reference's 1e7 sentinel,
  // src/PoseEstimator.cpp:44-46); the other shards' records are complete and valid.  The call returns the first error.
  for (int r = 0; r < n_shards; ++r) {
    if (!shard_rc[r]) continue;
    const int lo = r * base + std::min(r, extra), n = base + (r < extra ? 1 : 0);
    for (int k = 0; k < n; ++k) {
      ndt_result z;
      memset(&z, 0, sizeof(z));
      z.status = shard_rc[r]; z.fitness = DBL_MAX;
      out[lo + k] = z;
    }
  }
  return rc_first;
}

namespace {
__global__ void __launch_bounds__(256)
selftest_libm_f32_kernel(const float *__restrict__ yaw, size_t n, float *__restrict__ c, float *__restrict__ s, float *__restrict__ y0) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float cc = sincosf_glibc(yaw[i], 1), ss = sincosf_glibc(yaw[i], 0);
    if (c) c[i] = cc;
    if (s) s[i] = ss;
    if (y0) y0[i] = eigen_init_yaw(cc, ss);
  }
}
}  // namespace

int ndt_selftest_libm_f32(ndt_ctx *ctx, const float *yaw, size_t n, float *cos_out, float *sin_out, float *init_yaw_out) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!yaw || n == 0) return fail(ctx, NDT_E_ARG, "ndt_selftest_libm_f32: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DevBuf<float> buf;
  { int rc = buf.alloc(ctx, 4 * n * sizeof(float)); if (rc) return rc; }
  float *d = buf.p;
  hipError_t e = hipMemcpyAsync(d, yaw, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    selftest_libm_f32_kernel<<<grid_for(n, 256), 256, 0, ctx->stream>>>(d, n, d + n, d + 2 * n, d + 3 * n);
    e = hipGetLastError();
  }
  if (e == hipSuccess && cos_out) e = hipMemcpyAsync(cos_out, d + n, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && sin_out) e = hipMemcpyAsync(sin_out, d + 2 * n, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && init_yaw_out) e = hipMemcpyAsync(init_yaw_out, d + 3 * n, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail(ctx, NDT_E_HIP, std::string("ndt_selftest_libm_f32: ") + hipGetErrorString(e));
  return NDT_OK;
}

namespace {
// One lane per row through the optimiser's own device functions (ndt_optimizer.hip.h); a part whose input is NULL is skipped.
__global__ void __launch_bounds__(256)
selftest_optimizer_kernel(const double *__restrict__ s3_in, size_t n_s3, double *__restrict__ s3_out,
                          const double *__restrict__ tr_in, size_t n_tr, double *__restrict__ tr_out,
                          const double *__restrict__ up_in, size_t n_up, double *__restrict__ up_out,
                          const float *__restrict__ yw_in, size_t n_yw, double *__restrict__ yw_out) {
  const size_t i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  if (s3_in) for (size_t i = i0; i < n_s3; i += step) {
    const double *r = s3_in + 9 * i;
    const double Hs[6] = {r[0], r[1], r[2], r[3], r[4], r[5]};
    double x0, x1, x2;
    solve3(Hs, r[6], r[7], r[8], x0, x1, x2);
    s3_out[3 * i] = x0; s3_out[3 * i + 1] = x1; s3_out[3 * i + 2] = x2;
  }
  if (tr_in) for (size_t i = i0; i < n_tr; i += step) {
    const double *r = tr_in + 9 * i;
    tr_out[i] = mt_trial(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8]);
  }
  if (up_in) for (size_t i = i0; i < n_up; i += step) {
    const double *r = up_in + 9 * i;
    AlignState S;
    S.a_l = r[0]; S.f_l = r[1]; S.g_l = r[2]; S.a_u = r[3]; S.f_u = r[4]; S.g_u = r[5];
    const int rc = mt_update(S, r[6], r[7], r[8]);
    double *o = up_out + 7 * i;
    o[0] = S.a_l; o[1] = S.f_l; o[2] = S.g_l; o[3] = S.a_u; o[4] = S.f_u; o[5] = S.g_u; o[6] = (double)rc;
  }
  if (yw_in) for (size_t i = i0; i < n_yw; i += step) yw_out[i] = yaw_from_T(yw_in[2 * i], yw_in[2 * i + 1]);
}
}  // namespace

int ndt_selftest_optimizer(ndt_ctx *ctx, const double *solve3_in, size_t n_solve3, double *solve3_out,
                           const double *mt_trial_in, size_t n_mt_trial, double *mt_trial_out,
                           const double *mt_update_in, size_t n_mt_update, double *mt_update_out,
                           const float *yaw_in, size_t n_yaw, double *yaw_out) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!solve3_in) n_solve3 = 0;
  if (!mt_trial_in) n_mt_trial = 0;
  if (!mt_update_in) n_mt_update = 0;
  if (!yaw_in) n_yaw = 0;
  const size_t n_max = std::max(std::max(n_solve3, n_mt_trial), std::max(n_mt_update, n_yaw));
  if (n_max == 0 || n_max > ((size_t)1 << 26) || (n_solve3 && !solve3_out) || (n_mt_trial && !mt_trial_out) ||
      (n_mt_update && !mt_update_out) || (n_yaw && !yaw_out))
    return fail(ctx, NDT_E_ARG, "ndt_selftest_optimizer: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // one buffer of doubles: [solve3 in 9 | out 3] [mt_trial in 9 | out 1] [mt_update in 9 | out 7] [yaw out 1 | in 2 floats = 1 double]
  const size_t o_s3 = 0, o_tr = o_s3 + 12 * n_solve3, o_up = o_tr + 10 * n_mt_trial, o_yw = o_up + 16 * n_mt_update,
               total = o_yw + 2 * n_yaw;
  DevBuf<double> buf;
  { int rc = buf.alloc(ctx, total * sizeof(double)); if (rc) return rc; }
  double *d = buf.p;
  double *d_s3 = d + o_s3, *d_tr = d + o_tr, *d_up = d + o_up, *d_yw = d + o_yw;
  hipStream_t st = ctx->stream;
  hipError_t e = hipSuccess;
  if (e == hipSuccess && n_solve3) e = hipMemcpyAsync(d_s3, solve3_in, 9 * n_solve3 * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && n_mt_trial) e = hipMemcpyAsync(d_tr, mt_trial_in, 9 * n_mt_trial * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && n_mt_update) e = hipMemcpyAsync(d_up, mt_update_in, 9 * n_mt_update * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && n_yaw) e = hipMemcpyAsync(d_yw + n_yaw, yaw_in, 2 * n_yaw * sizeof(float), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    selftest_optimizer_kernel<<<grid_for(n_max, 256), 256, 0, st>>>(
        n_solve3 ? d_s3 : nullptr, n_solve3, d_s3 + 9 * n_solve3, n_mt_trial ? d_tr : nullptr, n_mt_trial, d_tr + 9 * n_mt_trial,
        n_mt_update ? d_up : nullptr, n_mt_update, d_up + 9 * n_mt_update,
        n_yaw ? (const float *)(d_yw + n_yaw) : nullptr, n_yaw, d_yw);
    e = hipGetLastError();
  }
  if (e == hipSuccess && n_solve3) e = hipMemcpyAsync(solve3_out, d_s3 + 9 * n_solve3, 3 * n_solve3 * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && n_mt_trial) e = hipMemcpyAsync(mt_trial_out, d_tr + 9 * n_mt_trial, n_mt_trial * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && n_mt_update) e = hipMemcpyAsync(mt_update_out, d_up + 9 * n_mt_update, 7 * n_mt_update * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && n_yaw) e = hipMemcpyAsync(yaw_out, d_yw, n_yaw * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(ctx, NDT_E_HIP, std::string("ndt_selftest_optimizer: ") + hipGetErrorString(e));
  return NDT_OK;
}

int ndt_align(ndt_ctx *ctx, const ndt_map *map, const float *scan, size_t n, size_t stride,
              const double init[3], ndt_result *out) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!map || !scan || n == 0 || !init || !out || stride < 8 || (stride & 3)) return fail(ctx, NDT_E_ARG, "ndt_align: bad arguments");
  const uint64_t off[2] = {0, (uint64_t)n};
  return align_host(ctx, map, scan, stride, off, 1, 0, init, out, nullptr, 0, nullptr);
}

}  // extern "C"

namespace {
// ndt_eval_at / ndt_fitness_at on the context's stream, synchronous: the scan goes up, st waits for the map's build
// (MapRead::begin; no ring entry), `launch(st, d_scan, d_part, blocks)` queues the kernel, `words` doubles per block come back.
template <typename Launch>
int probe_map(ndt_ctx *ctx, const ndt_map *map, const float *scan, size_t n, size_t stride, int words, std::vector<double> *hp, Launch &&launch) {
  int rc;
  CallFrame fr(ctx);
  if ((rc = fr.open())) return rc;
  hipStream_t st = fr.st;
  if ((rc = MapRead{ctx, st, &map, 1}.begin())) return rc;
  const int grid = grid_for(n, 256, 1024);
  hp->resize((size_t)grid * words);
  if ((rc = ctx->d_scan.ensure(ctx, n * stride))) return rc;
  if ((rc = ctx->d_tmp.ensure(ctx, hp->size() * 8))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_scan.p, scan, n * stride, hipMemcpyHostToDevice, st));
  launch(st, (const float *)ctx->d_scan.p, (double *)ctx->d_tmp.p, grid);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(hp->data(), ctx->d_tmp.p, hp->size() * 8, hipMemcpyDeviceToHost, st));
  return fr.close_and_wait();
}
}  // namespace

extern "C" {

int ndt_eval_at(ndt_ctx *ctx, const ndt_map *map, const float *scan, size_t n, size_t stride,
                const double p[3], double *score, double g[3], double H[9], double *pairs) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!map || !scan || n == 0 || !p || stride < 8 || (stride & 7)) return fail(ctx, NDT_E_ARG, "ndt_eval_at: bad arguments");
  std::vector<double> hp;
  const int rc = probe_map(ctx, map, scan, n, stride, kAcc, &hp, [&](hipStream_t st, const float *ds, double *dt, int grid) {
    with_bool(map->prm.transform_sse != 0, [&](auto Sse) { with_bool(map->prm.radius_inclusive != 0, [&](auto Incl) {
      ndt_eval_kernel<decltype(Sse)::value, decltype(Incl)::value><<<grid, 256, 0, st>>>(map->view, map->prm.snap_thresh, map->prm.libm_f32, ds, stride,
                                                                                         (int)n, p[0], p[1], p[2], dt);
    }); });
  });
  if (rc) return rc;
  double t[kAcc] = {0};
  for (size_t b = 0; b < hp.size() / kAcc; ++b) for (int k = 0; k < kAcc; ++k) t[k] += hp[b * kAcc + k];
  const double w = map->view.d1 * map->view.d2;
  if (score) *score = -map->view.d1 * t[0];
  if (g) { g[0] = w * t[1]; g[1] = w * t[2]; g[2] = w * t[3]; }
  if (H) {
    H[0] = w * t[4]; H[1] = H[3] = w * t[5]; H[2] = H[6] = w * t[6];
    H[4] = w * t[7]; H[5] = H[7] = w * t[8]; H[8] = w * t[9];
  }
  if (pairs) *pairs = t[10];
  return NDT_OK;
}

int ndt_fitness_at(ndt_ctx *ctx, const ndt_map *map, const float *scan, size_t n, size_t stride,
                   float c, float s, float tx, float ty, double *fitness) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!map || !scan || n == 0 || !fitness || stride < 8 || (stride & 7)) return fail(ctx, NDT_E_ARG, "ndt_fitness_at: bad arguments");
  std::vector<double> hp;
  const int rc = probe_map(ctx, map, scan, n, stride, 2, &hp, [&](hipStream_t st, const float *ds, double *dt, int grid) {
    ndt_fitness_kernel<<<grid, 256, 0, st>>>(map->view, ds, stride, (int)n, Tf32{c, s, tx, ty}, dt);
  });
  if (rc) return rc;
  double sum = 0, cnt = 0;
  for (size_t b = 0; b < hp.size() / 2; ++b) { sum += hp[2 * b]; cnt += hp[2 * b + 1]; }
  *fitness = cnt > 0 ? sum / cnt : DBL_MAX;
  return NDT_OK;
}

}  // extern "C"

namespace {
// The kernels of the pre-filter over B scans, inside the caller's frame (d_pf).  kTarget
// (ndt_local_map_batch_dev): scan b's filtered points go behind prev[b] (device table, points at prev_stride), which
// is copied in front of them, and out_offsets is the scan of prev[b].n + count b (of 0 where status[b] != NDT_OK);
// total_prev_points: the sum of prev[b].n.
template <bool kTarget>
int pf_run(ndt_ctx *ctx, const float *raw_xy, size_t stride, const uint64_t *raw_offsets, int B, size_t total_raw_points,
           float leaf, float *out_xy, uint64_t *out_offsets, const PfPrev *prev, size_t prev_stride,
           size_t total_prev_points, const int *status, hipStream_t st) {
  int rc;
  // filtered points at the raw offsets (dense; the step-by-step kernel's flushes at the index of their cause), the per-scan counts
  Regions R;
  const size_t o_tmp = R.take(total_raw_points * sizeof(float2)), o_sparse = R.take(total_raw_points * sizeof(float2)),
               o_counts = R.take((size_t)B * sizeof(unsigned));
  if ((rc = ctx->d_pf.ensure(ctx, R.end))) return rc;
  float2 *tmp = R.at<float2>(ctx->d_pf.p, o_tmp), *sparse = R.at<float2>(ctx->d_pf.p, o_sparse);
  unsigned *counts = R.at<unsigned>(ctx->d_pf.p, o_counts);
  const int grid = B < 8 * ctx->num_cus ? B : 8 * ctx->num_cus;
  // scans of up to kPfSortMax points: ordered by slot, one thread per slot; longer ones: the step-by-step replay
  prefilter_sorted_kernel<<<grid, kPfSortThreads, 0, st>>>(raw_xy, stride, (const unsigned long long *)raw_offsets, B, leaf,
                                                           tmp, counts);
  prefilter_mw_kernel<<<grid, 64 * kPfWaves, 0, st>>>(raw_xy, stride, (const unsigned long long *)raw_offsets, B, leaf,
                                                      sparse, tmp, counts, kPfSortMax);
  prefilter_offsets_kernel<kTarget><<<1, 1024, 0, st>>>(counts, B, (unsigned long long *)out_offsets, prev, status);
  const int gx = (int)std::min<size_t>(64, ((total_raw_points + total_prev_points) / (size_t)B + 255) / 256 + 1);
  prefilter_pack_kernel<kTarget><<<dim3((unsigned)gx, (unsigned)std::min(B, 65535)), 256, 0, st>>>(
      tmp, (const unsigned long long *)raw_offsets, (const unsigned long long *)out_offsets, B, (float2 *)out_xy, prev,
      prev_stride, status);
  HIP_TRY(ctx, hipGetLastError());
  return NDT_OK;
}
}  // namespace

extern "C" {

int ndt_prefilter_batch_dev(ndt_ctx *ctx, const float *raw_xy, size_t stride, const uint64_t *raw_offsets, int B,
                            size_t total_raw_points, float leaf, float *out_xy, uint64_t *out_offsets, void *stream) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!raw_xy || !raw_offsets || !out_xy || !out_offsets || B <= 0 || total_raw_points == 0 || !(leaf > 0) ||
      stride < 8 || (stride & 7))
    return fail(ctx, NDT_E_ARG, "ndt_prefilter_batch: bad arguments");
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {
    return pf_run<false>(ctx, raw_xy, stride, raw_offsets, B, total_raw_points, leaf, out_xy, out_offsets, nullptr, 0, 0, nullptr, st);
  });
}

// B scans in host memory (raw_offsets[B + 1] in points of raw_xy_host): one upload, the filter, the offsets read back, one
// copy of the result.  out_xy_host needs room for every input point.  Empty scans stay empty.
int ndt_prefilter_batch(ndt_ctx *ctx, const float *raw_xy_host, size_t stride, const uint64_t *raw_offsets, int B,
                        float leaf, float *out_xy_host, uint64_t *out_offsets_host) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (B < 1) return fail(ctx, NDT_E_ARG, "ndt_prefilter_batch: B < 1");
  if (!raw_offsets || !out_offsets_host) return fail(ctx, NDT_E_ARG, "ndt_prefilter_batch: NULL array (raw_offsets or out_offsets)");
  if (stride < 8 || (stride & 7)) return fail(ctx, NDT_E_ARG, "ndt_prefilter_batch: bad stride (need stride_bytes >= 8 and % 8 == 0)");
  if (!(leaf > 0)) return fail(ctx, NDT_E_ARG, "ndt_prefilter_batch: leaf <= 0");
  for (int b = 0; b < B; ++b)
    if (raw_offsets[b + 1] < raw_offsets[b])
      return fail(ctx, NDT_E_ARG, "ndt_prefilter_batch: scan " + std::to_string(b) + ": offsets decrease");
  const size_t n = (size_t)(raw_offsets[B] - raw_offsets[0]), B1 = (size_t)B + 1;
  if (n && (!raw_xy_host || !out_xy_host)) return fail(ctx, NDT_E_ARG, "ndt_prefilter_batch: NULL array (raw_xy or out_xy)");
  if (n == 0) { for (int b = 0; b <= B; ++b) out_offsets_host[b] = 0; return NDT_OK; }
  int rc;
  CallFrame fr(ctx);
  if ((rc = fr.open())) return rc;
  hipStream_t st = fr.st;
  Regions R;
  const size_t o_in = R.take(n * stride), o_out = R.take(n * sizeof(float2));
  if ((rc = ctx->d_scan.ensure(ctx, R.end))) return rc;
  if ((rc = ctx->d_off.ensure(ctx, 2 * B1))) return rc;
  float *d_in = R.at<float>(ctx->d_scan.p, o_in), *d_out = R.at<float>(ctx->d_scan.p, o_out);
  uint64_t *d_offs = ctx->d_off.p;                              // [0 .. B] raw, [B + 1 .. 2 B + 1] filtered
  const std::vector<uint64_t> rel = rel_offsets(raw_offsets, (size_t)B);
  HIP_TRY(ctx, hipMemcpyAsync(d_in, (const char *)raw_xy_host + (size_t)raw_offsets[0] * stride, n * stride, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d_offs, rel.data(), rel.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  if ((rc = pf_run<false>(ctx, d_in, stride, d_offs, B, n, leaf, d_out, d_offs + B1, nullptr, 0, 0, nullptr, st))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(out_offsets_host, d_offs + B1, B1 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  const size_t m = (size_t)out_offsets_host[B];
  if (m) HIP_TRY(ctx, hipMemcpyAsync(out_xy_host, d_out, m * sizeof(float2), hipMemcpyDeviceToHost, st));
  return fr.close_and_wait();
}

int ndt_prefilter(ndt_ctx *ctx, const float *xy_host, size_t n, size_t stride, float leaf, float *out_xy_host,
                  size_t *n_out) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!xy_host || n == 0 || !out_xy_host || !n_out || stride < 8 || (stride & 7) || !(leaf > 0))
    return fail(ctx, NDT_E_ARG, "ndt_prefilter: bad arguments");
  const uint64_t raw[2] = {0, (uint64_t)n};                     // one scan of the batch form
  uint64_t filtered[2] = {0, 0};
  const int rc = ndt_prefilter_batch(ctx, xy_host, stride, raw, 1, leaf, out_xy_host, filtered);
  if (rc == NDT_OK) *n_out = (size_t)filtered[1];
  return rc;
}

namespace {
// k_max of ndt_resample_capacity: the most points one input point can emit; 0 = refused parameters
size_t resample_k_max(double space, double space_thre) {
  if (!std::isfinite(space) || !std::isfinite(space_thre) || space < 0 || space_thre < 0) return 0;
  if (space == 0 && space_thre > 0) return 0;        // the reference interpolates at distance 0 forever there
  if (space_thre <= space) return 1;                 // dis + L >= space implies >= space_thre: kept, never interpolated
  const double k = std::floor(space_thre / space) + 2;
  return k < 9.0e18 ? (size_t)k : 0;
}
}  // namespace

int ndt_resample_capacity(size_t total_points, double space, double space_thre, size_t *capacity) {
  const size_t k = resample_k_max(space, space_thre);
  if (!capacity || k == 0) return fail(nullptr, NDT_E_ARG, "ndt_resample_capacity: bad arguments");
  if (total_points && k > SIZE_MAX / total_points) return fail(nullptr, NDT_E_ARG, "ndt_resample_capacity: overflow");
  *capacity = total_points * k;
  return NDT_OK;
}

namespace {
// What the resampler refuses of either form (the host form names its own refusals first); *cap: ndt_resample_capacity.
int resample_check(ndt_ctx *ctx, const double *raw_xy, size_t stride, const uint64_t *raw_offsets, int B, size_t total_raw_points,
                   double space, double space_thre, const void *out_xy64, const void *out_xy32, const uint64_t *out_offsets, size_t *cap) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!raw_xy || !raw_offsets || (!out_xy64 && !out_xy32) || !out_offsets || B <= 0 || total_raw_points == 0 ||
      stride < 16 || (stride & 7) || ndt_resample_capacity(total_raw_points, space, space_thre, cap))
    return fail(ctx, NDT_E_ARG, "ndt_resample_batch: bad arguments");
  if (*cap > SIZE_MAX / sizeof(double2) / 2) return fail(ctx, NDT_E_NOMEM, "ndt_resample_batch: scratch too large");
  return NDT_OK;
}

// The resampler's kernels over B scans on st, inside the caller's frame (d_rs).
int queue_resample(ndt_ctx *ctx, hipStream_t st, const double *raw_xy, size_t stride, const uint64_t *raw_offsets, int B, size_t N,
                   double space, double space_thre, size_t cap, double *out_xy64, float *out_xy32, uint64_t *out_offsets, int *status) {
  const size_t k_max = cap / N;
  int rc;
  // scratch: walk outputs (k_max slots per raw point) | L | cnt | pos | tot | dist | bad
  Regions R;
  const size_t o_scr = R.take(cap * sizeof(double2)), o_l = R.take(N * sizeof(double)), o_cnt = R.take(N * sizeof(unsigned long long)),
               o_pos = R.take(N * sizeof(unsigned long long)), o_tot = R.take((size_t)B * sizeof(unsigned long long)),
               o_dist = R.take(N * sizeof(unsigned)), o_bad = R.take((size_t)B * sizeof(int));
  if ((rc = ctx->d_rs.ensure(ctx, R.end))) return rc;
  unsigned char *d = ctx->d_rs.p;
  double2 *scr = R.at<double2>(d, o_scr);
  double *L = R.at<double>(d, o_l);
  unsigned long long *cnt = R.at<unsigned long long>(d, o_cnt), *pos = R.at<unsigned long long>(d, o_pos), *tot = R.at<unsigned long long>(d, o_tot);
  unsigned *dist = R.at<unsigned>(d, o_dist);
  int *bad = R.at<int>(d, o_bad);
  const unsigned long long *offs = (const unsigned long long *)raw_offsets;
  const double resync = std::max(space, space_thre);
  const unsigned gx = (unsigned)std::min<size_t>(64, (N / (size_t)B + 255) / 256 + 1), gy = (unsigned)std::min(B, 65535);
  HIP_TRY(ctx, hipMemsetAsync(bad, 0, (size_t)B * sizeof(int), st));
  resample_prepass_kernel<<<dim3(gx, gy), 256, 0, st>>>(raw_xy, stride, offs, B, N, L, bad);
  resample_walk_kernel<<<(unsigned)((N + 255) / 256), 256, 0, st>>>(raw_xy, stride, offs, B, N, L, space, space_thre, resync,
                                                                     k_max, bad, scr, cnt, dist);
  resample_segscan_kernel<<<std::min(B, 8 * ctx->num_cus), kRsScanThreads, 0, st>>>(offs, B, N, L, resync, bad, cnt, pos, tot);
  resample_offsets_kernel<<<1, kRsScanThreads, 0, st>>>(tot, bad, B, (unsigned long long *)out_offsets, status);
  resample_pack_kernel<<<dim3(gx, gy), 256, 0, st>>>(offs, B, N, bad, scr, k_max, cnt, pos, dist,
                                                      (const unsigned long long *)out_offsets, (double2 *)out_xy64,
                                                      (float2 *)out_xy32);
  HIP_TRY(ctx, hipGetLastError());
  return NDT_OK;
}
}  // namespace

int ndt_resample_batch_dev(ndt_ctx *ctx, const double *raw_xy, size_t stride, const uint64_t *raw_offsets, int B,
                           size_t total_raw_points, double space, double space_thre, double *out_xy64, float *out_xy32,
                           uint64_t *out_offsets, int *status, void *stream) {
  size_t cap = 0;
  int rc = resample_check(ctx, raw_xy, stride, raw_offsets, B, total_raw_points, space, space_thre, out_xy64, out_xy32, out_offsets, &cap);
  if (rc) return rc;
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {
    return queue_resample(ctx, st, raw_xy, stride, raw_offsets, B, total_raw_points, space, space_thre, cap, out_xy64, out_xy32,
                           out_offsets, status);
  });
}

int ndt_resample(ndt_ctx *ctx, const double *xy_host, size_t n, size_t stride, double space, double space_thre,
                 double *out_xy_host, size_t *n_out) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  size_t cap = 0;
  if ((n && (!xy_host || !out_xy_host)) || !n_out || stride < 16 || (stride & 7) ||
      ndt_resample_capacity(n, space, space_thre, &cap))
    return fail(ctx, NDT_E_ARG, "ndt_resample: bad arguments");
  if (n == 0) { *n_out = 0; return NDT_OK; }           // an empty scan stays empty (src/ScanPointResampler.cpp:7-8)
  const uint64_t raw[2] = {0, (uint64_t)n};
  int rc = resample_check(ctx, xy_host, stride, raw, 1, n, space, space_thre, out_xy_host, nullptr, raw, &cap);
  if (rc) return rc;
  CallFrame fr(ctx);
  if ((rc = fr.open())) return rc;
  hipStream_t st = fr.st;
  Regions R;
  const size_t o_in = R.take(n * stride), o_out = R.take(cap * sizeof(double2));
  if ((rc = ctx->d_scan.ensure(ctx, R.end))) return rc;
  if ((rc = ctx->d_off.ensure(ctx, 5))) return rc;
  double *d_in = R.at<double>(ctx->d_scan.p, o_in), *d_out = R.at<double>(ctx->d_scan.p, o_out);
  uint64_t *d_offs = ctx->d_off.p;                              // [0..1] raw, [2..3] resampled, [4] status
  HIP_TRY(ctx, hipMemcpyAsync(d_in, xy_host, n * stride, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d_offs, raw, sizeof(raw), hipMemcpyHostToDevice, st));
  if ((rc = queue_resample(ctx, st, d_in, stride, d_offs, 1, n, space, space_thre, cap, d_out, nullptr, d_offs + 2, (int *)(d_offs + 4))))
    return rc;
  return read_back_counted<3>(fr, d_offs + 2, d_out, sizeof(double2), out_xy_host, n_out, [&](const uint64_t *fo) {
    int scan_status = 0;
    memcpy(&scan_status, &fo[2], sizeof(int));
    return scan_status != NDT_OK ? fail(ctx, NDT_E_ARG, "ndt_resample: the scan holds a non-finite coordinate") : NDT_OK;
  });
}

int ndt_scan_to_map_batch_dev(ndt_ctx *ctx, const double *xy, size_t stride, const uint64_t *offsets, int B,
                              size_t total_points, const double *poses, float *out_xy, void *stream) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!xy || !offsets || !poses || !out_xy || B <= 0 || total_points == 0 || stride < 16 || (stride & 7))
    return fail(ctx, NDT_E_ARG, "ndt_scan_to_map_batch: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  const unsigned gx = (unsigned)std::min<size_t>(64, (total_points / (size_t)B + 255) / 256 + 1), gy = (unsigned)std::min(B, 65535);
  scan_to_map_kernel<<<dim3(gx, gy), 256, 0, st>>>(xy, stride, (const unsigned long long *)offsets, B, total_points, poses,
                                                    (float2 *)out_xy);
  HIP_TRY(ctx, hipGetLastError());
  return NDT_OK;
}

int ndt_fuse_default_params(ndt_fuse_params *p) {
  if (!p) return NDT_E_ARG;
  p->coe_ndt_cov = 1.0; p->coe_vel = 0.1; p->coe_omega = 0.1; p->del_time = 0.5; p->score_thre = 0.0;
  return NDT_OK;
}

int ndt_predict_batch_dev(ndt_ctx *ctx, const double *odo_cur, const double *odo_prev, const double *last_pose, int B,
                          double *odo_motion, double *pred_pose, double *init_xyyaw, void *stream) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!odo_cur || !odo_prev || !last_pose || !odo_motion || !pred_pose || B <= 0)
    return fail(ctx, NDT_E_ARG, "ndt_predict_batch: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  predict_kernel<<<(B + 255) / 256, 256, 0, st>>>(odo_cur, odo_prev, last_pose, B, odo_motion, pred_pose, init_xyyaw);
  HIP_TRY(ctx, hipGetLastError());
  return NDT_OK;
}

int ndt_fuse_batch_dev(ndt_ctx *ctx, const ndt_result *results, const double *pred_pose, const double *odo_motion,
                       const double *last_pose, const double *last_cov, int B, const ndt_fuse_params *prm,
                       double *fused_pose, double *cov, int *successful, void *stream) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!results || !pred_pose || !odo_motion || !last_pose || !last_cov || !prm || !fused_pose || !cov || B <= 0 ||
      !(prm->del_time > 0))
    return fail(ctx, NDT_E_ARG, "ndt_fuse_batch: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  FuseParams P = {prm->coe_ndt_cov, prm->coe_vel, prm->coe_omega, prm->del_time, prm->score_thre};
  fuse_kernel<<<(B + 255) / 256, 256, 0, st>>>(results, pred_pose, odo_motion, last_pose, last_cov, B, P, fused_pose,
                                               cov, successful);
  HIP_TRY(ctx, hipGetLastError());
  return NDT_OK;
}

}  // extern "C"

namespace {

// Local-map assembly, one chain for every caller (ndt_localmap.hip.h): the job table (one entry per scan triple), the unit
// table (256-point stretches of the result) and the submap table are written into pinned memory and uploaded with one copy.
// Device scratch (ctx->d_mm): [jobs][units][submaps][previous clouds][one count word], then the chain's own (MmScratch).
// A call describes 0 submaps (ndt_difference_extraction_dev: one job, no units), 1 (ndt_make_map_dev, ndt_remove_neighbors_dev)
// or many (ndt_local_map_batch_dev, which alone fills the previous clouds); the sessions' step queues the same chain over
// tables of its own (SsStep::behind).
size_t pow2_at_least(size_t v) { size_t c = 64; while (c < v) c <<= 1; return c; }

// The rules every entry point of the assembly holds its arguments to (each with its own message):
// MmUnit::stride and MmJob::sa / sb / ls are 32-bit
bool mm_stride_ok(size_t stride) { return stride >= 8 && !(stride & 7) && stride <= (size_t)UINT32_MAX; }
bool mm_scan_count_ok(int n_scans) { return n_scans >= 1 && n_scans <= (1 << 20); }
bool mm_offsets_ok(const uint64_t *offsets, int n_scans) {      // non-decreasing, scans below 2^29 points
  for (int i = 0; i < n_scans; ++i)
    if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > (uint64_t)(1u << 29)) return false;
  return true;
}

// The jobs of a call (of a step of a session set), still unbound (mm_bind).
struct MmPlan {
  std::vector<MmJob> jobs;
  size_t sa = 8, sb = 8;     // set before the first add()
  size_t unit_room = 0;
  size_t n_subs = 0;         // submaps (the tables of MmSub and PfPrev follow the units)
  size_t tab_words = 0, list_pts = 0;      // over the jobs: the voxel sets' words, the difference lists' points
  // One triple: base cloud a0 ++ a1, test cloud b.  The one place that sizes a voxel set.
  void add(const float *a0, const float *a1, const float *b, size_t n0, size_t n1, size_t nb, double res, float cut) {
    const size_t cap = pow2_at_least(2 * (n0 + n1) + 2);
    MmJob J{};
    J.a0 = a0; J.a1 = a1; J.b = b; J.n0 = (unsigned)n0; J.n1 = (unsigned)n1; J.nb = (unsigned)nb;
    J.sa = (unsigned)sa; J.sb = (unsigned)sb; J.tab_mask = (unsigned)(cap - 1); J.res = res; J.cut = cut; J.ls = sizeof(float2);
    jobs.push_back(J);
    tab_words += cap; list_pts += nb;
  }
  // A job that is a list for the flag kernel and nothing else: no clouds, no voxel set (a plan of such jobs has
  // tab_words == 0, and neither the fill nor make_map_diff_kernel is queued); its list and count are the caller's (mm_bind)
  void add_list(size_t stride, float cut) {
    MmJob J{};
    J.cut = cut; J.ls = (unsigned)stride;
    jobs.push_back(J);
  }
};

// The chain's device-only scratch for P's jobs and P.unit_room units, as offsets into the block the caller lays out (behind the
// uploaded tables in ctx->d_mm, behind the units in a session set's mm)
struct MmScratch {
  size_t ucnt = 0, uoff = 0, keep = 0, cnt = 0, tab = 0, diff = 0, coff = 0, stat = 0, nj = 0, nu = 0, tab_words = 0;
  MmScratch() = default;
  MmScratch(Regions &R, const MmPlan &P) : nj(P.jobs.size()), nu(P.unit_room), tab_words(P.tab_words) {
    ucnt = R.take(nu * 4); uoff = R.take(nu * 8); keep = R.take(nu * (kMmUnit / 64) * 8);      // per unit
    cnt = R.take(nj * 8 + 8); tab = R.take(tab_words * 8); diff = R.take(P.list_pts * 8 + 64);      // difference counts, voxel sets, lists
    coff = R.take(2 * 8); stat = R.take(4);      // cloud_off[2] and the status of a call whose one submap reports through n_out alone
  }
};
struct MmLayout {
  size_t o_units = 0, o_subs = 0, o_prev = 0, o_word = 0, o_up = 0;      // o_up: where the uploaded tables end
  MmScratch x;
  size_t ns = 0;
  MmJob *jobs = nullptr; MmUnit *units = nullptr;      // pinned, valid until the next call on this context
  MmSub *subs = nullptr; PfPrev *prevs = nullptr;      // pinned; prevs: zero unless the caller fills them
  unsigned long long *word = nullptr;                  // pinned: the count of a caller's list (add_list), zero otherwise
};

// Jobs [0, nj) get their voxel sets, difference lists and counters in scratch X of the block at d, one behind the other.
// diff_override / n_diff_override: every list / counter is the caller's instead (one job).
void mm_bind(MmJob *jobs, size_t nj, char *d, const MmScratch &X, float2 *diff_override = nullptr, unsigned long long *n_diff_override = nullptr) {
  size_t tw = 0, lp = 0;
  for (size_t j = 0; j < nj; ++j) {
    MmJob &J = jobs[j];
    J.tab = (unsigned long long *)(d + X.tab) + tw;
    J.diff = diff_override ? diff_override : (float2 *)(d + X.diff) + lp;
    J.n_diff = n_diff_override ? n_diff_override : (unsigned long long *)(d + X.cnt) + j;
    tw += (size_t)J.tab_mask + 1; lp += J.nb;
  }
}

// One submap's scan triples (added to P) and the pieces of its cloud (appended to `pieces`) in the order
// Submap::makeMap appends them -- the rule of the assembly of a whole submap; the sessions' step
// holds the same branches in their incremental form (SsStep::book, ndt_sessions.hip.h).  cut: rn_cutoff(D.thre_neighbor).
// Returns the units (stretches of kMmUnit points) the pieces take.
struct MmPiece { const float *p; size_t n; int job; };      // job: the piece's triple in P.jobs, or -1
size_t submap_pieces(const ndt_submap_desc &D, size_t stride, float cut, MmPlan *P, std::vector<MmPiece> *pieces) {
  auto scan_ptr = [&](int i) { return (const float *)((const char *)D.scans_xy + (size_t)D.offsets[i] * stride); };
  auto scan_n = [&](int i) { return (size_t)(D.offsets[i + 1] - D.offsets[i]); };
  size_t nu = 0;
  auto piece = [&](int i, int job) { pieces->push_back({scan_ptr(i), scan_n(i), job}); nu += (scan_n(i) + kMmUnit - 1) / kMmUnit; };
  if (D.remove_moving) {
    if (D.first_submap) piece(0, -1);
    for (int i = 0; i + 2 < D.n_scans; ++i)
      if (scan_n(i + 1)) {      // an empty middle scan contributes nothing
        piece(i + 1, (int)P->jobs.size());
        P->add(scan_ptr(i), scan_ptr(i + 2), scan_ptr(i + 1), scan_n(i), scan_n(i + 2), scan_n(i + 1), D.resol, cut);
      }
    if (D.newest) piece(D.n_scans - 1, -1);
  } else {
    for (int i = D.first_submap ? 0 : 2; i < D.n_scans; ++i) piece(i, -1);
  }
  return nu;
}

size_t submap_points(const ndt_submap_desc &D) {        // points the submap's cloud may hold (the header's capacity rule)
  const size_t total = (size_t)(D.offsets[D.n_scans] - D.offsets[0]);
  return D.n_scans == 1 ? 2 * total : total;            // a lone scan is appended twice (first + newest)
}

// The units of pieces [first, last), which belong to submap `sub`, written from `units` on; returns the end.
MmUnit *fill_units(MmUnit *units, const MmPiece *first, const MmPiece *last, size_t stride, unsigned sub) {
  for (const MmPiece *pc = first; pc != last; ++pc)
    for (size_t o = 0; o < pc->n; o += kMmUnit)
      *units++ = MmUnit{(const float *)((const char *)pc->p + o * stride), (unsigned)stride,
                        (unsigned)std::min<size_t>(kMmUnit, pc->n - o), pc->job, sub};
  return units;
}

// Lays out ctx->d_mm and the pinned tables, and writes the jobs, bound.  Queues nothing.
int mm_prepare(ndt_ctx *ctx, const MmPlan &P, float2 *diff_override, unsigned long long *n_diff_override, MmLayout *Lo) {
  const size_t nj = P.jobs.size(), nu = P.unit_room, ns = P.n_subs;
  MmLayout L;
  Regions R;
  R.take(nj * sizeof(MmJob));
  L.o_units = R.take(nu * sizeof(MmUnit)); L.o_subs = R.take(ns * sizeof(MmSub)); L.o_prev = R.take(ns * sizeof(PfPrev));
  L.o_word = R.take(8);
  L.o_up = R.end;
  L.x = MmScratch(R, P);
  L.ns = ns;
  int rc;                                            // (the frame around mm_prepare + mm_upload_queue is the caller's)
  if ((rc = ctx->d_mm.ensure(ctx, R.end))) return rc;
  if ((rc = ctx->mm_tab.reserve(ctx, L.o_up))) return rc;      // (waits for the previous call's upload)
  char *h = (char *)ctx->mm_tab.h.p;
  L.jobs = (MmJob *)h; L.units = (MmUnit *)(h + L.o_units); L.subs = (MmSub *)(h + L.o_subs); L.prevs = (PfPrev *)(h + L.o_prev);
  L.word = (unsigned long long *)(h + L.o_word);
  if (nj) memcpy(L.jobs, P.jobs.data(), nj * sizeof(MmJob));
  memset(h + L.o_prev, 0, L.o_up - L.o_prev);
  mm_bind(L.jobs, nj, (char *)ctx->d_mm.p, L.x, diff_override, n_diff_override);
  *Lo = L;
  return NDT_OK;
}

// The chain over tables that are on the device (jobs, units, subs) and scratch X of the block at d, for ns = 0, 1 or many
// submaps: the fill of the voxel sets and the triples' differences, then every kernel once for all submaps, with a status
// per submap and the offsets in two levels (per submap; over the submaps when there is more than one -- with one, cloud_off[0 .. 1]
// is final after the first).  The offsets run even with no units.  n_out (one submap; may be NULL): make_map_sub_offsets_kernel.
int mm_queue(ndt_ctx *ctx, const MmJob *jobs, const MmUnit *units, const MmSub *subs, char *d, const MmScratch &X, size_t ns,
             float2 *cloud_xy, unsigned long long *cloud_off, int *status, unsigned long long *n_out, hipStream_t st) {
  const size_t nu = X.nu;
  unsigned *ucnt = (unsigned *)(d + X.ucnt);
  unsigned long long *uoff = (unsigned long long *)(d + X.uoff), *keep = (unsigned long long *)(d + X.keep);
  if (X.tab_words) {      // (jobs with voxel sets: triples, MmPlan::add)
    HIP_TRY(ctx, hipMemsetAsync(d + X.tab, 0xff, X.tab_words * 8, st));
    make_map_diff_kernel<<<(unsigned)X.nj, kMmBlock, 0, st>>>(jobs);
  }
  if (nu) make_map_flag_kernel<<<(unsigned)nu, kMmUnit, 0, st>>>(jobs, units, keep, ucnt);
  if (ns) make_map_sub_offsets_kernel<<<(unsigned)ns, 1024, 0, st>>>(ucnt, subs, uoff, cloud_off, status, n_out);
  if (ns > 1) make_map_sub_scan_kernel<<<1, 1024, 0, st>>>(cloud_off, (int)ns);
  if (nu) make_map_copy_kernel<<<(unsigned)nu, kMmUnit, 0, st>>>(units, keep, uoff, cloud_xy, cloud_off, status);
  HIP_TRY(ctx, hipGetLastError());
  return NDT_OK;
}

// For the callers that stage through ctx->mm_tab (mm_prepare): ONE upload of the tables, then the chain.  A call of one submap
// that reports through n_out alone leaves cloud_off and status NULL: they are the scratch's.
int mm_upload_queue(ndt_ctx *ctx, const MmLayout &L, float *cloud_xy, uint64_t *cloud_off, int *status, uint64_t *n_out, hipStream_t st) {
  char *d = (char *)ctx->d_mm.p;
  HIP_TRY(ctx, ctx->mm_tab.upload(d, 0, L.o_up, st));
  return mm_queue(ctx, (const MmJob *)d, (const MmUnit *)(d + L.o_units), (const MmSub *)(d + L.o_subs), d, L.x, L.ns, (float2 *)cloud_xy,
                  cloud_off ? (unsigned long long *)cloud_off : (unsigned long long *)(d + L.x.coff), status ? status : (int *)(d + L.x.stat),
                  (unsigned long long *)n_out, st);
}

// What the neighbour removal refuses of either form (the host form names its own refusals first).
int remove_neighbors_check(ndt_ctx *ctx, const float *base_xy, size_t base_stride, size_t n_base, const float *list_xy, size_t list_stride,
                           size_t n_list, const float *out_xy, const void *n_out) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!base_xy || n_base == 0 || n_base > (size_t)INT32_MAX || n_list > (size_t)INT32_MAX || (n_list && !list_xy) ||
      !out_xy || !n_out || !mm_stride_ok(base_stride) || (n_list && !mm_stride_ok(list_stride)))
    return fail(ctx, NDT_E_ARG, "ndt_remove_neighbors: bad arguments");
  return NDT_OK;
}

// The all-pairs step on its own, on st, inside the caller's frame: one submap of units over the base cloud, one job whose
// list is the caller's and whose count is the uploaded word.
int queue_remove_neighbors(ndt_ctx *ctx, hipStream_t st, const float *base_xy, size_t base_stride, size_t n_base, const float *list_xy,
                           size_t list_stride, size_t n_list, double thre_neighbor, float *out_xy, uint64_t *n_out) {
  MmPlan P;
  P.add_list(n_list ? list_stride : sizeof(float2), rn_cutoff(thre_neighbor));
  P.unit_room = (n_base + kMmUnit - 1) / kMmUnit;
  P.n_subs = 1;
  MmLayout L;
  int rc;
  if ((rc = mm_prepare(ctx, P, (float2 *)list_xy, nullptr, &L))) return rc;
  L.jobs[0].n_diff = (unsigned long long *)((char *)ctx->d_mm.p + L.o_word);
  *L.word = n_list;
  const MmPiece base = {base_xy, n_base, 0};
  fill_units(L.units, &base, &base + 1, base_stride, 0u);
  L.subs[0] = MmSub{0u, (unsigned)P.unit_room};
  return mm_upload_queue(ctx, L, out_xy, nullptr, nullptr, n_out, st);
}

// What the difference extraction refuses of either form (the host form names its own refusals first).
int difference_check(ndt_ctx *ctx, const float *base_xy, size_t base_stride, size_t n_base, const float *test_xy, size_t test_stride,
                     size_t n_test, double resol, const float *out_xy, const void *n_out) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if ((n_base && !base_xy) || !test_xy || n_test == 0 || n_base + n_test > (size_t)(1u << 30) || !out_xy || !n_out ||
      !mm_stride_ok(base_stride) || !mm_stride_ok(test_stride) || !(resol > 0.0) || !std::isfinite(resol))
    return fail(ctx, NDT_E_ARG, "ndt_difference_extraction: bad arguments");
  return NDT_OK;
}

// One job on st, inside the caller's frame, no units and no submap: the difference list goes straight to out_xy, its count to n_out.
int queue_difference(ndt_ctx *ctx, hipStream_t st, const float *base_xy, size_t base_stride, size_t n_base, const float *test_xy,
                     size_t test_stride, size_t n_test, double resol, float *out_xy, uint64_t *n_out) {
  MmPlan P;
  P.sa = base_stride; P.sb = test_stride;
  P.add(base_xy, base_xy, test_xy, n_base, 0, n_test, resol, 0.f);
  MmLayout L;
  int rc;
  if ((rc = mm_prepare(ctx, P, (float2 *)out_xy, (unsigned long long *)n_out, &L))) return rc;
  return mm_upload_queue(ctx, L, nullptr, nullptr, nullptr, nullptr, st);
}

// What the assembly of one submap refuses of either form (the host form names its own refusals first).
int make_map_check(ndt_ctx *ctx, const float *scans_xy, size_t stride, const uint64_t *offsets, int n_scans, int remove_moving,
                   double resol, double thre_neighbor, const float *out_xy, const void *n_out) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!scans_xy || !offsets || !mm_scan_count_ok(n_scans) || !out_xy || !n_out || !mm_stride_ok(stride) ||
      (remove_moving && (!(resol > 0.0) || !std::isfinite(resol) || !std::isfinite(thre_neighbor))))
    return fail(ctx, NDT_E_ARG, "ndt_make_map: bad arguments");
  if (!mm_offsets_ok(offsets, n_scans))
    return fail(ctx, NDT_E_ARG, "ndt_make_map: offsets must be non-decreasing, scans below 2^29 points");
  return NDT_OK;
}

// One submap on st, inside the caller's frame; scans_xy is device memory, offsets host memory.
int queue_make_map(ndt_ctx *ctx, hipStream_t st, const float *scans_xy, size_t stride, const uint64_t *offsets, int n_scans,
                   int first_submap, int newest, int remove_moving, double resol, double thre_neighbor, float *out_xy, uint64_t *n_out) {
  MmPlan P;
  P.sa = P.sb = stride;
  P.n_subs = 1;
  const ndt_submap_desc D = {scans_xy, offsets, n_scans, first_submap, newest, remove_moving, resol, thre_neighbor, nullptr, 0};
  std::vector<MmPiece> pieces;
  P.unit_room = submap_pieces(D, stride, rn_cutoff(thre_neighbor), &P, &pieces);
  MmLayout L;
  int rc;
  if ((rc = mm_prepare(ctx, P, nullptr, nullptr, &L))) return rc;
  fill_units(L.units, pieces.data(), pieces.data() + pieces.size(), stride, 0u);
  L.subs[0] = MmSub{0u, (unsigned)P.unit_room};
  return mm_upload_queue(ctx, L, out_xy, nullptr, nullptr, n_out, st);
}

}  // namespace

extern "C" {

int ndt_remove_neighbors_dev(ndt_ctx *ctx, const float *base_xy, size_t base_stride, size_t n_base, const float *list_xy,
                             size_t list_stride, size_t n_list, double thre_neighbor, float *out_xy, uint64_t *n_out,
                             void *stream) {
  int rc = remove_neighbors_check(ctx, base_xy, base_stride, n_base, list_xy, list_stride, n_list, out_xy, n_out);
  if (rc) return rc;
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {
    return queue_remove_neighbors(ctx, st, base_xy, base_stride, n_base, list_xy, list_stride, n_list, thre_neighbor, out_xy, n_out);
  });
}

int ndt_remove_neighbors(ndt_ctx *ctx, const float *base_xy_host, size_t base_stride, size_t n_base,
                         const float *list_xy_host, size_t list_stride, size_t n_list, double thre_neighbor,
                         float *out_xy_host, size_t *n_out) {
  if (!n_list) list_stride = 8;
  int rc = remove_neighbors_check(ctx, base_xy_host, base_stride, n_base, list_xy_host, list_stride, n_list, out_xy_host, n_out);
  if (rc) return rc;
  CallFrame fr(ctx);
  if ((rc = fr.open())) return rc;
  hipStream_t st = fr.st;
  const size_t bb = n_base * base_stride, lb = n_list * list_stride;
  Regions R;
  const size_t o_base = R.take(bb), o_list = R.take(lb), o_out = R.take(n_base * sizeof(float2) + 64);
  if ((rc = ctx->d_scan.ensure(ctx, R.end))) return rc;
  if ((rc = ctx->d_off.ensure(ctx, 4))) return rc;
  float *d_base = R.at<float>(ctx->d_scan.p, o_base), *d_list = R.at<float>(ctx->d_scan.p, o_list), *d_out = R.at<float>(ctx->d_scan.p, o_out);
  HIP_TRY(ctx, hipMemcpyAsync(d_base, base_xy_host, bb, hipMemcpyHostToDevice, st));
  if (n_list) HIP_TRY(ctx, hipMemcpyAsync(d_list, list_xy_host, lb, hipMemcpyHostToDevice, st));
  if ((rc = queue_remove_neighbors(ctx, st, d_base, base_stride, n_base, n_list ? d_list : nullptr, list_stride, n_list, thre_neighbor,
                                   d_out, ctx->d_off.p)))
    return rc;
  return read_back_counted<1>(fr, ctx->d_off.p, d_out, sizeof(float2), out_xy_host, n_out, no_check);
}

int ndt_difference_extraction_dev(ndt_ctx *ctx, const float *base_xy, size_t base_stride, size_t n_base,
                                  const float *test_xy, size_t test_stride, size_t n_test, double resol, float *out_xy,
                                  uint64_t *n_out, void *stream) {
  int rc = difference_check(ctx, base_xy, base_stride, n_base, test_xy, test_stride, n_test, resol, out_xy, n_out);
  if (rc) return rc;
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {
    return queue_difference(ctx, st, base_xy, base_stride, n_base, test_xy, test_stride, n_test, resol, out_xy, n_out);
  });
}

int ndt_difference_extraction(ndt_ctx *ctx, const float *base_xy_host, size_t base_stride, size_t n_base,
                              const float *test_xy_host, size_t test_stride, size_t n_test, double resol,
                              float *out_xy_host, size_t *n_out) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if ((n_base && !base_xy_host) || (n_test && !test_xy_host) || !out_xy_host || !n_out || !mm_stride_ok(base_stride) ||
      !mm_stride_ok(test_stride))
    return fail(ctx, NDT_E_ARG, "ndt_difference_extraction: bad arguments");
  if (n_test == 0) { *n_out = 0; return NDT_OK; }
  int rc = difference_check(ctx, base_xy_host, base_stride, n_base, test_xy_host, test_stride, n_test, resol, out_xy_host, n_out);
  if (rc) return rc;
  CallFrame fr(ctx);
  if ((rc = fr.open())) return rc;
  hipStream_t st = fr.st;
  Regions R;
  const size_t o_base = R.take(n_base * base_stride), o_test = R.take(n_test * test_stride), o_out = R.take(n_test * sizeof(float2) + 64);
  if ((rc = ctx->d_scan.ensure(ctx, R.end))) return rc;
  if ((rc = ctx->d_off.ensure(ctx, 4))) return rc;
  float *d_base = R.at<float>(ctx->d_scan.p, o_base), *d_test = R.at<float>(ctx->d_scan.p, o_test), *d_out = R.at<float>(ctx->d_scan.p, o_out);
  if (n_base) HIP_TRY(ctx, hipMemcpyAsync(d_base, base_xy_host, n_base * base_stride, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d_test, test_xy_host, n_test * test_stride, hipMemcpyHostToDevice, st));
  if ((rc = queue_difference(ctx, st, d_base, base_stride, n_base, d_test, test_stride, n_test, resol, d_out, ctx->d_off.p))) return rc;
  return read_back_counted<1>(fr, ctx->d_off.p, d_out, sizeof(float2), out_xy_host, n_out, [&](const uint64_t *cnt) {
    return *cnt == ~0ull ? fail(ctx, NDT_E_ARG, "ndt_difference_extraction: the clouds span more than 2^30 voxels") : NDT_OK;
  });
}

int ndt_make_map_dev(ndt_ctx *ctx, const float *scans_xy, size_t stride, const uint64_t *offsets, int n_scans,
                     int first_submap, int newest, int remove_moving, double resol, double thre_neighbor, float *out_xy,
                     uint64_t *n_out, void *stream) {
  int rc = make_map_check(ctx, scans_xy, stride, offsets, n_scans, remove_moving, resol, thre_neighbor, out_xy, n_out);
  if (rc) return rc;
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {
    return queue_make_map(ctx, st, scans_xy, stride, offsets, n_scans, first_submap, newest, remove_moving, resol, thre_neighbor,
                           out_xy, n_out);
  });
}

int ndt_make_map(ndt_ctx *ctx, const float *scans_xy_host, size_t stride, const uint64_t *offsets, int n_scans,
                 int first_submap, int newest, int remove_moving, double resol, double thre_neighbor,
                 float *out_xy_host, size_t *n_out) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!scans_xy_host || !offsets || n_scans <= 0 || !out_xy_host || !n_out || !mm_stride_ok(stride))
    return fail(ctx, NDT_E_ARG, "ndt_make_map: bad arguments");
  const size_t total = (size_t)offsets[n_scans] - (size_t)offsets[0];
  if (total == 0) { *n_out = 0; return NDT_OK; }
  int rc = make_map_check(ctx, scans_xy_host, stride, offsets, n_scans, remove_moving, resol, thre_neighbor, out_xy_host, n_out);
  if (rc) return rc;
  CallFrame fr(ctx);
  if ((rc = fr.open())) return rc;
  hipStream_t st = fr.st;
  const ndt_submap_desc whole = {scans_xy_host, offsets, n_scans, first_submap, newest, remove_moving, resol, thre_neighbor, nullptr, 0};
  Regions R;
  const size_t o_in = R.take(total * stride), o_out = R.take(submap_points(whole) * sizeof(float2) + 64);
  if ((rc = ctx->d_scan.ensure(ctx, R.end))) return rc;
  if ((rc = ctx->d_off.ensure(ctx, 4))) return rc;
  float *d_in = R.at<float>(ctx->d_scan.p, o_in), *d_out = R.at<float>(ctx->d_scan.p, o_out);
  HIP_TRY(ctx, hipMemcpyAsync(d_in, (const char *)scans_xy_host + (size_t)offsets[0] * stride, total * stride,
                              hipMemcpyHostToDevice, st));
  const std::vector<uint64_t> rel = rel_offsets(offsets, (size_t)n_scans);
  if ((rc = queue_make_map(ctx, st, d_in, stride, rel.data(), n_scans, first_submap, newest, remove_moving, resol, thre_neighbor, d_out,
                           ctx->d_off.p)))
    return rc;
  return read_back_counted<1>(fr, ctx->d_off.p, d_out, sizeof(float2), out_xy_host, n_out, [&](const uint64_t *cnt) {
    return *cnt == ~0ull ? fail(ctx, NDT_E_ARG, "ndt_make_map: a scan triple spans more than 2^30 voxels") : NDT_OK;
  });
}

}  // extern "C"

// ---- batched local-map assembly (ndt_local_map_batch_dev / ndt_local_map_batch) ----

namespace {

// The synchronous refusals of a batched assembly: nothing changed, nothing queued.
int check_local_map_batch(ndt_ctx *ctx, const ndt_submap_desc *subs, int n_subs, size_t stride, float leaf, const void *cloud_xy,
                          const void *cloud_off, const void *target_xy, const void *target_off, const void *status,
                          const std::string &fn) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (n_subs < 1) return fail(ctx, NDT_E_ARG, fn + ": n_subs < 1");
  if (!subs || !cloud_xy || !cloud_off || !status || (!target_xy) != (!target_off))
    return fail(ctx, NDT_E_ARG, fn + ": NULL array (subs, cloud_xy, cloud_off, status, or one of target_xy / target_off alone)");
  for (int s = 0; s < n_subs; ++s) {
    const ndt_submap_desc &D = subs[s];
    const std::string which = fn + ": submap " + std::to_string(s);
    if (!mm_scan_count_ok(D.n_scans)) return fail(ctx, NDT_E_ARG, which + ": n_scans < 1 (or above 2^20)");
    if (!D.scans_xy || !D.offsets) return fail(ctx, NDT_E_ARG, which + ": NULL scans_xy or offsets");
    if (!mm_offsets_ok(D.offsets, D.n_scans))
      return fail(ctx, NDT_E_ARG, which + ": offsets must be non-decreasing, scans below 2^29 points");
  }
  if (!mm_stride_ok(stride)) return fail(ctx, NDT_E_ARG, fn + ": bad stride (need stride_bytes >= 8, % 8 == 0 and below 2^32)");
  for (int s = 0; s < n_subs; ++s) {
    const ndt_submap_desc &D = subs[s];
    const std::string which = fn + ": submap " + std::to_string(s);
    if (D.remove_moving && (!(D.resol > 0.0) || !std::isfinite(D.resol) || !std::isfinite(D.thre_neighbor)))
      return fail(ctx, NDT_E_ARG, which + ": remove_moving needs a positive finite resol (and a finite thre_neighbor)");
    if (D.n_prev > 0 && !D.prev_xy) return fail(ctx, NDT_E_ARG, which + ": n_prev > 0 with NULL prev_xy");
    if (D.n_prev > (size_t)1 << 40) return fail(ctx, NDT_E_ARG, which + ": n_prev above 2^40 points");
  }
  if (target_xy && !(leaf > 0)) return fail(ctx, NDT_E_ARG, fn + ": a target needs leaf > 0");
  return NDT_OK;
}

// The assembly of every submap (and, with a target, the filter behind it) on st, inside the caller's frame; the scans and
// previous clouds of `subs` are device memory, its offsets host memory.  up_bytes, n_triples (may be NULL): the size of the
// call's one table upload and the scan triples it computes (a session set's statistics).
int queue_local_map_batch(ndt_ctx *ctx, hipStream_t st, const ndt_submap_desc *subs, int n_subs, size_t stride, float leaf,
                          float *cloud_xy, uint64_t *cloud_off, float *target_xy, uint64_t *target_off, int *status,
                          size_t *up_bytes = nullptr, size_t *n_triples = nullptr) {
  // the triples (jobs) and the pieces of every submap's cloud
  MmPlan P;
  P.sa = P.sb = stride;
  P.n_subs = (size_t)n_subs;
  std::vector<MmPiece> pieces;
  std::vector<size_t> piece_end((size_t)n_subs);       // pieces of submap s: [piece_end[s - 1], piece_end[s])
  size_t nu = 0, cap_cloud = 0, total_prev = 0;
  double cut_of = 0.0; float cut = 0.f; bool have_cut = false;
  for (int s = 0; s < n_subs; ++s) {
    const ndt_submap_desc &D = subs[s];
    if (D.remove_moving && (!have_cut || !same_bits(&cut_of, &D.thre_neighbor, sizeof(double)))) {
      cut = rn_cutoff(D.thre_neighbor); cut_of = D.thre_neighbor; have_cut = true;      // (a search over float bits: once per distinct bound)
    }
    nu += submap_pieces(D, stride, cut, &P, &pieces);
    piece_end[s] = pieces.size();
    cap_cloud += submap_points(D);
    total_prev += D.n_prev;
  }
  if (nu > (size_t)INT32_MAX || P.jobs.size() > (size_t)INT32_MAX)
    return fail(ctx, NDT_E_ARG, "ndt_local_map_batch_dev: more than 2^31 units of 256 points or scan triples in one call");
  P.unit_room = nu;
  MmLayout L;
  int rc;
  if ((rc = mm_prepare(ctx, P, nullptr, nullptr, &L))) return rc;
  MmUnit *u = L.units;
  for (int s = 0; s < n_subs; ++s) {
    L.subs[s].u0 = (unsigned)(u - L.units);
    u = fill_units(u, pieces.data() + (s ? piece_end[s - 1] : 0), pieces.data() + piece_end[s], stride, (unsigned)s);
    L.subs[s].u1 = (unsigned)(u - L.units);
    L.prevs[s] = PfPrev{subs[s].n_prev ? subs[s].prev_xy : nullptr, (unsigned long long)subs[s].n_prev};
  }
  if (up_bytes) *up_bytes = L.o_up;
  if (n_triples) *n_triples = P.jobs.size();
  if ((rc = mm_upload_queue(ctx, L, cloud_xy, cloud_off, status, nullptr, st))) return rc;
  if (target_xy) {
    // Submap::filterPoints of every cloud, behind its previous submap's cloud: cloud_xy / cloud_off are the filter's input form
    const PfPrev *d_prev = (const PfPrev *)((const char *)ctx->d_mm.p + L.o_prev);
    if ((rc = pf_run<true>(ctx, cloud_xy, sizeof(float2), cloud_off, n_subs, cap_cloud, leaf, target_xy, target_off, d_prev,
                           stride, total_prev, status, st)))
      return rc;
  }
  return NDT_OK;
}

}  // namespace

extern "C" {

int ndt_local_map_batch_dev(ndt_ctx *ctx, const ndt_submap_desc *subs, int n_subs, size_t stride, float leaf,
                            float *cloud_xy, uint64_t *cloud_off, float *target_xy, uint64_t *target_off, int *status,
                            void *stream) {
  int rc = check_local_map_batch(ctx, subs, n_subs, stride, leaf, cloud_xy, cloud_off, target_xy, target_off, status,
                                 "ndt_local_map_batch_dev");
  if (rc) return rc;
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {
    return queue_local_map_batch(ctx, st, subs, n_subs, stride, leaf, cloud_xy, cloud_off, target_xy, target_off, status);
  });
}

int ndt_local_map_batch(ndt_ctx *ctx, const ndt_submap_desc *subs, int n_subs, size_t stride, float leaf,
                        float *cloud_xy_host, uint64_t *cloud_off_host, float *target_xy_host, uint64_t *target_off_host,
                        int *status_host) {
  int rc = check_local_map_batch(ctx, subs, n_subs, stride, leaf, cloud_xy_host, cloud_off_host, target_xy_host,
                                 target_off_host, status_host, "ndt_local_map_batch");
  if (rc) return rc;
  const bool want_target = target_xy_host != nullptr;
  // every submap's scans and previous cloud into one host block, uploaded with ONE copy; the clouds and the targets behind it
  const size_t S = (size_t)n_subs;
  std::vector<size_t> o_scan(S), o_prev(S);
  Regions R;
  size_t cap_cloud = 0, total_prev = 0;
  for (size_t s = 0; s < S; ++s) {
    const ndt_submap_desc &D = subs[s];
    o_scan[s] = R.take((size_t)(D.offsets[D.n_scans] - D.offsets[0]) * stride);
    o_prev[s] = R.take(want_target ? D.n_prev * stride : 0);
    cap_cloud += submap_points(D);
    total_prev += D.n_prev;
  }
  const size_t in_bytes = R.end, cap_target = want_target ? cap_cloud + total_prev : 0;
  const size_t o_cloud = R.take(cap_cloud * sizeof(float2) + 64), o_target = R.take(cap_target * sizeof(float2) + 64);
  CallFrame fr(ctx);
  if ((rc = fr.open())) return rc;
  hipStream_t st = fr.st;
  if ((rc = ctx->d_scan.ensure(ctx, R.end))) return rc;
  if ((rc = ctx->d_off.ensure(ctx, 3 * (S + 1)))) return rc;   // cloud_off | target_off | status (ints)
  std::vector<unsigned char> stage(in_bytes);
  std::vector<ndt_submap_desc> dsubs(subs, subs + S);
  std::vector<std::vector<uint64_t>> rel(S);
  char *d = (char *)ctx->d_scan.p;
  for (size_t s = 0; s < S; ++s) {
    const ndt_submap_desc &D = subs[s];
    const size_t nb = (size_t)(D.offsets[D.n_scans] - D.offsets[0]) * stride;
    if (nb) memcpy(stage.data() + o_scan[s], (const char *)D.scans_xy + (size_t)D.offsets[0] * stride, nb);
    if (want_target && D.n_prev) memcpy(stage.data() + o_prev[s], D.prev_xy, D.n_prev * stride);
    rel[s] = rel_offsets(D.offsets, (size_t)D.n_scans);
    dsubs[s].scans_xy = (const float *)(d + o_scan[s]);
    dsubs[s].offsets = rel[s].data();
    dsubs[s].prev_xy = want_target && D.n_prev ? (const float *)(d + o_prev[s]) : nullptr;
    if (!want_target) dsubs[s].n_prev = 0;
  }
  if (in_bytes) HIP_TRY(ctx, hipMemcpyAsync(d, stage.data(), in_bytes, hipMemcpyHostToDevice, st));
  uint64_t *d_coff = ctx->d_off.p, *d_toff = d_coff + S + 1;
  int *d_status = (int *)(d_toff + S + 1);
  if ((rc = queue_local_map_batch(ctx, st, dsubs.data(), n_subs, stride, leaf, (float *)(d + o_cloud), d_coff,
                                  want_target ? (float *)(d + o_target) : nullptr, want_target ? d_toff : nullptr, d_status))) {
    hipError_t e = hipStreamSynchronize(st); (void)e;          // (the staged block is read by the copy queued above)
    return rc;
  }
  std::vector<uint64_t> back(3 * (S + 1));
  HIP_TRY(ctx, hipMemcpyAsync(back.data(), d_coff, back.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  memcpy(cloud_off_host, back.data(), (S + 1) * sizeof(uint64_t));
  if (want_target) memcpy(target_off_host, back.data() + S + 1, (S + 1) * sizeof(uint64_t));
  memcpy(status_host, back.data() + 2 * (S + 1), S * sizeof(int));
  const size_t nc = (size_t)back[S], nt = want_target ? (size_t)back[2 * S + 1] : 0;
  if (nc) HIP_TRY(ctx, hipMemcpyAsync(cloud_xy_host, d + o_cloud, nc * sizeof(float2), hipMemcpyDeviceToHost, st));
  if (nt) HIP_TRY(ctx, hipMemcpyAsync(target_xy_host, d + o_target, nt * sizeof(float2), hipMemcpyDeviceToHost, st));
  return fr.close_and_wait();
}

}  // extern "C"

// ---- device-resident lockstep sessions (ndt_sessions_*; state, kernels and the step in ndt_sessions.hip.h) ----

#include "ndt_sessions.hip.h"

namespace {

// the refusals every call on a set starts with; `i` < 0: the call names no session
int check_set(const ndt_sessions *s, int i, bool with_index, const char *fn) {
  if (!s) return fail(nullptr, NDT_E_ARG, "null session set");
  if (s->dead) return fail(s->ctx, NDT_E_HIP, std::string(fn) + ": the set is unusable after a HIP failure inside a step");
  if (with_index && (i < 0 || i >= s->S)) return fail(s->ctx, NDT_E_ARG, std::string(fn) + ": session " + std::to_string(i) + " out of range");
  return NDT_OK;
}

// a set without an archive, to a call that reads it (the one sentence)
int refuse_no_archive(const ndt_sessions *s, const std::string &f) { return fail(s->ctx, NDT_E_ARG, f + ": the set has no scan archive (ndt_sessions_archive_enable)"); }

// ... and those of the archive's read-outs: check_set's, then a set without an archive
int check_archive(const ndt_sessions *s, int i, const char *fn) {
  const int rc = check_set(s, i, true, fn);
  return rc || s->archive ? rc : refuse_no_archive(s, fn);
}

// The bracket of every call that changes or searches a set, in CallFrame's manner: enter() holds check_set's refusals; the call's
// own refusals follow in the call's own order (refuse(): one under the call's name); run() refuses while an ndt_map_rebuild_begin
// is open on the context, runs the body and, on NDT_E_HIP / NDT_E_NOMEM, marks the set dead and drains the stream (the context
// stays usable: nothing of the set is in flight).  kills = false, ndt_sessions_occ_integrate and ndt_sessions_occ_rebuild: their
// scratch is the context's, taken through CallFrame, and they write grids, nothing of the set: it stays as usable as it was.
struct SetCall {
  ndt_sessions *s; const char *fn; bool kills = true;
  ndt_ctx *ctx = nullptr; std::string f;
  int enter() { const int rc = check_set(s, 0, false, fn); if (!rc) { ctx = s->ctx; f = fn; } return rc; }
  int refuse(const std::string &what) const { return fail(ctx, NDT_E_ARG, f + ": " + what); }
  template <typename Body> int run(Body &&body) {
    if (ctx->pending_map) return refuse_pending(ctx, f);
    const int rc = body();
    if (kills && (rc == NDT_E_HIP || rc == NDT_E_NOMEM)) { s->dead = true; hipError_t e = hipStreamSynchronize(ctx->stream); (void)e; }
    return rc;
  }
};

// Entry c of a named-session list: out of range, not started, named twice (entry_of: S entries, -1 before the first); *who: the
// entry's name, for the caller's own refusals of it.
int check_named(const SetCall &call, const int *which, int c, std::vector<int> &entry_of, std::string *who) {
  const int i = which[c];
  *who = "entry " + std::to_string(c) + ": session " + std::to_string(i);
  if (i < 0 || i >= call.s->S) return call.refuse(*who + " out of range");
  if (!call.s->ses[(size_t)i].started) return call.refuse(*who + " has not started");
  if (entry_of[(size_t)i] >= 0) return call.refuse(*who + " is entry " + std::to_string(entry_of[(size_t)i]) + " again");
  entry_of[(size_t)i] = c;
  return NDT_OK;
}

int step_entry(ndt_sessions *s, const double *raw_host, const double *raw_dev, size_t stride, const uint64_t *raw_offsets,
               const double *odo_host, const double *odo_dev, const unsigned char *active, ndt_session_step *out, const char *fn) {
  SetCall call{s, fn};
  const int rc = call.enter();
  if (rc) return rc;
  if (!raw_offsets || !out || (!odo_host && !odo_dev)) return call.refuse("NULL array (raw_offsets, odo or out)");
  if (stride < 16 || (stride & 7)) return call.refuse("bad stride (need stride_bytes >= 16 and % 8 == 0)");
  for (int i = 0; i < s->S; ++i)
    if (raw_offsets[i + 1] < raw_offsets[i]) return call.refuse("session " + std::to_string(i) + ": offsets decrease");
  if (raw_offsets[s->S] > raw_offsets[0] && !raw_host && !raw_dev) return call.refuse("NULL array (raw_xy)");
  return call.run([&] { return SsStep{s, raw_host, raw_dev, stride, raw_offsets, odo_host, odo_dev, active, out}.run(); });
}

}  // namespace

extern "C" {

int ndt_session_default_params(ndt_session_params *p) {
  if (!p) return NDT_E_ARG;
  memset(p, 0, sizeof(*p));
  ndt_default_params(&p->match);
  p->match.resolution = 0.3f; p->match.step_size = 0.1; p->match.trans_eps = 0.01; p->match.max_iter = 35;
  p->match.grid_margin = 8;
  ndt_fuse_default_params(&p->fuse);
  p->fuse.coe_ndt_cov = 1.0; p->fuse.coe_vel = 0.1; p->fuse.coe_omega = 0.5; p->fuse.del_time = 0.5; p->fuse.score_thre = 0.5;
  p->space = 0.05; p->space_thre = 0.25; p->leaf = 0.05f; p->resol = 0.05; p->thre_neighbor = 0.2; p->sep_thre = 10.0;
  p->remove_moving = 1;
  return NDT_OK;
}

int ndt_sessions_create(ndt_ctx *ctx, int n_sessions, const ndt_session_params *prm, ndt_sessions **out) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (n_sessions < 1) return fail(ctx, NDT_E_ARG, "ndt_sessions_create: n_sessions < 1");
  if (!prm || !out) return fail(ctx, NDT_E_ARG, "ndt_sessions_create: NULL argument (prm or out)");
  int rc = ss_check_params(ctx, *prm);
  if (rc) return rc;
  if (ctx->pending_map) return refuse_pending(ctx, "ndt_sessions_create");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ndt_sessions *s = new (std::nothrow) ndt_sessions;
  if (!s) return fail(ctx, NDT_E_NOMEM, "ndt_sessions_create: out of memory");
  s->ctx = ctx; s->S = n_sessions; s->prm = *prm;
  s->ses.resize((size_t)n_sessions);
  const size_t S = (size_t)n_sessions;
  auto zeroed = [&](auto &buf, size_t n) {
    int r = buf.ensure(ctx, n);
    if (!r && hipMemsetAsync(buf.p, 0, buf.bytes, ctx->stream) != hipSuccess) r = fail(ctx, NDT_E_HIP, "ndt_sessions_create: hipMemsetAsync failed");
    return r;
  };
  if ((rc = zeroed(s->last_pose, 3 * S)) || (rc = zeroed(s->last_cov, 9 * S)) || (rc = zeroed(s->prev_odo, 3 * S)) ||
      (rc = zeroed(s->plen, S)) || (rc = zeroed(s->motion, 3 * S)) || (rc = zeroed(s->pred, 3 * S)) || (rc = zeroed(s->init, 3 * S)) ||
      (rc = zeroed(s->fused, 3 * S)) || (rc = zeroed(s->cov, 9 * S)) || (rc = zeroed(s->rs_status, S)) || (rc = zeroed(s->successful, S)) ||
      (rc = zeroed(s->res, S)) || (rc = zeroed(s->rec, S)) || (rc = zeroed(s->cloud_off, S + 1)) || (rc = zeroed(s->target_off, S + 1)) ||
      (rc = zeroed(s->status, S)) || (rc = zeroed(s->tri_off, S + 1)) || (rc = zeroed(s->tri_status, S))) {
    delete s;
    return rc;
  }
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) { delete s; return fail(ctx, NDT_E_HIP, "ndt_sessions_create: hipStreamSynchronize failed"); }
  *out = s;
  return NDT_OK;
}

int ndt_sessions_destroy(ndt_sessions *s) {
  if (!s) return fail(nullptr, NDT_E_ARG, "null session set");
  ndt_ctx *ctx = s->ctx;
  hipError_t e = hipSetDevice(ctx->device);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)e;
  for (auto &Q : s->ses) {
    if (Q.map) ndt_map_destroy(Q.map);
    for (ndt_map *m : Q.loop_maps)
      if (m) ndt_map_destroy(m);
  }
  delete s;
  return NDT_OK;
}

int ndt_sessions_step(ndt_sessions *s, const double *raw_xy_host, size_t stride, const uint64_t *raw_offsets, const double *odo_host,
                      const unsigned char *active, ndt_session_step *out) {
  return step_entry(s, raw_xy_host, nullptr, stride, raw_offsets, odo_host, nullptr, active, out, "ndt_sessions_step");
}

int ndt_sessions_step_dev(ndt_sessions *s, const double *raw_xy_dev, size_t stride, const uint64_t *raw_offsets, const double *odo_dev,
                          const unsigned char *active, ndt_session_step *out) {
  return step_entry(s, nullptr, raw_xy_dev, stride, raw_offsets, nullptr, odo_dev, active, out, "ndt_sessions_step_dev");
}

int ndt_sessions_local_map(const ndt_sessions *s, int i, const float **xy_dev, size_t *n, const ndt_map **map) {
  const int rc = check_set(s, i, true, "ndt_sessions_local_map");
  if (rc) return rc;
  const SsSession &Q = s->ses[(size_t)i];
  if (xy_dev) *xy_dev = Q.has_target && Q.t_n ? (const float *)(s->target[Q.buf].p + Q.t_off) : nullptr;
  if (n) *n = Q.has_target ? (size_t)Q.t_n : 0;
  if (map) *map = Q.map;
  return NDT_OK;
}

int ndt_sessions_submap_cloud(const ndt_sessions *s, int i, const float **xy_dev, size_t *n) {
  const int rc = check_set(s, i, true, "ndt_sessions_submap_cloud");
  if (rc) return rc;
  const SsSession &Q = s->ses[(size_t)i];
  if (xy_dev) *xy_dev = Q.has_target && Q.c_n ? (const float *)(s->cloud[Q.buf].p + Q.c_off) : nullptr;
  if (n) *n = Q.has_target ? (size_t)Q.c_n : 0;
  return NDT_OK;
}

int ndt_sessions_global_map(ndt_sessions *s, int i, float *out_xy_host, size_t capacity, size_t *n_out, uint64_t *sub_offsets,
                            int *n_submaps) {
  const int rc = check_set(s, i, true, "ndt_sessions_global_map");
  if (rc) return rc;
  ndt_ctx *ctx = s->ctx;
  const SsSession &Q = s->ses[(size_t)i];
  const size_t n_closed = (size_t)Q.closed_off.back(), n_tail = Q.has_target ? (size_t)(Q.t_n - Q.n_prev) : 0;
  if (out_xy_host && capacity < n_closed + n_tail)
    return fail(ctx, NDT_E_ARG, "ndt_sessions_global_map: session " + std::to_string(i) + ": capacity below the map's " +
                                    std::to_string(n_closed + n_tail) + " points");
  if (n_out) *n_out = n_closed + n_tail;
  if (n_submaps) *n_submaps = Q.n_closed + 1;
  if (sub_offsets) {
    for (size_t k = 0; k < Q.closed_off.size(); ++k) sub_offsets[k] = Q.closed_off[k];
    sub_offsets[Q.closed_off.size()] = n_closed + n_tail;
  }
  if (!out_xy_host) return NDT_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (n_closed) HIP_TRY(ctx, hipMemcpyAsync(out_xy_host, Q.closed.p, n_closed * sizeof(float2), hipMemcpyDeviceToHost, ctx->stream));
  if (n_tail)
    HIP_TRY(ctx, hipMemcpyAsync(out_xy_host + 2 * n_closed, s->target[Q.buf].p + Q.t_off + Q.n_prev, n_tail * sizeof(float2),
                                hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return NDT_OK;
}

int ndt_sessions_get_stats(const ndt_sessions *s, ndt_sessions_stats *out) {
  if (!s) return fail(nullptr, NDT_E_ARG, "null session set");
  if (!out) return fail(s->ctx, NDT_E_ARG, "ndt_sessions_get_stats: NULL out");
  *out = s->stats;
  return NDT_OK;
}

int ndt_sessions_trajectory(const ndt_sessions *s, int i, double *poses_host, size_t capacity, size_t *n_scans, int *sub_first,
                            int *sub_anchor, int *n_submaps, size_t *store_first) {
  const int rc = check_set(s, i, true, "ndt_sessions_trajectory");
  if (rc) return rc;
  const SsSession &Q = s->ses[(size_t)i];
  const size_t n = (size_t)Q.n_poses;
  if (poses_host && capacity < n)
    return fail(s->ctx, NDT_E_ARG, "ndt_sessions_trajectory: session " + std::to_string(i) + ": capacity below the trajectory's " +
                                       std::to_string(n) + " poses");
  if (n_scans) *n_scans = n;
  if (n_submaps) *n_submaps = Q.n_closed + 1;
  if (store_first) *store_first = n - (Q.scan_off.size() - 1);
  if (!poses_host) return NDT_OK;
  if (n) memcpy(poses_host, Q.traj.data(), n * 24);
  for (int m = 0; m <= Q.n_closed; ++m) {
    if (sub_first) sub_first[m] = Q.sub_first[(size_t)m];
    if (sub_anchor) sub_anchor[m] = n ? ss_anchor(Q, m) : 0;
  }
  return NDT_OK;
}

int ndt_sessions_correct(ndt_sessions *s, const int *which, int n_corr, const double *const *new_poses_host, const size_t *n_poses,
                         int *status_host) {
  SetCall call{s, "ndt_sessions_correct"};
  int rc = call.enter();
  if (rc) return rc;
  if (!which || !new_poses_host || !n_poses || !status_host) return call.refuse("NULL array (which, new_poses, n_poses or status)");
  if (n_corr < 1) return call.refuse("n_corr < 1");
  std::vector<int> entry_of((size_t)s->S, -1);
  std::string who;
  for (int c = 0; c < n_corr; ++c) {
    if ((rc = check_named(call, which, c, entry_of, &who))) return rc;
    const int have = s->ses[(size_t)which[c]].n_poses;
    if (!new_poses_host[c]) return call.refuse(who + ": NULL trajectory");
    if (n_poses[c] != (size_t)have)
      return call.refuse(who + ": " + std::to_string(n_poses[c]) + " poses for a trajectory of " + std::to_string(have) + " scans (a stale trajectory)");
    for (size_t k = 0; k < 3 * n_poses[c]; ++k)
      if (!(std::fabs(new_poses_host[c][k]) <= DBL_MAX)) return call.refuse(who + ": scan " + std::to_string(k / 3) + ": a pose is not finite");
  }
  return call.run([&] { return SsCorrect{s, which, n_corr, new_poses_host, status_host}.run(); });
}

// ---- the scan archive (filled by SsStep::book, read by ndt_sessions_occ_rebuild) ----

int ndt_sessions_archive_enable(ndt_sessions *s) {
  const int rc = check_set(s, 0, false, "ndt_sessions_archive_enable");
  if (rc) return rc;
  if (s->archive) return NDT_OK;
  for (int i = 0; i < s->S; ++i)
    if (s->ses[(size_t)i].started)
      return fail(s->ctx, NDT_E_ARG, "ndt_sessions_archive_enable: session " + std::to_string(i) + " has already started");
  s->archive = true;
  return NDT_OK;
}

int ndt_sessions_archive_info(const ndt_sessions *s, int i, size_t *n_scans, size_t *n_points) {
  const int rc = check_archive(s, i, "ndt_sessions_archive_info");
  if (rc) return rc;
  const SsSession &Q = s->ses[(size_t)i];
  if (n_scans) *n_scans = Q.arch_off.size() - 1;
  if (n_points) *n_points = (size_t)Q.arch_off.back();
  return NDT_OK;
}

int ndt_sessions_archive_scans(ndt_sessions *s, int i, size_t first, size_t count, double *xy_host, size_t capacity_points,
                               uint64_t *offsets, size_t *n_points) {
  const int rc = check_archive(s, i, "ndt_sessions_archive_scans");
  if (rc) return rc;
  ndt_ctx *ctx = s->ctx;
  const SsSession &Q = s->ses[(size_t)i];
  const size_t have = Q.arch_off.size() - 1;
  const std::string who = "ndt_sessions_archive_scans: session " + std::to_string(i);
  if (first > have || count > have - first)
    return fail(ctx, NDT_E_ARG, who + ": scans [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(count) +
                                    ") outside the archive's " + std::to_string(have));
  const uint64_t p0 = Q.arch_off[first], np = Q.arch_off[first + count] - p0;
  if (xy_host && capacity_points < np)
    return fail(ctx, NDT_E_ARG, who + ": capacity below the range's " + std::to_string(np) + " points");
  if (n_points) *n_points = (size_t)np;
  if (offsets)
    for (size_t k = 0; k <= count; ++k) offsets[k] = Q.arch_off[first + k] - p0;
  if (!xy_host || !np) return NDT_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemcpyAsync(xy_host, Q.arch.p + p0, (size_t)np * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return NDT_OK;
}

int ndt_sessions_archive_view(const ndt_sessions *s, int i, const double **xy_dev, size_t *n_points) {
  const int rc = check_archive(s, i, "ndt_sessions_archive_view");
  if (rc) return rc;
  const SsSession &Q = s->ses[(size_t)i];
  if (xy_dev) *xy_dev = Q.arch_off.back() ? (const double *)Q.arch.p : nullptr;
  if (n_points) *n_points = (size_t)Q.arch_off.back();
  return NDT_OK;
}

int ndt_sessions_remake_closed(ndt_sessions *s, const int *which, int n_named, int *status_host) {
  SetCall call{s, "ndt_sessions_remake_closed"};
  int rc = call.enter();
  if (rc) return rc;
  if (!which || !status_host) return call.refuse("NULL array (which or status)");
  if (n_named < 1) return call.refuse("n_named < 1");
  std::vector<int> entry_of((size_t)s->S, -1);
  std::string who;
  for (int c = 0; c < n_named; ++c)
    if ((rc = check_named(call, which, c, entry_of, &who))) return rc;
  if (!s->archive) return refuse_no_archive(s, call.f);
  return call.run([&] { return SsRemakeCall{s, which, n_named, status_host}.run(); });
}

}  // extern "C"

// ---- relocalisation: score sweep, candidate pick, refinement (ndt_score_*, ndt_lattice_*, ndt_relocalize*; kernels in
//      ndt_score.hip.h) ----

namespace {

// ndt_lattice_size's rule: false for a NULL lattice, a dimension below 1, a non-finite origin or step, more than 2^31 - 1 poses
bool lattice_count(const ndt_pose_lattice *l, uint64_t *n) {
  if (!l || l->nx < 1 || l->ny < 1 || l->nyaw < 1) return false;
  for (double v : {l->x0, l->y0, l->yaw0, l->step_x, l->step_y, l->step_yaw})
    if (!std::isfinite(v)) return false;
  const uint64_t xy = (uint64_t)l->nx * (uint64_t)l->ny;                // < 2^62
  if (xy > (uint64_t)INT32_MAX || xy * (uint64_t)l->nyaw > (uint64_t)INT32_MAX) return false;
  *n = xy * (uint64_t)l->nyaw;
  return true;
}

Lattice lattice_of(const ndt_pose_lattice &l) { return Lattice{l.x0, l.y0, l.yaw0, l.step_x, l.step_y, l.step_yaw, l.nx, l.ny, l.nyaw}; }

// The refusals every score call starts with (synchronous, nothing queued).
int score_check(ndt_ctx *ctx, const ndt_map *map, const void *scan, size_t n, size_t stride, const char *fn) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  const std::string f(fn);
  if (!map || !scan) return fail(ctx, NDT_E_ARG, f + ": NULL map or scan");
  if (!map->ctx || !map->view.cent) return fail(ctx, NDT_E_ARG, f + ": the map was never built");
  if (map->device != ctx->device) return fail(ctx, NDT_E_ARG, f + ": the map was built on another device");
  if (n == 0 || n > (size_t)INT32_MAX) return fail(ctx, NDT_E_ARG, f + ": need 1 <= n <= 2^31 - 1 scan points");
  if (stride < 8 || (stride & 7)) return fail(ctx, NDT_E_ARG, f + ": bad stride (need stride_bytes >= 8 and % 8 == 0)");
  if (ctx->pending_map) return refuse_pending(ctx, f);
  return NDT_OK;
}

// The sweep on st, inside the caller's frame: one kernel that reads the map (MapRead).  A sweep on another stream than the one
// that carries the map's builds is, to a build, what a deferred launch is -- work its stream order does not cover -- and is
// entered as one.
int queue_score(ndt_ctx *ctx, const ndt_map *map, hipStream_t st, const float *scan, size_t n, size_t stride, const double *poses,
                const Lattice &L, uint64_t P, double *score, unsigned *pairs) {
  MapRead rd{ctx, st, &map, 1};
  { const int rc = rd.begin(); if (rc) return rc; }
  const MapView &V = map->view;
  const bool sse = map->prm.transform_sse != 0, incl = map->prm.radius_inclusive != 0;
  const bool chk = !(V.e_hi > 1.0 + 1e-6);            // (launch_align's rule, in the same instances)
  const int staged = ctx->score_stage && n <= (size_t)kScoreStagePts;
  const size_t lds = staged ? n * sizeof(float2) : 0;
  // workgroups: as many as the CUs hold at this LDS size (four of four waves at most: the kernel's registers allow four waves per SIMD), or NDT_OPT_WORKGROUPS
  const size_t per_cu = std::min<size_t>(4, std::max<size_t>(1, (size_t)(150 * 1024) / (lds + 1024)));
  const uint64_t tiles = (P + kScoreTile - 1) / kScoreTile;
  const uint64_t want = ctx->workgroups > 0 ? (uint64_t)ctx->workgroups : (uint64_t)ctx->num_cus * per_cu;
  const unsigned grid = (unsigned)std::min<uint64_t>(tiles, want);
  Event *evr = rd.ev;
  auto sweep = [&](auto S, auto I, auto C) {
    hipExtLaunchKernelGGL((ndt_score_kernel<decltype(S)::value, decltype(I)::value, decltype(C)::value>), dim3(grid), dim3(kScoreBlock),
                          lds, st, evr[0], evr[1], 0, V, map->prm.libm_f32, scan, stride, (int)n, staged, poses, L,
                          (unsigned long long)P, score, pairs);
  };
  const std::true_type yes; const std::false_type no;
  if (sse && incl)      sweep(yes, yes, yes);
  else if (sse && !chk) sweep(yes, no, no);
  else if (sse)         sweep(yes, no, yes);
  else if (incl)        sweep(no, yes, yes);
  else                  sweep(no, no, yes);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(ctx, NDT_E_HIP, std::string("ndt_score: ") + hipGetErrorString(e));
  return rd.entered(NDT_OK, /*end_carried=*/false, /*deferred=*/st != map->ctx->stream, "ndt_score");
}

// The pick on st, inside the caller's frame (d_sel).
int queue_select(ndt_ctx *ctx, hipStream_t st, const Lattice &L, uint64_t P, const double *score, const unsigned *pairs, int top_k,
                 int local_max, unsigned long long *cand, int *n_cand) {
  const size_t tiles = (size_t)((P + kSelTile - 1) / kSelTile);
  Regions R;
  const size_t o_sorted = R.take(tiles * kSelTile * sizeof(unsigned short), 256), o_cnt = R.take(tiles * sizeof(unsigned), 256),
               o_head = R.take(tiles * sizeof(unsigned), 256);
  int rc;
  if ((rc = ctx->d_sel.ensure(ctx, R.end))) return rc;
  unsigned short *sorted = R.at<unsigned short>(ctx->d_sel.p, o_sorted);
  unsigned *cnt = R.at<unsigned>(ctx->d_sel.p, o_cnt), *head = R.at<unsigned>(ctx->d_sel.p, o_head);
  const unsigned grid = (unsigned)std::min<size_t>(tiles, (size_t)ctx->num_cus * 2);
  lattice_rank_kernel<<<grid, kSelTile, 0, st>>>(L, (unsigned long long)P, score, pairs, local_max, sorted, cnt, head);
  lattice_merge_kernel<<<1, kSelTile, 0, st>>>((unsigned long long)P, score, sorted, cnt, head, top_k, cand, n_cand);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(ctx, NDT_E_HIP, std::string("ndt_lattice_select_dev: ") + hipGetErrorString(e));
  return NDT_OK;
}

// ndt_relocalize / ndt_relocalize_dev: the scan is host memory (scan_host) or device memory (scan_dev).
int relocalize_impl(ndt_ctx *ctx, const ndt_map *map, const float *scan_host, const float *scan_dev, size_t n, size_t stride,
                    const ndt_reloc_params *prm, uint64_t *cand_index, double *cand_score, ndt_result *records, int *n_cand, int *best,
                    double *scores_host, const char *fn) {
  int rc = score_check(ctx, map, scan_host ? (const void *)scan_host : (const void *)scan_dev, n, stride, fn);
  if (rc) return rc;
  const std::string f(fn);
  if (!prm || !cand_index || !cand_score || !records || !n_cand || !best) return fail(ctx, NDT_E_ARG, f + ": NULL parameters or outputs");
  uint64_t P = 0;
  if (!lattice_count(&prm->lattice, &P)) return fail(ctx, NDT_E_ARG, f + ": bad lattice (a dimension below 1, a non-finite origin or step, or more than 2^31 - 1 poses)");
  const int K = prm->top_k;
  if (K < 1 || K > 1024) return fail(ctx, NDT_E_ARG, f + ": top_k must be in 1 .. 1024");
  const Lattice L = lattice_of(prm->lattice);
  CallFrame fr(ctx);
  if ((rc = fr.open())) return rc;
  hipStream_t st = fr.st;
  // the volume, the candidates, the guesses and the records: one grow-only allocation
  Regions R;
  const size_t o_score = R.take((size_t)P * 8, 256), o_pairs = R.take((size_t)P * 4, 256), o_cand = R.take((size_t)K * 8, 256),
               o_ncand = R.take(sizeof(int), 256), o_init = R.take((size_t)K * 24, 256), o_cscore = R.take((size_t)K * 8, 256),
               o_off = R.take(2 * 8, 256), o_res = R.take((size_t)K * sizeof(ndt_result), 256);
  if ((rc = ctx->d_rl.ensure(ctx, R.end))) return rc;
  unsigned char *base = ctx->d_rl.p;
  double *d_score = R.at<double>(base, o_score); unsigned *d_pairs = R.at<unsigned>(base, o_pairs);
  unsigned long long *d_cand = R.at<unsigned long long>(base, o_cand); int *d_ncand = R.at<int>(base, o_ncand);
  double *d_init = R.at<double>(base, o_init), *d_cscore = R.at<double>(base, o_cscore);
  unsigned long long *d_off = R.at<unsigned long long>(base, o_off); ndt_result *d_res = R.at<ndt_result>(base, o_res);
  // the scan, packed: what the match reads (the sweep reads the same copy)
  const float *scan = nullptr;
  if ((rc = stage_scan_f2(ctx, st, scan_host, scan_dev, n, stride, &scan))) return rc;
  const unsigned long long h_off[2] = {0ull, (unsigned long long)n};
  HIP_TRY(ctx, hipMemcpyAsync(d_off, h_off, sizeof(h_off), hipMemcpyHostToDevice, st));
  // sweep, pick, the candidates' poses -- then the call's one host wait before the match: how many there are
  if ((rc = queue_score(ctx, map, st, scan, n, 8, nullptr, L, P, d_score, d_pairs))) return rc;
  if ((rc = queue_select(ctx, st, L, P, d_score, d_pairs, K, prm->local_max, d_cand, d_ncand))) return rc;
  lattice_cand_kernel<<<(K + 255) / 256, 256, 0, st>>>(L, d_cand, d_ncand, K, d_score, d_init, d_cscore);
  HIP_TRY(ctx, hipGetLastError());
  int nc = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&nc, d_ncand, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  *n_cand = nc; *best = -1;
  if (nc > 0) {
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, st));
    if ((rc = launch_align(ctx, map, st, scan, d_off, nc, 1, n, d_init, d_res, nullptr, 0, nullptr, nullptr))) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, st));
    HIP_TRY(ctx, hipMemcpyAsync(records, d_res, (size_t)nc * sizeof(ndt_result), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(cand_index, d_cand, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(cand_score, d_cscore, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  }
  if (scores_host) HIP_TRY(ctx, hipMemcpyAsync(scores_host, d_score, (size_t)P * 8, hipMemcpyDeviceToHost, st));
  if ((rc = fr.close_and_wait())) return rc;
  if (nc > 0) HIP_TRY(ctx, hipEventElapsedTime(&ctx->align_ms, ctx->ev0, ctx->ev1));
  // the shim's cost (src/PoseEstimator.cpp:43-46): the fitness of a converged match, else 1e7; lowest first, ties to the lower index
  double best_cost = 0.0;
  for (int c = 0; c < nc; ++c) {
    const double cost = records[c].converged ? records[c].fitness : 1e7;
    if (*best < 0 || cost < best_cost) { *best = c; best_cost = cost; }
  }
  return NDT_OK;
}

}  // namespace

extern "C" {

int ndt_lattice_size(const ndt_pose_lattice *l, uint64_t *n_poses) {
  uint64_t n = 0;
  if (!n_poses || !lattice_count(l, &n))
    return fail(nullptr, NDT_E_ARG, "ndt_lattice_size: NULL pointer, a dimension below 1, a non-finite origin or step, or more than 2^31 - 1 poses");
  *n_poses = n;
  return NDT_OK;
}

int ndt_lattice_pose(const ndt_pose_lattice *l, uint64_t index, double pose_xyyaw[3]) {
#pragma clang fp contract(off)
  uint64_t n = 0;
  if (!pose_xyyaw || !lattice_count(l, &n) || index >= n) return fail(nullptr, NDT_E_ARG, "ndt_lattice_pose: NULL pointer, bad lattice or index out of range");
  const uint64_t row = index / (uint64_t)l->nx;
  const uint64_t i = index - row * (uint64_t)l->nx, k = row / (uint64_t)l->ny, j = row - k * (uint64_t)l->ny;
  // one rounded multiply, one rounded add: this IS the definition (lattice_pose on the device gives the same bits)
  const double mx = (double)i * l->step_x, my = (double)j * l->step_y, mk = (double)k * l->step_yaw;
  pose_xyyaw[0] = l->x0 + mx; pose_xyyaw[1] = l->y0 + my; pose_xyyaw[2] = l->yaw0 + mk;
  return NDT_OK;
}

int ndt_score_poses_dev(ndt_ctx *ctx, const ndt_map *map, const float *scan_xy_dev, size_t n, size_t stride, const double *poses_dev,
                        uint64_t P, double *score_dev, uint32_t *pairs_dev, void *stream) {
  int rc = score_check(ctx, map, scan_xy_dev, n, stride, "ndt_score_poses_dev");
  if (rc) return rc;
  if (!poses_dev || !score_dev) return fail(ctx, NDT_E_ARG, "ndt_score_poses_dev: NULL poses or score");
  if (P < 1 || P > (uint64_t)INT32_MAX) return fail(ctx, NDT_E_ARG, "ndt_score_poses_dev: need 1 <= P <= 2^31 - 1 poses");
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {   // (no scratch of its own: the bracket keeps the context's launches in order)
    return queue_score(ctx, map, st, scan_xy_dev, n, stride, poses_dev, Lattice{}, P, score_dev, pairs_dev);
  });
}

int ndt_score_lattice_dev(ndt_ctx *ctx, const ndt_map *map, const float *scan_xy_dev, size_t n, size_t stride,
                          const ndt_pose_lattice *lattice, double *score_dev, uint32_t *pairs_dev, void *stream) {
  int rc = score_check(ctx, map, scan_xy_dev, n, stride, "ndt_score_lattice_dev");
  if (rc) return rc;
  if (!score_dev) return fail(ctx, NDT_E_ARG, "ndt_score_lattice_dev: NULL score");
  uint64_t P = 0;
  if (!lattice_count(lattice, &P))
    return fail(ctx, NDT_E_ARG, "ndt_score_lattice_dev: bad lattice (NULL, a dimension below 1, a non-finite origin or step, or more than 2^31 - 1 poses)");
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {
    return queue_score(ctx, map, st, scan_xy_dev, n, stride, nullptr, lattice_of(*lattice), P, score_dev, pairs_dev);
  });
}

int ndt_score_poses(ndt_ctx *ctx, const ndt_map *map, const float *scan_xy_host, size_t n, size_t stride, const double *poses_host,
                    uint64_t P, double *score_host, uint32_t *pairs_host) {
  int rc = score_check(ctx, map, scan_xy_host, n, stride, "ndt_score_poses");
  if (rc) return rc;
  if (!poses_host || !score_host) return fail(ctx, NDT_E_ARG, "ndt_score_poses: NULL poses or score");
  if (P < 1 || P > (uint64_t)INT32_MAX) return fail(ctx, NDT_E_ARG, "ndt_score_poses: need 1 <= P <= 2^31 - 1 poses");
  CallFrame fr(ctx);
  if ((rc = fr.open())) return rc;
  hipStream_t st = fr.st;
  Regions R;
  const size_t o_poses = R.take((size_t)P * 24, 256), o_score = R.take((size_t)P * 8, 256), o_pairs = R.take((size_t)P * 4, 256);
  if ((rc = ctx->d_scan.ensure(ctx, n * stride))) return rc;
  if ((rc = ctx->d_rl.ensure(ctx, R.end))) return rc;
  double *d_poses = R.at<double>(ctx->d_rl.p, o_poses), *d_score = R.at<double>(ctx->d_rl.p, o_score);
  unsigned *d_pairs = R.at<unsigned>(ctx->d_rl.p, o_pairs);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_scan.p, scan_xy_host, n * stride, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d_poses, poses_host, (size_t)P * 24, hipMemcpyHostToDevice, st));
  if ((rc = queue_score(ctx, map, st, (const float *)ctx->d_scan.p, n, stride, d_poses, Lattice{}, P, d_score, d_pairs))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(score_host, d_score, (size_t)P * 8, hipMemcpyDeviceToHost, st));
  if (pairs_host) HIP_TRY(ctx, hipMemcpyAsync(pairs_host, d_pairs, (size_t)P * 4, hipMemcpyDeviceToHost, st));
  return fr.close_and_wait();
}

int ndt_lattice_select_dev(ndt_ctx *ctx, const ndt_pose_lattice *lattice, const double *score_dev, const uint32_t *pairs_dev, int top_k,
                           int local_max, uint64_t *cand_index_dev, int *n_cand_dev, void *stream) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!score_dev || !pairs_dev || !cand_index_dev || !n_cand_dev) return fail(ctx, NDT_E_ARG, "ndt_lattice_select_dev: NULL array");
  uint64_t P = 0;
  if (!lattice_count(lattice, &P))
    return fail(ctx, NDT_E_ARG, "ndt_lattice_select_dev: bad lattice (NULL, a dimension below 1, a non-finite origin or step, or more than 2^31 - 1 poses)");
  if (top_k < 1 || top_k > 1024) return fail(ctx, NDT_E_ARG, "ndt_lattice_select_dev: top_k must be in 1 .. 1024");
  if (ctx->pending_map) return refuse_pending(ctx, "ndt_lattice_select_dev");
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {
    return queue_select(ctx, st, lattice_of(*lattice), P, score_dev, pairs_dev, top_k, local_max, (unsigned long long *)cand_index_dev, n_cand_dev);
  });
}

int ndt_relocalize(ndt_ctx *ctx, const ndt_map *map, const float *scan_xy_host, size_t n, size_t stride, const ndt_reloc_params *prm,
                   uint64_t *cand_index, double *cand_score, ndt_result *records, int *n_cand, int *best, double *scores_host) {
  return relocalize_impl(ctx, map, scan_xy_host, nullptr, n, stride, prm, cand_index, cand_score, records, n_cand, best, scores_host,
                         "ndt_relocalize");
}

int ndt_relocalize_dev(ndt_ctx *ctx, const ndt_map *map, const float *scan_xy_dev, size_t n, size_t stride, const ndt_reloc_params *prm,
                       uint64_t *cand_index, double *cand_score, ndt_result *records, int *n_cand, int *best, double *scores_host) {
  return relocalize_impl(ctx, map, nullptr, scan_xy_dev, n, stride, prm, cand_index, cand_score, records, n_cand, best, scores_host,
                         "ndt_relocalize_dev");
}

}  // extern "C"

// ---- ndt_fit_points_batch_dev / ndt_fit_points_batch: per-point nearest distances and the ranged fitness ----

namespace {

// The refusals both forms start with (synchronous, nothing queued or written).
int fit_points_check(ndt_ctx *ctx, const ndt_map *map, const void *scans, const void *offsets, int B, const void *tf,
                     size_t tf_stride, double max_d2, const void *d2, const void *stats, const char *fn) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  const std::string f(fn);
  if (!map || !scans || !offsets || !tf) return fail(ctx, NDT_E_ARG, f + ": NULL map, scans, offsets or tf");
  if (!d2 && !stats) return fail(ctx, NDT_E_ARG, f + ": d2 and stats are both NULL");
  if (B < 1) return fail(ctx, NDT_E_ARG, f + ": need B >= 1");
  if (!map->ctx || !map->view.cent) return fail(ctx, NDT_E_ARG, f + ": the map was never built");
  if (map->device != ctx->device) return fail(ctx, NDT_E_ARG, f + ": the map was built on another device");
  if (tf_stride < 16 || (tf_stride & 3)) return fail(ctx, NDT_E_ARG, f + ": bad tf_stride_bytes (need >= 16 and % 4 == 0)");
  if (!(max_d2 >= 0.0)) return fail(ctx, NDT_E_ARG, f + ": max_d2 is NaN or negative");
  if (ctx->pending_map) return refuse_pending(ctx, f);
  return NDT_OK;
}

// The two kernels on st, inside the caller's frame (d_fit_pts): they read the map (MapRead), entered the way the score sweep
// is (queue_score).  The ring's first two events ride on the search kernel's dispatch.
// mm (ndt_fit_points_multi_dev): match b reads mm->maps[map_of[b]]; `map` is then mm->maps[0], whose transform_sse every map
// has (fit_points_multi_check).  The views as they are now go up once, staged in pinned memory, into a table of the call's
// own (ndt_ctx::d_fp_views / fpv_tab -- not views_tab, which lives in a match launch's workspace): the scratch bracket
// orders the copy behind the previous call's kernels, reserve() waits for the previous call's copy.
int queue_fit_points(ndt_ctx *ctx, const ndt_map *map, hipStream_t st, const float *scans, const unsigned long long *offsets, int B,
                     size_t total_points, int shared_scan, const void *tf, size_t tf_stride, double max_d2, float *d2,
                     ndt_fit_stats *stats, const MultiMaps *mm = nullptr) {
  int rc;
  if (stats && (rc = ctx->d_fit_pts.ensure(ctx, fit_parts_needed(total_points, (size_t)B, shared_scan)))) return rc;   // (the call's one allocation, in front of its first kernel)
  if (mm && ((rc = ctx->d_fp_views.ensure(ctx, (size_t)mm->n_maps)) || (rc = ctx->fpv_tab.reserve(ctx, (size_t)mm->n_maps)))) return rc;
  const ndt_map *const *maps = mm ? mm->distinct.data() : &map;
  const int n_read = mm ? (int)mm->distinct.size() : 1;
  MapRead rd{ctx, st, maps, n_read};
  if ((rc = rd.begin())) return rc;
  if (mm) {
    for (int i = 0; i < mm->n_maps; ++i) ctx->fpv_tab.h.p[i] = mm->maps[i]->view;
    HIP_TRY(ctx, ctx->fpv_tab.upload(ctx->d_fp_views.p, 0, (size_t)mm->n_maps, st));
  }
  const MapView *views = mm ? ctx->d_fp_views.p : nullptr;
  const int *map_of = mm ? mm->map_of : nullptr; const int n_maps = mm ? mm->n_maps : 0;
  const FitGrid G = fit_grid(total_points, B, shared_scan, ctx->workgroups);     // (queue_fitness's grid; NDT_OPT_WORKGROUPS bounds it)
  FitPtsPart *parts = stats ? ctx->d_fit_pts.p : nullptr;
  Event *evr = rd.ev;
  with_bool(map->prm.transform_sse != 0, [&](auto S) { with_bool(mm != nullptr, [&](auto M) {
    hipExtLaunchKernelGGL((fit_points_kernel<decltype(S)::value, decltype(M)::value>), dim3(G.workgroups), dim3(256), 0, st, evr[0], evr[1], 0,
                          map->view, reinterpret_cast<const float2 *>(scans), offsets, B, shared_scan, (const unsigned char *)tf, tf_stride,
                          max_d2, d2, parts, (int)G.gx, views, map_of, n_maps);
  }); });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(ctx, NDT_E_HIP, std::string("ndt_fit_points: ") + hipGetErrorString(e));
  if (stats) {
    fit_points_close_kernel<<<dim3((unsigned)(((size_t)B + 3) / 4)), dim3(256), 0, st>>>(offsets, B, shared_scan, parts, stats);
    e = hipGetLastError();
  }
  return rd.entered(e != hipSuccess ? fail(ctx, NDT_E_HIP, std::string("ndt_fit_points: ") + hipGetErrorString(e)) : NDT_OK,
                    /*end_carried=*/false,
                    /*deferred=*/std::any_of(maps, maps + n_read, [&](const ndt_map *m) { return st != m->ctx->stream; }), "ndt_fit_points");
}

// The refusals of the multi-map forms: the maps first (the text names the first offending one), then those of the single-map
// call, then what ties the maps to the matches and to one kernel instance.  Fills mm on success (map_of is the caller's to set).
int fit_points_multi_check(ndt_ctx *ctx, const ndt_map *const *maps, int n_maps, bool have_map_of, const void *scans, const void *offsets,
                           int B, const void *tf, size_t tf_stride, double max_d2, const void *d2, const void *stats, const char *fn,
                           MultiMaps *mm) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  const std::string f(fn);
  if (!maps || n_maps < 1) return fail(ctx, NDT_E_ARG, f + ": no maps (maps == NULL or n_maps < 1)");
  for (int i = 0; i < n_maps; ++i) {
    const ndt_map *m = maps[i];
    const std::string which = f + ": map " + std::to_string(i);
    if (!m) return fail(ctx, NDT_E_ARG, which + " is NULL");
    if (!m->ctx || !m->view.cent) return fail(ctx, NDT_E_ARG, which + " was never built");
    if (m->device != ctx->device) return fail(ctx, NDT_E_ARG, which + " was built on another device");
  }
  const int rc = fit_points_check(ctx, maps[0], scans, offsets, B, tf, tf_stride, max_d2, d2, stats, fn);
  if (rc) return rc;
  if (!have_map_of && n_maps != B) return fail(ctx, NDT_E_ARG, f + ": map_of == NULL needs n_maps == B");
  for (int i = 1; i < n_maps; ++i)
    if ((maps[i]->prm.transform_sse != 0) != (maps[0]->prm.transform_sse != 0))
      return fail(ctx, NDT_E_ARG, f + ": map " + std::to_string(i) + " has another transform_sse than map 0 (the kernel instance depends on it)");
  mm->maps = maps; mm->n_maps = n_maps; mm->map_of = nullptr;
  mm->distinct.assign(maps, maps + n_maps);
  std::sort(mm->distinct.begin(), mm->distinct.end());
  mm->distinct.erase(std::unique(mm->distinct.begin(), mm->distinct.end()), mm->distinct.end());
  return NDT_OK;
}

// The host forms behind their refusals: one upload (the offsets, the transforms packed to 16 bytes each, the multi-map form's
// map_of and the scans, staged in pinned memory), the two kernels, the read-backs, one wait.
int fit_points_host(ndt_ctx *ctx, const ndt_map *map, MultiMaps *mm, const int *map_of_host, const float *scans_xy_host,
                    const uint64_t *offsets_host, int B, int shared_scan, const float *tf_host, size_t tf_stride_bytes, double max_d2,
                    float *d2_host, ndt_fit_stats *stats_host, const char *fn) {
  int rc;
  const size_t nscan = shared_scan ? 1 : (size_t)B;
  for (size_t b = 0; b < nscan; ++b)
    if (offsets_host[b + 1] < offsets_host[b]) return fail(ctx, NDT_E_ARG, std::string(fn) + ": offsets not monotone");
  const size_t ntot = (size_t)offsets_host[nscan];
  const size_t n_d2 = shared_scan ? (size_t)B * (size_t)(offsets_host[1] - offsets_host[0]) : ntot;
  CallFrame fr(ctx);
  if ((rc = fr.open())) return rc;
  hipStream_t st = fr.st;
  Regions U;
  U.take((nscan + 1) * 8, 256);
  const size_t o_tf = U.take((size_t)B * 16, 256), o_mapof = map_of_host ? U.take((size_t)B * sizeof(int), 256) : 0,
               o_scan = U.take(ntot * 8, 256), bytes = U.end;
  if ((rc = ctx->fp_tab.reserve(ctx, bytes))) return rc;
  if ((rc = ctx->d_scan.ensure(ctx, bytes))) return rc;
  if (d2_host && (rc = ctx->d_fit.ensure(ctx, n_d2 + 4))) return rc;
  if (stats_host && (rc = ctx->d_tmp.ensure(ctx, (size_t)B * sizeof(ndt_fit_stats)))) return rc;
  unsigned char *h = ctx->fp_tab.h.p, *d = ctx->d_scan.p;
  memcpy(h, offsets_host, (nscan + 1) * 8);
  for (int b = 0; b < B; ++b) memcpy(h + o_tf + (size_t)b * 16, (const unsigned char *)tf_host + (size_t)b * tf_stride_bytes, 16);
  if (map_of_host) memcpy(h + o_mapof, map_of_host, (size_t)B * sizeof(int));
  if (ntot) memcpy(h + o_scan, scans_xy_host, ntot * 8);
  HIP_TRY(ctx, ctx->fp_tab.upload(d, 0, bytes, st));
  if (mm) mm->map_of = map_of_host ? (const int *)(d + o_mapof) : nullptr;
  float *d_d2 = d2_host ? ctx->d_fit.p : nullptr;
  ndt_fit_stats *d_stats = stats_host ? (ndt_fit_stats *)ctx->d_tmp.p : nullptr;
  if ((rc = queue_fit_points(ctx, map, st, (const float *)(d + o_scan), (const unsigned long long *)d, B, ntot, shared_scan, d + o_tf, 16,
                             max_d2, d_d2, d_stats, mm)))
    return rc;
  if (d2_host && n_d2) HIP_TRY(ctx, hipMemcpyAsync(d2_host, d_d2, n_d2 * sizeof(float), hipMemcpyDeviceToHost, st));
  if (stats_host) HIP_TRY(ctx, hipMemcpyAsync(stats_host, d_stats, (size_t)B * sizeof(ndt_fit_stats), hipMemcpyDeviceToHost, st));
  return fr.close_and_wait();
}

}  // namespace

extern "C" {

int ndt_fit_points_batch_dev(ndt_ctx *ctx, const ndt_map *map, const float *scans_xy_dev, const uint64_t *offsets_dev, int B,
                             size_t total_points, int shared_scan, const float *tf_dev, size_t tf_stride_bytes, double max_d2,
                             float *d2_dev, ndt_fit_stats *stats_dev, void *stream) {
  int rc = fit_points_check(ctx, map, scans_xy_dev, offsets_dev, B, tf_dev, tf_stride_bytes, max_d2, d2_dev, stats_dev, "ndt_fit_points_batch_dev");
  if (rc) return rc;
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {
    return queue_fit_points(ctx, map, st, scans_xy_dev, (const unsigned long long *)offsets_dev, B, total_points, shared_scan, tf_dev,
                             tf_stride_bytes, max_d2, d2_dev, stats_dev);
  });
}

int ndt_fit_points_batch(ndt_ctx *ctx, const ndt_map *map, const float *scans_xy_host, const uint64_t *offsets_host, int B,
                         int shared_scan, const float *tf_host, size_t tf_stride_bytes, double max_d2, float *d2_host,
                         ndt_fit_stats *stats_host) {
  int rc = fit_points_check(ctx, map, scans_xy_host, offsets_host, B, tf_host, tf_stride_bytes, max_d2, d2_host, stats_host, "ndt_fit_points_batch");
  if (rc) return rc;
  return fit_points_host(ctx, map, nullptr, nullptr, scans_xy_host, offsets_host, B, shared_scan, tf_host, tf_stride_bytes, max_d2, d2_host,
                         stats_host, "ndt_fit_points_batch");
}

int ndt_fit_points_multi_dev(ndt_ctx *ctx, const ndt_map *const *maps, int n_maps, const int *map_of_dev, const float *scans_xy_dev,
                             const uint64_t *offsets_dev, int B, size_t total_points, int shared_scan, const float *tf_dev,
                             size_t tf_stride_bytes, double max_d2, float *d2_dev, ndt_fit_stats *stats_dev, void *stream) {
  MultiMaps mm;
  int rc = fit_points_multi_check(ctx, maps, n_maps, map_of_dev != nullptr, scans_xy_dev, offsets_dev, B, tf_dev, tf_stride_bytes, max_d2,
                                  d2_dev, stats_dev, "ndt_fit_points_multi_dev", &mm);
  if (rc) return rc;
  mm.map_of = map_of_dev;
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {
    return queue_fit_points(ctx, maps[0], st, scans_xy_dev, (const unsigned long long *)offsets_dev, B, total_points, shared_scan, tf_dev,
                             tf_stride_bytes, max_d2, d2_dev, stats_dev, &mm);
  });
}

int ndt_fit_points_multi(ndt_ctx *ctx, const ndt_map *const *maps, int n_maps, const int *map_of_host, const float *scans_xy_host,
                         const uint64_t *offsets_host, int B, int shared_scan, const float *tf_host, size_t tf_stride_bytes,
                         double max_d2, float *d2_host, ndt_fit_stats *stats_host) {
  MultiMaps mm;
  int rc = fit_points_multi_check(ctx, maps, n_maps, map_of_host != nullptr, scans_xy_host, offsets_host, B, tf_host, tf_stride_bytes, max_d2,
                                  d2_host, stats_host, "ndt_fit_points_multi", &mm);
  if (rc) return rc;
  return fit_points_host(ctx, maps[0], &mm, map_of_host, scans_xy_host, offsets_host, B, shared_scan, tf_host, tf_stride_bytes, max_d2,
                         d2_host, stats_host, "ndt_fit_points_multi");
}

}  // extern "C"

// ---- ndt_occ_*: occupancy grids of {hit, pass} counters, ray-cast from scans (kernels in ndt_occupancy.hip.h) ----

struct ndt_occ {
  ndt_ctx *ctx = nullptr;
  int device = 0;
  ndt_occ_geometry g{};
  size_t n_cells = 0;
  DevBuf<unsigned> cells;                     // 2 * n_cells: {hit, pass} per cell
  // the last call that wrote the grid: its number among the context's writers (ndt_ctx::occ_ev) and its stream
  bool written = false;
  unsigned long long wseq = 0;
  hipStream_t wstream = nullptr;
};

namespace {

int occ_geometry_check(ndt_ctx *ctx, const ndt_occ_geometry *g, const char *fn) {
  const std::string f(fn);
  if (!g) return fail(ctx, NDT_E_ARG, f + ": NULL geometry");
  if (!(g->res > 0.0) || !std::isfinite(g->res)) return fail(ctx, NDT_E_ARG, f + ": res is not positive and finite");
  if (!std::isfinite(g->x0) || !std::isfinite(g->y0)) return fail(ctx, NDT_E_ARG, f + ": the origin is not finite");
  if (g->nx < 1 || g->ny < 1) return fail(ctx, NDT_E_ARG, f + ": nx or ny below 1");
  if ((uint64_t)g->nx * (uint64_t)g->ny > ((uint64_t)1 << 28)) return fail(ctx, NDT_E_GRID, f + ": more than 2^28 cells");
  return NDT_OK;
}

// The event of the context's writer number k.  A writer that has left the ring is covered by the latest one: every writer
// opens the scratch bracket, so each is ordered behind the one before it, on whatever stream.
hipEvent_t occ_event_of(ndt_ctx *ctx, unsigned long long k) {
  const unsigned long long last = ctx->occ_seq - 1;
  return ctx->occ_ev[(last - k >= (unsigned long long)ndt_ctx::kOccEv ? last : k) % ndt_ctx::kOccEv];
}

// A call on st is about to touch the grid: behind the grid's last writer, if that was on another stream.
int occ_touch(ndt_ctx *ctx, const ndt_occ *o, hipStream_t st) {
  if (o->written && o->wstream != st) HIP_TRY(ctx, hipStreamWaitEvent(st, occ_event_of(ctx, o->wseq), 0));
  return NDT_OK;
}

// The call on st has queued its writes of occs[0 .. n) (NULL entries: not written): one event for all of them.
int occ_wrote(ndt_ctx *ctx, ndt_occ *const *occs, int n, hipStream_t st) {
  Event &ev = ctx->occ_ev[ctx->occ_seq % ndt_ctx::kOccEv];
  if (!ev) { const int rc = ev.create(ctx, hipEventDisableTiming); if (rc) return rc; }
  HIP_TRY(ctx, hipEventRecord(ev, st));
  for (int i = 0; i < n; ++i)
    if (occs[i]) { occs[i]->written = true; occs[i]->wseq = ctx->occ_seq; occs[i]->wstream = st; }
  ctx->occ_seq++;
  return NDT_OK;
}

// One call's beams: the batch forms (xy, offsets, grid_of: device arrays; rows = the grids) or the sessions form (xy ==
// nullptr: row b is scan b and its grid).
struct OccCall {
  ndt_occ *const *occs; int n_rows;           // NULL entries (sessions form): rows not taken
  const OccRow *own;                          // sessions form: pts / n per row (host), else nullptr
  const int *grid_of; const float *xy; const unsigned long long *offsets; int B; size_t total_points;
  const void *origins; size_t origin_stride; double max_range2; ndt_occ_stats *stats;
};

// The table's upload and the two kernels on st, inside the caller's frame (d_occ); the grids are entered as written.
int queue_occ(ndt_ctx *ctx, hipStream_t st, const OccCall &C) {
  int rc;
  const size_t job_cap = std::min<size_t>(C.total_points / (size_t)kOccRun + (size_t)C.B, (size_t)UINT32_MAX);
  Regions R;
  const size_t o_tab = R.take((size_t)C.n_rows * sizeof(OccRow)), o_nj = R.take(256), o_jobs = R.take(job_cap * sizeof(OccJob));
  if ((rc = ctx->occ_tab.reserve(ctx, (size_t)C.n_rows * sizeof(OccRow)))) return rc;      // (waits for the previous call's copy)
  if ((rc = ctx->d_occ.ensure(ctx, R.end))) return rc;
  for (int i = 0; i < C.n_rows; ++i)
    if (C.occs[i] && (rc = occ_touch(ctx, C.occs[i], st))) return rc;
  OccRow *h = reinterpret_cast<OccRow *>(ctx->occ_tab.h.p);
  for (int i = 0; i < C.n_rows; ++i) {
    OccRow r{};
    if (C.occs[i]) {
      const ndt_occ &o = *C.occs[i];
      r.cells = o.cells.p; r.x0 = o.g.x0; r.y0 = o.g.y0; r.res = o.g.res; r.nx = o.g.nx; r.ny = o.g.ny;
      if (C.own) { r.pts = C.own[i].pts; r.n = C.own[i].n; }
    }
    h[i] = r;
  }
  unsigned char *d = ctx->d_occ.p;
  HIP_TRY(ctx, ctx->occ_tab.upload(d + o_tab, 0, (size_t)C.n_rows * sizeof(OccRow), st));
  const OccRow *tab = reinterpret_cast<const OccRow *>(d + o_tab);
  OccJob *jobs = reinterpret_cast<OccJob *>(d + o_jobs);
  unsigned *nj = reinterpret_cast<unsigned *>(d + o_nj);
  unsigned long long *stats = reinterpret_cast<unsigned long long *>(C.stats);
  occ_jobs_kernel<<<1, 256, 0, st>>>(tab, C.offsets, C.B, jobs, (unsigned)job_cap, nj, stats);
  // as many workgroups as there can be runs, eight per CU at most (or NDT_OPT_WORKGROUPS): each takes runs in turn
  const size_t wgs = std::max<size_t>(1, std::min<size_t>(job_cap, ctx->workgroups > 0 ? (size_t)ctx->workgroups : (size_t)ctx->num_cus * 8));
  occ_integrate_kernel<<<dim3((unsigned)wgs), dim3(kOccRun), 0, st>>>(tab, C.n_rows, C.grid_of, reinterpret_cast<const float2 *>(C.xy), C.offsets,
                                                                       (const unsigned char *)C.origins, C.origin_stride, C.max_range2, jobs, nj, stats);
  const hipError_t e = hipGetLastError();
  // the kernels are queued (or not): either way the grids count as written behind this point of st
  rc = occ_wrote(ctx, C.occs, C.n_rows, st);
  if (e != hipSuccess) return fail(ctx, NDT_E_HIP, std::string("ndt_occ_integrate: ") + hipGetErrorString(e));
  return rc;
}

// The refusals both batch forms start with (synchronous, nothing queued or written).
int occ_integrate_check(ndt_ctx *ctx, ndt_occ *const *occs, int n_occ, const void *xy, const void *offsets, int B, const void *origins,
                        size_t origin_stride, double max_range2, const char *fn) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  const std::string f(fn);
  if (!occs || !xy || !offsets || !origins) return fail(ctx, NDT_E_ARG, f + ": NULL array (occs, xy, offsets or origins)");
  if (n_occ < 1 || B < 1) return fail(ctx, NDT_E_ARG, f + ": need n_occ >= 1 and B >= 1");
  for (int i = 0; i < n_occ; ++i) {
    if (!occs[i]) return fail(ctx, NDT_E_ARG, f + ": grid " + std::to_string(i) + " is NULL");
    if (occs[i]->ctx != ctx || occs[i]->device != ctx->device) return fail(ctx, NDT_E_ARG, f + ": grid " + std::to_string(i) + " belongs to another context");
    for (int k = 0; k < i; ++k)
      if (occs[k] == occs[i]) return fail(ctx, NDT_E_ARG, f + ": grid " + std::to_string(i) + " is given twice (also as grid " + std::to_string(k) + ")");
  }
  if (origin_stride < 16 || (origin_stride & 7)) return fail(ctx, NDT_E_ARG, f + ": bad origin_stride_bytes (need >= 16 and % 8 == 0)");
  if (!(max_range2 >= 0.0)) return fail(ctx, NDT_E_ARG, f + ": max_range2 is NaN or negative");
  if (ctx->pending_map) return refuse_pending(ctx, f);
  return NDT_OK;
}

// ... and those of the calls on one grid
int occ_one_check(ndt_ctx *ctx, const ndt_occ *occ, const char *fn) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  const std::string f(fn);
  if (!occ) return fail(ctx, NDT_E_ARG, f + ": NULL grid");
  if (occ->ctx != ctx || occ->device != ctx->device) return fail(ctx, NDT_E_ARG, f + ": the grid belongs to another context");
  if (ctx->pending_map) return refuse_pending(ctx, f);
  return NDT_OK;
}

int queue_occ_render(ndt_ctx *ctx, const ndt_occ *occ, unsigned min_obs, signed char *out, hipStream_t st) {
  int rc = occ_touch(ctx, occ, st);
  if (rc) return rc;
  occ_render_kernel<<<dim3((unsigned)grid_for(occ->n_cells, 256, ctx->num_cus * 8)), dim3(256), 0, st>>>(
      reinterpret_cast<const uint2 *>(occ->cells.p), occ->n_cells, min_obs, out);
  HIP_TRY(ctx, hipGetLastError());
  return NDT_OK;
}

}  // namespace

extern "C" {

int ndt_occ_cell(const ndt_occ_geometry *g, double x, double y, int64_t *ix, int64_t *iy) {
  const int rc = occ_geometry_check(nullptr, g, "ndt_occ_cell");
  if (rc) return rc;
  if (!ix || !iy) return fail(nullptr, NDT_E_ARG, "ndt_occ_cell: NULL output");
  if (!std::isfinite(x) || !std::isfinite(y)) return fail(nullptr, NDT_E_ARG, "ndt_occ_cell: a coordinate is not finite");
  const double lim = 4611686018427387904.0;      // 2^62
  const double fx = occ_axis(x, g->x0, g->res), fy = occ_axis(y, g->y0, g->res);
  *ix = (int64_t)std::max(-lim, std::min(lim, fx));
  *iy = (int64_t)std::max(-lim, std::min(lim, fy));
  return NDT_OK;
}

int ndt_occ_create(ndt_ctx *ctx, const ndt_occ_geometry *g, ndt_occ **out) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  if (!out) return fail(ctx, NDT_E_ARG, "ndt_occ_create: NULL out");
  int rc = occ_geometry_check(ctx, g, "ndt_occ_create");
  if (rc) return rc;
  if (ctx->pending_map) return refuse_pending(ctx, "ndt_occ_create");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ndt_occ *o = new (std::nothrow) ndt_occ;
  if (!o) return fail(ctx, NDT_E_NOMEM, "ndt_occ_create: out of memory");
  o->ctx = ctx; o->device = ctx->device; o->g = *g; o->n_cells = (size_t)g->nx * (size_t)g->ny;
  if ((rc = o->cells.alloc(ctx, o->n_cells * 2 * sizeof(unsigned)))) { delete o; return rc; }
  hipError_t e = hipMemsetAsync(o->cells.p, 0, o->cells.bytes, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { delete o; return fail(ctx, NDT_E_HIP, std::string("ndt_occ_create: ") + hipGetErrorString(e)); }
  *out = o;
  return NDT_OK;
}

int ndt_occ_destroy(ndt_occ *o) {
  if (!o) return NDT_E_ARG;
  bool ctx_live;
  { std::lock_guard<std::mutex> lk(g_live_mu); ctx_live = g_live_ctx.count(o->ctx) != 0; }
  hipError_t e = hipSetDevice(o->device);
  if (ctx_live) {                               // (a context destroyed first has drained its streams: ndt_map_destroy's rule)
    e = hipStreamSynchronize(o->ctx->stream);
    if (o->written) e = hipEventSynchronize(occ_event_of(o->ctx, o->wseq));      // (the last writer may have been on another stream)
  }
  (void)e;
  delete o;
  return NDT_OK;
}

int ndt_occ_geometry_get(const ndt_occ *o, ndt_occ_geometry *out) {
  if (!o || !out) return fail(o ? o->ctx : nullptr, NDT_E_ARG, "ndt_occ_geometry_get: NULL argument");
  *out = o->g;
  return NDT_OK;
}

int ndt_occ_view(const ndt_occ *o, const uint32_t **cells_dev) {
  if (!o || !cells_dev) return fail(o ? o->ctx : nullptr, NDT_E_ARG, "ndt_occ_view: NULL argument");
  *cells_dev = o->cells.p;
  return NDT_OK;
}

int ndt_occ_clear(ndt_ctx *ctx, ndt_occ *occ, void *stream) {
  int rc = occ_one_check(ctx, occ, "ndt_occ_clear");
  if (rc) return rc;
  CallFrame fr(ctx);   // (no scratch: the bracket orders the call among the context's)
  if ((rc = fr.open(stream))) return rc;
  hipStream_t st = fr.st;
  if ((rc = occ_touch(ctx, occ, st))) return rc;
  HIP_TRY(ctx, hipMemsetAsync(occ->cells.p, 0, occ->cells.bytes, st));
  if ((rc = occ_wrote(ctx, &occ, 1, st))) return rc;
  return fr.close();
}

int ndt_occ_integrate_dev(ndt_ctx *ctx, ndt_occ *const *occs, int n_occ, const int *grid_of_dev, const float *xy_dev,
                          const uint64_t *offsets_dev, int B, size_t total_points, const double *origins_dev,
                          size_t origin_stride_bytes, double max_range2, ndt_occ_stats *stats_dev, void *stream) {
  int rc = occ_integrate_check(ctx, occs, n_occ, xy_dev, offsets_dev, B, origins_dev, origin_stride_bytes, max_range2, "ndt_occ_integrate_dev");
  if (rc) return rc;
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {
    return queue_occ(ctx, st, OccCall{occs, n_occ, nullptr, grid_of_dev, xy_dev, (const unsigned long long *)offsets_dev, B, total_points,
                                       origins_dev, origin_stride_bytes, max_range2, stats_dev});
  });
}

int ndt_occ_integrate(ndt_ctx *ctx, ndt_occ *const *occs, int n_occ, const int *grid_of_host, const float *xy_host,
                      const uint64_t *offsets_host, int B, const double *origins_host, size_t origin_stride_bytes,
                      double max_range2, ndt_occ_stats *stats_host) {
  int rc = occ_integrate_check(ctx, occs, n_occ, xy_host, offsets_host, B, origins_host, origin_stride_bytes, max_range2, "ndt_occ_integrate");
  if (rc) return rc;
  for (int b = 0; b < B; ++b)
    if (offsets_host[b + 1] < offsets_host[b]) return fail(ctx, NDT_E_ARG, "ndt_occ_integrate: scan " + std::to_string(b) + ": offsets decrease");
  const size_t first = (size_t)offsets_host[0], ntot = (size_t)(offsets_host[B] - offsets_host[0]);
  CallFrame fr(ctx);
  if ((rc = fr.open())) return rc;
  hipStream_t st = fr.st;
  // one upload: the offsets (relative), grid_of, the origins (packed: 16 bytes each) and the scans, staged in pinned memory
  Regions U;
  const size_t o_off = U.take(((size_t)B + 1) * 8), o_gof = U.take(grid_of_host ? (size_t)B * 4 : 0), o_org = U.take((size_t)B * 16),
               o_xy = U.take(ntot * 8);
  if ((rc = ctx->occ_up.reserve(ctx, U.end))) return rc;
  if ((rc = ctx->d_scan.ensure(ctx, U.end))) return rc;
  if (stats_host && (rc = ctx->d_tmp.ensure(ctx, sizeof(ndt_occ_stats)))) return rc;
  unsigned char *h = ctx->occ_up.h.p, *d = ctx->d_scan.p;
  rel_offsets(offsets_host, (size_t)B, U.at<uint64_t>(h, o_off));
  if (grid_of_host) memcpy(h + o_gof, grid_of_host, (size_t)B * 4);
  for (int b = 0; b < B; ++b) memcpy(h + o_org + (size_t)b * 16, (const unsigned char *)origins_host + (size_t)b * origin_stride_bytes, 16);
  if (ntot) memcpy(h + o_xy, xy_host + 2 * first, ntot * 8);
  HIP_TRY(ctx, ctx->occ_up.upload(d, 0, U.end, st));
  ndt_occ_stats *d_stats = stats_host ? (ndt_occ_stats *)ctx->d_tmp.p : nullptr;
  if ((rc = queue_occ(ctx, st, OccCall{occs, n_occ, nullptr, grid_of_host ? (const int *)(d + o_gof) : nullptr, (const float *)(d + o_xy),
                                       (const unsigned long long *)(d + o_off), B, ntot, d + o_org, 16, max_range2, d_stats})))
    return rc;
  if (stats_host) HIP_TRY(ctx, hipMemcpyAsync(stats_host, d_stats, sizeof(ndt_occ_stats), hipMemcpyDeviceToHost, st));
  return fr.close_and_wait();
}

int ndt_occ_render_dev(ndt_ctx *ctx, ndt_occ *occ, uint32_t min_obs, int8_t *out_dev, void *stream) {
  int rc = occ_one_check(ctx, occ, "ndt_occ_render_dev");
  if (rc) return rc;
  if (!out_dev) return fail(ctx, NDT_E_ARG, "ndt_occ_render_dev: NULL out");
  if (min_obs < 1) return fail(ctx, NDT_E_ARG, "ndt_occ_render_dev: min_obs below 1");
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {   // (no scratch: the bracket orders the call among the context's)
    return queue_occ_render(ctx, occ, min_obs, (signed char *)out_dev, st);
  });
}

int ndt_occ_render(ndt_ctx *ctx, ndt_occ *occ, uint32_t min_obs, int8_t *out_host) {
  int rc = occ_one_check(ctx, occ, "ndt_occ_render");
  if (rc) return rc;
  if (!out_host) return fail(ctx, NDT_E_ARG, "ndt_occ_render: NULL out");
  if (min_obs < 1) return fail(ctx, NDT_E_ARG, "ndt_occ_render: min_obs below 1");
  CallFrame fr(ctx);
  if ((rc = fr.open())) return rc;
  hipStream_t st = fr.st;
  if ((rc = ctx->d_tmp.ensure(ctx, occ->n_cells))) return rc;
  if ((rc = queue_occ_render(ctx, occ, min_obs, (signed char *)ctx->d_tmp.p, st))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(out_host, ctx->d_tmp.p, occ->n_cells, hipMemcpyDeviceToHost, st));
  return fr.close_and_wait();
}

int ndt_occ_counts(ndt_ctx *ctx, ndt_occ *occ, uint32_t *hit_host, uint32_t *pass_host) {
  int rc = occ_one_check(ctx, occ, "ndt_occ_counts");
  if (rc) return rc;
  if (!hit_host && !pass_host) return fail(ctx, NDT_E_ARG, "ndt_occ_counts: hit and pass are both NULL");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  std::vector<uint32_t> both;
  try { both.resize(occ->n_cells * 2); } catch (const std::bad_alloc &) { return fail(ctx, NDT_E_NOMEM, "ndt_occ_counts: out of memory"); }
  if ((rc = occ_touch(ctx, occ, st))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(both.data(), occ->cells.p, both.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  for (size_t i = 0; i < occ->n_cells; ++i) {
    if (hit_host) hit_host[i] = both[2 * i];
    if (pass_host) pass_host[i] = both[2 * i + 1];
  }
  return NDT_OK;
}

// Session i's grid, to a call that takes it: NULL, another context's, given twice (seen: the grids taken so far).
static int check_grid(const SetCall &call, ndt_occ *const *occs, int i, std::set<const ndt_occ *> &seen) {
  const std::string who = "session " + std::to_string(i);
  if (!occs[i]) return call.refuse(who + ": NULL grid");
  if (occs[i]->ctx != call.ctx || occs[i]->device != call.ctx->device) return call.refuse(who + ": the grid belongs to another context");
  if (!seen.insert(occs[i]).second) return call.refuse(who + ": its grid is given twice");
  return NDT_OK;
}

int ndt_sessions_occ_integrate(ndt_sessions *s, ndt_occ *const *occs, const unsigned char *which, double max_range2,
                               ndt_occ_stats *stats_host) {
  SetCall call{s, "ndt_sessions_occ_integrate", false};
  int rc = call.enter();
  if (rc) return rc;
  ndt_ctx *ctx = call.ctx;
  if (!occs) return call.refuse("NULL occs");
  if (!(max_range2 >= 0.0)) return call.refuse("max_range2 is NaN or negative");
  return call.run([&]() -> int {      // who is taken: the newest scan is the last range of scan_off in store[cur]
    const int S = s->S;
    std::vector<ndt_occ *> taken((size_t)S, nullptr);
    std::vector<OccRow> own((size_t)S);
    std::set<const ndt_occ *> seen;
    size_t total = 0;
    for (int i = 0; i < S; ++i) {
      const SsSession &Q = s->ses[(size_t)i];
      if ((which && !which[i]) || !Q.started || Q.scan_off.size() < 2) continue;
      if ((rc = check_grid(call, occs, i, seen))) return rc;
      const size_t k = Q.scan_off.size() - 2;
      taken[(size_t)i] = occs[i];
      own[(size_t)i].pts = Q.store[Q.cur].p + Q.scan_off[k];
      own[(size_t)i].n = Q.scan_off[k + 1] - Q.scan_off[k];
      total += (size_t)own[(size_t)i].n;
    }
    CallFrame fr(ctx);
    if ((rc = fr.open())) return rc;
    hipStream_t st = fr.st;
    if (stats_host && (rc = ctx->d_tmp.ensure(ctx, sizeof(ndt_occ_stats)))) return rc;
    ndt_occ_stats *d_stats = stats_host ? (ndt_occ_stats *)ctx->d_tmp.p : nullptr;
    if ((rc = queue_occ(ctx, st, OccCall{taken.data(), S, own.data(), nullptr, nullptr, nullptr, S, total, s->last_pose.p, 24, max_range2, d_stats})))
      return rc;
    if (stats_host) HIP_TRY(ctx, hipMemcpyAsync(stats_host, d_stats, sizeof(ndt_occ_stats), hipMemcpyDeviceToHost, st));
    if ((rc = fr.close())) return rc;
    if (stats_host) HIP_TRY(ctx, hipStreamSynchronize(st));
    return NDT_OK;
  });
}

// ndt_sessions_occ_rebuild behind its bracket.  Who is taken; the call's scans are the taken sessions' archives one behind the other.
static int ss_occ_rebuild(const SetCall &call, ndt_occ *const *occs, const unsigned char *which, int clear, double max_range2,
                          ndt_occ_stats *stats_host) {
  ndt_sessions *s = call.s; ndt_ctx *ctx = call.ctx;
  if (!s->archive) return refuse_no_archive(s, call.f);
  int rc = NDT_OK;
  const int S = s->S;
  std::vector<ndt_occ *> taken((size_t)S, nullptr);
  std::vector<int> rows;
  std::set<const ndt_occ *> seen;
  uint64_t n_scans = 0, n_runs = 0;
  for (int i = 0; i < S; ++i) {
    const SsSession &Q = s->ses[(size_t)i];
    if ((which && !which[i]) || !Q.started) continue;
    if ((rc = check_grid(call, occs, i, seen))) return rc;
    taken[(size_t)i] = occs[i]; rows.push_back(i);
    n_scans += Q.arch_off.size() - 1;
    for (size_t k = 0; k + 1 < Q.arch_off.size(); ++k) n_runs += (Q.arch_off[k + 1] - Q.arch_off[k] + (uint64_t)kOccRun - 1) / (uint64_t)kOccRun;
    if (n_scans > (uint64_t)INT32_MAX || n_runs > (uint64_t)INT32_MAX)
      return call.refuse("more than 2^31 - 1 scans or runs of 256 beams over the sessions taken");
  }
  if (rows.empty()) {
    if (stats_host) memset(stats_host, 0, sizeof(*stats_host));
    return NDT_OK;
  }
  const size_t T = rows.size(), Q1 = (size_t)n_scans + 1;
  CallFrame fr(ctx);
  if ((rc = fr.open())) return rc;
  hipStream_t st = fr.st;
  // the table, one upload: the rows | the scans; behind it on the device the runs and every scan's (cos, sin)
  Regions R;
  const size_t o_tab = R.take(T * sizeof(OccRow)), o_scans = R.take(Q1 * sizeof(OccScan)), up_bytes = R.end,
               o_jobs = R.take((size_t)n_runs * sizeof(OccJob)), o_cs = R.take((size_t)n_scans * sizeof(double2));
  if ((rc = ctx->occ_tab.reserve(ctx, up_bytes))) return rc;
  if ((rc = ctx->d_occ.ensure(ctx, R.end))) return rc;
  if (stats_host && (rc = ctx->d_tmp.ensure(ctx, sizeof(ndt_occ_stats)))) return rc;
  unsigned char *h = ctx->occ_tab.h.p, *d = ctx->d_occ.p;
  memset(h, 0, up_bytes);
  OccRow *hr = Regions::at<OccRow>(h, o_tab);
  OccScan *hs = Regions::at<OccScan>(h, o_scans);
  uint64_t b = 0, off = 0;
  for (size_t t = 0; t < T; ++t) {
    const SsSession &Q = s->ses[(size_t)rows[t]];
    const ndt_occ &o = *occs[rows[t]];
    OccRow &r = hr[t];
    r.cells = o.cells.p; r.x0 = o.g.x0; r.y0 = o.g.y0; r.res = o.g.res; r.nx = o.g.nx; r.ny = o.g.ny;
    r.pts = reinterpret_cast<const float2 *>(Q.arch.p); r.n = b; r.pad = off;
    for (size_t k = 0; k + 1 < Q.arch_off.size(); ++k, ++b)
      hs[b] = OccScan{Q.traj[3 * k], Q.traj[3 * k + 1], Q.traj[3 * k + 2], off + Q.arch_off[k]};
    off += Q.arch_off.back();
  }
  hs[b] = OccScan{0.0, 0.0, 0.0, off};
  // the runs are dealt with a stride of about one session's runs, coprime to their number (occ_rebuild_kernel)
  uint64_t stride = std::max<uint64_t>(1, n_runs / T);
  while (n_runs && std::gcd(stride, n_runs) != 1) ++stride;
  for (int i : rows) {
    if ((rc = occ_touch(ctx, occs[i], st))) return rc;
    if (clear) HIP_TRY(ctx, hipMemsetAsync(occs[i]->cells.p, 0, occs[i]->cells.bytes, st));
  }
  HIP_TRY(ctx, ctx->occ_tab.upload(d, 0, up_bytes, st));
  const OccRow *tab = reinterpret_cast<const OccRow *>(d + o_tab);
  const OccScan *scans = reinterpret_cast<const OccScan *>(d + o_scans);
  OccJob *jobs = reinterpret_cast<OccJob *>(d + o_jobs);
  double2 *cs = reinterpret_cast<double2 *>(d + o_cs);
  unsigned long long *d_stats = stats_host ? (unsigned long long *)ctx->d_tmp.p : nullptr;
  occ_rebuild_jobs_kernel<<<1, 256, 0, st>>>(tab, (int)T, scans, (int)n_scans, jobs, (unsigned)n_runs, cs, d_stats);
  // as many workgroups as there are runs, eight per CU at most (or NDT_OPT_WORKGROUPS): each takes runs in turn
  const size_t wgs = std::max<size_t>(1, std::min<size_t>((size_t)n_runs, ctx->workgroups > 0 ? (size_t)ctx->workgroups : (size_t)ctx->num_cus * 8));
  occ_rebuild_kernel<<<dim3((unsigned)wgs), dim3(kOccRun), 0, st>>>(tab, scans, cs, max_range2, jobs, (unsigned)n_runs, (unsigned long long)stride, d_stats);
  const hipError_t e = hipGetLastError();
  rc = occ_wrote(ctx, taken.data(), S, st);      // (queued or not: the grids count as written behind this point of st)
  if (e != hipSuccess) return fail(ctx, NDT_E_HIP, call.f + ": " + hipGetErrorString(e));
  if (rc) return rc;
  if (stats_host) HIP_TRY(ctx, hipMemcpyAsync(stats_host, d_stats, sizeof(ndt_occ_stats), hipMemcpyDeviceToHost, st));
  if ((rc = fr.close())) return rc;
  if (stats_host) HIP_TRY(ctx, hipStreamSynchronize(st));
  return NDT_OK;
}

int ndt_sessions_occ_rebuild(ndt_sessions *s, ndt_occ *const *occs, const unsigned char *which, int clear, double max_range2,
                             ndt_occ_stats *stats_host) {
  SetCall call{s, "ndt_sessions_occ_rebuild", false};
  const int rc = call.enter();
  if (rc) return rc;
  if (!occs) return call.refuse("NULL occs");
  if (!(max_range2 >= 0.0)) return call.refuse("max_range2 is NaN or negative");
  return call.run([&] { return ss_occ_rebuild(call, occs, which, clear, max_range2, stats_host); });
}

}  // extern "C"

// ---- ndt_pg_*: pose graphs of many sessions optimised in one launch; ndt_repose_points: stored clouds moved to new poses
// (kernels in ndt_posegraph.hip.h) ----

namespace {

constexpr uint64_t kPgMax = 1ull << 28;              // nodes or arcs of one graph

// The refusals both forms start with (synchronous, nothing queued or written).
int pg_check(ndt_ctx *ctx, const void *poses, const uint64_t *node_off, const void *edges, const uint64_t *edge_off, int G,
             const ndt_pg_params *prm, const void *out, const char *fn) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  const std::string f(fn);
  if (!poses || !node_off || !edges || !edge_off || !prm || !out) return fail(ctx, NDT_E_ARG, f + ": NULL poses, offsets, edges, params or out");
  if (G < 1) return fail(ctx, NDT_E_ARG, f + ": need n_graphs >= 1");
  for (int g = 0; g < G; ++g) {
    if (node_off[g + 1] < node_off[g] || edge_off[g + 1] < edge_off[g]) return fail(ctx, NDT_E_ARG, f + ": offsets not monotone");
    if (node_off[g + 1] - node_off[g] >= kPgMax || edge_off[g + 1] - edge_off[g] >= kPgMax)
      return fail(ctx, NDT_E_ARG, f + ": a graph of 2^28 nodes or arcs or more");
  }
  if (prm->max_iter < 1 || prm->max_iter > 10000 || !(prm->eps_step >= 0.0) || !(prm->eps_step <= DBL_MAX) || prm->cg_max_iter < 0 ||
      prm->cg_max_iter > (1 << 30) || !(prm->cg_rtol > 0.0) || !(prm->cg_rtol < 1.0) || prm->max_halvings < 0 || prm->max_halvings > 60)
    return fail(ctx, NDT_E_ARG, f + ": parameters out of range");
  if (ctx->pending_map) return refuse_pending(ctx, f);
  return NDT_OK;
}

// The robust form's own refusals, behind pg_check on params->pg.
int pg_robust_check(ndt_ctx *ctx, const ndt_pg_robust_params *rp, const char *fn) {
  if (!((rp->mu0 == 0.0) || (rp->mu0 >= 1.0 && rp->mu0 <= kPgMuMax)) || !(rp->factor >= 1.05) || !(rp->factor <= 1e6) ||
      !(rp->eps_level >= 0.0) || !(rp->eps_level <= DBL_MAX) || rp->level_iter < 1 || rp->level_iter > 10000)
    return fail(ctx, NDT_E_ARG, std::string(fn) + ": robust parameters out of range");
  return NDT_OK;
}

// Graph g's row of a call's table but for its scratch offset: where its nodes and arcs start, how many, the key array's length.
PgRow pg_row(const uint64_t *node_off, const uint64_t *edge_off, int g) {
  PgRow r{};
  r.node0 = node_off[g]; r.edge0 = edge_off[g];
  r.n = (int)(node_off[g + 1] - node_off[g]); r.m = (int)(edge_off[g + 1] - edge_off[g]);
  r.n2 = 2;
  while (r.n2 < 2 * (size_t)r.m) r.n2 <<= 1;
  return r;
}

// The table and the launch on st, inside the caller's frame (d_pg, pg_tab).  node_off / edge_off index poses / edges as given
// (and phi, weight_out, chi2_out as edges).  rp == NULL: the plain form, out holds ndt_pg_result; else the robust one, out
// holds ndt_pg_robust_result.
int queue_pg(ndt_ctx *ctx, hipStream_t st, double *poses, const uint64_t *node_off, const ndt_pg_edge *edges, const uint64_t *edge_off,
             int G, const ndt_pg_params *prm, void *out, const ndt_pg_robust_params *rp = nullptr, const double *phi = nullptr,
             double *weight_out = nullptr, double *chi2_out = nullptr) {
  Regions R;
  const size_t o_tab = R.take((size_t)G * sizeof(PgRow), 256);
  int rc;
  if ((rc = ctx->pg_tab.reserve(ctx, (size_t)G * sizeof(PgRow)))) return rc;
  PgRow *rows = reinterpret_cast<PgRow *>(ctx->pg_tab.h.p);
  for (int g = 0; g < G; ++g) {
    PgRow r = pg_row(node_off, edge_off, g);
    r.scratch = r.m ? R.take(PgLayout((size_t)r.n, (size_t)r.m, (size_t)r.n2).end * sizeof(double), 256) : 0;   // (a graph without arcs uses none)
    rows[g] = r;
  }
  if ((rc = ctx->d_pg.ensure(ctx, R.end))) return rc;
  HIP_TRY(ctx, ctx->pg_tab.upload(ctx->d_pg.p + o_tab, 0, (size_t)G * sizeof(PgRow), st));
  PgParams P{};
  P.max_iter = prm->max_iter; P.cg_max_iter = prm->cg_max_iter; P.max_halvings = prm->max_halvings;
  P.eps_step = prm->eps_step; P.cg_rtol = prm->cg_rtol;
  const PgRow *d_rows = reinterpret_cast<const PgRow *>(ctx->d_pg.p + o_tab);
  const dim3 grid((unsigned)std::min(G, 1 << 20));
  if (!rp) {
    pg_solve_kernel<false><<<grid, dim3(kPgThreads), 0, st>>>(poses, edges, d_rows, G, P, ctx->d_pg.p, static_cast<ndt_pg_result *>(out));
  } else {
    PgExtra<true> X{};
    X.RP.mu0 = rp->mu0; X.RP.factor = rp->factor; X.RP.eps_level = rp->eps_level; X.RP.level_iter = rp->level_iter;
    X.phi = phi; X.weight_out = weight_out; X.chi2_out = chi2_out;
    pg_solve_kernel<true><<<grid, dim3(kPgThreads), 0, st>>>(poses, edges, d_rows, G, P, ctx->d_pg.p, static_cast<ndt_pg_robust_result *>(out), X);
  }
  HIP_TRY(ctx, hipGetLastError());
  return NDT_OK;
}

constexpr int kPgMarginalGrid = 1024;                // workgroups of one marginals launch at the most: one scratch slot each

// ndt_pg_marginals_batch*: the table of graphs and the queries in one upload, one scratch slot per workgroup sized for the
// largest graph that a query names, the launch on st; inside the caller's frame (d_pg, pg_tab).  Offsets index poses / edges /
// weight as given.
int queue_pg_marginals(ndt_ctx *ctx, hipStream_t st, const double *poses, const uint64_t *node_off, const ndt_pg_edge *edges,
                       const uint64_t *edge_off, int G, const double *weight, const ndt_pg_query *queries, int Q, const ndt_pg_params *prm,
                       ndt_pg_marginal *out) {
  Regions R;
  const size_t o_tab = R.take((size_t)G * sizeof(PgRow), 256), o_qry = R.take((size_t)Q * sizeof(ndt_pg_query), 256), tab_end = R.end;
  int rc;
  if ((rc = ctx->pg_tab.reserve(ctx, tab_end))) return rc;
  PgRow *rows = Regions::at<PgRow>(ctx->pg_tab.h.p, o_tab);
  for (int g = 0; g < G; ++g) rows[g] = pg_row(node_off, edge_off, g);     // (scratch: unused, the slot is the workgroup's)
  std::memcpy(Regions::at<ndt_pg_query>(ctx->pg_tab.h.p, o_qry), queries, (size_t)Q * sizeof(ndt_pg_query));
  size_t slot = 0;
  for (int k = 0; k < Q; ++k) {
    const int g = queries[k].graph;
    if (g < 0 || g >= G) continue;                           // (the kernel gives that query NDT_E_ARG)
    slot = std::max(slot, PgMLayout((size_t)rows[g].n, (size_t)rows[g].m, (size_t)rows[g].n2).end * sizeof(double));
  }
  slot = align_up(slot, 256);
  const int grid = std::min(Q, kPgMarginalGrid);
  const size_t o_slots = R.take((size_t)grid * slot, 256);
  if ((rc = ctx->d_pg.ensure(ctx, R.end))) return rc;
  HIP_TRY(ctx, ctx->pg_tab.upload(ctx->d_pg.p + o_tab, 0, tab_end, st));
  pg_marginal_kernel<<<dim3((unsigned)grid), dim3(kPgThreads), 0, st>>>(
      poses, edges, Regions::at<const PgRow>(ctx->d_pg.p, o_tab), G, weight, Regions::at<const ndt_pg_query>(ctx->d_pg.p, o_qry), Q,
      prm->cg_max_iter, prm->cg_rtol, ctx->d_pg.p + o_slots, (unsigned long long)slot, out);
  HIP_TRY(ctx, hipGetLastError());
  return NDT_OK;
}

int pg_marginals_check(ndt_ctx *ctx, const void *queries, int Q, const char *fn) {
  if (!queries) return fail(ctx, NDT_E_ARG, std::string(fn) + ": NULL queries");
  if (Q < 1) return fail(ctx, NDT_E_ARG, std::string(fn) + ": need n_queries >= 1");
  return NDT_OK;
}

// The bracket of a host-pointer entry point: offsets relative to the first graph's, the call frame, the call's block of d_scan
// (poses, arcs, then the regions that the entry point takes before open()) and the copies on the frame's stream.  An array of one
// double per arc is optional on either side: a NULL host pointer copies nothing and gives the kernel NULL.
struct PgStage {
  ndt_ctx *ctx;
  CallFrame fr;
  Regions U;
  const size_t G, n0, nn, e0, ne;                      // graphs; first node, nodes, first arc, arcs of the call
  const std::vector<uint64_t> noff, eoff;
  const size_t o_pose, o_edge;
  unsigned char *d = nullptr;
  PgStage(ndt_ctx *c, const uint64_t *node_off, const uint64_t *edge_off, int n_graphs)
      : ctx(c), fr(c), G((size_t)n_graphs), n0((size_t)node_off[0]), nn((size_t)node_off[G] - n0), e0((size_t)edge_off[0]),
        ne((size_t)edge_off[G] - e0), noff(rel_offsets(node_off, G)), eoff(rel_offsets(edge_off, G)), o_pose(U.take(nn * 24 + 8, 256)),
        o_edge(U.take(ne * sizeof(ndt_pg_edge) + 8, 256)) {}
  size_t take_arcs() { return U.take(ne * 8 + 8, 256); }
  int open(const double *poses_host, const ndt_pg_edge *edges_host) {
    int rc;
    if ((rc = fr.open()) || (rc = ctx->d_scan.ensure(ctx, U.end))) return rc;
    d = ctx->d_scan.p;
    if (nn) HIP_TRY(ctx, hipMemcpyAsync(d + o_pose, poses_host + 3 * n0, nn * 24, hipMemcpyHostToDevice, fr.st));
    if (ne) HIP_TRY(ctx, hipMemcpyAsync(d + o_edge, edges_host + e0, ne * sizeof(ndt_pg_edge), hipMemcpyHostToDevice, fr.st));
    return NDT_OK;
  }
  double *poses() const { return Regions::at<double>(d, o_pose); }
  const ndt_pg_edge *edges() const { return Regions::at<const ndt_pg_edge>(d, o_edge); }
  double *arcs(size_t o, const double *host) const { return host ? Regions::at<double>(d, o) : nullptr; }
  int up_arcs(size_t o, const double *host) {
    if (ne && host) HIP_TRY(ctx, hipMemcpyAsync(d + o, host + e0, ne * 8, hipMemcpyHostToDevice, fr.st));
    return NDT_OK;
  }
  int down_arcs(size_t o, double *host) {
    if (ne && host) HIP_TRY(ctx, hipMemcpyAsync(host + e0, d + o, ne * 8, hipMemcpyDeviceToHost, fr.st));
    return NDT_OK;
  }
  int down_poses(double *poses_host) {
    if (nn) HIP_TRY(ctx, hipMemcpyAsync(poses_host + 3 * n0, d + o_pose, nn * 24, hipMemcpyDeviceToHost, fr.st));
    return NDT_OK;
  }
  int down(size_t o, void *host, size_t bytes) {
    HIP_TRY(ctx, hipMemcpyAsync(host, d + o, bytes, hipMemcpyDeviceToHost, fr.st));
    return NDT_OK;
  }
};

// The residual of an arc with the measurement rel between two poses (tx, ty, th[deg]) and its two Jacobian blocks, as
// pg_linearise and pg_jac (ndt_posegraph.hip.h) state them; rel == NULL: the Jacobians alone.
void pg_host_arc(const double pa[3], const double pb[3], const double *rel, double r[3], double Ja[9], double Jb[9]) {
  const double ta = pa[2] * (M_PI / 180.0), tb = pb[2] * (M_PI / 180.0);
  const double c = std::cos(ta), s = std::sin(ta), dx = pb[0] - pa[0], dy = pb[1] - pa[1];
  const double a = -s * dx + c * dy, b = -c * dx - s * dy;
  const double A[9] = {-c, -s, a, s, -c, b, 0, 0, -1}, B[9] = {c, s, 0, -s, c, 0, 0, 0, 1};
  std::copy(A, A + 9, Ja); std::copy(B, B + 9, Jb);
  if (!rel) return;
  r[0] = c * dx + s * dy - rel[0];
  r[1] = a - rel[1];
  r[2] = pg_wrap(tb - ta - rel[2] * (M_PI / 180.0));
}

// The inverse of a symmetric 3 x 3 given as xx xy xt yy yt tt; false unless it is finite and positive definite (Sylvester).
bool pg_host_spd_inverse(const double S[6], double Inv[6]) {
  const double c00 = S[3] * S[5] - S[4] * S[4], c01 = S[4] * S[2] - S[1] * S[5], c02 = S[1] * S[4] - S[3] * S[2];
  const double m2 = S[0] * S[3] - S[1] * S[1], det = S[0] * c00 + S[1] * c01 + S[2] * c02;
  if (!(S[0] > 0.0) || !(m2 > 0.0) || !(det > 0.0) || !(det <= DBL_MAX)) return false;
  Inv[0] = c00 / det; Inv[1] = c01 / det; Inv[2] = c02 / det;
  Inv[3] = (S[0] * S[5] - S[2] * S[2]) / det; Inv[4] = (S[1] * S[2] - S[0] * S[4]) / det; Inv[5] = m2 / det;
  for (int k = 0; k < 6; ++k)
    if (!(std::fabs(Inv[k]) <= DBL_MAX)) return false;
  return true;
}

bool pg_host_finite(const double *v, int n) {
  for (int k = 0; k < n; ++k)
    if (!(std::fabs(v[k]) <= DBL_MAX)) return false;
  return true;
}

int repose_check(ndt_ctx *ctx, const void *xy, size_t stride, const void *off, int n_segs, const void *old_p, const void *new_p,
                 const void *out, size_t out_stride, const char *fn) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  const std::string f(fn);
  if (!xy || !off || !old_p || !new_p || !out) return fail(ctx, NDT_E_ARG, f + ": NULL points, offsets, poses or out");
  if (n_segs < 1) return fail(ctx, NDT_E_ARG, f + ": need n_segs >= 1");
  if (stride < 8 || (stride & 3) || out_stride < 8 || (out_stride & 3)) return fail(ctx, NDT_E_ARG, f + ": bad stride (need >= 8 and % 4 == 0)");
  if (out == xy && out_stride != stride) return fail(ctx, NDT_E_ARG, f + ": out is xy at another stride");
  return NDT_OK;
}

int queue_repose(ndt_ctx *ctx, hipStream_t st, const void *xy, size_t stride, const uint64_t *off, int n_segs, const double *old_p,
                 const double *new_p, void *out, size_t out_stride) {
  const unsigned gy = (unsigned)std::min(n_segs, 65535), gx = std::max(64u, std::min(2048u, 8192u / gy));
  repose_points_kernel<<<dim3(gx, gy), 256, 0, st>>>((const unsigned char *)xy, stride, (const unsigned long long *)off, n_segs, old_p, new_p,
                                                      (unsigned char *)out, out_stride);
  HIP_TRY(ctx, hipGetLastError());
  return NDT_OK;
}

// Pose2D::calRmat's entries (include/ndt_slam/Pose2D.h:43-47)
void pg_cos_sin(double th_deg, double *c, double *s) { const double a = th_deg * M_PI / 180; *c = std::cos(a); *s = std::sin(a); }

}  // namespace

extern "C" {

int ndt_pg_default_params(ndt_pg_params *p) {
  if (!p) return NDT_E_ARG;
  p->max_iter = 20; p->eps_step = 1e-9; p->cg_max_iter = 0; p->cg_rtol = 1e-10; p->max_halvings = 8;
  return NDT_OK;
}

int ndt_pg_edge_between(const double from_pose[3], const double to_pose[3], ndt_pg_edge *edge) {
  if (!from_pose || !to_pose || !edge) return fail(nullptr, NDT_E_ARG, "ndt_pg_edge_between: NULL pointer");
  for (int k = 0; k < 3; ++k)
    if (!(std::fabs(from_pose[k]) <= DBL_MAX) || !(std::fabs(to_pose[k]) <= DBL_MAX))
      return fail(nullptr, NDT_E_ARG, "ndt_pg_edge_between: a pose is not finite");
  // Pose2D::calMotion(curPose = to, prevPose = from) (src/Pose2D.cpp:5-14)
  double c, s;
  pg_cos_sin(from_pose[2], &c, &s);
  const double dx = to_pose[0] - from_pose[0], dy = to_pose[1] - from_pose[1];
  edge->rel[0] = c * dx + s * dy;
  edge->rel[1] = -s * dx + c * dy;
  double dif = to_pose[2] - from_pose[2];                  // MyUtil::sub_angle (src/MyUtil.cpp:15-23)
  if (dif < -180) dif += 360; else if (dif >= 180) dif -= 360;
  edge->rel[2] = dif;
  return NDT_OK;
}

int ndt_pg_info_from_cov(const double cov_world[9], double th_deg, double info[6]) {
  if (!cov_world || !info) return fail(nullptr, NDT_E_ARG, "ndt_pg_info_from_cov: NULL pointer");
  if (!pg_host_finite(cov_world, 9)) return fail(nullptr, NDT_E_ARG, "ndt_pg_info_from_cov: the covariance is not finite");
  if (!pg_host_finite(&th_deg, 1)) return fail(nullptr, NDT_E_ARG, "ndt_pg_info_from_cov: the heading is not finite");
  const double *C = cov_world;
  if (!(C[0] > 0.0) || !(C[4] > 0.0) || !(C[8] > 0.0)) return fail(nullptr, NDT_E_ARG, "ndt_pg_info_from_cov: the covariance is not positive definite");
  const int pr[3][2] = {{1, 3}, {2, 6}, {5, 7}}, di[3][2] = {{0, 4}, {0, 8}, {4, 8}};
  for (int k = 0; k < 3; ++k)
    if (std::fabs(C[pr[k][0]] - C[pr[k][1]]) > 1e-9 * std::sqrt(C[di[k][0]] * C[di[k][1]]))
      return fail(nullptr, NDT_E_ARG, "ndt_pg_info_from_cov: the covariance is not symmetric");
  const double cxy = 0.5 * (C[1] + C[3]), cxt = 0.5 * (C[2] + C[6]), cyt = 0.5 * (C[5] + C[7]);
  double c, s;
  pg_cos_sin(th_deg, &c, &s);
  // C' = R3^T C R3, R3 = diag(R(th), 1): the xy block R^T Cxy R, the (xy, t) column R^T (cxt, cyt)
  const double a00 = c * C[0] + s * cxy, a01 = c * cxy + s * C[4];       // rows of R^T Cxy
  const double a10 = -s * C[0] + c * cxy, a11 = -s * cxy + c * C[4];
  const double S[9] = {a00 * c + a01 * s, -a00 * s + a01 * c, c * cxt + s * cyt,
                       0, -a10 * s + a11 * c, -s * cxt + c * cyt,
                       0, 0, C[8]};
  const double xx = S[0], xy = S[1], xt = S[2], yy = S[4], yt = S[5], tt = S[8];
  const double c00 = yy * tt - yt * yt, c01 = yt * xt - xy * tt, c02 = xy * yt - yy * xt;
  const double m2 = xx * yy - xy * xy, det = xx * c00 + xy * c01 + xt * c02;
  // Sylvester's criterion to working precision: the pivots xx, m2 / xx, det / m2 against the largest diagonal entry of their
  // unit (a first matched scan's covariance has 1e-35 m^2 along the motion: positive, and no information anyone can use)
  const double big = std::max(xx, yy);
  if (!(xx > 0.0) || !(m2 > 0.0) || !(det > 0.0) || !(det <= DBL_MAX) || !(xx > 1e-12 * big) || !(m2 > 1e-12 * big * xx) ||
      !(det > 1e-12 * tt * m2))
    return fail(nullptr, NDT_E_ARG, "ndt_pg_info_from_cov: the covariance is not positive definite");
  info[0] = c00 / det; info[1] = c01 / det; info[2] = c02 / det;
  info[3] = (xx * tt - xt * xt) / det; info[4] = (xy * xt - xx * yt) / det; info[5] = m2 / det;
  if (!pg_host_finite(info, 6)) return fail(nullptr, NDT_E_ARG, "ndt_pg_info_from_cov: the inverse is not finite");
  return NDT_OK;
}

int ndt_pg_optimize_batch_dev(ndt_ctx *ctx, double *poses_dev, const uint64_t *node_offsets_host, const ndt_pg_edge *edges_dev,
                              const uint64_t *edge_offsets_host, int n_graphs, const ndt_pg_params *params, ndt_pg_result *out_dev,
                              void *stream) {
  int rc = pg_check(ctx, poses_dev, node_offsets_host, edges_dev, edge_offsets_host, n_graphs, params, out_dev, "ndt_pg_optimize_batch_dev");
  if (rc) return rc;
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {
    return queue_pg(ctx, st, poses_dev, node_offsets_host, edges_dev, edge_offsets_host, n_graphs, params, out_dev);
  });
}

int ndt_pg_optimize_batch(ndt_ctx *ctx, double *poses_host, const uint64_t *node_offsets_host, const ndt_pg_edge *edges_host,
                          const uint64_t *edge_offsets_host, int n_graphs, const ndt_pg_params *params, ndt_pg_result *out_host) {
  int rc = pg_check(ctx, poses_host, node_offsets_host, edges_host, edge_offsets_host, n_graphs, params, out_host, "ndt_pg_optimize_batch");
  if (rc) return rc;
  PgStage S(ctx, node_offsets_host, edge_offsets_host, n_graphs);
  const size_t res_bytes = S.G * sizeof(ndt_pg_result), o_res = S.U.take(res_bytes, 256);
  if ((rc = S.open(poses_host, edges_host)) ||
      (rc = queue_pg(ctx, S.fr.st, S.poses(), S.noff.data(), S.edges(), S.eoff.data(), n_graphs, params, S.d + o_res)) ||
      (rc = S.down_poses(poses_host)) || (rc = S.down(o_res, out_host, res_bytes)))
    return rc;
  return S.fr.close_and_wait();
}

int ndt_pg_robust_default_params(ndt_pg_robust_params *p) {
  if (!p) return NDT_E_ARG;
  ndt_pg_default_params(&p->pg);
  p->pg.max_iter = 200;
  p->mu0 = 0.0; p->factor = 1.4; p->eps_level = 1e-3; p->level_iter = 3;
  return NDT_OK;
}

int ndt_pg_optimize_robust_batch_dev(ndt_ctx *ctx, double *poses_dev, const uint64_t *node_offsets_host, const ndt_pg_edge *edges_dev,
                                     const uint64_t *edge_offsets_host, int n_graphs, const double *phi_dev,
                                     const ndt_pg_robust_params *params, ndt_pg_robust_result *out_dev, double *weight_out_dev,
                                     double *chi2_out_dev, void *stream) {
  const char *fn = "ndt_pg_optimize_robust_batch_dev";
  int rc = pg_check(ctx, poses_dev, node_offsets_host, edges_dev, edge_offsets_host, n_graphs, params ? &params->pg : nullptr, out_dev, fn);
  if (rc || (rc = pg_robust_check(ctx, params, fn))) return rc;
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {
    return queue_pg(ctx, st, poses_dev, node_offsets_host, edges_dev, edge_offsets_host, n_graphs, &params->pg, out_dev, params, phi_dev,
                    weight_out_dev, chi2_out_dev);
  });
}

int ndt_pg_optimize_robust_batch(ndt_ctx *ctx, double *poses_host, const uint64_t *node_offsets_host, const ndt_pg_edge *edges_host,
                                 const uint64_t *edge_offsets_host, int n_graphs, const double *phi_host,
                                 const ndt_pg_robust_params *params, ndt_pg_robust_result *out_host, double *weight_out_host,
                                 double *chi2_out_host) {
  const char *fn = "ndt_pg_optimize_robust_batch";
  int rc = pg_check(ctx, poses_host, node_offsets_host, edges_host, edge_offsets_host, n_graphs, params ? &params->pg : nullptr, out_host, fn);
  if (rc || (rc = pg_robust_check(ctx, params, fn))) return rc;
  PgStage S(ctx, node_offsets_host, edge_offsets_host, n_graphs);
  const size_t res_bytes = S.G * sizeof(ndt_pg_robust_result), o_res = S.U.take(res_bytes, 256), o_phi = S.take_arcs(), o_w = S.take_arcs(),
               o_c = S.take_arcs();
  if ((rc = S.open(poses_host, edges_host)) || (rc = S.up_arcs(o_phi, phi_host)) ||
      (rc = queue_pg(ctx, S.fr.st, S.poses(), S.noff.data(), S.edges(), S.eoff.data(), n_graphs, &params->pg, S.d + o_res, params,
                     S.arcs(o_phi, phi_host), S.arcs(o_w, weight_out_host), S.arcs(o_c, chi2_out_host))) ||
      (rc = S.down_poses(poses_host)) || (rc = S.down(o_res, out_host, res_bytes)) || (rc = S.down_arcs(o_w, weight_out_host)) ||
      (rc = S.down_arcs(o_c, chi2_out_host)))
    return rc;
  return S.fr.close_and_wait();
}

int ndt_pg_marginals_batch_dev(ndt_ctx *ctx, const double *poses_dev, const uint64_t *node_offsets_host, const ndt_pg_edge *edges_dev,
                               const uint64_t *edge_offsets_host, int n_graphs, const double *weight_dev,
                               const ndt_pg_query *queries_host, int n_queries, const ndt_pg_params *params,
                               ndt_pg_marginal *out_dev, void *stream) {
  const char *fn = "ndt_pg_marginals_batch_dev";
  int rc = pg_check(ctx, poses_dev, node_offsets_host, edges_dev, edge_offsets_host, n_graphs, params, out_dev, fn);
  if (rc || (rc = pg_marginals_check(ctx, queries_host, n_queries, fn))) return rc;
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {
    return queue_pg_marginals(ctx, st, poses_dev, node_offsets_host, edges_dev, edge_offsets_host, n_graphs, weight_dev, queries_host,
                              n_queries, params, out_dev);
  });
}

int ndt_pg_marginals_batch(ndt_ctx *ctx, const double *poses_host, const uint64_t *node_offsets_host, const ndt_pg_edge *edges_host,
                           const uint64_t *edge_offsets_host, int n_graphs, const double *weight_host,
                           const ndt_pg_query *queries_host, int n_queries, const ndt_pg_params *params,
                           ndt_pg_marginal *out_host) {
  const char *fn = "ndt_pg_marginals_batch";
  int rc = pg_check(ctx, poses_host, node_offsets_host, edges_host, edge_offsets_host, n_graphs, params, out_host, fn);
  if (rc || (rc = pg_marginals_check(ctx, queries_host, n_queries, fn))) return rc;
  PgStage S(ctx, node_offsets_host, edge_offsets_host, n_graphs);
  const size_t o_w = S.take_arcs(), res_bytes = (size_t)n_queries * sizeof(ndt_pg_marginal), o_res = S.U.take(res_bytes, 256);
  if ((rc = S.open(poses_host, edges_host)) || (rc = S.up_arcs(o_w, weight_host)) ||
      (rc = queue_pg_marginals(ctx, S.fr.st, S.poses(), S.noff.data(), S.edges(), S.eoff.data(), n_graphs, S.arcs(o_w, weight_host),
                               queries_host, n_queries, params, Regions::at<ndt_pg_marginal>(S.d, o_res))) ||
      (rc = S.down(o_res, out_host, res_bytes)))
    return rc;
  return S.fr.close_and_wait();
}

int ndt_pg_relative_cov(const double pose_a[3], const double pose_b[3], const ndt_pg_marginal *m, double cov[9]) {
  if (!pose_a || !pose_b || !m || !cov) return fail(nullptr, NDT_E_ARG, "ndt_pg_relative_cov: NULL pointer");
  if (!pg_host_finite(pose_a, 3) || !pg_host_finite(pose_b, 3) || !pg_host_finite(m->Saa, 9) || !pg_host_finite(m->Sab, 9) ||
      !pg_host_finite(m->Sbb, 9))
    return fail(nullptr, NDT_E_ARG, "ndt_pg_relative_cov: a number is not finite");
  double Ja[9], Jb[9];
  pg_host_arc(pose_a, pose_b, nullptr, nullptr, Ja, Jb);
  // M = [Ja Jb] [[Saa Sab] [Sab^T Sbb]] [Ja Jb]^T, term by term
  const auto mul3 = [](const double *X, const double *Y, bool y_transposed, double *Z) {
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        double v = 0.0;
        for (int k = 0; k < 3; ++k) v += X[3 * r + k] * (y_transposed ? Y[3 * c + k] : Y[3 * k + c]);
        Z[3 * r + c] = v;
      }
  };
  double T1[9], T2[9], C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const double *J[2] = {Ja, Jb};
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) {
      double Sab_t[9];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Sab_t[3 * r + c] = m->Sab[3 * c + r];
      const double *S = i == 0 ? (j == 0 ? m->Saa : m->Sab) : (j == 0 ? Sab_t : m->Sbb);
      mul3(J[i], S, false, T1);
      mul3(T1, J[j], true, T2);
      for (int k = 0; k < 9; ++k) C[k] += T2[k];
    }
  const double S6[6] = {C[0], 0.5 * (C[1] + C[3]), 0.5 * (C[2] + C[6]), C[4], 0.5 * (C[5] + C[7]), C[8]};
  double inv[6];
  if (!pg_host_finite(C, 9) || !pg_host_spd_inverse(S6, inv))
    return fail(nullptr, NDT_E_ARG, "ndt_pg_relative_cov: the covariance is not positive definite");
  cov[0] = S6[0]; cov[1] = S6[1]; cov[2] = S6[2]; cov[3] = S6[1]; cov[4] = S6[3]; cov[5] = S6[4]; cov[6] = S6[2]; cov[7] = S6[4]; cov[8] = S6[5];
  return NDT_OK;
}

int ndt_pg_edge_chi2(const double pose_a[3], const double pose_b[3], const ndt_pg_edge *edge, const double rel_cov[9], double *d2) {
  if (!pose_a || !pose_b || !edge || !rel_cov || !d2) return fail(nullptr, NDT_E_ARG, "ndt_pg_edge_chi2: NULL pointer");
  if (!pg_host_finite(pose_a, 3) || !pg_host_finite(pose_b, 3) || !pg_host_finite(edge->rel, 3) || !pg_host_finite(edge->info, 6) ||
      !pg_host_finite(rel_cov, 9))
    return fail(nullptr, NDT_E_ARG, "ndt_pg_edge_chi2: a number is not finite");
  double r[3], Ja[9], Jb[9], om_inv[6], inv[6];
  pg_host_arc(pose_a, pose_b, edge->rel, r, Ja, Jb);
  if (!pg_host_spd_inverse(edge->info, om_inv)) return fail(nullptr, NDT_E_ARG, "ndt_pg_edge_chi2: the information is not positive definite");
  const double *C = rel_cov;
  const double S[6] = {C[0] + om_inv[0], 0.5 * (C[1] + C[3]) + om_inv[1], 0.5 * (C[2] + C[6]) + om_inv[2], C[4] + om_inv[3],
                       0.5 * (C[5] + C[7]) + om_inv[4], C[8] + om_inv[5]};
  if (!pg_host_spd_inverse(S, inv)) return fail(nullptr, NDT_E_ARG, "ndt_pg_edge_chi2: rel_cov + Omega^-1 is not positive definite");
  const double w[3] = {inv[0] * r[0] + inv[1] * r[1] + inv[2] * r[2], inv[1] * r[0] + inv[3] * r[1] + inv[4] * r[2],
                       inv[2] * r[0] + inv[4] * r[1] + inv[5] * r[2]};
  const double v = r[0] * w[0] + r[1] * w[1] + r[2] * w[2];
  if (!(std::fabs(v) <= DBL_MAX)) return fail(nullptr, NDT_E_ARG, "ndt_pg_edge_chi2: the distance is not finite");
  *d2 = v;
  return NDT_OK;
}

int ndt_repose_points_dev(ndt_ctx *ctx, const float *xy_dev, size_t stride_bytes, const uint64_t *seg_offsets_dev, int n_segs,
                          const double *old_poses_dev, const double *new_poses_dev, float *out_xy_dev, size_t out_stride_bytes,
                          void *stream) {
  int rc = repose_check(ctx, xy_dev, stride_bytes, seg_offsets_dev, n_segs, old_poses_dev, new_poses_dev, out_xy_dev, out_stride_bytes,
                        "ndt_repose_points_dev");
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  return queue_repose(ctx, st, xy_dev, stride_bytes, seg_offsets_dev, n_segs, old_poses_dev, new_poses_dev, out_xy_dev, out_stride_bytes);
}

int ndt_repose_points(ndt_ctx *ctx, const float *xy_host, size_t stride_bytes, const uint64_t *seg_offsets_host, int n_segs,
                      const double *old_poses_host, const double *new_poses_host, float *out_xy_host, size_t out_stride_bytes) {
  int rc = repose_check(ctx, xy_host, stride_bytes, seg_offsets_host, n_segs, old_poses_host, new_poses_host, out_xy_host, out_stride_bytes,
                        "ndt_repose_points");
  if (rc) return rc;
  const size_t K = (size_t)n_segs;
  for (size_t k = 0; k < K; ++k)
    if (seg_offsets_host[k + 1] < seg_offsets_host[k]) return fail(ctx, NDT_E_ARG, "ndt_repose_points: offsets not monotone");
  const size_t p0 = (size_t)seg_offsets_host[0], np = (size_t)seg_offsets_host[K] - p0;
  if (np == 0) return NDT_OK;
  const std::vector<uint64_t> off = rel_offsets(seg_offsets_host, K);
  // the points packed (8 bytes each) through the call's one staging block; the result comes back into the same place
  std::vector<float> pk(2 * np);
  for (size_t i = 0; i < np; ++i) memcpy(&pk[2 * i], (const unsigned char *)xy_host + (p0 + i) * stride_bytes, 8);
  CallFrame fr(ctx);
  if ((rc = fr.open())) return rc;
  hipStream_t st = fr.st;
  Regions U;
  const size_t o_off = U.take((K + 1) * 8, 256), o_old = U.take(K * 24, 256), o_new = U.take(K * 24, 256), o_xy = U.take(np * 8, 256);
  if ((rc = ctx->d_scan.ensure(ctx, U.end))) return rc;
  unsigned char *d = ctx->d_scan.p;
  HIP_TRY(ctx, hipMemcpyAsync(d + o_off, off.data(), (K + 1) * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_old, old_poses_host, K * 24, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_new, new_poses_host, K * 24, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_xy, pk.data(), np * 8, hipMemcpyHostToDevice, st));
  if ((rc = queue_repose(ctx, st, d + o_xy, 8, (const uint64_t *)(d + o_off), n_segs, (const double *)(d + o_old), (const double *)(d + o_new),
                         d + o_xy, 8)))
    return rc;
  HIP_TRY(ctx, hipMemcpyAsync(pk.data(), d + o_xy, np * 8, hipMemcpyDeviceToHost, st));
  if ((rc = fr.close_and_wait())) return rc;
  for (size_t i = 0; i < np; ++i) memcpy((unsigned char *)out_xy_host + (p0 + i) * out_stride_bytes, &pk[2 * i], 8);
  return NDT_OK;
}

}  // extern "C"

// ---- many (scan, map, lattice) jobs in one sweep and one pick (ndt_score_lattice_multi_dev, ndt_lattice_select_multi_dev;
//      kernels in ndt_score.hip.h) ----

namespace {

// The refusals both calls make of their job list (behind the NULL checks): n_jobs, every job's indices (n_maps, n_scans: -1
// where the call has none) and lattice, the volume offsets, the pose count.  P[j]: the size of job j's lattice.
int check_score_jobs(ndt_ctx *ctx, const std::string &f, const ndt_score_job *jobs, int n_jobs, int n_maps, int n_scans,
                     const uint64_t *vol_offsets, uint64_t max_poses, std::vector<uint64_t> *P) {
  if (n_jobs < 1) return fail(ctx, NDT_E_ARG, f + ": need n_jobs >= 1");
  P->resize((size_t)n_jobs);
  uint64_t run = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const std::string which = f + ": job " + std::to_string(j);
    if (n_maps >= 0 && (jobs[j].map < 0 || jobs[j].map >= n_maps)) return fail(ctx, NDT_E_ARG, which + ": map index out of range");
    if (n_scans >= 0 && (jobs[j].scan < 0 || jobs[j].scan >= n_scans)) return fail(ctx, NDT_E_ARG, which + ": scan index out of range");
    if (!lattice_count(&jobs[j].lattice, &(*P)[j]))
      return fail(ctx, NDT_E_ARG, which + ": bad lattice (a dimension below 1, a non-finite origin or step, or more than 2^31 - 1 poses)");
    if ((*P)[j] > max_poses) return fail(ctx, NDT_E_ARG, which + ": a lattice of more than 2^24 poses (ndt_lattice_select_dev takes it)");
    if (vol_offsets[j] != run) return fail(ctx, NDT_E_ARG, which + ": vol_offsets is not the running sum of the lattice sizes");
    run += (*P)[j];
    if (run > (uint64_t)INT32_MAX) return fail(ctx, NDT_E_ARG, f + ": more than 2^31 - 1 poses in all (at job " + std::to_string(j) + ")");
  }
  if (vol_offsets[n_jobs] != run) return fail(ctx, NDT_E_ARG, f + ": vol_offsets[n_jobs] is not the sum of the lattice sizes");
  return NDT_OK;
}

// ndt_score_lattice_multi_dev.  longest: no scan of the call has more points (the public call: total_points; the lengths
// themselves are on the device) -- what the dynamic LDS is sized for.
int score_multi(ndt_ctx *ctx, const ndt_map *const *maps, int n_maps, const float *scans_xy_dev, const uint64_t *offsets_dev,
                int n_scans, size_t total_points, size_t longest, const ndt_score_job *jobs, int n_jobs, double *score_dev,
                uint32_t *pairs_dev, const uint64_t *vol_offsets_host, void *stream) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  const std::string f("ndt_score_lattice_multi_dev");
  if (!maps || !scans_xy_dev || !offsets_dev || !jobs || !score_dev || !vol_offsets_host)
    return fail(ctx, NDT_E_ARG, f + ": NULL maps, scans, offsets, jobs, score or vol_offsets");
  if (n_scans < 1 || total_points > (size_t)INT32_MAX) return fail(ctx, NDT_E_ARG, f + ": need n_scans >= 1 and total_points <= 2^31 - 1");
  std::vector<uint64_t> P;
  int rc = check_score_jobs(ctx, f, jobs, n_jobs, n_maps < 0 ? 0 : n_maps, n_scans, vol_offsets_host, (uint64_t)INT32_MAX, &P);
  if (rc) return rc;
  MultiMaps mm;
  if ((rc = check_multi(ctx, maps, n_maps, true, 0, f.c_str(), &mm))) return rc;
  if (ctx->pending_map) return refuse_pending(ctx, f);
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {
    // the table: a row per job (the map's view as it is now), then the prefix of tiles; staged in pinned memory, one copy
    Regions R;
    const size_t o_jobs = R.take((size_t)n_jobs * sizeof(ScoreJob), 256), o_tile0 = R.take(((size_t)n_jobs + 1) * 8, 256);
    int rc2;
    if ((rc2 = ctx->d_sj.ensure(ctx, R.end)) || (rc2 = ctx->sj_tab.reserve(ctx, R.end))) return rc2;
    ScoreJob *h_jobs = R.at<ScoreJob>(ctx->sj_tab.h.p, o_jobs);
    unsigned long long *h_tile0 = R.at<unsigned long long>(ctx->sj_tab.h.p, o_tile0);
    unsigned long long units = 0;
    for (int j = 0; j < n_jobs; ++j) {
      ScoreJob &J = h_jobs[j];
      J.M = maps[jobs[j].map]->view; J.L = lattice_of(jobs[j].lattice); J.P = P[(size_t)j]; J.vol_off = vol_offsets_host[j]; J.scan = jobs[j].scan;
      h_tile0[j] = units;
      units += (P[(size_t)j] + kScoreTile - 1) / kScoreTile;
    }
    h_tile0[n_jobs] = units;
    MapRead rd{ctx, st, mm.distinct.data(), (int)mm.distinct.size()};
    if ((rc2 = rd.begin())) return rc2;
    HIP_TRY(ctx, ctx->sj_tab.upload(ctx->d_sj.p, 0, R.end, st));
    // LDS for the longest scan that can be staged
    const ndt_map *m0 = maps[0];
    const bool sse = m0->prm.transform_sse != 0, incl = m0->prm.radius_inclusive != 0;
    const bool chk = !(m0->view.e_hi > 1.0 + 1e-6);    // (queue_score's instances; check_multi: the same in every map)
    const unsigned stage_pts = ctx->score_stage ? (unsigned)std::min<size_t>(longest, (size_t)kScoreStagePts) : 0u;
    const size_t lds = (size_t)stage_pts * sizeof(float2);
    const size_t per_cu = std::min<size_t>(4, std::max<size_t>(1, (size_t)(150 * 1024) / (lds + 1024)));
    const uint64_t want = ctx->workgroups > 0 ? (uint64_t)ctx->workgroups : (uint64_t)ctx->num_cus * per_cu;
    const unsigned grid = (unsigned)std::min<uint64_t>(units, want);
    Event *evr = rd.ev;
    auto sweep = [&](auto S, auto I, auto C) {
      hipExtLaunchKernelGGL((ndt_score_multi_kernel<decltype(S)::value, decltype(I)::value, decltype(C)::value>), dim3(grid), dim3(kScoreBlock),
                            lds, st, evr[0], evr[1], 0, (const ScoreJob *)R.at<ScoreJob>(ctx->d_sj.p, o_jobs),
                            (const unsigned long long *)R.at<unsigned long long>(ctx->d_sj.p, o_tile0), n_jobs, m0->prm.libm_f32,
                            (const float2 *)scans_xy_dev, (const unsigned long long *)offsets_dev, stage_pts, score_dev, pairs_dev);
    };
    const std::true_type yes; const std::false_type no;
    if (sse && incl)      sweep(yes, yes, yes);
    else if (sse && !chk) sweep(yes, no, no);
    else if (sse)         sweep(yes, no, yes);
    else if (incl)        sweep(no, yes, yes);
    else                  sweep(no, no, yes);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, NDT_E_HIP, f + ": " + hipGetErrorString(e));
    // (queue_score's rule: to a map whose builds another stream carries, this sweep is a deferred launch)
    const bool deferred = std::any_of(mm.distinct.begin(), mm.distinct.end(), [&](const ndt_map *m) { return st != m->ctx->stream; });
    return rd.entered(NDT_OK, /*end_carried=*/false, deferred, "ndt_score_lattice_multi_dev");
  });
}

}  // namespace

extern "C" {

int ndt_score_lattice_multi_dev(ndt_ctx *ctx, const ndt_map *const *maps, int n_maps, const float *scans_xy_dev,
                                const uint64_t *offsets_dev, int n_scans, size_t total_points, const ndt_score_job *jobs, int n_jobs,
                                double *score_dev, uint32_t *pairs_dev, const uint64_t *vol_offsets_host, void *stream) {
  return score_multi(ctx, maps, n_maps, scans_xy_dev, offsets_dev, n_scans, total_points, total_points, jobs, n_jobs, score_dev, pairs_dev,
                     vol_offsets_host, stream);
}

int ndt_lattice_select_multi_dev(ndt_ctx *ctx, const ndt_score_job *jobs, int n_jobs, const double *score_dev, const uint32_t *pairs_dev,
                                 const uint64_t *vol_offsets_host, int top_k, int local_max, uint64_t *cand_index_dev, int *n_cand_dev,
                                 void *stream) {
  if (!ctx) return fail(nullptr, NDT_E_ARG, "null context");
  const std::string f("ndt_lattice_select_multi_dev");
  if (!jobs || !score_dev || !pairs_dev || !vol_offsets_host || !cand_index_dev || !n_cand_dev) return fail(ctx, NDT_E_ARG, f + ": NULL array");
  std::vector<uint64_t> P;
  int rc = check_score_jobs(ctx, f, jobs, n_jobs, -1, -1, vol_offsets_host, (uint64_t)kPickMaxPoses, &P);
  if (rc) return rc;
  if (top_k < 1 || top_k > kPickMaxK) return fail(ctx, NDT_E_ARG, f + ": top_k must be in 1 .. 16");
  if (ctx->pending_map) return refuse_pending(ctx, f);
  return CallFrame::run(ctx, stream, [&](hipStream_t st) {
    const size_t bytes = (size_t)n_jobs * sizeof(PickJob);
    int rc2;
    if ((rc2 = ctx->d_pk.ensure(ctx, bytes)) || (rc2 = ctx->pk_tab.reserve(ctx, bytes))) return rc2;
    PickJob *h = reinterpret_cast<PickJob *>(ctx->pk_tab.h.p);
    for (int j = 0; j < n_jobs; ++j) h[j] = PickJob{lattice_of(jobs[j].lattice), P[(size_t)j], vol_offsets_host[j]};
    HIP_TRY(ctx, ctx->pk_tab.upload(ctx->d_pk.p, 0, bytes, st));
    lattice_pick_multi_kernel<<<(unsigned)n_jobs, kPickBlock, (size_t)top_k * kPickBlock * (sizeof(double) + sizeof(unsigned)), st>>>(
        reinterpret_cast<const PickJob *>(ctx->d_pk.p), score_dev, pairs_dev, top_k, local_max, (unsigned long long *)cand_index_dev, n_cand_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, NDT_E_HIP, f + ": " + hipGetErrorString(e));
    return (int)NDT_OK;
  });
}

}  // extern "C"

#include "ndt_loops.hip.h"
#include "ndt_cross.hip.h"
#include "ndt_place.hip.h"
