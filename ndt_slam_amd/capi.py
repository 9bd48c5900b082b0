"""ctypes binding of libndt_mi355x.so (include/ndt_mi355x.h).

This is the only way Python reaches the kernels: every call goes through the C ABI a C++
maintainer of the reference would bind.  There is no CPU fallback: a missing
library or a missing GPU raises.
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NDT_LIB_PATH") or os.path.join(_HERE, "libndt_mi355x.so")   # override: diagnostic builds
_LIB = None


class NdtError(RuntimeError):
    pass


class Params(C.Structure):
    """ndt_params (include/ndt_mi355x.h)."""
    _fields_ = [
        ("resolution", C.c_float), ("step_size", C.c_double), ("trans_eps", C.c_double),
        ("max_iter", C.c_int), ("outlier_ratio", C.c_double), ("min_pts", C.c_int),
        ("eig_mult", C.c_double), ("cov_unbiased", C.c_int), ("cov_init_identity", C.c_int),
        ("conv_ge", C.c_int), ("radius_inclusive", C.c_int), ("transform_sse", C.c_int),
        ("stale_h_ang", C.c_int), ("snap_thresh", C.c_double), ("mt_max_iter", C.c_int),
        ("mt_mu", C.c_double), ("mt_nu", C.c_double), ("libm_f32", C.c_int), ("grid_margin", C.c_int),
    ]


class FuseParams(C.Structure):
    """ndt_fuse_params (include/ndt_mi355x.h)."""
    _fields_ = [("coe_ndt_cov", C.c_double), ("coe_vel", C.c_double), ("coe_omega", C.c_double),
                ("del_time", C.c_double), ("score_thre", C.c_double)]


class SubmapDesc(C.Structure):
    """ndt_submap_desc (include/ndt_mi355x.h): one submap of ndt_local_map_batch{,_dev}."""
    _fields_ = [("scans_xy", C.c_void_p), ("offsets", C.c_void_p), ("n_scans", C.c_int), ("first_submap", C.c_int),
                ("newest", C.c_int), ("remove_moving", C.c_int), ("resol", C.c_double), ("thre_neighbor", C.c_double),
                ("prev_xy", C.c_void_p), ("n_prev", C.c_size_t)]


class SessionParams(C.Structure):
    """ndt_session_params (include/ndt_mi355x.h): the parameters of one session set."""
    _fields_ = [("match", Params), ("fuse", FuseParams), ("space", C.c_double), ("space_thre", C.c_double),
                ("leaf", C.c_float), ("resol", C.c_double), ("thre_neighbor", C.c_double), ("sep_thre", C.c_double),
                ("remove_moving", C.c_int)]


class SessionStep(C.Structure):
    """ndt_session_step (include/ndt_mi355x.h): one session's record of one lockstep step."""
    _fields_ = [("pose", C.c_double * 3), ("cov", C.c_double * 9), ("cost", C.c_double), ("stepped", C.c_int),
                ("matched", C.c_int), ("successful", C.c_int), ("status", C.c_int), ("submap", C.c_int),
                ("split", C.c_int)]


class SessionsStats(C.Structure):
    """ndt_sessions_stats (include/ndt_mi355x.h): transfers and host waits of the most recent step."""
    _fields_ = [("h2d_bytes", C.c_uint64), ("d2h_bytes", C.c_uint64), ("host_waits", C.c_int),
                ("triples_run", C.c_int), ("sessions_stepped", C.c_int)]


SESSION_STEP_DTYPE = np.dtype(SessionStep)           # (numpy reads a Structure's layout: written once)


class PoseLattice(C.Structure):
    """ndt_pose_lattice (include/ndt_mi355x.h): index = (k * ny + j) * nx + i, pose = origin + (i, j, k) * step."""
    _fields_ = [("x0", C.c_double), ("y0", C.c_double), ("yaw0", C.c_double), ("step_x", C.c_double), ("step_y", C.c_double),
                ("step_yaw", C.c_double), ("nx", C.c_int), ("ny", C.c_int), ("nyaw", C.c_int)]

    @property
    def size(self):
        """ndt_lattice_size (host only); raises NdtError for a lattice the library refuses."""
        n = C.c_uint64()
        _check(lib().ndt_lattice_size(C.byref(self), C.byref(n)), "ndt_lattice_size")
        return n.value

    def pose(self, index):
        """ndt_lattice_pose (host only): the definition of the lattice's poses."""
        p = (C.c_double * 3)()
        _check(lib().ndt_lattice_pose(C.byref(self), int(index), p), "ndt_lattice_pose")
        return np.array(p[:])

    def poses(self, indices=None):
        """[len, 3] float64 lattice poses of `indices` (default: all), through ndt_lattice_pose."""
        idx = range(self.size) if indices is None else indices
        return np.array([self.pose(i) for i in idx], dtype=np.float64).reshape(-1, 3)


class RelocParams(C.Structure):
    """ndt_reloc_params (include/ndt_mi355x.h)."""
    _fields_ = [("lattice", PoseLattice), ("top_k", C.c_int), ("local_max", C.c_int)]


class ScoreJob(C.Structure):
    """ndt_score_job (include/ndt_mi355x.h): one (map, scan, lattice) of a multi-job sweep or pick."""
    _fields_ = [("map", C.c_int), ("scan", C.c_int), ("lattice", PoseLattice)]


def score_jobs(jobs):
    """[(map index, scan index, PoseLattice)] -> (ScoreJob array, vol_offsets [len + 1] uint64: the running sum of the
    lattice sizes, in poses)."""
    arr = (ScoreJob * len(jobs))(*[ScoreJob(int(m), int(sc), lat) for m, sc, lat in jobs])
    vol = np.zeros(len(jobs) + 1, dtype=np.uint64)
    vol[1:] = np.cumsum([lat.size for _, _, lat in jobs], dtype=np.uint64)
    return arr, vol


class FitStats(C.Structure):
    """ndt_fit_stats (include/ndt_mi355x.h): one match's getFitnessScore(max_range) and its counts."""
    _fields_ = [("fitness", C.c_double), ("fitness_all", C.c_double), ("n_in", C.c_uint32), ("n_dist", C.c_uint32),
                ("n_points", C.c_uint32), ("reserved", C.c_uint32)]


FIT_STATS_DTYPE = np.dtype(FitStats)
DBL_MAX = float(np.finfo(np.float64).max)


class OccGeometry(C.Structure):
    """ndt_occ_geometry (include/ndt_mi355x.h): cell (ix, iy) covers [x0 + ix res, x0 + (ix + 1) res) x [y0 + iy res, ...)."""
    _fields_ = [("x0", C.c_double), ("y0", C.c_double), ("res", C.c_double), ("nx", C.c_int), ("ny", C.c_int)]

    def cell(self, x, y):
        """ndt_occ_cell: the (ix, iy) of a point -- the definition the device follows."""
        ix, iy = C.c_int64(), C.c_int64()
        _check(lib().ndt_occ_cell(C.byref(self), float(x), float(y), C.byref(ix), C.byref(iy)), "ndt_occ_cell")
        return ix.value, iy.value


class OccStats(C.Structure):
    """ndt_occ_stats: one integrate call's counts."""
    _fields_ = [("n_beams", C.c_uint64), ("n_hit", C.c_uint64), ("n_pass", C.c_uint64), ("n_skipped", C.c_uint64)]


OCC_STATS_DTYPE = np.dtype(OccStats)


class PgEdge(C.Structure):
    """ndt_pg_edge (include/ndt_mi355x.h): one arc of a pose graph."""
    _fields_ = [("from_", C.c_int32), ("to", C.c_int32), ("rel", C.c_double * 3), ("info", C.c_double * 6)]


class PgParams(C.Structure):
    """ndt_pg_params (include/ndt_mi355x.h)."""
    _fields_ = [("max_iter", C.c_int), ("eps_step", C.c_double), ("cg_max_iter", C.c_int), ("cg_rtol", C.c_double),
                ("max_halvings", C.c_int)]


class PgRobustParams(C.Structure):
    """ndt_pg_robust_params (include/ndt_mi355x.h): the pose-graph parameters and the level schedule."""
    _fields_ = [("pg", PgParams), ("mu0", C.c_double), ("factor", C.c_double), ("eps_level", C.c_double), ("level_iter", C.c_int)]


NDT_LOOP_MAX_CAND = 8


class LoopParams(C.Structure):
    """ndt_loop_params (include/ndt_mi355x.h)."""
    _fields_ = [("min_path", C.c_double), ("radius", C.c_double), ("step_xy", C.c_double), ("step_yaw", C.c_double),
                ("half_x", C.c_int), ("half_y", C.c_int), ("half_yaw", C.c_int), ("top_k", C.c_int), ("local_max", C.c_int),
                ("max_cost", C.c_double), ("info", C.c_double * 6)]


class LoopCandidate(C.Structure):
    """ndt_loop_candidate (include/ndt_mi355x.h): what the search of one session will run on."""
    _fields_ = [("session", C.c_int), ("submap", C.c_int), ("anchor_scan", C.c_int), ("newest_scan", C.c_int),
                ("nearest_scan", C.c_int), ("dist", C.c_double), ("path", C.c_double), ("lattice", PoseLattice)]


class Loop(C.Structure):
    """ndt_loop (include/ndt_mi355x.h): one candidate's search result."""
    _fields_ = [("cand", LoopCandidate), ("status", C.c_int), ("found", C.c_int), ("n_cand", C.c_int), ("best", C.c_int),
                ("cand_index", C.c_uint64 * NDT_LOOP_MAX_CAND), ("cand_score", C.c_double * NDT_LOOP_MAX_CAND),
                ("cand_cost", C.c_double * NDT_LOOP_MAX_CAND), ("pose", C.c_double * 3), ("edge", PgEdge)]


NDT_LOOP_MAX_SUBMAPS = 4


class LoopMultiParams(C.Structure):
    """ndt_loop_multi_params (include/ndt_mi355x.h): the loop search over several submaps per session."""
    _fields_ = [("loop", LoopParams), ("max_submaps", C.c_int), ("reserved", C.c_int), ("max_d2", C.c_double),
                ("min_overlap", C.c_double)]


class LoopMulti(C.Structure):
    """ndt_loop_multi (include/ndt_mi355x.h): one candidate's search result with its slots' ranged statistics."""
    _fields_ = [("loop", Loop), ("fit", FitStats * NDT_LOOP_MAX_CAND), ("rank", C.c_int), ("reserved", C.c_int)]


class CrossTrack(C.Structure):
    """ndt_cross_track (include/ndt_mi355x.h): one trajectory whose closed submaps may be searched."""
    _fields_ = [("poses", C.c_void_p), ("n_scans", C.c_size_t), ("sub_first", C.c_void_p), ("sub_anchor", C.c_void_p),
                ("sub_offsets", C.c_void_p), ("n_submaps", C.c_int)]


class CrossCandidate(C.Structure):
    """ndt_cross_candidate (include/ndt_mi355x.h): a closed submap of another track that a searcher's newest scan is near."""
    _fields_ = [("cand", LoopCandidate), ("map_session", C.c_int), ("rank", C.c_int), ("d2", C.c_double)]


class CrossLoop(C.Structure):
    """ndt_cross_loop (include/ndt_mi355x.h): one cross candidate's search result."""
    _fields_ = [("m", LoopMulti), ("map_session", C.c_int), ("reserved", C.c_int)]


class PlaceParams(C.Structure):
    """ndt_place_params (include/ndt_mi355x.h): the place descriptor's geometry and the match's selection."""
    _fields_ = [("ring_width", C.c_double), ("r_min", C.c_double), ("n_rings", C.c_int), ("min_pts", C.c_int), ("min_key", C.c_int),
                ("top_k", C.c_int), ("centre_stride", C.c_int), ("reserved", C.c_int)]


class PlaceHit(C.Structure):
    """ndt_place_hit (include/ndt_mi355x.h): one item a query's descriptor matched, at its best descriptor and shift."""
    _fields_ = [(n, C.c_int) for n in ("item", "desc", "shift", "key", "overlap", "n_query", "n_entry", "rank")]


class PlaceCandidate(C.Structure):
    """ndt_place_candidate (include/ndt_mi355x.h): a closed submap of another session that a searcher's local map resembles."""
    _fields_ = [(n, C.c_int) for n in ("session", "map_session", "submap", "centre_scan", "shift", "key", "overlap", "n_query",
                                       "n_entry", "rank")] + [("guess", C.c_double * 3)]


NDT_PLACE_SECTORS, NDT_PLACE_MAX_RINGS, NDT_PLACE_MAX_TOP_K = 64, 32, 16
PLACE_HIT_DTYPE = np.dtype(PlaceHit)
PLACE_CANDIDATE_DTYPE = np.dtype(PlaceCandidate)
LOOP_CANDIDATE_DTYPE = np.dtype(LoopCandidate)
CROSS_CANDIDATE_DTYPE = np.dtype(CrossCandidate)
CROSS_LOOP_DTYPE = np.dtype(CrossLoop)
LOOP_DTYPE = np.dtype(Loop)                          # (its edge's first field is from_, as PgEdge's)
LOOP_MULTI_DTYPE = np.dtype(LoopMulti)

# (hand-written: the C field is `from`, a Python keyword, so the Structure's is from_)
PG_EDGE_DTYPE = np.dtype([("from", "i4"), ("to", "i4"), ("rel", "f8", 3), ("info", "f8", 6)], align=True)
PG_RESULT_DTYPE = np.dtype([("cost_initial", "f8"), ("cost_final", "f8"), ("iterations", "i4"), ("cg_iterations", "i4"),
                            ("converged", "i4"), ("status", "i4")], align=True)
PG_ROBUST_RESULT_DTYPE = np.dtype([("pg", PG_RESULT_DTYPE), ("mu0", "f8"), ("levels", "i4"), ("n_robust", "i4"), ("n_rejected", "i4"),
                                   ("pad", "i4")], align=True)
PG_QUERY_DTYPE = np.dtype([("graph", "i4"), ("a", "i4"), ("b", "i4"), ("pad", "i4")], align=True)
PG_MARGINAL_DTYPE = np.dtype([("Saa", "f8", 9), ("Sab", "f8", 9), ("Sbb", "f8", 9), ("cg_iterations", "i4"), ("converged", "i4"),
                              ("status", "i4"), ("pad", "i4")], align=True)


class MapInfo(C.Structure):
    _fields_ = [("min_bx", C.c_int), ("min_by", C.c_int), ("div_x", C.c_int), ("div_y", C.c_int),
                ("n_cells", C.c_int), ("n_valid", C.c_int), ("n_points", C.c_size_t)]


# ndt_result as a numpy record (same layout as the C struct)
RESULT_DTYPE = np.dtype([
    ("pose", "f8", 3), ("T00", "f4"), ("T10", "f4"), ("T03", "f4"), ("T13", "f4"),
    ("fitness", "f8"), ("trans_prob", "f8"), ("score", "f8"), ("H", "f8", 9), ("p", "f8", 3),
    ("iters", "i4"), ("evals", "i4"), ("ref_evals", "i4"), ("converged", "i4"), ("status", "i4"),
    ("flags", "i4"), ("kbar", "f8")], align=True)
RESULT_BYTES = RESULT_DTYPE.itemsize
FLAG_WINDOW_SPILL, FLAG_REGION_CLIPPED, FLAG_UNSORTED = 1, 2, 4      # ndt_result.flags
NDT_OK, NDT_E_ARG, NDT_E_HIP, NDT_E_NO_DEVICE, NDT_E_GRID, NDT_E_NOMEM = 0, -1, -2, -3, -4, -5    # ndt_status
OPT_MAX_HELPERS, OPT_WORKGROUPS, OPT_INJECT_FAULT, OPT_DEFER_FITNESS, OPT_SCORE_STAGE = 1, 2, 3, 4, 5     # ndt_ctx_set_option
SCORE_STAGE_POINTS = 8000            # the score sweep stages scans up to this many points in LDS (kScoreStagePts, ndt_score.hip.h)

_vp, _sz, _i, _f, _d, _u32, _u64, _P = C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_double, C.c_uint32, C.c_uint64, C.POINTER

# Every function of include/ndt_mi355x.h, in the header's order, with its argtypes: the one place a new entry point is
# declared (tests/test_capi_binding.py holds each entry to the header's declaration).
PROTOTYPES = {
    "ndt_default_params": [_P(Params)],
    "ndt_params_pcl110": [_P(Params)],
    "ndt_params_pcl18": [_P(Params)],
    "ndt_params_pcl_new": [_P(Params)],
    "ndt_ctx_create": [_i, _P(_vp)],
    "ndt_ctx_destroy": [_vp],
    "ndt_last_error": [_vp],
    "ndt_ctx_stream": [_vp],
    "ndt_ctx_set_option": [_vp, _i, C.c_longlong],
    "ndt_ctx_set_stream": [_vp, _vp],
    "ndt_map_build": [_vp, _vp, _sz, _sz, _P(Params), _P(_vp)],
    "ndt_map_build_dev": [_vp, _vp, _sz, _sz, _P(Params), _P(_vp)],
    "ndt_map_rebuild_begin": [_vp, _vp, _sz, _sz, _P(Params), _vp],
    "ndt_map_rebuild_end": [_vp, _vp],
    "ndt_map_build_batch_dev": [_vp, _vp, _vp, _sz, _i, _vp, _vp],
    "ndt_map_build_batch": [_vp, _vp, _vp, _sz, _i, _vp, _vp],
    "ndt_map_destroy": [_vp],
    "ndt_map_info_get": [_vp, _P(MapInfo)],
    "ndt_map_export": [_vp, _vp, _vp, _vp, _vp, _vp],
    "ndt_align": [_vp, _vp, _vp, _sz, _sz, _vp, _vp],
    "ndt_align_batch": [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp],
    "ndt_align_batch_dev": [_vp, _vp, _vp, _vp, _i, _sz, _i, _vp, _vp, _vp],
    "ndt_align_batch_prepare_dev": [_vp, _vp, _vp, _vp, _i, _sz, _i, _vp, _vp],
    "ndt_prepare_timing": [_vp, _P(_f)],
    "ndt_align_batch_multi_dev": [_vp, _vp, _i, _vp, _vp, _vp, _i, _sz, _i, _vp, _vp, _vp],
    "ndt_align_batch_multi": [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp],
    "ndt_align_batch_sharded": [_vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp],
    "ndt_align_batch_trace": [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp],
    "ndt_eval_at": [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp],
    "ndt_fitness_at": [_vp, _vp, _vp, _sz, _sz, _f, _f, _f, _f, _vp],
    "ndt_prefilter": [_vp, _vp, _sz, _sz, _f, _vp, _P(_sz)],
    "ndt_prefilter_batch_dev": [_vp, _vp, _sz, _vp, _i, _sz, _f, _vp, _vp, _vp],
    "ndt_resample_capacity": [_sz, _d, _d, _P(_sz)],
    "ndt_resample_batch_dev": [_vp, _vp, _sz, _vp, _i, _sz, _d, _d, _vp, _vp, _vp, _vp, _vp],
    "ndt_resample": [_vp, _vp, _sz, _sz, _d, _d, _vp, _P(_sz)],
    "ndt_scan_to_map_batch_dev": [_vp, _vp, _sz, _vp, _i, _sz, _vp, _vp, _vp],
    "ndt_fuse_default_params": [_P(FuseParams)],
    "ndt_predict_batch_dev": [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp],
    "ndt_fuse_batch_dev": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _P(FuseParams), _vp, _vp, _vp, _vp],
    "ndt_remove_neighbors": [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _d, _vp, _P(_sz)],
    "ndt_remove_neighbors_dev": [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _d, _vp, _vp, _vp],
    "ndt_difference_extraction": [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _d, _vp, _P(_sz)],
    "ndt_difference_extraction_dev": [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _d, _vp, _vp, _vp],
    "ndt_make_map": [_vp, _vp, _sz, _vp, _i, _i, _i, _i, _d, _d, _vp, _P(_sz)],
    "ndt_make_map_dev": [_vp, _vp, _sz, _vp, _i, _i, _i, _i, _d, _d, _vp, _vp, _vp],
    "ndt_prefilter_batch": [_vp, _vp, _sz, _vp, _i, _f, _vp, _vp],
    "ndt_local_map_batch_dev": [_vp, _vp, _i, _sz, _f, _vp, _vp, _vp, _vp, _vp, _vp],
    "ndt_local_map_batch": [_vp, _vp, _i, _sz, _f, _vp, _vp, _vp, _vp, _vp],
    "ndt_session_default_params": [_P(SessionParams)],
    "ndt_sessions_create": [_vp, _i, _P(SessionParams), _P(_vp)],
    "ndt_sessions_destroy": [_vp],
    "ndt_sessions_step": [_vp, _vp, _sz, _vp, _vp, _vp, _vp],
    "ndt_sessions_step_dev": [_vp, _vp, _sz, _vp, _vp, _vp, _vp],
    "ndt_sessions_local_map": [_vp, _i, _P(_vp), _P(_sz), _P(_vp)],
    "ndt_sessions_submap_cloud": [_vp, _i, _P(_vp), _P(_sz)],
    "ndt_sessions_global_map": [_vp, _i, _vp, _sz, _P(_sz), _vp, _P(_i)],
    "ndt_sessions_get_stats": [_vp, _P(SessionsStats)],
    "ndt_lattice_size": [_P(PoseLattice), _P(_u64)],
    "ndt_lattice_pose": [_P(PoseLattice), _u64, _vp],
    "ndt_score_poses_dev": [_vp, _vp, _vp, _sz, _sz, _vp, _u64, _vp, _vp, _vp],
    "ndt_score_lattice_dev": [_vp, _vp, _vp, _sz, _sz, _P(PoseLattice), _vp, _vp, _vp],
    "ndt_score_poses": [_vp, _vp, _vp, _sz, _sz, _vp, _u64, _vp, _vp],
    "ndt_lattice_select_dev": [_vp, _P(PoseLattice), _vp, _vp, _i, _i, _vp, _vp, _vp],
    "ndt_relocalize": [_vp, _vp, _vp, _sz, _sz, _P(RelocParams), _vp, _vp, _vp, _P(_i), _P(_i), _vp],
    "ndt_relocalize_dev": [_vp, _vp, _vp, _sz, _sz, _P(RelocParams), _vp, _vp, _vp, _P(_i), _P(_i), _vp],
    "ndt_score_lattice_multi_dev": [_vp, _vp, _i, _vp, _vp, _i, _sz, _vp, _i, _vp, _vp, _vp, _vp],
    "ndt_lattice_select_multi_dev": [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp],
    "ndt_fit_points_batch_dev": [_vp, _vp, _vp, _vp, _i, _sz, _i, _vp, _sz, _d, _vp, _vp, _vp],
    "ndt_fit_points_batch": [_vp, _vp, _vp, _vp, _i, _i, _vp, _sz, _d, _vp, _vp],
    "ndt_fit_points_multi_dev": [_vp, _vp, _i, _vp, _vp, _vp, _i, _sz, _i, _vp, _sz, _d, _vp, _vp, _vp],
    "ndt_fit_points_multi": [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _sz, _d, _vp, _vp],
    "ndt_occ_cell": [_P(OccGeometry), _d, _d, _P(C.c_int64), _P(C.c_int64)],
    "ndt_occ_create": [_vp, _P(OccGeometry), _P(_vp)],
    "ndt_occ_destroy": [_vp],
    "ndt_occ_clear": [_vp, _vp, _vp],
    "ndt_occ_geometry_get": [_vp, _P(OccGeometry)],
    "ndt_occ_view": [_vp, _P(_vp)],
    "ndt_occ_integrate_dev": [_vp, _vp, _i, _vp, _vp, _vp, _i, _sz, _vp, _sz, _d, _vp, _vp],
    "ndt_occ_integrate": [_vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _sz, _d, _vp],
    "ndt_occ_render_dev": [_vp, _vp, _u32, _vp, _vp],
    "ndt_occ_render": [_vp, _vp, _u32, _vp],
    "ndt_occ_counts": [_vp, _vp, _vp, _vp],
    "ndt_sessions_occ_integrate": [_vp, _vp, _vp, _d, _vp],
    "ndt_pg_default_params": [_P(PgParams)],
    "ndt_pg_edge_between": [_vp, _vp, _vp],
    "ndt_pg_info_from_cov": [_vp, _d, _vp],
    "ndt_pg_optimize_batch_dev": [_vp, _vp, _vp, _vp, _vp, _i, _P(PgParams), _vp, _vp],
    "ndt_pg_optimize_batch": [_vp, _vp, _vp, _vp, _vp, _i, _P(PgParams), _vp],
    "ndt_pg_robust_default_params": [_P(PgRobustParams)],
    "ndt_pg_optimize_robust_batch_dev": [_vp, _vp, _vp, _vp, _vp, _i, _vp, _P(PgRobustParams), _vp, _vp, _vp, _vp],
    "ndt_pg_optimize_robust_batch": [_vp, _vp, _vp, _vp, _vp, _i, _vp, _P(PgRobustParams), _vp, _vp, _vp],
    "ndt_pg_marginals_batch_dev": [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _P(PgParams), _vp, _vp],
    "ndt_pg_marginals_batch": [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _P(PgParams), _vp],
    "ndt_pg_relative_cov": [_vp, _vp, _vp, _vp],
    "ndt_pg_edge_chi2": [_vp, _vp, _vp, _vp, _vp],
    "ndt_repose_points_dev": [_vp, _vp, _sz, _vp, _i, _vp, _vp, _vp, _sz, _vp],
    "ndt_repose_points": [_vp, _vp, _sz, _vp, _i, _vp, _vp, _vp, _sz],
    "ndt_sessions_trajectory": [_vp, _i, _vp, _sz, _P(_sz), _vp, _vp, _P(_i), _P(_sz)],
    "ndt_sessions_correct": [_vp, _vp, _i, _vp, _vp, _vp],
    "ndt_loop_default_params": [_P(LoopParams)],
    "ndt_loop_gate": [_vp, _sz, _vp, _vp, _vp, _i, _P(LoopParams), _P(LoopCandidate), _P(_i)],
    "ndt_sessions_loop_candidates": [_vp, _vp, _P(LoopParams), _vp, _P(_i)],
    "ndt_sessions_find_loops": [_vp, _vp, _P(LoopParams), _vp, _P(_i), _vp],
    "ndt_loop_multi_default_params": [_P(LoopMultiParams)],
    "ndt_loop_gate_multi": [_vp, _sz, _vp, _vp, _vp, _i, _P(LoopMultiParams), _vp, _P(_i)],
    "ndt_sessions_loop_candidates_multi": [_vp, _vp, _P(LoopMultiParams), _vp, _P(_i)],
    "ndt_sessions_find_loops_multi": [_vp, _vp, _P(LoopMultiParams), _vp, _P(_i), _vp],
    "ndt_cross_gate": [_vp, _i, _i, _vp, _i, _P(LoopMultiParams), _vp, _P(_i)],
    "ndt_cross_gate_batch": [_vp, _vp, _vp, _vp, _i, _vp, _i, _P(LoopMultiParams), _vp, _vp],
    "ndt_sessions_cross_candidates": [_vp, _vp, _vp, _P(LoopMultiParams), _vp, _P(_i)],
    "ndt_sessions_find_cross_loops": [_vp, _vp, _vp, _P(LoopMultiParams), _vp, _P(_i), _vp],
    "ndt_place_default_params": [_P(PlaceParams)],
    "ndt_place_describe": [_vp, _sz, _sz, _d, _d, _P(PlaceParams), _vp],
    "ndt_place_describe_batch_dev": [_vp, _vp, _sz, _vp, _i, _vp, _vp, _i, _P(PlaceParams), _vp, _vp],
    "ndt_place_describe_batch": [_vp, _vp, _sz, _vp, _i, _vp, _vp, _i, _P(PlaceParams), _vp],
    "ndt_place_key": [_vp, _vp, _i, _i, _P(_i), _P(_i)],
    "ndt_place_match_host": [_vp, _vp, _i, _vp, _vp, _vp, _i, _P(PlaceParams), _vp, _vp, _vp],
    "ndt_place_match_dev": [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _P(PlaceParams), _vp, _vp, _vp, _vp],
    "ndt_place_match": [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _P(PlaceParams), _vp, _vp, _vp],
    "ndt_sessions_place_candidates": [_vp, _vp, _vp, _P(PlaceParams), _vp, _P(_i)],
    "ndt_sessions_archive_enable": [_vp],
    "ndt_sessions_archive_info": [_vp, _i, _P(_sz), _P(_sz)],
    "ndt_sessions_archive_scans": [_vp, _i, _sz, _sz, _vp, _sz, _vp, _P(_sz)],
    "ndt_sessions_archive_view": [_vp, _i, _P(_vp), _P(_sz)],
    "ndt_sessions_occ_rebuild": [_vp, _vp, _vp, _i, _d, _vp],
    "ndt_sessions_remake_closed": [_vp, _vp, _i, _vp],
    "ndt_kernel_timing": [_vp, _i, _P(_f), _P(_f)],
    "ndt_launch_interval": [_vp, _i, _P(_f)],
    "ndt_ctx_wait_launch": [_vp, _i, _vp],
    "ndt_last_timing": [_vp, _P(_f), _P(_f)],
    "ndt_selftest_libm_f32": [_vp, _vp, _sz, _vp, _vp, _vp],
    "ndt_selftest_optimizer": [_vp] + [_vp, _sz, _vp] * 4,
}
RESTYPES = {"ndt_last_error": C.c_char_p, "ndt_ctx_stream": _vp}      # every other function returns an int status
EXPORTS = list(PROTOTYPES)


def lib():
    """Load the shared library; fail loudly when it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise NdtError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    for name, argtypes in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = argtypes, RESTYPES.get(name, _i)
    _LIB = L
    return L


def _error(rc, what, h=None):
    """The NdtError of a failed call: "<what> -> <rc>: <ndt_last_error of the context h, or of the calling thread>"."""
    return NdtError("%s -> %d: %s" % (what, rc, lib().ndt_last_error(h).decode()))


def _check(rc, what):
    """Raise for a non-zero return code of a call that takes no context."""
    if rc:
        raise _error(rc, what)


def _ptr(a):
    """The address of an array's data, NULL for an empty one."""
    return a.ctypes.data if len(a) else None


def pack_scans(scans, dtype=np.float32, width=2, offsets_dtype=np.uint64):
    """A list of [n_i, width] arrays (empty ones allowed) -> (points [N, width] `dtype`, C-contiguous; offsets [len + 1]
    `offsets_dtype`): scan i is points[offsets[i]:offsets[i + 1]].  No scans: a (0, width) array and [0]."""
    scans = [np.ascontiguousarray(x, dtype=dtype).reshape(-1, width) for x in scans]
    off = np.zeros(len(scans) + 1, dtype=offsets_dtype)
    off[1:] = np.cumsum([len(x) for x in scans])
    return (np.ascontiguousarray(np.concatenate(scans)) if scans else np.zeros((0, width), dtype)), off


def _batch_args(scans, offsets, inits):
    """(scans, offsets, inits) of a host align call as contiguous arrays, then B and its zeroed records."""
    inits = np.ascontiguousarray(inits, dtype=np.float64).reshape(-1, 3)
    return _f32c(scans), np.ascontiguousarray(offsets, dtype=np.uint64), inits, len(inits), np.zeros(len(inits), dtype=RESULT_DTYPE)


def _defaults(struct, fn, kw, nested=()):
    """struct() as the C function `fn` fills it, fields overridden by keyword (AttributeError for an unknown one).  A
    keyword <name>_<field> with name in `nested` reaches the struct nested under that name, which itself is not replaced."""
    p = struct()
    getattr(lib(), fn)(C.byref(p))
    for k, v in kw.items():
        head, _, tail = k.partition("_")
        obj, field = (getattr(p, head), tail) if head in nested and hasattr(getattr(p, head), tail) else (p, k)
        if k in nested or not hasattr(obj, field):
            raise AttributeError(k)
        setattr(obj, field, v)
    return p


class _Handle:
    """The owner of a C handle `h` that the library function named `_destroy` frees: close() frees it once, h = C.c_void_p()
    gives it up without freeing."""
    _destroy = None
    h = None

    def close(self):
        if self.h:
            getattr(lib(), self._destroy)(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        # at interpreter shutdown the HIP runtime may already be gone: leave the handles to the OS
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


PRESETS = {"default": "ndt_default_params", "pcl110": "ndt_params_pcl110", "pcl18": "ndt_params_pcl18",
           "pcl_new": "ndt_params_pcl_new"}


def default_params(preset="default", **kw):
    """ndt_params of a PCL-version preset (include/ndt_mi355x.h), fields overridden by keyword."""
    return _defaults(Params, PRESETS[preset], kw)


def align_batch_sharded(maps, scans, offsets, inits, shared_scan=False, partial=False):
    """ndt_align_batch_sharded: `maps` = one Map per device (each with its own Context), the batch on the host.
    `partial`: return (rc, records) instead of raising when a shard failed -- every record of a failed shard carries
    that shard's error in `status`, the others are complete."""
    scans, offsets, inits, B, res = _batch_args(scans, offsets, inits)
    n = len(maps)
    cx = (C.c_void_p * n)(*[m.ctx.h for m in maps])
    mp = (C.c_void_p * n)(*[m.h for m in maps])
    rc = lib().ndt_align_batch_sharded(cx, mp, n, scans.ctypes.data, offsets.ctypes.data, B, int(shared_scan),
                                       inits.ctypes.data, res.ctypes.data)
    if partial:
        return rc, res
    _check(rc, "ndt_align_batch_sharded")
    return res


def _map_handles(maps):
    """(ndt_map *)[n] of a list of Map objects (None entries pass as NULL)."""
    n = len(maps)
    return (C.c_void_p * max(n, 1))(*[(m.h if m is not None else None) for m in maps]), n


def align_batch_multi(ctx, maps, scans, offsets, inits, map_of=None, shared_scan=False):
    """ndt_align_batch_multi: match b against maps[map_of[b]] (map_of None: maps[b], one map per match) in one launch on
    `ctx`; records in the format of Map.align_batch.  A map_of entry outside [0, len(maps)) gives that record alone
    status NDT_E_ARG (zeroed, fitness DBL_MAX)."""
    scans, offsets, inits, B, res = _batch_args(scans, offsets, inits)
    mp, n = _map_handles(maps)
    mo = None if map_of is None else np.ascontiguousarray(map_of, dtype=np.int32)
    if mo is not None and len(mo) != B:
        raise ValueError("map_of needs one entry per match")
    ctx.check(lib().ndt_align_batch_multi(ctx.h, mp, n, None if mo is None else mo.ctypes.data, scans.ctypes.data,
                                          offsets.ctypes.data, B, int(shared_scan), inits.ctypes.data, res.ctypes.data),
              "ndt_align_batch_multi")
    return res


def _build_batch(ctx, fn, ptrs, ns, stride, params, maps):
    """ndt_map_build_batch{,_dev}: the call's arrays from Python lists; existing maps rebuilt in place, new ones adopted."""
    S = len(ptrs)
    prms = list(params) if isinstance(params, (list, tuple)) else [params] * S
    maps = list(maps) if maps is not None else [None] * S
    if len(prms) != S or len(maps) != S:
        raise ValueError("build_maps: one Params (or one for all) and one map slot per cloud")
    k = max(S, 1)
    xy = (C.c_void_p * k)(*ptrs)
    n = (C.c_size_t * k)(*ns)
    P = (Params * k)(*prms)
    mp = (C.c_void_p * k)(*[(m.h if m is not None else None) for m in maps])
    ctx.check(getattr(lib(), fn)(ctx.h, xy, n, stride, S, P, mp), fn)
    out = []
    for s in range(S):
        if maps[s] is None:
            out.append(Map.adopt(ctx, mp[s], prms[s]))
        else:
            maps[s].params = prms[s]
            out.append(maps[s])
    return out


def build_maps(ctx, clouds, params, maps=None):
    """ndt_map_build_batch: map s from clouds[s] ([n, 2] float32) with params (one Params for all, or a list), in one set
    of launches on `ctx`.  `maps`: a list of Map or None per cloud (None: all new); existing maps are rebuilt in place, new
    ones created.  Returns the list of Map, in the order of `clouds`."""
    clouds = [_f32c(c) for c in clouds]
    return _build_batch(ctx, "ndt_map_build_batch", [_ptr(c) for c in clouds],
                        [len(c) for c in clouds], 8, params, maps)


def resample_capacity(total_points, space, space_thre):
    """ndt_resample_capacity: the output bound (in points) of the resampler for total_points raw points.  Needs no
    context and no device; raises NdtError on refused parameters."""
    cap = C.c_size_t()
    _check(lib().ndt_resample_capacity(int(total_points), float(space), float(space_thre), C.byref(cap)), "ndt_resample_capacity")
    return cap.value


def default_fuse_params(**kw):
    """ndt_fuse_default_params, fields overridden by keyword."""
    return _defaults(FuseParams, "ndt_fuse_default_params", kw)


def default_session_params(**kw):
    """ndt_session_default_params (the launch file's values), fields overridden by keyword; match_* and fuse_* reach the
    nested ndt_params / ndt_fuse_params (match_resolution=0.5, fuse_score_thre=1.0)."""
    return _defaults(SessionParams, "ndt_session_default_params", kw, nested=("match", "fuse"))


def session_params_from_launch(params):
    """ndt_session_params of a dict of launch-file parameters (replay.LAUNCH_PARAMS' names)."""
    q = params
    return default_session_params(
        match_resolution=q["Resolution"], match_step_size=q["StepSize"], match_trans_eps=q["TransformationEpsilon"],
        match_max_iter=q["MaximumIterations"], fuse_coe_ndt_cov=q["coeNDTCov"], fuse_coe_vel=q["coeVel"],
        fuse_coe_omega=q["coeOmega"], fuse_del_time=q["delTime"], fuse_score_thre=q["score_thre"], space=q["space"],
        space_thre=q["space_thre"], leaf=q["LeafSize"], resol=q["resol"], thre_neighbor=q["thre_neighbor"],
        sep_thre=q["sepThre"], remove_moving=int(bool(q["removeMoving"])))


def default_pg_params(**kw):
    """ndt_pg_default_params, fields overridden by keyword."""
    return _defaults(PgParams, "ndt_pg_default_params", kw)


def default_pg_robust_params(**kw):
    """ndt_pg_robust_default_params; mu0, factor, eps_level and level_iter by keyword, pg_<field> reaches the nested
    ndt_pg_params (pg_max_iter=50)."""
    return _defaults(PgRobustParams, "ndt_pg_robust_default_params", kw, nested=("pg",))


def default_loop_params(**kw):
    """ndt_loop_default_params, fields overridden by keyword (info: six numbers)."""
    info = kw.pop("info", None)
    p = _defaults(LoopParams, "ndt_loop_default_params", kw)
    if info is not None:
        p.info[:] = [float(v) for v in info]
    return p


def loop_gate(poses, sub_first, sub_anchor, sub_offsets, params):
    """ndt_loop_gate (host only): the candidate of one trajectory -- Sessions.trajectory's poses, sub_first and sub_anchor, the
    closed clouds' offsets in points (len(sub_first) + 1 entries) -- as a LOOP_CANDIDATE_DTYPE record, or None."""
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    first, anchor = np.ascontiguousarray(sub_first, dtype=np.int32), np.ascontiguousarray(sub_anchor, dtype=np.int32)
    off = np.ascontiguousarray(sub_offsets, dtype=np.uint64)
    if len(anchor) != len(first) or len(off) != len(first) + 1:
        raise ValueError("loop_gate needs one sub_anchor per submap and one more sub_offsets")
    out, has = np.zeros(1, dtype=LOOP_CANDIDATE_DTYPE), C.c_int()
    _check(lib().ndt_loop_gate(_ptr(poses), len(poses), _ptr(first), _ptr(anchor), off.ctypes.data, len(first), C.byref(params),
                               out.ctypes.data_as(_P(LoopCandidate)), C.byref(has)), "ndt_loop_gate")
    return out[0] if has.value else None


def default_loop_multi_params(**kw):
    """ndt_loop_multi_default_params; max_submaps, max_d2 and min_overlap by keyword, every other keyword a field of its
    `loop` part (info: six numbers)."""
    own = {k: kw.pop(k) for k in ("max_submaps", "max_d2", "min_overlap") if k in kw}
    p = _defaults(LoopMultiParams, "ndt_loop_multi_default_params", own)
    info = kw.pop("info", None)
    for k, v in kw.items():
        if not hasattr(p.loop, k):
            raise AttributeError("ndt_loop_params has no field %r" % k)
        setattr(p.loop, k, v)
    if info is not None:
        p.loop.info[:] = [float(v) for v in info]
    return p


def loop_gate_multi(poses, sub_first, sub_anchor, sub_offsets, params):
    """ndt_loop_gate_multi (host only): loop_gate with up to params.max_submaps candidates, nearest first, as
    LOOP_CANDIDATE_DTYPE records (possibly none)."""
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    first, anchor = np.ascontiguousarray(sub_first, dtype=np.int32), np.ascontiguousarray(sub_anchor, dtype=np.int32)
    off = np.ascontiguousarray(sub_offsets, dtype=np.uint64)
    if len(anchor) != len(first) or len(off) != len(first) + 1:
        raise ValueError("loop_gate_multi needs one sub_anchor per submap and one more sub_offsets")
    out, n = np.zeros(NDT_LOOP_MAX_SUBMAPS, dtype=LOOP_CANDIDATE_DTYPE), C.c_int()
    _check(lib().ndt_loop_gate_multi(_ptr(poses), len(poses), _ptr(first), _ptr(anchor), off.ctypes.data, len(first), C.byref(params),
                                     out.ctypes.data, C.byref(n)), "ndt_loop_gate_multi")
    return out[:n.value]


def _cross_tracks(tracks):
    """Tracks given as (poses, sub_first, sub_anchor, sub_offsets) -> (the CrossTrack array, the arrays it points into)."""
    keep, arr = [], (CrossTrack * max(len(tracks), 1))()
    for t, (poses, sub_first, sub_anchor, sub_offsets) in enumerate(tracks):
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        first, anchor = np.ascontiguousarray(sub_first, dtype=np.int32), np.ascontiguousarray(sub_anchor, dtype=np.int32)
        off = np.ascontiguousarray(sub_offsets, dtype=np.uint64)
        if len(anchor) != len(first) or len(off) != len(first) + 1:
            raise ValueError("track %d needs one sub_anchor per submap and one more sub_offsets" % t)
        keep.append((poses, first, anchor, off))
        arr[t] = CrossTrack(poses.ctypes.data, len(poses), first.ctypes.data, anchor.ctypes.data, off.ctypes.data, len(first))
    return arr, keep


def cross_gate(last_pose, newest_scan, own, tracks, params):
    """ndt_cross_gate (host only): the closed submaps of the other tracks -- each (poses, sub_first, sub_anchor, sub_offsets) as
    loop_gate takes them -- that lie within params.loop.radius of last_pose, nearest first, as CROSS_CANDIDATE_DTYPE records."""
    last = np.ascontiguousarray(last_pose, dtype=np.float64).reshape(3)
    arr, keep = _cross_tracks(tracks)
    out, n = np.zeros(NDT_LOOP_MAX_SUBMAPS, dtype=CROSS_CANDIDATE_DTYPE), C.c_int()
    _check(lib().ndt_cross_gate(last.ctypes.data, int(newest_scan), int(own), C.addressof(arr), len(tracks), C.byref(params),
                                out.ctypes.data, C.byref(n)), "ndt_cross_gate")
    return out[:n.value]


def cross_gate_batch(ctx, last_poses, newest_scan, own, tracks, params):
    """ndt_cross_gate_batch: cross_gate for many searchers in one upload, two launches and one read-back -> a list with one
    array of CROSS_CANDIDATE_DTYPE records per searcher (cand.session = the searcher's index), byte for byte cross_gate's."""
    last = np.ascontiguousarray(last_poses, dtype=np.float64).reshape(-1, 3)
    newest, own = np.ascontiguousarray(newest_scan, dtype=np.int32), np.ascontiguousarray(own, dtype=np.int32)
    if len(newest) != len(last) or len(own) != len(last):
        raise ValueError("cross_gate_batch needs one newest_scan and one own per searcher")
    arr, keep = _cross_tracks(tracks)
    K = params.max_submaps if 1 <= params.max_submaps <= NDT_LOOP_MAX_SUBMAPS else NDT_LOOP_MAX_SUBMAPS
    out, n = np.zeros((max(len(last), 1), K), dtype=CROSS_CANDIDATE_DTYPE), np.zeros(max(len(last), 1), dtype=np.int32)
    ctx.check(lib().ndt_cross_gate_batch(ctx.h, _ptr(last), _ptr(newest), _ptr(own), len(last), C.addressof(arr), len(tracks),
                                         C.byref(params), out.ctypes.data, n.ctypes.data), "ndt_cross_gate_batch")
    return [out[i, :n[i]] for i in range(len(last))]


def default_place_params(**kw):
    """ndt_place_default_params, fields overridden by keyword."""
    return _defaults(PlaceParams, "ndt_place_default_params", kw)


def _place_clouds(clouds, stride):
    """Clouds ([n_i, 2] float32 each, empty ones allowed) packed `stride` bytes apart (8, or 16 with two unused floats per
    point) -> (the packed array, offsets in points)."""
    pts, off = pack_scans(clouds)
    if stride == 16:
        wide = np.zeros((len(pts), 4), dtype=np.float32)
        wide[:, :2] = pts
        pts = wide
    return pts, off


def _place_centres(centres, cloud_of):
    centres = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1, 2)
    cloud_of = np.ascontiguousarray(cloud_of, dtype=np.int32)
    if len(cloud_of) != len(centres):
        raise ValueError("one cloud_of per centre")
    return centres, cloud_of


def place_describe(xy, centre, params, stride=8):
    """ndt_place_describe (host only, the definition): the descriptor of one cloud about `centre` -> [n_rings] uint64."""
    pts, _ = _place_clouds([xy], stride)
    desc = np.zeros(max(params.n_rings, 1), dtype=np.uint64)
    _check(lib().ndt_place_describe(_ptr(pts), len(pts), stride, float(centre[0]), float(centre[1]), C.byref(params), desc.ctypes.data),
           "ndt_place_describe")
    return desc


def place_describe_batch(ctx, clouds, centres, cloud_of, params, stride=8):
    """ndt_place_describe_batch: descriptor k of clouds[cloud_of[k]] about centres[k], in one upload and one launch ->
    [n_desc, n_rings] uint64, byte for byte place_describe's."""
    pts, off = _place_clouds(clouds, stride)
    centres, cloud_of = _place_centres(centres, cloud_of)
    desc = np.zeros((len(centres), max(params.n_rings, 1)), dtype=np.uint64)
    ctx.check(lib().ndt_place_describe_batch(ctx.h, _ptr(pts), stride, off.ctypes.data, len(off) - 1, _ptr(centres), _ptr(cloud_of),
                                             len(centres), C.byref(params), _ptr(desc)), "ndt_place_describe_batch")
    return desc


def place_describe_batch_dev(ctx, xy_ptr, stride, offsets, centres, cloud_of, params, desc_ptr, stream=None):
    """ndt_place_describe_batch_dev: device addresses of the points and of the descriptors; offsets, centres and cloud_of host
    arrays."""
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    centres, cloud_of = _place_centres(centres, cloud_of)
    ctx.check(lib().ndt_place_describe_batch_dev(ctx.h, xy_ptr, stride, off.ctypes.data, len(off) - 1, _ptr(centres), _ptr(cloud_of),
                                                 len(centres), C.byref(params), desc_ptr, stream), "ndt_place_describe_batch_dev")


def place_key(q_desc, d_desc, shift):
    """ndt_place_key (host only): (key, overlap) of a query descriptor against an entry at one shift."""
    q, d = np.ascontiguousarray(q_desc, dtype=np.uint64), np.ascontiguousarray(d_desc, dtype=np.uint64)
    if q.shape != d.shape or q.ndim != 1:
        raise ValueError("place_key needs two descriptors of one length")
    key, c = C.c_int(), C.c_int()
    _check(lib().ndt_place_key(_ptr(q), _ptr(d), len(q), int(shift), C.byref(key), C.byref(c)), "ndt_place_key")
    return key.value, c.value


def _place_match_args(q_desc, q_group, d_desc, item_first, item_group, params):
    R = params.n_rings if 1 <= params.n_rings <= NDT_PLACE_MAX_RINGS else 1        # (outside: the library refuses)
    q, d =np.ascontiguousarray(q_desc, dtype=np.uint64).reshape(-1, R), np.ascontiguousarray(d_desc, dtype=np.uint64).reshape(-1, R)
    qg, first = np.ascontiguousarray(q_group, dtype=np.int32), np.ascontiguousarray(item_first, dtype=np.int32)
    group = np.ascontiguousarray(item_group, dtype=np.int32)
    if len(qg) != len(q) or len(first) != len(group) + 1 or (len(first) and int(first[-1]) > len(d)):
        raise ValueError("place match: one group per query, one more item_first than items, item_first within the descriptors")
    K = params.top_k if 1 <= params.top_k <= NDT_PLACE_MAX_TOP_K else NDT_PLACE_MAX_TOP_K
    table = np.zeros((len(q), len(group)), dtype=np.uint64)
    out, n = np.zeros((max(len(q), 1), K), dtype=PLACE_HIT_DTYPE), np.zeros(max(len(q), 1), dtype=np.int32)
    return q, qg, d, first, group, table, out, n


def place_match_host(q_desc, q_group, d_desc, item_first, item_group, params):
    """ndt_place_match_host (host only, the definition) -> (hits [n_q, top_k] PLACE_HIT_DTYPE, n [n_q], table [n_q, n_items])."""
    q, qg, d, first, group, table, out, n = _place_match_args(q_desc, q_group, d_desc, item_first, item_group, params)
    _check(lib().ndt_place_match_host(_ptr(q), _ptr(qg), len(q), _ptr(d), first.ctypes.data, _ptr(group), len(group), C.byref(params),
                                      _ptr(table.reshape(-1)), out.ctypes.data, n.ctypes.data), "ndt_place_match_host")
    return out[:len(q)], n[:len(q)], table


def place_match(ctx, q_desc, q_group, d_desc, item_first, item_group, params):
    """ndt_place_match: place_match_host on the device (one table upload, two launches), byte for byte."""
    q, qg, d, first, group, table, out, n = _place_match_args(q_desc, q_group, d_desc, item_first, item_group, params)
    ctx.check(lib().ndt_place_match(ctx.h, _ptr(q), _ptr(qg), len(q), _ptr(d), first.ctypes.data, _ptr(group), len(group), C.byref(params),
                                    _ptr(table.reshape(-1)), out.ctypes.data, n.ctypes.data), "ndt_place_match")
    return out[:len(q)], n[:len(q)], table


def place_match_dev(ctx, q_desc_ptr, q_group, d_desc_ptr, item_first, item_group, params, out_ptr, n_out_ptr, table_ptr=None, stream=None):
    """ndt_place_match_dev: device addresses of the descriptors and the outputs; the groups and item_first host arrays."""
    qg, first = np.ascontiguousarray(q_group, dtype=np.int32), np.ascontiguousarray(item_first, dtype=np.int32)
    group = np.ascontiguousarray(item_group, dtype=np.int32)
    ctx.check(lib().ndt_place_match_dev(ctx.h, q_desc_ptr, _ptr(qg), len(qg), d_desc_ptr, first.ctypes.data, _ptr(group), len(group),
                                        C.byref(params), table_ptr, out_ptr, n_out_ptr, stream), "ndt_place_match_dev")


def pg_edge_between(from_pose, to_pose):
    """ndt_pg_edge_between: Pose2D::calMotion(to, from) -> the arc's rel (tx, ty, th[deg])."""
    a = np.ascontiguousarray(from_pose, dtype=np.float64).reshape(3)
    b = np.ascontiguousarray(to_pose, dtype=np.float64).reshape(3)
    e = np.zeros(1, dtype=PG_EDGE_DTYPE)
    _check(lib().ndt_pg_edge_between(a.ctypes.data, b.ctypes.data, e.ctypes.data), "ndt_pg_edge_between")
    return e[0]["rel"].copy()


def pg_info_from_cov(cov_world, th_deg):
    """ndt_pg_info_from_cov: a world-frame 3 x 3 covariance seen from the frame at heading th_deg, inverted -> info[6]."""
    cov = np.ascontiguousarray(cov_world, dtype=np.float64).reshape(9)
    info = np.zeros(6, dtype=np.float64)
    _check(lib().ndt_pg_info_from_cov(cov.ctypes.data, float(th_deg), info.ctypes.data), "ndt_pg_info_from_cov")
    return info


def optimize_pose_graphs(ctx, poses, node_offsets, edges, edge_offsets, params=None):
    """ndt_pg_optimize_batch: graph g = the pose triples [node_offsets[g], node_offsets[g + 1]) of `poses` ([n, 3] float64,
    th in degrees) and the arcs [edge_offsets[g], edge_offsets[g + 1]) of `edges` (PG_EDGE_DTYPE) -> (new poses, one
    PG_RESULT_DTYPE record per graph).  `poses` itself is not changed."""
    out = np.array(poses, dtype=np.float64, order="C").reshape(-1, 3)
    edges = np.ascontiguousarray(edges, dtype=PG_EDGE_DTYPE)
    no = np.ascontiguousarray(node_offsets, dtype=np.uint64)
    eo = np.ascontiguousarray(edge_offsets, dtype=np.uint64)
    G = len(no) - 1
    if len(eo) != len(no):
        raise ValueError("node_offsets and edge_offsets need one entry per graph, plus one")
    pad_p = out if out.size else np.zeros((1, 3), dtype=np.float64)            # (an address for a batch without nodes)
    pad_e = edges if edges.size else np.zeros(1, dtype=PG_EDGE_DTYPE)
    res = np.zeros(max(G, 1), dtype=PG_RESULT_DTYPE)
    prm = params if params is not None else default_pg_params()
    ctx.check(lib().ndt_pg_optimize_batch(ctx.h, pad_p.ctypes.data, no.ctypes.data, pad_e.ctypes.data, eo.ctypes.data, G, C.byref(prm),
                                          res.ctypes.data), "ndt_pg_optimize_batch")
    return out, res[:G]


def optimize_pose_graphs_dev(ctx, poses_ptr, node_offsets, edges_ptr, edge_offsets, out_ptr, params=None, stream=None):
    """ndt_pg_optimize_batch_dev: device addresses of poses, arcs and records, HOST offset arrays; asynchronous on `stream`."""
    no = np.ascontiguousarray(node_offsets, dtype=np.uint64)
    eo = np.ascontiguousarray(edge_offsets, dtype=np.uint64)
    prm = params if params is not None else default_pg_params()
    ctx.check(lib().ndt_pg_optimize_batch_dev(ctx.h, poses_ptr, no.ctypes.data, edges_ptr, eo.ctypes.data, len(no) - 1, C.byref(prm),
                                              out_ptr, stream), "ndt_pg_optimize_batch_dev")


def optimize_pose_graphs_robust(ctx, poses, node_offsets, edges, edge_offsets, phi=None, params=None):
    """ndt_pg_optimize_robust_batch: optimize_pose_graphs with a robust cost on the arcs whose `phi` (one float64 per arc, None:
    no robust arc) is above 0 -> (new poses, one PG_ROBUST_RESULT_DTYPE record per graph, every arc's weight at mu = 1 at the
    final poses, every arc's chi-square there).  A robust arc is rejected when its chi2 is above its phi (weight below 1/4)."""
    out = np.array(poses, dtype=np.float64, order="C").reshape(-1, 3)
    edges = np.ascontiguousarray(edges, dtype=PG_EDGE_DTYPE)
    no = np.ascontiguousarray(node_offsets, dtype=np.uint64)
    eo = np.ascontiguousarray(edge_offsets, dtype=np.uint64)
    G = len(no) - 1
    if len(eo) != len(no):
        raise ValueError("node_offsets and edge_offsets need one entry per graph, plus one")
    if phi is not None:
        phi = np.ascontiguousarray(phi, dtype=np.float64).reshape(-1)
        if len(phi) != len(edges):
            raise ValueError("phi needs one entry per arc")
    pad_p = out if out.size else np.zeros((1, 3), dtype=np.float64)            # (an address for a batch without nodes)
    pad_e = edges if edges.size else np.zeros(1, dtype=PG_EDGE_DTYPE)
    res = np.zeros(max(G, 1), dtype=PG_ROBUST_RESULT_DTYPE)
    w, c = np.zeros(max(len(edges), 1), dtype=np.float64), np.zeros(max(len(edges), 1), dtype=np.float64)
    prm = params if params is not None else default_pg_robust_params()
    ctx.check(lib().ndt_pg_optimize_robust_batch(ctx.h, pad_p.ctypes.data, no.ctypes.data, pad_e.ctypes.data, eo.ctypes.data, G,
                                                 phi.ctypes.data if phi is not None and len(phi) else None, C.byref(prm),
                                                 res.ctypes.data, w.ctypes.data, c.ctypes.data), "ndt_pg_optimize_robust_batch")
    return out, res[:G], w[:len(edges)], c[:len(edges)]


def optimize_pose_graphs_robust_dev(ctx, poses_ptr, node_offsets, edges_ptr, edge_offsets, out_ptr, phi_ptr=None, weight_ptr=None,
                                    chi2_ptr=None, params=None, stream=None):
    """ndt_pg_optimize_robust_batch_dev: device addresses of poses, arcs, records and (each or None) phi, weights and chi2; HOST
    offset arrays; asynchronous on `stream`."""
    no = np.ascontiguousarray(node_offsets, dtype=np.uint64)
    eo = np.ascontiguousarray(edge_offsets, dtype=np.uint64)
    prm = params if params is not None else default_pg_robust_params()
    ctx.check(lib().ndt_pg_optimize_robust_batch_dev(ctx.h, poses_ptr, no.ctypes.data, edges_ptr, eo.ctypes.data, len(no) - 1, phi_ptr,
                                                     C.byref(prm), out_ptr, weight_ptr, chi2_ptr, stream),
              "ndt_pg_optimize_robust_batch_dev")


def pg_queries(queries):
    """(graph, a, b) rows, or PG_QUERY_DTYPE records -> a contiguous PG_QUERY_DTYPE array."""
    if isinstance(queries, np.ndarray) and queries.dtype == PG_QUERY_DTYPE:
        return np.ascontiguousarray(queries)
    rows = np.asarray(queries, dtype=np.int64).reshape(-1, 3)
    q = np.zeros(len(rows), dtype=PG_QUERY_DTYPE)
    q["graph"], q["a"], q["b"] = rows[:, 0], rows[:, 1], rows[:, 2]
    return q


def pose_graph_marginals(ctx, poses, node_offsets, edges, edge_offsets, queries, weight=None, params=None):
    """ndt_pg_marginals_batch: blocks of the covariance H^-1 (node 0 fixed) of the graphs as optimize_pose_graphs takes them, at
    the poses given.  queries: (graph, a, b) rows or PG_QUERY_DTYPE; weight: one float64 per arc (optimize_pose_graphs_robust's
    weights), None: all 1 -> one PG_MARGINAL_DTYPE record per query (Saa, Sab, Sbb row-major 3 x 3 in (m, m, rad))."""
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    edges = np.ascontiguousarray(edges, dtype=PG_EDGE_DTYPE)
    no = np.ascontiguousarray(node_offsets, dtype=np.uint64)
    eo = np.ascontiguousarray(edge_offsets, dtype=np.uint64)
    if len(eo) != len(no):
        raise ValueError("node_offsets and edge_offsets need one entry per graph, plus one")
    if weight is not None:
        weight = np.ascontiguousarray(weight, dtype=np.float64).reshape(-1)
        if len(weight) != len(edges):
            raise ValueError("weight needs one entry per arc")
    q = pg_queries(queries)
    pad_p = poses if poses.size else np.zeros((1, 3), dtype=np.float64)        # (an address for a batch without nodes)
    pad_e = edges if edges.size else np.zeros(1, dtype=PG_EDGE_DTYPE)
    out = np.zeros(max(len(q), 1), dtype=PG_MARGINAL_DTYPE)
    prm = params if params is not None else default_pg_params()
    ctx.check(lib().ndt_pg_marginals_batch(ctx.h, pad_p.ctypes.data, no.ctypes.data, pad_e.ctypes.data, eo.ctypes.data, len(no) - 1,
                                           weight.ctypes.data if weight is not None and len(weight) else None, _ptr(q), len(q),
                                           C.byref(prm), out.ctypes.data), "ndt_pg_marginals_batch")
    return out[:len(q)]


def pose_graph_marginals_dev(ctx, poses_ptr, node_offsets, edges_ptr, edge_offsets, queries, out_ptr, weight_ptr=None, params=None,
                             stream=None):
    """ndt_pg_marginals_batch_dev: device addresses of poses, arcs, records and (or None) weights; HOST offsets and queries;
    asynchronous on `stream`."""
    no = np.ascontiguousarray(node_offsets, dtype=np.uint64)
    eo = np.ascontiguousarray(edge_offsets, dtype=np.uint64)
    q = pg_queries(queries)
    prm = params if params is not None else default_pg_params()
    ctx.check(lib().ndt_pg_marginals_batch_dev(ctx.h, poses_ptr, no.ctypes.data, edges_ptr, eo.ctypes.data, len(no) - 1, weight_ptr,
                                               _ptr(q), len(q), C.byref(prm), out_ptr, stream), "ndt_pg_marginals_batch_dev")


def pg_relative_cov(pose_a, pose_b, marginal):
    """ndt_pg_relative_cov: the first-order covariance of pose_b in pose_a's frame from a query's record -> [3, 3]."""
    a = np.ascontiguousarray(pose_a, dtype=np.float64).reshape(3)
    b = np.ascontiguousarray(pose_b, dtype=np.float64).reshape(3)
    m = np.zeros(1, dtype=PG_MARGINAL_DTYPE)
    m[0] = marginal
    cov = np.zeros(9, dtype=np.float64)
    _check(lib().ndt_pg_relative_cov(a.ctypes.data, b.ctypes.data, m.ctypes.data, cov.ctypes.data), "ndt_pg_relative_cov")
    return cov.reshape(3, 3)


def pg_edge_chi2(pose_a, pose_b, edge, rel_cov):
    """ndt_pg_edge_chi2: r^T (rel_cov + Omega^-1)^-1 r of an arc (a record with rel and info) from pose_a to pose_b."""
    a = np.ascontiguousarray(pose_a, dtype=np.float64).reshape(3)
    b = np.ascontiguousarray(pose_b, dtype=np.float64).reshape(3)
    e = np.zeros(1, dtype=PG_EDGE_DTYPE)
    e[0]["rel"], e[0]["info"] = edge["rel"], edge["info"]
    cov = np.ascontiguousarray(rel_cov, dtype=np.float64).reshape(9)
    d2 = C.c_double()
    _check(lib().ndt_pg_edge_chi2(a.ctypes.data, b.ctypes.data, e.ctypes.data, cov.ctypes.data, C.byref(d2)), "ndt_pg_edge_chi2")
    return d2.value


def repose_points(ctx, xy, seg_offsets, old_poses, new_poses, out=None):
    """ndt_repose_points: segment k = the points [seg_offsets[k], seg_offsets[k + 1]) of `xy` ([n, >= 2] float32, the first two
    of each row), moved from old_poses[k] to new_poses[k] ([K, 3] float64) -> a new array like xy (out=None), or written into
    `out` (which may be xy itself)."""
    if not (isinstance(xy, np.ndarray) and xy.dtype == np.float32 and xy.ndim == 2 and xy.shape[1] >= 2 and xy.flags.c_contiguous):
        xy = np.ascontiguousarray(np.asarray(xy, dtype=np.float32).reshape(len(xy), -1))
    if out is None:
        out = xy.copy()
    if not (out.dtype == np.float32 and out.ndim == 2 and out.shape[1] >= 2 and out.flags.c_contiguous and len(out) == len(xy)):
        raise ValueError("out needs to be a C-contiguous float32 array with xy's rows")
    off = np.ascontiguousarray(seg_offsets, dtype=np.uint64)
    po = np.ascontiguousarray(old_poses, dtype=np.float64).reshape(-1, 3)
    pn = np.ascontiguousarray(new_poses, dtype=np.float64).reshape(-1, 3)
    K = len(off) - 1
    if len(po) != K or len(pn) != K:
        raise ValueError("old_poses and new_poses need one row per segment")
    if K and int(off[-1]) > len(xy):
        raise ValueError("seg_offsets reach past the points")
    a = xy if xy.size else np.zeros((1, 2), dtype=np.float32)
    b = out if out.size else np.zeros((1, 2), dtype=np.float32)
    ctx.check(lib().ndt_repose_points(ctx.h, a.ctypes.data, a.strides[0], off.ctypes.data, K, po.ctypes.data, pn.ctypes.data, b.ctypes.data,
                                      b.strides[0]), "ndt_repose_points")
    return out


def repose_points_dev(ctx, xy_ptr, stride, seg_offsets_ptr, n_segs, old_poses_ptr, new_poses_ptr, out_ptr, out_stride, stream=None):
    """ndt_repose_points_dev: device addresses; asynchronous on `stream` (None: the context's)."""
    ctx.check(lib().ndt_repose_points_dev(ctx.h, xy_ptr, stride, seg_offsets_ptr, n_segs, old_poses_ptr, new_poses_ptr, out_ptr, out_stride,
                                          stream), "ndt_repose_points_dev")


def _f32c(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("expected an [n, 2] float32 array")
    return a


def _tf4(tf):
    """[B, 4] float32 (c, s, tx, ty) of a [B, 4] array or of align_batch's records (T00, T10, T03, T13)."""
    tf = np.asarray(tf)
    if tf.dtype.names is not None:
        tf = np.stack([tf["T00"], tf["T10"], tf["T03"], tf["T13"]], axis=-1)
    tf = np.ascontiguousarray(tf, dtype=np.float32)
    if tf.ndim != 2 or tf.shape[1] != 4:
        raise ValueError("expected a [B, 4] float32 array of (c, s, tx, ty) or a record array")
    return tf


def fit_points_multi(ctx, maps, scans, offsets, tf, map_of=None, max_d2=DBL_MAX, shared_scan=False, want_d2=True, want_stats=True):
    """ndt_fit_points_multi: Map.fit_points with match b searched in maps[map_of[b]] (map_of None: maps[b], one map per match),
    in one search launch and one close launch on `ctx` -> (d2 float32 or None, stats FIT_STATS_DTYPE [B] or None).  A map_of
    entry outside [0, len(maps)) gives that match alone +inf distances and stats (DBL_MAX, DBL_MAX, 0, 0, n_points, 0)."""
    scans = _f32c(scans)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    tf = _tf4(tf)
    B = len(tf)
    nscan = 1 if shared_scan else B
    if len(offsets) != nscan + 1:
        raise ValueError("offsets needs one entry per scan and one more")
    mo = None if map_of is None else np.ascontiguousarray(map_of, dtype=np.int32)
    if mo is not None and len(mo) != B:
        raise ValueError("map_of needs one entry per match")
    mp, n = _map_handles(maps)
    n_d2 = B * int(offsets[1] - offsets[0]) if shared_scan else int(offsets[-1])
    d2 = np.zeros(n_d2, dtype=np.float32) if want_d2 else None
    stats = np.zeros(B, dtype=FIT_STATS_DTYPE) if want_stats else None
    ctx.check(lib().ndt_fit_points_multi(ctx.h, mp, n, None if mo is None else mo.ctypes.data, scans.ctypes.data, offsets.ctypes.data,
                                         B, int(shared_scan), tf.ctypes.data, 16, float(max_d2), d2.ctypes.data if want_d2 else None,
                                         stats.ctypes.data if want_stats else None), "ndt_fit_points_multi")
    return d2, stats


def rerank(records, stats):
    """Index of the lowest `converged ? ranged fitness : 1e7` over a relocalisation's records and their FIT_STATS_DTYPE of
    one fit_points call; ties to the higher n_in, then the lower index.  -1 for no records."""
    best, key = -1, None
    for c in range(len(records)):
        k = (float(stats[c]["fitness"]) if records[c]["converged"] else 1e7, -int(stats[c]["n_in"]), c)
        if key is None or k < key:
            best, key = c, k
    return best


class Context(_Handle):
    """ndt_ctx: one per process and device."""
    _destroy = "ndt_ctx_destroy"

    def __init__(self, device=0):
        self.h = C.c_void_p()
        _check(lib().ndt_ctx_create(device, C.byref(self.h)), "ndt_ctx_create(%d)" % device)
        self.device = device

    def check(self, rc, what):
        if rc:
            raise _error(rc, what, self.h)

    @property
    def stream(self):
        return lib().ndt_ctx_stream(self.h)

    def set_stream(self, stream):
        """Order all work of this context on a caller-owned hipStream_t (int handle or None)."""
        self.check(lib().ndt_ctx_set_stream(self.h, stream), "ndt_ctx_set_stream")

    def set_option(self, option, value):
        """ndt_ctx_set_option: OPT_MAX_HELPERS (0 = no work sharing), OPT_WORKGROUPS (0 = one per CU)."""
        self.check(lib().ndt_ctx_set_option(self.h, option, value), "ndt_ctx_set_option")

    def wait_launch(self, back, stream=None):
        """ndt_ctx_wait_launch: `stream` (int handle; None = the context's stream) waits for the match launch `back`
        launches ago (0 = the most recent), fitness kernels included -- no event record on the launch's stream."""
        self.check(lib().ndt_ctx_wait_launch(self.h, back, stream), "ndt_ctx_wait_launch")

    def prefilter(self, xy, leaf):
        """pcl::ApproximateVoxelGrid on one scan ([n, 2] float32) -> filtered [m, 2] float32."""
        xy = _f32c(xy)
        out = np.empty_like(xy)
        m = C.c_size_t()
        self.check(lib().ndt_prefilter(self.h, xy.ctypes.data, len(xy), 8, leaf, out.ctypes.data, C.byref(m)),
                   "ndt_prefilter")
        return out[:m.value].copy()

    def prefilter_batch_dev(self, raw_ptr, stride, raw_offsets_ptr, B, total_raw_points, leaf, out_ptr,
                            out_offsets_ptr, stream=None):
        """Device pointers in and out (see include/ndt_mi355x.h); asynchronous."""
        self.check(lib().ndt_prefilter_batch_dev(self.h, raw_ptr, stride, raw_offsets_ptr, B, total_raw_points, leaf,
                                                 out_ptr, out_offsets_ptr, stream), "ndt_prefilter_batch_dev")

    def prefilter_batch(self, scans, leaf):
        """ndt_prefilter_batch: the pre-filter of every scan of a list ([n_b, 2] float32 each, empty ones allowed) in one
        call -> the list of filtered scans, each what prefilter gives for it."""
        allp, off = pack_scans(scans)
        B = len(off) - 1
        if not B:
            return []
        out = np.empty((len(allp) + 1, 2), dtype=np.float32)
        ooff = np.zeros(B + 1, dtype=np.uint64)
        self.check(lib().ndt_prefilter_batch(self.h, _ptr(allp), 8, off.ctypes.data, B, leaf,
                                             out.ctypes.data, ooff.ctypes.data), "ndt_prefilter_batch")
        return [out[int(ooff[b]):int(ooff[b + 1])].copy() for b in range(B)]

    def resample(self, xy, space, space_thre):
        """ScanPointResampler::resamplePoints on one scan ([n, 2] float64) -> resampled [m, 2] float64."""
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        out = np.empty((resample_capacity(len(xy), space, space_thre), 2), dtype=np.float64)
        m = C.c_size_t()
        self.check(lib().ndt_resample(self.h, _ptr(xy), len(xy), 16, space, space_thre, _ptr(out), C.byref(m)), "ndt_resample")
        return out[:m.value].copy()

    def resample_batch_dev(self, raw_ptr, stride, raw_offsets_ptr, B, total_raw_points, space, space_thre, out64_ptr,
                           out32_ptr, out_offsets_ptr, status_ptr=None, stream=None):
        """Device pointers in and out (see include/ndt_mi355x.h; outputs sized by resample_capacity); asynchronous."""
        self.check(lib().ndt_resample_batch_dev(self.h, raw_ptr, stride, raw_offsets_ptr, B, total_raw_points, space,
                                                space_thre, out64_ptr, out32_ptr, out_offsets_ptr, status_ptr, stream),
                   "ndt_resample_batch_dev")

    def scan_to_map_batch_dev(self, xy_ptr, stride, offsets_ptr, B, total_points, poses_ptr, out_ptr, stream=None):
        """growMap's transform for a batch: device pointers (doubles in, B x 3 poses in degrees, float2 out); asynchronous."""
        self.check(lib().ndt_scan_to_map_batch_dev(self.h, xy_ptr, stride, offsets_ptr, B, total_points, poses_ptr,
                                                   out_ptr, stream), "ndt_scan_to_map_batch_dev")

    def remove_neighbors(self, base, point_list, thre_neighbor):
        """PCFilter::remove_neighborPoint: base points with no list point within thre_neighbor, in order."""
        base = _f32c(base)
        lst = np.ascontiguousarray(point_list, dtype=np.float32).reshape(-1, 2)
        out = np.empty_like(base)
        m = C.c_size_t()
        self.check(lib().ndt_remove_neighbors(self.h, base.ctypes.data, 8, len(base), _ptr(lst), 8, len(lst), thre_neighbor,
                                              out.ctypes.data, C.byref(m)),
                   "ndt_remove_neighbors")
        return out[:m.value].copy()

    def difference_extraction(self, base, test, resol):
        """PCFilter::difference_extraction: points of `test` in octree voxels `base` does not occupy (input order)."""
        base = np.ascontiguousarray(base, dtype=np.float32).reshape(-1, 2)
        test = np.ascontiguousarray(test, dtype=np.float32).reshape(-1, 2)
        out = np.empty((len(test) + 1, 2), dtype=np.float32)
        m = C.c_size_t()
        self.check(lib().ndt_difference_extraction(self.h, _ptr(base), 8, len(base), _ptr(test), 8, len(test), resol,
                                                   out.ctypes.data, C.byref(m)), "ndt_difference_extraction")
        return out[:m.value].copy()

    def make_map(self, scans, first_submap, newest, remove_moving=True, resol=0.05, thre_neighbor=0.1):
        """Submap::makeMap over a list of (n_i, 2) float32 scans in the map frame -> (n, 2) float32."""
        allp, off = pack_scans(scans)
        n_scans = len(off) - 1
        out = np.empty(((2 if n_scans == 1 else 1) * len(allp) + 1, 2), dtype=np.float32)
        m = C.c_size_t()
        self.check(lib().ndt_make_map(self.h, allp.ctypes.data, 8, off.ctypes.data, n_scans, int(first_submap),
                                      int(newest), int(remove_moving), resol, thre_neighbor, out.ctypes.data,
                                      C.byref(m)), "ndt_make_map")
        return out[:m.value].copy()

    def make_map_dev(self, scans_ptr, stride, offsets, first_submap, newest, remove_moving, resol, thre_neighbor,
                     out_ptr, n_out_ptr, stream=None):
        """Device pointers for the points, the result and its uint64 count; `offsets` a host uint64 array."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.check(lib().ndt_make_map_dev(self.h, scans_ptr, stride, off.ctypes.data, len(off) - 1, int(first_submap),
                                          int(newest), int(remove_moving), resol, thre_neighbor, out_ptr, n_out_ptr,
                                          stream), "ndt_make_map_dev")

    def local_maps(self, items, leaf):
        """ndt_local_map_batch: Submap::makeMap and makeLocalMap's cloud for many submaps in one call.  An item is
        (scans, first_submap, newest, remove_moving, resol, thre_neighbor, prev_cloud): `scans` as make_map takes them,
        prev_cloud the p_cloud of the submap before it ([n, 2] float32) or None.  Returns per item (p_cloud, target,
        n_prev): p_cloud what make_map gives, target = prev_cloud followed by prefilter(p_cloud, leaf) (its first n_prev
        points are prev_cloud).  Raises NdtError for a failed item (a scan triple beyond 2^30 voxels), as make_map does."""
        items = list(items)
        if not items:
            return []
        S = len(items)
        descs = (SubmapDesc * S)()
        keep = []                                            # the arrays the descriptors point into
        cap_cloud = cap_prev = 0
        for s, (scans, first, newest, remove, resol, thre, prev) in enumerate(items):
            allp, off = pack_scans(scans)
            n_scans = len(off) - 1
            if len(allp) == 0:
                allp = np.zeros((1, 2), np.float32)          # (a non-NULL address for a submap without points)
            pv = np.zeros((0, 2), np.float32) if prev is None else np.ascontiguousarray(prev, dtype=np.float32).reshape(-1, 2)
            keep.append((allp, off, pv))
            descs[s] = SubmapDesc(allp.ctypes.data, off.ctypes.data, n_scans, int(first), int(newest), int(remove),
                                  float(resol), float(thre), _ptr(pv), len(pv))
            cap_cloud += (2 if n_scans == 1 else 1) * int(off[-1])
            cap_prev += len(pv)
        cloud = np.empty((cap_cloud + 1, 2), dtype=np.float32)
        target = np.empty((cap_cloud + cap_prev + 1, 2), dtype=np.float32)
        coff, toff = np.zeros(S + 1, dtype=np.uint64), np.zeros(S + 1, dtype=np.uint64)
        status = np.zeros(S, dtype=np.int32)
        self.check(lib().ndt_local_map_batch(self.h, descs, S, 8, leaf, cloud.ctypes.data, coff.ctypes.data,
                                             target.ctypes.data, toff.ctypes.data, status.ctypes.data),
                   "ndt_local_map_batch")
        bad = np.flatnonzero(status)
        if len(bad):
            raise NdtError("ndt_local_map_batch -> %d: submap %d: a scan triple spans more than 2^30 voxels"
                           % (int(status[bad[0]]), int(bad[0])))
        return [(cloud[int(coff[s]):int(coff[s + 1])].copy(), target[int(toff[s]):int(toff[s + 1])].copy(), len(keep[s][2]))
                for s in range(S)]

    def repose_points(self, clouds, old_poses, new_poses):
        """ndt_repose_points over a list of [n_k, 2] float32 clouds, cloud k moved from old_poses[k] to new_poses[k] (each
        (tx, ty, th[deg])) -> the list of moved clouds (new arrays): replay.PointCloudMap.remakeMaps' point move."""
        clouds = list(clouds)
        if not clouds:
            return []
        allp, off = pack_scans(clouds)
        moved = repose_points(self, allp, off, old_poses, new_poses)
        return [moved[int(off[k]):int(off[k + 1])].copy() for k in range(len(clouds))]

    def local_maps_dev(self, descs, leaf, cloud_ptr, cloud_off_ptr, target_ptr, target_off_ptr, status_ptr, stride=8,
                       stream=None):
        """ndt_local_map_batch_dev: `descs` a list of SubmapDesc (or a ctypes array of them) whose scans_xy / prev_xy are
        device addresses and whose offsets are host arrays; every other pointer a device address (target_ptr and
        target_off_ptr may both be None: the clouds alone); asynchronous."""
        n = len(descs)
        if isinstance(descs, (list, tuple)):
            descs = (SubmapDesc * max(n, 1))(*descs)
        self.check(lib().ndt_local_map_batch_dev(self.h, descs, n, stride, leaf, cloud_ptr, cloud_off_ptr, target_ptr,
                                                 target_off_ptr, status_ptr, stream), "ndt_local_map_batch_dev")

    def predict_batch_dev(self, odo_cur_ptr, odo_prev_ptr, last_pose_ptr, B, motion_ptr, pred_ptr, init_ptr=None,
                          stream=None):
        """Row f2, before the match: device pointers to B x 3 doubles (degrees); asynchronous."""
        self.check(lib().ndt_predict_batch_dev(self.h, odo_cur_ptr, odo_prev_ptr, last_pose_ptr, B, motion_ptr, pred_ptr,
                                               init_ptr, stream), "ndt_predict_batch_dev")

    def fuse_batch_dev(self, results_ptr, pred_ptr, motion_ptr, last_pose_ptr, last_cov_ptr, B, prm, fused_ptr, cov_ptr,
                       successful_ptr=None, stream=None):
        """Row f2, after the match: device pointers; asynchronous."""
        self.check(lib().ndt_fuse_batch_dev(self.h, results_ptr, pred_ptr, motion_ptr, last_pose_ptr, last_cov_ptr, B,
                                            C.byref(prm), fused_ptr, cov_ptr, successful_ptr, stream),
                   "ndt_fuse_batch_dev")

    def align_batch_multi_dev(self, maps, map_of_ptr, scans_ptr, offsets_ptr, B, total_points, inits_ptr, out_ptr,
                              shared_scan=False, stream=None):
        """ndt_align_batch_multi_dev: `maps` a list of Map objects (of any context of this device), map_of_ptr a device
        array of B int32 or None (match b against maps[b]); every other pointer a device address; asynchronous."""
        mp, n = _map_handles(maps)
        self.check(lib().ndt_align_batch_multi_dev(self.h, mp, n, map_of_ptr, scans_ptr, offsets_ptr, B, total_points,
                                                   int(shared_scan), inits_ptr, out_ptr, stream),
                   "ndt_align_batch_multi_dev")

    def fit_points_multi_dev(self, maps, map_of_ptr, scans_ptr, offsets_ptr, B, total_points, tf_ptr, tf_stride, max_d2, d2_ptr,
                             stats_ptr, shared_scan=False, stream=None):
        """ndt_fit_points_multi_dev: `maps` a list of Map objects, map_of_ptr a device array of B int32 or None (match b in
        maps[b]); every other pointer a device address (d2_ptr or stats_ptr may be None); asynchronous."""
        mp, n = _map_handles(maps)
        self.check(lib().ndt_fit_points_multi_dev(self.h, mp, n, map_of_ptr, scans_ptr, offsets_ptr, B, total_points, int(shared_scan),
                                                  tf_ptr, tf_stride, float(max_d2), d2_ptr, stats_ptr, stream),
                   "ndt_fit_points_multi_dev")

    def score_lattice_multi_dev(self, maps, scans_ptr, offsets_ptr, n_scans, total_points, jobs, score_ptr, pairs_ptr=None,
                                stream=None):
        """ndt_score_lattice_multi_dev: `maps` a list of Map objects, `jobs` a list of (map index, scan index, PoseLattice);
        every pointer a device address; asynchronous.  Returns vol_offsets (uint64, len(jobs) + 1): job j's volume is
        score[vol_offsets[j]:vol_offsets[j + 1]]."""
        mp, n = _map_handles(maps)
        arr, vol = score_jobs(jobs)
        self.check(lib().ndt_score_lattice_multi_dev(self.h, mp, n, scans_ptr, offsets_ptr, int(n_scans), int(total_points), arr, len(jobs),
                                                     score_ptr, pairs_ptr, vol.ctypes.data, stream), "ndt_score_lattice_multi_dev")
        return vol

    def lattice_select_multi_dev(self, jobs, score_ptr, pairs_ptr, top_k, local_max, cand_ptr, n_cand_ptr, stream=None):
        """ndt_lattice_select_multi_dev on the volumes of score_lattice_multi_dev's `jobs`: cand_ptr len(jobs) x top_k uint64,
        n_cand_ptr len(jobs) int32 (device addresses); asynchronous."""
        arr, vol = score_jobs(jobs)
        self.check(lib().ndt_lattice_select_multi_dev(self.h, arr, len(jobs), score_ptr, pairs_ptr, vol.ctypes.data, int(top_k),
                                                      int(local_max), cand_ptr, n_cand_ptr, stream), "ndt_lattice_select_multi_dev")

    def build_maps_dev(self, xy_ptrs, ns, params, maps=None, stride=8):
        """ndt_map_build_batch_dev: capi.build_maps with device cloud pointers (xy_ptrs[s], ns[s] points at `stride` bytes);
        asynchronous on this context's stream (the clouds must stay as they are until it has run)."""
        return _build_batch(self, "ndt_map_build_batch_dev", list(xy_ptrs), list(ns), stride, params, maps)

    def selftest_libm_f32(self, yaws):
        """Device cosf / sinf / initial yaw (ndt_libm_f32.hip.h) for an array of float32 yaws -> (cos, sin, init_yaw)."""
        y = np.ascontiguousarray(yaws, dtype=np.float32).ravel()
        c, s, y0 = np.zeros_like(y), np.zeros_like(y), np.zeros_like(y)
        self.check(lib().ndt_selftest_libm_f32(self.h, y.ctypes.data, len(y), c.ctypes.data, s.ctypes.data, y0.ctypes.data),
                   "ndt_selftest_libm_f32")
        return c, s, y0

    def selftest_optimizer(self, solve3=None, mt_trial=None, mt_update=None, yaw=None):
        """ndt_selftest_optimizer: rows through the device functions of ndt_optimizer.hip.h.  solve3 [n, 9] (Hxx Hxy Hxt Hyy Hyt
        Htt b0 b1 b2) -> [n, 3]; mt_trial [n, 9] -> [n]; mt_update [n, 9] -> [n, 7] (the six interval values, the return
        value); yaw [n, 2] float32 (T00, T10) -> [n].  Returns a dict with the parts that were given."""
        args, outs = [], {}
        for name, rows, dt, width, out_shape in (("solve3", solve3, np.float64, 9, (3,)), ("mt_trial", mt_trial, np.float64, 9, ()),
                                                 ("mt_update", mt_update, np.float64, 9, (7,)), ("yaw", yaw, np.float32, 2, ())):
            if rows is None or len(rows) == 0:
                args += [None, 0, None]
                continue
            a = np.ascontiguousarray(rows, dtype=dt).reshape(-1, width)
            o = np.zeros((len(a),) + out_shape, np.float64)
            outs[name] = (a, o)
            args += [a.ctypes.data, len(a), o.ctypes.data]
        self.check(lib().ndt_selftest_optimizer(self.h, *args), "ndt_selftest_optimizer")
        return {k: v[1] for k, v in outs.items()}

    def last_timing(self):
        a, b = C.c_float(), C.c_float()
        lib().ndt_last_timing(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def kernel_timing(self, back=0):
        """(match kernel ms, fitness kernels ms) of one of this context's last 64 launches; blocks until it is done."""
        a, b = C.c_float(), C.c_float()
        self.check(lib().ndt_kernel_timing(self.h, back, C.byref(a), C.byref(b)), "ndt_kernel_timing")
        return a.value, b.value

    def prepare_timing(self):
        """ms of the kernel of the prepared batch(es) this context's launches used (0.0: none)."""
        a = C.c_float()
        self.check(lib().ndt_prepare_timing(self.h, C.byref(a)), "ndt_prepare_timing")
        return a.value

    def launch_interval(self, back=0):
        """ms from the start of the match kernel of launch back + 1 to the start of launch back (both among the last 64)."""
        a = C.c_float()
        self.check(lib().ndt_launch_interval(self.h, back, C.byref(a)), "ndt_launch_interval")
        return a.value


class Sessions(_Handle):
    """ndt_sessions: n device-resident SLAM sessions stepped together (include/ndt_mi355x.h)."""
    _destroy = "ndt_sessions_destroy"

    def __init__(self, ctx, n_sessions, params=None, archive=False):
        """archive: ndt_sessions_archive_enable -- every stepped scan is kept on the device (robot frame, fp64) for occ_rebuild."""
        self.ctx = ctx
        self.params = params if params is not None else default_session_params()
        self.n = int(n_sessions)
        self.h = C.c_void_p()
        ctx.check(lib().ndt_sessions_create(ctx.h, self.n, C.byref(self.params), C.byref(self.h)), "ndt_sessions_create")
        if archive:
            ctx.check(lib().ndt_sessions_archive_enable(self.h), "ndt_sessions_archive_enable")

    def _active(self, active):
        if active is None:
            return None
        a = np.ascontiguousarray(active, dtype=np.uint8)
        if len(a) != self.n:
            raise ValueError("active needs one entry per session")
        return a

    def step(self, scans, odo, active=None):
        """ndt_sessions_step: scans = one [n_i, 2] float64 raw scan per session (empty ones allowed), odo = [S, 3]
        (tx, ty, th[deg]) -> the S records as a numpy array of SESSION_STEP_DTYPE."""
        allp, off = pack_scans(scans, dtype=np.float64)
        if len(off) - 1 != self.n:
            raise ValueError("step needs one scan per session")
        odo = np.ascontiguousarray(odo, dtype=np.float64).reshape(self.n, 3)
        a = self._active(active)
        out = np.zeros(self.n, dtype=SESSION_STEP_DTYPE)
        self.ctx.check(lib().ndt_sessions_step(self.h, _ptr(allp), 16, off.ctypes.data,
                                               odo.ctypes.data, None if a is None else a.ctypes.data, out.ctypes.data),
                       "ndt_sessions_step")
        return out

    def step_dev(self, raw_ptr, stride, raw_offsets, odo_ptr, active=None):
        """ndt_sessions_step_dev: device addresses of the raw scans and the odometry; `raw_offsets` a host uint64 array."""
        off = np.ascontiguousarray(raw_offsets, dtype=np.uint64)
        a = self._active(active)
        out = np.zeros(self.n, dtype=SESSION_STEP_DTYPE)
        self.ctx.check(lib().ndt_sessions_step_dev(self.h, raw_ptr, stride, off.ctypes.data, odo_ptr,
                                                   None if a is None else a.ctypes.data, out.ctypes.data),
                       "ndt_sessions_step_dev")
        return out

    def local_map(self, i):
        """(device address, points, ndt_map handle or None) of session i's local map; valid until the next step."""
        p, n, m = C.c_void_p(), C.c_size_t(), C.c_void_p()
        self.ctx.check(lib().ndt_sessions_local_map(self.h, i, C.byref(p), C.byref(n), C.byref(m)), "ndt_sessions_local_map")
        return p.value, n.value, m.value

    def submap_cloud(self, i):
        """(device address, points) of session i's current Submap::p_cloud; valid until the next step."""
        p, n = C.c_void_p(), C.c_size_t()
        self.ctx.check(lib().ndt_sessions_submap_cloud(self.h, i, C.byref(p), C.byref(n)), "ndt_sessions_submap_cloud")
        return p.value, n.value

    def map_export(self, i):
        """ndt_map_export of session i's map (the set keeps owning it), or None before it has one."""
        _, _, m = self.local_map(i)
        if not m:
            return None
        view = Map.adopt(self.ctx, m, self.params.match)
        try:
            return view.export()
        finally:
            view.h = C.c_void_p()                      # not ours to destroy

    def global_map(self, i):
        """ndt_sessions_global_map: (globalMap_cloud [n, 2] float32, [each submap's cloud]) as makeGlobalMap leaves them."""
        n, k = C.c_size_t(), C.c_int()
        self.ctx.check(lib().ndt_sessions_global_map(self.h, i, None, 0, C.byref(n), None, C.byref(k)), "ndt_sessions_global_map")
        out = np.zeros((n.value, 2), dtype=np.float32)
        off = np.zeros(k.value + 1, dtype=np.uint64)
        self.ctx.check(lib().ndt_sessions_global_map(self.h, i, _ptr(out), n.value, C.byref(n),
                                                     off.ctypes.data, C.byref(k)), "ndt_sessions_global_map")
        return out, [out[int(off[j]):int(off[j + 1])] for j in range(k.value)]

    def occ_integrate(self, grids, which=None, max_range2=DBL_MAX):
        """ndt_sessions_occ_integrate: every taken session's newest map-frame scan into its grid (grids: one OccGrid or None
        per session), from the session's resident pose -> the call's OCC_STATS_DTYPE record.  Pass the step records' `stepped`
        as `which`: a session taken that did not step has its last scan integrated again."""
        if len(grids) != self.n:
            raise ValueError("occ_integrate needs one grid (or None) per session")
        hs = (C.c_void_p * self.n)(*[g.h if g is not None else None for g in grids])
        w = self._active(which)
        st = np.zeros(1, dtype=OCC_STATS_DTYPE)
        self.ctx.check(lib().ndt_sessions_occ_integrate(self.h, hs, None if w is None else w.ctypes.data, float(max_range2),
                                                        st.ctypes.data), "ndt_sessions_occ_integrate")
        return st[0]

    def _grid_handles(self, grids, what):
        if len(grids) != self.n:
            raise ValueError("%s needs one grid (or None) per session" % what)
        return (C.c_void_p * self.n)(*[g.h if g is not None else None for g in grids])

    def archive_info(self, i):
        """ndt_sessions_archive_info: (scans, points) of session i's scan archive."""
        n, m = C.c_size_t(), C.c_size_t()
        self.ctx.check(lib().ndt_sessions_archive_info(self.h, i, C.byref(n), C.byref(m)), "ndt_sessions_archive_info")
        return n.value, m.value

    def archive_scans(self, i, first=0, count=None):
        """ndt_sessions_archive_scans: the archived scans [first, first + count) of session i (count None: to the end) as a
        list of [n, 2] float64 arrays -- the resampled scans in the robot frame, as the steps stored them."""
        if count is None:
            count = max(self.archive_info(i)[0] - first, 0)
        off, n = np.zeros(count + 1, dtype=np.uint64), C.c_size_t()
        self.ctx.check(lib().ndt_sessions_archive_scans(self.h, i, first, count, None, 0, off.ctypes.data, C.byref(n)),
                       "ndt_sessions_archive_scans")
        xy = np.zeros((n.value, 2), dtype=np.float64)
        self.ctx.check(lib().ndt_sessions_archive_scans(self.h, i, first, count, _ptr(xy), n.value, off.ctypes.data, C.byref(n)),
                       "ndt_sessions_archive_scans")
        return [xy[int(off[k]):int(off[k + 1])] for k in range(count)]

    def archive_view(self, i):
        """ndt_sessions_archive_view: (device address, points) of session i's whole archive; valid until the next step."""
        p, n = C.c_void_p(), C.c_size_t()
        self.ctx.check(lib().ndt_sessions_archive_view(self.h, i, C.byref(p), C.byref(n)), "ndt_sessions_archive_view")
        return p.value, n.value

    def occ_rebuild(self, grids, which=None, clear=True, max_range2=DBL_MAX):
        """ndt_sessions_occ_rebuild: every taken session's whole scan archive cast into its grid (cleared first with `clear`)
        at the poses its trajectory holds now -> the call's OCC_STATS_DTYPE record."""
        hs = self._grid_handles(grids, "occ_rebuild")
        w = self._active(which)
        st = np.zeros(1, dtype=OCC_STATS_DTYPE)
        self.ctx.check(lib().ndt_sessions_occ_rebuild(self.h, hs, None if w is None else w.ctypes.data, 1 if clear else 0,
                                                      float(max_range2), st.ctypes.data), "ndt_sessions_occ_rebuild")
        return st[0]

    def remake_closed(self, which):
        """ndt_sessions_remake_closed: every closed submap's cloud of the sessions `which` (an iterable of session indices)
        computed again from the scan archive at the poses the trajectories hold now, the local maps and NDT maps behind them
        -> {session index: status} (NDT_OK, or the code that session alone got; include/ndt_mi355x.h)."""
        who = [int(i) for i in which]
        w = np.array(who or [0], dtype=np.int32)          # (nobody named: n_named = 0 with arrays that are not NULL)
        status = np.zeros(len(w), dtype=np.int32)
        self.ctx.check(lib().ndt_sessions_remake_closed(self.h, w.ctypes.data, len(who), status.ctypes.data),
                       "ndt_sessions_remake_closed")
        return {i: int(status[c]) for c, i in enumerate(who)}

    def trajectory(self, i):
        """ndt_sessions_trajectory: (poses [n_scans, 3] float64 (tx, ty, th[deg]), sub_first [n_submaps] int32 -- every
        submap's first scan --, sub_anchor [n_submaps] int32 -- the scan whose pose pair moves the submap's closed cloud in
        correct() --, store_first: the current submap's scan store holds the scans [store_first, n_scans))."""
        n, k, first = C.c_size_t(), C.c_int(), C.c_size_t()
        self.ctx.check(lib().ndt_sessions_trajectory(self.h, i, None, 0, C.byref(n), None, None, C.byref(k), C.byref(first)),
                       "ndt_sessions_trajectory")
        poses = np.zeros((n.value, 3), dtype=np.float64)
        sub_first, sub_anchor = np.zeros(k.value, dtype=np.int32), np.zeros(k.value, dtype=np.int32)
        buf = poses if n.value else np.zeros((1, 3))           # (a session that has not started: a non-NULL address all the same)
        self.ctx.check(lib().ndt_sessions_trajectory(self.h, i, buf.ctypes.data, len(buf), C.byref(n), sub_first.ctypes.data,
                                                     sub_anchor.ctypes.data, C.byref(k), C.byref(first)), "ndt_sessions_trajectory")
        return poses, sub_first, sub_anchor, first.value

    def correct(self, new_poses):
        """ndt_sessions_correct: new_poses = {session index: its whole adjusted trajectory [n_scans, 3] (tx, ty, th[deg])}
        -> {session index: status} (NDT_OK, or the code that session alone got; include/ndt_mi355x.h)."""
        who = list(new_poses)
        arrs = [np.ascontiguousarray(new_poses[i], dtype=np.float64).reshape(-1, 3) for i in who]
        which = np.array(who, dtype=np.int32)
        ptrs = (C.c_void_p * max(len(who), 1))(*[a.ctypes.data if len(a) else None for a in arrs])
        ns = np.array([len(a) for a in arrs], dtype=np.uintp)
        status = np.zeros(max(len(who), 1), dtype=np.int32)
        self.ctx.check(lib().ndt_sessions_correct(self.h, which.ctypes.data, len(who), ptrs, ns.ctypes.data, status.ctypes.data),
                       "ndt_sessions_correct")
        return {i: int(status[c]) for c, i in enumerate(who)}

    def loop_candidates(self, params, which=None):
        """ndt_sessions_loop_candidates: the candidates ndt_sessions_find_loops would search, as LOOP_CANDIDATE_DTYPE records
        (host only, no device work)."""
        out = np.zeros(self.n, dtype=LOOP_CANDIDATE_DTYPE)
        n, w = C.c_int(), self._active(which)
        self.ctx.check(lib().ndt_sessions_loop_candidates(self.h, None if w is None else w.ctypes.data, C.byref(params),
                                                          out.ctypes.data, C.byref(n)), "ndt_sessions_loop_candidates")
        return out[:n.value]

    def find_loops(self, params, which=None, want_records=False):
        """ndt_sessions_find_loops: one LOOP_DTYPE record per candidate; with want_records also the match records, as
        [candidates, NDT_LOOP_MAX_CAND] RESULT_DTYPE (the first n_cand of a row are written)."""
        out = np.zeros(self.n, dtype=LOOP_DTYPE)
        rec = np.zeros((self.n, NDT_LOOP_MAX_CAND), dtype=RESULT_DTYPE) if want_records else None
        n, w = C.c_int(), self._active(which)
        self.ctx.check(lib().ndt_sessions_find_loops(self.h, None if w is None else w.ctypes.data, C.byref(params), out.ctypes.data,
                                                     C.byref(n), None if rec is None else rec.ctypes.data), "ndt_sessions_find_loops")
        return (out[:n.value], rec[:n.value]) if want_records else out[:n.value]

    def loop_candidates_multi(self, params, which=None):
        """ndt_sessions_loop_candidates_multi: the candidates ndt_sessions_find_loops_multi would search -- up to
        params.max_submaps per session, nearest first -- as LOOP_CANDIDATE_DTYPE records (host only)."""
        out = np.zeros(self.n * NDT_LOOP_MAX_SUBMAPS, dtype=LOOP_CANDIDATE_DTYPE)
        n, w = C.c_int(), self._active(which)
        self.ctx.check(lib().ndt_sessions_loop_candidates_multi(self.h, None if w is None else w.ctypes.data, C.byref(params),
                                                                out.ctypes.data, C.byref(n)), "ndt_sessions_loop_candidates_multi")
        return out[:n.value]

    def _cross(self, fn, dtype, params, which, against, want_records):
        """Both cross calls: `dtype` records for up to n * NDT_LOOP_MAX_SUBMAPS candidates.  want_records: None for the call
        that takes no record array (the candidates), else whether to pass one and return it beside the records."""
        room = self.n * NDT_LOOP_MAX_SUBMAPS
        out = np.zeros(room, dtype=dtype)
        rec = np.zeros((room, NDT_LOOP_MAX_CAND), dtype=RESULT_DTYPE) if want_records else None
        w, a, n = self._active(which), self._active(against), C.c_int()
        args = [self.h, None if w is None else w.ctypes.data, None if a is None else a.ctypes.data, C.byref(params), out.ctypes.data, C.byref(n)]
        if want_records is not None:
            args.append(None if rec is None else rec.ctypes.data)
        self.ctx.check(getattr(lib(), fn)(*args), fn)
        return (out[:n.value], rec[:n.value]) if want_records else out[:n.value]

    def cross_candidates(self, params, which=None, against=None):
        """ndt_sessions_cross_candidates: the candidates ndt_sessions_find_cross_loops would search -- for every searcher
        (`which`) up to params.max_submaps closed submaps of the OTHER sessions (`against`), nearest first -- as
        CROSS_CANDIDATE_DTYPE records (the device gate: one host wait)."""
        return self._cross("ndt_sessions_cross_candidates", CROSS_CANDIDATE_DTYPE, params, which, against, None)

    def find_cross_loops(self, params, which=None, against=None, want_records=False):
        """ndt_sessions_find_cross_loops: one CROSS_LOOP_DTYPE record per cross candidate; with want_records also the match
        records, as [candidates, NDT_LOOP_MAX_CAND] RESULT_DTYPE (the first n_cand of a row are written)."""
        return self._cross("ndt_sessions_find_cross_loops", CROSS_LOOP_DTYPE, params, which, against, bool(want_records))

    def place_candidates(self, params, which=None, against=None):
        """ndt_sessions_place_candidates: for every searcher (`which`) up to params.top_k closed submaps of the OTHER sessions
        (`against`) whose place descriptor resembles the searcher's local map, best first, with a pose guess in the other
        session's frame -- no shared frame needed -- as PLACE_CANDIDATE_DTYPE records (one host wait)."""
        K = params.top_k if 1 <= params.top_k <= NDT_PLACE_MAX_TOP_K else NDT_PLACE_MAX_TOP_K
        out = np.zeros(self.n * K, dtype=PLACE_CANDIDATE_DTYPE)
        w, a, n = self._active(which), self._active(against), C.c_int()
        self.ctx.check(lib().ndt_sessions_place_candidates(self.h, None if w is None else w.ctypes.data, None if a is None else a.ctypes.data,
                                                           C.byref(params), out.ctypes.data, C.byref(n)), "ndt_sessions_place_candidates")
        return out[:n.value]

    def find_loops_multi(self, params, which=None, want_records=False):
        """ndt_sessions_find_loops_multi: one LOOP_MULTI_DTYPE record per candidate; with want_records also the match records,
        as [candidates, NDT_LOOP_MAX_CAND] RESULT_DTYPE (the first n_cand of a row are written)."""
        room = self.n * NDT_LOOP_MAX_SUBMAPS
        out = np.zeros(room, dtype=LOOP_MULTI_DTYPE)
        rec = np.zeros((room, NDT_LOOP_MAX_CAND), dtype=RESULT_DTYPE) if want_records else None
        n, w = C.c_int(), self._active(which)
        self.ctx.check(lib().ndt_sessions_find_loops_multi(self.h, None if w is None else w.ctypes.data, C.byref(params),
                                                           out.ctypes.data, C.byref(n), None if rec is None else rec.ctypes.data),
                       "ndt_sessions_find_loops_multi")
        return (out[:n.value], rec[:n.value]) if want_records else out[:n.value]

    def stats(self):
        st = SessionsStats()
        self.ctx.check(lib().ndt_sessions_get_stats(self.h, C.byref(st)), "ndt_sessions_get_stats")
        return st


class Map(_Handle):
    """ndt_map: the NDT voxel grid of one target cloud (replaces ndt.setInputTarget)."""
    _destroy = "ndt_map_destroy"

    def __init__(self, ctx, xy=None, params=None, dev_ptr=None, n=None, stride=8):
        self.ctx = ctx
        self.params = params if params is not None else default_params()
        self.h = C.c_void_p()
        self.rebuild(xy=xy, dev_ptr=dev_ptr, n=n, stride=stride)

    @classmethod
    def adopt(cls, ctx, handle, params):
        """A Map that owns `handle`, an ndt_map * a C call created on ctx (ndt_map_build_batch) with `params`."""
        m = cls.__new__(cls)
        m.ctx, m.params, m.h = ctx, params, C.c_void_p(handle)
        return m

    def _cx(self, ctx):
        """The context that launches: the caller's, or the map's own."""
        return ctx if ctx is not None else self.ctx

    def rebuild(self, xy=None, dev_ptr=None, n=None, stride=8, params=None):
        """Build the map again in place; `params`: other ndt_params from now on (the resolution may not change)."""
        if params is not None:
            self.params = params
        if dev_ptr is not None:
            rc = lib().ndt_map_build_dev(self.ctx.h, dev_ptr, n, stride, C.byref(self.params), C.byref(self.h))
        else:
            xy = _f32c(xy)
            rc = lib().ndt_map_build(self.ctx.h, xy.ctypes.data, len(xy), 8, C.byref(self.params), C.byref(self.h))
        self.ctx.check(rc, "ndt_map_build")

    def rebuild_begin(self, dev_ptr, n, stride=8):
        """Queue the rebuild with the voxel grid of the previous build and return (no host wait); see rebuild_end."""
        self.ctx.check(lib().ndt_map_rebuild_begin(self.ctx.h, dev_ptr, n, stride, C.byref(self.params), self.h),
                       "ndt_map_rebuild_begin")

    def rebuild_end(self):
        """True if the cloud's bounding box had moved: the build was queued again and launches queued since
        rebuild_begin used a stale grid."""
        rc = lib().ndt_map_rebuild_end(self.ctx.h, self.h)
        if rc < 0:
            self.ctx.check(rc, "ndt_map_rebuild_end")
        return rc == 1

    def info(self):
        i = MapInfo()
        self.ctx.check(lib().ndt_map_info_get(self.h, C.byref(i)), "ndt_map_info_get")
        return i

    def export(self):
        n = self.info().n_cells
        idx = np.zeros(n, np.int32); cent = np.zeros((n, 2), np.float32)
        mean = np.zeros((n, 2), np.float64); icov = np.zeros((n, 3), np.float64)
        npts = np.zeros(n, np.int32)
        self.ctx.check(lib().ndt_map_export(self.h, idx.ctypes.data, cent.ctypes.data, mean.ctypes.data,
                                            icov.ctypes.data, npts.ctypes.data), "ndt_map_export")
        return dict(idx=idx, cent=cent, mean=mean, icov=icov, npts=npts)

    def align(self, scan, init):
        scan = _f32c(scan)
        init = np.ascontiguousarray(init, dtype=np.float64)
        res = np.zeros(1, dtype=RESULT_DTYPE)
        self.ctx.check(lib().ndt_align(self.ctx.h, self.h, scan.ctypes.data, len(scan), 8, init.ctypes.data,
                                       res.ctypes.data), "ndt_align")
        return res[0]

    def align_batch(self, scans, offsets, inits, shared_scan=False, trace_cap=0):
        scans, offsets, inits, B, res = _batch_args(scans, offsets, inits)
        if trace_cap:
            trace = np.zeros((B, trace_cap, 8)); rows = np.zeros(B, np.int32)
            self.ctx.check(lib().ndt_align_batch_trace(
                self.ctx.h, self.h, scans.ctypes.data, offsets.ctypes.data, B, int(shared_scan),
                inits.ctypes.data, res.ctypes.data, trace.ctypes.data, trace_cap, rows.ctypes.data),
                "ndt_align_batch_trace")
            return res, [trace[b, :min(rows[b], trace_cap)] for b in range(B)]
        self.ctx.check(lib().ndt_align_batch(self.ctx.h, self.h, scans.ctypes.data, offsets.ctypes.data, B,
                                             int(shared_scan), inits.ctypes.data, res.ctypes.data),
                       "ndt_align_batch")
        return res

    def align_batch_dev(self, scans_ptr, offsets_ptr, B, total_points, inits_ptr, out_ptr, shared_scan=False,
                        stream=None, ctx=None):
        """All pointers are device addresses (e.g. torch.Tensor.data_ptr()); asynchronous.  `ctx`: the context
        whose scratch the launch uses (default: the map's own) -- two contexts keep two batches in flight."""
        cx = self._cx(ctx)
        cx.check(lib().ndt_align_batch_dev(cx.h, self.h, scans_ptr, offsets_ptr, B, total_points,
                                           int(shared_scan), inits_ptr, out_ptr, stream), "ndt_align_batch_dev")

    def prepare_batch_dev(self, scans_ptr, offsets_ptr, B, total_points, inits_ptr, shared_scan=False, stream=None, ctx=None):
        """ndt_align_batch_prepare_dev: the optimiser's start, the window geometry and the voxel order of every scan of a batch,
        queued on `stream` ahead of the align_batch_dev call with the same arguments (and the same `ctx`); asynchronous."""
        cx = self._cx(ctx)
        cx.check(lib().ndt_align_batch_prepare_dev(cx.h, self.h, scans_ptr, offsets_ptr, B, total_points,
                                                   int(shared_scan), inits_ptr, stream), "ndt_align_batch_prepare_dev")

    def eval_at(self, scan, p):
        scan = _f32c(scan)
        p = np.ascontiguousarray(p, dtype=np.float64)
        s = C.c_double(); pr = C.c_double(); g = np.zeros(3); H = np.zeros(9)
        self.ctx.check(lib().ndt_eval_at(self.ctx.h, self.h, scan.ctypes.data, len(scan), 8, p.ctypes.data,
                                         C.addressof(s), g.ctypes.data, H.ctypes.data, C.addressof(pr)),
                       "ndt_eval_at")
        return s.value, g, H.reshape(3, 3), pr.value

    def fitness_at(self, scan, c, s, tx, ty):
        scan = _f32c(scan)
        f = C.c_double()
        self.ctx.check(lib().ndt_fitness_at(self.ctx.h, self.h, scan.ctypes.data, len(scan), 8, c, s, tx, ty,
                                            C.addressof(f)), "ndt_fitness_at")
        return f.value

    def score_poses(self, scan, poses, stride=8):
        """ndt_score_poses: the NDT score alone of one scan ([n, 2] float32) at every pose of `poses` ([P, 3] float64)
        -> (score [P] float64, pairs [P] uint32).  `stride` > 8: the scan is handed over in records of that many bytes."""
        scan = _f32c(scan)
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        if stride != 8:
            wide = np.zeros((len(scan), stride // 4), dtype=np.float32)
            wide[:, :2] = scan
            scan = wide
        P = len(poses)
        score = np.zeros(P, dtype=np.float64); pairs = np.zeros(P, dtype=np.uint32)
        self.ctx.check(lib().ndt_score_poses(self.ctx.h, self.h, scan.ctypes.data, len(scan), stride, poses.ctypes.data, P,
                                             score.ctypes.data, pairs.ctypes.data), "ndt_score_poses")
        return score, pairs

    def score_poses_dev(self, scan_ptr, n, poses_ptr, P, score_ptr, pairs_ptr=None, stride=8, stream=None, ctx=None):
        """ndt_score_poses_dev: device addresses; asynchronous.  `ctx`: the context that launches (default: the map's)."""
        cx = self._cx(ctx)
        cx.check(lib().ndt_score_poses_dev(cx.h, self.h, scan_ptr, n, stride, poses_ptr, P, score_ptr, pairs_ptr, stream),
                 "ndt_score_poses_dev")

    def score_lattice(self, scan_ptr, n, lattice, score_ptr, pairs_ptr=None, stride=8, stream=None, ctx=None):
        """ndt_score_lattice_dev: the score volume of a PoseLattice; device addresses; asynchronous."""
        cx = self._cx(ctx)
        cx.check(lib().ndt_score_lattice_dev(cx.h, self.h, scan_ptr, n, stride, C.byref(lattice), score_ptr, pairs_ptr, stream),
                 "ndt_score_lattice_dev")

    def lattice_select(self, lattice, score_ptr, pairs_ptr, top_k, local_max, cand_ptr, n_cand_ptr, stream=None, ctx=None):
        """ndt_lattice_select_dev: the top_k eligible poses of a score volume (device addresses: uint64 indices, one int32
        count); asynchronous."""
        cx = self._cx(ctx)
        cx.check(lib().ndt_lattice_select_dev(cx.h, C.byref(lattice), score_ptr, pairs_ptr, int(top_k), int(local_max), cand_ptr,
                                              n_cand_ptr, stream), "ndt_lattice_select_dev")

    def fit_points(self, scans, offsets, tf, max_d2=DBL_MAX, shared_scan=False, want_d2=True):
        """ndt_fit_points_batch: the float32 squared distance of every scan point, at transform b of `tf`, to its nearest raw
        map point, in input order, and getFitnessScore(max_range) per match -> (d2 float32 or None, stats FIT_STATS_DTYPE [B]).
        `tf`: a [B, 4] float32 array of (c, s, tx, ty), or a record array of align_batch (its T00, T10, T03, T13 are taken).
        shared_scan: scan 0 with every transform; d2 is then [B * n], row b at b * n."""
        scans = _f32c(scans)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        tf = _tf4(tf)
        B = len(tf)
        nscan = 1 if shared_scan else B
        if len(offsets) != nscan + 1:
            raise ValueError("offsets needs one entry per scan and one more")
        n_d2 = B * int(offsets[1] - offsets[0]) if shared_scan else int(offsets[-1])
        d2 = np.zeros(n_d2, dtype=np.float32) if want_d2 else None
        stats = np.zeros(B, dtype=FIT_STATS_DTYPE)
        self.ctx.check(lib().ndt_fit_points_batch(self.ctx.h, self.h, scans.ctypes.data, offsets.ctypes.data, B, int(shared_scan),
                                                  tf.ctypes.data, 16, float(max_d2), d2.ctypes.data if want_d2 else None,
                                                  stats.ctypes.data), "ndt_fit_points_batch")
        return d2, stats

    def fit_points_dev(self, scans_ptr, offsets_ptr, B, total_points, tf_ptr, tf_stride, max_d2, d2_ptr, stats_ptr,
                       shared_scan=False, stream=None, ctx=None):
        """ndt_fit_points_batch_dev: device addresses (d2_ptr or stats_ptr may be None); asynchronous.  tf_ptr = the address of
        a record's T00 with tf_stride = RESULT_BYTES reads the transforms of a launch's records where they lie."""
        cx = self._cx(ctx)
        cx.check(lib().ndt_fit_points_batch_dev(cx.h, self.h, scans_ptr, offsets_ptr, B, total_points, int(shared_scan), tf_ptr,
                                                tf_stride, float(max_d2), d2_ptr, stats_ptr, stream), "ndt_fit_points_batch_dev")

    def relocalize(self, scan, lattice, top_k=16, local_max=True, want_scores=False, dev_ptr=None, n=None, stride=8, max_d2=None):
        """ndt_relocalize (or, with dev_ptr / n / stride, ndt_relocalize_dev): sweep the lattice, pick top_k candidates,
        refine them with the shared-scan match -> dict(cand_index [m] uint64, cand_score [m], records [m] RESULT_DTYPE,
        best (index of the lowest cost `converged ? fitness : 1e7`, -1 when m == 0), scores (the whole volume or None)).
        max_d2 (host scans only): the candidates are ranked again by `converged ? ranged fitness : 1e7` -- getFitnessScore
        with max_range, from ONE fit_points call with shared_scan on the candidates' records -- ties to the higher n_in, then
        the lower index; `best` is that ranking's, and the dict also holds fit_stats and best_unbounded (the C call's)."""
        if max_d2 is not None and dev_ptr is not None:
            raise ValueError("relocalize: max_d2 needs the scan in host memory")
        prm = RelocParams(lattice, int(top_k), int(bool(local_max)))
        idx = np.zeros(top_k, dtype=np.uint64); cs = np.zeros(top_k, dtype=np.float64)
        rec = np.zeros(top_k, dtype=RESULT_DTYPE)
        m, best = C.c_int(), C.c_int()
        vol = np.zeros(lattice.size, dtype=np.float64) if want_scores else None
        volp = vol.ctypes.data if vol is not None else None
        if dev_ptr is not None:
            rc = lib().ndt_relocalize_dev(self.ctx.h, self.h, dev_ptr, n, stride, C.byref(prm), idx.ctypes.data, cs.ctypes.data,
                                          rec.ctypes.data, C.byref(m), C.byref(best), volp)
        else:
            scan = _f32c(scan)
            rc = lib().ndt_relocalize(self.ctx.h, self.h, scan.ctypes.data, len(scan), 8, C.byref(prm), idx.ctypes.data,
                                      cs.ctypes.data, rec.ctypes.data, C.byref(m), C.byref(best), volp)
        self.ctx.check(rc, "ndt_relocalize")
        k = m.value
        out = dict(cand_index=idx[:k].copy(), cand_score=cs[:k].copy(), records=rec[:k].copy(), best=best.value, scores=vol)
        if max_d2 is not None:
            out["best_unbounded"] = out["best"]
            out["fit_stats"] = np.zeros(0, dtype=FIT_STATS_DTYPE)
            if k > 0:
                _, st = self.fit_points(scan, np.array([0, len(scan)], dtype=np.uint64), out["records"], max_d2=max_d2,
                                        shared_scan=True, want_d2=False)
                out["fit_stats"] = st
                out["best"] = rerank(out["records"], st)
        return out


def _occ_handles(grids):
    grids = list(grids)
    return (C.c_void_p * len(grids))(*[g.h for g in grids]), len(grids)


def integrate_occ(ctx, grids, scans, offsets, origins, grid_of=None, max_range2=DBL_MAX):
    """ndt_occ_integrate: scan b = the float32 map-frame points [offsets[b], offsets[b + 1]) of `scans`, ray-cast from
    origins[b] (a [B, 2] or [B, 3] float64 array: the first two of each row) into grids[grid_of[b]] (None: all into grids[0])
    -> the call's OCC_STATS_DTYPE record."""
    scans = _f32c(scans)
    if scans.size == 0:
        scans = np.zeros((1, 2), dtype=np.float32)     # (an address for a batch of empty scans)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    origins = np.ascontiguousarray(origins, dtype=np.float64)
    B = len(offsets) - 1
    if origins.ndim != 2 or origins.shape[0] != B or origins.shape[1] < 2:
        raise ValueError("origins needs one row of at least two doubles per scan")
    gof = None if grid_of is None else np.ascontiguousarray(grid_of, dtype=np.int32)
    if gof is not None and len(gof) != B:
        raise ValueError("grid_of needs one entry per scan")
    hs, n = _occ_handles(grids)
    st = np.zeros(1, dtype=OCC_STATS_DTYPE)
    ctx.check(lib().ndt_occ_integrate(ctx.h, hs, n, None if gof is None else gof.ctypes.data, scans.ctypes.data, offsets.ctypes.data,
                                      B, origins.ctypes.data, origins.strides[0], float(max_range2), st.ctypes.data),
              "ndt_occ_integrate")
    return st[0]


def integrate_occ_dev(ctx, grids, grid_of_ptr, xy_ptr, offsets_ptr, B, total_points, origins_ptr, origin_stride=24,
                      max_range2=DBL_MAX, stats_ptr=None, stream=None):
    """ndt_occ_integrate_dev: device addresses (grid_of_ptr None: every scan into grids[0]; stats_ptr None: no stats);
    asynchronous on `stream` (None: the context's)."""
    hs, n = _occ_handles(grids)
    ctx.check(lib().ndt_occ_integrate_dev(ctx.h, hs, n, grid_of_ptr, xy_ptr, offsets_ptr, B, total_points, origins_ptr, origin_stride,
                                          float(max_range2), stats_ptr, stream), "ndt_occ_integrate_dev")


class OccGrid(_Handle):
    """ndt_occ: an occupancy grid of {hit, pass} counters on the device (include/ndt_mi355x.h)."""
    _destroy = "ndt_occ_destroy"

    def __init__(self, ctx, geometry):
        self.ctx = ctx
        self.geometry = OccGeometry(geometry.x0, geometry.y0, geometry.res, geometry.nx, geometry.ny)
        self.h = C.c_void_p()
        ctx.check(lib().ndt_occ_create(ctx.h, C.byref(self.geometry), C.byref(self.h)), "ndt_occ_create")

    @property
    def shape(self):
        return (self.geometry.ny, self.geometry.nx)

    def cells_ptr(self):
        """ndt_occ_view: the device address of the interleaved {hit, pass} uint32 array."""
        p = C.c_void_p()
        self.ctx.check(lib().ndt_occ_view(self.h, C.byref(p)), "ndt_occ_view")
        return p.value

    def integrate(self, scans, offsets, origins, max_range2=DBL_MAX):
        """integrate_occ with this grid alone."""
        return integrate_occ(self.ctx, [self], scans, offsets, origins, None, max_range2)

    def integrate_dev(self, xy_ptr, offsets_ptr, B, total_points, origins_ptr, origin_stride=24, max_range2=DBL_MAX,
                      stats_ptr=None, stream=None):
        """integrate_occ_dev with this grid alone: device addresses; asynchronous."""
        integrate_occ_dev(self.ctx, [self], None, xy_ptr, offsets_ptr, B, total_points, origins_ptr, origin_stride, max_range2,
                          stats_ptr, stream)

    def render(self, min_obs=1):
        """ndt_occ_render -> [ny, nx] int8: 100 hit / n rounded half up, -1 below min_obs observations."""
        out = np.zeros(self.shape, dtype=np.int8)
        self.ctx.check(lib().ndt_occ_render(self.ctx.h, self.h, int(min_obs), out.ctypes.data), "ndt_occ_render")
        return out

    def render_dev(self, out_ptr, min_obs=1, stream=None):
        self.ctx.check(lib().ndt_occ_render_dev(self.ctx.h, self.h, int(min_obs), out_ptr, stream), "ndt_occ_render_dev")

    def counts(self):
        """ndt_occ_counts -> (hit, pass), [ny, nx] uint32 each."""
        hit = np.zeros(self.shape, dtype=np.uint32)
        pas = np.zeros(self.shape, dtype=np.uint32)
        self.ctx.check(lib().ndt_occ_counts(self.ctx.h, self.h, hit.ctypes.data, pas.ctypes.data), "ndt_occ_counts")
        return hit, pas

    def clear(self, stream=None):
        self.ctx.check(lib().ndt_occ_clear(self.ctx.h, self.h, stream), "ndt_occ_clear")
