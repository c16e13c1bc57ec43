"""picp_amd -- Python binding of libpicp_amd.so (the MI355X PICP hot path, include/picp_c.h).

Thin ctypes layer used by the tests, bench.py and __graft_entry__; the product itself is the
C-ABI library and the C++ facade (include/pr/*.h).  There is deliberately no CPU fallback:
if the native library is missing or no HIP device is present, every compute call raises.

Mirrors the reference interface (llepa/02-VisualOdometry):
  * PICPSolver  -- pr::PICPSolver (src/picp_solver.h:21-82): init / oneRound /
                   setKernelThreshold / chiInliers / chiOutliers / numInliers / camera pose,
                   plus solve() = the exec/icp_test.cpp:88-107 loop fused on the device.
  * Batch       -- independent frames solved together on one device (the batch split).
  * triangulate -- Cam::triangulatePoints' DLT (src/cam.cpp:94-140).
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
# PICP_LIB selects a diagnostic build (tools/stamps.py); the default is the shipped library
LIB_PATH = os.environ.get("PICP_LIB") or os.path.join(PKG_ROOT, "lib", "libpicp_amd.so")

OK = 0
ERR_ARG = -1
ERR_DEVICE = -2
ERR_RANGE = -3
ERR_STATE = -4
ERR_NOMEM = -5
TOO_FEW_INLIERS = 1

K_REF = np.array([[180, 0, 320], [0, 180, 240], [0, 0, 1]], np.float32)  # src/cam.cpp:11-16

# every symbol include/picp_c.h declares (tests check the library exports all of them)
EXPORTED = [
    "picp_params_default", "picp_abi_version", "picp_last_error", "picp_device_count",
    "picp_create", "picp_destroy", "picp_set_camera", "picp_clone", "picp_set_points",
    "picp_set_correspondences", "picp_set_pose", "picp_get_pose", "picp_one_round",
    "picp_solve", "picp_linearize", "picp_batch_create", "picp_batch_destroy",
    "picp_batch_set_data", "picp_batch_set_data_device", "picp_batch_set_poses",
    "picp_batch_get_poses", "picp_batch_get_stats", "picp_batch_solve",
    "picp_batch_solve_async", "picp_batch_sync", "picp_batch_time", "picp_batch_time_single",
    "picp_batch_info", "picp_batch_residency",
    "picp_triangulate", "picp_projection_matrix", "picp_match", "picp_match_batch", "picp_match_batch_form",
    "picp_vo_create", "picp_vo_destroy", "picp_vo_set_segments", "picp_vo_run", "picp_vo_run_async", "picp_vo_debug_matches", "picp_vo_debug_guard",
    "picp_vo_sync", "picp_vo_get_poses", "picp_vo_get_steps", "picp_vo_get_map", "picp_vo_time",
    "picp_vo_info", "picp_selftest_rcp", "picp_selftest_finish", "picp_essential_params_default", "picp_essential_batch",
    "picp_shard_range", "picp_shard_pad", "picp_shard_unpack", "picp_comm_unique_id", "picp_comm_create", "picp_comm_destroy", "picp_comm_info",
    "picp_comm_allreduce_max", "picp_comm_barrier", "picp_batch_allgather", "picp_batch_allgather_host",
    "picp_classify", "picp_batch_classify", "picp_batch_classify_time",
    "picp_vo_set_track_stats", "picp_vo_get_map_stats",
    "picp_refine_params_default", "picp_refine_create", "picp_refine_destroy", "picp_refine_set_poses",
    "picp_refine_set_tracks", "picp_refine_set_points", "picp_refine_run", "picp_refine_get_points",
    "picp_refine_get_stats", "picp_refine_time",
    "picp_vo_set_track_log", "picp_vo_get_tracks", "picp_vo_get_poses_wc", "picp_vo_refine_map",
    "picp_vo_get_refined_map", "picp_vo_refine_time",
    "picp_adjust_params_default", "picp_refine_set_fixed_poses", "picp_refine_run_poses", "picp_refine_adjust",
    "picp_refine_get_poses", "picp_refine_get_pose_stats", "picp_refine_get_pose_view", "picp_refine_get_sweeps",
    "picp_refine_adjust_time", "picp_vo_adjust", "picp_vo_get_adjusted_poses_wc", "picp_vo_get_adjusted_map",
    "picp_pnp_params_default", "picp_pnp_batch", "picp_pnp_batch_debug", "picp_pnp_batch_time", "picp_relocalize",
    "picp_sim3_params_default", "picp_sim3_batch", "picp_sim3_batch_debug", "picp_sim3_batch_time", "picp_sim3_fit_batch",
    "picp_vo_align_segments",
    "picp_pgo_params_default", "picp_pgo_batch", "picp_pgo_batch_time",
]
# state of one correspondence at a pose (include/picp_c.h PICP_CORR_*)
CORR_SKIPPED, CORR_INLIER, CORR_OUTLIER = 0, 1, 2
COMM_ID_BYTES = 128


class PicpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("picp error %d: %s" % (code, msg))
        self.code = code


class Stats(ctypes.Structure):
    _fields_ = [("chi_in", ctypes.c_float), ("chi_out", ctypes.c_float),
                ("n_in", ctypes.c_int32), ("ok", ctypes.c_int32), ("rounds", ctypes.c_int32),
                ("converged", ctypes.c_int32), ("n_projected", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class VOStep(ctypes.Structure):
    _fields_ = [("n_corr", ctypes.c_int32), ("n_in", ctypes.c_int32), ("rounds", ctypes.c_int32),
                ("n_new", ctypes.c_int32), ("chi_in", ctypes.c_float), ("chi_out", ctypes.c_float),
                ("converged", ctypes.c_int32), ("n_projected", ctypes.c_int32)]


class Params(ctypes.Structure):
    _fields_ = [("threshold", ctypes.c_float), ("damping", ctypes.c_float),
                ("min_inliers", ctypes.c_int32), ("keep_outliers", ctypes.c_int32),
                ("max_rounds", ctypes.c_int32), ("conv_eps", ctypes.c_float)]


class AdjustParams(ctypes.Structure):
    """picp_adjust_params: the point step's parameters, the pose step's, and the sweeps."""
    _fields_ = [("points", Params), ("poses", Params), ("sweeps", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class AdjustSweep(ctypes.Structure):
    """picp_adjust_sweep: the sums of one sweep's per-point and per-pose stats."""
    _fields_ = [("chi_in_points", ctypes.c_double), ("chi_in_poses", ctypes.c_double),
                ("n_in_points", ctypes.c_int64), ("n_in_poses", ctypes.c_int64),
                ("ok_points", ctypes.c_int64), ("ok_poses", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PnpParams(ctypes.Structure):
    """picp_pnp_params (include/picp_c.h): the P3P RANSAC's gate, hypothesis count and seed."""
    _fields_ = [("threshold", ctypes.c_float), ("hypotheses", ctypes.c_int32), ("min_inliers", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("seed", ctypes.c_uint64)]


class Sim3Params(ctypes.Structure):
    """picp_sim3_params (include/picp_c.h): the Sim(3) RANSAC's gate, hypothesis count, refits and seed."""
    _fields_ = [("threshold", ctypes.c_float), ("hypotheses", ctypes.c_int32), ("min_inliers", ctypes.c_int32),
                ("with_scale", ctypes.c_int32), ("refits", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("seed", ctypes.c_uint64)]


class PgoParams(ctypes.Structure):
    """picp_pgo_params (include/picp_c.h): the pose-graph solver's form, step count, damping and stop."""
    _fields_ = [("with_scale", ctypes.c_int32), ("iterations", ctypes.c_int32), ("damping", ctypes.c_double),
                ("eps", ctypes.c_double)]


# picp_pgo_batch's per-graph status (include/picp_c.h PICP_PGO_*)
PGO_OK, PGO_BAD_INPUT, PGO_BAD_EDGE, PGO_DISCONNECTED, PGO_NOT_PD, PGO_TOO_LARGE = range(6)

_lib = None
# picp_exchange_fn (include/picp_c.h): int (*)(void* user, const void* send, void* recv, size_t bytes)
EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)


def build():
    import subprocess
    subprocess.check_call(["make", "-s", "-j8", "-C", PKG_ROOT])


def lib():
    """Load libpicp_amd.so (fails loudly if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PicpError(ERR_STATE, "native library %s missing: run `make -C %s`" % (LIB_PATH, PKG_ROOT))
    L = ctypes.CDLL(LIB_PATH)
    vp, i, i64, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    fp = ctypes.POINTER(ctypes.c_float)
    dp = ctypes.POINTER(ctypes.c_double)
    sp = ctypes.POINTER(Stats)
    pp = ctypes.POINTER(Params)
    i32p, u8p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8)
    sig = {
        "picp_params_default": ([pp], None),
        "picp_abi_version": ([], i),
        "picp_last_error": ([], ctypes.c_char_p),
        "picp_device_count": ([ctypes.POINTER(i)], i),
        "picp_create": ([ctypes.POINTER(vp), i, i, i, fp], i),
        "picp_destroy": ([vp], i),
        "picp_set_camera": ([vp, i, i, fp], i),
        "picp_clone": ([vp, ctypes.POINTER(vp)], i),
        "picp_set_points": ([vp, fp, i64, fp, i64], i),
        "picp_set_correspondences": ([vp, ctypes.POINTER(ctypes.c_int32), i64], i),
        "picp_set_pose": ([vp, fp], i),
        "picp_get_pose": ([vp, fp], i),
        "picp_one_round": ([vp, f, f, i, i, sp], i),
        "picp_solve": ([vp, pp, sp], i),
        "picp_linearize": ([vp, f, i, dp, dp, sp], i),
        "picp_batch_create": ([ctypes.POINTER(vp), i, i, ctypes.POINTER(i64), i, i, fp], i),
        "picp_batch_destroy": ([vp], i),
        "picp_batch_set_data": ([vp, fp, fp], i),
        "picp_batch_set_data_device": ([vp, vp, vp, vp, vp, vp], i),
        "picp_batch_set_poses": ([vp, fp], i),
        "picp_batch_get_poses": ([vp, fp], i),
        "picp_batch_get_stats": ([vp, sp], i),
        "picp_batch_solve": ([vp, pp], i),
        "picp_batch_solve_async": ([vp, pp], i),
        "picp_batch_sync": ([vp], i),
        "picp_batch_time": ([vp, pp, i, fp, fp], i),
        "picp_batch_time_single": ([vp, pp, fp], i),
        "picp_batch_residency": ([vp, ctypes.POINTER(i), ctypes.POINTER(i), ctypes.POINTER(i)], i),
        "picp_batch_info": ([vp, ctypes.POINTER(i64), ctypes.POINTER(i), ctypes.POINTER(i)], i),
        "picp_triangulate": ([i, fp, fp, fp, fp, i64, fp], i),
        "picp_projection_matrix": ([fp, fp, fp], i),
        "picp_match": ([i, fp, i64, fp, i64, i, f, f, ctypes.POINTER(ctypes.c_int32), fp, fp,
                        ctypes.POINTER(ctypes.c_int32)], i),
        "picp_match_batch": ([i, i, ctypes.POINTER(i64), ctypes.POINTER(i64), fp, fp, i, f, f,
                              ctypes.POINTER(ctypes.c_int32), fp, fp, ctypes.POINTER(ctypes.c_int32)], i),
        "picp_match_batch_form": ([i, i, ctypes.POINTER(i64), ctypes.POINTER(i64), fp, fp, i, f, f,
                                   ctypes.POINTER(ctypes.c_int32), fp, fp, ctypes.POINTER(ctypes.c_int32), i], i),
        "picp_vo_create": ([ctypes.POINTER(vp), i, i, i, fp, i64, ctypes.POINTER(i64), fp, fp, i], i),
        "picp_vo_destroy": ([vp], i),
        "picp_vo_set_segments": ([vp, i, ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_int32), fp, pp], i),
        "picp_vo_run": ([vp], i),
        "picp_vo_run_async": ([vp], i),
        "picp_vo_debug_matches": ([vp, i, ctypes.POINTER(ctypes.c_int32)], i),
        "picp_vo_debug_guard": ([vp, ctypes.POINTER(i64), ctypes.POINTER(i)], i),
        "picp_vo_sync": ([vp], i),
        "picp_vo_get_poses": ([vp, fp], i),
        "picp_vo_get_steps": ([vp, ctypes.POINTER(VOStep)], i),
        "picp_vo_get_map": ([vp, i, i64, fp, fp, ctypes.POINTER(i64)], i),
        "picp_vo_time": ([vp, i, fp], i),
        "picp_selftest_rcp": ([i, i, i, ctypes.POINTER(ctypes.c_uint64)], i),
        "picp_selftest_finish": ([i, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p], i),
        "picp_vo_info": ([vp, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i)], i),
        "picp_shard_range": ([i64, i, i, ctypes.POINTER(i64), ctypes.POINTER(i64)], i),
        "picp_shard_pad": ([i64, i], i64),
        "picp_shard_unpack": ([i64, i, i64, vp, vp], i),
        "picp_comm_unique_id": ([ctypes.POINTER(ctypes.c_uint8)], i),
        "picp_comm_create": ([ctypes.POINTER(vp), i, i, i, ctypes.POINTER(ctypes.c_uint8)], i),
        "picp_comm_destroy": ([vp], i),
        "picp_comm_info": ([vp, ctypes.POINTER(i), ctypes.POINTER(i), ctypes.POINTER(i)], i),
        "picp_comm_allreduce_max": ([vp, dp, i], i),
        "picp_comm_barrier": ([vp], i),
        "picp_batch_allgather": ([vp, vp, i64, fp, sp], i),
        "picp_batch_allgather_host": ([vp, i, i, EXCHANGE_FN, vp, i64, fp, sp], i),
        "picp_classify": ([vp, f, ctypes.POINTER(ctypes.c_uint8), fp, fp, ctypes.POINTER(ctypes.c_int32),
                           ctypes.POINTER(i64)], i),
        "picp_batch_classify": ([vp, f, fp, ctypes.POINTER(ctypes.c_uint8), fp, ctypes.POINTER(i64),
                                 ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(i64)], i),
        "picp_batch_classify_time": ([vp, f, i, fp], i),
        "picp_vo_set_track_stats": ([vp, i], i),
        "picp_vo_get_map_stats": ([vp, i, i64, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                   ctypes.POINTER(i64)], i),
        "picp_refine_params_default": ([pp], None),
        "picp_refine_create": ([ctypes.POINTER(vp), i, i, i, fp], i),
        "picp_refine_destroy": ([vp], i),
        "picp_refine_set_poses": ([vp, fp, i], i),
        "picp_refine_set_tracks": ([vp, i64, ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_int32), fp], i),
        "picp_refine_set_points": ([vp, fp], i),
        "picp_refine_run": ([vp, pp], i),
        "picp_refine_get_points": ([vp, fp], i),
        "picp_refine_get_stats": ([vp, sp], i),
        "picp_refine_time": ([vp, pp, i, fp], i),
        "picp_vo_set_track_log": ([vp, i], i),
        "picp_vo_get_tracks": ([vp, i, ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(i64),
                                ctypes.POINTER(i64), ctypes.POINTER(i64)], i),
        "picp_vo_get_poses_wc": ([vp, fp], i),
        "picp_vo_refine_map": ([vp, pp], i),
        "picp_vo_get_refined_map": ([vp, i, i64, fp, sp, ctypes.POINTER(i64)], i),
        "picp_vo_refine_time": ([vp, pp, i, fp, fp], i),
        "picp_adjust_params_default": ([ctypes.POINTER(AdjustParams)], None),
        "picp_refine_set_fixed_poses": ([vp, ctypes.POINTER(ctypes.c_uint8)], i),
        "picp_refine_run_poses": ([vp, pp], i),
        "picp_refine_adjust": ([vp, ctypes.POINTER(AdjustParams)], i),
        "picp_refine_get_poses": ([vp, fp], i),
        "picp_refine_get_pose_stats": ([vp, sp], i),
        "picp_refine_get_pose_view": ([vp, ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_int32), fp], i),
        "picp_refine_get_sweeps": ([vp, ctypes.POINTER(AdjustSweep), i, ctypes.POINTER(i)], i),
        "picp_refine_adjust_time": ([vp, ctypes.POINTER(AdjustParams), i, fp, fp, fp, fp], i),
        "picp_vo_adjust": ([vp, ctypes.POINTER(AdjustParams)], i),
        "picp_vo_get_adjusted_poses_wc": ([vp, fp], i),
        "picp_vo_get_adjusted_map": ([vp, i, i64, fp, sp, ctypes.POINTER(i64)], i),
        "picp_pnp_params_default": ([ctypes.POINTER(PnpParams)], None),
        "picp_pnp_batch": ([i, i, ctypes.POINTER(i64), fp, fp, fp, i, i, ctypes.POINTER(PnpParams), fp, i32p, i32p, u8p], i),
        "picp_pnp_batch_debug": ([i, i, ctypes.POINTER(i64), fp, fp, fp, i, i, ctypes.POINTER(PnpParams), fp, i32p, i32p,
                                  u8p, i32p, i32p, fp, i32p], i),
        "picp_pnp_batch_time": ([i, i, ctypes.POINTER(i64), fp, fp, fp, i, i, ctypes.POINTER(PnpParams), i, fp], i),
        "picp_relocalize": ([vp, ctypes.POINTER(PnpParams), i32p], i),
        "picp_sim3_params_default": ([ctypes.POINTER(Sim3Params)], None),
        "picp_sim3_batch": ([i, i, ctypes.POINTER(i64), fp, fp, ctypes.POINTER(Sim3Params), fp, fp, i32p, i32p, fp, u8p], i),
        "picp_sim3_batch_debug": ([i, i, ctypes.POINTER(i64), fp, fp, ctypes.POINTER(Sim3Params), fp, fp, i32p, i32p, fp,
                                   u8p, i32p, i32p, fp, i32p, fp, i32p], i),
        "picp_sim3_batch_time": ([i, i, ctypes.POINTER(i64), fp, fp, ctypes.POINTER(Sim3Params), i, fp], i),
        "picp_sim3_fit_batch": ([i, i, ctypes.POINTER(i64), fp, fp, u8p, i, fp, fp, fp, i32p], i),
        "picp_vo_align_segments": ([vp, ctypes.POINTER(Sim3Params), fp, fp, i32p, i32p, ctypes.POINTER(i64)], i),
        "picp_pgo_params_default": ([ctypes.POINTER(PgoParams)], None),
        "picp_pgo_batch": ([i, i, ctypes.POINTER(i64), ctypes.POINTER(i64), fp, u8p, i32p, fp, fp,
                            ctypes.POINTER(PgoParams), fp, dp, dp, dp, dp, i32p, i32p], i),
        "picp_pgo_batch_time": ([i, i, ctypes.POINTER(i64), ctypes.POINTER(i64), fp, u8p, i32p, fp, fp,
                                 ctypes.POINTER(PgoParams), i, fp], i),
    }
    for name, (args, res) in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    _lib = L
    return L


def _check(rc, allow=()):
    if rc != OK and rc not in allow:
        raise PicpError(rc, lib().picp_last_error().decode(errors="replace"))
    return rc


def _fptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a if shape is None else a.reshape(shape)


def pose_to_c(T):
    """4x4 (row, col) -> column-major float[16] (Eigen::Isometry3f memory)."""
    return np.ascontiguousarray(np.asarray(T, np.float32).T.reshape(16))


def pose_from_c(p16):
    return np.asarray(p16, np.float32).reshape(4, 4).T.copy()


def k_to_c(K):
    return np.ascontiguousarray(np.asarray(K, np.float32).T.reshape(9))


def device_count():
    n = ctypes.c_int(0)
    _check(lib().picp_device_count(ctypes.byref(n)))
    return n.value


def default_params(**kw):
    p = Params()
    lib().picp_params_default(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class PICPSolver:
    """pr::PICPSolver over the C-ABI (src/picp_solver.h:21-82).

    init(camera, world_points, image_points) copies the arrays to the device (the reference
    keeps raw pointers, src/picp_solver.cpp:21-22).  Correspondences are (image idx, world idx)
    pairs (src/picp_solver.cpp:65-66)."""

    def __init__(self, device=0, rows=480, cols=640, K=K_REF):
        self._h = ctypes.c_void_p()
        self.device = device
        _check(lib().picp_create(ctypes.byref(self._h), device, rows, cols, _fptr(k_to_c(K))))
        self._threshold = 1000.0  # src/picp_solver.cpp:14
        self._damping = 1.0       # src/picp_solver.cpp:11
        self._min_inliers = 0     # src/picp_solver.cpp:12
        self._stats = Stats()

    def close(self):
        if self._h:
            lib().picp_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- reference surface -------------------------------------------------------------
    def init(self, T_wc, world_points, image_points, rows=None, cols=None, K=None):
        if rows is not None:
            _check(lib().picp_set_camera(self._h, rows, cols, _fptr(k_to_c(K))))
        w = _f32(world_points, (-1,))
        im = _f32(image_points, (-1,))
        _check(lib().picp_set_points(self._h, _fptr(w), w.size // 3, _fptr(im), im.size // 2))
        self.set_pose(T_wc)

    def kernelThreshold(self):
        return self._threshold

    def setKernelThreshold(self, t):
        self._threshold = float(t)

    def chiInliers(self):
        return self._stats.chi_in

    def chiOutliers(self):
        return self._stats.chi_out

    def numInliers(self):
        return self._stats.n_in

    def set_pose(self, T_wc):
        _check(lib().picp_set_pose(self._h, _fptr(pose_to_c(T_wc))))

    def pose(self):
        out = np.zeros(16, np.float32)
        _check(lib().picp_get_pose(self._h, _fptr(out)))
        return pose_from_c(out)

    def set_correspondences(self, pairs):
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        _check(lib().picp_set_correspondences(
            self._h, pr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), pr.shape[0]))

    def oneRound(self, correspondences, keep_outliers=False):
        """Returns the reference's bool (False when n_in < min_inliers)."""
        self.set_correspondences(correspondences)
        rc = _check(lib().picp_one_round(self._h, self._threshold, self._damping,
                                         self._min_inliers, int(keep_outliers),
                                         ctypes.byref(self._stats)), allow=(TOO_FEW_INLIERS,))
        return rc == OK

    # --- extensions ----------------------------------------------------------------------
    def solve(self, correspondences, max_rounds=50, conv_eps=1e-5, keep_outliers=False):
        """exec/icp_test.cpp:88-107 fused on the device.  Returns stats dict."""
        self.set_correspondences(correspondences)
        prm = default_params(threshold=self._threshold, damping=self._damping,
                             min_inliers=self._min_inliers, keep_outliers=int(keep_outliers),
                             max_rounds=max_rounds, conv_eps=conv_eps)
        _check(lib().picp_solve(self._h, ctypes.byref(prm), ctypes.byref(self._stats)))
        return self._stats.as_dict()

    def linearize(self, correspondences, keep_outliers=False):
        self.set_correspondences(correspondences)
        H = np.zeros(36, np.float64)
        b = np.zeros(6, np.float64)
        st = Stats()
        _check(lib().picp_linearize(self._h, self._threshold, int(keep_outliers),
                                    H.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                    b.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                    ctypes.byref(st)))
        return {"H": H.reshape(6, 6).T.copy(), "b": b, **st.as_dict()}

    def classify(self, correspondences):
        """picp_classify at the current pose and kernel threshold: which correspondences the pose
        rests on.  Returns dict(state (m,) uint8 CORR_*, chi2 (m,), uv (m, 2) (-1 where skipped),
        inlier_idx (ascending correspondence indices of the inliers), counts (skipped, inlier,
        outlier)).  Leaves the pose and the stats alone."""
        self.set_correspondences(correspondences)
        m = np.ascontiguousarray(correspondences, np.int32).reshape(-1, 2).shape[0]
        state = np.zeros(max(m, 1), np.uint8)
        chi2 = np.zeros(max(m, 1), np.float32)
        uv = np.zeros(2 * max(m, 1), np.float32)
        idx = np.zeros(max(m, 1), np.int32)
        counts = np.zeros(3, np.int64)
        _check(lib().picp_classify(self._h, self._threshold, state.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                   _fptr(chi2), _fptr(uv), _i32ptr(idx),
                                   counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return {"state": state[:m], "chi2": chi2[:m], "uv": uv[:2 * m].reshape(-1, 2),
                "inlier_idx": idx[:int(counts[1])], "counts": counts}

    def relocalize(self, correspondences, threshold=9.0, hypotheses=256, min_inliers=4, seed=0):
        """picp_relocalize: P3P RANSAC on the correspondences, no prior needed.  On success the pose
        is the winner (polish it with solve()).  Returns (found, inliers); a failure leaves the pose
        and the stats as they were."""
        self.set_correspondences(correspondences)
        prm = PnpParams(threshold, hypotheses, min_inliers, 0, seed)
        n = ctypes.c_int32(0)
        rc = _check(lib().picp_relocalize(self._h, ctypes.byref(prm), ctypes.byref(n)), allow=(TOO_FEW_INLIERS,))
        return rc == OK, n.value


class Batch:
    """Independent PICP problems (frames) solved together on one device."""

    def __init__(self, sizes, device=0, rows=480, cols=640, K=K_REF):
        sizes = np.asarray(sizes, np.int64)
        offs = np.zeros(len(sizes) + 1, np.int64)
        offs[1:] = np.cumsum(sizes)
        self.offs = offs
        self.n = len(sizes)
        self.device = device
        self._b = ctypes.c_void_p()
        _check(lib().picp_batch_create(ctypes.byref(self._b), device, self.n,
                                       offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                       rows, cols, _fptr(k_to_c(K))))

    def close(self):
        if self._b:
            lib().picp_batch_destroy(self._b)
            self._b = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_data(self, xyz, uv):
        xyz = _f32(xyz, (-1,))
        uv = _f32(uv, (-1,))
        assert xyz.size == 3 * self.offs[-1] and uv.size == 2 * self.offs[-1]
        _check(lib().picp_batch_set_data(self._b, _fptr(xyz), _fptr(uv)))

    def set_poses(self, Ts):
        Ts = np.asarray(Ts, np.float32).reshape(self.n, 4, 4)
        flat = np.ascontiguousarray(np.transpose(Ts, (0, 2, 1)).reshape(-1))
        _check(lib().picp_batch_set_poses(self._b, _fptr(flat)))

    def poses(self):
        out = np.zeros(16 * self.n, np.float32)
        _check(lib().picp_batch_get_poses(self._b, _fptr(out)))
        return np.transpose(out.reshape(self.n, 4, 4), (0, 2, 1)).copy()

    def stats(self):
        st = (Stats * self.n)()
        _check(lib().picp_batch_get_stats(self._b, st))
        return [s.as_dict() for s in st]

    def solve(self, **params):
        prm = default_params(**params)
        _check(lib().picp_batch_solve(self._b, ctypes.byref(prm)))

    def solve_async(self, **params):
        prm = default_params(**params)
        _check(lib().picp_batch_solve_async(self._b, ctypes.byref(prm)))

    def sync(self):
        _check(lib().picp_batch_sync(self._b))

    def classify(self, threshold, poses=None, want_chi2=True):
        """picp_batch_classify at `poses` ((n, 4, 4) world-in-camera), or at the batch's current
        poses (the last solve's, or those of a set_poses since).  Returns dict(state, chi2 (packed
        order), inlier_off (n+1), inlier_idx (per problem ascending, relative to the problem's
        first correspondence), counts (n, 3) skipped / inlier / outlier)."""
        tot = int(self.offs[-1])
        flat = None
        if poses is not None:
            Ts = np.asarray(poses, np.float32).reshape(self.n, 4, 4)
            flat = np.ascontiguousarray(np.transpose(Ts, (0, 2, 1)).reshape(-1))
        state = np.zeros(max(tot, 1), np.uint8)
        chi2 = np.zeros(max(tot, 1), np.float32) if want_chi2 else None
        idx = np.zeros(max(tot, 1), np.int32)
        off = np.zeros(self.n + 1, np.int64)
        counts = np.zeros(3 * self.n, np.int64)
        i64p = ctypes.POINTER(ctypes.c_int64)
        _check(lib().picp_batch_classify(self._b, threshold, _fptr(flat) if flat is not None else None,
                                         state.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                         _fptr(chi2) if want_chi2 else None, off.ctypes.data_as(i64p),
                                         _i32ptr(idx), counts.ctypes.data_as(i64p)))
        return {"state": state[:tot], "chi2": chi2[:tot] if want_chi2 else None, "inlier_off": off,
                "inlier_idx": idx[:int(off[-1])], "counts": counts.reshape(self.n, 3)}

    def classify_time(self, threshold, reps):
        """Mean device time (us) of one classify pass (kernels only) at the current poses, with
        the outputs of the last classify() call."""
        us = ctypes.c_float(0)
        _check(lib().picp_batch_classify_time(self._b, threshold, reps, ctypes.byref(us)))
        return us.value

    def time(self, reps, **params):
        """reps back-to-back solves between two HIP events -> (total ms, mean launch period us)."""
        prm = default_params(**params)
        total = ctypes.c_float(0)
        lus = ctypes.c_float(0)
        _check(lib().picp_batch_time(self._b, ctypes.byref(prm), reps, ctypes.byref(total), ctypes.byref(lus)))
        return total.value, lus.value

    def time_single(self, **params):
        """Diagnostic: event pair around each launch of one solve (us; graph mode: per round)."""
        prm = default_params(**params)
        us = ctypes.c_float(0)
        _check(lib().picp_batch_time_single(self._b, ctypes.byref(prm), ctypes.byref(us)))
        return us.value

    def residency(self):
        g, r, f = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _check(lib().picp_batch_residency(self._b, ctypes.byref(g), ctypes.byref(r), ctypes.byref(f)))
        return {"handoff_grid": g.value, "resident_blocks": r.value, "fallbacks": f.value}

    def info(self):
        tot = ctypes.c_int64(0)
        nb = ctypes.c_int(0)
        mode = ctypes.c_int(0)
        _check(lib().picp_batch_info(self._b, ctypes.byref(tot), ctypes.byref(nb), ctypes.byref(mode)))
        return {"total_corr": tot.value, "n_blocks": nb.value,
                "mode": {0: "graph", 1: "persistent", 2: "block"}[mode.value]}


def shard_range(n_items, world, rank):
    """picp_shard_range: the contiguous [first, last) of n_items that rank owns."""
    a, e = ctypes.c_int64(0), ctypes.c_int64(0)
    _check(lib().picp_shard_range(n_items, world, rank, ctypes.byref(a), ctypes.byref(e)))
    return a.value, e.value


def shard_pad(n_items, world):
    """picp_shard_pad: rows per rank in the padded all-gather (ceil(n_items / world))."""
    r = lib().picp_shard_pad(n_items, world)
    if r < 0:
        raise PicpError(ERR_ARG, "picp_shard_pad: bad size")
    return int(r)


def shard_unpack(padded, n_items, world):
    """picp_shard_unpack: the (world * pad, ...) rank-ordered padded rows -> (n_items, ...) in
    problem order (host code: no device needed)."""
    padded = np.ascontiguousarray(padded)
    pad = shard_pad(n_items, world)
    assert padded.shape[0] == world * max(pad, 1) or (n_items == 0), "padded buffer has the wrong row count"
    row = padded.dtype.itemsize * int(np.prod(padded.shape[1:], dtype=np.int64))
    out = np.empty((n_items,) + padded.shape[1:], padded.dtype)
    _check(lib().picp_shard_unpack(n_items, world, row, padded.ctypes.data_as(ctypes.c_void_p),
                                   out.ctypes.data_as(ctypes.c_void_p)))
    return out


def comm_unique_id():
    """RCCL unique id (bytes) for Comm; rank 0 makes it, the launcher passes it to every rank."""
    buf = (ctypes.c_uint8 * COMM_ID_BYTES)()
    _check(lib().picp_comm_unique_id(buf))
    return bytes(buf)


class Comm:
    """picp_comm_t: this rank's RCCL communicator of the batch split, driven by the C++ library."""

    def __init__(self, device, world, rank, uid):
        assert len(uid) == COMM_ID_BYTES
        self._c = ctypes.c_void_p()
        buf = (ctypes.c_uint8 * COMM_ID_BYTES).from_buffer_copy(uid)
        _check(lib().picp_comm_create(ctypes.byref(self._c), device, world, rank, buf))
        self.device, self.world, self.rank = device, world, rank

    def close(self):
        if self._c:
            lib().picp_comm_destroy(self._c)
            self._c = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def allreduce_max(self, values):
        v = np.ascontiguousarray(values, np.float64).reshape(-1).copy()
        _check(lib().picp_comm_allreduce_max(self._c, v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), v.size))
        return v

    def barrier(self):
        _check(lib().picp_comm_barrier(self._c))

    def allgather_batch(self, batch, n_total):
        """Every rank's poses (n_total, 4, 4) and stats dicts, after this rank's batch solve."""
        T = np.zeros(16 * n_total, np.float32)
        st = (Stats * max(n_total, 1))()
        _check(lib().picp_batch_allgather(batch._b, self._c, n_total, _fptr(T), st))
        return np.transpose(T.reshape(n_total, 4, 4), (0, 2, 1)).copy(), [st[k].as_dict() for k in range(n_total)]


def allgather_batch_host(batch, world, rank, n_total, exchange):
    """picp_batch_allgather_host: the batch split's gather with the byte exchange done by the caller.
    exchange(send: bytes) -> bytes of world * len(send), rank order (e.g. a gloo all_gather).
    Returns every rank's poses (n_total, 4, 4) and stats dicts, like Comm.allgather_batch."""
    err = []

    def cb(user, send, recv, nbytes):
        try:
            out = exchange(ctypes.string_at(send, nbytes))
            if len(out) != world * nbytes:
                return 1
            ctypes.memmove(recv, out, len(out))
            return 0
        except Exception as e:  # reported through the library's status, never across the C frame
            err.append(e)
            return 2

    fn = EXCHANGE_FN(cb)
    T = np.zeros(16 * max(n_total, 1), np.float32)
    st = (Stats * max(n_total, 1))()
    rc = lib().picp_batch_allgather_host(batch._b, world, rank, fn, None, n_total, _fptr(T), st)
    if err:
        raise err[0]
    _check(rc)
    return (np.transpose(T[:16 * n_total].reshape(n_total, 4, 4), (0, 2, 1)).copy(),
            [st[k].as_dict() for k in range(n_total)])


def projection_matrix(K, T_cw):
    P = np.zeros(12, np.float32)
    _check(lib().picp_projection_matrix(_fptr(k_to_c(K)), _fptr(pose_to_c(T_cw)), _fptr(P)))
    return P.reshape(3, 4)


def triangulate(P1, P2, uv1, uv2, device=0):
    uv1 = _f32(uv1, (-1, 2))
    uv2 = _f32(uv2, (-1, 2))
    out = np.zeros((uv1.shape[0], 3), np.float32)
    _check(lib().picp_triangulate(device, _fptr(_f32(P1, (12,))), _fptr(_f32(P2, (12,))),
                                  _fptr(uv1), _fptr(uv2), uv1.shape[0], _fptr(out)))
    return out


def _i32ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


# picp_match_batch_form kernel forms (include/picp_c.h PICP_MATCH_FORM_*)
MATCH_FORMS = {"full": 0, "accept_only": 1, "exact": 2}


def match_points(desc1, desc2, dist_thr=0.2, ratio_thr=0.8, device=0, form="full"):
    """match_points (src/my_utilities.h:70-120) on the GPU -> dict(best_idx, best_dist,
    second_dist, accepted); the reference's correspondences are the accepted (i, best_idx[i]).
    form: "full" (default), "accept_only" (only accepted and the best index of accepted queries
    are defined: the form the VO sequence runs) or "exact" (the exact scan; the same bits)."""
    d1 = np.asarray(desc1, np.float32)
    d2 = np.asarray(desc2, np.float32)
    dim = d1.shape[1] if d1.ndim == 2 and d1.shape[1] else (d2.shape[1] if d2.ndim == 2 else 10)
    return match_points_batch([d1.reshape(-1, dim)], [d2.reshape(-1, dim)], dist_thr, ratio_thr, device, form=form)[0]


def match_points_batch(desc1_list, desc2_list, dist_thr=0.2, ratio_thr=0.8, device=0, form="full"):
    """Many (set 1, set 2) pairs in one launch; returns a list of per-problem dicts."""
    o1 = np.zeros(len(desc1_list) + 1, np.int64)
    o2 = np.zeros(len(desc2_list) + 1, np.int64)
    o1[1:] = np.cumsum([len(d) for d in desc1_list])
    o2[1:] = np.cumsum([len(d) for d in desc2_list])
    dim = next((np.asarray(d).shape[1] for d in list(desc1_list) + list(desc2_list) if len(d)), 10)
    d1 = np.ascontiguousarray(np.concatenate([np.asarray(d, np.float32).reshape(-1, dim) for d in desc1_list]))
    d2 = np.ascontiguousarray(np.concatenate([np.asarray(d, np.float32).reshape(-1, dim) for d in desc2_list]))
    n1 = int(o1[-1])
    bi = np.zeros(n1, np.int32)
    bd = np.zeros(n1, np.float32)
    sd = np.zeros(n1, np.float32)
    acc = np.zeros(n1, np.int32)
    if n1 == 0:
        return [{"best_idx": bi, "best_dist": bd, "second_dist": sd, "accepted": acc.astype(bool)}
                for _ in desc1_list]
    _check(lib().picp_match_batch_form(device, len(desc1_list), o1.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                       o2.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _fptr(d1),
                                       _fptr(d2) if d2.size else None, dim, dist_thr, ratio_thr,
                                       _i32ptr(bi), _fptr(bd), _fptr(sd), _i32ptr(acc), MATCH_FORMS[form]))
    return [{"best_idx": bi[o1[i]:o1[i + 1]], "best_dist": bd[o1[i]:o1[i + 1]],
             "second_dist": sd[o1[i]:o1[i + 1]], "accepted": acc[o1[i]:o1[i + 1]].astype(bool)}
            for i in range(len(desc1_list))]


class EssentialParams(ctypes.Structure):
    """picp_essential_params (include/picp_c.h): cv::findEssentialMat / cv::recoverPose knobs."""
    _fields_ = [("prob", ctypes.c_double), ("threshold", ctypes.c_double), ("max_iters", ctypes.c_int),
                ("reserved", ctypes.c_int), ("dist", ctypes.c_double)]


def essential_recover_pose_batch(p1_list, p2_list, K=None, prob=0.999, threshold=1.0, max_iters=1000,
                                 dist=50.0, device=0, want_mask=False):
    """Cam::computeEssentialAndRecoverPose (src/cam.cpp:37-91) on the GPU for many two-view
    problems: findEssentialMat(RANSAC) + recoverPose.  Returns per problem a dict with T (4x4
    camera-in-world of the second view, the first at the origin, unit baseline), inliers, good
    (and mask)."""
    K = K_REF if K is None else K
    offs = np.zeros(len(p1_list) + 1, np.int64)
    offs[1:] = np.cumsum([len(p) for p in p1_list])
    n = int(offs[-1])
    p1 = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float32).reshape(-1, 2) for p in p1_list])
                              if n else np.zeros((0, 2), np.float32))
    p2 = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float32).reshape(-1, 2) for p in p2_list])
                              if n else np.zeros((0, 2), np.float32))
    prm = EssentialParams(prob, threshold, max_iters, 0, dist)
    T = np.zeros(16 * len(p1_list), np.float32)
    inl = np.zeros(len(p1_list), np.int32)
    good = np.zeros(len(p1_list), np.int32)
    mask = np.zeros(max(n, 1), np.uint8) if want_mask else None
    _check(lib().picp_essential_batch(device, len(p1_list), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                      _fptr(p1) if n else None, _fptr(p2) if n else None, _fptr(k_to_c(K)),
                                      ctypes.byref(prm), _fptr(T), _i32ptr(inl), _i32ptr(good),
                                      mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if want_mask else None))
    out = []
    for i in range(len(p1_list)):
        d = {"T": pose_from_c(T[16 * i:16 * i + 16]), "inliers": int(inl[i]), "good": int(good[i])}
        if want_mask:
            d["mask"] = mask[offs[i]:offs[i + 1]].astype(bool)
        out.append(d)
    return out


def _pnp_pack(xyz_list, uv_list):
    offs = np.zeros(len(xyz_list) + 1, np.int64)
    offs[1:] = np.cumsum([len(x) for x in xyz_list])
    n = int(offs[-1])
    xyz = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x in xyz_list])
                               if n else np.zeros((0, 3), np.float32))
    uv = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1, 2) for x in uv_list])
                              if n else np.zeros((0, 2), np.float32))
    assert len(xyz) == len(uv) == n
    return offs, xyz, uv


def pnp_ransac_batch(xyz_list, uv_list, K=None, rows=480, cols=640, threshold=9.0, hypotheses=256, min_inliers=4,
                     seed=0, want_mask=False, debug=False, device=0):
    """picp_pnp_batch: absolute pose without a prior for many 2D-3D problems (P3P inside RANSAC,
    scored with the solver's gate at `threshold`).  Returns per problem a dict with T (4x4
    world-in-camera; the identity when found is False), inliers, found (and mask); with debug also
    samples (H, 3), n_roots (H,), hyp_T (H, 4, 4, 4) and hyp_count (H, 4)."""
    K = K_REF if K is None else K
    P = len(xyz_list)
    offs, xyz, uv = _pnp_pack(xyz_list, uv_list)
    n, H = int(offs[-1]), hypotheses
    prm = PnpParams(threshold, hypotheses, min_inliers, 0, seed)
    T = np.zeros(16 * max(P, 1), np.float32)
    inl = np.zeros(max(P, 1), np.int32)
    found = np.zeros(max(P, 1), np.int32)
    mask = np.zeros(max(n, 1), np.uint8) if want_mask else None
    u8 = ctypes.POINTER(ctypes.c_uint8)
    args = [device, P, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _fptr(xyz) if n else None,
            _fptr(uv) if n else None, _fptr(k_to_c(K)), rows, cols, ctypes.byref(prm), _fptr(T), _i32ptr(inl),
            _i32ptr(found), mask.ctypes.data_as(u8) if want_mask else None]
    if debug:
        G = max(P * max(H, 0), 1)
        smp = np.zeros(3 * G, np.int32)
        nr = np.zeros(G, np.int32)
        hT = np.zeros(64 * G, np.float32)
        hc = np.zeros(4 * G, np.int32)
        _check(lib().picp_pnp_batch_debug(*args, _i32ptr(smp), _i32ptr(nr), _fptr(hT), _i32ptr(hc)))
    else:
        _check(lib().picp_pnp_batch(*args))
    out = []
    for i in range(P):
        d = {"T": pose_from_c(T[16 * i:16 * i + 16]), "inliers": int(inl[i]), "found": bool(found[i])}
        if want_mask:
            d["mask"] = mask[offs[i]:offs[i + 1]].astype(bool)
        if debug:
            g = slice(i * H, (i + 1) * H)
            d["samples"] = smp.reshape(-1, 3)[g]
            d["n_roots"] = nr[g]
            d["hyp_T"] = np.transpose(hT.reshape(-1, 4, 4, 4)[g], (0, 1, 3, 2)).copy()
            d["hyp_count"] = hc.reshape(-1, 4)[g]
        out.append(d)
    return out


def pnp_ransac_time(xyz_list, uv_list, reps, K=None, rows=480, cols=640, threshold=9.0, hypotheses=256, seed=0,
                    device=0):
    """picp_pnp_batch_time: mean device time in us of the (samples, solve, score, select) stages."""
    K = K_REF if K is None else K
    offs, xyz, uv = _pnp_pack(xyz_list, uv_list)
    prm = PnpParams(threshold, hypotheses, 4, 0, seed)
    us = np.zeros(4, np.float32)
    _check(lib().picp_pnp_batch_time(device, len(xyz_list), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                     _fptr(xyz), _fptr(uv), _fptr(k_to_c(K)), rows, cols, ctypes.byref(prm), reps,
                                     _fptr(us)))
    return tuple(float(x) for x in us)


def _sim3_pack(src_list, dst_list):
    offs = np.zeros(len(src_list) + 1, np.int64)
    offs[1:] = np.cumsum([len(x) for x in src_list])
    n = int(offs[-1])
    pack = lambda L: np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x in L])
                                          if n else np.zeros((0, 3), np.float32))
    src, dst = pack(src_list), pack(dst_list)
    assert len(src) == len(dst) == n and all(len(a) == len(b) for a, b in zip(src_list, dst_list))
    return offs, src, dst


def default_sim3_params(**kw):
    p = Sim3Params()
    lib().picp_sim3_params_default(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def sim3_ransac_batch(src_list, dst_list, threshold=0.01, hypotheses=256, min_inliers=4, with_scale=True, refits=2,
                      seed=0, want_mask=False, debug=False, device=0):
    """picp_sim3_batch: the similarity dst ~ c R src + t of many sets of 3D-3D matches, robust to wrong
    ones (Umeyama's closed form inside RANSAC, then `refits` least-squares refits of the inliers;
    `threshold` is a squared distance in dst units).  Returns per problem a dict with S (4x4
    [[c R, t], [0, 1]]; the identity when found is False), scale, inliers, found, rms (and mask);
    with debug also samples (H, 3), hyp_valid (H,), hyp_S (H, 4, 4), hyp_count (H,), refit_S
    (refits, 4, 4) and refit_count (refits,)."""
    P = len(src_list)
    offs, src, dst = _sim3_pack(src_list, dst_list)
    n, H = int(offs[-1]), hypotheses
    prm = Sim3Params(threshold, hypotheses, min_inliers, 1 if with_scale else 0, refits, 0, seed)
    S = np.zeros(16 * max(P, 1), np.float32)
    scale = np.zeros(max(P, 1), np.float32)
    inl = np.zeros(max(P, 1), np.int32)
    found = np.zeros(max(P, 1), np.int32)
    rms = np.zeros(max(P, 1), np.float32)
    mask = np.zeros(max(n, 1), np.uint8) if want_mask else None
    u8 = ctypes.POINTER(ctypes.c_uint8)
    args = [device, P, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _fptr(src) if n else None,
            _fptr(dst) if n else None, ctypes.byref(prm), _fptr(S), _fptr(scale), _i32ptr(inl), _i32ptr(found),
            _fptr(rms), mask.ctypes.data_as(u8) if want_mask else None]
    if debug:
        G, NR = max(P * max(H, 0), 1), max(P * max(refits, 0), 1)
        smp = np.zeros(3 * G, np.int32)
        hv = np.zeros(G, np.int32)
        hS = np.zeros(16 * G, np.float32)
        hc = np.zeros(G, np.int32)
        rS = np.zeros(16 * NR, np.float32)
        rc = np.zeros(NR, np.int32)
        _check(lib().picp_sim3_batch_debug(*args, _i32ptr(smp), _i32ptr(hv), _fptr(hS), _i32ptr(hc), _fptr(rS),
                                           _i32ptr(rc)))
    else:
        _check(lib().picp_sim3_batch(*args))
    out = []
    for i in range(P):
        d = {"S": pose_from_c(S[16 * i:16 * i + 16]), "scale": float(scale[i]), "inliers": int(inl[i]),
             "found": bool(found[i]), "rms": float(rms[i])}
        if want_mask:
            d["mask"] = mask[offs[i]:offs[i + 1]].astype(bool)
        if debug:
            g, r = slice(i * H, (i + 1) * H), slice(i * refits, (i + 1) * refits)
            d["samples"] = smp.reshape(-1, 3)[g]
            d["hyp_valid"] = hv[g]
            d["hyp_S"] = np.transpose(hS.reshape(-1, 4, 4)[g], (0, 2, 1)).copy()
            d["hyp_count"] = hc[g]
            d["refit_S"] = np.transpose(rS.reshape(-1, 4, 4)[r], (0, 2, 1)).copy()
            d["refit_count"] = rc[r]
        out.append(d)
    return out


def sim3_fit_batch(src_list, dst_list, mask_list=None, with_scale=True, device=0):
    """picp_sim3_fit_batch: the least-squares similarity of every finite pair (of those whose mask
    entry is set), one per problem -> list of dict(S, scale, rms, found)."""
    P = len(src_list)
    offs, src, dst = _sim3_pack(src_list, dst_list)
    n = int(offs[-1])
    mask = None
    if mask_list is not None:
        mask = np.ascontiguousarray(np.concatenate([np.asarray(m).astype(np.uint8).reshape(-1) for m in mask_list])
                                    if n else np.zeros(0, np.uint8))
        assert len(mask) == n
    S = np.zeros(16 * max(P, 1), np.float32)
    scale = np.zeros(max(P, 1), np.float32)
    rms = np.zeros(max(P, 1), np.float32)
    found = np.zeros(max(P, 1), np.int32)
    _check(lib().picp_sim3_fit_batch(device, P, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                     _fptr(src) if n else None, _fptr(dst) if n else None,
                                     mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if mask is not None and n else None,
                                     1 if with_scale else 0, _fptr(S), _fptr(scale), _fptr(rms), _i32ptr(found)))
    return [{"S": pose_from_c(S[16 * i:16 * i + 16]), "scale": float(scale[i]), "rms": float(rms[i]),
             "found": bool(found[i])} for i in range(P)]


def sim3_ransac_time(src_list, dst_list, reps, threshold=0.01, hypotheses=256, with_scale=True, refits=2, seed=0,
                     device=0):
    """picp_sim3_batch_time: mean device time in us of the (samples, hypotheses, score, select, refit) stages."""
    offs, src, dst = _sim3_pack(src_list, dst_list)
    prm = Sim3Params(threshold, hypotheses, 4, 1 if with_scale else 0, refits, 0, seed)
    us = np.zeros(5, np.float32)
    _check(lib().picp_sim3_batch_time(device, len(src_list), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                      _fptr(src), _fptr(dst), ctypes.byref(prm), reps, _fptr(us)))
    return tuple(float(x) for x in us)


def default_pgo_params(**kw):
    p = PgoParams()
    lib().picp_pgo_params_default(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _pgo_pack(graphs):
    """The ragged arrays of picp_pgo_batch from dicts with S (n, 4, 4), fixed (n,), edges (m, 2), Z (m, 4, 4)
    and, in all of them or in none, weight (m,)."""
    G = len(graphs)
    node_off, edge_off = np.zeros(G + 1, np.int64), np.zeros(G + 1, np.int64)
    S, fixed, idx, Z, w = [], [], [], [], []
    has_w = [g.get("weight") is not None for g in graphs]
    assert all(has_w) or not any(has_w), "weights in every graph or in none"
    for k, g in enumerate(graphs):
        s = np.asarray(g["S"], np.float32).reshape(-1, 4, 4)
        e = np.asarray(g["edges"], np.int32).reshape(-1, 2)
        z = np.asarray(g["Z"], np.float32).reshape(-1, 4, 4)
        f = np.asarray(g["fixed"]).astype(np.uint8).reshape(-1)
        assert len(f) == len(s) and len(z) == len(e)
        node_off[k + 1], edge_off[k + 1] = node_off[k] + len(s), edge_off[k] + len(e)
        S.append(np.transpose(s, (0, 2, 1)).reshape(-1))  # column-major
        Z.append(np.transpose(z, (0, 2, 1)).reshape(-1))
        fixed.append(f)
        idx.append(e.reshape(-1))
        if has_w[k]:
            w.append(np.asarray(g["weight"], np.float32).reshape(-1))
            assert len(w[-1]) == len(e)
    cat = lambda L, t: np.ascontiguousarray(np.concatenate(L) if L else np.zeros(0, t), dtype=t)
    return (node_off, edge_off, cat(S, np.float32), cat(fixed, np.uint8), cat(idx, np.int32), cat(Z, np.float32),
            cat(w, np.float32) if G and all(has_w) else None)


def _pgo_args(device, graphs, packed):
    node_off, edge_off, S, fixed, idx, Z, w = packed
    i64p, u8p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint8)
    return [device, len(graphs), node_off.ctypes.data_as(i64p), edge_off.ctypes.data_as(i64p),
            _fptr(S) if len(S) else None, fixed.ctypes.data_as(u8p) if len(fixed) else None,
            _i32ptr(idx) if len(idx) else None, _fptr(Z) if len(Z) else None, _fptr(w) if w is not None and len(w) else None]


def pose_graph_batch(graphs, with_scale=True, iterations=10, damping=0.0, eps=0.0, device=0):
    """picp_pgo_batch: pose-graph optimisation over Sim(3) of many graphs.  Each graph is a dict with S
    (n, 4, 4) [[c R, t], [0, 1]] mapping node k's frame into the common frame, fixed (n,), edges
    (m, 2) local (i, j), Z (m, 4, 4) mapping node j's frame into node i's and optionally weight (m,).
    Returns per graph a dict with S (n, 4, 4) float32, cost_initial, cost_final, grad_initial,
    grad_final, steps and status (PGO_*); a graph whose status is not PGO_OK keeps its input S."""
    G = len(graphs)
    packed = _pgo_pack(graphs)
    node_off = packed[0]
    prm = PgoParams(1 if with_scale else 0, iterations, damping, eps)
    So = np.zeros(16 * max(int(node_off[-1]), 1), np.float32)
    fig = [np.zeros(max(G, 1), np.float64) for _ in range(4)]
    steps, status = np.zeros(max(G, 1), np.int32), np.zeros(max(G, 1), np.int32)
    dptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    _check(lib().picp_pgo_batch(*_pgo_args(device, graphs, packed), ctypes.byref(prm), _fptr(So), dptr(fig[0]),
                                dptr(fig[1]), dptr(fig[2]), dptr(fig[3]), _i32ptr(steps), _i32ptr(status)))
    out = []
    for k in range(G):
        s = So[16 * node_off[k]:16 * node_off[k + 1]].reshape(-1, 4, 4)
        out.append({"S": np.transpose(s, (0, 2, 1)).copy(), "cost_initial": float(fig[0][k]),
                    "cost_final": float(fig[1][k]), "grad_initial": float(fig[2][k]), "grad_final": float(fig[3][k]),
                    "steps": int(steps[k]), "status": int(status[k])})
    return out


def pose_graph_time(graphs, reps, with_scale=True, iterations=10, damping=0.0, eps=0.0, device=0):
    """picp_pgo_batch_time: mean device time in us of the solve's one launch."""
    packed = _pgo_pack(graphs)
    prm = PgoParams(1 if with_scale else 0, iterations, damping, eps)
    us = np.zeros(1, np.float32)
    _check(lib().picp_pgo_batch_time(*_pgo_args(device, graphs, packed), ctypes.byref(prm), reps, _fptr(us)))
    return float(us[0])


class VOSequence:
    """Device-resident VO over a packed observation sequence (C-ABI picp_vo_*): the reference's
    per-frame loop (exec/icp_test.cpp:61-136) run on the GPU for independent segments in
    lockstep.  Poses are camera-in-world 4x4 (numpy row/col)."""

    def __init__(self, frame_off, uv, desc, device=0, rows=480, cols=640, K=K_REF):
        self.frame_off = np.ascontiguousarray(frame_off, np.int64)
        uv = _f32(uv, (-1,))
        desc = np.ascontiguousarray(desc, np.float32)
        self.dim = desc.shape[1]
        self.n_frames = len(self.frame_off) - 1
        self._h = ctypes.c_void_p()
        _check(lib().picp_vo_create(ctypes.byref(self._h), device, rows, cols, _fptr(k_to_c(K)),
                                    self.n_frames, self.frame_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                    _fptr(uv), _fptr(desc.reshape(-1)), self.dim))
        self.first = self.steps = None

    def close(self):
        if self._h:
            lib().picp_vo_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_segments(self, first, steps, boot_poses, threshold=3000.0, **params):
        """boot_poses: (n_seg, 2, 4, 4) camera-in-world poses of frames first and first+1."""
        first = np.ascontiguousarray(first, np.int64)
        steps = np.ascontiguousarray(steps, np.int32)
        B = np.asarray(boot_poses, np.float32).reshape(len(first), 2, 4, 4)
        flat = np.ascontiguousarray(np.transpose(B, (0, 1, 3, 2)).reshape(-1))
        p = default_params(threshold=threshold, **params)
        _check(lib().picp_vo_set_segments(self._h, len(first), first.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                          steps.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                          _fptr(flat), ctypes.byref(p)))
        # a rejected call leaves the handle (and this view of it) unchanged
        self.first, self.steps = first, steps

    def run(self):
        _check(lib().picp_vo_run(self._h))

    def time(self, reps):
        ms = ctypes.c_float()
        _check(lib().picp_vo_time(self._h, reps, ctypes.byref(ms)))
        return ms.value

    def info(self):
        n_obs, n_slots, map_slots, npt = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
        _check(lib().picp_vo_info(self._h, ctypes.byref(n_obs), ctypes.byref(n_slots), ctypes.byref(map_slots),
                                  ctypes.byref(npt)))
        return {"n_obs": n_obs.value, "n_slots": n_slots.value, "map_slots": map_slots.value, "npt": npt.value}

    def _split(self, flat):
        out, o = [], 0
        for st in self.steps:
            out.append(flat[o:o + st + 1])
            o += st + 1
        return out

    def poses(self):
        """list over segments of (steps+1, 4, 4) camera-in-world poses ([0] = bootstrap pose)."""
        n = int((self.steps + 1).sum())
        out = np.zeros(16 * n, np.float32)
        _check(lib().picp_vo_get_poses(self._h, _fptr(out)))
        return self._split(np.transpose(out.reshape(n, 4, 4), (0, 2, 1)).copy())

    def step_records(self):
        """list over segments of dicts of arrays (steps+1 entries; entry 0 = bootstrap)."""
        n = int((self.steps + 1).sum())
        arr = (VOStep * n)()
        _check(lib().picp_vo_get_steps(self._h, arr))
        recs = {k: np.array([getattr(a, k) for a in arr]) for k, _ in VOStep._fields_}
        out, o = [], 0
        for st in self.steps:
            out.append({k: v[o:o + st + 1] for k, v in recs.items()})
            o += st + 1
        return out

    def track_stats(self, enable=True):
        """Switch the per-map-point track counters (off by default); takes effect at the next run."""
        _check(lib().picp_vo_set_track_stats(self._h, int(bool(enable))))

    def map_stats(self, seg):
        """(n_matched, n_inlier) per map point of segment seg after a run with tracking on:
        accepted frame->map matches of the point, and those that are inliers at their step's final
        PICP pose.  Raises PicpError(ERR_STATE) with tracking off."""
        n = ctypes.c_int64()
        _check(lib().picp_vo_get_map_stats(self._h, seg, 0, None, None, ctypes.byref(n)))
        nm = np.zeros(max(n.value, 1), np.int32)
        ni = np.zeros(max(n.value, 1), np.int32)
        _check(lib().picp_vo_get_map_stats(self._h, seg, n.value, _i32ptr(nm), _i32ptr(ni), ctypes.byref(n)))
        return nm[:n.value], ni[:n.value]

    def track_log(self, enable=True):
        """Switch the recording of observation tracks (off by default); takes effect at the next run."""
        _check(lib().picp_vo_set_track_log(self._h, int(bool(enable))))

    def tracks(self, seg):
        """(track_off, obs_slot, obs_index) of segment seg after a run with the track log on: map
        point j (in map(seg)'s order) owns entries [track_off[j], track_off[j+1]) of obs_slot (the
        pose slot inside the segment) and obs_index (the index into the uv / desc arrays the
        sequence was created from), ascending by obs_index.  Raises PicpError(ERR_STATE) with the
        log off or before a run."""
        n, m = ctypes.c_int64(), ctypes.c_int64()
        _check(lib().picp_vo_get_tracks(self._h, seg, None, None, None, ctypes.byref(n), ctypes.byref(m)))
        off = np.zeros(n.value + 1, np.int64)
        slot = np.zeros(max(m.value, 1), np.int32)
        idx = np.zeros(max(m.value, 1), np.int64)
        i64p = ctypes.POINTER(ctypes.c_int64)
        _check(lib().picp_vo_get_tracks(self._h, seg, off.ctypes.data_as(i64p), _i32ptr(slot),
                                        idx.ctypes.data_as(i64p), ctypes.byref(n), ctypes.byref(m)))
        return off, slot[:m.value], idx[:m.value]

    def poses_wc(self):
        """list over segments of (steps+1, 4, 4) world-in-camera poses: the table refine_map uses
        (the float32 rigid inverse of poses())."""
        n = int((self.steps + 1).sum())
        out = np.zeros(16 * n, np.float32)
        _check(lib().picp_vo_get_poses_wc(self._h, _fptr(out)))
        return self._split(np.transpose(out.reshape(n, 4, 4), (0, 2, 1)).copy())

    def refine_map(self, **params):
        """Refine every segment's map against its tracks with the poses fixed (PointRefiner's kernel
        and parameters); read the result with refined_map.  The map itself is not changed."""
        prm = default_refine_params(**params)
        _check(lib().picp_vo_refine_map(self._h, ctypes.byref(prm)))

    def refined_map(self, seg):
        """(xyz (n, 3), stats) of segment seg after refine_map; stats as PointRefiner.stats()."""
        n = ctypes.c_int64()
        _check(lib().picp_vo_get_refined_map(self._h, seg, 0, None, None, ctypes.byref(n)))
        xyz = np.zeros((max(n.value, 1), 3), np.float32)
        st = (Stats * max(n.value, 1))()
        _check(lib().picp_vo_get_refined_map(self._h, seg, n.value, _fptr(xyz), st, ctypes.byref(n)))
        rec = np.frombuffer(st, dtype=np.dtype([(k, np.float32 if t is ctypes.c_float else np.int32)
                                                for k, t in Stats._fields_]), count=n.value)
        return xyz[:n.value], {k: rec[k].copy() for k, _ in Stats._fields_ if k != "reserved"}

    def refine_time(self, reps, **params):
        """Mean device time in us of (the CSR build, the refine launch) over reps repetitions."""
        prm = default_refine_params(**params)
        b, r = ctypes.c_float(0), ctypes.c_float(0)
        _check(lib().picp_vo_refine_time(self._h, ctypes.byref(prm), reps, ctypes.byref(b), ctypes.byref(r)))
        return b.value, r.value

    def adjust(self, sweeps=None, points=None, poses=None):
        """Alternating adjustment of every segment's poses and map on the run's tracks, slot 0 of
        every segment fixed (PointRefiner.adjust's arguments); read the result with
        adjusted_poses_wc and adjusted_map.  The run's own poses and map are not changed."""
        prm = default_adjust_params(sweeps=sweeps, points=points, poses=poses)
        _check(lib().picp_vo_adjust(self._h, ctypes.byref(prm)))

    def adjusted_poses_wc(self):
        """list over segments of (steps+1, 4, 4) world-in-camera poses after adjust (poses_wc's layout)."""
        n = int((self.steps + 1).sum())
        out = np.zeros(16 * n, np.float32)
        _check(lib().picp_vo_get_adjusted_poses_wc(self._h, _fptr(out)))
        return self._split(np.transpose(out.reshape(n, 4, 4), (0, 2, 1)).copy())

    def adjusted_map(self, seg):
        """(xyz (n, 3), stats) of segment seg after adjust; stats as PointRefiner.stats()."""
        n = ctypes.c_int64()
        _check(lib().picp_vo_get_adjusted_map(self._h, seg, 0, None, None, ctypes.byref(n)))
        xyz = np.zeros((max(n.value, 1), 3), np.float32)
        st = (Stats * max(n.value, 1))()
        _check(lib().picp_vo_get_adjusted_map(self._h, seg, n.value, _fptr(xyz), st, ctypes.byref(n)))
        return xyz[:n.value], _stats_arrays(st, n.value)

    def align_segments(self, **params):
        """picp_vo_align_segments: consecutive segments aligned through their shared landmarks
        (segment s + 1's map matched against segment s's on the device, then the Sim(3) RANSAC with
        `params`: Sim3Params' fields).  Returns one dict per s < n_seg - 1: S (4x4, maps segment
        s + 1's frame into segment s's), scale, inliers, found, n_pairs.  Reads the run only."""
        prm = default_sim3_params(**params)
        P = max(len(self.steps) - 1, 0) if self.steps is not None else 0
        S = np.zeros(16 * max(P, 1), np.float32)
        scale = np.zeros(max(P, 1), np.float32)
        inl = np.zeros(max(P, 1), np.int32)
        found = np.zeros(max(P, 1), np.int32)
        npairs = np.zeros(max(P, 1), np.int64)
        _check(lib().picp_vo_align_segments(self._h, ctypes.byref(prm), _fptr(S), _fptr(scale), _i32ptr(inl),
                                            _i32ptr(found), npairs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return [{"S": pose_from_c(S[16 * s:16 * s + 16]), "scale": float(scale[s]), "inliers": int(inl[s]),
                 "found": bool(found[s]), "n_pairs": int(npairs[s])} for s in range(P)]

    def map(self, seg):
        n = ctypes.c_int64()
        _check(lib().picp_vo_get_map(self._h, seg, 0, None, None, ctypes.byref(n)))
        xyz = np.zeros(max(n.value, 1) * 3, np.float32)
        desc = np.zeros(max(n.value, 1) * self.dim, np.float32)
        _check(lib().picp_vo_get_map(self._h, seg, n.value, _fptr(xyz), _fptr(desc), ctypes.byref(n)))
        return xyz[:3 * n.value].reshape(-1, 3), desc[:self.dim * n.value].reshape(-1, self.dim)


def default_refine_params(**kw):
    """picp_refine_params (the same layout as picp_params): threshold 3000, damping 1, min_inliers 2,
    keep_outliers 0, max_rounds 10, conv_eps 1e-5."""
    p = Params()
    lib().picp_refine_params_default(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _stats_arrays(st, n):
    """A ctypes array of Stats -> dict of per-item numpy arrays."""
    rec = np.frombuffer(st, dtype=np.dtype([(k, np.float32 if t is ctypes.c_float else np.int32)
                                            for k, t in Stats._fields_]), count=n)
    return {k: rec[k].copy() for k, _ in Stats._fields_ if k != "reserved"}


def default_adjust_params(sweeps=None, points=None, poses=None):
    """picp_adjust_params: points (picp_refine_params fields) and poses (picp_params fields) are
    dicts of overrides of the defaults (the refiner's; the solver's with threshold 3000); sweeps 3."""
    p = AdjustParams()
    lib().picp_adjust_params_default(ctypes.byref(p))
    for k, v in (points or {}).items():
        setattr(p.points, k, v)
    for k, v in (poses or {}).items():
        setattr(p.poses, k, v)
    if sweeps is not None:
        p.sweeps = sweeps
    return p


def adjust_rank_tile():
    """Entries the view build's rank kernel stages per LDS tile (tests pick list lengths around it)."""
    fn = lib().picp_adjust_rank_tile
    fn.restype = ctypes.c_int
    return fn()


class PointRefiner:
    """picp_refine_t: refine map points against all of their observations with the poses held
    fixed (structure-only Gauss-Newton, csrc/picp_refine.hip).  Poses, tracks and points stay on
    the device between calls."""

    def __init__(self, device=0, rows=480, cols=640, K=K_REF):
        self._h = ctypes.c_void_p()
        self.device = device
        self.n_points = None
        self.n_poses = None
        _check(lib().picp_refine_create(ctypes.byref(self._h), device, rows, cols, _fptr(k_to_c(K))))

    def close(self):
        if self._h:
            lib().picp_refine_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_poses(self, Ts):
        """(n, 4, 4) world-in-camera poses."""
        Ts = np.asarray(Ts, np.float32).reshape(-1, 4, 4)
        flat = np.ascontiguousarray(np.transpose(Ts, (0, 2, 1)).reshape(-1))
        _check(lib().picp_refine_set_poses(self._h, _fptr(flat) if flat.size else None, Ts.shape[0]))
        self.n_poses = Ts.shape[0]

    def set_tracks(self, track_off, obs_pose, obs_uv):
        """CSR tracks: point i owns observations [track_off[i], track_off[i+1]) of obs_pose (pose
        indices) and obs_uv ((n_obs, 2) pixels)."""
        off = np.ascontiguousarray(track_off, np.int64)
        op = np.ascontiguousarray(obs_pose, np.int32).reshape(-1)
        uv = _f32(obs_uv, (-1,))
        assert off.size >= 1 and uv.size == 2 * op.size
        _check(lib().picp_refine_set_tracks(self._h, off.size - 1, off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                            _i32ptr(op) if op.size else None, _fptr(uv) if uv.size else None))
        self.n_points = off.size - 1

    def set_points(self, xyz):
        xyz = _f32(xyz, (-1,))
        assert self.n_points is None or xyz.size == 3 * self.n_points
        _check(lib().picp_refine_set_points(self._h, _fptr(xyz) if xyz.size else None))

    def points(self):
        n = self.n_points or 0
        out = np.zeros((n, 3), np.float32)
        _check(lib().picp_refine_get_points(self._h, _fptr(out) if n else None))
        return out

    def stats(self):
        """dict of per-point arrays: chi_in, chi_out, n_in, ok, rounds, converged, n_projected."""
        n = self.n_points or 0
        st = (Stats * max(n, 1))()
        _check(lib().picp_refine_get_stats(self._h, st))
        rec = np.frombuffer(st, dtype=np.dtype([(k, np.float32 if t is ctypes.c_float else np.int32)
                                                for k, t in Stats._fields_]), count=n)
        return {k: rec[k].copy() for k, _ in Stats._fields_ if k != "reserved"}

    def run(self, **params):
        """Refine the current points in place -> (xyz (n, 3), stats)."""
        prm = default_refine_params(**params)
        _check(lib().picp_refine_run(self._h, ctypes.byref(prm)))
        return self.points(), self.stats()

    def time(self, reps, **params):
        """Mean device time (us) of one run; the points are restored before every repetition."""
        prm = default_refine_params(**params)
        us = ctypes.c_float(0)
        _check(lib().picp_refine_time(self._h, ctypes.byref(prm), reps, ctypes.byref(us)))
        return us.value

    # --- alternating adjustment (picp_refine_run_poses, picp_refine_adjust) ---------------------
    def set_fixed_poses(self, fixed):
        """(n_poses,) flags: a fixed pose never moves.  None: no pose is fixed."""
        if fixed is None:
            _check(lib().picp_refine_set_fixed_poses(self._h, None))
            return
        m = np.ascontiguousarray(np.asarray(fixed) != 0, np.uint8)
        assert self.n_poses is None or m.size == self.n_poses
        _check(lib().picp_refine_set_fixed_poses(self._h, m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))

    def poses(self):
        """(n_poses, 4, 4) current world-in-camera poses."""
        n = self.n_poses or 0
        out = np.zeros(16 * n, np.float32)
        _check(lib().picp_refine_get_poses(self._h, _fptr(out) if n else None))
        return np.transpose(out.reshape(n, 4, 4), (0, 2, 1)).copy()

    def pose_stats(self):
        """dict of per-pose arrays of the last pose step (all zero for fixed and unobserved poses)."""
        n = self.n_poses or 0
        st = (Stats * max(n, 1))()
        _check(lib().picp_refine_get_pose_stats(self._h, st))
        return _stats_arrays(st, n)

    def pose_view(self):
        """The pose-major view of the tracks: (pose_off (n_poses+1,), obs_point, obs_uv (n_obs, 2));
        pose k owns entries [pose_off[k], pose_off[k+1]) in ascending position of the point-major arrays."""
        n = self.n_poses or 0
        off = np.zeros(n + 1, np.int64)
        i64p = ctypes.POINTER(ctypes.c_int64)
        _check(lib().picp_refine_get_pose_view(self._h, off.ctypes.data_as(i64p), None, None))
        m = int(off[-1])
        pt = np.zeros(max(m, 1), np.int32)
        uv = np.zeros((max(m, 1), 2), np.float32)
        _check(lib().picp_refine_get_pose_view(self._h, off.ctypes.data_as(i64p), _i32ptr(pt), _fptr(uv)))
        return off, pt[:m], uv[:m]

    def run_poses(self, **params):
        """One pose step (picp_batch_solve's parameters) -> (poses (n, 4, 4), pose stats)."""
        prm = default_params(**params)
        _check(lib().picp_refine_run_poses(self._h, ctypes.byref(prm)))
        return self.poses(), self.pose_stats()

    def adjust(self, sweeps=None, points=None, poses=None):
        """sweeps x (point step, pose step); points / poses: dicts of parameter overrides."""
        prm = default_adjust_params(sweeps=sweeps, points=points, poses=poses)
        _check(lib().picp_refine_adjust(self._h, ctypes.byref(prm)))

    def sweeps(self):
        """list of dicts, one per sweep of the last adjust: the sums of the steps' stats."""
        n = ctypes.c_int(0)
        _check(lib().picp_refine_get_sweeps(self._h, None, 0, ctypes.byref(n)))
        out = (AdjustSweep * max(n.value, 1))()
        _check(lib().picp_refine_get_sweeps(self._h, out, n.value, ctypes.byref(n)))
        return [out[k].as_dict() for k in range(n.value)]

    def adjust_time(self, reps, sweeps=None, points=None, poses=None):
        """Mean device times in us: (view build, and per sweep: gather + write-back, pose solve, point step)."""
        prm = default_adjust_params(sweeps=sweeps, points=points, poses=poses)
        t = [ctypes.c_float(0) for _ in range(4)]
        _check(lib().picp_refine_adjust_time(self._h, ctypes.byref(prm), reps, *[ctypes.byref(x) for x in t]))
        return tuple(x.value for x in t)


def refine_points(K, rows, cols, poses, track_off, obs_pose, obs_uv, xyz, device=0, **params):
    """One-shot PointRefiner: -> (refined xyz (n, 3), stats)."""
    r = PointRefiner(device=device, rows=rows, cols=cols, K=K)
    try:
        r.set_poses(poses)
        r.set_tracks(track_off, obs_pose, obs_uv)
        r.set_points(xyz)
        return r.run(**params)
    finally:
        r.close()


def selftest_rcp(e_lo=-8, e_hi=8, device=0):
    """Floats (both signs, exponents [e_lo, e_hi)) where the kernels' fast reciprocal differs
    from the IEEE division; 0 proves it for every |x| in [2^-100, 2^100] (picp_recip.h)."""
    n = ctypes.c_uint64()
    _check(lib().picp_selftest_rcp(device, e_lo, e_hi, ctypes.byref(n)))
    return n.value


SELFTEST_FINISH_IN, SELFTEST_FINISH_OUT = 52, 20  # include/picp_c.h


def selftest_finish(cases, device=0):
    """Runs the uniform and the lane-parallel finish of a round on every case (uint32 words,
    shape (n, SELFTEST_FINISH_IN): include/picp_c.h picp_selftest_finish).  Returns (the count of
    output words that differ between the two, the lane-parallel form's outputs and the uniform
    form's, each uint32 (n, SELFTEST_FINISH_OUT))."""
    cases = np.ascontiguousarray(cases, np.uint32)
    if cases.ndim != 2 or cases.shape[1] != SELFTEST_FINISH_IN:
        raise ValueError("cases must be (n, %d) uint32 words" % SELFTEST_FINISH_IN)
    out = np.zeros((cases.shape[0], 2, SELFTEST_FINISH_OUT), np.uint32)
    n = ctypes.c_uint64()
    _check(lib().picp_selftest_finish(device, cases.shape[0], cases.ctypes.data, ctypes.byref(n), out.ctypes.data))
    return n.value, out[:, 0].copy(), out[:, 1].copy()
