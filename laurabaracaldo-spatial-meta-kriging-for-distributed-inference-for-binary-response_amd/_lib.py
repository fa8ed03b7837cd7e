"""ctypes binding of include/mk.h (libmk.so, built in-tree for gfx950).

There is no fallback: if libmk.so is missing or cannot be loaded the import of
any compute entry point raises MkError.  Structures mirror include/mk.h field
for field.
"""
import ctypes
import os

import numpy as np

from ._build import LIB_PATH

MK_OK = 0
MK_E_ARG = -1
MK_E_HIP = -2
MK_E_NOMEM = -3
MK_E_NODEV = -4
MK_E_INTERRUPT = -5
MK_COMBINE_MEAN = 0
MK_COMBINE_MEDIAN = 1
MK_COV_EXPONENTIAL = 0
MK_COV_MATERN = 1
MK_LINK_LOGIT = 0
MK_LINK_PROBIT = 1
N_LEVELS = 200
N_DIAG = 3             # MK_N_DIAG: rows ess, mcse, rhat
N_CRIT = 8             # MK_N_CRIT: the rows of mk_criteria, in CRIT_NAMES' order
CRIT_NAMES = ["bar.D", "D.bar.Omega", "pD", "DIC", "lppd", "p.waic", "WAIC", "lconst"]
N_LOO = 8              # MK_N_LOO: the rows of mk_loo, in LOO_NAMES' order
LOO_NAMES = ["elpd_loo", "p_loo", "looic", "se_elpd_loo", "lppd", "k_max", "n_k_bad", "lconst"]
LOO_MIN_STATES, LOO_MAX_STATES = 25, 8192      # MK_LOO_MIN_STATES, MK_LOO_MAX_STATES
N_SCORE = 5            # MK_N_SCORE: the rows of mk_scores, in SCORE_NAMES' order
SCORE_NAMES = ["n", "lpd", "brier", "err", "lconst"]
MAP_MAXT = 8           # MK_MAP_MAXT: exceedance thresholds at most
N_MAP_BASE = 4         # MK_N_MAP_BASE: the planes before the exceedances, in MAP_BASE_NAMES' order
MAP_BASE_NAMES = ["w_mean", "w_sd", "p_mean", "p_sd"]
N_PAIR_BASE = 6        # MK_N_PAIR_BASE: the pair planes before joint_1..J, in PAIR_BASE_NAMES' order
PAIR_BASE_NAMES = ["both_mean", "both_sd", "diff_mean", "diff_sd", "corr", "a_gt_b"]
REGION_MAXM = 128      # MK_REGION_MAXM: sites per region at most
REGION_BASE_NAMES = ["mean", "sd"]     # the region planes before exc_1..J
REGIONS_EXACT, REGIONS_INTERP = 0, 1    # MK_REGIONS_EXACT, MK_REGIONS_INTERP: the routes of the areal prediction
REGION_ROUTE_NAMES = ["exact", "interpolated"]
VG_MAXBINS = 64        # MK_VG_MAXBINS: variogram bins at most
VG_MAXQ = 4            # MK_VG_MAXQ: outcomes of a variogram at most
CKPT_NFIELDS = 24      # MK_CKPT_NFIELDS: the fields of mk_checkpoint, in CKPT_FIELDS' order
CKPT_FIELDS = ["beta", "theta", "w", "eta", "tune", "acc", "u", "z", "Z", "logdetR", "quad", "A_full", "Ainv", "notpd",
               "crit_acc", "crit_part", "crit_sbeta", "samples", "w_samples", "acc_hist", "kz", "kth", "kA", "w_pred"]
CKPT_NDIGEST = 4       # MK_CKPT_NDIGEST: the digests per (subset, outcome) pair, in DIGEST_NAMES' order
DIGEST_NAMES = ["L", "Winv", "W", "QB"]

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)


class MkError(RuntimeError):
    """Raised for every non-zero libmk status (R glue: Rf_error)."""

    def __init__(self, code, msg):
        super().__init__(f"libmk error {code}: {msg}")
        self.code = code


class Problem(ctypes.Structure):
    _fields_ = [("n_subsets", ctypes.c_int32), ("subset_base", ctypes.c_int32), ("q", ctypes.c_int32),
                ("p", ctypes.c_int32), ("n_part", _ip), ("coords", _dp), ("y", _dp), ("weights", _dp),
                ("x", _dp), ("n_test", ctypes.c_int32), ("coords_test", _dp), ("x_test", _dp)]


class Config(ctypes.Structure):
    _fields_ = [("cov_model", ctypes.c_int32), ("n_batch", ctypes.c_int32), ("batch_length", ctypes.c_int32),
                ("accept_rate", ctypes.c_double), ("burn_in", ctypes.c_int32),
                ("beta_starting", _dp), ("beta_tuning", _dp), ("phi_starting", _dp), ("phi_tuning", _dp),
                ("A_starting", _dp), ("A_tuning", _dp), ("nu_starting", _dp), ("nu_tuning", _dp),
                ("w_starting", ctypes.c_double), ("w_tuning", ctypes.c_double),
                ("phi_unif_a", _dp), ("phi_unif_b", _dp), ("nu_unif_a", _dp), ("nu_unif_b", _dp),
                ("K_IW_df", ctypes.c_double), ("K_IW_S", _dp), ("seed", ctypes.c_uint64),
                ("record_samples", ctypes.c_int32), ("record_w", ctypes.c_int32), ("device", ctypes.c_int32),
                ("n_streams", ctypes.c_int32), ("predict_tile", ctypes.c_int32), ("link", ctypes.c_int32)]


class Outputs(ctypes.Structure):
    _fields_ = [("parameters", _dp), ("w_predict", _dp), ("samples", _dp), ("w_samples", _dp),
                ("w_pred_samples", _dp), ("acceptance", _dp), ("w_predict_sum", _dp), ("p_predict", _dp),
                ("p_pred_samples", _dp), ("p_predict_sum", _dp)]


class Summary(ctypes.Structure):
    _fields_ = [("sample_par", _dp), ("sample_w", _dp), ("p_sample", _dp), ("w_quant", _dp),
                ("param_quant", _dp), ("p_quant", _dp), ("index", _ip)]


class Combined(ctypes.Structure):
    _fields_ = [("result", _dp), ("result2", _dp), ("method", ctypes.c_int32), ("max_iter", ctypes.c_int32),
                ("tol", ctypes.c_double), ("exchange", ctypes.c_int32), ("comm_ranks", ctypes.c_int32), ("result3", _dp)]


class Diagnostics(ctypes.Structure):
    _fields_ = [("parameters", _dp), ("w_predict", _dp), ("p_predict", _dp), ("parameters_worst", _dp),
                ("w_predict_worst", _dp), ("p_predict_worst", _dp)]


class Criteria(ctypes.Structure):
    _fields_ = [("subsets", _dp), ("total", _dp), ("pointwise", _dp)]


class Loo(ctypes.Structure):
    _fields_ = [("subsets", _dp), ("total", _dp), ("pointwise", _dp)]


class Validation(ctypes.Structure):
    _fields_ = [("y_test", _dp), ("wt_test", _dp)]


class Scores(ctypes.Structure):
    _fields_ = [("subsets", _dp), ("pointwise", _dp), ("combined", _dp), ("combined_pointwise", _dp)]


class MapSpec(ctypes.Structure):
    _fields_ = [("thresholds", _dp), ("n_thresholds", ctypes.c_int32)]


class Maps(ctypes.Structure):
    _fields_ = [("subsets", _dp), ("combined", _dp)]


class PairSpec(ctypes.Structure):
    _fields_ = [("n_thresholds", ctypes.c_int32), ("thresholds", _dp)]


class Pairs(ctypes.Structure):
    _fields_ = [("both_predict", _dp), ("diff_predict", _dp), ("planes", _dp), ("combined_both", _dp),
                ("combined_diff", _dp)]


class RegionSpec(ctypes.Structure):
    _fields_ = [("n_regions", ctypes.c_int32), ("offsets", _ip), ("weights", _dp), ("n_thresholds", ctypes.c_int32),
                ("thresholds", _dp)]


class Regions(ctypes.Structure):
    _fields_ = [("region_predict", _dp), ("planes", _dp), ("region_samples", _dp), ("singular", _ip), ("timing_ms", _dp)]


class Variogram(ctypes.Structure):
    _fields_ = [("count", ctypes.POINTER(ctypes.c_int64)), ("dist", _dp), ("gamma", _dp), ("ms", ctypes.c_double)]


class Chain(ctypes.Structure):
    _fields_ = [("samples", _dp), ("w_samples", _dp), ("n_w", ctypes.c_int32), ("acceptance", _dp)]


class Checkpoint(ctypes.Structure):
    _fields_ = [("field", ctypes.c_void_p * CKPT_NFIELDS), ("digests", ctypes.POINTER(ctypes.c_uint64)),
                ("lookahead", ctypes.c_int32)]


# int (*mk_progress_fn)(void* user, int32_t iterations, int32_t n_samples)
PROGRESS_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32)

EXPORTS = {
    "mk_meta_fit_ex": (ctypes.c_int, [ctypes.POINTER(Problem), ctypes.POINTER(Config), _ip, ctypes.c_int32,
                                      PROGRESS_FN, ctypes.c_void_p, ctypes.POINTER(Outputs), ctypes.POINTER(Combined),
                                      ctypes.POINTER(Diagnostics), ctypes.POINTER(Criteria)]),
    "mk_meta_fit_val": (ctypes.c_int, [ctypes.POINTER(Problem), ctypes.POINTER(Config), _ip, ctypes.c_int32,
                                       PROGRESS_FN, ctypes.c_void_p, ctypes.POINTER(Outputs), ctypes.POINTER(Combined),
                                       ctypes.POINTER(Diagnostics), ctypes.POINTER(Criteria), ctypes.POINTER(Validation),
                                       ctypes.POINTER(Scores)]),
    "mk_meta_fit_maps": (ctypes.c_int, [ctypes.POINTER(Problem), ctypes.POINTER(Config), _ip, ctypes.c_int32,
                                        PROGRESS_FN, ctypes.c_void_p, ctypes.POINTER(Outputs), ctypes.POINTER(Combined),
                                        ctypes.POINTER(Diagnostics), ctypes.POINTER(Criteria), ctypes.POINTER(Validation),
                                        ctypes.POINTER(Scores), ctypes.POINTER(MapSpec), ctypes.POINTER(Maps)]),
    "mk_meta_fit_pairs": (ctypes.c_int, [ctypes.POINTER(Problem), ctypes.POINTER(Config), _ip, ctypes.c_int32,
                                         PROGRESS_FN, ctypes.c_void_p, ctypes.POINTER(Outputs), ctypes.POINTER(Combined),
                                         ctypes.POINTER(Diagnostics), ctypes.POINTER(Criteria), ctypes.POINTER(Validation),
                                         ctypes.POINTER(Scores), ctypes.POINTER(MapSpec), ctypes.POINTER(Maps),
                                         ctypes.POINTER(PairSpec), ctypes.POINTER(Pairs)]),
    "mk_session_set_pairs": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(PairSpec)]),
    "mk_session_pairs": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Pairs)]),
    "mk_session_set_regions": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RegionSpec)]),
    "mk_session_regions": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Regions)]),
    "mk_session_set_regions_route": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "mk_session_regions_route": (ctypes.c_int, [ctypes.c_void_p, _ip, _ip, _dp]),
    "mk_session_set_maps": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(MapSpec)]),
    "mk_session_maps": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Maps)]),
    "mk_map_grid": (ctypes.c_int, [_dp, ctypes.c_int32, ctypes.c_int64, _dp, ctypes.c_int32, _dp, ctypes.c_int32]),
    "mk_session_set_validation": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Validation)]),
    "mk_session_scores": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Scores)]),
    "mk_score_grid": (ctypes.c_int, [_dp, ctypes.c_int32, ctypes.c_int64, _dp, _dp, _dp, _dp, ctypes.c_int32]),
    "mk_session_set_criteria": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "mk_session_criteria": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(Criteria)]),
    "mk_session_loo": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(Loo)]),
    "mk_loo_matrix": (ctypes.c_int, [_dp, ctypes.c_int64, ctypes.c_int32, _dp, _dp, ctypes.c_int32]),
    "mk_meta_fit": (ctypes.c_int, [ctypes.POINTER(Problem), ctypes.POINTER(Config), _ip, ctypes.c_int32,
                                   PROGRESS_FN, ctypes.c_void_p, ctypes.POINTER(Outputs), ctypes.POINTER(Combined)]),
    "mk_meta_fit_diag": (ctypes.c_int, [ctypes.POINTER(Problem), ctypes.POINTER(Config), _ip, ctypes.c_int32,
                                        PROGRESS_FN, ctypes.c_void_p, ctypes.POINTER(Outputs), ctypes.POINTER(Combined),
                                        ctypes.POINTER(Diagnostics)]),
    "mk_session_diagnostics": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Diagnostics)]),
    "mk_session_set_diagnostics": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Diagnostics)]),
    "mk_chain_diagnostics": (ctypes.c_int, [_dp, ctypes.c_int32, ctypes.c_int64, _dp, ctypes.c_int32]),
    "mk_session_create": (ctypes.c_int, [ctypes.POINTER(Problem), ctypes.POINTER(Config), ctypes.POINTER(ctypes.c_void_p)]),
    "mk_session_run": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "mk_session_iteration": (ctypes.c_int32, [ctypes.c_void_p]),
    "mk_session_predict_tile": (ctypes.c_int32, [ctypes.c_void_p]),
    "mk_session_chain_state": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _dp, _dp, _dp, _dp, _dp]),
    "mk_session_notpd_counts": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]),
    "mk_session_set_lookahead": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "mk_session_lookahead": (ctypes.c_int32, [ctypes.c_void_p]),
    "mk_session_outputs": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Outputs)]),
    "mk_session_set_test_sites": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_double)]),
    "mk_session_set_test_covars": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]),
    "mk_session_tile_grids_wp": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_int32]),
    "mk_session_grids": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32]),
    "mk_session_tile_grids": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32]),
    "mk_session_set_kept_window": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]),
    "mk_session_profile": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "mk_session_profile_every": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "mk_session_kernel_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64),
                                               _dp, _dp]),
    "mk_session_import_chain": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Chain)]),
    "mk_session_imported": (ctypes.c_int32, [ctypes.c_void_p]),
    "mk_session_import_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), _dp, _dp]),
    "mk_session_checkpoint_layout": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)]),
    "mk_session_checkpoint": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(Checkpoint)]),
    "mk_session_restore": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64),
                                          ctypes.POINTER(Checkpoint)]),
    "mk_session_digest": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "mk_digest": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64)]),
    "mk_session_restore_stats": (ctypes.c_int, [ctypes.c_void_p, _dp, _dp, _dp]),
    "mk_session_destroy": (None, [ctypes.c_void_p]),
    "mk_session_count": (ctypes.c_int32, []),
    "mk_fit_predict_batched": (ctypes.c_int, [ctypes.POINTER(Problem), ctypes.POINTER(Config), ctypes.POINTER(Outputs)]),
    "mk_combine": (ctypes.c_int, [_dp, ctypes.c_int32, ctypes.c_int64, _dp, ctypes.c_int32]),
    "mk_combine_sum": (ctypes.c_int, [_dp, ctypes.c_int32, ctypes.c_int64, _dp, ctypes.c_int32]),
    "mk_combine_median_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                                ctypes.c_int32, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_int32, ctypes.c_void_p]),
    "mk_combine_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p,
                                         ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]),
    "mk_combine_median": (ctypes.c_int, [_dp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                         ctypes.c_double, _dp, _ip, ctypes.c_int32]),
    "mk_posterior_summary": (ctypes.c_int, [_dp, ctypes.c_int32, _dp, ctypes.c_int64, _dp, ctypes.c_int32,
                                            ctypes.c_int32, ctypes.c_uint64, ctypes.POINTER(Summary),
                                            ctypes.c_int32]),
    "mk_posterior_summary_ex": (ctypes.c_int, [_dp, ctypes.c_int32, _dp, ctypes.c_int64, _dp, ctypes.c_int32,
                                               ctypes.c_int32, ctypes.c_uint64, _ip, ctypes.c_int32,
                                               ctypes.POINTER(Summary), ctypes.c_int32]),
    "mk_glm_binomial_link": (ctypes.c_int, [_dp, _dp, _dp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                            ctypes.c_double, ctypes.c_int32, _dp, _dp, _ip, ctypes.c_int32]),
    "mk_glm_binomial": (ctypes.c_int, [_dp, _dp, _dp, ctypes.c_int64, ctypes.c_int32, ctypes.c_double,
                                       ctypes.c_int32, _dp, _dp, _ip, ctypes.c_int32]),
    "mk_variogram_compute": (ctypes.c_int, [_dp, ctypes.c_int64, _dp, ctypes.c_int32, ctypes.c_int32, ctypes.c_double,
                                            ctypes.POINTER(Variogram), ctypes.c_int32]),
    "mk_variogram_tile_edge": (ctypes.c_int32, []),
    "mk_correlation_batched": (ctypes.c_int, [_dp, ctypes.c_int32, ctypes.c_int32, _dp, _dp, ctypes.c_int32, _dp,
                                              ctypes.c_int32]),
    "mk_correlation_cross_batched": (ctypes.c_int, [_dp, ctypes.c_int32, ctypes.c_int32, _dp, ctypes.c_int32, _dp, _dp,
                                                    ctypes.c_int32, ctypes.c_int32, _dp, _dp, ctypes.c_int32]),
    "mk_cholesky_batched": (ctypes.c_int, [_dp, ctypes.c_int32, ctypes.c_int32, _dp, _dp, _dp, ctypes.c_int32]),
    "mk_partition_r": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _ip, _ip]),
    "mk_r_sample": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _ip]),
    "mk_r_sample_replace": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _ip]),
    "mk_inv_map_jobs": (ctypes.c_int, [ctypes.c_int32] * 7 + [_ip, ctypes.c_int32]),
    "mk_set_hw_queues": (ctypes.c_int, [ctypes.c_int32]),
    "mk_hip_initialized": (ctypes.c_int, []),
    "mk_shutdown": (None, []),
    "mk_set_watchdog": (ctypes.c_int, [ctypes.c_int32]),
    "mk_last_error": (ctypes.c_char_p, []),
    "mk_device_count": (ctypes.c_int, []),
    "mk_device_memory": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
}

_LIB = None
HW_QUEUES = None     # hardware queues of this process's HIP runtime, as passed to mk_set_hw_queues


def _hip_started():
    """True when this process's HIP runtime is already initialised (torch first, or any other
    library): a GPU_MAX_HW_QUEUES set now would no longer be read.  The process then holds /dev/kfd
    open (mk_hip_initialized checks the same without starting HIP)."""
    try:
        for fd in os.listdir("/proc/self/fd"):
            try:
                if os.readlink("/proc/self/fd/" + fd) == "/dev/kfd":
                    return True
            except OSError:
                pass
    except OSError:
        pass
    return False


def load():
    """Load libmk.so (raises MkError if it is absent -- no CPU fallback exists)."""
    global _LIB, HW_QUEUES
    if _LIB is not None:
        return _LIB
    path = os.environ.get("MK_LIB") or LIB_PATH      # MK_LIB: a development build (tools/ probes)
    # the lookahead schedule runs up to five HIP streams: give the process 8 hardware queues when
    # HIP has not started yet (the variable is read once, when HIP initialises).  If it has started
    # (torch first), keep the count it started with and tell libmk, which then runs three streams
    # instead of five on too few queues.
    before = int(os.environ.get("GPU_MAX_HW_QUEUES", "0") or 0)
    if _hip_started():
        HW_QUEUES = before if before > 0 else 4
    else:
        if before < 8:
            os.environ["GPU_MAX_HW_QUEUES"] = "8"
        HW_QUEUES = max(before, 8)
    if not os.path.exists(path):
        raise MkError(MK_E_ARG, f"{path} not built; run __graft_entry__.build()")
    lib = ctypes.CDLL(path)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    lib.mk_set_hw_queues(HW_QUEUES)
    # libmk's pooled streams (CU-masked / priority queues) are destroyed while the HIP runtime is
    # alive: Python's atexit runs before the C library's exit handlers (libmk registers mk_shutdown
    # there too; it is idempotent)
    import atexit
    atexit.register(lib.mk_shutdown)
    _LIB = lib
    return lib


def check(rc):
    if rc != MK_OK:
        raise MkError(rc, load().mk_last_error().decode())


def dptr(a):
    """Pointer to a C-contiguous float64 array (or NULL for None)."""
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(_dp)


def iptr(a):
    assert a.dtype == np.int32 and a.flags.c_contiguous
    return a.ctypes.data_as(_ip)
