"""ctypes binding of libptm_engine.so (C ABI: include/ptm_engine.h).

Thin by design: numpy arrays in, numpy arrays out; every call goes straight through the C ABI
into the HIP engine.  There is no CPU fallback -- without the built library or without an
MI355X the constructor raises.
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PTM_ENGINE_LIB") or os.path.join(_HERE, "libptm_engine.so")   # override: A/B builds

# enums of include/ptm_engine.h
BOUND_OPEN, BOUND_LIMIT, BOUND_REFLECT, BOUND_WRAP = 0, 1, 2, 3
PRIOR_FLAT, PRIOR_UNIFORM, PRIOR_GAUSSIAN, PRIOR_POLAR, PRIOR_COPOLAR, PRIOR_LOG = 0, 1, 2, 3, 4, 5
PROP_DENSE, PROP_DIAG, PROP_LOWER = 0, 1, 2
ARR_LLIKE, ARR_LPRIOR, ARR_LPOST, ARR_NTRIES, ARR_NACCEPT, ARR_LAST_TYPE, ARR_NHIST, ARR_NSIZE, ARR_ROW_LABELS = range(9)
FN_LOG, FN_EXP, FN_SIN_0_PI, FN_COS_HPI, FN_SQRT, FN_DIV, FN_SQRT_RAW = range(7)
COUNT_MAX = 2**31 - 1   # PTM_COUNT_MAX: the largest Ntries / Naccept / Nhist the engine represents (include/ptm_engine.h, "The horizon")
PRIOR_NAMES = {"uni": 1, "uniform": 1, "gauss": 2, "gaussian": 2, "pol": 3, "polar": 3, "cpol": 4, "copol": 4, "log": 5}

EXPORTS = [
    "ptm_last_error", "ptm_abi_version", "ptm_device_count", "ptm_engine_create", "ptm_engine_destroy",
    "ptm_set_bounds", "ptm_set_prior", "ptm_set_target_gaussian", "ptm_set_target_callback", "ptm_set_prior_callback", "ptm_set_ladder", "ptm_set_evolve_temps", "ptm_get_invtemps", "ptm_set_invtemps",
    "ptm_set_proposals", "ptm_set_proposal_rung", "ptm_set_proposal_mixture", "ptm_set_proposal_callback", "ptm_set_proposal_de", "ptm_set_proposal_prior_draw", "ptm_set_states", "ptm_init_from_prior", "ptm_init_from_prior_k", "ptm_draw_prior_rows", "ptm_get_history_chains", "ptm_sweep", "ptm_step", "ptm_sync",
    "ptm_copy_llike", "ptm_copy_lprior", "ptm_llike_device_ptr", "ptm_exchange_decide", "ptm_exchange_decide_gathered", "ptm_set_shard_map", "ptm_exchange_redo_count", "ptm_exchange_redo", "ptm_exchange_finish_and_sweep", "ptm_exchange_install", "ptm_sweep_rungs", "ptm_exchange_buffer_doubles", "ptm_exchange_row_capacity", "ptm_shard_unique_id", "ptm_shard_init", "ptm_shard_step", "ptm_shard_finalize", "ptm_get_states", "ptm_batch_begin", "ptm_batch_end",
    "ptm_get_array", "ptm_get_swap_counts", "ptm_get_last_swaps", "ptm_max_swaps_per_step", "ptm_get_history", "ptm_get_history_invtemps", "ptm_set_history", "ptm_set_map", "ptm_get_map", "ptm_restore", "ptm_step_count",
    "ptm_timer_start", "ptm_timer_stop", "ptm_get_kernel_times", "ptm_calibrate", "ptm_get_counter_sums", "ptm_get_ladder_stats", "ptm_sweep_kernel_name", "ptm_step_kernel_name", "ptm_debug_eval",
    "ptm_debug_philox", "ptm_debug_boxmuller", "ptm_debug_sqrt_scan", "ptm_debug_boxmuller_f32_scan", "ptm_debug_evaluate",
    "ptm_dev_alloc", "ptm_dev_free", "ptm_dev_copy",
    "ptm_set_target_device", "ptm_target_device_rows", "ptm_get_best_evaluated",
    "ptm_set_proposal_adaptive", "ptm_get_proposal_adapt_state", "ptm_set_proposal_adapt_state",
    "ptm_ess_windowed", "ptm_ess_report", "ptm_ess_series_windowed", "ptm_ess_series_report", "ptm_ess_last_on_device",
    "ptm_log_evidence",
    "ptm_rhat", "ptm_rhat_series",
    "ptm_moments", "ptm_moments_series", "ptm_moments_tile_rows",
    "ptm_moments_rungs", "ptm_eigen_factors", "ptm_adapt_proposals",
    "ptm_quantiles", "ptm_quantiles_series", "ptm_quantiles_last_path",
    "ptm_histograms", "ptm_histograms_series", "ptm_histograms_last_launch",
    "ptm_get_prefilter_counts",
    "ptm_set_proposal_device",
    "ptm_nn_dist2", "ptm_nn_dist2_tile",
    "ptm_set_prior_device",
]


class PtmConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("dim", C.c_int32), ("n_rungs", C.c_int32), ("rung_begin", C.c_int32),
                ("rung_count", C.c_int32), ("n_walkers", C.c_int32), ("seed", C.c_uint64), ("swap_rate", C.c_double),
                ("add_every_n", C.c_int32), ("min_prior", C.c_double), ("device", C.c_int32), ("stream", C.c_void_p),
                ("time_kernels", C.c_int32), ("swap_log_steps", C.c_int32), ("exchange_row_capacity", C.c_int32), ("history_rungs", C.c_int32),
                ("history_capacity", C.c_int32), ("map_rungs", C.c_int32), ("walker_begin", C.c_int32)]


class PtmCalibration(C.Structure):
    _fields_ = [("copy_GBs", C.c_double), ("copy_bytes", C.c_double), ("copy_ms", C.c_double), ("f64_fma_TFs", C.c_double),
                ("fma_ms", C.c_double), ("sclk_MHz", C.c_double), ("compute_units", C.c_int32), ("reserved", C.c_int32)]


class PtmDeParams(C.Structure):
    _fields_ = [("snooker", C.c_double), ("gamma_one_frac", C.c_double), ("reduce_gamma", C.c_double), ("ignore_frac", C.c_double)]


class PtmAdaptiveSet(C.Structure):
    _fields_ = [("K", C.c_int), ("nested", C.c_int), ("K_inner", C.c_int), ("rate", C.c_double), ("rate_inner", C.c_double)]


class PtmError(RuntimeError):
    pass


_lib = None
_dp = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_u32p = C.POINTER(C.c_uint32)

LOGLIKE_BATCH_FN = C.CFUNCTYPE(None, C.c_void_p, _dp, C.c_int, C.c_int, _dp)
# ptm_propose_batch_fn / ptm_proposal_result_fn (include/ptm_engine.h)
PROPOSE_BATCH_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, _dp, _i32p, _i32p, C.c_uint64, _dp, _dp, _i32p, _i32p)
PROPOSAL_RESULT_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, _i32p, _i32p, _i32p)
# ptm_loglike_device_fn (include/ptm_engine.h): user, stream, n_rows, dim, X_dev, count_dev, out_llike_dev (device pointers)
LOGLIKE_DEVICE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
# ptm_propose_device_fn: user, stream, n_rows, dim, X_cur_dev, rung_dev, walker_dev, count_dev, step, X_prop_dev, log_hastings_dev, type_dev, valid_dev
PROPOSE_DEVICE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
# ptm_proposal_result_device_fn: user, stream, n_rows, rung_dev, walker_dev, count_dev, accepted_dev
PROPOSAL_RESULT_DEVICE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


TORCH_LOADED_FIRST = None


def load():
    """dlopen the engine; raises if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PtmError("HIP engine not built: %s is missing (run `python -c 'import __graft_entry__ as g; g.build()'`)" % LIB_PATH)
    global TORCH_LOADED_FIRST
    TORCH_LOADED_FIRST = "torch" in sys.modules      # (see ptmcmc_amd.parallel.EngineShard: one HIP runtime per process)
    L = C.CDLL(LIB_PATH)
    L.ptm_last_error.restype = C.c_char_p
    L.ptm_sweep_kernel_name.restype = C.c_char_p
    L.ptm_sweep_kernel_name.argtypes = [C.c_void_p]
    if hasattr(L, "ptm_step_kernel_name"):
        L.ptm_step_kernel_name.restype = C.c_char_p
        L.ptm_step_kernel_name.argtypes = [C.c_void_p]
    L.ptm_step_count.restype = C.c_uint64
    L.ptm_step_count.argtypes = [C.c_void_p]
    L.ptm_engine_create.argtypes = [C.POINTER(PtmConfig), C.POINTER(C.c_void_p)]
    L.ptm_engine_destroy.argtypes = [C.c_void_p]
    L.ptm_set_bounds.argtypes = [C.c_void_p, _i32p, _i32p, _dp, _dp]
    L.ptm_set_prior.argtypes = [C.c_void_p, _i32p, _dp, _dp]
    L.ptm_set_target_gaussian.argtypes = [C.c_void_p, _dp, _dp, C.c_double]
    L.ptm_set_target_callback.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "ptm_set_prior_callback"):   # (absent from older builds handed over through PTM_ENGINE_LIB for A/B timing)
        L.ptm_set_prior_callback.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ptm_set_ladder.argtypes = [C.c_void_p, _dp]
    L.ptm_set_evolve_temps.argtypes = [C.c_void_p, C.c_double, C.c_double]
    L.ptm_get_invtemps.argtypes = [C.c_void_p, _dp]
    L.ptm_set_invtemps.argtypes = [C.c_void_p, _dp]
    L.ptm_set_proposals.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    L.ptm_set_states.argtypes = [C.c_void_p, _dp, _dp]
    L.ptm_init_from_prior.argtypes = [C.c_void_p]
    L.ptm_init_from_prior_k.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "ptm_draw_prior_rows"):
        L.ptm_draw_prior_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp]
    L.ptm_sweep.argtypes = [C.c_void_p, C.c_int]
    L.ptm_step.argtypes = [C.c_void_p, C.c_int]
    L.ptm_sync.argtypes = [C.c_void_p]
    L.ptm_llike_device_ptr.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.ptm_exchange_decide.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.ptm_copy_llike.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    if hasattr(L, "ptm_copy_lprior"):
        L.ptm_copy_lprior.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.ptm_exchange_decide_gathered.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "ptm_set_shard_map"):
        L.ptm_set_shard_map.argtypes = [C.c_void_p, C.c_int, _i32p, C.c_int]
        L.ptm_exchange_redo_count.argtypes = [C.c_void_p, _i32p]
        L.ptm_exchange_redo.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ptm_dev_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    L.ptm_dev_free.argtypes = [C.c_void_p]
    L.ptm_dev_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.ptm_exchange_finish_and_sweep.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ptm_exchange_install.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ptm_sweep_rungs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.ptm_get_states.argtypes = [C.c_void_p, _dp]
    if hasattr(L, "ptm_batch_begin"):
        L.ptm_batch_begin.argtypes = [C.c_void_p]
        L.ptm_batch_end.argtypes = [C.c_void_p]
    L.ptm_get_array.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.ptm_get_swap_counts.argtypes = [C.c_void_p, _i64p, _i64p]
    L.ptm_get_last_swaps.argtypes = [C.c_void_p, _i32p, _i32p]
    L.ptm_max_swaps_per_step.argtypes = [C.c_void_p]
    L.ptm_timer_start.argtypes = [C.c_void_p]
    L.ptm_timer_stop.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.ptm_get_kernel_times.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]
    L.ptm_calibrate.argtypes = [C.c_void_p, C.POINTER(PtmCalibration)]
    L.ptm_get_counter_sums.argtypes = [C.c_void_p, _i64p, _i64p]
    if hasattr(L, "ptm_get_prefilter_counts"):   # (an older library, PTM_ENGINE_LIB in A/B runs, has no box pre-pass)
        L.ptm_get_prefilter_counts.argtypes = [C.c_void_p, _i64p]
    L.ptm_get_ladder_stats.argtypes = [C.c_void_p, _i64p]
    L.ptm_debug_eval.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, C.c_int]
    L.ptm_debug_philox.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_uint32, C.c_uint64, C.c_uint32, _u32p]
    L.ptm_debug_boxmuller.argtypes = [C.c_int, _u32p, _u32p, _dp, _dp, C.c_int]
    L.ptm_exchange_buffer_doubles.argtypes = [C.c_void_p]
    L.ptm_exchange_row_capacity.argtypes = [C.c_void_p]
    L.ptm_get_history.argtypes = [C.c_void_p, _dp, _dp, _dp, _i32p]
    L.ptm_get_history_invtemps.argtypes = [C.c_void_p, _dp]
    L.ptm_set_history.argtypes = [C.c_void_p, _dp, _dp, _dp, _i32p, _dp]
    L.ptm_set_map.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp]
    L.ptm_get_map.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp]
    L.ptm_set_proposal_rung.argtypes = [C.c_void_p, C.c_int, _dp, C.c_double]
    L.ptm_set_proposal_mixture.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
    L.ptm_set_proposal_de.argtypes = [C.c_void_p, C.POINTER(PtmDeParams), C.c_int, _dp]
    L.ptm_set_proposal_prior_draw.argtypes = [C.c_void_p, C.c_int]
    L.ptm_set_proposal_callback.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ptm_shard_unique_id.argtypes = [C.c_void_p]
    L.ptm_shard_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _i32p, C.c_int]
    L.ptm_shard_step.argtypes = [C.c_void_p, C.c_int]
    L.ptm_shard_finalize.argtypes = [C.c_void_p]
    L.ptm_restore.argtypes = [C.c_void_p, _dp, _dp, _i32p, _i32p, _i32p, C.POINTER(C.c_int64), C.c_uint64, C.POINTER(C.c_int64),
                              C.POINTER(C.c_int64)]
    L.ptm_debug_sqrt_scan.argtypes = [C.c_int, C.POINTER(C.c_uint64)]
    if hasattr(L, "ptm_debug_boxmuller_f32_scan"):   # (an older library, PTM_ENGINE_LIB in A/B runs, has no single-precision pre-pass)
        L.ptm_debug_boxmuller_f32_scan.argtypes = [C.c_int, C.POINTER(C.c_double)]
    L.ptm_debug_evaluate.argtypes = [C.c_void_p, _dp, C.c_int, _i32p, _dp, _dp, _dp]
    if hasattr(L, "ptm_set_target_device"):
        L.ptm_set_target_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ptm_target_device_rows.argtypes = [C.c_void_p]
        L.ptm_get_best_evaluated.argtypes = [C.c_void_p, _dp, _dp]
    if hasattr(L, "ptm_set_proposal_device"):   # (absent from older builds handed over through PTM_ENGINE_LIB for A/B timing)
        L.ptm_set_proposal_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "ptm_set_prior_device"):   # (absent from older builds handed over through PTM_ENGINE_LIB for A/B timing)
        L.ptm_set_prior_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "ptm_set_proposal_adaptive"):
        L.ptm_set_proposal_adaptive.argtypes = [C.c_void_p, C.POINTER(PtmAdaptiveSet), _dp, _dp, _dp, _dp, _i32p, _i32p]
        L.ptm_get_proposal_adapt_state.argtypes = [C.c_void_p, _dp, _dp, _i32p, _i32p]
        L.ptm_set_proposal_adapt_state.argtypes = [C.c_void_p, _dp, _dp, _i32p, _i32p]
    if hasattr(L, "ptm_ess_windowed"):
        L.ptm_ess_windowed.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _i32p]
        L.ptm_ess_report.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _dp, _i32p]
        L.ptm_ess_series_windowed.argtypes = [C.c_int, _dp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _i32p]
        L.ptm_ess_series_report.argtypes = [C.c_int, _dp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _dp, _i32p]
        L.ptm_ess_last_on_device.argtypes = [C.c_void_p]
    if hasattr(L, "ptm_log_evidence"):
        L.ptm_log_evidence.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _i32p]
    if hasattr(L, "ptm_rhat"):
        L.ptm_rhat.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]
        L.ptm_rhat_series.argtypes = [C.c_int, _dp, C.c_int64, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]
    if hasattr(L, "ptm_moments"):   # (absent from older builds handed over through PTM_ENGINE_LIB for A/B timing)
        L.ptm_moments.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _i64p]
        L.ptm_moments_series.argtypes = [C.c_int, _dp, C.c_int64, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _i64p]
        L.ptm_moments_tile_rows.argtypes = [C.c_int]
    if hasattr(L, "ptm_adapt_proposals"):   # (absent from older builds handed over through PTM_ENGINE_LIB for A/B timing)
        L.ptm_moments_rungs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _i64p]
        L.ptm_eigen_factors.argtypes = [C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _i32p]
        L.ptm_adapt_proposals.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, _i32p, _dp]
    if hasattr(L, "ptm_quantiles"):   # (absent from older builds handed over through PTM_ENGINE_LIB for A/B timing)
        L.ptm_quantiles.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _i64p]
        L.ptm_quantiles_series.argtypes = [C.c_int, _dp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _i64p]
        L.ptm_quantiles_last_path.argtypes = [_i32p, _i32p]
    if hasattr(L, "ptm_histograms"):   # (absent from older builds handed over through PTM_ENGINE_LIB for A/B timing)
        L.ptm_histograms.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _i64p, _i64p, _i64p, _i64p, _i64p]
        L.ptm_histograms_series.argtypes = [C.c_int, _dp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _i64p, _i64p, _i64p, _i64p, _i64p]
        L.ptm_histograms_last_launch.argtypes = [_i32p, _i32p, _i32p]
    if hasattr(L, "ptm_nn_dist2"):   # (absent from older builds handed over through PTM_ENGINE_LIB for A/B timing)
        L.ptm_nn_dist2.argtypes = [C.c_int, _dp, C.c_int64, _dp, C.c_int64, C.c_int, _i32p, _dp, _dp, C.c_int, _dp]
    _lib = L
    return L


def _wrap_device(torch, ptr, shape, typestr, dev):
    """a torch view of an engine-allocated device buffer (no copy), through the CUDA array interface"""
    class _Arr:
        __cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(_Arr(), device=dev)


def _wrap_int32_device(torch, ptr, dev):
    """a 1-element int32 torch tensor over a device pointer (the engine's count)"""
    return _wrap_device(torch, ptr, (1,), "<i4", dev)


def _chk(rc):
    if rc != 0:
        raise PtmError("ptm error %d: %s" % (rc, load().ptm_last_error().decode()))


def _d(a):
    return a.ctypes.data_as(_dp)


def device_count():
    return load().ptm_device_count()


def debug_eval(fn, a, b=None, device=-1):
    a = np.ascontiguousarray(a, dtype=np.float64)
    bb = a if b is None else np.ascontiguousarray(b, dtype=np.float64)
    out = np.empty_like(a)
    _chk(load().ptm_debug_eval(device, fn, _d(a), _d(bb), _d(out), a.size))
    return out


def debug_philox(seed, tag, stream, step, block, device=-1):
    o = (C.c_uint32 * 4)()
    _chk(load().ptm_debug_philox(device, seed, tag, stream, step, block, o))
    return [int(v) for v in o]


def debug_boxmuller(k1, k2, device=-1):
    k1 = np.ascontiguousarray(k1, dtype=np.uint32)
    k2 = np.ascontiguousarray(k2, dtype=np.uint32)
    z0, z1 = np.empty(k1.size), np.empty(k1.size)
    _chk(load().ptm_debug_boxmuller(device, k1.ctypes.data_as(_u32p), k2.ctypes.data_as(_u32p), _d(z0), _d(z1), k1.size))
    return z0, z1


def debug_sqrt_scan(device=-1):
    n = C.c_uint64()
    _chk(load().ptm_debug_sqrt_scan(device, C.byref(n)))
    return n.value


def debug_boxmuller_f32_scan(device=-1):
    """the box pre-pass's single-precision Box-Muller against the sweep's, over all 2^32 arguments of either half"""
    o = (C.c_double * 8)()
    _chk(load().ptm_debug_boxmuller_f32_scan(device, o))
    return dict(max_dr=o[0], max_r=o[1], radius_nan=int(o[2]), max_dtrig=o[3], trig_nan=int(o[4]), dz=o[5], f32_slack=o[6])


def _series3(series):
    a = np.ascontiguousarray(series, dtype=np.float64)
    if a.ndim != 3:
        raise ValueError("series must be an array [n, nseries, nfeat]")
    return a


def ess_series_windowed(series, width, every, burn, device=-1):
    """one pass of the effective-sample-size estimator with fixed windows over series [n, nseries, nfeat] (every feature of a
    series is looked at), on the device: (ess[nseries], nwin[nseries]) (ptm_ess_series_windowed)"""
    a = _series3(series)
    n, ns, nf = a.shape
    ess, nwin = np.empty(ns), np.empty(ns, dtype=np.int32)
    _chk(load().ptm_ess_series_windowed(device, _d(a), n, ns, nf, int(width), int(every), int(burn), _d(ess), nwin.ctypes.data_as(_i32p)))
    return ess, nwin


def effective_samples_series(series, width, every, esslimit=-1, device=-1):
    """chain::report_effective_samples for series [n, nseries, nfeat] on the device: (ess[nseries], useful length[nseries])
    (ptm_ess_series_report; esslimit >= 0: the coarse-to-fine stride search)"""
    a = _series3(series)
    n, ns, nf = a.shape
    ess, length = np.empty(ns), np.empty(ns, dtype=np.int32)
    _chk(load().ptm_ess_series_report(device, _d(a), n, ns, nf, int(width), int(every), float(esslimit), _d(ess), length.ctypes.data_as(_i32p)))
    return ess, length


def _rhat_outputs(m, nfeat, sequences, out):
    """(rhat, mean, within, between[, seq_mean, seq_var]) to fill: the caller's `out` or new arrays"""
    if out is not None:
        return tuple(out)
    o = tuple(np.empty(nfeat) for _ in range(4))
    return o + (np.empty((m, nfeat)), np.empty((m, nfeat))) if sequences else o


def rhat_series(series, nrows=None, sequences=False, out=None, device=-1):
    """split R-hat across series [n, nseries, nfeat] on the device, over the newest `nrows` rows (None: the largest even count) of
    every series: (rhat, mean, within, between)[nfeat]; sequences=True adds (seq_mean, seq_var)[2 nseries, nfeat], the halves of
    series s being sequences 2s and 2s + 1 (ptm_rhat_series).  out: arrays to fill instead (they keep their contents when the call fails)."""
    a = _series3(series)
    n, ns, nf = a.shape
    if nrows is None:
        nrows = n - n % 2
    o = _rhat_outputs(2 * ns, nf, sequences, out)
    p = [_d(v) for v in o] + [None] * (6 - len(o))
    _chk(load().ptm_rhat_series(device, _d(a), n, ns, nf, int(nrows), *p))
    return o


def _moments_outputs(m, nfeat, cov, walker_sums, out):
    """(mean, cov, var[, walker_sum]) to fill, cov None where it is not asked for: the caller's `out` or new arrays"""
    if out is not None:
        return tuple(out)
    o = (np.empty(nfeat), np.empty((nfeat, nfeat)) if cov else None, np.empty(nfeat))
    return o + (np.empty((m, nfeat)),) if walker_sums else o


def _moments_call(fn, head, o):
    count = C.c_int64(0)
    p = [None if v is None else _d(v) for v in o] + [None] * (4 - len(o))
    _chk(fn(*head, *p, C.byref(count)))
    return tuple(o) + (int(count.value),)


def moments_series(series, nrows=None, cov=True, walker_sums=False, out=None, device=-1):
    """pooled mean and covariance across series [n, nseries, nfeat] on the device, over the newest `nrows` rows (None: all) of every
    series: (mean[nfeat], cov[nfeat, nfeat], var[nfeat], N); cov=False (needed above 128 features): cov is None; walker_sums=True adds
    the per-series sums [nseries, nfeat] in front of N (ptm_moments_series).  out: arrays to fill instead, (mean, cov or None, var
    [, walker_sum]) (they keep their contents when the call fails)."""
    a = _series3(series)
    n, ns, nf = a.shape
    if nrows is None:
        nrows = n
    o = _moments_outputs(ns, nf, cov, walker_sums, out)
    return _moments_call(load().ptm_moments_series, (device, _d(a), n, ns, nf, int(nrows)), o)


def eigen_factors(cov, lambdas=False, sweeps=False, device=-1):
    """the Gaussian proposal factors F = V diag(sqrt(max(lambda, 0))) of symmetric matrices cov [n_mat, n, n] (or one, [n, n]) by the
    facade's cyclic Jacobi, on the device, with the host's bits (ptm_eigen_factors): F shaped like cov; lambdas=True adds the ascending
    eigenvalues [n_mat, n], sweeps=True the sweeps that rotated [n_mat] (a tuple then)."""
    a = np.ascontiguousarray(cov, dtype=np.float64)
    if a.ndim not in (2, 3) or a.shape[-1] != a.shape[-2]:
        raise PtmError("eigen_factors: cov must be [n, n] or [n_mat, n, n]")
    n = a.shape[-1]
    m = 1 if a.ndim == 2 else a.shape[0]
    f = np.empty_like(a)
    lam = np.empty(a.shape[:-1]) if lambdas else None
    sw = np.empty(a.shape[:-2], dtype=np.int32) if sweeps else None
    _chk(load().ptm_eigen_factors(device, _d(a), m, n, _d(f), None if lam is None else _d(lam), None if sw is None else sw.ctypes.data_as(_i32p)))
    o = (f,) + ((lam,) if lambdas else ()) + ((sw,) if sweeps else ())
    return f if len(o) == 1 else o


def moments_tile_rows(nfeat):
    """the rows of a window one staging tile of the covariance kernel holds (ptm_moments_tile_rows)"""
    return int(load().ptm_moments_tile_rows(int(nfeat)))


def _quantiles_call(fn, head, probs, nfeat, brackets, out):
    """(q[nq, nfeat][, x_lo, x_hi], N): the caller's `out` arrays or new ones"""
    p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    o = tuple(out) if out is not None else tuple(np.empty((p.size, nfeat)) for _ in range(3 if brackets else 1))
    count = C.c_int64(0)
    a = [_d(v) for v in o] + [None] * (3 - len(o))
    _chk(fn(*head, p.size, _d(p), *a, C.byref(count)))
    return tuple(o) + (int(count.value),)


def quantiles_series(series, probs, nrows=None, brackets=False, out=None, device=-1):
    """exact pooled quantiles across series [n, nseries, nfeat] on the device, over the newest `nrows` rows (None: all) of every
    series, at the probabilities `probs` (numpy's linear rule): (q[nq, nfeat], N); brackets=True: (q, x_lo, x_hi, N) with the two
    order statistics each quantile lies between (ptm_quantiles_series).  out: arrays to fill instead, (q[, x_lo, x_hi]) (they
    keep their contents when the call fails)."""
    a = _series3(series)
    n, ns, nf = a.shape
    if nrows is None:
        nrows = n
    return _quantiles_call(load().ptm_quantiles_series, (device, _d(a), n, ns, nf, int(nrows)), probs, nf, brackets, out)


def quantiles_last_path():
    """(packed, ring_passes, packed_passes) of the last quantiles call of this process (ptm_quantiles_last_path)"""
    r, k = C.c_int32(0), C.c_int32(0)
    packed = load().ptm_quantiles_last_path(C.byref(r), C.byref(k))
    return bool(packed), int(r.value), int(k.value)


def _i64(a):
    return a.ctypes.data_as(_i64p)


def histogram_edges(lo, hi, nbins):
    """the nbins + 1 edges of the range [lo, hi] as ptm_histograms defines them: lo + k * ((hi - lo) / nbins), the last one hi
    itself -- np.linspace(lo, hi, nbins + 1) bit for bit.  lo, hi: numbers or arrays [nfeat] (the edges: [nfeat, nbins + 1])"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    step = (hi - lo) / np.float64(nbins)
    e = lo[..., None] + np.arange(nbins + 1, dtype=np.float64) * step[..., None]
    e[..., nbins] = hi
    return e


def _histograms_call(fn, head, lo, hi, nbins, nfeat, pairs, out):
    """(h1[nfeat, nbins], h2[npairs, nbins, nbins] or None, below, above, N): the caller's `out` arrays or new ones"""
    lo = np.ascontiguousarray(lo, dtype=np.float64).reshape(-1)
    hi = np.ascontiguousarray(hi, dtype=np.float64).reshape(-1)
    if lo.size != nfeat or hi.size != nfeat:
        raise ValueError("lo and hi must hold one value for each of the %d features" % nfeat)
    nb, npairs = max(int(nbins), 0), nfeat * (nfeat - 1) // 2
    if out is not None:
        h1, h2, below, above = out
    else:
        if pairs and npairs * nb * nb > 1 << 25:
            h2 = np.zeros((0, nb, nb), dtype=np.int64)   # (refused by the call: nothing that large is allocated for it)
        else:
            h2 = np.zeros((npairs, nb, nb), dtype=np.int64) if pairs else None
        h1, below, above = np.zeros((nfeat, nb), dtype=np.int64), np.zeros(nfeat, dtype=np.int64), np.zeros(nfeat, dtype=np.int64)
    count = C.c_int64(0)
    _chk(fn(*head, int(nbins), _d(lo), _d(hi), _i64(h1), _i64(h2) if h2 is not None else None, _i64(below), _i64(above), C.byref(count)))
    return h1, h2, below, above, int(count.value)


def histograms_series(series, lo, hi, nbins, nrows=None, pairs=True, out=None, device=-1):
    """the corner plot's counts across series [n, nseries, nfeat] on the device, over the newest `nrows` rows (None: all) of every
    series: (h1[nfeat, nbins], h2[npairs, nbins, nbins] or None, below[nfeat], above[nfeat], N), int64; the bins of feature f are
    histogram_edges(lo[f], hi[f], nbins), the last one closed (np.histogram's counts), the pairs i < j in row-major order
    (np.histogram2d's counts); pairs=False: no h2 (ptm_histograms_series).  out: arrays to fill instead, (h1, h2 or None, below,
    above) (they keep their contents when the call fails)."""
    a = _series3(series)
    n, ns, nf = a.shape
    if nrows is None:
        nrows = n
    return _histograms_call(load().ptm_histograms_series, (device, _d(a), n, ns, nf, int(nrows)), lo, hi, nbins, nf, pairs, out)


def histograms_last_launch():
    """(tiles, pairs of a tile, mapping) of the 2-D kernel in the last histograms call of this process (ptm_histograms_last_launch)"""
    t, n, m = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    load().ptm_histograms_last_launch(C.byref(t), C.byref(n), C.byref(m))
    return int(n.value), int(t.value), "rows" if m.value else "pairs"


def read_corner(path):
    """the corner file --corner_out writes (the facade's write_corner): a dict with dim, nbins, count, replicas, rows, names, lo, hi,
    below, above [dim], h1 [dim, nbins] and h2 [npairs, nbins, nbins] (int64; the pairs i < j in row-major order)"""
    lines = [ln.split() for ln in open(path) if ln.strip()]
    head = lines[0]
    if head[:4] != ["#", "posterior", "histograms:", "dim"]:
        raise ValueError("%s: the header line is missing" % path)
    keys = dict(zip(head[3::2], head[4::2]))
    dim, nbins = int(keys["dim"]), int(keys["nbins"])
    body = [ln for ln in lines[1:] if not ln[0].startswith("#")]
    npairs = int(keys["pairs"])                                        # (0: written without the pairs)
    if npairs not in (0, dim * (dim - 1) // 2) or len(body) != dim + npairs:
        raise ValueError("%s: expected %d lines, found %d" % (path, dim + npairs, len(body)))
    one, two = body[:dim], body[dim:]
    if any(len(ln) != 5 + nbins for ln in one) or any(len(ln) != 2 + nbins * nbins for ln in two):
        raise ValueError("%s: a line holds another number of values than its bins" % path)
    return {
        "dim": dim, "nbins": nbins, "count": int(keys["N"]), "replicas": int(keys["replicas"]), "rows": int(keys["rows"]),
        "names": [ln[0] for ln in one],
        "lo": np.array([float(ln[1]) for ln in one]), "hi": np.array([float(ln[2]) for ln in one]),
        "below": np.array([int(ln[3]) for ln in one], dtype=np.int64), "above": np.array([int(ln[4]) for ln in one], dtype=np.int64),
        "h1": np.array([[int(v) for v in ln[5:]] for ln in one], dtype=np.int64).reshape(dim, nbins),
        "h2": np.array([[int(v) for v in ln[2:]] for ln in two], dtype=np.int64).reshape(npairs, nbins, nbins),
        "pairs": [(ln[0], ln[1]) for ln in two],
    }


SEAM_SIGMAS = 6.0   # a wrapped dimension's Gaussian target keeps this many sigma inside its domain (proposal_invariance)
KL_FLOOR = 5    # test_proposal.hh:402: the floor of the distances is element KL_FLOOR + 1 of the sorted distances within P


def _sets2(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError("a sample set must be an array [n, dim]")
    return a


def nn_dist2(P, Q=None, wrapped=None, xmin=None, xmax=None, out=None, device=-1):
    """for every point of P [nP, dim] the squared distance to its nearest point of Q [nQ, dim], exactly, on the device; Q=None: to the
    nearest OTHER point of P itself (a duplicate gives 0).  wrapped [dim]: the dimensions that wrap around [xmin, xmax) -- there the
    distance is the smaller of |b - a| and the same with both points shifted by half the domain and wrapped (state::dist2).
    The bits are those of the facade's kl_estimator (ptm_nn_dist2).  out: the array to fill (it keeps its contents when the call fails)."""
    p = _sets2(P)
    q = p if Q is None else _sets2(Q)
    if q.shape[1] != p.shape[1]:
        raise ValueError("P and Q differ in dimension")
    dim = p.shape[1]
    w = lo = hi = None
    if wrapped is not None:
        w = np.ascontiguousarray(wrapped, dtype=np.int32)
        lo, hi = (np.ascontiguousarray(np.zeros(dim) if v is None else v, dtype=np.float64) for v in (xmin, xmax))
        if w.size != dim or lo.size != dim or hi.size != dim:
            raise ValueError("wrapped, xmin and xmax must have one entry per dimension")
    o = np.empty(p.shape[0]) if out is None else out
    _chk(load().ptm_nn_dist2(device, _d(p), p.shape[0], _d(q), q.shape[0], dim, None if w is None else w.ctypes.data_as(_i32p),
                             None if w is None else _d(lo), None if w is None else _d(hi), 1 if Q is None else 0, _d(o)))
    return o


def _c_log(v):
    """the C library's logarithm with its IEEE edges (numpy's own vectorised logarithm may round differently)"""
    import math
    v = float(v)
    if v != v or v < 0:
        return math.nan
    return -math.inf if v == 0 else (math.inf if v == math.inf else math.log(v))


def kl_from_distances(r1sqs, s1sqs, dim, M):
    """the k-NN KL estimate from the distances within P and to the M points of Q, in the estimator's order (test_proposal.hh:400-421)"""
    import math
    r, s = np.array(r1sqs, dtype=np.float64), np.array(s1sqs, dtype=np.float64)
    if r.size < KL_FLOOR + 2 or M < 1:
        raise ValueError("the KL estimator needs at least %d samples of P and 1 of Q" % (KL_FLOOR + 2))
    floor = np.sort(r)[KL_FLOOR + 1]
    r, s = np.where(r < floor, floor, r), np.where(s < floor, floor, s)
    with np.errstate(all="ignore"):
        ratio = r / s
    result, N = 0.0, float(r.size)
    for v in ratio:
        result = result + -_c_log(v)
    return result * ((0.5 * float(dim)) / N) + math.log(int(M) / (N - 1.0))


def kl_divergence(P, Q, wrapped=None, xmin=None, xmax=None, device=-1):
    """the k-NN Kullback-Leibler estimate of Perez-Cruz (k = 1) of the sets P from Q, as the reference's proposal test computes it with
    exact neighbours: the two nearest-neighbour searches run on the device (nn_dist2), floor and sum here"""
    p, q = _sets2(P), _sets2(Q)
    if p.shape[0] < KL_FLOOR + 2 or q.shape[0] < 1:
        raise ValueError("the KL estimator needs at least %d samples of P and 1 of Q" % (KL_FLOOR + 2))
    r = nn_dist2(p, None, wrapped, xmin, xmax, device=device)
    s = nn_dist2(p, q, wrapped, xmin, xmax, device=device)
    return kl_from_distances(r, s, p.shape[1], q.shape[0])


def _gauss_jordan(a):
    """(inverse, determinant) by Gauss-Jordan elimination with partial pivoting, as the facade's kl_estimator::invert"""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    inv, det = np.eye(n), 1.0
    for c in range(n):
        piv = c + int(np.argmax(np.abs(a[c:, c])))
        if a[piv, c] == 0.0:
            return None, 0.0
        if piv != c:
            a[[piv, c]], inv[[piv, c]] = a[[c, piv]], inv[[c, piv]]
            det = -det
        d = a[c, c]
        det = det * d
        a[c], inv[c] = a[c] / d, inv[c] / d
        f = a[:, c].copy()
        f[c] = 0.0
        a, inv = a - f[:, None] * a[c][None, :], inv - f[:, None] * inv[c][None, :]
    return inv, det


def fake_kl_divergence(P, Q):
    """the Gaussian "fake KL" of the reference's proposal test, from the two sets' means and covariances (test_proposal.hh:466-502, the
    unbiasing factor with the size of P as written there).  O(N dim^2): it stays on the host."""
    p, q = _sets2(P), _sets2(Q)
    dim, n = p.shape[1], p.shape[0]
    if n < 2 or q.shape[0] < 2 or q.shape[1] != dim:
        raise ValueError("the fake KL needs two sets of at least 2 samples in the same dimension")

    def moments(x):
        mean = np.add.accumulate(x, axis=0)[-1] / float(x.shape[0])
        d = x - mean
        cov = np.zeros((dim, dim))
        for lo in range(0, x.shape[0], 4096):   # (sequential in sample order, a block of outer products at a time)
            blk = d[lo:lo + 4096]
            cov = np.add.accumulate(np.concatenate([cov[None], blk[:, :, None] * blk[:, None, :]]), axis=0)[-1]
        return mean, cov / (float(x.shape[0]) - 1.0)

    mean_p, cov_p = moments(p)
    mean_q, cov_q = moments(q)
    factor = (n - dim - 2.0) / (n - 1.0)
    inv, _ = _gauss_jordan(cov_q)
    if inv is None:
        return float("nan")
    inv = inv * factor
    prod = np.zeros((dim, dim))
    for k in range(dim):
        prod = prod + cov_p[:, k][:, None] * inv[k][None, :]
    trace = 0.0
    for i in range(dim):
        trace = trace + prod[i, i]
    _, det = _gauss_jordan(prod / factor)
    dmu = mean_p - mean_q
    row = np.zeros(dim)
    for j in range(dim):
        row = row + inv[:, j] * dmu[j]
    quad = 0.0
    for i in range(dim):
        quad = quad + dmu[i] * row[i]
    return 0.5 * (((-dim + trace) + -_c_log(det)) + (quad - (dim + trace) / n))


class DeviceBuffer:
    """A raw device allocation (for tests and tools that have no GPU array library at hand)."""

    def __init__(self, nbytes):
        p = C.c_void_p()
        _chk(load().ptm_dev_alloc(nbytes, C.byref(p)))
        self.ptr, self.nbytes = p.value, nbytes

    def data_ptr(self):
        return self.ptr

    def copy_from(self, src_ptr, nbytes=None):
        _chk(load().ptm_dev_copy(self.ptr, src_ptr, self.nbytes if nbytes is None else nbytes))

    def to_numpy(self, dtype=np.float64):
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        _chk(load().ptm_dev_copy(out.ctypes.data_as(C.c_void_p), self.ptr, self.nbytes))
        return out

    def free(self):
        if self.ptr:
            load().ptm_dev_free(self.ptr)
            self.ptr = None

    __del__ = free

    def slice(self, offset_bytes, nbytes):
        """a view of part of the allocation (the parent keeps the memory)"""
        assert 0 <= offset_bytes and offset_bytes + nbytes <= self.nbytes
        return _DeviceView(self, offset_bytes, nbytes)


class _DeviceView:
    def __init__(self, parent, offset, nbytes):
        self.parent, self.ptr, self.nbytes = parent, parent.ptr + offset, nbytes

    def data_ptr(self):
        return self.ptr

    def copy_from(self, src_ptr, nbytes=None):
        _chk(load().ptm_dev_copy(self.ptr, src_ptr, self.nbytes if nbytes is None else nbytes))

    def to_numpy(self, dtype=np.float64):
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        _chk(load().ptm_dev_copy(out.ctypes.data_as(C.c_void_p), self.ptr, self.nbytes))
        return out


def geometric_ladder(n_rungs, tmax):
    """beta of parallel_tempering_chains' constructor + initialize (chain.cc:1181-1183,1340): host constants."""
    import math
    tratio = math.exp(math.log(tmax) / (n_rungs - 1)) if n_rungs > 1 else 1.0
    t, beta = 1.0, [1.0]
    for _ in range(1, n_rungs):
        t = t * tratio
        beta.append(1 / t)
    return np.array(beta)


class Engine:
    """One GPU shard of a parallel-tempering ladder: rungs [rung_begin, rung_begin+rung_count) x W walkers."""

    def __init__(self, dim, n_rungs, n_walkers=1, seed=0x5EED0001, swap_rate=0.1, add_every_n=1, min_prior=-30.0,
                 rung_begin=0, rung_count=None, device=-1, stream=None, time_kernels=False, exchange_row_capacity=0, history_rungs=0,
                 history_capacity=0, map_rungs=0, walker_begin=0):
        L = load()
        cfg = PtmConfig()
        cfg.struct_size = C.sizeof(PtmConfig)
        cfg.dim, cfg.n_rungs, cfg.rung_begin = dim, n_rungs, rung_begin
        cfg.rung_count = n_rungs if rung_count is None else rung_count
        cfg.n_walkers, cfg.seed, cfg.swap_rate = n_walkers, seed, swap_rate
        cfg.add_every_n, cfg.min_prior, cfg.device = add_every_n, min_prior, device
        cfg.stream = stream
        cfg.time_kernels = 1 if time_kernels else 0
        cfg.swap_log_steps = 0
        cfg.exchange_row_capacity = exchange_row_capacity
        cfg.history_rungs, cfg.history_capacity = history_rungs, history_capacity
        self.hist_rungs, self.hist_cap = history_rungs, history_capacity
        self.prop_kind = None   # the kind of the factors set_proposals installed (adapt_proposals sizes its factors by it)
        self.add_every_n = add_every_n
        cfg.map_rungs = map_rungs
        self.map_rungs = map_rungs
        cfg.walker_begin = walker_begin
        self.walker_begin = walker_begin
        h = C.c_void_p()
        _chk(L.ptm_engine_create(C.byref(cfg), C.byref(h)))
        self.h, self.L = h, L
        self.D, self.Nt, self.W = dim, n_rungs, n_walkers
        self.r0, self.nloc = rung_begin, cfg.rung_count
        self.Nc = self.nloc * n_walkers
        self._evolving = False
        self._evolve_cut = -1.0
        self._keep = []
        self._batch_depth, self._batch_keep = 0, []

    def close(self):
        if getattr(self, "h", None):
            self.L.ptm_engine_destroy(self.h)
            self.h = None

    __del__ = close

    # -- problem description
    def set_bounds(self, lo, hi, xmin, xmax):
        lo = np.ascontiguousarray(lo, dtype=np.int32); hi = np.ascontiguousarray(hi, dtype=np.int32)
        xmin = np.ascontiguousarray(xmin, dtype=np.float64); xmax = np.ascontiguousarray(xmax, dtype=np.float64)
        _chk(self.L.ptm_set_bounds(self.h, lo.ctypes.data_as(_i32p), hi.ctypes.data_as(_i32p), _d(xmin), _d(xmax)))

    def set_prior(self, types, centers, halfwidths):
        t = np.ascontiguousarray([PRIOR_NAMES[v] if isinstance(v, str) else int(v) for v in types], dtype=np.int32)
        c = np.ascontiguousarray(centers, dtype=np.float64); h = np.ascontiguousarray(halfwidths, dtype=np.float64)
        _chk(self.L.ptm_set_prior(self.h, t.ctypes.data_as(_i32p), _d(c), _d(h)))

    def set_target_gaussian(self, precision, like0, mean=None):
        P = np.ascontiguousarray(precision, dtype=np.float64).reshape(self.D, self.D)
        m = None if mean is None else np.ascontiguousarray(mean, dtype=np.float64)
        _chk(self.L.ptm_set_target_gaussian(self.h, None if m is None else _d(m), _d(P), like0))

    def set_target_callback(self, fn, batched=False):
        """user plug-in likelihood (the C shape of bayes_likelihood::register_evaluate_log, bayesian.hh:536-552).
        fn(x[D]) -> float, or with batched=True fn(X[n][D]) -> array of n."""
        def tramp(user, Xp, n, dim, outp):
            X = np.ctypeslib.as_array(Xp, shape=(n, dim))
            out = np.ctypeslib.as_array(outp, shape=(n,))
            if batched:
                out[:] = fn(X)
            else:
                for k in range(n):
                    out[k] = fn(X[k])
        cb = LOGLIKE_BATCH_FN(tramp)
        self._keep.append(cb)
        _chk(self.L.ptm_set_target_callback(self.h, C.cast(cb, C.c_void_p), None))

    def set_target_device(self, fn):
        """user likelihood on the DEVICE (ptm_set_target_device): fn(X, count, out) with torch views -- X (n_rows, D) float64,
        count a 1-element int32 tensor (rows [0, count) are the proposals to evaluate, the rest in-support states), out (n_rows,)
        float64 to fill.  It runs once per sweep with the engine's stream current and must only ENQUEUE its work (no .item(), no
        copy to the host): step(n) queues n steps and returns.  Needs torch imported before the engine library (one HIP runtime)."""
        import torch
        if not TORCH_LOADED_FIRST:
            raise PtmError("set_target_device needs torch imported BEFORE the engine library was loaded (one HIP runtime per process: "
                           "see ptmcmc_amd.parallel.EngineShard)")
        dev = torch.device("cuda", torch.cuda.current_device())
        n, D = self.Nc, self.D
        X = torch.zeros((n, D), dtype=torch.float64, device=dev)
        out = torch.zeros(n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        state = {}

        def tramp(user, stream, n_rows, dim, xp, cp, op):
            cnt = state.get(cp)
            if cnt is None:   # the engine's count buffer, wrapped once (torch has no public from-pointer constructor: a 1-element copy)
                cnt = state[cp] = _wrap_int32_device(torch, cp, dev)
            with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=dev)):
                fn(X, cnt, out)
        cb = LOGLIKE_DEVICE_FN(tramp)
        self._keep += [cb, X, out, state]
        _chk(self.L.ptm_set_target_device(self.h, C.cast(cb, C.c_void_p), None, C.c_void_p(X.data_ptr()), C.c_void_p(out.data_ptr())))

    def set_target_device_c(self, fnptr, user=None, x_batch_dev=None, llike_batch_dev=None):
        """user likelihood on the device through a raw C function pointer of the ptm_loglike_device_fn shape (e.g. from a hipcc-built
        .so: ctypes.cast(lib.my_launcher, ctypes.c_void_p)); batch buffers: device pointers, or None for the engine's own"""
        p = fnptr.value if isinstance(fnptr, C.c_void_p) else (C.cast(fnptr, C.c_void_p).value if isinstance(fnptr, C._CFuncPtr) else int(fnptr))
        self._keep.append(fnptr)
        _chk(self.L.ptm_set_target_device(self.h, C.c_void_p(p), C.c_void_p(user) if user is not None else None,
                                          None if x_batch_dev is None else C.c_void_p(x_batch_dev),
                                          None if llike_batch_dev is None else C.c_void_p(llike_batch_dev)))

    @property
    def target_device_rows(self):
        """n_rows of the device likelihood: the local chain count (ptm_target_device_rows)"""
        r = self.L.ptm_target_device_rows(self.h)
        if r < 0:
            _chk(r)
        return r

    def best_evaluated(self):
        """(best lprior + llike the device likelihood evaluated since the last state set-up, its state [D]) (ptm_get_best_evaluated)"""
        lp = C.c_double()
        x = np.empty(self.D)
        _chk(self.L.ptm_get_best_evaluated(self.h, C.byref(lp), x.ctypes.data_as(_dp)))
        return lp.value, x

    def set_prior_device(self, fn):
        """user prior on the DEVICE (ptm_set_prior_device), beside set_target_device: fn(X, count, out) with torch views of the
        engine's own buffers -- X (n_rows, D) float64, count a 1-element int32 tensor (rows [0, count) are the valid proposals, in
        local-chain order; the rest hold in-support states), out (n_rows,) float64 to fill with log-priors (-inf outside the support).
        It runs once per sweep with the engine's stream current, before the likelihood's function, and must only ENQUEUE its work (no
        .item(), no copy to the host): step(n) queues n steps and returns.  Needs torch imported before the engine library (one HIP
        runtime) and the device likelihood; start states come from set_states.  fn = None goes back to the built-in prior (set the
        states again afterwards)."""
        if fn is None:
            _chk(self.L.ptm_set_prior_device(self.h, None, None))
            return
        import torch
        if not TORCH_LOADED_FIRST:
            raise PtmError("set_prior_device needs torch imported BEFORE the engine library was loaded (one HIP runtime per process: "
                           "see ptmcmc_amd.parallel.EngineShard)")
        dev = torch.device("cuda", torch.cuda.current_device())
        views = {}

        def view(ptr, shape, typestr):
            key = (ptr, shape, typestr)
            v = views.get(key)
            if v is None:   # the engine's buffers are fixed for its lifetime: each is wrapped once
                v = views[key] = _wrap_device(torch, ptr, shape, typestr, dev)
            return v

        def tramp(user, stream, n_rows, dim, xp, cp, op):
            with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=dev)):
                fn(view(xp, (n_rows, dim), "<f8"), view(cp, (1,), "<i4"), view(op, (n_rows,), "<f8"))
        cb = LOGLIKE_DEVICE_FN(tramp)   # (ptm_logprior_device_fn has ptm_loglike_device_fn's shape)
        self._keep += [cb, views]
        _chk(self.L.ptm_set_prior_device(self.h, C.cast(cb, C.c_void_p), None))

    def set_prior_device_c(self, fnptr, user=None):
        """user prior on the device through a raw C function pointer of the ptm_logprior_device_fn shape (e.g. from a hipcc-built
        .so: ctypes.cast(lib.my_launcher, ctypes.c_void_p)); user: the pointer it is handed"""
        p = fnptr.value if isinstance(fnptr, C.c_void_p) else (C.cast(fnptr, C.c_void_p).value if isinstance(fnptr, C._CFuncPtr) else int(fnptr))
        self._keep.append(fnptr)
        _chk(self.L.ptm_set_prior_device(self.h, C.c_void_p(p), C.c_void_p(user) if user is not None else None))

    def set_prior_callback(self, fn, batched=False):
        """a prior evaluated on the host (ptm_set_prior_callback): the C shape of probability_function::evaluate_log
        (probability_function.hh:31-44) for priors ptm_set_prior cannot describe.  fn(x[D]) -> log-prior (-inf outside the
        support), or with batched=True fn(X[n][D]) -> array of n.  Needs set_target_callback; start states come from set_states."""
        if fn is None:
            _chk(self.L.ptm_set_prior_callback(self.h, None, None))
            return
        def tramp(user, Xp, n, dim, outp):
            X = np.ctypeslib.as_array(Xp, shape=(n, dim))
            out = np.ctypeslib.as_array(outp, shape=(n,))
            if batched:
                out[:] = fn(X)
            else:
                for k in range(n):
                    out[k] = fn(X[k])
        cb = LOGLIKE_BATCH_FN(tramp)
        self._keep.append(cb)
        _chk(self.L.ptm_set_prior_callback(self.h, C.cast(cb, C.c_void_p), None))

    def set_proposal_callback(self, propose, result=None):
        """host-side proposals (ptm_set_proposal_callback): the C shape of proposal_distribution::draw / log_hastings_ratio /
        type and accept / reject (proposal_distribution.hh:65-87).
        propose: a C callback (PROPOSE_BATCH_FN or any ctypes function pointer of that signature), or a Python function
          propose(X_cur[n][D], rung[n], walker[n], step) -> (X_prop[n][D], log_hastings[n], type[n], valid[n]);
        result:  optional Python function result(rung[n], walker[n], accepted[n]) called after every sweep."""
        if propose is None:
            _chk(self.L.ptm_set_proposal_callback(self.h, None, None, None))
            return
        if not isinstance(propose, C._CFuncPtr):
            fn = propose

            def tramp(user, n, dim, xc, rung, walker, step, xp, lh, ty, va):
                P, H, T, V = fn(np.ctypeslib.as_array(xc, shape=(n, dim)).copy(), np.ctypeslib.as_array(rung, shape=(n,)).copy(),
                                np.ctypeslib.as_array(walker, shape=(n,)).copy(), int(step))
                np.ctypeslib.as_array(xp, shape=(n, dim))[:] = P
                np.ctypeslib.as_array(lh, shape=(n,))[:] = H
                np.ctypeslib.as_array(ty, shape=(n,))[:] = T
                np.ctypeslib.as_array(va, shape=(n,))[:] = V
            propose = PROPOSE_BATCH_FN(tramp)
        rcb = None
        if result is not None:
            rf = result

            def rtramp(user, n, rung, walker, acc):
                rf(np.ctypeslib.as_array(rung, shape=(n,)).copy(), np.ctypeslib.as_array(walker, shape=(n,)).copy(),
                   np.ctypeslib.as_array(acc, shape=(n,)).copy())
            rcb = PROPOSAL_RESULT_FN(rtramp)
        self._keep += [propose, rcb]
        _chk(self.L.ptm_set_proposal_callback(self.h, C.cast(propose, C.c_void_p), None if rcb is None else C.cast(rcb, C.c_void_p), None))

    def set_proposal_device(self, fn, result=None):
        """proposals on the DEVICE (ptm_set_proposal_device): fn(X_cur, rung, walker, count, step, X_prop, log_hastings, type, valid)
        with torch views of the engine's buffers -- X_cur / X_prop (n_rows, D) float64, rung / walker / type / valid (n_rows,)
        int32, log_hastings (n_rows,) float64, count a 1-element int32 tensor, step a Python int.  Rows [0, count) are the chains
        that move this step, in local-chain order; the rest hold the other chains' states, so a fixed-shape evaluation is safe.
        log_hastings, type and valid arrive preset to 0, 0, 1; X_prop is to be filled with whole states.
        result(rung, walker, count, accepted), optional, sees the outcomes (accepted[k] in {0, 1} for k < count) after every sweep.
        Both run once per sweep with the engine's stream current and must only ENQUEUE their work (no .item(), no copy to the
        host): step(n) queues n steps and returns.  Needs torch imported before the engine library (one HIP runtime).
        fn = None goes back to the engine's own proposals."""
        if fn is None:
            _chk(self.L.ptm_set_proposal_device(self.h, None, None, None))
            return
        import torch
        if not TORCH_LOADED_FIRST:
            raise PtmError("set_proposal_device needs torch imported BEFORE the engine library was loaded (one HIP runtime per process: "
                           "see ptmcmc_amd.parallel.EngineShard)")
        dev = torch.device("cuda", torch.cuda.current_device())
        views = {}

        def view(ptr, shape, typestr):
            key = (ptr, shape, typestr)
            v = views.get(key)
            if v is None:   # the engine's buffers are fixed for its lifetime: each is wrapped once
                v = views[key] = _wrap_device(torch, ptr, shape, typestr, dev)
            return v

        def tramp(user, stream, n, dim, xc, rg, wk, cnt, step, xp, lh, ty, va):
            with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=dev)):
                fn(view(xc, (n, dim), "<f8"), view(rg, (n,), "<i4"), view(wk, (n,), "<i4"), view(cnt, (1,), "<i4"), int(step),
                   view(xp, (n, dim), "<f8"), view(lh, (n,), "<f8"), view(ty, (n,), "<i4"), view(va, (n,), "<i4"))
        cb = PROPOSE_DEVICE_FN(tramp)
        rcb = None
        if result is not None:
            def rtramp(user, stream, n, rg, wk, cnt, acc):
                with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=dev)):
                    result(view(rg, (n,), "<i4"), view(wk, (n,), "<i4"), view(cnt, (1,), "<i4"), view(acc, (n,), "<i4"))
            rcb = PROPOSAL_RESULT_DEVICE_FN(rtramp)
        self._keep += [cb, rcb, views]
        _chk(self.L.ptm_set_proposal_device(self.h, C.cast(cb, C.c_void_p), None if rcb is None else C.cast(rcb, C.c_void_p), None))

    def set_proposal_device_c(self, fnptr, result_fnptr=None, user=None):
        """proposals on the device through raw C function pointers of the ptm_propose_device_fn / ptm_proposal_result_device_fn
        shapes (e.g. from a hipcc-built .so: ctypes.cast(lib.my_launcher, ctypes.c_void_p)); user: the pointer both are handed"""
        def raw(f):
            if f is None:
                return None
            return f.value if isinstance(f, C.c_void_p) else (C.cast(f, C.c_void_p).value if isinstance(f, C._CFuncPtr) else int(f))
        self._keep += [fnptr, result_fnptr]
        p, r = raw(fnptr), raw(result_fnptr)
        _chk(self.L.ptm_set_proposal_device(self.h, None if p is None else C.c_void_p(p), None if r is None else C.c_void_p(r),
                                            C.c_void_p(user) if user is not None else None))

    def set_ladder(self, beta):
        b = np.ascontiguousarray(beta, dtype=np.float64)
        assert b.size == self.Nt
        _chk(self.L.ptm_set_ladder(self.h, _d(b)))

    def set_evolve_temps(self, rate, lpost_cut=-1.0):
        """parallel_tempering_chains::evolve_temps (chain.hh:302-307): every accepted exchange pries its gap apart"""
        _chk(self.L.ptm_set_evolve_temps(self.h, float(rate), float(lpost_cut)))
        self._evolving = self._evolving or rate > 0
        self._evolve_cut = lpost_cut if lpost_cut >= 0 else -1.0

    def invtemps(self):
        """[W][Nt] inverse temperatures of every ladder"""
        b = self._out(np.empty((self.W, self.Nt)))
        _chk(self.L.ptm_get_invtemps(self.h, b.ctypes.data_as(_dp)))
        return b

    def set_invtemps(self, beta):
        b = np.ascontiguousarray(beta, dtype=np.float64)
        assert b.size == self.W * self.Nt
        _chk(self.L.ptm_set_invtemps(self.h, b.ctypes.data_as(_dp)))

    def set_proposals(self, kind, factors, one_d_frac=None):
        f = np.ascontiguousarray(factors, dtype=np.float64)
        per = self.D if kind == PROP_DIAG else self.D * self.D
        assert f.size == self.nloc * per, (f.size, self.nloc, per)
        o = None if one_d_frac is None else np.ascontiguousarray(one_d_frac, dtype=np.float64)
        _chk(self.L.ptm_set_proposals(self.h, kind, _d(f), None if o is None else _d(o)))
        self.prop_kind = kind

    # -- state
    def set_states(self, X, llike=None):
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(self.Nc, self.D)
        ll = None if llike is None else np.ascontiguousarray(llike, dtype=np.float64)
        _chk(self.L.ptm_set_states(self.h, _d(X), None if ll is None else _d(ll)))

    # -- native RCCL sharding (ptm_shard_*): the C/C++ host's form of ptmcmc_amd.parallel.ShardedLadder
    @staticmethod
    def shard_unique_id():
        buf = C.create_string_buffer(128)
        _chk(load().ptm_shard_unique_id(buf))
        return buf.raw

    def shard_init(self, uid, rank, world, rung_counts, halo=0):
        rc = np.ascontiguousarray(rung_counts, dtype=np.int32)
        _chk(self.L.ptm_shard_init(self.h, C.c_char_p(uid), rank, world, rc.ctypes.data_as(_i32p), halo))

    def shard_step(self, n=1):
        _chk(self.L.ptm_shard_step(self.h, n))

    def shard_finalize(self):
        _chk(self.L.ptm_shard_finalize(self.h))

    def init_from_prior(self, k=0):
        """the k-th initial draw of every chain (k = 0: MH_chain::initialize(1)'s; ptm_init_from_prior_k)"""
        _chk(self.L.ptm_init_from_prior_k(self.h, int(k)))

    def history_chains(self, chain_begin, chain_count):
        """the ring entries of a range of history chains, in arrays of history()'s full layout whose other entries are NaN / -1 (ptm_get_history_chains)"""
        cap, HC, D = self.hist_cap, self.hist_rungs * self.W, self.D
        x = np.full((cap, HC, D), np.nan); ll = np.full((cap, HC), np.nan); lp = np.full((cap, HC), np.nan); beta = np.full((cap, HC), np.nan)
        meta = np.full((cap, HC, 4), -1, dtype=np.int32)
        self.L.ptm_get_history_chains.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, C.c_void_p, _dp]
        _chk(self.L.ptm_get_history_chains(self.h, int(chain_begin), int(chain_count), x.ctypes.data_as(_dp), ll.ctypes.data_as(_dp), lp.ctypes.data_as(_dp),
                                           meta.ctypes.data, beta.ctypes.data_as(_dp)))
        return dict(x=x, llike=ll, lprior=lp, meta=meta, invtemp=beta)

    def draw_prior_rows(self, k_begin, n):
        """draws k_begin .. k_begin + n - 1 of every chain, the engine's state untouched (ptm_draw_prior_rows): x [n][Nc][D], llike, lprior [n][Nc]"""
        x = np.empty((n, self.Nc, self.D)); ll = np.empty((n, self.Nc)); lp = np.empty((n, self.Nc))
        _chk(self.L.ptm_draw_prior_rows(self.h, int(k_begin), int(n), x.ctypes.data_as(_dp), ll.ctypes.data_as(_dp), lp.ctypes.data_as(_dp)))
        return x, ll, lp

    # -- hot path
    def sweep(self, n=1):
        _chk(self.L.ptm_sweep(self.h, n))

    def step(self, n=1):
        _chk(self.L.ptm_step(self.h, n))

    def sync(self):
        _chk(self.L.ptm_sync(self.h))

    def llike_device_ptr(self):
        p = C.c_void_p()
        _chk(self.L.ptm_llike_device_ptr(self.h, C.byref(p)))
        return p.value

    def copy_llike(self, first_local_rung, n_rungs, dst_dev):
        _chk(self.L.ptm_copy_llike(self.h, first_local_rung, n_rungs, dst_dev))

    def copy_lprior(self, first_local_rung, n_rungs, dst_dev):
        _chk(self.L.ptm_copy_lprior(self.h, first_local_rung, n_rungs, dst_dev))

    def exchange_decide_gathered(self, ll_all_dev, lp_all_dev, send_up_dev, send_down_dev):
        """the exchange phase from the whole ladder's llikes [Nt][W] (and lpriors, with a posterior-ordering cut)"""
        _chk(self.L.ptm_exchange_decide_gathered(self.h, ll_all_dev, lp_all_dev, send_up_dev, send_down_dev))

    def set_shard_map(self, rung_counts, halo):
        """recovery of runs longer than a halo (ptm_set_shard_map): every shard's rung count, the halo depth all ask for"""
        rc = np.ascontiguousarray(rung_counts, dtype=np.int32)
        _chk(self.L.ptm_set_shard_map(self.h, rc.size, rc.ctypes.data_as(_i32p), int(halo)))

    def exchange_redo_count(self):
        n = C.c_int32()
        _chk(self.L.ptm_exchange_redo_count(self.h, C.byref(n)))
        return n.value

    def exchange_redo(self, ll_all_dev, lp_all_dev, send_up_dev, send_down_dev):
        _chk(self.L.ptm_exchange_redo(self.h, ll_all_dev, lp_all_dev, send_up_dev, send_down_dev))

    def exchange_decide(self, ll_below_dev, ll_above_dev, halo_rungs, send_up_dev, send_down_dev):
        _chk(self.L.ptm_exchange_decide(self.h, ll_below_dev, ll_above_dev, halo_rungs, send_up_dev, send_down_dev))

    def exchange_install(self, recv_below_dev, recv_above_dev):
        _chk(self.L.ptm_exchange_install(self.h, recv_below_dev, recv_above_dev))

    def sweep_rungs(self, first_local_rung, n_rungs, closes_step):
        _chk(self.L.ptm_sweep_rungs(self.h, first_local_rung, n_rungs, 1 if closes_step else 0))

    @property
    def exchange_buffer_doubles(self):
        return self.L.ptm_exchange_buffer_doubles(self.h)

    def set_proposal_mixture(self, cum_shares, scales, one_d_fracs):
        """arrays [rung_count][K]; K = 0 (empty arrays) removes the mixture"""
        cs, sc, od = (np.ascontiguousarray(a, dtype=np.float64) for a in (cum_shares, scales, one_d_fracs))
        K = 0 if cs.size == 0 else cs.shape[1]
        _chk(self.L.ptm_set_proposal_mixture(self.h, K, cs.ctypes.data_as(_dp), sc.ctypes.data_as(_dp), od.ctypes.data_as(_dp)))

    def set_proposal_de(self, snooker=0.1, gamma_one_frac=0.3, reduce_gamma=4.0, ignore_frac=0.0, init_rows=None, off=False):
        """differential evolution on the device as the member of negative scale of the proposal sets (ptm_set_proposal_de);
        init_rows [n_extra][Nc][D] in the engine's chain order"""
        if off:
            _chk(self.L.ptm_set_proposal_de(self.h, None, 0, None))
            return
        q = PtmDeParams(snooker, gamma_one_frac, reduce_gamma, ignore_frac)
        ir = None if init_rows is None else np.ascontiguousarray(init_rows, dtype=np.float64).reshape(-1, self.Nc, self.D)
        _chk(self.L.ptm_set_proposal_de(self.h, C.byref(q), 0 if ir is None else ir.shape[0], None if ir is None else ir.ctypes.data_as(_dp)))

    def set_proposal_prior_draw(self, member):
        """the member of the current proposal set (mixture, or top level of the adaptive set) that draws whole states from the prior
        on the device (ptm_set_proposal_prior_draw); -1 switches it off"""
        _chk(self.L.ptm_set_proposal_prior_draw(self.h, int(member)))

    def set_proposal_adaptive(self, K, scales, one_d_fracs, weights, thresholds, repeat_bits=None, outcomes=None, nested=-1, K_inner=0,
                              rate=0.0, rate_inner=0.0):
        """an adaptive proposal set (ptm_set_proposal_adaptive): leaves scales / one_d_fracs [rung_count][K + K_inner] (scale < 0: the
        differential-evolution member), the initial state per local chain in the engine's chain order: weights / thresholds
        [Nc][K + K_inner], repeat bits / outcome counts [Nc][2] (default: every last outcome an accept, no outcomes yet)"""
        L = K + K_inner
        sc = np.ascontiguousarray(scales, dtype=np.float64).reshape(self.nloc, L)
        od = np.ascontiguousarray(one_d_fracs, dtype=np.float64).reshape(self.nloc, L)
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(self.Nc, L)
        th = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(self.Nc, L)
        if repeat_bits is None:
            repeat_bits = np.tile(np.array([(1 << K) - 1, (1 << K_inner) - 1], dtype=np.int32), (self.Nc, 1))
        if outcomes is None:
            outcomes = np.zeros((self.Nc, 2), dtype=np.int32)
        rb = np.ascontiguousarray(repeat_bits, dtype=np.int32).reshape(self.Nc, 2)
        oc = np.ascontiguousarray(outcomes, dtype=np.int32).reshape(self.Nc, 2)
        a = PtmAdaptiveSet(int(K), int(nested), int(K_inner), float(rate), float(rate_inner))
        _chk(self.L.ptm_set_proposal_adaptive(self.h, C.byref(a), sc.ctypes.data_as(_dp), od.ctypes.data_as(_dp), w.ctypes.data_as(_dp),
                                              th.ctypes.data_as(_dp), rb.ctypes.data_as(_i32p), oc.ctypes.data_as(_i32p)))
        self._ada_L = L

    def proposal_adapt_state(self):
        """the adaptive set's per-chain state (ptm_get_proposal_adapt_state): dict weights, thresholds [Nc][L], repeat_bits, outcomes [Nc][2]"""
        L = getattr(self, "_ada_L", 0)
        w = self._out(np.empty((self.Nc, max(L, 1)))); th = self._out(np.empty((self.Nc, max(L, 1))))
        rb = self._out(np.empty((self.Nc, 2), dtype=np.int32)); oc = self._out(np.empty((self.Nc, 2), dtype=np.int32))
        _chk(self.L.ptm_get_proposal_adapt_state(self.h, w.ctypes.data_as(_dp), th.ctypes.data_as(_dp), rb.ctypes.data_as(_i32p), oc.ctypes.data_as(_i32p)))
        return dict(weights=w, thresholds=th, repeat_bits=rb, outcomes=oc)

    def set_proposal_adapt_state(self, weights, thresholds, repeat_bits, outcomes):
        w = np.ascontiguousarray(weights, dtype=np.float64)
        th = np.ascontiguousarray(thresholds, dtype=np.float64)
        rb = np.ascontiguousarray(repeat_bits, dtype=np.int32)
        oc = np.ascontiguousarray(outcomes, dtype=np.int32)
        _chk(self.L.ptm_set_proposal_adapt_state(self.h, w.ctypes.data_as(_dp), th.ctypes.data_as(_dp), rb.ctypes.data_as(_i32p), oc.ctypes.data_as(_i32p)))

    def set_proposal_rung(self, local_rung, factor, one_d_frac=-1.0):
        f = np.ascontiguousarray(factor, dtype=np.float64)
        _chk(self.L.ptm_set_proposal_rung(self.h, local_rung, f.ctypes.data_as(_dp), float(one_d_frac)))

    def map(self):
        """MAP of the tracked rungs: dict x [map_rungs*W][D], lpost, llike, lprior [map_rungs*W]"""
        n = self.map_rungs * self.W
        X = self._out(np.empty((n, self.D))); lpo = self._out(np.empty(n)); ll = self._out(np.empty(n)); lp = self._out(np.empty(n))
        _chk(self.L.ptm_get_map(self.h, X.ctypes.data_as(_dp), lpo.ctypes.data_as(_dp), ll.ctypes.data_as(_dp), lp.ctypes.data_as(_dp)))
        return dict(x=X, lpost=lpo, llike=ll, lprior=lp)

    def checkpoint(self):
        """everything the run's future depends on (ptm_restore)"""
        t, a = self.swap_counts()
        return dict(invtemps=self.invtemps() if self._evolving else None, history=self.history() if self.hist_rungs else None,
                    map=self.map() if self.map_rungs else None, x=self.states(), llike=self.llike, ntries=self.ntries.astype(np.int32), naccept=self.naccept.astype(np.int32),
                    last_type=self.last_type.astype(np.int32), nhist=self.nhist.astype(np.int64), step=self.step_count,
                    swap_tries=np.ascontiguousarray(t, dtype=np.int64), swap_accepts=np.ascontiguousarray(a, dtype=np.int64))

    def restore(self, ck):
        i64 = lambda v: np.ascontiguousarray(v, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
        i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32).ctypes.data_as(_i32p)
        f64 = lambda v: np.ascontiguousarray(v, dtype=np.float64).ctypes.data_as(_dp)
        _chk(self.L.ptm_restore(self.h, f64(ck["x"]), f64(ck["llike"]), i32(ck["ntries"]), i32(ck["naccept"]), i32(ck["last_type"]),
                                i64(ck["nhist"]), int(ck["step"]), i64(ck["swap_tries"]), i64(ck["swap_accepts"])))
        if ck.get("invtemps") is not None:   # an evolving run: set_evolve_temps first, then the ladders as they were
            self.set_invtemps(ck["invtemps"])
        h = ck.get("history")
        if h is not None and self.hist_rungs:
            meta = np.ascontiguousarray(np.stack([h["naccept"], h["ntries"], h["last_type"], h["row"]], axis=-1), dtype=np.int32)
            _chk(self.L.ptm_set_history(self.h, f64(h["x"]), f64(h["llike"]), f64(h["lprior"]), meta.ctypes.data_as(_i32p),
                                        f64(h["invtemp"])))
        m = ck.get("map")
        if m is not None and self.map_rungs:
            _chk(self.L.ptm_set_map(self.h, f64(m["x"]), f64(m["lpost"]), f64(m["llike"]), f64(m["lprior"])))

    def history(self):
        """dict of arrays [cap][history_rungs*W](,D): x, llike, lprior, naccept, ntries, last_type, row (saved row number,
        -1 = empty slot), invtemp (the temperature the row was saved at); saved row s of a chain sits in slot s % cap"""
        n = self.hist_cap * self.hist_rungs * self.W
        X = self._out(np.empty((n, self.D))); ll = self._out(np.empty(n)); lp = self._out(np.empty(n)); meta = self._out(np.empty((n, 4), dtype=np.int32))
        _chk(self.L.ptm_get_history(self.h, X.ctypes.data_as(_dp), ll.ctypes.data_as(_dp), lp.ctypes.data_as(_dp),
                                    meta.ctypes.data_as(_i32p)))
        sh = (self.hist_cap, self.hist_rungs * self.W)
        b = self._out(np.empty(n))
        _chk(self.L.ptm_get_history_invtemps(self.h, b.ctypes.data_as(_dp)))
        m = meta.reshape(sh + (4,))   # (views, not copies: inside a batch() the arrays are filled later)
        return dict(x=X.reshape(sh + (self.D,)), llike=ll.reshape(sh), lprior=lp.reshape(sh), naccept=m[..., 0],
                    ntries=m[..., 1], last_type=m[..., 2], row=m[..., 3], invtemp=b.reshape(sh))

    def ess_windowed(self, rung=0, nfeat=None, width=40000, every=100, burn=2):
        """one pass of the effective-sample-size estimator with fixed windows over the saved history of local rung `rung`, every
        walker at once, on the device: (ess[W], nwin[W]) (ptm_ess_windowed); nfeat: the first parameters looked at (None: all)"""
        ess, nwin = np.empty(self.W), np.empty(self.W, dtype=np.int32)
        _chk(self.L.ptm_ess_windowed(self.h, int(rung), self.D if nfeat is None else int(nfeat), int(width), int(every), int(burn), _d(ess),
                                     nwin.ctypes.data_as(_i32p)))
        return ess, nwin

    def effective_samples(self, rung=0, nfeat=None, width=40000, every=100, esslimit=-1):
        """chain::report_effective_samples of every walker's chain on local rung `rung`, from the history ring, on the device:
        (ess[W], useful length[W]) (ptm_ess_report)"""
        ess, length = np.empty(self.W), np.empty(self.W, dtype=np.int32)
        _chk(self.L.ptm_ess_report(self.h, int(rung), self.D if nfeat is None else int(nfeat), int(width), int(every), float(esslimit), _d(ess),
                                   length.ctypes.data_as(_i32p)))
        return ess, length

    @property
    def ess_last_on_device(self):
        """the last ess_windowed / effective_samples call ran the device kernels (ptm_ess_last_on_device)"""
        return bool(self.L.ptm_ess_last_on_device(self.h))

    def log_evidence(self, ilen, out=None):
        """log-evidence of every walker's ladder by thermodynamic integration over the last `ilen` steps of each chain's saved llikes,
        on the device (ptm_log_evidence): (log_evidence[W], up[Nt-1][W], down[Nt-1][W], count[Nt][W]).  out: arrays to fill instead
        (they keep their contents when the call fails)."""
        if out is None:
            out = (np.empty(self.W), np.empty((self.Nt - 1, self.W)), np.empty((self.Nt - 1, self.W)), np.empty((self.Nt, self.W), dtype=np.int32))
        ev, up, down, count = out
        _chk(self.L.ptm_log_evidence(self.h, int(ilen), _d(ev), _d(up), _d(down), count.ctypes.data_as(_i32p)))
        return ev, up, down, count

    def split_rhat(self, rung=0, nfeat=None, nrows=None, sequences=False, out=None):
        """split R-hat across the walkers of local rung `rung`, from the history ring, on the device: every walker's newest `nrows`
        saved rows (even, >= 4; None: the largest even window every walker of the rung still has), their halves the 2 W sequences:
        (rhat, mean, within, between)[nfeat]; sequences=True adds (seq_mean, seq_var)[2 W, nfeat] (ptm_rhat).  out: arrays to fill
        instead (they keep their contents when the call fails)."""
        nf = self.D if nfeat is None else int(nfeat)
        if nrows is None:
            if not (0 <= int(rung) < self.hist_rungs):
                raise PtmError("rung %d keeps no history (history_rungs = %d)" % (rung, self.hist_rungs))
            nh = self.nhist.reshape(self.nloc, self.W)[int(rung)].astype(np.int64)
            newest = np.where(nh > 0, 1 + (nh - 1) // self.add_every_n, 0)    # = the saved rows behind the start state
            have = min(int(newest.min()), self.hist_cap)                       # (a wrapped ring holds its newest `capacity` rows)
            nrows = have - have % 2
        o = _rhat_outputs(2 * self.W, max(nf, 0), sequences, out)
        p = [_d(v) for v in o] + [None] * (6 - len(o))
        _chk(self.L.ptm_rhat(self.h, int(rung), nf, int(nrows), *p))
        return o

    def posterior_moments(self, rung=0, nfeat=None, nrows=None, walker_sums=False, out=None, cov=None):
        """pooled mean and covariance of the first `nfeat` parameters over the walkers of local rung `rung`, from the history ring, on
        the device: every walker's newest `nrows` saved rows (None: the largest window every walker of the rung still has):
        (mean[nfeat], cov[nfeat, nfeat], var[nfeat], N) (ptm_moments).  cov=False (None: above 128 features, where no covariance is
        offered): cov is None.  walker_sums=True adds the walkers' sums [W, nfeat] in front of N.  out: arrays to fill instead,
        (mean, cov or None, var[, walker_sum]) (they keep their contents when the call fails)."""
        nf = self.D if nfeat is None else int(nfeat)
        if nrows is None:
            if not (0 <= int(rung) < self.hist_rungs):
                raise PtmError("rung %d keeps no history (history_rungs = %d)" % (rung, self.hist_rungs))
            nh = self.nhist.reshape(self.nloc, self.W)[int(rung)].astype(np.int64)
            newest = np.where(nh > 0, 1 + (nh - 1) // self.add_every_n, 0)    # = the saved rows behind the start state
            nrows = min(int(newest.min()), self.hist_cap)                      # (a wrapped ring holds its newest `capacity` rows)
        if cov is None:
            cov = nf <= 128
        o = _moments_outputs(self.W, max(nf, 0), cov, walker_sums, out)
        return _moments_call(self.L.ptm_moments, (self.h, int(rung), nf, int(nrows)), o)

    def posterior_quantiles(self, probs, rung=0, nfeat=None, nrows=None, brackets=False, out=None):
        """exact quantiles of the first `nfeat` parameters pooled over the walkers of local rung `rung`, from the history ring, on the
        device: every walker's newest `nrows` saved rows (None: the largest window every walker of the rung still has), at the
        probabilities `probs` (numpy's linear rule): (q[nq, nfeat], N); brackets=True: (q, x_lo, x_hi, N) with the two order
        statistics each quantile lies between (ptm_quantiles).  out: arrays to fill instead, (q[, x_lo, x_hi]) (they keep their
        contents when the call fails)."""
        nf = self.D if nfeat is None else int(nfeat)
        if nrows is None:
            if not (0 <= int(rung) < self.hist_rungs):
                raise PtmError("rung %d keeps no history (history_rungs = %d)" % (rung, self.hist_rungs))
            nh = self.nhist.reshape(self.nloc, self.W)[int(rung)].astype(np.int64)
            newest = np.where(nh > 0, 1 + (nh - 1) // self.add_every_n, 0)    # = the saved rows behind the start state
            nrows = min(int(newest.min()), self.hist_cap)                      # (a wrapped ring holds its newest `capacity` rows)
        return _quantiles_call(self.L.ptm_quantiles, (self.h, int(rung), nf, int(nrows)), probs, max(nf, 0), brackets, out)

    def posterior_histograms(self, lo, hi, nbins=20, rung=0, nfeat=None, nrows=None, pairs=True, out=None):
        """the corner plot's counts of the first `nfeat` parameters pooled over the walkers of local rung `rung`, from the history
        ring, on the device: every walker's newest `nrows` saved rows (None: the largest window every walker of the rung still has):
        (h1[nfeat, nbins], h2[npairs, nbins, nbins] or None, below[nfeat], above[nfeat], N), int64; the bins of feature f are
        histogram_edges(lo[f], hi[f], nbins), the last one closed (np.histogram's counts), the pairs i < j in row-major order
        (np.histogram2d's counts); pairs=False: no h2 (ptm_histograms).  out: arrays to fill instead, (h1, h2 or None, below, above)
        (they keep their contents when the call fails)."""
        nf = self.D if nfeat is None else int(nfeat)
        if nrows is None:
            if not (0 <= int(rung) < self.hist_rungs):
                raise PtmError("rung %d keeps no history (history_rungs = %d)" % (rung, self.hist_rungs))
            nh = self.nhist.reshape(self.nloc, self.W)[int(rung)].astype(np.int64)
            newest = np.where(nh > 0, 1 + (nh - 1) // self.add_every_n, 0)    # = the saved rows behind the start state
            nrows = min(int(newest.min()), self.hist_cap)                      # (a wrapped ring holds its newest `capacity` rows)
        return _histograms_call(self.L.ptm_histograms, (self.h, int(rung), nf, int(nrows)), lo, hi, nbins, max(nf, 0), pairs, out)

    def _common_window(self, first_rung, n_rungs):
        """the largest window every walker of every rung of the range still has (posterior_moments' rule)"""
        if not (0 <= first_rung and n_rungs >= 1 and first_rung + n_rungs <= self.hist_rungs):
            raise PtmError("rungs %d .. %d are not all recorded (history_rungs = %d)" % (first_rung, first_rung + n_rungs - 1, self.hist_rungs))
        nh = self.nhist.reshape(self.nloc, self.W)[first_rung:first_rung + n_rungs].astype(np.int64)
        newest = np.where(nh > 0, 1 + (nh - 1) // self.add_every_n, 0)    # = the saved rows behind the start state
        return min(int(newest.min()), self.hist_cap)                      # (a wrapped ring holds its newest `capacity` rows)

    def moments_rungs(self, first_rung=0, n_rungs=None, nfeat=None, nrows=None, cov=None):
        """posterior_moments for the local rungs first_rung .. first_rung + n_rungs - 1 (None: up to the last recorded rung) with one
        wait and every rung's bits (ptm_moments_rungs): (mean[n_rungs, nfeat], cov[n_rungs, nfeat, nfeat] or None, var[n_rungs, nfeat],
        N).  nrows None: the largest window every walker of every rung of the range still has."""
        first_rung = int(first_rung)
        nr = self.hist_rungs - first_rung if n_rungs is None else int(n_rungs)
        nf = self.D if nfeat is None else int(nfeat)
        if nrows is None:
            nrows = self._common_window(first_rung, nr)
        if cov is None:
            cov = nf <= 128
        m, k = max(nr, 0), max(nf, 0)
        o = (np.empty((m, k)), np.empty((m, k, k)) if cov else None, np.empty((m, k)))
        count = C.c_int64(0)
        _chk(self.L.ptm_moments_rungs(self.h, first_rung, nr, nf, int(nrows), *[None if v is None else _d(v) for v in o], C.byref(count)))
        return o + (int(count.value),)

    def adapt_proposals(self, nrows=None, scale=None, first_rung=0, n_rungs=None, factors=False):
        """every rung's Gaussian factor replaced by scale * (the eigen factor of its own pooled covariance) -- DIAG: scale * sqrt(var) --
        over every walker's newest `nrows` saved rows, on the device (ptm_adapt_proposals).  scale None: 2.38 / sqrt(D); nrows None: the
        largest window every walker of every rung of the range still has.  Returns status[n_rungs] (0 installed, 1 kept: not finite, 2 kept:
        not positive definite); factors=True: (status, factors[n_rungs, D, D] or [n_rungs, D]), what was computed, kept rungs included."""
        first_rung = int(first_rung)
        nr = self.hist_rungs - first_rung if n_rungs is None else int(n_rungs)
        if nrows is None:
            nrows = self._common_window(first_rung, nr)
        if scale is None:
            scale = 2.38 / np.sqrt(self.D)
        status = np.zeros(max(nr, 0), dtype=np.int32)
        f = None
        if factors:
            if self.prop_kind is None:
                raise PtmError("adapt_proposals(factors=True): the kind of the factors is not known (call Engine.set_proposals first)")
            f = np.empty((max(nr, 0), self.D) if self.prop_kind == PROP_DIAG else (max(nr, 0), self.D, self.D))
        _chk(self.L.ptm_adapt_proposals(self.h, first_rung, nr, int(nrows), float(scale), status.ctypes.data_as(_i32p), None if f is None else _d(f)))
        return (status, f) if factors else status

    @property
    def exchange_row_capacity(self):
        return self.L.ptm_exchange_row_capacity(self.h)

    def exchange_finish_and_sweep(self, recv_below_dev, recv_above_dev):
        _chk(self.L.ptm_exchange_finish_and_sweep(self.h, recv_below_dev, recv_above_dev))

    # -- read-back
    def batch(self):
        """context manager: the reads inside only queue their copies; the arrays they returned are filled when the block ends
        (ptm_batch_begin / ptm_batch_end: one wait on the device for all of them).  Keep the returned arrays alive until then."""
        eng = self
        class _Batch:
            def __enter__(self):
                _chk(eng.L.ptm_batch_begin(eng.h))
                eng._batch_depth += 1
            def __exit__(self, *exc):
                try:
                    _chk(eng.L.ptm_batch_end(eng.h))
                finally:
                    eng._batch_depth -= 1
                    if eng._batch_depth == 0:
                        eng._batch_keep.clear()     # the outputs are filled: temporaries may go now
                return False
        return _Batch()

    def _out(self, arr):
        """inside a batch() the C side fills an output when the bracket ends: hold a reference to every array handed out until
        then, so that a temporary (eng.naccept.sum()) or a discarded return value is not freed under the pending write"""
        if self._batch_depth > 0:
            self._batch_keep.append(arr)
        return arr

    def states(self):
        X = self._out(np.empty((self.Nc, self.D)))
        _chk(self.L.ptm_get_states(self.h, _d(X)))
        return X

    def array(self, which):
        dt = {ARR_LLIKE: np.float64, ARR_LPRIOR: np.float64, ARR_LPOST: np.float64, ARR_NTRIES: np.int32,
              ARR_NACCEPT: np.int32, ARR_LAST_TYPE: np.int32, ARR_NHIST: np.int64, ARR_NSIZE: np.int64, ARR_ROW_LABELS: np.int32}[which]
        out = self._out(np.empty(self.Nc, dtype=dt))
        _chk(self.L.ptm_get_array(self.h, which, out.ctypes.data_as(C.c_void_p)))
        return out

    llike = property(lambda s: s.array(ARR_LLIKE))
    lprior = property(lambda s: s.array(ARR_LPRIOR))
    lpost = property(lambda s: s.array(ARR_LPOST))
    ntries = property(lambda s: s.array(ARR_NTRIES))
    naccept = property(lambda s: s.array(ARR_NACCEPT))
    last_type = property(lambda s: s.array(ARR_LAST_TYPE))
    nhist = property(lambda s: s.array(ARR_NHIST))
    nsize = property(lambda s: s.array(ARR_NSIZE))
    row_labels = property(lambda s: s.array(ARR_ROW_LABELS))   # debug: rung slot holding each chain's row (identity once the states were read)

    def swap_counts(self):
        n = self.W * max(self.Nt - 1, 1)
        t, a = self._out(np.empty(n, dtype=np.int64)), self._out(np.empty(n, dtype=np.int64))
        _chk(self.L.ptm_get_swap_counts(self.h, t.ctypes.data_as(_i64p), a.ctypes.data_as(_i64p)))
        return t.reshape(self.W, -1), a.reshape(self.W, -1)

    def last_swaps(self):
        ms = self.max_swaps
        p, a = self._out(np.empty(self.W * ms, dtype=np.int32)), self._out(np.empty(self.W * ms, dtype=np.int32))
        _chk(self.L.ptm_get_last_swaps(self.h, p.ctypes.data_as(_i32p), a.ctypes.data_as(_i32p)))
        return p.reshape(self.W, ms), a.reshape(self.W, ms)

    @property
    def max_swaps(self):
        return self.L.ptm_max_swaps_per_step(self.h)

    @property
    def step_count(self):
        return int(self.L.ptm_step_count(self.h))

    def debug_evaluate(self, X):
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, self.D)
        n = X.shape[0]
        valid = np.empty(n, dtype=np.int32); Xe = np.empty_like(X); lp = np.empty(n); ll = np.full(n, np.nan)
        _chk(self.L.ptm_debug_evaluate(self.h, _d(X), n, valid.ctypes.data_as(_i32p), _d(Xe), _d(lp), _d(ll)))
        return valid, Xe, lp, ll

    # -- measurement
    def timer_start(self):
        _chk(self.L.ptm_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        _chk(self.L.ptm_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def kernel_times(self, capacity=1 << 16, drop=False):
        """per-launch durations (ms) of the sweep kernel since the last call; drop=True: forget them unread (no event queries)"""
        n = C.c_int()
        if drop:
            _chk(self.L.ptm_get_kernel_times(self.h, None, 0, C.byref(n)))
            return np.zeros(0)
        buf = (C.c_float * capacity)()
        _chk(self.L.ptm_get_kernel_times(self.h, buf, capacity, C.byref(n)))
        return np.array(buf[:min(n.value, capacity)], dtype=np.float64)

    def ladder_stats(self):
        """persistent ladder kernel: launches, launches that gave up (repeated on the two-launch path), whole-ladder steps, switched off"""
        o = (C.c_int64 * 4)()
        _chk(self.L.ptm_get_ladder_stats(self.h, o))
        return dict(launches=o[0], fallbacks=o[1], whole_steps=o[2], disabled=bool(o[3]))

    def counter_sums(self):
        """(sum of MH_chain::Ntries, sum of ::Naccept) over the engine's chains, reduced on the device (ptm_get_counter_sums)"""
        t, a = C.c_int64(), C.c_int64()
        _chk(self.L.ptm_get_counter_sums(self.h, C.byref(t), C.byref(a)))
        return t.value, a.value

    def prefilter_counts(self):
        """box pre-pass (ptm_get_prefilter_counts): chains it saw and chains it settled so far, local rungs flagged for it, whether a
        whole step's sweep of this engine is eligible for it"""
        o = (C.c_int64 * 4)()
        _chk(self.L.ptm_get_prefilter_counts(self.h, o))
        return dict(seen=o[0], settled=o[1], rungs_flagged=o[2], eligible=bool(o[3]))

    def calibrate(self):
        """what this device gives a streaming copy and an f64 fma loop right now (ptm_calibrate)"""
        c = PtmCalibration()
        _chk(self.L.ptm_calibrate(self.h, C.byref(c)))
        return {"copy_GBs": c.copy_GBs, "copy_bytes": c.copy_bytes, "copy_ms": c.copy_ms, "f64_fma_TFs": c.f64_fma_TFs,
                "fma_ms": c.fma_ms, "sclk_MHz": c.sclk_MHz, "compute_units": c.compute_units}

    @property
    def sweep_kernel_name(self):
        return self.L.ptm_sweep_kernel_name(self.h).decode()

    @property
    def step_kernel_name(self):
        """what step() launches (ptm_step_kernel_name)"""
        return self.L.ptm_step_kernel_name(self.h).decode()


def proposal_verdict(redraws, alt):
    """how the reference's proposal test judges a statistic (test_proposal.hh:311-343): the redraw values by magnitude, Ncut =
    int(sqrt(ntry)), the cut half way between sorted entries ntry - Ncut and ntry - Ncut - 1 (0 with one redraw):
    (cut, "PASS" if alt < cut else "FAIL")"""
    import math
    d = np.sort(np.abs(np.asarray(redraws, dtype=np.float64)))
    ntry = d.size
    ncut = int(math.sqrt(ntry))
    cut = float((d[ntry - ncut] + d[ntry - ncut - 1]) / 2.0) if ntry > 1 else 0.0
    return cut, "PASS" if alt < cut else "FAIL"


def proposal_invariance(dim, centre, sigma, install, nsamp=10000, ncyc=5, ntry=10, bounds=None, seed=0x5EED0001, min_accept=0.0, device=-1):
    """Does a proposal leave a known target invariant?  The reference's test_proposal::test (test_proposal.hh:202-348) on the engine:
    nsamp samples of the target -- a Gaussian per dimension (centre, sigma) on the space `bounds` = (lower types, upper types, xmin,
    xmax) or None, samples outside a limit redrawn -- are the walkers of a one-rung engine whose prior is that target over a
    constant likelihood; install(engine) sets the proposal under test (set_proposals, set_proposal_device, set_proposal_callback ...);
    sweeps are made until ncyc * nsamp moves have been accepted (after 2000 sweeps with under 1% of them the goal is halved, or the
    test gives up below min_accept: None is returned).  In a wrapped dimension the target must keep SEAM_SIGMAS sigma inside the domain
    (ValueError otherwise): the engine wraps a Gaussian's draws but evaluates the plain Gaussian, where the reference sums the images.  The transformed set is then compared with the target set and with a fresh
    draw by the k-NN KL estimate (exact neighbours, on the device) and the Gaussian fake KL, both calibrated on ntry and 30 ntry redraws.
    Returns a dict: kl, kl_x, fake_kl, fake_kl_x (transformed against the start set, and the other way round), alt_kl, alt_kl_x,
    alt_fake_kl, alt_fake_kl_x (against a fresh draw), kl_redraws, fake_kl_redraws, kl_cut, fake_kl_cut, kl_verdict, fake_kl_verdict,
    acceptance (of the last sweep), sweeps, ncyc, target, transformed."""
    if bounds is not None:   # a wrapped dimension: the engine wraps the Gaussian's draws but evaluates the plain Gaussian (no periodic sum)
        c, sg = np.asarray(centre, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
        for d in range(dim):
            if bounds[0][d] == BOUND_WRAP and bounds[1][d] == BOUND_WRAP and (c[d] - SEAM_SIGMAS * sg[d] < bounds[2][d] or c[d] + SEAM_SIGMAS * sg[d] > bounds[3][d]):
                raise ValueError("the target comes within %g sigma of the seam of wrapped dimension %d: its samples wrap around, the density the steps "
                                 "aim at does not; move the centre inside or shrink sigma" % (SEAM_SIGMAS, d))
    eng = Engine(dim, 1, nsamp, seed=seed, min_prior=-1e300, device=device)   # (min_prior: the prior gate never acts)
    try:
        wrap = None
        if bounds is not None:
            eng.set_bounds(*bounds)
            lo_t, hi_t, xmin, xmax = (np.asarray(v) for v in bounds)
            wrap = ((lo_t == BOUND_WRAP) & (hi_t == BOUND_WRAP)).astype(np.int32), xmin.astype(np.float64), xmax.astype(np.float64)
            if not wrap[0].any():
                wrap = None
        eng.set_prior(["gauss"] * dim, centre, sigma)
        eng.set_target_gaussian(np.zeros((dim, dim)), 0.0)
        eng.set_ladder([1.0])
        install(eng)
        eng.init_from_prior()
        target = eng.states().reshape(nsamp, dim).copy()
        goal, cum, icyc, sweeps, rate = int(ncyc * nsamp), 0, 1, 0, 0.0
        accepted = eng.counter_sums()[1]
        while cum < goal:
            eng.sweep(1)
            now = eng.counter_sums()[1]
            step, accepted = now - accepted, now
            cum, sweeps, rate = cum + step, sweeps + 1, step / nsamp
            if icyc == 2000 and cum < goal * 0.01:
                ncyc = ncyc / 2.0
                if rate < min_accept:
                    return None
                goal, icyc, cum = int(ncyc * nsamp), 0, 0
            icyc += 1
        transformed = eng.states().reshape(nsamp, dim).copy()
        fntry = 30 * ntry
        redraw = lambda k: eng.draw_prior_rows(1 + k, 1)[0].reshape(nsamp, dim)
        w = wrap or (None, None, None)
        kl = lambda a, b: kl_divergence(a, b, *w, device=device)
        out = dict(kl=kl(transformed, target), kl_x=kl(target, transformed), fake_kl=fake_kl_divergence(transformed, target),
                   fake_kl_x=fake_kl_divergence(target, transformed))
        out["kl_redraws"] = np.array([kl(redraw(k), target) for k in range(ntry)])
        out["fake_kl_redraws"] = np.array([fake_kl_divergence(redraw(ntry + k), target) for k in range(fntry)])
        alt = redraw(ntry + fntry)
        out.update(alt_kl=kl(transformed, alt), alt_kl_x=kl(alt, transformed), alt_fake_kl=fake_kl_divergence(transformed, alt),
                   alt_fake_kl_x=fake_kl_divergence(alt, transformed))
        out["kl_cut"], out["kl_verdict"] = proposal_verdict(out["kl_redraws"], out["alt_kl"])
        out["fake_kl_cut"], out["fake_kl_verdict"] = proposal_verdict(out["fake_kl_redraws"], out["alt_fake_kl"])
        out.update(acceptance=rate, sweeps=sweeps, ncyc=ncyc, target=target, transformed=transformed)
        return out
    finally:
        eng.close()
