"""ctypes binding of ``liboaxaca_boot.so`` (the C ABI declared in ``include/oaxaca_boot.h``).

The library is built in-tree by ``__graft_entry__.build()`` (``make -C csrc``). There is no
fallback: if the library is missing, or no MI355X is visible when a compute entry point is
called, the call raises -- the bootstrap never silently runs on the CPU.
"""
from __future__ import annotations

import contextlib
import math
import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# OB_LIB_PATH: an alternative build for A/B timing runs (tools/build_alt.sh); never set in tests.
LIB_PATH = os.environ.get("OB_LIB_PATH") or os.path.join(_HERE, "liboaxaca_boot.so")

OB_OK = 0
OB_E_POLARS, OB_E_COLUMN, OB_E_GROUP, OB_E_LINALG, OB_E_DIAG, OB_E_INSUFFICIENT = 1, 2, 3, 4, 5, 6
OB_E_HIP, OB_E_INVALID, OB_E_UNSUPPORTED, OB_E_OVERFLOW, OB_E_RCCL = 7, 8, 9, 10, 11

OB_COL_F64, OB_COL_I64, OB_COL_STR = 0, 1, 2
OB_TABLE_TWO_FOLD, OB_TABLE_DETAILED_EXPLAINED, OB_TABLE_DETAILED_UNEXPLAINED = 0, 1, 2
OB_TABLE_DETAILED_SELECTION, OB_TABLE_THREE_FOLD = 3, 4
OB_VEC_RESIDUALS, OB_VEC_XA_MEAN, OB_VEC_XB_MEAN, OB_VEC_BETA_STAR = 0, 1, 2, 3

OB_E_CONVERGENCE = 12
OB_LOGIT_MAX_K = 64  # include/oaxaca_boot.h
OB_RIFQ_MAX_K, OB_RIFQ_MAX_TAUS = 32, 8
OB_RIFS_MAX_STATS = 8
OB_HECKMAN_MAX_ZSEL = 31
OB_AKM_MAX_CONTROLS = 64
OB_VIF_MAX_K = 120
OB_REMEDY_MAX_K = 120  # design columns, the intercept included
OB_REMEDY_MAX_STEPS = 127
OB_JACK_MAX_K = 119  # design columns, the intercept included
OB_CLUSTER_JACK_MAX_K = 32  # design columns, the intercept included
OB_REMEDY_TARGETS = {"reference": 0, "pooled": 1}
OB_REMEDY_STRATEGIES = {"greedy": 0, "equitable": 1}
OB_REMEDY_RANGE_TARGETS = {"midpoint": 0, "lower": 1, "upper": 2}
OB_MATCH_MAX_DIM, OB_MATCH_MAX_K = 64, 16
OB_MATCH_EUCLIDEAN, OB_MATCH_MAHALANOBIS, OB_MATCH_PSM = 0, 1, 2
OB_RIF_VARIANCE, OB_RIF_GINI, OB_RIF_IQR = 0, 1, 2
OB_RIF_STATS = {"variance": OB_RIF_VARIANCE, "gini": OB_RIF_GINI, "iqr": OB_RIF_IQR}
OB_RIF_QUANTILE = 3  # the weighted entry points only
OB_RIF_WSTATS = {**OB_RIF_STATS, "quantile": OB_RIF_QUANTILE}
OB_REWEIGHT_MAX_STATS = 16
OB_BINARY_MAX_K = 32  # design columns, the intercept included
OB_BINARY_PROBIT, OB_BINARY_LOGIT = 0, 1
OB_BINARY_MODELS = {"probit": OB_BINARY_PROBIT, "logit": OB_BINARY_LOGIT}
OB_REWEIGHT_MAX_K = 32  # design columns, the intercept included
OB_RW_TABLE_AGGREGATE, OB_RW_TABLE_PURE_EXPLAINED, OB_RW_TABLE_SPECIFICATION_ERROR = 0, 1, 2
OB_RW_TABLE_PURE_UNEXPLAINED, OB_RW_TABLE_REWEIGHTING_ERROR = 3, 4
OB_DR_MAX_K, OB_DR_MAX_T, OB_DR_MAX_Q, OB_DR_MAX_VECTORS = 32, 64, 32, 128
OB_DR_TABLE_QUANTILE_EFFECTS, OB_DR_TABLE_QUANTILES, OB_DR_TABLE_DISTRIBUTION_EFFECTS, OB_DR_TABLE_CDF = 0, 1, 2, 3
OB_DENSITY_MAX_GRID, OB_DENSITY_MAX_VECTORS = 256, 64
OB_DENSITY_TABLE_CURVES, OB_DENSITY_TABLE_BANDS = 0, 1
OB_TOBIT_MAX_K, OB_TOBIT_MAX_PASSES, OB_TOBIT_MAX_ARRAY_REPS = 31, 100, 1024
OB_TOBIT_DONE, OB_TOBIT_FAILED = 1, 2
OB_TOBIT_TABLE_LATENT = 3


class OaxacaError(RuntimeError):
    """Raised for any non-OB_OK return; ``code`` is the OB_E_* value (error.rs variants)."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code


class ob_group_desc(C.Structure):
    _fields_ = [("n", C.c_int64), ("x", C.POINTER(C.c_double)), ("ldx", C.c_int64),
                ("y", C.POINTER(C.c_double)), ("w", C.POINTER(C.c_double))]


class ob_panel_desc(C.Structure):
    _fields_ = [("p", C.c_int32), ("n_num", C.c_int32), ("weighted", C.c_int32),
                ("a", ob_group_desc), ("b", ob_group_desc), ("n_norm", C.c_int32),
                ("norm_start", C.POINTER(C.c_int32)), ("norm_idx", C.POINTER(C.c_int32)),
                ("norm_m", C.POINTER(C.c_int32)), ("pooled_start", C.POINTER(C.c_int32)),
                ("pooled_idx", C.POINTER(C.c_int32)), ("has_base", C.POINTER(C.c_int32)),
                ("n_y", C.c_int32), ("heckman", C.c_int32), ("n_zsel", C.c_int32),
                ("za", C.POINTER(C.c_double)), ("zb", C.POINTER(C.c_double)),
                ("sa", C.POINTER(C.c_double)), ("sb", C.POINTER(C.c_double))]


class ob_timing(C.Structure):
    _fields_ = [("level1_ms", C.c_double), ("gram_ms", C.c_double), ("reduce_ms", C.c_double),
                ("solve_ms", C.c_double), ("gram_launches", C.c_int32), ("chunks", C.c_int32),
                ("blocks", C.c_int32), ("counts_ms", C.c_double),
                ("heckman_ms", C.c_double), ("probit_iterations", C.c_int32),
                ("mm_assemble_ms", C.c_double), ("mm_fit_rows", C.c_double), ("mm_iterations", C.c_int32),
                ("mm_ms", C.c_double), ("gather_ms", C.c_double), ("gram_path", C.c_int32),
                ("probit_ms", C.c_double), ("probit_launches", C.c_int32), ("heck_sums_ms", C.c_double),
                ("mm_reduced", C.c_int32), ("mm_retried", C.c_int64), ("prep_ms", C.c_double),
                ("oz_exceptions", C.c_int32), ("oz_bits", C.c_int32), ("oz_tiles6", C.c_int32),
                ("oz_tiles", C.c_int32), ("oz_wide", C.c_int32)]


class ob_unique_id(C.Structure):
    _fields_ = [("internal", C.c_uint8 * 128)]  # raw bytes (a c_char array would stop at NUL)


class ob_column(C.Structure):
    _fields_ = [("name", C.c_char_p), ("kind", C.c_int32), ("f64", C.POINTER(C.c_double)),
                ("i64", C.POINTER(C.c_int64)), ("str", C.POINTER(C.c_char_p)),
                ("valid", C.POINTER(C.c_uint8))]


class ob_builder_config(C.Structure):
    _fields_ = [("outcome", C.c_char_p), ("group", C.c_char_p), ("reference_group", C.c_char_p),
                ("predictors", C.POINTER(C.c_char_p)), ("n_predictors", C.c_int32),
                ("categorical", C.POINTER(C.c_char_p)), ("n_categorical", C.c_int32),
                ("normalize", C.POINTER(C.c_char_p)), ("n_normalize", C.c_int32),
                ("weights", C.c_char_p), ("selection_outcome", C.c_char_p),
                ("bootstrap_reps", C.c_uint64), ("reference_coeffs", C.c_int32),
                ("has_seed", C.c_int32), ("seed", C.c_uint64),
                ("selection_predictors", C.POINTER(C.c_char_p)), ("n_selection_predictors", C.c_int32)]


class ob_qd_config(C.Structure):
    _fields_ = [("outcome", C.c_char_p), ("group", C.c_char_p), ("reference_group", C.c_char_p),
                ("predictors", C.POINTER(C.c_char_p)), ("n_predictors", C.c_int32),
                ("categorical", C.POINTER(C.c_char_p)), ("n_categorical", C.c_int32),
                ("quantiles", C.POINTER(C.c_double)), ("n_quantiles", C.c_int32),
                ("simulations", C.c_int32), ("bootstrap_reps", C.c_uint64),
                ("has_seed", C.c_int32), ("seed", C.c_uint64)]


class ob_dfl_config(C.Structure):
    _fields_ = [("outcome", C.c_char_p), ("group", C.c_char_p), ("reference_group", C.c_char_p),
                ("predictors", C.POINTER(C.c_char_p)), ("n_predictors", C.c_int32), ("grid_size", C.c_int32)]


class ob_dfl_info(C.Structure):
    _fields_ = [("n_a", C.c_int64), ("n_b", C.c_int64), ("logit_iterations", C.c_int32),
                ("logit_converged", C.c_int32), ("bandwidth_a", C.c_double), ("bandwidth_b", C.c_double),
                ("group_a", C.c_char_p), ("logit_ms", C.c_double), ("kde_ms", C.c_double)]


class ob_match_config(C.Structure):
    _fields_ = [("treatment", C.c_char_p), ("outcome", C.c_char_p), ("covariates", C.POINTER(C.c_char_p)),
                ("n_covariates", C.c_int32), ("k", C.c_int32), ("method", C.c_int32)]


class ob_match_info(C.Structure):
    _fields_ = [("n_treated", C.c_int64), ("n_control", C.c_int64), ("logistic_iterations", C.c_int32),
                ("logistic_converged", C.c_int32), ("knn_ms", C.c_double), ("prep_ms", C.c_double)]


class ob_akm_config(C.Structure):
    _fields_ = [("outcome", C.c_char_p), ("worker_col", C.c_char_p), ("firm_col", C.c_char_p),
                ("controls", C.POINTER(C.c_char_p)), ("n_controls", C.c_int32), ("tolerance", C.c_double),
                ("max_iters", C.c_int64)]


class ob_akm_info(C.Structure):
    _fields_ = [("n_rows_kept", C.c_int64), ("n_workers", C.c_int64), ("n_firms", C.c_int64),
                ("n_components", C.c_int64), ("demean_iterations", C.POINTER(C.c_int32)), ("n_demean", C.c_int32),
                ("recover_iterations", C.c_int32), ("launches_per_iteration", C.c_int32),
                ("demean_ms", C.c_double), ("ols_ms", C.c_double), ("recover_ms", C.c_double)]


class ob_remedy_request(C.Structure):
    _fields_ = [("budget", C.c_double), ("min_gap_pct", C.c_double), ("confidence_level", C.c_double),
                ("strategy", C.c_int32), ("range_target", C.c_int32), ("forensic_mode", C.c_int32),
                ("adjust_both_groups", C.c_int32)]


class ob_remedy_info(C.Structure):
    _fields_ = [("n_a", C.c_int64), ("n_b", C.c_int64), ("n_adjustments", C.c_int64),
                ("total_cost", C.c_double), ("required_budget", C.c_double), ("effective_budget", C.c_double),
                ("net_residual_sum_b", C.c_double), ("original_unexplained_gap", C.c_double),
                ("new_unexplained_gap", C.c_double), ("z_score", C.c_double), ("sigma_squared", C.c_double),
                ("classify_ms", C.c_double), ("order_ms", C.c_double), ("allocate_ms", C.c_double),
                ("original_gap", C.c_double), ("new_gap", C.c_double), ("gram_ms", C.c_double),
                ("score_ms", C.c_double)]


class ob_defend_info(C.Structure):
    _fields_ = [("n_a", C.c_int64), ("n_b", C.c_int64), ("n_adjustments", C.c_int64), ("n_skipped", C.c_int64),
                ("total_cost", C.c_double), ("original_gap", C.c_double), ("new_gap", C.c_double),
                ("original_unexplained_gap", C.c_double), ("new_unexplained_gap", C.c_double),
                ("required_budget", C.c_double), ("z_score", C.c_double), ("sigma_squared", C.c_double),
                ("gram_ms", C.c_double), ("score_ms", C.c_double), ("defend_ms", C.c_double),
                ("scatter_ms", C.c_double), ("adjust_ms", C.c_double), ("rows_ms", C.c_double),
                ("sums", C.c_double * 7)]


class ob_jackknife_out(C.Structure):
    _fields_ = [("capacity", C.c_int32), ("n_components", C.c_int32), ("n_used", C.c_int64 * 2),
                ("n_dropped", C.c_int64 * 2), ("point", C.POINTER(C.c_double)), ("sums", C.POINTER(C.c_double)),
                ("stats", C.POINTER(C.c_double))]


class ob_cluster_config(C.Structure):
    _fields_ = [("column", C.c_char_p), ("stratified", C.c_int32)]


class ob_cluster_info(C.Structure):
    _fields_ = [("n_clusters", C.c_int64), ("n_clusters_a", C.c_int64), ("n_clusters_b", C.c_int64),
                ("max_cluster_rows", C.c_int64), ("stratified", C.c_int32)]


class ob_cluster_timing(C.Structure):
    _fields_ = [("gram_ms", C.c_double), ("counts_ms", C.c_double), ("apply_ms", C.c_double),
                ("solve_ms", C.c_double)]


class ob_rif_spec(C.Structure):
    _fields_ = [("stat", C.c_int32), ("p0", C.c_double), ("p1", C.c_double)]


class ob_rif_timing(C.Structure):
    _fields_ = [("sort_ms", C.c_double), ("scan_ms", C.c_double), ("kde_ms", C.c_double),
                ("scatter_ms", C.c_double)]


class ob_binary_timing(C.Structure):
    _fields_ = [("probit_ms", C.c_double), ("probit_launches", C.c_int32), ("probit_iterations", C.c_int32),
                ("means_ms", C.c_double), ("epilogue_ms", C.c_double)]


class ob_reweight_timing(C.Structure):
    _fields_ = [("logit_passes", C.c_int32), ("logit_launches", C.c_int32), ("logit_ms", C.c_double),
                ("gram_ms", C.c_double), ("row_ms", C.c_double)]


class ob_dr_config(C.Structure):
    _fields_ = [("thresholds", C.POINTER(C.c_double)), ("n_thresholds", C.c_int32), ("lo", C.c_double),
                ("hi", C.c_double), ("quantiles", C.POINTER(C.c_double)), ("n_quantiles", C.c_int32)]


class ob_dr_timing(C.Structure):
    _fields_ = [("passes", C.c_int32), ("launches", C.c_int32), ("pass_ms", C.c_double), ("cdf_ms", C.c_double),
                ("row_ms", C.c_double)]


class ob_rifq_timing(C.Structure):
    _fields_ = [("search_ms", C.c_double), ("density_ms", C.c_double), ("patch_ms", C.c_double),
                ("gram_ms", C.c_double), ("solve_ms", C.c_double)]


class ob_rifs_timing(C.Structure):
    _fields_ = [("moment_ms", C.c_double), ("scan_ms", C.c_double), ("gini_ms", C.c_double), ("tie_ms", C.c_double),
                ("finish_ms", C.c_double), ("gram_ms", C.c_double), ("solve_ms", C.c_double), ("rifq_ms", C.c_double)]


class ob_rifs_info(C.Structure):
    _fields_ = [("n_specs", C.c_int32), ("k", C.c_int32), ("n_a", C.c_int64), ("n_b", C.c_int64),
                ("n_density_floored", C.c_int64), ("specs", C.POINTER(ob_rif_spec)), ("perm_a", C.POINTER(C.c_int32)),
                ("perm_b", C.POINTER(C.c_int32)), ("nu", C.POINTER(C.c_double))]


class ob_rifq_info(C.Structure):
    _fields_ = [("n_taus", C.c_int32), ("k", C.c_int32), ("n_a", C.c_int64), ("n_b", C.c_int64),
                ("n_density_floored", C.c_int64), ("taus", C.POINTER(C.c_double)), ("perm_a", C.POINTER(C.c_int32)),
                ("perm_b", C.POINTER(C.c_int32)), ("q", C.POINTER(C.c_double)), ("f", C.POINTER(C.c_double))]


class ob_dr_info(C.Structure):
    _fields_ = [("n_thresholds", C.c_int32), ("n_quantiles", C.c_int32), ("k", C.c_int32), ("n_requested", C.c_int32),
                ("n_out_of_range", C.c_int32), ("thresholds", C.POINTER(C.c_double)),
                ("quantiles", C.POINTER(C.c_double)), ("beta", C.POINTER(C.c_double)),
                ("passes", C.POINTER(C.c_int32)), ("out_of_range", C.POINTER(C.c_uint8))]


class ob_nopo_timing(C.Structure):
    _fields_ = [("cell_ms", C.c_double), ("row_ms", C.c_double), ("counts_ms", C.c_double)]


class ob_nopo_info(C.Structure):
    _fields_ = [("n_cells", C.c_int32), ("n_support_cells", C.c_int32), ("n_rows", C.c_int64), ("n_a", C.c_int64),
                ("n_b", C.c_int64), ("n_cell_a", C.POINTER(C.c_int64)), ("n_cell_b", C.POINTER(C.c_int64)),
                ("w_a", C.POINTER(C.c_double)), ("w_b", C.POINTER(C.c_double)), ("mean_a", C.POINTER(C.c_double)),
                ("mean_b", C.POINTER(C.c_double)), ("in_support", C.POINTER(C.c_uint8)),
                ("row_cell", C.POINTER(C.c_int32))]


class ob_density_config(C.Structure):
    _fields_ = [("grid_size", C.c_int32), ("grid", C.POINTER(C.c_double)), ("bandwidth_a", C.c_double),
                ("bandwidth_b", C.c_double)]


class ob_density_timing(C.Structure):
    _fields_ = [("logit_passes", C.c_int32), ("logit_launches", C.c_int32), ("logit_ms", C.c_double),
                ("density_ms", C.c_double), ("finish_ms", C.c_double)]


class ob_density_info(C.Structure):
    _fields_ = [("grid_size", C.c_int32), ("k", C.c_int32), ("grid", C.POINTER(C.c_double)),
                ("bandwidth_a", C.c_double), ("bandwidth_b", C.c_double), ("n_a", C.c_int64), ("n_b", C.c_int64)]


class ob_tobit_config(C.Structure):
    _fields_ = [("lower", C.c_double), ("upper", C.c_double), ("has_lower", C.c_int32), ("has_upper", C.c_int32)]


class ob_tobit_timing(C.Structure):
    _fields_ = [("passes", C.c_int32), ("pass_launches", C.c_int32), ("pass_ms", C.c_double),
                ("means_ms", C.c_double), ("row_ms", C.c_double)]


class ob_tobit_info(C.Structure):
    _fields_ = [("k", C.c_int32), ("has_lower", C.c_int32), ("has_upper", C.c_int32), ("passes_a", C.c_int32),
                ("passes_b", C.c_int32), ("lower", C.c_double), ("upper", C.c_double), ("n_a", C.c_int64),
                ("n_b", C.c_int64), ("n_left_a", C.c_int64), ("n_right_a", C.c_int64), ("n_left_b", C.c_int64),
                ("n_right_b", C.c_int64), ("eta", C.POINTER(C.c_double))]


class ob_component(C.Structure):
    _fields_ = [("name", C.c_char_p), ("estimate", C.c_double), ("std_err", C.c_double),
                ("t_stat", C.c_double), ("p_value", C.c_double), ("ci_lower", C.c_double),
                ("ci_upper", C.c_double)]


_P = C.c_void_p
_D = C.POINTER(C.c_double)
_U8 = C.POINTER(C.c_uint8)
_H = C.POINTER(_P)  # a handle out parameter
# the prefix of every entry point that takes a frame: ctx, cols, n_cols, n_rows (then the builder's config)
_FRAME = [_P, C.POINTER(ob_column), C.c_int32, C.c_int64]
_FRAME_CFG = _FRAME + [C.POINTER(ob_builder_config)]
_TOBIT = C.POINTER(ob_tobit_config)
_CLUSTER = C.POINTER(ob_cluster_config)
_SPEC = C.POINTER(ob_rif_spec)
_SIGS = {
    "ob_last_error": (C.c_char_p, []),
    "ob_version": (C.c_char_p, []),
    "ob_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "ob_ctx_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "ob_ctx_destroy": (None, [_P]),
    "ob_panel_create": (C.c_int, [_P, C.POINTER(ob_panel_desc), C.POINTER(_P)]),
    "ob_panel_destroy": (None, [_P]),
    "ob_panel_row_len": (C.c_int, [_P]),
    "ob_panel_k": (C.c_int, [_P]),
    "ob_panel_n_base": (C.c_int, [_P]),
    "ob_panel_n_y": (C.c_int, [_P]),
    "ob_point_estimate": (C.c_int, [_P, C.c_int, _D, _D]),
    "ob_boot_run": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _D, _U8]),
    "ob_boot_run_device": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _P, _P, _P]),
    "ob_panel_last_timing": (C.c_int, [_P, C.POINTER(ob_timing)]),
    "ob_panel_sync": (C.c_int, [_P]),
    "ob_bootstrap_stats": (C.c_int, [_D, C.c_int64, C.c_double, _D]),
    "ob_aggregate": (C.c_int, [_D, _U8, C.c_uint64, C.c_int32, C.POINTER(C.c_int32), C.c_int32, _D]),
    "ob_rif": (C.c_int, [_D, C.c_int64, C.c_double, _D]),
    "ob_builder_prepare": (C.c_int, _FRAME_CFG + [_H]),
    "ob_prepared_row_len": (C.c_int, [_P]),
    "ob_prepared_n_y": (C.c_int, [_P]),
    "ob_prepared_seed": (C.c_uint64, [_P]),
    "ob_prepared_panel": (_P, [_P]),
    "ob_prepared_boot": (C.c_int, [_P, C.c_uint64, C.c_uint64, _D, _U8]),
    "ob_prepared_boot_device": (C.c_int, [_P, C.c_uint64, C.c_uint64, _P, _P, _P]),
    "ob_prepared_finish": (C.c_int, [_P, _D, _U8, C.c_uint64, C.POINTER(_P)]),
    "ob_prepared_destroy": (None, [_P]),
    "ob_builder_run": (C.c_int, _FRAME_CFG + [_H]),
    "ob_builder_decompose_quantile": (C.c_int, _FRAME_CFG + [C.c_double, _H]),
    "ob_builder_decompose_quantiles": (C.c_int, _FRAME_CFG + [_D, C.c_int32, _H]),
    "ob_builder_data_matrices": (C.c_int, _FRAME_CFG[1:] + [_H]),  # host only: no ctx
    "ob_csv_read": (C.c_int, [C.c_char_p, C.POINTER(_P)]),
    "ob_csv_dims": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "ob_csv_column": (C.c_int, [_P, C.c_int32, C.POINTER(ob_column)]),
    "ob_csv_free": (None, [_P]),
    "ob_results_total_gap": (C.c_double, [_P]),
    "ob_results_n_a": (C.c_int64, [_P]),
    "ob_results_n_b": (C.c_int64, [_P]),
    "ob_results_n_failed": (C.c_int64, [_P]),
    "ob_results_count": (C.c_int, [_P, C.c_int32]),
    "ob_results_component": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(ob_component)]),
    "ob_results_vector": (C.c_int, [_P, C.c_int32, C.POINTER(_D), C.POINTER(C.c_int64)]),
    "ob_results_free": (None, [_P]),
    "ob_matrices_dims": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "ob_matrices_get": (C.c_int, [_P, C.POINTER(_D), C.POINTER(_D), C.POINTER(_D), C.POINTER(_D)]),
    "ob_matrices_name": (C.c_char_p, [_P, C.c_int32]),
    "ob_matrices_free": (None, [_P]),
    "ob_mm_run": (C.c_int, [_P, C.c_uint64, C.c_int32, _D, C.c_int32, C.c_uint64, C.c_uint64, C.c_int32, _D, _U8]),
    "ob_quantile_decomposition_run": (C.c_int, _FRAME + [C.POINTER(ob_qd_config), _H]),
    "ob_qd_results_dims": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ob_qd_results_get": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(ob_component)]),
    "ob_qd_results_n_failed": (C.c_int64, [_P]),
    "ob_qd_results_free": (None, [_P]),
    "ob_get_unique_id": (C.c_int, [C.POINTER(ob_unique_id)]),
    "ob_ctx_create_rank": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(ob_unique_id), C.POINTER(_P)]),
    "ob_ctx_rank": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ob_boot_run_sharded": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _D, _U8]),
    "ob_boot_run_sharded_device": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _P, _P, _P]),
    "ob_boot_run_multi": (C.c_int, [C.POINTER(_P), C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _D, _U8]),
    "ob_debug_gram": (C.c_int, [_P, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, _D]),
    "ob_debug_mm_fail": (C.c_int, [_P, _U8, C.c_int32]),
    "ob_panel_set_gather_columns": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int32]),
    "ob_debug_shard_sim": (C.c_int, [_P, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _D, _U8]),
    "ob_debug_gram_exceptions": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                           C.POINTER(C.c_uint32), C.c_int32]),
    "ob_prepared_boot_sharded": (C.c_int, [_P, C.c_uint64, C.c_uint64, _D, _U8]),
    "ob_debug_counts": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), _U8]),
    "ob_debug_chunks": (C.c_int, [_P, C.POINTER(C.c_uint32), C.c_int32, C.POINTER(C.c_int32)]),
    "ob_debug_mm_betas": (C.c_int, [_P, C.c_uint64, C.c_int32, C.c_uint64, _D, _U8]),
    "ob_set_option": (C.c_int, [C.c_char_p, C.c_double]),
    "ob_get_option": (C.c_int, [C.c_char_p, C.POINTER(C.c_double)]),
    "ob_tuning_build": (C.c_int, []),
    "ob_debug_normal": (C.c_int, [C.c_int, _D, C.c_int64, _D, _D]),
    "ob_logit": (C.c_int, [_P, _D, C.c_int64, _D, C.c_int64, C.c_int32, C.c_int32, C.c_double, _D, _D,
                           C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ob_probit": (C.c_int, [_P, _D, C.c_int64, _D, C.c_int64, C.c_int32, C.c_int32, C.c_double, _D,
                            C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ob_kde": (C.c_int, [_P, _D, _D, C.c_int64, _D, C.c_int64, C.c_double, _D]),
    "ob_silverman_bandwidth": (C.c_int, [_D, C.c_int64, _D]),
    "ob_dfl_run": (C.c_int, _FRAME + [C.POINTER(ob_dfl_config), _H]),
    "ob_dfl_results_get": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(_D), C.POINTER(_D), C.POINTER(_D),
                                     C.POINTER(_D)]),
    "ob_dfl_results_info": (C.c_int, [_P, C.POINTER(ob_dfl_info)]),
    "ob_dfl_results_free": (None, [_P]),
    "ob_knn": (C.c_int, [_P, _D, C.c_int64, C.c_int64, _D, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                         C.POINTER(C.c_int64), _D]),
    "ob_match_logistic": (C.c_int, [_P, _D, C.c_int64, _D, C.c_int64, C.c_int32, C.c_int32, C.c_double, _D, _D,
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ob_match_run": (C.c_int, _FRAME + [C.POINTER(ob_match_config), _H]),
    "ob_match_results_get": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(_D), C.POINTER(C.c_int64),
                                       C.POINTER(C.c_int32), C.POINTER(C.POINTER(C.c_int64)),
                                       C.POINTER(C.POINTER(C.c_int64)), C.POINTER(_D)]),
    "ob_match_results_info": (C.c_int, [_P, C.POINTER(ob_match_info)]),
    "ob_match_results_free": (None, [_P]),
    "ob_akm_connected_set": (C.c_int, _FRAME[1:] + [C.c_char_p, C.c_char_p, _H]),  # host only: no ctx
    "ob_akm_set_get": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(_U8), C.POINTER(C.c_int64),
                                 C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_int32)),
                                 C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ob_akm_set_id": (C.c_char_p, [_P, C.c_int32, C.c_int64]),
    "ob_akm_set_free": (None, [_P]),
    "ob_akm_demean": (C.c_int, [_P, _D, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                C.c_int64, C.c_int64, C.c_double, C.c_int64, _D, C.POINTER(C.c_int32),
                                C.POINTER(C.c_int32)]),
    "ob_akm_recover_fe": (C.c_int, [_P, _D, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64,
                                    C.c_int64, C.c_double, C.c_int64, _D, _D, C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int32)]),
    "ob_akm_run": (C.c_int, _FRAME + [C.POINTER(ob_akm_config), _H]),
    "ob_akm_results_get": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(_D), C.POINTER(C.c_int64),
                                     C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(_D), C.POINTER(C.c_int64),
                                     C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(_D), C.POINTER(C.c_double)]),
    "ob_akm_results_info": (C.c_int, [_P, C.POINTER(ob_akm_info)]),
    "ob_akm_results_free": (None, [_P]),
    "ob_vif_gram": (C.c_int, [_P, _D, C.c_int64, C.c_int64, C.c_int32, _D]),
    "ob_vif_solve": (C.c_int, [_D, C.c_int64, C.c_int32, _D]),
    "ob_vif_sums": (C.c_int, [_P, _D, C.c_int64, C.c_int64, C.c_int32, _D, _D, _D, _D]),
    "ob_vif": (C.c_int, [_P, _D, C.c_int64, C.c_int64, C.c_int32, _D]),
    "ob_vif_last_timing": (C.c_int, [_D, _D, _D]),
    "ob_vif_run": (C.c_int, _FRAME + [C.POINTER(C.c_char_p), C.c_int32, _D]),
    "ob_normal_inverse_cdf": (C.c_double, [C.c_double]),
    "ob_remedy_solve": (C.c_int, [_D, _D, C.c_int32, _D, _D]),
    "ob_remedy_score": (C.c_int, [_P, _D, C.c_int64, _D, C.c_int64, C.c_int64, C.c_int32, _D, _D, _D, _D, _D, _D]),
    "ob_remedy_allocate": (C.c_int, [_P, _D, _D, _D, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.c_double,
                                     C.POINTER(ob_remedy_request), C.POINTER(_P)]),
    "ob_remedy_results_info": (C.c_int, [_P, C.POINTER(ob_remedy_info)]),
    "ob_remedy_results_get": (C.c_int, [_P, C.POINTER(C.POINTER(C.c_int64)), C.POINTER(_D), C.POINTER(_D),
                                        C.POINTER(_D), C.POINTER(_D), C.POINTER(_D), C.POINTER(_D),
                                        C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_int64))]),
    "ob_remedy_results_free": (None, [_P]),
    "ob_remedy_results_model": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(_D),
                                          C.POINTER(_D)]),
    "ob_remedy_frontier": (C.c_int, _FRAME_CFG + [C.c_int32, C.c_double, _D, _D, _D, C.POINTER(C.c_int32), _D]),
    "ob_remedy_run": (C.c_int, _FRAME_CFG + [C.POINTER(ob_remedy_request), C.c_int32, C.c_int32, _H]),
    "ob_remedy_defend_rows": (C.c_int, [_P, _D, _D, _D, C.c_int64, C.c_int64, C.POINTER(C.c_int64), _D, C.c_int64,
                                        C.c_double, C.c_double, C.POINTER(_P)]),
    "ob_remedy_defend": (C.c_int, _FRAME_CFG + [C.POINTER(C.c_int64), _D, C.c_int64, C.POINTER(C.c_int64),
                                                C.POINTER(C.c_char_p), _D, C.c_int64, C.c_double, C.c_int32, _H]),
    "ob_remedy_resolve_overrides": (C.c_int, [C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64),
                                              C.POINTER(C.c_char_p), _D, C.c_int64, C.POINTER(C.c_char_p), C.c_int32,
                                              C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _D,
                                              C.POINTER(C.c_int64)]),
    "ob_remedy_results_defensible": (C.c_int, [_P, C.POINTER(C.POINTER(C.c_int32))]),
    "ob_remedy_results_defend_info": (C.c_int, [_P, C.POINTER(ob_defend_info)]),
    "ob_remedy_apply_adjustments": (C.c_int, [_D, _U8, C.c_int64, C.POINTER(C.c_int64), _D, C.c_int64, _D]),
    "ob_remedy_verify": (C.c_int, _FRAME_CFG + [C.POINTER(C.c_int64), _D, C.c_int64, _H]),
    "ob_jackknife_check_shape": (C.c_int, [C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "ob_jackknife": (C.c_int, [_P, C.c_int, C.POINTER(ob_jackknife_out)]),
    "ob_jackknife_rows": (C.c_int, [_P, C.c_int, _D, _U8, C.POINTER(C.c_int64)]),
    "ob_jackknife_last_timing": (C.c_int, [_D]),
    "ob_jackknife_finish": (C.c_int, [_D, C.POINTER(C.c_int64), C.c_int32, _D]),
    "ob_bca_stats": (C.c_int, [_D, C.c_int64, C.c_double, C.c_double, C.c_double, _D]),
    "ob_aggregate_bca": (C.c_int, [_D, _U8, C.c_uint64, C.c_int32, C.POINTER(C.c_int32), C.c_int32, _D, _D, C.c_double,
                                   _D]),
    "ob_prepared_jackknife": (C.c_int, [_P, C.POINTER(ob_jackknife_out)]),
    "ob_prepared_finish_bca": (C.c_int, [_P, _D, _U8, C.c_uint64, C.c_double, C.POINTER(_P)]),
    "ob_builder_run_bca": (C.c_int, _FRAME_CFG + [C.c_double, _H]),
    "ob_results_jackknife": (C.c_int, [_P, C.c_int32, C.c_int32, _D]),
    "ob_cluster_check_shape": (C.c_int, [C.c_int64, C.c_int32]),
    "ob_cluster_index": (C.c_int, [C.POINTER(ob_column), C.POINTER(C.c_int32), C.c_int64, C.c_int32,
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(ob_cluster_info)]),
    "ob_cluster_gram": (C.c_int, [_P, _D, C.c_int64, C.c_int64, C.c_int32, _D, _D, C.POINTER(C.c_int64),
                                  C.POINTER(C.c_int64), C.c_int64, _D, C.POINTER(C.c_uint32)]),
    "ob_cluster_counts": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int64, C.c_int64, C.c_int32,
                                    C.POINTER(C.c_uint32)]),
    "ob_cluster_apply": (C.c_int, [_P, C.POINTER(C.c_uint32), C.c_uint32, C.c_int64, _D, C.c_int32, _D]),
    "ob_cluster_last_timing": (C.c_int, [C.POINTER(ob_cluster_timing)]),
    "ob_builder_prepare_clustered": (C.c_int, _FRAME_CFG + [_CLUSTER, _H]),
    "ob_builder_run_clustered": (C.c_int, _FRAME_CFG + [_CLUSTER, _H]),
    "ob_builder_decompose_quantiles_clustered": (C.c_int, _FRAME_CFG + [_CLUSTER, _D, C.c_int32, _H]),
    "ob_prepared_cluster_info": (C.c_int, [_P, C.POINTER(ob_cluster_info)]),
    "ob_results_n_clusters": (C.c_int64, [_P]),
    "ob_cluster_jackknife_check_shape": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "ob_prepared_cluster_jackknife": (C.c_int, [_P, C.POINTER(ob_jackknife_out)]),
    "ob_prepared_cluster_jackknife_rows": (C.c_int, [_P, _D, _U8, C.POINTER(C.c_int64), _D]),
    "ob_cluster_jackknife": (C.c_int, [_P, _D, C.POINTER(C.c_uint32), C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_int64, C.c_int64, _D, _D, C.c_int, C.POINTER(ob_jackknife_out)]),
    "ob_cluster_jackknife_rows": (C.c_int, [_P, _D, C.POINTER(C.c_uint32), C.c_int64, C.c_int64, C.c_int32, C.c_int,
                                            _D, _U8, C.POINTER(C.c_int64), _D]),
    "ob_prepared_finish_cluster_bca": (C.c_int, [_P, _D, _U8, C.c_uint64, C.c_double, C.POINTER(_P)]),
    "ob_builder_run_clustered_bca": (C.c_int, _FRAME_CFG + [_CLUSTER, C.c_double, _H]),
    "ob_cluster_jackknife_last_timing": (C.c_int, [_D]),
    "ob_rif_stat": (C.c_int, [_P, _D, C.c_int64, C.POINTER(ob_rif_spec), _D, _D]),
    "ob_rif_scan_block": (C.c_int32, []),
    "ob_rif_last_timing": (C.c_int, [C.POINTER(ob_rif_timing)]),
    "ob_builder_decompose_statistics": (C.c_int, _FRAME_CFG + [_SPEC, C.c_int32, _H]),
    "ob_builder_decompose_statistics_clustered": (C.c_int, _FRAME_CFG + [_CLUSTER, _SPEC, C.c_int32, _H]),
    "ob_binary_row_len": (C.c_int, [C.c_int32]),
    "ob_binary_check_shape": (C.c_int, [C.c_int32, C.c_int64, C.c_int64]),
    "ob_binary_means": (C.c_int, [_P, _D, C.c_int64, _D, C.c_int64, C.c_int32, _U8, _D, _D]),
    "ob_binary_last_timing": (C.c_int, [C.POINTER(ob_binary_timing)]),
    "ob_builder_prepare_binary": (C.c_int, _FRAME_CFG + [C.c_int32, _H]),
    "ob_builder_run_binary": (C.c_int, _FRAME_CFG + [C.c_int32, _H]),
    "ob_prepared_point_row": (C.c_int, [_P, C.POINTER(_D), C.POINTER(C.c_int64)]),
    "ob_reweight_row_len": (C.c_int, [C.c_int32]),
    "ob_reweight_check_shape": (C.c_int, [C.c_int32, C.c_int64, C.c_int64]),
    "ob_reweight_last_timing": (C.c_int, [C.POINTER(ob_reweight_timing)]),
    "ob_reweight_logit_pass": (C.c_int, [_P, _D, C.c_int64, _D, _D, _U8, C.c_int64, C.c_int32, _D, C.c_int32, _D, _D]),
    "ob_reweight_gram": (C.c_int, [_P, _D, C.c_int64, _D, _D, _U8, C.c_int64, C.c_int32, _D, C.c_int32, _D, _D]),
    "ob_builder_prepare_reweighted": (C.c_int, _FRAME_CFG + [_H]),
    "ob_builder_run_reweighted": (C.c_int, _FRAME_CFG + [_H]),
    "ob_rif_stat_weighted": (C.c_int, [_P, _D, _D, C.c_int64, _SPEC, _D, _D]),
    "ob_builder_prepare_reweighted_statistic": (C.c_int, _FRAME_CFG + [_SPEC, _H]),
    "ob_prepared_reweight_statistics": (C.c_int, [_P, _D]),
    "ob_builder_run_reweighted_statistics": (C.c_int, _FRAME_CFG + [_SPEC, C.c_int32, _H]),
    "ob_dr_row_len": (C.c_int, [C.c_int32, C.c_int32]),
    "ob_dr_check_shape": (C.c_int, [C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "ob_dr_last_timing": (C.c_int, [C.POINTER(ob_dr_timing)]),
    "ob_dr_thresholds": (C.c_int, [_D, C.c_int64, C.c_int32, C.c_double, C.c_double, _D, C.POINTER(C.c_int32)]),
    "ob_dr_quantiles": (C.c_int, [_D, _D, C.c_int32, _D, C.c_int32, _D, _D, _U8]),
    "ob_dr_finish_rows": (C.c_int, [_D, C.c_int32, C.c_int32, _D, _U8, C.c_uint64, C.POINTER(_P)]),
    "ob_dr_logit_pass": (C.c_int, [_P, _D, C.c_int64, _D, _D, _U8, C.c_int64, C.c_int32, _D, C.c_int32, _D, _D, _D]),
    "ob_dr_cdf": (C.c_int, [_P, _D, C.c_int64, _D, _U8, C.c_int64, C.c_int32, _D, C.c_int32, _D, _D]),
    "ob_builder_prepare_dr": (C.c_int, _FRAME_CFG + [C.POINTER(ob_dr_config), _H]),
    "ob_builder_run_dr": (C.c_int, _FRAME_CFG + [C.POINTER(ob_dr_config), _H]),
    "ob_prepared_dr_info": (C.c_int, [_P, C.POINTER(ob_dr_info)]),
    "ob_rifq_row_len": (C.c_int, [C.c_int32, C.c_int32]),
    "ob_rifq_check_shape": (C.c_int, [C.c_int32, C.c_int32, _D, C.c_int64, C.c_int64]),
    "ob_rifq_pass": (C.c_int, [_P, _D, C.c_int64, _U8, C.c_int32, _D, C.c_int32, _D, C.c_int64, C.c_int32, _D, _D, _D, _D,
                               _D, _D, _U8]),
    "ob_rifq_last_timing": (C.c_int, [C.POINTER(ob_rifq_timing)]),
    "ob_builder_prepare_quantiles_refit": (C.c_int, _FRAME_CFG + [_D, C.c_int32, _H]),
    "ob_builder_decompose_quantiles_refit": (C.c_int, _FRAME_CFG + [_D, C.c_int32, _H]),
    "ob_prepared_rifq_info": (C.c_int, [_P, C.POINTER(ob_rifq_info)]),
    "ob_prepared_finish_tau": (C.c_int, [_P, C.c_int32, _D, _U8, C.c_uint64, C.POINTER(_P)]),
    "ob_rifs_row_len": (C.c_int, [C.c_int32, C.c_int32]),
    "ob_rifs_check_shape": (C.c_int, [C.c_int32, C.POINTER(ob_rif_spec), C.c_int32, C.c_int64, C.c_int64]),
    "ob_rifs_pass": (C.c_int, [_P, _D, C.c_int64, _U8, C.c_int32, C.POINTER(ob_rif_spec), C.c_int32, _D, C.c_int64,
                               C.c_int32, _D, _D, _U8, _U8]),
    "ob_rifs_last_timing": (C.c_int, [C.POINTER(ob_rifs_timing)]),
    "ob_builder_prepare_statistics_refit": (C.c_int, _FRAME_CFG + [_SPEC, C.c_int32, _H]),
    "ob_builder_decompose_statistics_refit": (C.c_int, _FRAME_CFG + [_SPEC, C.c_int32, _H]),
    "ob_prepared_rifs_info": (C.c_int, [_P, C.POINTER(ob_rifs_info)]),
    "ob_nopo_row_len": (C.c_int, []),
    "ob_nopo_check_shape": (C.c_int, [C.c_int64, C.c_int64, C.c_int64]),
    "ob_nopo_cells": (C.c_int, _FRAME_CFG[1:] + [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ob_nopo_sums": (C.c_int, [_P, _D, _D, C.POINTER(C.c_int32), C.c_int64, C.c_int32, _U8, C.c_int32, _D, _D]),
    "ob_nopo_finish_rows": (C.c_int, [_D, _D, _U8, C.c_uint64, C.POINTER(_P)]),
    "ob_nopo_last_timing": (C.c_int, [C.POINTER(ob_nopo_timing)]),
    "ob_builder_prepare_nopo": (C.c_int, _FRAME_CFG + [_H]),
    "ob_builder_run_nopo": (C.c_int, _FRAME_CFG + [_H]),
    "ob_prepared_nopo_info": (C.c_int, [_P, C.POINTER(ob_nopo_info)]),
    "ob_density_row_len": (C.c_int, [C.c_int32, C.c_int32]),
    "ob_density_check_shape": (C.c_int, [C.c_int32, C.c_int64, C.c_int64, C.c_int32]),
    "ob_density_last_timing": (C.c_int, [C.POINTER(ob_density_timing)]),
    "ob_density_grid": (C.c_int, [_D, C.c_int64, C.c_int32, _D]),
    "ob_density_pass": (C.c_int, [_P, _D, C.c_int64, _D, _D, _U8, C.c_int64, C.c_int32, _D, C.c_int32, _D, C.c_int32,
                                  C.c_double, _D, _D, _D]),
    "ob_density_finish_rows": (C.c_int, [_D, C.c_int32, C.c_int32, _D, _U8, C.c_uint64, C.POINTER(_P)]),
    "ob_builder_prepare_density": (C.c_int, _FRAME_CFG + [C.POINTER(ob_density_config), _H]),
    "ob_builder_run_density": (C.c_int, _FRAME_CFG + [C.POINTER(ob_density_config), _H]),
    "ob_prepared_density_info": (C.c_int, [_P, C.POINTER(ob_density_info)]),
    "ob_tobit_row_len": (C.c_int, [C.c_int32]),
    "ob_tobit_check_shape": (C.c_int, [C.c_int32, C.c_int64, C.c_int64]),
    "ob_tobit_last_timing": (C.c_int, [C.POINTER(ob_tobit_timing)]),
    "ob_tobit_lambda": (C.c_int, [_D, C.c_int64, _D]),
    "ob_tobit_pass": (C.c_int, [_P, _D, C.c_int64, _D, _D, _U8, C.c_int64, C.c_int32, _TOBIT, _D, C.c_int32, _D, _D,
                                _D]),
    "ob_tobit_fit": (C.c_int, [_P, _D, C.c_int64, _D, _D, C.c_int64, C.c_int32, _TOBIT, _U8, C.c_int32, _D, _D,
                               C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "ob_tobit_means": (C.c_int, [_P, _D, C.c_int64, _D, _D, _U8, C.c_int64, C.c_int32, _TOBIT, _D, _D]),
    "ob_tobit_rows": (C.c_int, [_P, C.c_int32, _TOBIT, C.c_int32, _D, C.c_int64, _D, _D, C.c_int64, _U8, _D, C.c_int64,
                                _D, _D, C.c_int64, _U8, C.c_int32, _D, _U8]),
    "ob_tobit_finish_rows": (C.c_int, [_D, C.c_int32, _D, _U8, C.c_uint64, C.POINTER(_P)]),
    "ob_builder_prepare_tobit": (C.c_int, _FRAME_CFG + [_TOBIT, _H]),
    "ob_builder_run_tobit": (C.c_int, _FRAME_CFG + [_TOBIT, _H]),
    "ob_prepared_tobit_info": (C.c_int, [_P, C.POINTER(ob_tobit_info)]),
}

# Every exported entry point of include/oaxaca_boot.h (tests/test_capi_host.py checks both ways).
EXPORTED = tuple(_SIGS)


def _pointer_to(ctype):
    ptr = C.POINTER(ctype)
    return lambda a: None if a is None else a.ctypes.data_as(ptr)


# A numpy array's buffer as the C ABI takes it (None stays NULL). The array must outlive the call.
dp, u8p, u32p = _pointer_to(C.c_double), _pointer_to(C.c_uint8), _pointer_to(C.c_uint32)
i32p, i64p = _pointer_to(C.c_int32), _pointer_to(C.c_int64)


def strs(names):
    """A ``char**`` of the encoded names -> (pointer, the array behind it). The pointer is only good while the
    array is alive: hold the array until the C call has returned (``api._frame_call`` does)."""
    arr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    return C.cast(arr, C.POINTER(C.c_char_p)), arr


def struct_dict(s) -> dict:
    """A ctypes struct's fields by name."""
    return {f: getattr(s, f) for f, _ in s._fields_}


def array_copy(ptr, shape):
    """A copy of the library-owned array at the typed pointer ``ptr``. Zero elements never touch the pointer (it
    may be NULL): they give zeros of the shape in the pointer's type."""
    shape = tuple(int(v) for v in shape)
    if not math.prod(shape):
        return np.zeros(shape, dtype=np.dtype(ptr._type_))
    return np.ctypeslib.as_array(ptr, shape=shape).copy()


_lib = None
_lib_lock = threading.Lock()


def _share_torch_runtime():
    """PyTorch-ROCm bundles its own libamdhip64.so.7. Loading ours first would put two HIP
    runtimes in the process (torch's stream/allocations would then be foreign handles), so when
    torch is installed it is imported first and the engine binds to its runtime (same soname)."""
    if os.environ.get("OB_NO_TORCH") == "1":
        return
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def lib() -> C.CDLL:
    """Load the engine library once; raise loudly if it was not built."""
    global _lib
    if _lib is None:
        _share_torch_runtime()
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise ImportError(
                    f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                    "(make -C oaxaca-blinder-rs_amd/csrc). There is no CPU fallback.")
            handle = C.CDLL(LIB_PATH)
            for name, (res, args) in _SIGS.items():
                fn = getattr(handle, name)
                fn.restype = res
                fn.argtypes = args
            _lib = handle
    return _lib


def check(rc: int) -> None:
    if rc != OB_OK:
        msg = lib().ob_last_error().decode("utf-8", "replace")
        raise OaxacaError(rc, msg)


_ctx_cache: dict = {}


def resolve_device(device: int | None = None) -> int:
    """The GPU a ``device=None`` call uses: OB_DEVICE, else LOCAL_RANK, else 0."""
    if device is None:
        device = int(os.environ.get("OB_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    return int(device)


def context(device: int | None = None) -> C.c_void_p:
    """Process-wide ob_ctx for ``device`` (default: resolve_device())."""
    device = resolve_device(device)
    with _lib_lock:
        ctx = _ctx_cache.get(device)
    if ctx is None:
        ctx = C.c_void_p()
        check(lib().ob_ctx_create(device, C.byref(ctx)))
        with _lib_lock:
            _ctx_cache[device] = ctx
    return ctx


def unique_id() -> bytes:
    """ncclGetUniqueId through the engine (rank 0 calls it and broadcasts the 128 bytes)."""
    u = ob_unique_id()
    check(lib().ob_get_unique_id(C.byref(u)))
    return C.string_at(C.addressof(u), C.sizeof(u))


_rank_ctx_cache: dict = {}


def rank_context(device: int, rank: int, world: int, uid: bytes) -> C.c_void_p:
    """An ob_ctx that is rank ``rank`` of ``world`` on an RCCL communicator (ob_ctx_create_rank).
    Cached per (device, rank, world, uid); panels created in it run sharded."""
    key = (device, rank, world, bytes(uid))
    with _lib_lock:
        ctx = _rank_ctx_cache.get(key)
    if ctx is None:
        uid = bytes(uid)
        if len(uid) != C.sizeof(ob_unique_id):
            raise ValueError("a unique id is 128 bytes")
        u = ob_unique_id()
        C.memmove(C.addressof(u), uid, len(uid))
        ctx = C.c_void_p()
        check(lib().ob_ctx_create_rank(device, rank, world, C.byref(u), C.byref(ctx)))
        with _lib_lock:
            _rank_ctx_cache[key] = ctx
    return ctx


def ctx_rank(ctx) -> tuple:
    """(rank, world) of the engine's RCCL communicator in ``ctx`` (ob_ctx_rank; (0, 1) for a
    plain context)."""
    r, w = C.c_int(0), C.c_int(0)
    check(lib().ob_ctx_rank(ctx, C.byref(r), C.byref(w)))
    return r.value, w.value


def set_option(name: str, value) -> None:
    """ob_set_option: a process-wide engine switch (include/oaxaca_boot.h); None restores the default.
    The library reads no environment variable -- tests and tools set these explicitly."""
    check(lib().ob_set_option(name.encode(), float("nan") if value is None else float(value)))


def get_option(name: str):
    """ob_get_option: the value ob_set_option stored for ``name``, or None when it is unset."""
    v = C.c_double()
    check(lib().ob_get_option(name.encode(), C.byref(v)))
    return None if math.isnan(v.value) else v.value


@contextlib.contextmanager
def option(name: str, value):
    """set_option for the duration of a with-block, then back to the value it had before (so
    nested blocks and fixtures that already set the option keep their setting)."""
    prev = get_option(name)
    set_option(name, value)
    try:
        yield
    finally:
        set_option(name, prev)


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().ob_device_count(C.byref(n))
    return n.value if rc == OB_OK else 0
