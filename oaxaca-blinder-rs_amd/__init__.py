"""MI355X-native bootstrap-inference engine for Oaxaca-Blinder decomposition.

Drop-in for the bootstrap driver of ``OaxacaBuilder::run()`` in dot-comma-hyphen/oaxaca-blinder-rs.
Import with ``importlib.import_module("oaxaca-blinder-rs_amd")`` (the directory name carries a
hyphen). See DESIGN.md for the kernels and INTEGRATION.md for the Rust/C binding.
"""
from . import _native
from ._native import OaxacaError
from .api import (Adjustment, AkmBuilder, AkmResult, BinaryDecompositionResults, BudgetAdjustment, ComponentResult, Contribution, DataSummary,
                  DecompositionDetail, DecompositionResult, DflResult, DistributionDecompositionResults, dr_finish_rows, JackknifeResult, defensibility_message, parse_rust_f64, FrontierPoint, MatchingEngine, MatchResult, OaxacaBlinder, OaxacaBuilder,
                  OaxacaResults, OptimizationResult, PreparedRun,
                  QuantileDecompositionBuilder, QuantileDecompositionDetail, QuantileDecompositionResults,
                  ReferenceCoefficients, ReweightedDecompositionResults, TwoFoldResults, VifResult, calculate_vif, estimate_akm, match_units,
                  parse_formula, run_dfl, run_dfl_from_csv, NopoDecompositionResults, nopo_cells, nopo_finish_rows,
                  DensityCurve, DensityDecompositionResults, density_finish_rows, TobitDecompositionResults,
                  tobit_finish_rows)
from .engine import (binary_check_shape, binary_last_timing, binary_means, binary_row_len, cluster_apply, cluster_check_shape, cluster_counts, cluster_gram, cluster_index,
                     cluster_last_timing, cluster_jackknife, cluster_jackknife_rows, cluster_jackknife_check_shape, cluster_jackknife_last_timing, Panel, aggregate, aggregate_bca, bca_stats, jackknife_check_shape, jackknife_finish,
                     jackknife_last_timing, jackknife_rows, akm_connected_set, akm_demean, akm_recover_fe, boot_multi, bootstrap_stats, kde,
                     knn, logit, match_logistic, normal_inverse_cdf, probit, remedy_allocate, remedy_apply_adjustments, remedy_defend_rows,
                     remedy_resolve_overrides, remedy_score, remedy_solve, rif, parse_rif_statistic, parse_weighted_rif_statistic,
                     rif_statistic_weighted, rif_last_timing,
                     rif_scan_block, rif_statistic, reweight_check_shape, reweight_gram, reweight_last_timing,
                     reweight_logit_pass, reweight_row_len,
                     dr_cdf, dr_check_shape, dr_last_timing, dr_logit_pass, dr_quantiles, dr_row_len, dr_thresholds,
                     rifq_check_shape, rifq_last_timing, rifq_pass, rifq_row_len,
                     rifs_check_shape, rifs_last_timing, rifs_pass, rifs_row_len,
                     nopo_check_shape, nopo_last_timing, nopo_row_len, nopo_sums,
                     density_check_shape, density_grid, density_last_timing, density_pass, density_row_len,
                     tobit, tobit_check_shape, tobit_fit, tobit_lambda, tobit_last_timing, tobit_means, tobit_pass,
                     tobit_row_len, tobit_rows,
                     row_layout, silverman_bandwidth, vif, vif_gram, vif_last_timing, vif_solve, vif_sums)
from .frame import Frame, read_csv

__all__ = [
    "OaxacaBuilder", "OaxacaBlinder", "OaxacaResults", "TwoFoldResults", "DecompositionDetail",
    "ComponentResult", "BudgetAdjustment", "ReferenceCoefficients", "OaxacaError", "PreparedRun",
    "Panel", "boot_multi", "Frame", "read_csv", "aggregate", "bootstrap_stats", "rif", "row_layout", "parse_formula",
    "QuantileDecompositionBuilder", "QuantileDecompositionDetail", "QuantileDecompositionResults",
    "DflResult", "run_dfl", "run_dfl_from_csv", "logit", "probit", "kde", "silverman_bandwidth",
    "MatchingEngine", "MatchResult", "match_units", "knn", "match_logistic",
    "AkmBuilder", "AkmResult", "estimate_akm", "akm_connected_set", "akm_demean", "akm_recover_fe",
    "VifResult", "calculate_vif", "vif", "vif_gram", "vif_solve", "vif_sums", "vif_last_timing",
    "OptimizationResult", "Adjustment", "Contribution", "FrontierPoint", "normal_inverse_cdf", "remedy_solve", "remedy_score",
    "remedy_allocate", "remedy_defend_rows", "remedy_resolve_overrides", "remedy_apply_adjustments",
    "DecompositionResult", "DataSummary", "defensibility_message", "parse_rust_f64",
    "JackknifeResult", "jackknife_rows", "jackknife_finish", "jackknife_check_shape", "jackknife_last_timing", "bca_stats",
    "aggregate_bca",
    "cluster_index", "cluster_gram", "cluster_counts", "cluster_apply", "cluster_check_shape", "cluster_last_timing",
    "cluster_jackknife", "cluster_jackknife_rows", "cluster_jackknife_check_shape", "cluster_jackknife_last_timing",
    "rif_statistic", "rif_last_timing", "rif_scan_block", "parse_rif_statistic",
    "rif_statistic_weighted", "parse_weighted_rif_statistic",
    "BinaryDecompositionResults", "binary_means", "binary_check_shape", "binary_row_len", "binary_last_timing",
    "ReweightedDecompositionResults", "reweight_logit_pass", "reweight_gram", "reweight_check_shape",
    "reweight_row_len", "reweight_last_timing",
    "DistributionDecompositionResults", "dr_logit_pass", "dr_cdf", "dr_thresholds", "dr_quantiles", "dr_last_timing",
    "dr_check_shape", "dr_row_len", "dr_finish_rows",
    "rifq_pass", "rifq_check_shape", "rifq_row_len", "rifq_last_timing",
    "rifs_pass", "rifs_check_shape", "rifs_row_len", "rifs_last_timing",
    "NopoDecompositionResults", "nopo_cells", "nopo_sums", "nopo_check_shape", "nopo_row_len", "nopo_last_timing",
    "nopo_finish_rows",
    "DensityDecompositionResults", "DensityCurve", "density_pass", "density_grid", "density_check_shape",
    "density_row_len", "density_last_timing", "density_finish_rows",
    "TobitDecompositionResults", "tobit", "tobit_pass", "tobit_fit", "tobit_means", "tobit_rows", "tobit_lambda",
    "tobit_check_shape", "tobit_row_len", "tobit_last_timing", "tobit_finish_rows",
]
