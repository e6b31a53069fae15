"""Python surface of the engine, mirroring the reference's public API for the bootstrap path:

* ``OaxacaBuilder``  -- builder.rs:37-757 (setters, run, decompose_quantile, get_data_matrices)
* ``OaxacaBlinder``  -- the pyo3 class declared in python.rs:193-276 (fit, fit_quantile,
  optimize_budget); ``bootstrap_reps`` defaults to 100 and the reference coefficients to the
  builder default GroupA, as there.
* ``OaxacaResults`` / ``TwoFoldResults`` / ``DecompositionDetail`` / ``ComponentResult`` --
  types.rs:8-47,160-180 (field names and order are the API).

Every compute call goes through the C ABI into the HIP engine; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import enum
import json
import re
from dataclasses import dataclass, field

import numpy as np

from . import _native as N
from .frame import Frame


class ReferenceCoefficients(enum.IntEnum):
    """decomposition.rs:5-20"""
    GroupA = 0
    GroupB = 1
    Pooled = 2
    Weighted = 3
    Cotton = 4
    Neumark = 5


@dataclass
class ComponentResult:
    name: str
    estimate: float
    std_err: float
    t_stat: float
    p_value: float
    ci_lower: float
    ci_upper: float

    def __repr__(self):
        return f"ComponentResult(name={self.name}, estimate={self.estimate})"


@dataclass
class JackknifeResult:
    """The leave-one-out pass over the panel: one entry per component, in the order of a
    replicate row's first 6 + 2K columns. ``names``: explained, unexplained, endowments, coefficients,
    interaction, total_gap, then ``explained:<column>`` and ``unexplained:<column>`` per design column."""
    names: list
    estimate: np.ndarray
    accel: np.ndarray
    std_err: np.ndarray
    bias: np.ndarray
    n_used: tuple
    n_dropped: tuple
    sums: np.ndarray = field(repr=False, default=None)


@dataclass
class TwoFoldResults:
    aggregate: list
    detailed_explained: list
    detailed_unexplained: list
    detailed_selection: list


@dataclass
class DecompositionDetail:
    aggregate: list
    detailed: list


@dataclass
class BudgetAdjustment:
    index: int
    original_residual: float
    adjustment: float


@dataclass
class Contribution:
    """engine/src/types.rs:89-93"""
    name: str
    value: float


@dataclass
class Adjustment:
    """engine/src/types.rs:95-107. ``optimize()`` leaves ``is_defensible`` and ``defensibility_message``
    None; ``check_defensibility()`` fills both (``new_wage >= lower bound - 1.0`` and the reference's two
    message strings)."""
    index: int
    adjustment: float
    current_wage: float
    new_wage: float
    fair_wage: float
    fair_wage_lower_bound: float | None = None
    fair_wage_upper_bound: float | None = None
    contributions: list = field(default_factory=list)
    is_defensible: bool | None = None
    defensibility_message: str | None = None


@dataclass
class OptimizationResult:
    """engine/src/types.rs:109-119"""
    adjustments: list
    total_cost: float
    original_gap: float
    new_gap: float
    original_unexplained_gap: float
    new_unexplained_gap: float
    required_budget: float
    model_coefficients: list


@dataclass
class DataSummary:
    """engine/src/types.rs:27-34: counts and group means of the (adjusted) outcome; group A is the
    reference group, B every other row."""
    total_count: int
    group_a_count: int
    group_b_count: int
    group_a_mean: float
    group_b_mean: float


@dataclass
class DecompositionResult:
    """engine/src/types.rs:36-49. The detailed lists hold ``ComponentResult``s (the reference's
    ``DetailedComponent`` fields and ``t_stat``); ``results`` is the full ``OaxacaResults``."""
    total_gap: float
    explained_gap: float
    unexplained_gap: float
    interaction_gap: float | None
    explained_percentage: float
    unexplained_percentage: float
    interaction_percentage: float | None
    detailed_explained: list
    detailed_unexplained: list
    data_summary: DataSummary | None
    unexplained_standard_error: float | None
    results: "OaxacaResults" = field(default=None, repr=False)


_RUST_F64 = re.compile(r"[+-]?(?:(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?|(?i:inf|infinity|nan))")


def parse_rust_f64(text):
    """``str::parse::<f64>`` (defensibility.rs:40): the float, or None where Rust returns Err. No
    surrounding whitespace and no underscores; ``inf``, ``infinity`` and ``nan`` in any case, a sign and
    an exponent are taken."""
    if not isinstance(text, str) or not _RUST_F64.fullmatch(text):
        return None
    return float(text)


def defensibility_message(is_defensible: bool, new_wage: float, lower: float) -> str:
    """defensibility.rs:227-235; ``:.2f`` rounds the exact binary value to even, as Rust's ``{:.2}``."""
    if is_defensible:
        return "Wage is within or above the calculated fair range."
    return f"Wage is {lower - new_wage:.2f} below the defensible lower bound ({lower:.2f})."


def _proposed(adjustments):
    """(index, value, overrides) per proposed adjustment: an ``Adjustment`` (its ``.adjustment``), an
    ``(index, value[, overrides])`` tuple or a dict with the reference's field names. Override values are
    numbers or strings; a string Rust would not parse is dropped (defensibility.rs:40)."""
    out = []
    for a in adjustments:
        if isinstance(a, Adjustment):
            idx, val, ovr = a.index, a.adjustment, None
        elif isinstance(a, dict):
            idx, val, ovr = a["index"], a["value"], a.get("predictor_overrides")
        else:
            idx, val, ovr = (tuple(a) + (None,))[:3]
        kept = {}
        for name, v in (ovr or {}).items():
            v = parse_rust_f64(v) if isinstance(v, str) else float(v)
            if v is not None:
                kept[str(name)] = v
        out.append((int(idx), float(val), kept))
    return out


@dataclass
class FrontierPoint:
    """engine/src/types.rs:135-141"""
    budget: float
    t_statistic: float
    p_value: float
    is_significant: bool


@dataclass
class OaxacaResults:
    total_gap: float
    two_fold: TwoFoldResults
    three_fold: DecompositionDetail
    n_a: int
    n_b: int
    residuals: np.ndarray
    xa_mean: np.ndarray = field(repr=False)
    xb_mean: np.ndarray = field(repr=False)
    beta_star: np.ndarray = field(repr=False)
    n_failed: int = 0
    jackknife: dict = None  # run_bca / finish_bca: (table, name) -> {accel, std_err, bias, z0, flag}
    n_clusters: int = None  # a cluster bootstrap's C (OaxacaBuilder.cluster), else None
    # decompose_quantile(s)(refit=True) only: the point (q_A, q_B), the point (f_A, f_B) after the floor and the
    # floored densities over the point pass and every replicate, group and quantile of the run
    quantile_values: tuple = None
    density_values: tuple = None
    n_density_floored: int = None
    # decompose_statistic(s)(refit=True) only: the point (nu_A, nu_B); a range also sets n_density_floored
    statistic_values: tuple = None

    def explained(self):
        return next((c for c in self.two_fold.aggregate if c.name == "explained"), None)

    def unexplained(self):
        return next((c for c in self.two_fold.aggregate if c.name == "unexplained"), None)

    def get_summary_table(self):
        return [(c.name, c) for c in self.two_fold.aggregate]

    def get_detailed_table(self):
        m = {}
        for c in self.two_fold.detailed_explained:
            m.setdefault(c.name, [0.0, 0.0])[0] = c.estimate
        for c in self.two_fold.detailed_unexplained:
            m.setdefault(c.name, [0.0, 0.0])[1] = c.estimate
        return [(k, v[0], v[1]) for k, v in m.items()]

    def optimize_budget(self, budget: float, target_gap: float):
        """types.rs:98-156 (greedy raises for the most negative group-B residuals)."""
        if self.total_gap <= target_gap:
            return []
        needed = (self.total_gap - target_gap) * self.n_b
        eff = min(budget, needed)
        cand = sorted(((i, r) for i, r in enumerate(self.residuals) if r < 0.0), key=lambda t: t[1])
        out, spent = [], 0.0
        for idx, res in cand:
            if spent >= eff:
                break
            raise_ = min(-res, eff - spent)
            if raise_ > 1e-9:
                out.append(BudgetAdjustment(idx, float(res), float(raise_)))
                spent += raise_
        return out

    def to_json(self) -> str:
        def comp(c):
            return c.__dict__

        def fix(v):  # serde_json writes non-finite floats as null
            return v if isinstance(v, str) or np.isfinite(v) else None

        d = {
            "total_gap": self.total_gap,
            "two_fold": {k: [{kk: fix(vv) for kk, vv in comp(c).items()} for c in getattr(self.two_fold, k)]
                         for k in ("aggregate", "detailed_explained", "detailed_unexplained", "detailed_selection")},
            "three_fold": {k: [{kk: fix(vv) for kk, vv in comp(c).items()} for c in getattr(self.three_fold, k)]
                           for k in ("aggregate", "detailed")},
            "n_a": self.n_a,
            "n_b": self.n_b,
            "residuals": [fix(float(v)) for v in self.residuals],
        }
        if self.n_clusters is not None:  # absent without clustering: the JSON of a row bootstrap is unchanged
            d["n_clusters"] = self.n_clusters
        if self.quantile_values is not None:  # absent without the refit
            d["quantile_values"] = list(self.quantile_values)
            d["density_values"] = list(self.density_values)
            d["n_density_floored"] = self.n_density_floored
        if self.statistic_values is not None:  # absent without the refit
            d["statistic_values"] = list(self.statistic_values)
            if self.n_density_floored is not None:
                d["n_density_floored"] = self.n_density_floored
        return json.dumps(d)

    def summary(self) -> str:
        """display.rs:9-82 (plain-text tables)."""
        lines = ["Oaxaca-Blinder Decomposition Results", "=" * 40,
                 f"Group A (Advantaged): {self.n_a} observations",
                 f"Group B (Reference):  {self.n_b} observations",
                 f"Total Gap: {self.total_gap:.4f}", ""]

        def table(title, comps, first="Component"):
            lines.append(title)
            lines.append(f"{first:<28} {'Estimate':>10} {'Std. Err.':>10} {'p-value':>8}  95% CI")
            for c in comps:
                lines.append(f"{c.name:<28} {c.estimate:>10.4f} {c.std_err:>10.4f} {c.p_value:>8.4f}"
                             f"  [{c.ci_lower:.3f}, {c.ci_upper:.3f}]")
            lines.append("")

        table("Two-Fold Decomposition", self.two_fold.aggregate)
        table("Detailed Decomposition (Explained)", self.two_fold.detailed_explained, "Variable")
        table("Detailed Decomposition (Unexplained)", self.two_fold.detailed_unexplained, "Variable")
        text = "\n".join(lines)
        print(text)
        return text

    def interpret(self) -> str:
        """python.rs:155-185"""
        e = self.explained().estimate if self.explained() else 0.0
        u = self.unexplained().estimate if self.unexplained() else 0.0
        t = self.total_gap
        return (f"The total gap is {t:.4f}. \n{e / t * 100:.1f}% of this gap is explained by differences in "
                f"endowments (observables), while {u / t * 100:.1f}% is unexplained (coefficients/discrimination).")


@dataclass
class BinaryDecompositionResults:
    """``OaxacaBuilder.decompose_binary``: the probit Oaxaca-Blinder decomposition of a 0/1 outcome. The
    component objects are ``OaxacaResults``' (estimate, standard error, percentile interval, p-value over the
    bootstrap); ``total_gap`` is the predicted gap Pbar(A, beta_A) - Pbar(B, beta_B), ``raw_gap`` the gap in the
    groups' observed rates; ``probabilities`` maps (group, coefficients) to the six mean probabilities."""
    model: str
    total_gap: float
    raw_gap: float
    two_fold: list
    three_fold: list
    detailed_explained: list
    detailed_unexplained: list
    probabilities: dict
    beta_a: np.ndarray = field(repr=False)
    beta_b: np.ndarray = field(repr=False)
    beta_star: np.ndarray = field(repr=False)
    xa_mean: np.ndarray = field(repr=False)
    xb_mean: np.ndarray = field(repr=False)
    names: list = field(repr=False)
    n_a: int = 0
    n_b: int = 0
    n_failed: int = 0

    def to_json(self) -> str:
        def fix(v):  # serde_json writes non-finite floats as null
            return v if isinstance(v, str) or np.isfinite(v) else None

        def comps(cs):
            return [{k: fix(v) for k, v in c.__dict__.items()} for c in cs]

        return json.dumps({
            "model": self.model, "total_gap": fix(self.total_gap), "raw_gap": fix(self.raw_gap),
            "two_fold": comps(self.two_fold), "three_fold": comps(self.three_fold),
            "detailed_explained": comps(self.detailed_explained),
            "detailed_unexplained": comps(self.detailed_unexplained),
            "probabilities": {f"{g}|{b}": fix(v) for (g, b), v in self.probabilities.items()},
            "names": list(self.names),
            "beta_a": [fix(float(v)) for v in self.beta_a], "beta_b": [fix(float(v)) for v in self.beta_b],
            "beta_star": [fix(float(v)) for v in self.beta_star],
            "n_a": self.n_a, "n_b": self.n_b, "n_failed": self.n_failed})


@dataclass
class ReweightedDecompositionResults:
    """``OaxacaBuilder.decompose_reweighted``: the reweighted Oaxaca-Blinder decomposition (Fortin, Lemieux and
    Firpo 2011, section 5). ``aggregate`` holds total_gap, composition, structure, pure_explained,
    specification_error, pure_unexplained and reweighting_error; the four detailed tables their summands per
    design column. The component objects are ``OaxacaResults``' (estimate, standard error, percentile interval,
    p-value over the bootstrap, in which the propensity logit is refitted per replicate).
    With a statistic (``decompose_reweighted("gini")``) the outcome of the three fits is the statistic's weighted
    RIF in A, B and C: ``statistic`` is (name, params), ``statistics`` (nu_A, nu_B, nu_C) the statistic itself in the
    three samples, and ``y_means`` the weighted means of the RIFs. Both are ``None`` for the mean."""
    total_gap: float
    aggregate: list
    detailed_pure_explained: list
    detailed_specification_error: list
    detailed_pure_unexplained: list
    detailed_reweighting_error: list
    beta_a: np.ndarray = field(repr=False)
    beta_b: np.ndarray = field(repr=False)
    beta_c: np.ndarray = field(repr=False)
    gamma: np.ndarray = field(repr=False)
    xa_mean: np.ndarray = field(repr=False)
    xb_mean: np.ndarray = field(repr=False)
    xc_mean: np.ndarray = field(repr=False)
    y_means: tuple = (0.0, 0.0, 0.0)
    effective_sample_size: float = 0.0
    logit_passes: int = 0
    names: list = field(default_factory=list, repr=False)
    n_a: int = 0
    n_b: int = 0
    n_failed: int = 0
    statistic: tuple | None = None
    statistics: tuple | None = None

    def component(self, name: str):
        return next(c for c in self.aggregate if c.name == name)

    def to_json(self) -> str:
        def fix(v):  # serde_json writes non-finite floats as null
            return v if isinstance(v, str) or np.isfinite(v) else None

        def comps(cs):
            return [{k: fix(v) for k, v in c.__dict__.items()} for c in cs]

        def vec(a):
            return [fix(float(v)) for v in a]

        extra = {}
        if self.statistic is not None:
            extra["statistic"] = {"stat": self.statistic[0], **self.statistic[1]}
        if self.statistics is not None:
            extra["statistics"] = vec(self.statistics)
        return json.dumps({
            "total_gap": fix(self.total_gap), "aggregate": comps(self.aggregate),
            "detailed_pure_explained": comps(self.detailed_pure_explained),
            "detailed_specification_error": comps(self.detailed_specification_error),
            "detailed_pure_unexplained": comps(self.detailed_pure_unexplained),
            "detailed_reweighting_error": comps(self.detailed_reweighting_error),
            "names": list(self.names), "beta_a": vec(self.beta_a), "beta_b": vec(self.beta_b),
            "beta_c": vec(self.beta_c), "gamma": vec(self.gamma), "xa_mean": vec(self.xa_mean),
            "xb_mean": vec(self.xb_mean), "xc_mean": vec(self.xc_mean), "y_means": vec(self.y_means),
            "effective_sample_size": fix(self.effective_sample_size), "logit_passes": self.logit_passes,
            "n_a": self.n_a, "n_b": self.n_b, "n_failed": self.n_failed, **extra})


def _reweighted_results(res, point, statistic=None, statistics=None) -> ReweightedDecompositionResults:
    """The tables of a reweighted handle's finish() and its point row."""
    k = (len(point) - 12) // 11
    tail = point[7 + 4 * k:]
    sc = tail[7 * k:]
    # the reweighted handle's five tables travel in the slots of run()'s (OB_RW_TABLE_*)
    return ReweightedDecompositionResults(
        total_gap=float(point[0]), aggregate=res.two_fold.aggregate,
        detailed_pure_explained=res.two_fold.detailed_explained,
        detailed_specification_error=res.two_fold.detailed_unexplained,
        detailed_pure_unexplained=res.two_fold.detailed_selection,
        detailed_reweighting_error=res.three_fold.aggregate,
        beta_a=tail[:k].copy(), beta_b=tail[k:2 * k].copy(), beta_c=tail[2 * k:3 * k].copy(),
        xa_mean=tail[3 * k:4 * k].copy(), xb_mean=tail[4 * k:5 * k].copy(), xc_mean=tail[5 * k:6 * k].copy(),
        gamma=tail[6 * k:7 * k].copy(), y_means=(float(sc[0]), float(sc[1]), float(sc[2])),
        effective_sample_size=float(sc[3]), logit_passes=int(sc[4]),
        names=[c.name for c in res.two_fold.detailed_explained],
        n_a=res.n_a, n_b=res.n_b, n_failed=res.n_failed, statistic=statistic, statistics=statistics)


@dataclass
class DistributionDecompositionResults:
    """``OaxacaBuilder.decompose_distribution``: the distribution-regression decomposition of Chernozhukov,
    Fernandez-Val and Melly (2013). ``quantile_effects`` and ``distribution_effects`` hold, under ``"total"``,
    ``"composition"`` and ``"structure"``, one component per quantile / threshold (estimate, standard error,
    percentile interval, p-value over the bootstrap, in which every threshold logit is refitted per replicate);
    ``quantile_values`` the quantiles of A, B and the counterfactual C; ``cdf`` the four distributions ``"AA"``,
    ``"BB"``, ``"AB"`` (= C: A's covariates, B's coefficients) and ``"BA"`` as fitted, and ``cdf_rearranged`` the
    monotone rearrangement of their point estimates, which the quantiles are read from. ``beta_a`` / ``beta_b``:
    (T, K) point fits. ``n_out_of_range``: (tau, distribution) pairs whose tau lies outside the fitted range of the
    threshold grid, where the quantile is the grid's end."""
    quantiles: np.ndarray
    thresholds: np.ndarray
    quantile_effects: dict
    quantile_values: dict
    distribution_effects: dict
    cdf: dict
    cdf_rearranged: dict = field(repr=False, default_factory=dict)
    beta_a: np.ndarray = field(repr=False, default=None)
    beta_b: np.ndarray = field(repr=False, default=None)
    passes: np.ndarray = field(repr=False, default=None)
    out_of_range: np.ndarray = field(repr=False, default=None)
    names: list = field(default_factory=list, repr=False)
    n_a: int = 0
    n_b: int = 0
    n_failed: int = 0
    n_out_of_range: int = 0
    n_thresholds_requested: int = 0

    def to_json(self) -> str:
        def fix(v):  # serde_json writes non-finite floats as null
            return v if isinstance(v, str) or np.isfinite(v) else None

        def comps(d):
            return {key: [{k: fix(v) for k, v in c.__dict__.items()} for c in cs] for key, cs in d.items()}

        def vec(a):
            return [fix(float(v)) for v in np.asarray(a).ravel()]

        return json.dumps({
            "quantiles": vec(self.quantiles), "thresholds": vec(self.thresholds),
            "quantile_effects": comps(self.quantile_effects), "quantile_values": comps(self.quantile_values),
            "distribution_effects": comps(self.distribution_effects), "cdf": comps(self.cdf),
            "cdf_rearranged": {key: vec(v) for key, v in self.cdf_rearranged.items()},
            "beta_a": [vec(r) for r in self.beta_a], "beta_b": [vec(r) for r in self.beta_b],
            "passes": [int(v) for v in np.asarray(self.passes).ravel()], "names": list(self.names),
            "n_a": self.n_a, "n_b": self.n_b, "n_failed": self.n_failed, "n_out_of_range": self.n_out_of_range,
            "n_thresholds_requested": self.n_thresholds_requested})


def _dr_tables(handle):
    """The four tables of a distribution-regression finish() -> (dicts of component lists, n_failed); frees the
    handle."""
    lib = N.lib()

    def table(t, parts):
        cs = []
        for i in range(lib.ob_results_count(handle, t)):
            c = N.ob_component()
            N.check(lib.ob_results_component(handle, t, i, C.byref(c)))
            cs.append(ComponentResult(c.name.decode(), c.estimate, c.std_err, c.t_stat, c.p_value, c.ci_lower,
                                      c.ci_upper))
        n = len(cs) // len(parts)
        return {p: cs[i * n:(i + 1) * n] for i, p in enumerate(parts)}

    try:
        eff = ("total", "composition", "structure")
        return (table(N.OB_DR_TABLE_QUANTILE_EFFECTS, eff), table(N.OB_DR_TABLE_QUANTILES, ("A", "B", "C")),
                table(N.OB_DR_TABLE_DISTRIBUTION_EFFECTS, eff), table(N.OB_DR_TABLE_CDF, ("AA", "BB", "AB", "BA")),
                int(lib.ob_results_n_failed(handle)), int(lib.ob_results_n_a(handle)), int(lib.ob_results_n_b(handle)))
    finally:
        lib.ob_results_free(handle)


def dr_finish_rows(point_row, thresholds, quantiles, rows, ok) -> DistributionDecompositionResults:
    """ob_dr_finish_rows (host only): the aggregation of ``decompose_distribution`` on given replicate rows (each
    ``dr_row_len(T, n_q)`` doubles) and their point row."""
    from .engine import dr_quantiles

    point = np.ascontiguousarray(point_row, dtype=np.float64)
    thr = np.ascontiguousarray(thresholds, dtype=np.float64)
    taus = np.ascontiguousarray(quantiles, dtype=np.float64)
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    ok = np.ascontiguousarray(ok, dtype=np.uint8)
    T, nq = len(thr), len(taus)
    if point.shape != (6 * nq + 7 * T + 1,) or rows.shape != (len(ok), len(point)):
        raise ValueError("point_row and rows must have 6 n_q + 7 T + 1 entries per row")
    h = C.c_void_p()
    N.check(N.lib().ob_dr_finish_rows(N.dp(point), T, nq, N.dp(rows), N.u8p(ok), len(ok), C.byref(h)))
    qe, qv, de, cdf, n_failed, n_a, n_b = _dr_tables(h)
    fr = point[6 * nq + 3 * T:6 * nq + 7 * T].reshape(4, T)
    re, edge = {}, np.zeros((3, nq), dtype=np.uint8)
    for i, key in enumerate(("AA", "BB", "AB")):
        _, re[key], edge[i] = dr_quantiles(fr[i], thr, taus)
    return DistributionDecompositionResults(
        quantiles=taus.copy(), thresholds=thr.copy(), quantile_effects=qe, quantile_values=qv,
        distribution_effects=de, cdf=cdf, cdf_rearranged=re, out_of_range=edge, n_a=n_a, n_b=n_b,
        n_failed=n_failed, n_out_of_range=int((edge != 0).sum()))


DENSITY_CURVES = ("density_a", "density_b", "density_counterfactual", "total", "composition", "structure")


@dataclass
class DensityCurve:
    """One curve of ``DensityDecompositionResults`` on its grid: per grid point the point estimate, the bootstrap
    standard error, the pointwise percentile interval and p-value, and the uniform 95 % band ``estimate -+
    band_critical * std_err`` (the band covers the whole curve at once; ``band_critical`` is the 95 % point of the
    replicates' largest standardised deviation over the grid)."""
    estimate: np.ndarray
    std_err: np.ndarray
    ci_lower: np.ndarray
    ci_upper: np.ndarray
    p_value: np.ndarray
    band_lower: np.ndarray
    band_upper: np.ndarray
    band_critical: float = float("nan")


@dataclass
class DensityDecompositionResults:
    """``OaxacaBuilder.decompose_density``: the DFL density decomposition (DiNardo, Fortin and Lemieux 1996) with
    bootstrap inference. ``density_a``, ``density_b`` and ``density_counterfactual`` (B reweighted to A's covariates)
    are the kernel densities on ``grid``; ``total`` = f_A - f_B, ``composition`` = f_C - f_B and ``structure`` =
    f_A - f_C their differences. Each is a ``DensityCurve``. ``gamma``: the point logit; ``effective_sample_size``:
    that of the reweighting factor on B's rows."""
    grid: np.ndarray
    bandwidth_a: float
    bandwidth_b: float
    density_a: DensityCurve
    density_b: DensityCurve
    density_counterfactual: DensityCurve
    total: DensityCurve
    composition: DensityCurve
    structure: DensityCurve
    gamma: np.ndarray = field(repr=False, default=None)
    effective_sample_size: float = float("nan")
    logit_passes: int = 0
    names: list = field(default_factory=list, repr=False)
    n_a: int = 0
    n_b: int = 0
    n_failed: int = 0

    def to_json(self) -> str:
        def vec(a):  # serde_json writes non-finite floats as null
            return [float(v) if np.isfinite(v) else None for v in np.asarray(a, dtype=np.float64).ravel()]

        def curve(c):
            d = {key: vec(v) for key, v in c.__dict__.items() if key != "band_critical"}
            d["band_critical"] = vec([c.band_critical])[0]
            return d

        out = {"grid": vec(self.grid), "bandwidth_a": self.bandwidth_a, "bandwidth_b": self.bandwidth_b}
        out.update({name: curve(getattr(self, name)) for name in DENSITY_CURVES})
        out.update({"gamma": vec(self.gamma), "effective_sample_size": vec([self.effective_sample_size])[0],
                    "logit_passes": self.logit_passes, "names": list(self.names), "n_a": self.n_a, "n_b": self.n_b,
                    "n_failed": self.n_failed})
        return json.dumps(out)

    def plot(self):
        """The three densities with their uniform bands on one matplotlib figure (returned), in the manner of
        ``DflResult.plot``."""
        try:
            import matplotlib.pyplot as plt
        except ImportError as e:
            raise ImportError("DensityDecompositionResults.plot() needs matplotlib, which is not installed") from e
        fig = plt.figure()
        ax = fig.gca()
        for c, label in ((self.density_a, "Group A"), (self.density_b, "Group B"),
                         (self.density_counterfactual, "Group B (Counterfactual)")):
            ax.plot(self.grid, c.estimate, label=label)
            ax.fill_between(self.grid, c.band_lower, c.band_upper, alpha=0.2)
        ax.legend()
        ax.set_title("DFL Decomposition: Density Estimates (uniform 95 % bands)")
        return fig


def _density_results(handle, grid, bandwidth_a, bandwidth_b, point, k, names=()) -> DensityDecompositionResults:
    """The two tables of a density finish() and the tail of the point row; frees the handle."""
    lib = N.lib()
    G = len(grid)

    def table(t):
        c = N.ob_component()
        rows = []
        for i in range(lib.ob_results_count(handle, t)):
            N.check(lib.ob_results_component(handle, t, i, C.byref(c)))
            rows.append((c.estimate, c.std_err, c.t_stat, c.p_value, c.ci_lower, c.ci_upper))
        return np.array(rows, dtype=np.float64).reshape(6, G, 6)

    try:
        cv, bd = table(N.OB_DENSITY_TABLE_CURVES), table(N.OB_DENSITY_TABLE_BANDS)
        n_failed, n_a, n_b = (int(lib.ob_results_n_failed(handle)), int(lib.ob_results_n_a(handle)),
                              int(lib.ob_results_n_b(handle)))
    finally:
        lib.ob_results_free(handle)
    curves = {name: DensityCurve(estimate=cv[i, :, 0].copy(), std_err=cv[i, :, 1].copy(), ci_lower=cv[i, :, 4].copy(),
                                 ci_upper=cv[i, :, 5].copy(), p_value=cv[i, :, 3].copy(), band_lower=bd[i, :, 4].copy(),
                                 band_upper=bd[i, :, 5].copy(), band_critical=float(bd[i, 0, 2]))
              for i, name in enumerate(DENSITY_CURVES)}
    return DensityDecompositionResults(
        grid=np.array(grid, dtype=np.float64), bandwidth_a=float(bandwidth_a), bandwidth_b=float(bandwidth_b),
        gamma=np.array(point[6 * G:6 * G + k]), effective_sample_size=float(point[6 * G + k]),
        logit_passes=int(point[6 * G + k + 1]) if np.isfinite(point[6 * G + k + 1]) else 0, names=list(names),
        n_a=n_a, n_b=n_b, n_failed=n_failed, **curves)


def density_finish_rows(point_row, k: int, grid, rows, ok, bandwidth_a: float = float("nan"),
                        bandwidth_b: float = float("nan")) -> DensityDecompositionResults:
    """ob_density_finish_rows (host only): the aggregation of ``decompose_density`` on given replicate rows (each
    ``density_row_len(k, G)`` doubles) and their point row."""
    point = np.ascontiguousarray(point_row, dtype=np.float64)
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    ok = np.ascontiguousarray(ok, dtype=np.uint8)
    G = len(grid)
    if point.shape != (6 * G + int(k) + 2,) or rows.shape != (len(ok), len(point)):
        raise ValueError("point_row and rows must have 6 G + k + 2 entries per row")
    h = C.c_void_p()
    N.check(N.lib().ob_density_finish_rows(N.dp(point), int(k), G, N.dp(rows), N.u8p(ok), len(ok), C.byref(h)))
    return _density_results(h, grid, bandwidth_a, bandwidth_b, point, int(k))


NOPO_COMPONENTS = ("total_gap", "composition", "unexplained", "unmatched_a", "unmatched_b", "matched_share_a",
                   "matched_share_b")


@dataclass
class NopoDecompositionResults:
    """``OaxacaBuilder.decompose_nopo``: Nopo's (2008) exact-matching decomposition, ``total_gap = composition +
    unexplained + unmatched_a + unmatched_b``. ``components`` holds the four terms, the gap and the two matched
    shares (the weight of a group that lies in the common support), each with its point estimate and the standard
    error, percentile interval and p-value over the bootstrap, in which the support is decided again per replicate.
    ``cells``: one dict per cell (``key``: the tuple of matching values, ``n_a``, ``n_b``, ``mean_a``, ``mean_b``,
    ``in_support``) in id order; ``row_cell``: the cell of every row of the frame (-1 outside A and B).
    ``relative``: with ``relative=True`` the five terms over ybar_B, computed per replicate."""
    components: dict
    cells: list = field(repr=False, default_factory=list)
    row_cell: np.ndarray = field(repr=False, default=None)
    relative: dict = field(default_factory=dict)
    n_cells: int = 0
    n_support_cells: int = 0
    n_a: int = 0
    n_b: int = 0
    n_failed: int = 0

    def __getattr__(self, name):  # the seven components by name
        if name in NOPO_COMPONENTS:
            return self.__dict__["components"][name]
        raise AttributeError(name)

    def to_json(self) -> str:
        def fix(v):  # serde_json writes non-finite floats as null
            if isinstance(v, (bytes, np.bytes_)):
                return v.decode("utf-8", "replace")
            if isinstance(v, (str, bool)):
                return v
            if isinstance(v, (int, np.integer)):
                return int(v)
            return float(v) if np.isfinite(v) else None

        def comps(d):
            return {key: {k: fix(v) for k, v in c.__dict__.items()} for key, c in d.items()}

        return json.dumps({
            "components": comps(self.components), "relative": comps(self.relative),
            "cells": [{**{k: fix(v) for k, v in c.items() if k != "key"}, "key": [fix(v) for v in c["key"]]}
                      for c in self.cells],
            "row_cell": [] if self.row_cell is None else [int(v) for v in self.row_cell], "n_cells": self.n_cells,
            "n_support_cells": self.n_support_cells, "n_a": self.n_a, "n_b": self.n_b, "n_failed": self.n_failed})


def _nopo_components(handle):
    """Table 0 of a matching decomposition's finish() -> (components by name, n_failed, n_a, n_b); frees the
    handle."""
    lib = N.lib()
    try:
        out = {}
        for i in range(lib.ob_results_count(handle, 0)):
            c = N.ob_component()
            N.check(lib.ob_results_component(handle, 0, i, C.byref(c)))
            out[c.name.decode()] = ComponentResult(c.name.decode(), c.estimate, c.std_err, c.t_stat, c.p_value,
                                                   c.ci_lower, c.ci_upper)
        return out, int(lib.ob_results_n_failed(handle)), int(lib.ob_results_n_a(handle)), int(lib.ob_results_n_b(handle))
    finally:
        lib.ob_results_free(handle)


def _nopo_relative(point, rows, ok) -> dict:
    """The five terms over ybar_B (row entry 6), per replicate, through ``ob_bootstrap_stats``."""
    from .engine import bootstrap_stats

    rows = np.asarray(rows)[np.asarray(ok).astype(bool)]
    out = {}
    for i, name in enumerate(NOPO_COMPONENTS[:5]):
        est = float(point[i] / point[6])
        se, p, (lo, hi) = bootstrap_stats(rows[:, i] / rows[:, 6], est)
        out[name] = ComponentResult(name, est, se, (est / se if abs(se) > 1e-9 else 0.0), p, lo, hi)
    return out


def nopo_finish_rows(point_row, rows, ok) -> NopoDecompositionResults:
    """ob_nopo_finish_rows (host only): the aggregation of ``decompose_nopo`` on given replicate rows (each
    ``nopo_row_len()`` doubles) and their point row."""
    point = np.ascontiguousarray(point_row, dtype=np.float64)
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    ok = np.ascontiguousarray(ok, dtype=np.uint8)
    rl = N.lib().ob_nopo_row_len()
    if point.shape != (rl,) or rows.shape != (len(ok), rl):
        raise ValueError(f"point_row and rows must have {rl} entries per row")
    h = C.c_void_p()
    N.check(N.lib().ob_nopo_finish_rows(N.dp(point), N.dp(rows), N.u8p(ok), len(ok), C.byref(h)))
    comps, n_failed, n_a, n_b = _nopo_components(h)
    return NopoDecompositionResults(components=comps, n_support_cells=int(point[12]), n_a=n_a, n_b=n_b,
                                    n_failed=n_failed)


def nopo_cells(dataframe, outcome: str, group: str, reference_group: str, predictors=(), categorical_predictors=(),
               bins=None):
    """ob_nopo_cells (host only): (row_cell, n_cells) of ``decompose_nopo`` over the frame: the cell id of every row
    (-1 for a row of neither group), ids numbering the distinct tuples of matching values in lexicographic order."""
    b = OaxacaBuilder(dataframe, outcome, group, reference_group).predictors(predictors)
    return b.categorical_predictors(categorical_predictors)._nopo_binned(bins)._nopo_cells()


@dataclass
class TobitDecompositionResults:
    """``OaxacaBuilder.decompose_tobit``: the Tobit decomposition of a censored outcome (Bauer and Sinning 2008,
    2010). The component objects are ``OaxacaResults``' (estimate, standard error, percentile interval, p-value over
    the bootstrap, in which both censored-normal fits are redone per replicate). ``total_gap`` is the predicted gap
    M[A][A] - M[B][B] in the conditional means of the observed (censored) outcome, ``raw_gap`` the gap in the groups'
    observed means; ``expected_values`` maps (group, coefficients) to the four M; ``latent`` decomposes the gap in
    the uncensored outcome x'beta (explained, unexplained, total_gap): what the gap would be without the limits.
    ``censored_share`` maps (group, side) to the weighted share of rows at a limit."""
    total_gap: float
    raw_gap: float
    two_fold: list
    three_fold: list
    latent: list
    detailed_explained: list
    detailed_unexplained: list
    expected_values: dict
    censored_share: dict
    beta_a: np.ndarray = field(repr=False)
    beta_b: np.ndarray = field(repr=False)
    sigma_a: float = 0.0
    sigma_b: float = 0.0
    xa_mean: np.ndarray = field(repr=False, default=None)
    xb_mean: np.ndarray = field(repr=False, default=None)
    names: list = field(repr=False, default_factory=list)
    lower: float | None = None
    upper: float | None = None
    passes: tuple = (0, 0)
    n_a: int = 0
    n_b: int = 0
    n_failed: int = 0

    def to_json(self) -> str:
        def fix(v):  # serde_json writes non-finite floats as null
            return v if v is None or isinstance(v, str) or np.isfinite(v) else None

        def comps(cs):
            return [{k: fix(v) for k, v in c.__dict__.items()} for c in cs]

        return json.dumps({
            "total_gap": fix(self.total_gap), "raw_gap": fix(self.raw_gap), "two_fold": comps(self.two_fold),
            "three_fold": comps(self.three_fold), "latent": comps(self.latent),
            "detailed_explained": comps(self.detailed_explained),
            "detailed_unexplained": comps(self.detailed_unexplained),
            "expected_values": {f"{g}|{b}": fix(v) for (g, b), v in self.expected_values.items()},
            "censored_share": {f"{g}|{side}": fix(v) for (g, side), v in self.censored_share.items()},
            "names": list(self.names), "beta_a": [fix(float(v)) for v in self.beta_a],
            "beta_b": [fix(float(v)) for v in self.beta_b], "sigma_a": fix(self.sigma_a), "sigma_b": fix(self.sigma_b),
            "lower": fix(self.lower), "upper": fix(self.upper), "passes": [int(v) for v in self.passes],
            "n_a": self.n_a, "n_b": self.n_b, "n_failed": self.n_failed})


def _tobit_results(res, point, lower=None, upper=None) -> TobitDecompositionResults:
    """The results of a Tobit run from finish()'s tables (``res``: an ``OaxacaResults`` whose selection table holds
    the latent terms) and the point row."""
    k = (len(point) - 23) // 7
    tail = point[6 + 2 * k:]
    sc = tail[5 * k:]
    keys = [(g, b) for g in ("A", "B") for b in ("beta_a", "beta_b")]
    sides = [(g, side) for g in ("A", "B") for side in ("left", "right")]
    return TobitDecompositionResults(
        total_gap=float(point[5]), raw_gap=float(sc[7] - sc[8]), two_fold=res.two_fold.aggregate,
        three_fold=res.three_fold.aggregate, latent=res.two_fold.detailed_selection,
        detailed_explained=res.two_fold.detailed_explained, detailed_unexplained=res.two_fold.detailed_unexplained,
        expected_values={key: float(v) for key, v in zip(keys, sc[3:7])},
        censored_share={key: float(v) for key, v in zip(sides, sc[11:15])},
        beta_a=tail[:k].copy(), beta_b=tail[k:2 * k].copy(), sigma_a=float(sc[9]), sigma_b=float(sc[10]),
        xa_mean=tail[2 * k:3 * k].copy(), xb_mean=tail[3 * k:4 * k].copy(),
        names=[c.name for c in res.two_fold.detailed_explained], lower=lower, upper=upper,
        passes=(int(sc[15]), int(sc[16])), n_a=res.n_a, n_b=res.n_b, n_failed=res.n_failed)


def tobit_finish_rows(point_row, k: int, rows, ok) -> TobitDecompositionResults:
    """ob_tobit_finish_rows (host only): the aggregation of ``decompose_tobit`` on given replicate rows (each
    ``tobit_row_len(k)`` doubles) and their point row; the detailed components are named x0 .. x<k-1>."""
    point = np.ascontiguousarray(point_row, dtype=np.float64)
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    ok = np.ascontiguousarray(ok, dtype=np.uint8)
    if point.shape != (6 + 7 * int(k) + 17,) or rows.shape != (len(ok), len(point)):
        raise ValueError("point_row and rows must have 6 + 7 k + 17 entries per row")
    h = C.c_void_p()
    N.check(N.lib().ob_tobit_finish_rows(N.dp(point), int(k), N.dp(rows), N.u8p(ok), len(ok), C.byref(h)))
    return _tobit_results(_results_from_c(h), point)


def _jackknife_out(k: int):
    c = 6 + 2 * k
    bufs = (np.zeros(c), np.zeros((2, c, 3)), np.zeros((c, 3)))
    o = N.ob_jackknife_out()
    o.capacity = c
    o.point, o.sums, o.stats = (N.dp(b) for b in bufs)
    return o, bufs


def _jackknife_result(o, bufs, names) -> JackknifeResult:
    k = (o.n_components - 6) // 2
    names = list(names) if names else [f"x{j}" for j in range(k)]
    full = (["explained", "unexplained", "endowments", "coefficients", "interaction", "total_gap"]
            + [f"explained:{n}" for n in names] + [f"unexplained:{n}" for n in names])
    point, sums, stats = bufs
    return JackknifeResult(full, point.copy(), stats[:, 0].copy(), stats[:, 1].copy(), stats[:, 2].copy(),
                           (int(o.n_used[0]), int(o.n_used[1])), (int(o.n_dropped[0]), int(o.n_dropped[1])),
                           sums.copy())


_JACK_TABLES = {"two_fold": N.OB_TABLE_TWO_FOLD, "three_fold": N.OB_TABLE_THREE_FOLD,
                "detailed_explained": N.OB_TABLE_DETAILED_EXPLAINED,
                "detailed_unexplained": N.OB_TABLE_DETAILED_UNEXPLAINED}


def _results_from_c(handle, jackknife: bool = False) -> OaxacaResults:
    lib = N.lib()

    def jack():
        out = {}
        for tname, t in _JACK_TABLES.items():
            for i in range(lib.ob_results_count(handle, t)):
                c = N.ob_component()
                N.check(lib.ob_results_component(handle, t, i, C.byref(c)))
                v = (C.c_double * 5)()
                N.check(lib.ob_results_jackknife(handle, t, i, v))
                out[(tname, c.name.decode())] = {"accel": v[0], "std_err": v[1], "bias": v[2], "z0": v[3],
                                                 "flag": int(v[4])}
        return out

    def table(t):
        out = []
        for i in range(lib.ob_results_count(handle, t)):
            c = N.ob_component()
            N.check(lib.ob_results_component(handle, t, i, C.byref(c)))
            out.append(ComponentResult(c.name.decode(), c.estimate, c.std_err, c.t_stat, c.p_value,
                                       c.ci_lower, c.ci_upper))
        return out

    def vec(w):
        ptr = C.POINTER(C.c_double)()
        n = C.c_int64()
        N.check(lib.ob_results_vector(handle, w, C.byref(ptr), C.byref(n)))
        return N.array_copy(ptr, (n.value,))

    try:
        nc = int(lib.ob_results_n_clusters(handle))
        return OaxacaResults(
            n_clusters=None if nc < 0 else nc,
            total_gap=lib.ob_results_total_gap(handle),
            two_fold=TwoFoldResults(table(N.OB_TABLE_TWO_FOLD), table(N.OB_TABLE_DETAILED_EXPLAINED),
                                    table(N.OB_TABLE_DETAILED_UNEXPLAINED), table(N.OB_TABLE_DETAILED_SELECTION)),
            three_fold=DecompositionDetail(table(N.OB_TABLE_THREE_FOLD), []),
            n_a=int(lib.ob_results_n_a(handle)), n_b=int(lib.ob_results_n_b(handle)),
            residuals=vec(N.OB_VEC_RESIDUALS), xa_mean=vec(N.OB_VEC_XA_MEAN), xb_mean=vec(N.OB_VEC_XB_MEAN),
            beta_star=vec(N.OB_VEC_BETA_STAR), n_failed=int(lib.ob_results_n_failed(handle)),
            jackknife=jack() if jackknife else None)
    finally:
        lib.ob_results_free(handle)


def _remedy_result(handle, info, contributions: bool, defensible: bool = False) -> OptimizationResult:
    """The adjustments and the fair-wage model of a remediation handle (``ob_remedy_results_get`` / ``_model``);
    ``info`` is its ``ob_remedy_info`` or ``ob_defend_info``. ``defensible``: the handle carries the defensibility
    flags, and every adjustment gets its verdict and message."""
    lib = N.lib()
    pi, pf = C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)()
    pd = [C.POINTER(C.c_double)() for _ in range(6)]
    N.check(lib.ob_remedy_results_get(handle, C.byref(pi), *[C.byref(p) for p in pd], None, None))
    if defensible:
        N.check(lib.ob_remedy_results_defensible(handle, C.byref(pf)))
    k, pn = C.c_int32(), C.POINTER(C.c_char_p)()
    pb, pc = C.POINTER(C.c_double)(), C.POINTER(C.c_double)()
    N.check(lib.ob_remedy_results_model(handle, C.byref(k), C.byref(pn), C.byref(pb), C.byref(pc)))
    names = [pn[j].decode() for j in range(k.value)]
    adjustments = []
    for i in range(int(info.n_adjustments)):
        con = [Contribution(names[j], pc[i * k.value + j]) for j in range(k.value)] if contributions and pc else []
        verdict = (bool(pf[i]), defensibility_message(bool(pf[i]), pd[2][i], pd[4][i])) if defensible else ()
        adjustments.append(Adjustment(int(pi[i]), *[p[i] for p in pd], con, *verdict))
    return OptimizationResult(
        adjustments=adjustments, total_cost=info.total_cost, original_gap=info.original_gap, new_gap=info.new_gap,
        original_unexplained_gap=info.original_unexplained_gap, new_unexplained_gap=info.new_unexplained_gap,
        required_budget=info.required_budget, model_coefficients=[Contribution(names[j], pb[j]) for j in range(k.value)])


def parse_formula(formula: str):
    """formula.rs:12-58: 'y ~ a + b + C(cat)' -> (outcome, predictors, categorical)."""
    parts = formula.split("~")
    if len(parts) != 2:
        raise N.OaxacaError(N.OB_E_GROUP, "Invalid group variable: Invalid formula format. Expected "
                                          f"'outcome ~ predictors', got '{formula}'")
    outcome = parts[0].strip()
    if not outcome:
        raise N.OaxacaError(N.OB_E_GROUP, "Invalid group variable: Outcome variable is missing")
    preds, cats = [], []
    for term in parts[1].split("+"):
        term = term.strip()
        if not term:
            continue
        if term.startswith("C(") and term.endswith(")"):
            cats.append(term[2:-1].strip())
        elif term.startswith("factor(") and term.endswith(")"):
            cats.append(term[7:-1].strip())
        else:
            preds.append(term)
    if not preds and not cats:
        raise N.OaxacaError(N.OB_E_GROUP, "Invalid group variable: No predictors specified")
    return outcome, preds, cats


def _set_names(cfg, field: str, names):
    """``cfg.<field>`` = the names as a ``char**`` and ``cfg.n_<field>`` = their number -> the array behind the
    pointer, which goes into ``_frame_call``'s ``keep``."""
    ptr, arr = N.strs(names)
    setattr(cfg, field, ptr)
    setattr(cfg, "n_" + field, len(names))
    return arr


# How an entry point that takes a frame gets its context. The policy is part of a method's
# behaviour on a machine without a GPU: which error comes first.
CONTEXT_FIRST = "context-first"      # N.context(device) before the call: the missing device is the first error
ARGUMENTS_FIRST = "arguments-first"  # engine.with_context: the call's argument errors come before the missing device
HOST_ONLY = "host-only"              # the entry point takes no context


def _frame_call(symbol: str, frame, cfg, keep, *args, policy: str, device=None, ctx=None, handles=None):
    """``lib.<symbol>(ctx, cols, n_cols, n_rows, &cfg, *args, &handle)``, checked -> the handle.
    ``keep``: the arrays behind the ``char**`` fields of ``cfg`` and of ``args``; they are held here until the call
    has returned. ``cfg`` None: an entry point without a config struct. ``policy``: see above; an explicit ``ctx``
    (a rank context) is used as it is under either policy. ``handles`` = n: the entry point fills an array of n
    handles, returned as a list; 0: it returns none."""
    from .engine import with_context

    fn = getattr(N.lib(), symbol)
    cols, ncol, nrow = frame.as_c()
    hs = (C.c_void_p * (1 if handles is None else handles))()
    tail = (() if cfg is None else (C.byref(cfg),)) + args + ((C.cast(hs, C.POINTER(C.c_void_p)),) if len(hs) else ())
    if policy == HOST_ONLY:
        N.check(fn(cols, ncol, nrow, *tail))
    elif ctx is not None:
        N.check(fn(ctx, cols, ncol, nrow, *tail))
    elif policy == ARGUMENTS_FIRST:
        with_context(lambda c: fn(c, cols, ncol, nrow, *tail), device)
    else:
        assert policy == CONTEXT_FIRST, policy
        N.check(fn(N.context(device), cols, ncol, nrow, *tail))
    del keep  # held until here
    out = [C.c_void_p(h) for h in hs]
    return out[0] if handles is None else out


class OaxacaBuilder:
    """builder.rs:37-757. Defaults: bootstrap_reps 20, reference coefficients GroupA."""

    def __init__(self, dataframe, outcome: str, group: str, reference_group: str):
        self._frame = dataframe if isinstance(dataframe, Frame) else Frame(dataframe)
        self.outcome, self.group, self.reference_group = outcome, group, reference_group
        self._predictors: list[str] = []
        self._categorical: list[str] = []
        self._bootstrap_reps = 20
        self._ref = ReferenceCoefficients.GroupA
        self._normalize: list[str] = []
        self._weights: str | None = None
        self._selection: str | None = None
        self._selection_predictors: list[str] = []
        self._seed: int | None = None
        self._device: int | None = None
        self._ctx = None  # an explicit ob_ctx (distributed.fit_sharded's rank context)
        self._cluster: str | None = None
        self._cluster_stratified = False

    @classmethod
    def from_formula(cls, dataframe, formula: str, group: str, reference_group: str):
        outcome, preds, cats = parse_formula(formula)
        b = cls(dataframe, outcome, group, reference_group)
        b._predictors, b._categorical = preds, cats
        return b

    def predictors(self, names):
        self._predictors = [str(n) for n in names]
        return self

    def categorical_predictors(self, names):
        self._categorical = [str(n) for n in names]
        return self

    def bootstrap_reps(self, reps: int):
        self._bootstrap_reps = int(reps)
        return self

    def reference_coefficients(self, ref):
        self._ref = ReferenceCoefficients(ref)
        return self

    def normalize(self, names):
        self._normalize = [str(n) for n in names]
        return self

    def weights(self, name: str):
        self._weights = name
        return self

    def cluster(self, column: str | None, stratified: bool = False):
        """Extension: resample whole clusters (the values of ``column``, strings or integers) instead of rows
        in ``run()``, ``prepare()``, ``decompose_quantile(s)``: Stata's ``bootstrap, cluster()``. Joint mode
        draws C clusters from all C, both groups sharing the counts; ``stratified=True`` draws C_A from group
        A's clusters and C_B from B's (every cluster must lie in one group). Point estimates do not change."""
        self._cluster = None if column is None else str(column)
        self._cluster_stratified = bool(stratified)
        return self

    def _cluster_config(self):
        cc = N.ob_cluster_config()
        cc.column = self._cluster.encode()
        cc.stratified = 1 if self._cluster_stratified else 0
        return cc

    def _refuse_clustered(self, what: str):
        if self._cluster is not None:
            raise N.OaxacaError(N.OB_E_UNSUPPORTED, f"cluster bootstrap: {what} is outside its scope "
                                                    "(delete-one-row is the wrong jackknife under clustering)")

    def heckman_selection(self, outcome: str, predictors):
        self._selection = outcome
        self._selection_predictors = list(predictors)
        return self

    def seed(self, seed: int | None):
        """Extension: fix the OBRS-3 stream (the reference is unseeded; None = fresh entropy)."""
        self._seed = None if seed is None else int(seed) & ((1 << 64) - 1)
        return self

    def device(self, device: int | None):
        self._device = device
        return self

    def _config(self):
        """(ob_builder_config, the arrays its ``char**`` fields point into)."""
        cfg = N.ob_builder_config()
        cfg.outcome, cfg.group, cfg.reference_group = (self.outcome.encode(), self.group.encode(),
                                                       self.reference_group.encode())
        keep = [_set_names(cfg, field, names) for field, names in (
            ("predictors", self._predictors), ("categorical", self._categorical), ("normalize", self._normalize),
            ("selection_predictors", self._selection_predictors))]
        cfg.weights = self._weights.encode() if self._weights else None
        cfg.selection_outcome = self._selection.encode() if self._selection else None
        cfg.bootstrap_reps = self._bootstrap_reps
        cfg.reference_coeffs = int(self._ref)
        cfg.has_seed = 0 if self._seed is None else 1
        cfg.seed = 0 if self._seed is None else self._seed
        return cfg, keep

    def _call(self, symbol: str, *args, policy: str, ctx=None, handles=None, keep=(), clustered: bool = False):
        """``_frame_call`` on this builder's frame, configuration and device. ``clustered``: the entry point takes the
        cluster configuration after the builder's. ``keep``: arrays behind ``char**`` arguments of ``args``."""
        cfg, held = self._config()
        if clustered:
            cc = self._cluster_config()
            args = (C.byref(cc),) + args
        return _frame_call(symbol, self._frame, cfg, (held, keep), *args, policy=policy, device=self._device, ctx=ctx,
                           handles=handles)

    def _prepared(self, handle) -> "PreparedRun":
        return PreparedRun(handle, self._bootstrap_reps, N.resolve_device(self._device))

    def get_data_matrices(self):
        """builder.rs:252-291 -> (X_A, y_A, X_B, y_B, names); X includes the intercept column."""
        lib = N.lib()
        h = self._call("ob_builder_data_matrices", policy=HOST_ONLY)
        try:
            na, nb, k = C.c_int64(), C.c_int64(), C.c_int32()
            N.check(lib.ob_matrices_dims(h, C.byref(na), C.byref(nb), C.byref(k)))
            ptrs = [C.POINTER(C.c_double)() for _ in range(4)]
            N.check(lib.ob_matrices_get(h, *[C.byref(p) for p in ptrs]))

            def mat(p, n, kk):
                if n * kk == 0:
                    return np.zeros((n, kk))
                return np.ctypeslib.as_array(p, shape=(kk, n)).T.copy()

            xa, xb = mat(ptrs[0], na.value, k.value), mat(ptrs[2], nb.value, k.value)
            ya, yb = N.array_copy(ptrs[1], (na.value,)), N.array_copy(ptrs[3], (nb.value,))
            names = [lib.ob_matrices_name(h, i).decode() for i in range(k.value)]
            return xa, ya, xb, yb, names
        finally:
            lib.ob_matrices_free(h)

    def vif(self) -> list:
        """The variance inflation factors of this builder's own design (``VifResult`` per column): the
        predictors and the dummies of ``get_data_matrices()`` without the intercept, over the cleaned
        frame with both groups stacked (A's rows, then B's). The check to make before ``run()``:
        collinear columns make the detailed terms meaningless."""
        from .engine import vif

        xa, _, xb, _, names = self.get_data_matrices()
        scores = vif(np.vstack([xa, xb])[:, 1:], device=self._device)
        return [VifResult(nm, float(s)) for nm, s in zip(names[1:], scores)]

    def optimize(self, budget: float = 0.0, target: str = "reference", strategy: str = "greedy",
                 min_gap_pct: float = 0.0, forensic_mode: bool = False, adjust_both_groups: bool = False,
                 confidence_level: float = 0.95, range_target: str = "midpoint",
                 contributions: bool = False) -> OptimizationResult:
        """engine/src/analysis.rs:309-869 (optimize_inner) on the MI355X engine (``ob_remedy_run``): the
        fair-wage model of the reference group (``target="reference"``) or of both groups (``"pooled"``), a
        prediction interval per employee, and the greedy or equitable allocation of ``budget`` (0: what
        closes every eligible gap) over the target group's positive gaps. ``contributions`` fills each
        adjustment's ``contributions`` (x_ij beta_j per design column). ``last_remedy_info`` keeps the
        call's ``ob_remedy_info`` (counts, z, sigma squared, HIP-event times per pass)."""
        if target not in N.OB_REMEDY_TARGETS or strategy not in N.OB_REMEDY_STRATEGIES \
                or range_target not in N.OB_REMEDY_RANGE_TARGETS:
            raise ValueError("target: reference|pooled, strategy: greedy|equitable, range_target: midpoint|lower|upper")
        rq = N.ob_remedy_request(float(budget), float(min_gap_pct), float(confidence_level),
                                 N.OB_REMEDY_STRATEGIES[strategy], N.OB_REMEDY_RANGE_TARGETS[range_target],
                                 int(bool(forensic_mode)), int(bool(adjust_both_groups)))
        h = self._call("ob_remedy_run", C.byref(rq), N.OB_REMEDY_TARGETS[target], int(bool(contributions)),
                       policy=ARGUMENTS_FIRST)
        try:
            info = N.ob_remedy_info()
            N.check(N.lib().ob_remedy_results_info(h, C.byref(info)))
            self.last_remedy_info = N.struct_dict(info)
            return _remedy_result(h, info, contributions)
        finally:
            N.lib().ob_remedy_results_free(h)

    def efficient_frontier(self, steps: int = 50, max_budget: float | None = None) -> list:
        """engine/src/analysis.rs:871-1153 (calculate_efficient_frontier_inner) on the MI355X engine
        (``ob_remedy_frontier``): ``steps + 1`` ``FrontierPoint``s, the first at budget 0, each the group
        dummy's t statistic in the pooled regression after the greedy raises that budget pays for.
        ``max_budget`` defaults to 1.1 times the total need. ``last_frontier_ms`` keeps the HIP-event ms of the
        two passes (X'Y, rss)."""
        s = max(int(steps), 0) + 1
        b, t, p, ms = np.zeros(s), np.zeros(s), np.zeros(s), np.zeros(2)
        sig = np.zeros(s, dtype=np.int32)
        self._call("ob_remedy_frontier", int(steps), float("nan") if max_budget is None else float(max_budget),
                   N.dp(b), N.dp(t), N.dp(p), N.i32p(sig), N.dp(ms), policy=CONTEXT_FIRST, handles=0)
        self.last_frontier_ms = {"xty_ms": float(ms[0]), "rss_ms": float(ms[1])}
        return [FrontierPoint(float(b[i]), float(t[i]), float(p[i]), bool(sig[i])) for i in range(s)]

    def check_defensibility(self, adjustments, confidence_level: float = 0.95,
                            contributions: bool = True) -> OptimizationResult:
        """engine/src/defensibility.rs (check_defensibility_inner) on the MI355X engine
        (``ob_remedy_defend``): every proposed raise scored against the reference group's fair-wage
        interval, and the gaps before and after. ``adjustments``: ``Adjustment``s (as ``optimize()``
        returns them, perhaps edited), ``(index, value)`` or ``(index, value, overrides)`` tuples, or dicts
        with ``index``, ``value`` and ``predictor_overrides``. An override replaces a numeric predictor of
        that row before the model is fit ("what if this person were re-levelled"); per row the last
        adjustment that carries overrides replaces every earlier set as a whole, and an override of a
        reference-group row changes the model for everyone, as in the reference. Where several
        adjustments name one row, all are returned and the first decides the row's new wage in the gaps.
        An index outside the frame is skipped (``last_defend_info["n_skipped"]``). The reference
        hard-wires ``confidence_level`` 0.95. ``last_defend_info`` keeps the call's ``ob_defend_info``."""
        prop = _proposed(adjustments)
        m = len(prop)
        idx = np.array([p[0] for p in prop], dtype=np.int64)
        val = np.array([p[1] for p in prop], dtype=np.float64)
        flat = [(j, name, v) for j, p in enumerate(prop) for name, v in p[2].items()]
        opos = np.array([f[0] for f in flat], dtype=np.int64)
        oval = np.array([f[2] for f in flat], dtype=np.float64)
        onames, keep_names = N.strs([f[1] for f in flat])
        h = self._call("ob_remedy_defend", N.i64p(idx), N.dp(val), m, N.i64p(opos), onames, N.dp(oval), len(flat),
                       float(confidence_level), int(bool(contributions)), policy=ARGUMENTS_FIRST, keep=keep_names)
        try:
            info = N.ob_defend_info()
            N.check(N.lib().ob_remedy_results_defend_info(h, C.byref(info)))
            self.last_defend_info = {**N.struct_dict(info), "sums": list(info.sums)}
            return _remedy_result(h, info, contributions, defensible=True)
        finally:
            N.lib().ob_remedy_results_free(h)

    def verify_adjustments(self, adjustments, three_fold: bool = False) -> "DecompositionResult":
        """engine/src/analysis.rs:40-96 (verify_inner) on the MI355X engine (``ob_remedy_verify``): the
        raises are added to a copy of the outcome one by one in request order (two raises of one row give
        ``(w + a1) + a2``) and the decomposition runs again with this builder's configuration as it stands
        (reference coefficients, replicates, seed, weights, normalisation). The gaps come from the two-fold
        table, or from the three-fold one with ``interaction_gap`` when ``three_fold`` is set (the detailed
        lists and ``unexplained_standard_error`` are two-fold only). An index outside the frame raises
        ``OB_E_INVALID``. The reference's ``quantile`` switch is not built."""
        from .engine import remedy_apply_adjustments

        prop = _proposed(adjustments)
        idx = np.array([p[0] for p in prop], dtype=np.int64)
        val = np.array([p[1] for p in prop], dtype=np.float64)
        res = _results_from_c(self._call("ob_remedy_verify", N.i64p(idx), N.dp(val), len(prop), policy=ARGUMENTS_FIRST))
        # run_decomposition_on_df's summary (analysis.rs:102-140) of the adjusted wages
        kind, wage, valid = self._frame.columns[self.outcome]
        adjusted = remedy_apply_adjustments(wage, idx, val, valid)
        ok = np.ones(len(adjusted), dtype=bool) if valid is None else valid.astype(bool)
        gkind, groups, _ = self._frame.columns[self.group]
        ref = self.reference_group.encode()
        in_a = np.array([g == ref for g in groups], dtype=bool) if gkind == N.OB_COL_STR else np.zeros(len(adjusted), bool)
        mean = lambda mask: float(np.mean(adjusted[mask & ok])) if (mask & ok).any() else 0.0  # noqa: E731
        summary = DataSummary(len(adjusted), int(in_a.sum()), int((~in_a).sum()), mean(in_a), mean(~in_a))
        total = res.total_gap
        comp = {c.name: c for c in (res.three_fold.aggregate if three_fold else res.two_fold.aggregate)}
        exp_ = comp.get("endowments" if three_fold else "explained")
        une = comp.get("coefficients" if three_fold else "unexplained")
        inter = comp.get("interaction") if three_fold else None
        e, u = (exp_.estimate if exp_ else 0.0), (une.estimate if une else 0.0)

        def pct(x):  # analysis.rs:299-301; IEEE division, so a zero gap gives inf or NaN as there
            with np.errstate(divide="ignore", invalid="ignore"):
                return float((np.float64(x) / np.float64(total)) * 100.0)

        return DecompositionResult(
            total_gap=total, explained_gap=e, unexplained_gap=u,
            interaction_gap=inter.estimate if inter else None,
            explained_percentage=pct(e), unexplained_percentage=pct(u),
            interaction_percentage=pct(inter.estimate) if inter else None,
            detailed_explained=[] if three_fold else list(res.two_fold.detailed_explained),
            detailed_unexplained=[] if three_fold else list(res.two_fold.detailed_unexplained),
            data_summary=summary,
            unexplained_standard_error=None if three_fold or une is None else une.std_err, results=res)

    def decompose(self, three_fold: bool = False) -> "DecompositionResult":
        """engine/src/analysis.rs:8-38 (decompose_inner): ``verify_adjustments`` with no adjustments."""
        return self.verify_adjustments([], three_fold)

    def run(self) -> OaxacaResults:
        """builder.rs:787-951 on the MI355X engine."""
        if self._cluster is not None:
            return _results_from_c(self._call("ob_builder_run_clustered", policy=CONTEXT_FIRST, clustered=True))
        return _results_from_c(self._call("ob_builder_run", policy=CONTEXT_FIRST))

    def run_bca(self, confidence_level: float = 0.95) -> OaxacaResults:
        """``run()`` with every component's interval replaced by the bias-corrected and accelerated (BCa)
        one: z0 from the replicates, the acceleration from one leave-one-out pass over the panel. Estimates,
        standard errors and p-values are those of ``run()`` with the same seed; ``.jackknife`` holds, per
        (table, name), the acceleration, the jackknife standard error and bias, z0 and the BCa flag."""
        self._refuse_clustered("run_bca")
        h = self._call("ob_builder_run_bca", float(confidence_level), policy=CONTEXT_FIRST)
        return _results_from_c(h, jackknife=True)

    def jackknife(self) -> "JackknifeResult":
        """The leave-one-out pass alone: acceleration, jackknife standard error and bias of every component."""
        self._refuse_clustered("jackknife")
        with self.prepare() as pr:
            return pr.jackknife()

    def _require_clustered(self, what: str):
        if self._cluster is None:
            raise N.OaxacaError(N.OB_E_INVALID, f"{what}: this builder is not clustered (call .cluster(column) first)")

    def run_cluster_bca(self, confidence_level: float = 0.95) -> OaxacaResults:
        """The clustered ``run()`` with every component's interval replaced by the BCa one: z0 from the cluster
        bootstrap's replicates, the acceleration from one delete-one-cluster pass. Estimates,
        standard errors and p-values are those of ``run()`` with the same seed; ``.jackknife`` holds, per
        (table, name), the acceleration, the cluster jackknife standard error and bias, z0 and the BCa flag."""
        self._require_clustered("run_cluster_bca")
        h = self._call("ob_builder_run_clustered_bca", float(confidence_level), policy=CONTEXT_FIRST, clustered=True)
        return _results_from_c(h, jackknife=True)

    def cluster_jackknife(self) -> "JackknifeResult":
        """The delete-one-cluster pass alone (Stata's ``jackknife, cluster()``): acceleration, cluster-robust
        jackknife standard error and bias of every component. ``n_used`` / ``n_dropped`` count clusters per
        stratum: all clusters as stratum 0 in joint mode, A's and B's clusters in stratified mode."""
        self._require_clustered("cluster_jackknife")
        with self.prepare() as pr:
            return pr.cluster_jackknife()

    def decompose_quantile(self, quantile: float, refit: bool = False) -> OaxacaResults:
        """builder.rs:711-757: RIF-regression decomposition at ``quantile``. ``refit=True``: see
        ``decompose_quantiles``."""
        if refit:
            return self.decompose_quantiles([float(quantile)], refit=True)[0]
        if self._cluster is not None:
            return self.decompose_quantiles([float(quantile)])[0]
        return _results_from_c(self._call("ob_builder_decompose_quantile", float(quantile), policy=CONTEXT_FIRST))

    def prepare_quantiles_refit(self, quantiles) -> "PreparedRun":
        """ob_builder_prepare_quantiles_refit: a handle whose replicates refit the quantile, the bandwidth, the
        density and so the RIF on every resample. ``boot`` returns rows (T, n_reps, row_len) and
        ok (T, n_reps); ``point_row()`` is (T * row_len,). Each group's rows stand in stable ascending order of y,
        so the same seed draws other rows than the fixed-RIF run."""
        taus = np.ascontiguousarray(quantiles, dtype=np.float64)
        if taus.ndim != 1 or taus.size == 0:
            raise ValueError("quantiles must be a non-empty 1-D sequence")
        if self._cluster is not None:
            raise N.OaxacaError(N.OB_E_UNSUPPORTED, "quantile refit: the cluster bootstrap is outside its scope")
        return self._prepared(self._call("ob_builder_prepare_quantiles_refit", N.dp(taus), int(taus.size),
                                         policy=ARGUMENTS_FIRST))

    def _decompose_quantiles_refit(self, quantiles) -> list:
        with self.prepare_quantiles_refit(quantiles) as pr:
            rows, ok = pr.boot(0, pr.bootstrap_reps)
            info = pr.rifq_info()
            out = []
            for t in range(pr.n_taus):
                r = pr.finish_tau(t, rows[t], ok[t])
                r.quantile_values = (float(info["q"][0, t]), float(info["q"][1, t]))
                r.density_values = (float(info["f"][0, t]), float(info["f"][1, t]))
                r.n_density_floored = info["n_density_floored"]
                out.append(r)
            return out

    def decompose_quantiles(self, quantiles, refit: bool = False) -> list:
        """RIF decompositions at several quantiles in one run: one panel
        whose outcomes are the RIF columns, so every replicate's resample and Gram pass serve all
        quantiles. Element t equals ``decompose_quantile(quantiles[t])`` bitwise (same seed).
        ``refit=True``: every replicate refits the quantile, the bandwidth and the density of its
        own resample, so the standard errors carry their sampling error; the results gain ``quantile_values``,
        ``density_values`` and ``n_density_floored``. Unweighted, no ``normalize``, Heckman or ``cluster``."""
        if refit:
            return self._decompose_quantiles_refit(quantiles)
        taus = np.ascontiguousarray(quantiles, dtype=np.float64)
        if taus.ndim != 1 or taus.size == 0:
            raise ValueError("quantiles must be a non-empty 1-D sequence")
        clustered = self._cluster is not None
        hs = self._call("ob_builder_decompose_quantiles" + ("_clustered" if clustered else ""), N.dp(taus),
                        int(taus.size), policy=CONTEXT_FIRST, handles=int(taus.size), clustered=clustered)
        return [_results_from_c(h) for h in hs]

    def decompose_statistic(self, stat, refit: bool = False, **params) -> OaxacaResults:
        """RIF-regression decomposition of the gap in a distributional statistic (Firpo, Fortin, Lemieux):
        ``"variance"``, ``"gini"`` or ``"iqr"`` (``upper=0.9, lower=0.1``). The statistic's recentred influence
        function of each group's outcome, computed on the GPU (``ob_rif_stat``), is the outcome of ``run()``:
        ``total_gap`` is the gap in mean RIF, the statistic's gap up to the identities of DESIGN.md §5.12.
        ``refit=True``: see ``decompose_statistics``."""
        from .engine import parse_rif_statistic

        return self.decompose_statistics([parse_rif_statistic(stat, **params)], refit=refit)[0]

    def prepare_statistics_refit(self, stats) -> "PreparedRun":
        """ob_builder_prepare_statistics_refit: a handle whose replicates refit the statistic and so its RIF on every
        resample. ``boot`` returns rows (S, n_reps, row_len) and ok (S, n_reps); ``point_row()``
        is (S * row_len,). Row-order convention of §5.18: each group's rows stand in stable ascending order of y and
        OBRS-3 position i is the i-th row in that order, so the same seed draws other rows than the fixed-RIF
        run."""
        from .engine import _rif_specs

        specs, parsed = _rif_specs(stats)
        if not parsed:
            raise ValueError("statistics must be a non-empty sequence")
        if self._cluster is not None:
            raise N.OaxacaError(N.OB_E_UNSUPPORTED, "statistics refit: the cluster bootstrap is outside its scope")
        return self._prepared(self._call("ob_builder_prepare_statistics_refit", specs, len(parsed),
                                         policy=ARGUMENTS_FIRST))

    def _decompose_statistics_refit(self, stats) -> list:
        with self.prepare_statistics_refit(stats) as pr:
            rows, ok = pr.boot(0, pr.bootstrap_reps)
            info = pr.rifs_info()
            out = []
            for t in range(pr.n_taus):
                r = pr.finish_tau(t, rows[t], ok[t])
                r.statistic_values = (float(info["nu"][0, t]), float(info["nu"][1, t]))
                if info["specs"][t][0] == N.OB_RIF_IQR:
                    r.n_density_floored = info["n_density_floored"]
                out.append(r)
            return out

    def decompose_statistics(self, stats, refit: bool = False) -> list:
        """Several statistics in one run: one panel whose outcomes are the RIF columns, so every replicate's
        resample and Gram pass serve all of them. ``stats``: names, ``(name, params)`` pairs or dicts with a
        ``stat`` key. Element t equals ``decompose_statistic`` of element t bitwise (same seed). Honours
        ``.cluster(...)`` the way ``decompose_quantiles`` does.
        ``refit=True``: every replicate refits the statistic on its own resample, so the standard
        errors carry its sampling error; the results gain ``statistic_values`` and, for a range,
        ``n_density_floored``. Unweighted, no ``normalize``, Heckman or ``cluster``."""
        from .engine import parse_rif_statistic

        stats = list(stats)
        parsed = [s if isinstance(s, tuple) and len(s) == 3 else parse_rif_statistic(s) for s in stats]
        if not parsed:
            raise ValueError("statistics must be a non-empty sequence")
        if refit:
            return self._decompose_statistics_refit(parsed)
        specs = (N.ob_rif_spec * len(parsed))(*[N.ob_rif_spec(*p) for p in parsed])
        clustered = self._cluster is not None
        hs = self._call("ob_builder_decompose_statistics" + ("_clustered" if clustered else ""), specs, len(parsed),
                        policy=ARGUMENTS_FIRST, handles=len(parsed), clustered=clustered)
        return [_results_from_c(h) for h in hs]

    def prepare_binary(self, model: str = "probit") -> "PreparedRun":
        if model not in N.OB_BINARY_MODELS:
            raise ValueError(f"unknown binary model {model!r}: 'probit' (or 'logit', which is refused)")
        if self._cluster is not None:
            raise N.OaxacaError(N.OB_E_UNSUPPORTED, "binary decomposition: the cluster bootstrap is outside its scope")
        return self._prepared(self._call("ob_builder_prepare_binary", N.OB_BINARY_MODELS[model], policy=ARGUMENTS_FIRST,
                                         ctx=self._ctx))

    def decompose_binary(self, model: str = "probit") -> "BinaryDecompositionResults":
        """Extension (no counterpart in the reference crate): the nonlinear decomposition of a gap in a 0/1
        outcome (Fairlie 1999, Yun 2004, Bauer-Sinning 2008): a probit per group and replicate on the GPU, the
        counterfactual mean probabilities Pbar(X_g, beta), two-fold and three-fold terms from them and Yun's
        detailed terms, bootstrapped like ``run()``. Reference coefficients GroupA, GroupB, Weighted or Cotton.
        Refused (``OB_E_UNSUPPORTED``): ``model="logit"``, weights, ``normalize``, ``cluster``, Heckman settings,
        Pooled / Neumark, more than 32 design columns."""
        with self.prepare_binary(model) as pr:
            rows, ok = pr.boot(0, self._bootstrap_reps)
            res = pr.finish(rows, ok)
            point = pr.point_row()
        k = (len(point) - 14) // 7
        tail = point[6 + 2 * k:]
        names = [c.name for c in res.two_fold.detailed_explained]
        keys = [(g, b) for g in ("A", "B") for b in ("beta_a", "beta_b", "beta_star")]
        return BinaryDecompositionResults(
            model=model, total_gap=float(point[5]), raw_gap=float(tail[5 * k + 6] - tail[5 * k + 7]),
            two_fold=res.two_fold.aggregate, three_fold=res.three_fold.aggregate,
            detailed_explained=res.two_fold.detailed_explained,
            detailed_unexplained=res.two_fold.detailed_unexplained,
            probabilities={key: float(v) for key, v in zip(keys, tail[5 * k:5 * k + 6])},
            beta_a=tail[:k].copy(), beta_b=tail[k:2 * k].copy(), beta_star=tail[4 * k:5 * k].copy(),
            xa_mean=tail[2 * k:3 * k].copy(), xb_mean=tail[3 * k:4 * k].copy(), names=names,
            n_a=res.n_a, n_b=res.n_b, n_failed=res.n_failed)

    def prepare_tobit(self, lower=None, upper=None) -> "PreparedRun":
        """The handle of ``decompose_tobit`` (``ob_builder_prepare_tobit``): the limits are fixed and the point fits
        have run; ``boot`` / ``boot_device`` / ``finish`` / ``point_row`` / ``tobit_info`` work on it."""
        if self._cluster is not None:
            raise N.OaxacaError(N.OB_E_UNSUPPORTED, "tobit decomposition: the cluster bootstrap is outside its scope")
        from .engine import _tobit_config

        tc = _tobit_config(lower, upper)
        return self._prepared(self._call("ob_builder_prepare_tobit", C.byref(tc), policy=ARGUMENTS_FIRST, ctx=self._ctx))

    def decompose_tobit(self, lower=None, upper=None) -> "TobitDecompositionResults":
        """Extension (no counterpart in the reference crate): the decomposition of a gap in a censored outcome
        (Bauer and Sinning 2008, 2010; Stata's ``nldecompose ..., tobit``) -- top-coded earnings, or a bonus that is
        zero for many. The outcome is read as max(``lower``, min(``upper``, x'beta + sigma eps)); a row at a limit
        is censored, either limit may be ``None``. A censored-normal fit per group and replicate on the GPU, the
        conditional means of the censored outcome under own and other coefficients, two-fold and three-fold terms
        from them, Yun's detailed terms and the decomposition of the latent gap, bootstrapped like ``run()``.
        Sample weights are served. Reference coefficients GroupA or GroupB. Refused (``OB_E_UNSUPPORTED``):
        Weighted, Cotton, Pooled and Neumark coefficients, ``normalize``, ``cluster``, Heckman settings, more than
        31 design columns; ``boot_sharded``, the jackknife and BCa on its handle."""
        with self.prepare_tobit(lower, upper) as pr:
            rows, ok = pr.boot(0, self._bootstrap_reps)
            res = pr.finish(rows, ok)
            point = pr.point_row()
        return _tobit_results(res, point, lower, upper)

    def prepare_reweighted(self, statistic=None, **params) -> "PreparedRun":
        """The handle of ``decompose_reweighted``. ``statistic`` (with its parameters, as
        ``parse_weighted_rif_statistic`` takes them) makes it the decomposition of that statistic; ``None`` is
        the mean."""
        from .engine import parse_weighted_rif_statistic

        if statistic is None and params:
            raise ValueError(f"unexpected parameter(s) {', '.join(sorted(params))} without a statistic")
        spec = None if statistic is None else N.ob_rif_spec(*parse_weighted_rif_statistic(statistic, **params))
        if self._cluster is not None:
            raise N.OaxacaError(N.OB_E_UNSUPPORTED,
                                "reweighted decomposition: the cluster bootstrap is outside its scope")
        if spec is None:
            h = self._call("ob_builder_prepare_reweighted", policy=ARGUMENTS_FIRST, ctx=self._ctx)
        else:
            h = self._call("ob_builder_prepare_reweighted_statistic", C.byref(spec), policy=ARGUMENTS_FIRST,
                           ctx=self._ctx)
        return self._prepared(h)

    def decompose_reweighted_statistics(self, stats) -> list:
        """Several statistics in one reweighted run (``ob_builder_run_reweighted_statistics``): every replicate's
        resample and logit fit serve all of them. ``stats``: names, ``(name, params)`` pairs or dicts with a
        ``stat`` key, at most 16. Element t equals ``decompose_reweighted`` of element t bitwise (same seed)."""
        from .engine import parse_weighted_rif_statistic, weighted_rif_name

        parsed = [parse_weighted_rif_statistic(s) for s in stats]
        if not parsed:
            raise ValueError("statistics must be a non-empty sequence")
        if self._cluster is not None:
            raise N.OaxacaError(N.OB_E_UNSUPPORTED,
                                "reweighted decomposition: the cluster bootstrap is outside its scope")
        specs = (N.ob_rif_spec * len(parsed))(*[N.ob_rif_spec(*p) for p in parsed])
        hs = self._call("ob_builder_run_reweighted_statistics", specs, len(parsed), policy=ARGUMENTS_FIRST,
                        handles=len(parsed))
        results = [_results_from_c(h) for h in hs]
        outs = []
        for p, res in zip(parsed, results):  # the tables came from the one run; a handle gives the point row and nu
            with self.prepare_reweighted(weighted_rif_name(p)) as pr:
                outs.append(_reweighted_results(res, pr.point_row(), weighted_rif_name(p), pr.reweight_statistics()))
        return outs

    def decompose_reweighted(self, statistic=None, **params) -> "ReweightedDecompositionResults":
        """Extension (no counterpart in the reference crate): the reweighted decomposition of Fortin, Lemieux and
        Firpo (2011, section 5), Stata's ``oaxaca_rif ..., rwlogit()``. A propensity logit of the non-reference
        group on the design reweights the reference group B to A's covariates (the counterfactual sample C); a
        third regression on C splits the composition effect into a pure explained part and a specification
        error, and the structure effect into a pure unexplained part and a reweighting error. Every bootstrap
        replicate refits the logit on the GPU. Sample weights are served; ``reference_coefficients`` is ignored.
        Refused (``OB_E_UNSUPPORTED``): ``normalize``, ``cluster``, Heckman settings, more than 32 design
        columns.

        ``statistic`` ("variance", "gini", "quantile" with ``tau``, "iqr" with ``upper`` / ``lower``) decomposes the
        gap in that statistic instead (Firpo, Fortin and Lemieux; ``oaxaca_rif ..., rwlogit()``): the statistic's
        weighted RIF in A, in B and in the counterfactual sample C is the outcome of the three fits. The RIFs are
        computed once, at the point estimate; replicates refit the logit and the regressions. ``None`` is the mean,
        exactly as before."""
        from .engine import parse_weighted_rif_statistic, weighted_rif_name

        with self.prepare_reweighted(statistic, **params) as pr:
            rows, ok = pr.boot(0, self._bootstrap_reps)
            res = pr.finish(rows, ok)
            point = pr.point_row()
            nu = None if statistic is None else pr.reweight_statistics()
        name = None if statistic is None else weighted_rif_name(parse_weighted_rif_statistic(statistic, **params))
        return _reweighted_results(res, point, name, nu)

    def prepare_distribution(self, quantiles=(0.1, 0.25, 0.5, 0.75, 0.9), thresholds=None, n_thresholds=50, lo=0.05,
                             hi=0.95) -> "PreparedRun":
        """The handle of ``decompose_distribution`` (``ob_builder_prepare_dr``): the thresholds are fixed and the
        point pass has run; ``boot`` / ``boot_device`` / ``finish`` / ``point_row`` / ``dr_info`` work on it."""
        if self._cluster is not None:
            raise N.OaxacaError(N.OB_E_UNSUPPORTED,
                                "distribution regression: the cluster bootstrap is outside its scope")
        taus = np.ascontiguousarray(np.atleast_1d(quantiles), dtype=np.float64)
        if taus.ndim != 1:
            raise ValueError("quantiles must be a 1-D sequence")
        dr = N.ob_dr_config()
        thr = None
        if thresholds is not None:
            thr = np.ascontiguousarray(thresholds, dtype=np.float64)
            if thr.ndim != 1:
                raise ValueError("thresholds must be a 1-D sequence")
            dr.thresholds, dr.n_thresholds = N.dp(thr), len(thr)
        else:
            dr.thresholds, dr.n_thresholds = None, int(n_thresholds)
        dr.lo, dr.hi = float(lo), float(hi)
        dr.quantiles, dr.n_quantiles = N.dp(taus), len(taus)
        return self._prepared(self._call("ob_builder_prepare_dr", C.byref(dr), policy=ARGUMENTS_FIRST, ctx=self._ctx))

    def decompose_distribution(self, quantiles=(0.1, 0.25, 0.5, 0.75, 0.9), thresholds=None, n_thresholds=50, lo=0.05,
                               hi=0.95) -> "DistributionDecompositionResults":
        """Extension (no counterpart in the reference crate): the distribution-regression decomposition of
        Chernozhukov, Fernandez-Val and Melly (2013), Stata's ``cdeco`` / ``counterfactual``. A logit of
        ``1[y <= c]`` on the design is fitted in each group at every threshold ``c`` (given, or ``n_thresholds``
        pooled sample quantiles at evenly spaced levels of ``[lo, hi]``, duplicates removed); averaging the
        reference group B's fitted probabilities over A's rows gives the counterfactual distribution C. The three
        distributions are rearranged and inverted at ``quantiles``: at each tau the gap splits into
        ``composition`` (Q_C - Q_B) and ``structure`` (Q_A - Q_C). Every bootstrap replicate refits all 2 T logits
        on the GPU; the thresholds stay fixed. Sample weights are served; ``reference_coefficients`` is ignored.
        Refused (``OB_E_UNSUPPORTED``): ``normalize``, ``cluster``, Heckman settings, more than 32 design columns,
        64 thresholds or 32 quantiles. Warns when a tau lies outside the range the threshold grid covers."""
        import warnings

        with self.prepare_distribution(quantiles, thresholds, n_thresholds, lo, hi) as pr:
            rows, ok = pr.boot(0, self._bootstrap_reps)
            h = C.c_void_p()  # not finish(): the four tables of this handle are read by _dr_tables
            N.check(N.lib().ob_prepared_finish(pr._h, N.dp(rows), N.u8p(ok), len(ok), C.byref(h)))
            qe, qv, de, cdf, n_failed, n_a, n_b = _dr_tables(h)
            info = pr.dr_info()
            point = pr.point_row()
        from .engine import dr_quantiles

        T, nq = len(info["thresholds"]), len(info["quantiles"])
        fr = point[6 * nq + 3 * T:6 * nq + 7 * T].reshape(4, T)
        re = {key: dr_quantiles(fr[i], info["thresholds"], info["quantiles"])[1] for i, key in enumerate(("AA", "BB", "AB"))}
        if info["n_out_of_range"]:
            warnings.warn(f"distribution regression: {info['n_out_of_range']} (quantile, distribution) pair(s) lie "
                          "outside the range of the threshold grid; their quantiles are the grid's end points",
                          RuntimeWarning, stacklevel=2)
        names = self.get_data_matrices()[4]
        return DistributionDecompositionResults(
            quantiles=info["quantiles"], thresholds=info["thresholds"], quantile_effects=qe, quantile_values=qv,
            distribution_effects=de, cdf=cdf, cdf_rearranged=re, beta_a=info["beta"][0], beta_b=info["beta"][1],
            passes=info["passes"], out_of_range=info["out_of_range"], names=list(names), n_a=n_a, n_b=n_b,
            n_failed=n_failed, n_out_of_range=info["n_out_of_range"],
            n_thresholds_requested=info["n_thresholds_requested"])

    def prepare_density(self, grid_size=100, grid=None, bandwidth=None) -> "PreparedRun":
        """The handle of ``decompose_density`` (``ob_builder_prepare_density``): the grid and the bandwidths are fixed
        and the point pass has run; ``boot`` / ``boot_device`` / ``finish`` / ``point_row`` / ``density_info`` work on
        it."""
        if self._cluster is not None:
            raise N.OaxacaError(N.OB_E_UNSUPPORTED, "density decomposition: the cluster bootstrap is outside its scope")
        dc = N.ob_density_config()
        gr = None
        if grid is not None:
            gr = np.ascontiguousarray(grid, dtype=np.float64)
            if gr.ndim != 1:
                raise ValueError("grid must be a 1-D sequence")
            dc.grid, dc.grid_size = N.dp(gr), len(gr)
        else:
            dc.grid, dc.grid_size = None, int(grid_size)
        if bandwidth is None:
            dc.bandwidth_a = dc.bandwidth_b = 0.0
        else:
            bw = np.atleast_1d(np.asarray(bandwidth, dtype=np.float64))
            if bw.shape not in ((1,), (2,)):
                raise ValueError("bandwidth must be one value or (bandwidth_a, bandwidth_b)")
            if (bw == 0.0).any():
                raise ValueError("a bandwidth of 0 is not a bandwidth; pass None for Silverman's")
            dc.bandwidth_a, dc.bandwidth_b = float(bw[0]), float(bw[-1])
        return self._prepared(self._call("ob_builder_prepare_density", C.byref(dc), policy=ARGUMENTS_FIRST,
                                         ctx=self._ctx, keep=(gr,)))

    def decompose_density(self, grid_size=100, grid=None, bandwidth=None) -> "DensityDecompositionResults":
        """Extension: the density decomposition of DiNardo, Fortin and Lemieux (1996) with bootstrap inference --
        ``run_dfl``'s picture under this builder's conventions, with sample weights and with bands. The kernel
        densities of the outcome in A, in the reference group B and in B reweighted to A's covariates (the
        counterfactual C, psi = p / (1 - p) of the reweighted decomposition's propensity logit) on a grid of
        ``grid_size`` points over the pooled outcome (dfl.rs's rule) or on ``grid``; the bandwidths are Silverman's
        per group at the point estimate (``bandwidth``: one value or a pair overrides them) and stay fixed. Every
        bootstrap replicate refits the logit and recomputes the three curves on the GPU. Each curve and each
        difference (total = f_A - f_B, composition = f_C - f_B, structure = f_A - f_C) comes with standard errors,
        pointwise percentile intervals and a uniform 95 % band. Sample weights are served;
        ``reference_coefficients`` is ignored. Refused (``OB_E_UNSUPPORTED``): ``normalize``, ``cluster``, Heckman
        settings, more than 32 design columns or 256 grid points."""
        with self.prepare_density(grid_size, grid, bandwidth) as pr:
            rows, ok = pr.boot(0, self._bootstrap_reps)
            h = C.c_void_p()  # not finish(): the two tables of this handle are read by _density_results
            N.check(N.lib().ob_prepared_finish(pr._h, N.dp(rows), N.u8p(ok), len(ok), C.byref(h)))
            info = pr.density_info()
            point = pr.point_row()
        names = self.get_data_matrices()[4]
        return _density_results(h, info["grid"], info["bandwidth_a"], info["bandwidth_b"], point, info["k"], names)

    def _nopo_binned(self, bins) -> "OaxacaBuilder":
        """This builder, or with ``bins`` a copy whose frame has each named numeric matching column replaced by its
        ``numpy.digitize`` index (host side, a convenience only)."""
        if not bins:
            return self
        frame = self._frame
        for name, edges in bins.items():
            if name not in self._predictors:
                raise ValueError(f"bins: `{name}` is not a numeric matching column (predictors)")
            if name not in frame.columns:
                raise N.OaxacaError(N.OB_E_COLUMN, f"Column not found: {name}")
            kind, values, valid = frame.columns[name]
            if kind == N.OB_COL_STR:
                raise ValueError(f"bins: `{name}` is a string column")
            idx = np.digitize(np.asarray(values, dtype=np.float64), np.asarray(edges, dtype=np.float64))
            out = Frame({})
            out.nrows, out.columns = frame.nrows, dict(frame.columns)
            out.columns[name] = (N.OB_COL_I64, np.ascontiguousarray(idx, dtype=np.int64), valid)
            frame = out
        b = OaxacaBuilder(frame, self.outcome, self.group, self.reference_group)
        for attr in ("_predictors", "_categorical", "_normalize", "_selection_predictors"):
            setattr(b, attr, list(getattr(self, attr)))
        for attr in ("_bootstrap_reps", "_ref", "_weights", "_selection", "_seed", "_device", "_ctx", "_cluster",
                     "_cluster_stratified"):
            setattr(b, attr, getattr(self, attr))
        return b

    def _nopo_cells(self):
        row_cell, n_cells = np.empty(self._frame.nrows, dtype=np.int32), C.c_int32()
        self._call("ob_nopo_cells", N.i32p(row_cell), C.byref(n_cells), policy=HOST_ONLY, handles=0)
        return row_cell, int(n_cells.value)

    def prepare_nopo(self, bins=None) -> "PreparedRun":
        """The handle of ``decompose_nopo`` (``ob_builder_prepare_nopo``): the cells are fixed and the point pass has
        run; ``boot`` / ``boot_device`` / ``finish`` / ``point_row`` / ``nopo_info`` work on it."""
        if self._cluster is not None:
            raise N.OaxacaError(N.OB_E_UNSUPPORTED, "matching decomposition: the cluster bootstrap is outside its scope")
        b = self._nopo_binned(bins)
        return b._prepared(b._call("ob_builder_prepare_nopo", policy=ARGUMENTS_FIRST, ctx=self._ctx))

    def decompose_nopo(self, bins=None, relative: bool = False) -> "NopoDecompositionResults":
        """Extension (no counterpart in the reference crate): Nopo's (2008) exact-matching decomposition, Stata's
        ``nopomatch``. Rows are matched on the exact values of all ``predictors`` and ``categorical_predictors`` (a
        cell is one combination); the gap splits into ``composition`` and ``unexplained`` inside the common support
        and ``unmatched_a`` / ``unmatched_b``, what each group's rows without a counterpart owe. Every bootstrap
        replicate decides the support again on the GPU, so the intervals carry the matching step. ``bins``:
        ``{"age": [20, 30, 40]}`` matches a numeric column on its ``numpy.digitize`` index instead of its value.
        ``relative=True`` adds the terms over ybar_B. Sample weights are served; ``reference_coefficients`` is
        ignored. Refused (``OB_E_UNSUPPORTED``): ``normalize``, ``cluster``, Heckman settings, more than 522240
        cells."""
        b = self._nopo_binned(bins)
        with b.prepare_nopo() as pr:
            rows, ok = pr.boot(0, self._bootstrap_reps)
            h = C.c_void_p()  # not finish(): table 0 of this handle is read by _nopo_components
            N.check(N.lib().ob_prepared_finish(pr._h, N.dp(rows), N.u8p(ok), len(ok), C.byref(h)))
            comps, n_failed, n_a, n_b = _nopo_components(h)
            info = pr.nopo_info()
            point = pr.point_row()
        row_cell = info["row_cell"]
        first = np.full(info["n_cells"], -1, dtype=np.int64)  # a cell's key: the matching values of its first row
        used = np.flatnonzero(row_cell >= 0)[::-1]
        first[row_cell[used]] = used
        keycols = [b._frame.columns[name][1] for name in (*b._predictors, *b._categorical)]
        def value(v):
            return v.decode() if isinstance(v, bytes) else (v.item() if hasattr(v, "item") else v)

        cells = [{"key": tuple(value(col[r]) for col in keycols),
                  "n_a": int(info["n_cell_a"][x]), "n_b": int(info["n_cell_b"][x]), "mean_a": float(info["mean_a"][x]),
                  "mean_b": float(info["mean_b"][x]), "in_support": bool(info["in_support"][x])}
                 for x, r in enumerate(first)]
        return NopoDecompositionResults(
            components=comps, cells=cells, row_cell=row_cell, relative=_nopo_relative(point, rows, ok) if relative else {},
            n_cells=info["n_cells"], n_support_cells=info["n_support_cells"], n_a=n_a, n_b=n_b, n_failed=n_failed)

    def statistic_builder(self, stat, **params) -> "OaxacaBuilder":
        """A fresh builder over this frame with the outcome replaced by the statistic's RIF of each group's
        outcome (the rows ``run()`` would keep, group by group, as ``decompose_statistic`` forms it), so that
        ``run_bca()``, ``jackknife()`` and ``prepare()`` serve the statistic. Every setting is carried over
        except the Heckman selection, as in ``decompose_quantile``."""
        from .engine import parse_rif_statistic, rif_statistic

        code, p0, p1 = parse_rif_statistic(stat, **params)
        name = {v: k for k, v in N.OB_RIF_STATS.items()}[code]
        kw = {"upper": p0, "lower": p1} if code == N.OB_RIF_IQR else {}
        used = [self.outcome, self.group, *self._predictors, *self._categorical, *self._selection_predictors]
        used += [c for c in (self._weights, self._selection, self._cluster) if c]
        fcols = self._frame.columns
        keep = np.ones(self._frame.nrows, dtype=bool)
        for c in used:  # clean_dataframe (builder.rs:760-784)
            if c not in fcols:
                raise N.OaxacaError(N.OB_E_COLUMN, f"Column not found: {c}")
            kind, values, valid = fcols[c]
            if kind == N.OB_COL_STR:
                keep &= np.array([v is not None for v in values], dtype=bool)
            elif valid is not None:
                keep &= valid.astype(bool)
        gkind, groups, _ = fcols[self.group]
        ykind, y, _ = fcols[self.outcome]
        if gkind != N.OB_COL_STR or ykind != N.OB_COL_F64:
            raise N.OaxacaError(N.OB_E_POLARS, "Polars error: invalid series dtype: the group column must be "
                                               "String and the outcome Float64")
        levels = sorted({g for g, k in zip(groups, keep) if k})  # split_groups (builder.rs:61-102)
        if len(levels) < 2:
            raise N.OaxacaError(N.OB_E_GROUP, "Invalid group variable: Not enough groups for comparison")
        ref = self.reference_group.encode()
        name_a = levels[1] if levels[0] == ref else levels[0]
        garr = np.array(groups, dtype=object)
        new_y = y.copy()
        for level in (name_a, ref):
            rows = np.flatnonzero(keep & (garr == level))
            new_y[rows] = rif_statistic(y[rows], name, device=self._device, **kw)[0]
        b = OaxacaBuilder(self._frame.with_f64_column(self.outcome, new_y), self.outcome, self.group,
                          self.reference_group)
        for attr in ("_predictors", "_categorical", "_normalize"):
            setattr(b, attr, list(getattr(self, attr)))
        for attr in ("_bootstrap_reps", "_ref", "_weights", "_seed", "_device", "_ctx", "_cluster",
                     "_cluster_stratified"):
            setattr(b, attr, getattr(self, attr))
        return b

    def prepare(self) -> "PreparedRun":
        """clean/dummies/split/upload/point estimate once; replicate ranges run separately
        (the multi-GPU path in ``distributed.py``)."""
        clustered = self._cluster is not None
        return self._prepared(self._call("ob_builder_prepare" + ("_clustered" if clustered else ""), policy=CONTEXT_FIRST,
                                         ctx=self._ctx, clustered=clustered))


class PreparedRun:
    """An ``ob_prepared`` handle: panel resident in HBM + point estimate."""

    def __init__(self, handle, reps: int, device: int = 0):
        self._h = handle
        self.bootstrap_reps = reps
        self.device = device  # the GPU holding the panel
        self.row_len = N.lib().ob_prepared_row_len(handle)
        self.seed = int(N.lib().ob_prepared_seed(handle))
        info = N.ob_cluster_info()
        self.cluster_info = None  # a clustered run: n_clusters, n_clusters_a, n_clusters_b, max_cluster_rows, stratified
        if N.lib().ob_prepared_cluster_info(handle, C.byref(info)) == N.OB_OK:
            self.cluster_info = {f: int(v) for f, v in N.struct_dict(info).items()}
        # a refit handle (prepare_quantiles_refit): its quantiles; boot then returns (n_taus, n_reps, ...) blocks
        rq = N.ob_rifq_info()
        self.n_taus = int(rq.n_taus) if N.lib().ob_prepared_rifq_info(handle, C.byref(rq)) == N.OB_OK else 0
        if not self.n_taus:  # a statistics refit handle (prepare_statistics_refit): its statistics, likewise
            rs = N.ob_rifs_info()
            self.n_taus = int(rs.n_specs) if N.lib().ob_prepared_rifs_info(handle, C.byref(rs)) == N.OB_OK else 0

    def boot(self, first_rep: int, n_reps: int):
        shape = (self.n_taus, n_reps) if self.n_taus else (n_reps,)
        rows = np.empty(shape + (self.row_len,), dtype=np.float64)
        ok = np.zeros(shape, dtype=np.uint8)
        if n_reps:
            N.check(N.lib().ob_prepared_boot(self._h, first_rep, n_reps, N.dp(rows), N.u8p(ok)))
        return rows, ok

    def boot_sharded(self, first_rep: int, n_reps: int):
        """ob_prepared_boot_sharded: this rank's shard + the engine's RCCL all-gather (a rank
        context) -> all rows on every rank."""
        rows = np.empty((n_reps, self.row_len), dtype=np.float64)
        ok = np.zeros(n_reps, dtype=np.uint8)
        if n_reps:
            N.check(N.lib().ob_prepared_boot_sharded(self._h, first_rep, n_reps, N.dp(rows), N.u8p(ok)))
        return rows, ok

    def boot_device(self, first_rep: int, n_reps: int, rows_ptr: int, ok_ptr: int, stream: int | None):
        """Enqueue replicates into device buffers (e.g. torch tensors' data_ptr()) on ``stream``."""
        N.check(N.lib().ob_prepared_boot_device(self._h, first_rep, n_reps, C.c_void_p(rows_ptr),
                                                C.c_void_p(ok_ptr), C.c_void_p(stream or 0)))

    def point_row(self) -> np.ndarray:
        """ob_prepared_point_row: the point-estimate row (a copy)."""
        ptr = C.POINTER(C.c_double)()
        n = C.c_int64()
        N.check(N.lib().ob_prepared_point_row(self._h, C.byref(ptr), C.byref(n)))
        return N.array_copy(ptr, (n.value,))

    def reweight_statistics(self) -> tuple:
        """ob_prepared_reweight_statistics: (nu_A, nu_B, nu_C) of a reweighted statistic's handle."""
        out = np.zeros(3)
        N.check(N.lib().ob_prepared_reweight_statistics(self._h, N.dp(out)))
        return tuple(float(v) for v in out)

    def dr_info(self) -> dict:
        """ob_prepared_dr_info: the thresholds kept, the quantiles, the point fits beta (2, T, K: A then B), their
        pass counts (2, T) and the edge cases of the point estimate (out_of_range (3, n_q): A, B, C)."""
        o = N.ob_dr_info()
        N.check(N.lib().ob_prepared_dr_info(self._h, C.byref(o)))
        T, nq, k = o.n_thresholds, o.n_quantiles, o.k
        arr = N.array_copy
        return {"thresholds": arr(o.thresholds, (T,)), "quantiles": arr(o.quantiles, (nq,)),
                "beta": arr(o.beta, (2, T, k)), "passes": arr(o.passes, (2, T)),
                "out_of_range": arr(o.out_of_range, (3, nq)), "n_out_of_range": int(o.n_out_of_range),
                "n_thresholds_requested": int(o.n_requested)}

    def nopo_info(self) -> dict:
        """ob_prepared_nopo_info: the point pass's cell table (per cell the rows of A and B, N_A(x), N_B(x), the cell
        means and the support flag) and the cell of every row of the frame."""
        o = N.ob_nopo_info()
        N.check(N.lib().ob_prepared_nopo_info(self._h, C.byref(o)))
        nc, arr = o.n_cells, N.array_copy
        return {"n_cells": int(nc), "n_support_cells": int(o.n_support_cells), "n_cell_a": arr(o.n_cell_a, (nc,)),
                "n_cell_b": arr(o.n_cell_b, (nc,)), "w_a": arr(o.w_a, (nc,)), "w_b": arr(o.w_b, (nc,)),
                "mean_a": arr(o.mean_a, (nc,)), "mean_b": arr(o.mean_b, (nc,)),
                "in_support": arr(o.in_support, (nc,)).astype(bool), "row_cell": arr(o.row_cell, (o.n_rows,))}

    def density_info(self) -> dict:
        """ob_prepared_density_info: the grid, the two bandwidths, the design columns and the groups' rows of a
        density handle."""
        o = N.ob_density_info()
        N.check(N.lib().ob_prepared_density_info(self._h, C.byref(o)))
        return {"grid": N.array_copy(o.grid, (o.grid_size,)), "bandwidth_a": float(o.bandwidth_a),
                "bandwidth_b": float(o.bandwidth_b), "k": int(o.k), "n_a": int(o.n_a), "n_b": int(o.n_b)}

    def tobit_info(self) -> dict:
        """ob_prepared_tobit_info: the limits (``None`` where absent), the groups' rows and rows at each limit and the
        point fits of a Tobit handle: ``eta`` (2, k + 1: A then B, [delta; theta]), ``beta`` (2, k), ``sigma`` (2)."""
        o = N.ob_tobit_info()
        N.check(N.lib().ob_prepared_tobit_info(self._h, C.byref(o)))
        eta = N.array_copy(o.eta, (2, o.k + 1))
        return {"k": int(o.k), "lower": float(o.lower) if o.has_lower else None,
                "upper": float(o.upper) if o.has_upper else None, "n_a": int(o.n_a), "n_b": int(o.n_b),
                "n_censored": {("A", "left"): int(o.n_left_a), ("A", "right"): int(o.n_right_a),
                               ("B", "left"): int(o.n_left_b), ("B", "right"): int(o.n_right_b)},
                "eta": eta, "beta": eta[:, :-1] / eta[:, -1:], "sigma": 1.0 / eta[:, -1],
                "passes": (int(o.passes_a), int(o.passes_b))}

    def rifq_info(self) -> dict:
        """ob_prepared_rifq_info: the quantiles, each group's sort permutation, the point q and f (2, T: A then B)
        and the floored densities of the point pass and every boot since."""
        o = N.ob_rifq_info()
        N.check(N.lib().ob_prepared_rifq_info(self._h, C.byref(o)))
        T = o.n_taus
        arr = N.array_copy
        return {"taus": arr(o.taus, (T,)), "k": int(o.k), "perm_a": arr(o.perm_a, (o.n_a,)),
                "perm_b": arr(o.perm_b, (o.n_b,)), "q": arr(o.q, (2, T)), "f": arr(o.f, (2, T)),
                "n_density_floored": int(o.n_density_floored)}

    def rifs_info(self) -> dict:
        """ob_prepared_rifs_info: the statistics as (code, p0, p1), each group's sort permutation, the point nu
        (2, S: A then B) and the floored densities of the point pass and every boot since."""
        o = N.ob_rifs_info()
        N.check(N.lib().ob_prepared_rifs_info(self._h, C.byref(o)))
        S = o.n_specs
        arr = N.array_copy
        return {"specs": [(int(o.specs[t].stat), float(o.specs[t].p0), float(o.specs[t].p1)) for t in range(S)],
                "k": int(o.k), "perm_a": arr(o.perm_a, (o.n_a,)), "perm_b": arr(o.perm_b, (o.n_b,)),
                "nu": arr(o.nu, (2, S)), "n_density_floored": int(o.n_density_floored)}

    def finish_tau(self, t: int, rows: np.ndarray, ok: np.ndarray) -> OaxacaResults:
        """ob_prepared_finish_tau: ``finish`` for quantile t of a refit handle, or statistic t of a statistics refit
        handle (rows / ok: its block)."""
        return self._finish("ob_prepared_finish_tau", rows, ok, tau=int(t))

    def sync(self):
        N.check(N.lib().ob_panel_sync(N.lib().ob_prepared_panel(self._h)))

    def timing(self) -> dict:
        t = N.ob_timing()
        N.check(N.lib().ob_panel_last_timing(N.lib().ob_prepared_panel(self._h), C.byref(t)))
        return N.struct_dict(t)

    def _flat_block(self, rows, ok):
        """rows (n_reps, row_len) and ok (n_reps,) of one outcome: a refit handle's (T, n_reps, ...) blocks go
        through ``finish_tau`` one quantile at a time."""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        ok = np.ascontiguousarray(ok, dtype=np.uint8)
        if rows.ndim != 2 or ok.ndim != 1 or len(rows) != len(ok):
            raise ValueError("rows must be (n_reps, row_len) and ok (n_reps,); pass one quantile's block of a refit "
                             "handle's boot to finish_tau")
        return rows, ok

    def _finish(self, symbol: str, rows, ok, *extra, jackknife: bool = False, tau=None, flat: bool = True):
        """``lib.<symbol>(handle[, tau], rows, ok, n_reps, *extra, &results)`` -> OaxacaResults. ``flat`` False skips
        ``_flat_block``'s shape check."""
        if flat:
            rows, ok = self._flat_block(rows, ok)
        else:
            rows, ok = np.ascontiguousarray(rows, dtype=np.float64), np.ascontiguousarray(ok, dtype=np.uint8)
        h = C.c_void_p()
        first = () if tau is None else (tau,)
        N.check(getattr(N.lib(), symbol)(self._h, *first, N.dp(rows), N.u8p(ok), len(ok), *extra, C.byref(h)))
        return _results_from_c(h, jackknife=jackknife)

    def finish(self, rows: np.ndarray, ok: np.ndarray) -> OaxacaResults:
        return self._finish("ob_prepared_finish", rows, ok)

    def jackknife(self) -> "JackknifeResult":
        """ob_prepared_jackknife: the leave-one-out pass over the resident panel (kept in the handle)."""
        panel = N.lib().ob_prepared_panel(self._h)
        o, bufs = _jackknife_out(N.lib().ob_panel_k(panel))
        N.check(N.lib().ob_prepared_jackknife(self._h, C.byref(o)))
        return _jackknife_result(o, bufs, None)

    def finish_bca(self, rows: np.ndarray, ok: np.ndarray, confidence_level: float = 0.95) -> OaxacaResults:
        """``finish`` with BCa intervals (ob_prepared_finish_bca); rows of ``boot`` or ``boot_sharded``."""
        return self._finish("ob_prepared_finish_bca", rows, ok, float(confidence_level), jackknife=True)

    def cluster_jackknife(self) -> "JackknifeResult":
        """ob_prepared_cluster_jackknife: the delete-one-cluster pass over the resident per-cluster Grams (kept in
        the handle); ``n_used`` / ``n_dropped`` are clusters per stratum."""
        panel = N.lib().ob_prepared_panel(self._h)
        o, bufs = _jackknife_out(N.lib().ob_panel_k(panel))
        N.check(N.lib().ob_prepared_cluster_jackknife(self._h, C.byref(o)))
        return _jackknife_result(o, bufs, None)

    def cluster_jackknife_rows(self, full: bool = False, deviations: bool = False):
        """ob_prepared_cluster_jackknife_rows -> (theta (C, 6 + 2K), kept (C,), n_dropped per stratum): theta_(c)
        from the solve kernel itself, NaN for a dropped cluster. ``full=True`` keeps the whole replicate-shaped
        rows (C, row_len): the components, then beta_A, beta_B, xbar_A, xbar_B, beta*. ``deviations=True`` appends
        d (C, 6 + 2K): every cluster's theta_(c) - theta_hat exactly as the production path forms and sums it."""
        if self.cluster_info is None:
            raise N.OaxacaError(N.OB_E_INVALID, "this prepared run is not clustered")
        nc = self.cluster_info["n_clusters"]
        k = N.lib().ob_panel_k(N.lib().ob_prepared_panel(self._h))
        theta = np.empty((nc, self.row_len), dtype=np.float64)
        kept = np.zeros(nc, dtype=np.uint8)
        dev = np.empty((nc, 6 + 2 * k), dtype=np.float64) if deviations else None
        nd = (C.c_int64 * 2)()
        N.check(N.lib().ob_prepared_cluster_jackknife_rows(self._h, N.dp(theta), N.u8p(kept), nd, N.dp(dev)))
        out = ((theta if full else theta[:, :6 + 2 * k].copy()), kept.astype(bool), (int(nd[0]), int(nd[1])))
        return out + (dev,) if deviations else out

    def finish_cluster_bca(self, rows: np.ndarray, ok: np.ndarray, confidence_level: float = 0.95) -> OaxacaResults:
        """``finish`` with BCa intervals from the delete-one-cluster accelerations (ob_prepared_finish_cluster_bca)."""
        return self._finish("ob_prepared_finish_cluster_bca", rows, ok, float(confidence_level), jackknife=True,
                            flat=False)

    def close(self):
        if self._h:
            N.lib().ob_prepared_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OaxacaBlinder:
    """python.rs:193-276 (declared pyo3 surface). Errors surface as RuntimeError (OaxacaError)."""

    def __init__(self, dataframe, outcome, group, reference_group, predictors, categorical_predictors=(),
                 bootstrap_reps=100, weights=None, selection_outcome=None, selection_predictors=None, *,
                 seed=None, device=None, cluster=None):
        self.dataframe = dataframe if isinstance(dataframe, Frame) else Frame(dataframe)
        self.outcome, self.group, self.reference_group = outcome, group, reference_group
        self.predictors = list(predictors)
        self.categorical_predictors = list(categorical_predictors)
        self.bootstrap_reps = int(bootstrap_reps)
        self.weights = weights
        self.selection_outcome = selection_outcome
        self.selection_predictors = list(selection_predictors or [])
        self.seed = seed
        self.device = device
        self.cluster = cluster

    def _create_builder(self) -> OaxacaBuilder:
        b = OaxacaBuilder(self.dataframe, self.outcome, self.group, self.reference_group)
        b.predictors(self.predictors).categorical_predictors(self.categorical_predictors)
        b.bootstrap_reps(self.bootstrap_reps).seed(self.seed).device(self.device)
        if self.weights:
            b.weights(self.weights)
        if self.selection_outcome:
            b.heckman_selection(self.selection_outcome, self.selection_predictors)
        if self.cluster:
            b.cluster(self.cluster)
        return b

    def fit(self) -> OaxacaResults:
        return self._create_builder().run()

    def fit_quantile(self, quantile: float, refit: bool = False) -> OaxacaResults:
        if refit:
            return self._create_builder().decompose_quantile(quantile, refit=True)
        return self._create_builder().decompose_quantile(quantile)

    def fit_quantiles(self, quantiles) -> list:
        """Several RIF quantiles sharing one bootstrap (``OaxacaBuilder.decompose_quantiles``)."""
        return self._create_builder().decompose_quantiles(quantiles)

    def fit_statistic(self, stat, refit: bool = False, **params) -> OaxacaResults:
        """The RIF decomposition of a distributional statistic (``OaxacaBuilder.decompose_statistic``)."""
        if refit:
            return self._create_builder().decompose_statistic(stat, refit=True, **params)
        return self._create_builder().decompose_statistic(stat, **params)

    def fit_statistics(self, stats, refit: bool = False) -> list:
        """Several statistics sharing one bootstrap (``OaxacaBuilder.decompose_statistics``)."""
        if refit:
            return self._create_builder().decompose_statistics(stats, refit=True)
        return self._create_builder().decompose_statistics(stats)

    def optimize_budget(self, budget: float, target_gap: float):
        b = self._create_builder()
        b.bootstrap_reps(0)
        res = b.run()
        return [{"index": float(a.index), "original_residual": a.original_residual, "adjustment": a.adjustment}
                for a in res.optimize_budget(budget, target_gap)]


# ---------------------------------------------------------------------------------------------
# Machado-Mata (quantile_decomposition.rs:21-522)
# ---------------------------------------------------------------------------------------------
@dataclass
class QuantileDecompositionDetail:
    total_gap: ComponentResult
    characteristics_effect: ComponentResult
    coefficients_effect: ComponentResult


@dataclass
class QuantileDecompositionResults:
    """results_by_quantile: {"q10": QuantileDecompositionDetail, ...} (:448-460)."""
    results_by_quantile: dict
    n_a: int
    n_b: int
    n_failed: int = 0

    def summary(self) -> str:  # quantile_decomposition.rs:462-505
        lines = ["Machado-Mata Quantile Decomposition Results", "=" * 44,
                 f"Group A (Advantaged): {self.n_a} observations", f"Group B (Reference):  {self.n_b} observations"]
        for key in sorted(self.results_by_quantile):
            d = self.results_by_quantile[key]
            lines += ["", f"--- Decomposition for Quantile: {key} ---",
                      f"{'Component':<16} {'Estimate':>10} {'Std. Err.':>10} {'p-value':>10}  95% CI"]
            for c in (d.total_gap, d.characteristics_effect, d.coefficients_effect):
                lines.append(f"{c.name:<16} {c.estimate:>10.4f} {c.std_err:>10.4f} {c.p_value:>10.4f}  "
                             f"[{c.ci_lower:.3f}, {c.ci_upper:.3f}]")
        text = "\n".join(lines)
        print(text)
        return text


class QuantileDecompositionBuilder:
    """quantile_decomposition.rs:21-95. Defaults: quantiles {0.1, 0.25, 0.5, 0.75, 0.9},
    simulations 200, bootstrap_reps 20. Every quantile regression of a pass runs on the GPU
    (ob_mm.hip); draws follow MM-1 (csrc/ob_spec.h) from ``seed`` instead of an unseeded RNG."""

    def __init__(self, dataframe, outcome: str, group: str, reference_group: str):
        self._frame = dataframe if isinstance(dataframe, Frame) else Frame(dataframe)
        self.outcome, self.group, self.reference_group = outcome, group, reference_group
        self._predictors: list[str] = []
        self._categorical: list[str] = []
        self._quantiles = [0.1, 0.25, 0.5, 0.75, 0.9]
        self._simulations = 200
        self._bootstrap_reps = 20
        self._seed: int | None = None
        self._device: int | None = None

    def predictors(self, names):
        self._predictors = [str(n) for n in names]
        return self

    def categorical_predictors(self, names):
        self._categorical = [str(n) for n in names]
        return self

    def quantiles(self, qs):
        self._quantiles = [float(q) for q in qs]
        return self

    def simulations(self, n: int):
        self._simulations = int(n)
        return self

    def bootstrap_reps(self, reps: int):
        self._bootstrap_reps = int(reps)
        return self

    def seed(self, seed: int | None):
        self._seed = None if seed is None else int(seed) & (2**64 - 1)
        return self

    def device(self, device: int | None):
        self._device = device
        return self

    def cluster(self, column: str | None, stratified: bool = False):
        """Accepted for symmetry with ``OaxacaBuilder.cluster``; ``run()`` then refuses: the Machado-Mata
        passes draw rows (MM-1), and a cluster bootstrap of them is not built."""
        self._cluster = None if column is None else str(column)
        return self

    def run(self) -> QuantileDecompositionResults:
        """quantile_decomposition.rs:281-445 on the MI355X engine."""
        if getattr(self, "_cluster", None) is not None:
            raise N.OaxacaError(N.OB_E_UNSUPPORTED, "cluster bootstrap: Machado-Mata is outside its scope")
        lib = N.lib()
        cfg = N.ob_qd_config()
        cfg.outcome, cfg.group, cfg.reference_group = (self.outcome.encode(), self.group.encode(),
                                                       self.reference_group.encode())
        keep = [_set_names(cfg, "predictors", self._predictors), _set_names(cfg, "categorical", self._categorical)]
        qs = np.ascontiguousarray(self._quantiles, dtype=np.float64)
        cfg.quantiles, cfg.n_quantiles = N.dp(qs), int(qs.size)
        cfg.simulations, cfg.bootstrap_reps = self._simulations, self._bootstrap_reps
        cfg.has_seed = 0 if self._seed is None else 1
        cfg.seed = 0 if self._seed is None else self._seed
        h = _frame_call("ob_quantile_decomposition_run", self._frame, cfg, keep, policy=CONTEXT_FIRST,
                        device=self._device)
        try:
            n, na, nb = C.c_int32(), C.c_int64(), C.c_int64()
            N.check(lib.ob_qd_results_dims(h, C.byref(n), C.byref(na), C.byref(nb)))
            out = {}
            for i in range(n.value):
                key = C.c_char_p()
                comps = (N.ob_component * 3)()
                N.check(lib.ob_qd_results_get(h, i, C.byref(key), comps))
                cr = [ComponentResult(c.name.decode(), c.estimate, c.std_err, c.t_stat, c.p_value, c.ci_lower,
                                      c.ci_upper) for c in comps]
                out[key.value.decode()] = QuantileDecompositionDetail(*cr)
            return QuantileDecompositionResults(out, int(na.value), int(nb.value),
                                                int(lib.ob_qd_results_n_failed(h)))
        finally:
            lib.ob_qd_results_free(h)


@dataclass
class DflResult:
    """dfl.rs:10-19 / python.rs:348-382 (``PyDflResult``): the grid and the three densities. The
    remaining fields are what ``ob_dfl_results_info`` reports about the run."""
    grid: np.ndarray
    density_a: np.ndarray
    density_b: np.ndarray
    density_b_counterfactual: np.ndarray
    n_a: int = 0
    n_b: int = 0
    group_a: str = ""
    logit_iterations: int = 0
    logit_converged: bool = False
    bandwidth_a: float = float("nan")
    bandwidth_b: float = float("nan")
    logit_ms: float = 0.0
    kde_ms: float = 0.0

    def to_json(self) -> str:
        """The reference's ``#[derive(Serialize)]`` fields, in its order."""
        return json.dumps({"grid": self.grid.tolist(), "density_a": self.density_a.tolist(),
                           "density_b": self.density_b.tolist(),
                           "density_b_counterfactual": self.density_b_counterfactual.tolist()})

    def plot(self):
        """python.rs:362-381: the three densities on one matplotlib figure (returned)."""
        try:
            import matplotlib.pyplot as plt
        except ImportError as e:
            raise ImportError("DflResult.plot() needs matplotlib, which is not installed") from e
        fig = plt.figure()
        ax = fig.gca()
        ax.plot(self.grid, self.density_a)
        ax.plot(self.grid, self.density_b)
        ax.plot(self.grid, self.density_b_counterfactual)
        ax.legend(["Group A", "Group B", "Group B (Counterfactual)"])
        ax.set_title("DFL Decomposition: Density Estimates")
        return fig


def run_dfl(dataframe, outcome: str, group: str, reference_group: str, predictors, device: int | None = None,
            grid_size: int = 0) -> DflResult:
    """dfl.rs:34-195 on the MI355X engine (``ob_dfl_run``). ``dataframe`` is what ``OaxacaBuilder``
    takes; ``grid_size`` 0 is the reference's 100 points."""
    lib = N.lib()
    frame = dataframe if isinstance(dataframe, Frame) else Frame(dataframe)
    cfg = N.ob_dfl_config()
    cfg.outcome, cfg.group, cfg.reference_group = outcome.encode(), group.encode(), reference_group.encode()
    keep = _set_names(cfg, "predictors", [str(p) for p in predictors])
    cfg.grid_size = int(grid_size)
    h = _frame_call("ob_dfl_run", frame, cfg, keep, policy=CONTEXT_FIRST, device=device)
    try:
        ng = C.c_int64()
        ptrs = [C.POINTER(C.c_double)() for _ in range(4)]
        N.check(lib.ob_dfl_results_get(h, C.byref(ng), *[C.byref(p) for p in ptrs]))
        arrs = [N.array_copy(p, (ng.value,)) for p in ptrs]
        info = N.ob_dfl_info()
        N.check(lib.ob_dfl_results_info(h, C.byref(info)))
        return DflResult(*arrs, n_a=int(info.n_a), n_b=int(info.n_b), group_a=info.group_a.decode(),
                         logit_iterations=int(info.logit_iterations), logit_converged=bool(info.logit_converged),
                         bandwidth_a=info.bandwidth_a, bandwidth_b=info.bandwidth_b, logit_ms=info.logit_ms,
                         kde_ms=info.kde_ms)
    finally:
        lib.ob_dfl_results_free(h)


def run_dfl_from_csv(csv_path, outcome: str, group: str, reference_group: str, predictors,
                     device: int | None = None, grid_size: int = 0) -> DflResult:
    """python.rs:316-346: the CSV read by the native reader (``ob_csv_read``), then ``run_dfl``."""
    from .frame import read_csv

    return run_dfl(read_csv(csv_path), outcome, group, reference_group, predictors, device=device,
                   grid_size=grid_size)


@dataclass
class MatchResult:
    """What ``ob_match_run`` returns: the reference's weights, and as an extension each treated
    row's neighbours (frame positions, -1 past min(k, n_control)) and their squared distances."""
    weights: np.ndarray
    treated_rows: np.ndarray
    neighbor_rows: np.ndarray
    neighbor_dist2: np.ndarray
    n_treated: int = 0
    n_control: int = 0
    logistic_iterations: int = 0
    logistic_converged: bool = False
    knn_ms: float = 0.0
    prep_ms: float = 0.0


_MATCH_METHODS = {"mahalanobis": N.OB_MATCH_MAHALANOBIS, "psm": N.OB_MATCH_PSM}


class MatchingEngine:
    """matching/engine.rs:10-284 on the MI355X engine (``ob_match_run``). ``dataframe`` is what
    ``OaxacaBuilder`` takes. Ties among exactly equidistant controls go to the smaller control
    position (the reference's depend on its tree's shape)."""

    def __init__(self, dataframe, treatment_col: str, outcome_col: str, covariates, device: int | None = None):
        self._frame = dataframe if isinstance(dataframe, Frame) else Frame(dataframe)
        self._treatment, self._outcome = str(treatment_col), str(outcome_col)
        self._covariates = [str(c) for c in covariates]
        self._device = device

    def run(self, k: int, method: int) -> MatchResult:
        lib = N.lib()
        cfg = N.ob_match_config()
        cfg.treatment, cfg.outcome = self._treatment.encode(), self._outcome.encode()
        keep = _set_names(cfg, "covariates", self._covariates)
        cfg.k, cfg.method = int(k), int(method)
        h = _frame_call("ob_match_run", self._frame, cfg, keep, policy=CONTEXT_FIRST, device=self._device)
        try:
            n, nt, kk = C.c_int64(), C.c_int64(), C.c_int32()
            w, d2 = C.POINTER(C.c_double)(), C.POINTER(C.c_double)()
            tr, nb = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)()
            N.check(lib.ob_match_results_get(h, C.byref(n), C.byref(w), C.byref(nt), C.byref(kk), C.byref(tr),
                                             C.byref(nb), C.byref(d2)))
            info = N.ob_match_info()
            N.check(lib.ob_match_results_info(h, C.byref(info)))
            return MatchResult(N.array_copy(w, (n.value,)), N.array_copy(tr, (nt.value,)),
                               N.array_copy(nb, (nt.value, kk.value)), N.array_copy(d2, (nt.value, kk.value)),
                               n_treated=int(info.n_treated), n_control=int(info.n_control),
                               logistic_iterations=int(info.logistic_iterations),
                               logistic_converged=bool(info.logistic_converged), knn_ms=info.knn_ms,
                               prep_ms=info.prep_ms)
        finally:
            lib.ob_match_results_free(h)

    def run_matching(self, k: int, use_mahalanobis: bool = False) -> list:
        """engine.rs:113-229: the weight of every row."""
        return self.match_nearest_neighbor(k, use_mahalanobis).tolist()

    def match_nearest_neighbor(self, k: int, use_mahalanobis: bool = False) -> np.ndarray:
        """engine.rs:103-110."""
        return self.run(k, N.OB_MATCH_MAHALANOBIS if use_mahalanobis else N.OB_MATCH_EUCLIDEAN).weights

    def match_psm(self, k: int) -> list:
        """engine.rs:232-283."""
        return self.run(k, N.OB_MATCH_PSM).weights.tolist()

    def neighbors(self, k: int, use_mahalanobis: bool = False):
        """(idx, dist2), both (n_treated, k): each treated row's neighbours as frame positions and
        their squared distances (an extension; the reference returns the weights only)."""
        r = self.run(k, N.OB_MATCH_MAHALANOBIS if use_mahalanobis else N.OB_MATCH_EUCLIDEAN)
        return r.neighbor_rows, r.neighbor_dist2


def match_units(csv_path, treatment: str, outcome: str, covariates, k: int = 1, method: str = "euclidean",
                device: int | None = None) -> list:
    """python.rs:387-423: the CSV read by the native reader, then the weights. Any method other than
    "psm" or "mahalanobis" is Euclidean (python.rs:411-420)."""
    from .frame import read_csv

    eng = MatchingEngine(read_csv(csv_path), treatment, outcome, covariates, device=device)
    return eng.run(k, _MATCH_METHODS.get(method, N.OB_MATCH_EUCLIDEAN)).weights.tolist()


@dataclass
class AkmResult:
    """akm.rs:39-44 as python.rs exposes it (``PyAkmResult``): ``beta`` in control order, the worker and
    firm effects as dicts from id string to effect, ``r2``; ``info`` is what ``ob_akm_results_info``
    reports (rows kept, counts, per-column demean iterations, recover_fe iterations, HIP-event ms)."""
    beta: list
    worker_effects: dict
    firm_effects: dict
    r2: float
    info: dict = field(default_factory=dict)


class AkmBuilder:
    """akm.rs:47-111 on the MI355X engine (``ob_akm_run``). ``dataframe`` is what ``OaxacaBuilder``
    takes. Among components with equally many nodes the one holding the smallest sorted worker id is
    kept (the reference's pick follows its HashMap's iteration order)."""

    def __init__(self, dataframe, outcome: str, worker_col: str, firm_col: str, device: int | None = None):
        self._frame = dataframe if isinstance(dataframe, Frame) else Frame(dataframe)
        self._outcome, self._worker, self._firm = str(outcome), str(worker_col), str(firm_col)
        self._controls: list = []
        self._tolerance, self._max_iters = 1e-8, 1000
        self._device = device

    def controls(self, controls):
        self._controls = [str(c) for c in controls]
        return self

    def tolerance(self, tol: float):
        self._tolerance = float(tol)
        return self

    def max_iters(self, iters: int):
        if int(iters) < 0:
            raise ValueError("max_iters is unsigned")
        self._max_iters = int(iters)
        return self

    def run(self) -> AkmResult:
        lib = N.lib()
        cfg = N.ob_akm_config()
        cfg.outcome, cfg.worker_col, cfg.firm_col = self._outcome.encode(), self._worker.encode(), self._firm.encode()
        keep = _set_names(cfg, "controls", self._controls)
        cfg.tolerance, cfg.max_iters = self._tolerance, self._max_iters
        h = _frame_call("ob_akm_run", self._frame, cfg, keep, policy=CONTEXT_FIRST, device=self._device)
        try:
            k, nw, nf, r2 = C.c_int32(), C.c_int64(), C.c_int64(), C.c_double()
            beta, alpha, psi = (C.POINTER(C.c_double)() for _ in range(3))
            wid, fid = C.POINTER(C.c_char_p)(), C.POINTER(C.c_char_p)()
            N.check(lib.ob_akm_results_get(h, C.byref(k), C.byref(beta), C.byref(nw), C.byref(wid), C.byref(alpha),
                                           C.byref(nf), C.byref(fid), C.byref(psi), C.byref(r2)))
            info = N.ob_akm_info()
            N.check(lib.ob_akm_results_info(h, C.byref(info)))
            return AkmResult(
                [beta[j] for j in range(k.value)],
                {wid[i].decode(): alpha[i] for i in range(nw.value)},
                {fid[i].decode(): psi[i] for i in range(nf.value)}, r2.value,
                {"n_rows_kept": int(info.n_rows_kept), "n_workers": int(info.n_workers),
                 "n_firms": int(info.n_firms), "n_components": int(info.n_components),
                 "demean_iterations": [int(info.demean_iterations[j]) for j in range(info.n_demean)],
                 "recover_iterations": int(info.recover_iterations),
                 "launches_per_iteration": int(info.launches_per_iteration), "demean_ms": info.demean_ms,
                 "ols_ms": info.ols_ms, "recover_ms": info.recover_ms})
        finally:
            lib.ob_akm_results_free(h)


def estimate_akm(csv_path, outcome: str, worker_col: str, firm_col: str, controls=None, tolerance: float = 1e-8,
                 max_iters: int = 1000, device: int | None = None) -> AkmResult:
    """python.rs ``estimate_akm``: the CSV read by the native reader, then ``AkmBuilder.run``."""
    from .frame import read_csv

    b = AkmBuilder(read_csv(csv_path), outcome, worker_col, firm_col, device=device)
    return b.controls(controls or []).tolerance(tolerance).max_iters(max_iters).run()


@dataclass
class VifResult:
    """math/diagnostics.rs:12-18: a predictor's name and its variance inflation factor."""
    variable_name: str
    vif_score: float


def calculate_vif(dataframe, predictor_names, device: int | None = None) -> list:
    """math/diagnostics.rs:29-109 on the MI355X engine (``ob_vif_run``): one ``VifResult`` per name, in
    the order given. ``dataframe`` is what ``OaxacaBuilder`` takes. Fewer than two names, a Cholesky
    failure of any auxiliary fit (perfect multicollinearity) and too few rows raise as the reference
    returns its errors; a null in a named column raises OB_E_INVALID (the reference would read it as
    0.0 in the regressand and as missing in the regressors)."""
    frame = dataframe if isinstance(dataframe, Frame) else Frame(dataframe)
    names = [str(p) for p in predictor_names]
    pp, keep = N.strs(names)
    out = np.empty(len(names))
    _frame_call("ob_vif_run", frame, None, keep, pp, len(names), N.dp(out), policy=CONTEXT_FIRST, device=device, handles=0)
    return [VifResult(nm, float(s)) for nm, s in zip(names, out)]
