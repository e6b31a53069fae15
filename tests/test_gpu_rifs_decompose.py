"""decompose_statistic(s)(refit=True) and its prepared handle on the GPU (csrc/ob_rifs.hip) against
the oracle of tests/rifs_ref.py: per group the rows in stable ascending order of y, per replicate O.resample_indices
into that order, tests/rif_stat_ref.py's RIF of the resampled outcome and O.single_pass of the resampled designs.

Groups of 130 and 257 rows (rifq_ref.frame with the outcome as a wage, so that the Gini is defined): a ragged sub-tile,
two tiles, group B over two chunks of the engine's chunk table. K = 3 and 9 with one categorical; GroupA and Pooled
beta*; one and three statistics; 64 + 3 replicates. Tolerance: the parity suite's 1e-6 relative to
max(|ref|, |total_gap|), unchanged, with `ok` equal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rif_stat_ref as S  # noqa: E402
import rifq_ref as R  # noqa: E402
import rifs_ref as F  # noqa: E402
from test_gpu_parity import RTOL, SEED  # noqa: E402

pytestmark = pytest.mark.gpu

REPS = 64 + 3
OREF = {"GroupA": "group_a", "Pooled": "pooled"}
ONE = (("gini", {}),)
THREE = (("variance", {}), ("gini", {}), ("iqr", {"upper": 0.9, "lower": 0.1}))
_cache = {}


def builder(ob, k, ref, reps=REPS, frame=None):
    f, xs, cs = F.positive_frame(k)
    return (ob.OaxacaBuilder(frame or f, "y", "g", "B").predictors(xs).categorical_predictors(cs).bootstrap_reps(reps)
            .reference_coefficients(getattr(ob.ReferenceCoefficients, ref)).seed(SEED))


def oracle(ob, O, k, ref, stats):
    """Point rows (S, rl) and replicate rows (S, REPS, rl) of a case, computed once and shared (read-only)."""
    key = (k, ref, tuple(s[0] for s in stats))
    if key not in _cache:
        xa, ya, xb, yb, _ = builder(ob, k, ref).get_data_matrices()
        _, xs, _ = F.positive_frame(k)
        xa, ya, xb, yb, _, _ = R.sorted_designs(xa, ya, xb, yb)
        cfg = O.PassConfig(k, len(xs), O.REF[OREF[ref]], False)
        point = np.stack([F.oracle_row(O, cfg, xa, ya, xb, yb, st, p)[1] for st, p in stats])
        rows, ok = F.oracle_boot(O, cfg, xa, ya, xb, yb, stats, SEED, 0, REPS)
        for a in (point, rows, ok):
            a.setflags(write=False)
        _cache[key] = (point, rows, ok)
    return _cache[key]


def check_rows(got, want, label):
    gap = want[..., 5:6]
    scale = np.maximum(np.abs(want), np.abs(gap))
    err = np.abs(got - want) / scale
    print(label, f"max rel err {np.nanmax(err):.3e}")
    assert np.all(np.abs(got - want) <= RTOL * scale), (label, float(np.nanmax(err)))


@pytest.mark.parametrize("stats", [ONE, THREE], ids=["one", "three"])
@pytest.mark.parametrize("ref", ["GroupA", "Pooled"])
@pytest.mark.parametrize("k", [3, 9])
def test_rows_match_oracle(ob, O, k, ref, stats):
    point, rows, ook = oracle(ob, O, k, ref, stats)
    pr = builder(ob, k, ref).prepare_statistics_refit(stats)
    try:
        assert pr.row_len == ob.rifs_row_len(k) == point.shape[1] and pr.n_taus == len(stats)
        got_point = pr.point_row().reshape(len(stats), -1)
        got, ok = pr.boot(0, REPS)
    finally:
        pr.close()
    assert np.array_equal(ok, ook)
    check_rows(got_point, point, ("point", k, ref))
    m = ok.astype(bool)
    check_rows(got[m], rows[m], ("rows", k, ref))


def test_gini_refit_results_and_the_unchanged_default(ob, O):
    k, ref = 3, "GroupA"
    b = builder(ob, k, ref)
    point, rows, ook = oracle(ob, O, k, ref, ONE)
    res = b.decompose_statistic("gini", refit=True)
    f, xs, cs = F.positive_frame(k)
    y, g = np.array(f["y"]), np.array(f["g"])
    nu_a, nu_b = ob.rif_statistic(y[g == "A"], "gini")[1], ob.rif_statistic(y[g == "B"], "gini")[1]
    assert abs(res.statistic_values[0] - nu_a) <= 1e-12 and abs(res.statistic_values[1] - nu_b) <= 1e-12
    assert abs(res.statistic_values[0] - S.gini(y[g == "A"])[1]) <= 1e-12
    assert res.n_density_floored is None and "statistic_values" in res.to_json()
    assert res.n_failed == int((ook[0] == 0).sum())
    good = rows[0][ook[0].astype(bool)]
    for i, c in enumerate(res.two_fold.aggregate):
        se, pv, (lo, hi) = O.bootstrap_stats(good[:, i])
        scale = max(abs(point[0, 5]), 1e-300)
        for gv, wv in zip([c.estimate, c.std_err, c.ci_lower, c.ci_upper], [point[0, i], se, lo, hi]):
            assert abs(gv - wv) <= RTOL * max(abs(wv), scale), (c.name, gv, wv)
    rng = b.decompose_statistic("iqr", refit=True, upper=0.75, lower=0.25)
    assert rng.n_density_floored == 0 and rng.statistic_values is not None and "n_density_floored" in rng.to_json()
    # without refit: bitwise run() on the RIF column, as on the parent commit
    plain = b.decompose_statistic("gini")
    assert plain.statistic_values is None and "statistic_values" not in plain.to_json()
    fr = dict(f)
    rif = np.empty(len(y))
    rif[g == "A"] = ob.rif_statistic(y[g == "A"], "gini")[0]
    rif[g == "B"] = ob.rif_statistic(y[g == "B"], "gini")[0]
    fr["y"] = rif.tolist()
    want = builder(ob, k, ref, frame=fr).run()
    assert plain.to_json() == want.to_json()
    assert b.decompose_statistic("gini", refit=False).to_json() == want.to_json()
    # the refit moves the standard errors, not the point estimates
    for cf, cr in zip(plain.two_fold.aggregate, res.two_fold.aggregate):
        assert abs(cf.estimate - cr.estimate) <= 1e-9 * max(abs(cf.estimate), 1.0)
        assert abs(cf.std_err - cr.std_err) > 1e-6 * cf.std_err


def test_bitwise_determinism(ob):
    b = builder(ob, 3, "Pooled")
    pr = b.prepare_statistics_refit(THREE)
    try:
        full, ok = pr.boot(0, REPS)
        for lo, n in ((0, 1), (0, 16), (16, 51), (40, 1)):
            part, pok = pr.boot(lo, n)
            assert part.tobytes() == np.ascontiguousarray(full[:, lo:lo + n]).tobytes(), (lo, n)
            assert np.array_equal(pok, ok[:, lo:lo + n])
        point3 = pr.point_row().reshape(3, -1)
        info = pr.rifs_info()
    finally:
        pr.close()
    assert [s[0] for s in info["specs"]] == [0, 1, 2] and info["nu"].shape == (2, 3)
    assert sorted(info["perm_a"].tolist()) == list(range(130)) and sorted(info["perm_b"].tolist()) == list(range(257))
    for t, stat in enumerate(THREE):
        p1 = b.prepare_statistics_refit([stat])
        try:
            one, _ = p1.boot(0, REPS)
            assert one[0].tobytes() == np.ascontiguousarray(full[t]).tobytes(), stat
            assert p1.point_row().tobytes() == point3[t].tobytes(), stat
        finally:
            p1.close()


def test_refusals(ob, N):
    """Weights, cluster, normalize and Heckman settings arrive with OB_E_UNSUPPORTED; sharded boots, the jackknives
    and BCa refuse the handle; the accessor refuses another handle."""
    def code(fn):
        with pytest.raises(N.OaxacaError) as e:
            fn()
        return e.value.code

    f, xs, cs = F.positive_frame(3)
    n = len(f["y"])
    rng = np.random.default_rng(2)
    f = dict(f, w=rng.uniform(0.5, 2.0, n).tolist(), s=(rng.random(n) < 0.7).astype(float).tolist(),
             cl=rng.integers(0, 9, n).tolist())
    base = lambda: ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).categorical_predictors(cs).bootstrap_reps(8).seed(3)  # noqa: E731
    for mk in (lambda: base().weights("w"), lambda: base().normalize(cs), lambda: base().heckman_selection("s", xs[:1]),
               lambda: base().cluster("cl")):
        assert code(lambda: mk().decompose_statistic("gini", refit=True)) == N.OB_E_UNSUPPORTED
        assert code(lambda: mk().prepare_statistics_refit(THREE)) == N.OB_E_UNSUPPORTED
    pr = base().prepare_statistics_refit(THREE[:2])
    try:
        rows, ok = pr.boot(0, 8)
        assert rows.shape == (2, 8, pr.row_len) and ok.shape == (2, 8)
        assert code(lambda: pr.boot_sharded(0, 4)) == N.OB_E_UNSUPPORTED
        assert code(lambda: pr.jackknife()) == N.OB_E_UNSUPPORTED
        assert code(lambda: pr.finish_bca(rows[0], ok[0])) == N.OB_E_UNSUPPORTED
        assert code(lambda: pr.finish_cluster_bca(rows[0], ok[0])) in (N.OB_E_UNSUPPORTED, N.OB_E_INVALID)
        assert code(lambda: pr.rifq_info()) == N.OB_E_INVALID
        lib, dp, up = N.lib(), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        h = C.c_void_p()
        assert lib.ob_prepared_finish_tau(pr._h, 2, rows[0].ctypes.data_as(dp), ok[0].ctypes.data_as(up), 8,
                                          C.byref(h)) == N.OB_E_INVALID
        assert pr.finish(rows[0], ok[0]).total_gap == pr.finish_tau(0, rows[0], ok[0]).total_gap
    finally:
        pr.close()
    plain = base().prepare()
    try:
        assert plain.n_taus == 0 and code(lambda: plain.rifs_info()) == N.OB_E_INVALID
    finally:
        plain.close()


def test_c_decompose_entry_point_equals_python_route(ob, N):
    """ob_builder_decompose_statistics_refit: out[t] is decompose_statistics(refit=True)[t]."""
    from importlib import import_module

    api = import_module(ob.__name__ + ".api")
    eng = import_module(ob.__name__ + ".engine")
    b = builder(ob, 3, "GroupA", reps=16)
    want = b.decompose_statistics(THREE, refit=True)
    specs, parsed = eng._rif_specs(THREE)
    cols, ncol, nrow = b._frame.as_c()
    cfg, keep = b._config()
    hs = (C.c_void_p * 3)()
    N.check(N.lib().ob_builder_decompose_statistics_refit(N.context(None), cols, ncol, nrow, C.byref(cfg), specs, 3,
                                                          C.cast(hs, C.POINTER(C.c_void_p))))
    got = [api._results_from_c(C.c_void_p(h)) for h in hs]
    for g, w in zip(got, want):
        assert g.total_gap == w.total_gap and g.n_failed == w.n_failed and len(g.residuals) == 0
        for cg, cw in zip(g.two_fold.aggregate + g.two_fold.detailed_explained + g.three_fold.aggregate,
                          w.two_fold.aggregate + w.two_fold.detailed_explained + w.three_fold.aggregate):
            assert cg == cw
