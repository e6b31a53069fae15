"""decompose_quantile(s)(refit=True) and its prepared handle on the GPU (csrc/ob_rifq.hip) against the
oracle of tests/rifq_ref.py: per group the rows in stable ascending order of y, per replicate O.resample_indices into
that order, O.rif of the resampled outcome and O.single_pass of the resampled designs.

Groups of 130 and 257 rows: a ragged sub-tile, two tiles, and -- checked below through ob_debug_chunks -- group B over
two chunks of the engine's own chunk table (257 is the smallest group size that does so beside a one-tile group), so
row prefixes cut the first and the second chunk and whole-chunk totals enter the masked sums. K = 3 and 9 with one
categorical; GroupA, GroupB, Weighted and Pooled beta*; one and three quantiles; 64 + 3 replicates. Tolerance: the
parity suite's 1e-6 relative to max(|ref|, |total_gap|), unchanged; the row tail's q bitwise."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rifq_ref as R  # noqa: E402
from test_gpu_parity import RTOL, SEED, close  # noqa: E402

pytestmark = pytest.mark.gpu

REPS = 64 + 3
REFS = ["GroupA", "GroupB", "Weighted", "Pooled"]
OREF = {"GroupA": "group_a", "GroupB": "group_b", "Weighted": "weighted", "Pooled": "pooled"}
_cache = {}


def builder(ob, k, ref, reps=REPS):
    f, xs, cs = R.frame(k)
    return (ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).categorical_predictors(cs).bootstrap_reps(reps)
            .reference_coefficients(getattr(ob.ReferenceCoefficients, ref)).seed(SEED))


def oracle(ob, O, k, ref, taus):
    """Point rows (T, rl) and replicate rows (T, REPS, rl) of a case, computed once and shared (read-only)."""
    key = (k, ref, tuple(taus))
    if key not in _cache:
        xa, ya, xb, yb, _ = builder(ob, k, ref).get_data_matrices()
        _, xs, _ = R.frame(k)
        xa, ya, xb, yb, _, _ = R.sorted_designs(xa, ya, xb, yb)
        cfg = O.PassConfig(k, len(xs), O.REF[OREF[ref]], False)
        point = np.stack([R.oracle_row(O, cfg, xa, ya, xb, yb, tau)[1] for tau in taus])
        rows, ok = R.oracle_boot(O, cfg, xa, ya, xb, yb, taus, SEED, 0, REPS)
        for a in (point, rows, ok):
            a.setflags(write=False)
        _cache[key] = (point, rows, ok)
    return _cache[key]


def check_rows(got, want, label):
    rl0 = got.shape[-1] - 6
    assert np.array_equal(got[..., rl0:rl0 + 2], want[..., rl0:rl0 + 2]), label  # q_A, q_B bitwise
    assert np.array_equal(got[..., rl0 + 4:], want[..., rl0 + 4:]), label  # N_le exactly
    gap = want[..., 5:6]
    scale = np.maximum(np.abs(want), np.abs(gap))
    err = np.abs(got - want) / scale
    print(label, f"max rel err {np.nanmax(err):.3e}")
    assert np.all(np.abs(got - want) <= RTOL * scale), (label, float(np.nanmax(err)))


@pytest.mark.parametrize("taus", [(0.9,), R.TAUS], ids=["one", "three"])
@pytest.mark.parametrize("ref", REFS)
@pytest.mark.parametrize("k", [3, 9])
def test_rows_match_oracle(ob, O, k, ref, taus):
    point, rows, ook = oracle(ob, O, k, ref, taus)
    pr = builder(ob, k, ref).prepare_quantiles_refit(taus)
    try:
        assert pr.row_len == ob.rifq_row_len(k) == point.shape[1]
        got_point = pr.point_row().reshape(len(taus), -1)
        got, ok = pr.boot(0, REPS)
    finally:
        pr.close()
    assert np.array_equal(ok, ook)
    check_rows(got_point, point, ("point", k, ref))
    m = ok.astype(bool)
    check_rows(got[m], rows[m], ("rows", k, ref))


@pytest.mark.parametrize("ref", ["GroupA", "Pooled"])
def test_statistics_match_bootstrap_stats_of_oracle_rows(ob, O, ref):
    k = 3
    point, rows, ook = oracle(ob, O, k, ref, R.TAUS)
    res = builder(ob, k, ref).decompose_quantiles(R.TAUS, refit=True)
    for t, r in enumerate(res):
        assert r.n_failed == int((ook[t] == 0).sum())
        good = rows[t][ook[t].astype(bool)]
        for i, c in enumerate(r.two_fold.aggregate):
            se, pv, (lo, hi) = O.bootstrap_stats(good[:, i])
            gap = abs(point[t, 5])
            assert close([c.estimate, c.std_err, c.ci_lower, c.ci_upper], [point[t, i], se, lo, hi], gap), (t, c.name)
            assert abs(c.p_value - pv) <= RTOL
        assert r.quantile_values == (point[t, -6], point[t, -5])
        assert r.n_density_floored == 0 and "quantile_values" in r.to_json()
    plain = builder(ob, k, ref, reps=8).decompose_quantiles([0.5])[0]
    assert plain.quantile_values is None and "quantile_values" not in plain.to_json()


def test_group_b_spans_two_engine_chunks(ob, N):
    pr = builder(ob, 3, "GroupA", reps=8).prepare_quantiles_refit([0.5])
    try:
        panel = N.lib().ob_prepared_panel(pr._h)
        nc = C.c_int32(0)
        N.check(N.lib().ob_debug_chunks(panel, None, 0, C.byref(nc)))
        table = (C.c_uint32 * (3 * nc.value))()
        N.check(N.lib().ob_debug_chunks(panel, table, nc.value, C.byref(nc)))
        groups = [table[3 * i] for i in range(nc.value)]
        assert groups.count(1) >= 2  # the parity cases above run with two chunks in group B
    finally:
        pr.close()


def test_bitwise_determinism(ob):
    """Replicates 0..66 in one boot, in boots of 1, 16 and 51, and at first_rep = 40 give the same bytes; element t of
    a three-tau run is bitwise the single-tau run."""
    b = builder(ob, 3, "Weighted")
    pr = b.prepare_quantiles_refit(R.TAUS)
    try:
        full, ok = pr.boot(0, REPS)
        for lo, n in ((0, 1), (0, 16), (16, 51), (40, 27), (40, 1)):
            part, pok = pr.boot(lo, n)
            assert part.tobytes() == np.ascontiguousarray(full[:, lo:lo + n]).tobytes(), (lo, n)
            assert np.array_equal(pok, ok[:, lo:lo + n])
        point3 = pr.point_row().reshape(3, -1)
    finally:
        pr.close()
    for t, tau in enumerate(R.TAUS):
        p1 = b.prepare_quantiles_refit([tau])
        try:
            one, _ = p1.boot(0, REPS)
            assert one[0].tobytes() == np.ascontiguousarray(full[t]).tobytes(), tau
            assert p1.point_row().tobytes() == point3[t].tobytes(), tau
        finally:
            p1.close()


def test_consistency(ob):
    k, tau = 3, 0.9
    b = builder(ob, k, "GroupA")
    pr = b.prepare_quantiles_refit([tau])
    try:
        rows, ok = pr.boot(0, REPS)
        point = pr.point_row()
        info = pr.rifq_info()
    finally:
        pr.close()
    na, nb = len(info["perm_a"]), len(info["perm_b"])
    assert sorted(info["perm_a"].tolist()) == list(range(na)) and sorted(info["perm_b"].tolist()) == list(range(nb))
    for row in [point] + list(rows[0][ok[0].astype(bool)]):  # total_gap = mean RIF_A - mean RIF_B
        qa, qb, fa, fb, la, lb = row[-6:]
        want = (qa + (tau - la / na) / fa) - (qb + (tau - lb / nb) / fb)
        # relative to the two mean RIFs whose difference the gap is (each near q, ten times the gap here): the row's
        # total_gap comes out of the solve, whose rounding scales with those terms, not with their difference
        assert abs(row[5] - want) <= 1e-12 * max(abs(want), abs(qa), abs(qb))
    fixed = b.decompose_quantiles([tau])[0]
    refit = b.decompose_quantiles([tau], refit=True)[0]
    coef = max(abs(v) for v in point[6 + 2 * k:6 + 4 * k])  # the largest coefficient
    for cf, cr in zip(fixed.two_fold.aggregate + fixed.two_fold.detailed_explained + fixed.two_fold.detailed_unexplained,
                      refit.two_fold.aggregate + refit.two_fold.detailed_explained + refit.two_fold.detailed_unexplained):
        assert cf.name == cr.name and abs(cf.estimate - cr.estimate) <= 1e-9 * coef, cf.name
    assert abs(fixed.total_gap - refit.total_gap) <= 1e-9 * coef
    gap_f = np.array([c.std_err for c in fixed.two_fold.aggregate])
    gap_r = np.array([c.std_err for c in refit.two_fold.aggregate])
    assert np.all(np.abs(gap_r - gap_f) > 1e-6 * np.abs(gap_f))
    # The sharper form: the fixed-RIF bootstrap over the same y-sorted rows, so that both runs draw the same rows of
    # every replicate and only the refit differs. run() on the sorted frame whose outcome is the point RIF.
    f, xs, cs = R.frame(k)
    y = np.array(f["y"])
    order = np.concatenate([np.argsort(y[:na], kind="stable"), na + np.argsort(y[na:], kind="stable")])
    rif = np.concatenate([ob.rif(y[:na], tau), ob.rif(y[na:], tau)])
    fs = {name: [col[i] for i in order] for name, col in f.items()}
    fs["y"] = rif[order].tolist()
    pf = (ob.OaxacaBuilder(fs, "y", "g", "B").predictors(xs).categorical_predictors(cs).bootstrap_reps(REPS)
          .seed(SEED).prepare())
    try:
        frows, fok = pf.boot(0, REPS)
    finally:
        pf.close()
    assert fok.all() and ok.all()
    se_fixed = np.std(frows[:, 5], ddof=1)
    se_refit = np.std(rows[0][:, 5], ddof=1)
    print(f"total_gap SE at tau = {tau}, same draws: fixed RIF {se_fixed:.6f}, refit {se_refit:.6f}")
    assert abs(se_refit - se_fixed) > 1e-6 * se_fixed  # the refit is not a no-op
    assert np.abs(frows[:, 5] - rows[0][:, 5]).max() > 1e-6 * abs(point[5])  # replicate by replicate


def test_handle_refusals(ob, N):
    """Sharded boots, the jackknives and BCa refuse a refit handle; the refit's accessors refuse another handle."""
    def code(fn):
        with pytest.raises(N.OaxacaError) as e:
            fn()
        return e.value.code

    pr = builder(ob, 3, "GroupA", reps=8).prepare_quantiles_refit([0.5, 0.9])
    try:
        assert pr.n_taus == 2
        rows, ok = pr.boot(0, 8)
        assert rows.shape == (2, 8, pr.row_len) and ok.shape == (2, 8)
        assert code(lambda: pr.boot_sharded(0, 4)) == N.OB_E_UNSUPPORTED
        assert code(lambda: pr.jackknife()) == N.OB_E_UNSUPPORTED
        assert code(lambda: pr.finish_bca(rows[0], ok[0])) == N.OB_E_UNSUPPORTED
        assert code(lambda: pr.finish_cluster_bca(rows[0], ok[0])) in (N.OB_E_UNSUPPORTED, N.OB_E_INVALID)
        lib, dp, up = N.lib(), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        h = C.c_void_p()
        assert lib.ob_prepared_finish_tau(pr._h, 2, rows[0].ctypes.data_as(dp), ok[0].ctypes.data_as(up), 8,
                                          C.byref(h)) == N.OB_E_INVALID
        with pytest.raises(ValueError):  # the whole (T, n_reps, row_len) block is not one outcome's rows
            pr.finish(rows, ok)
        with pytest.raises(ValueError):
            pr.finish_bca(rows, ok)
        first = pr.finish(rows[0], ok[0])  # ob_prepared_finish is tau 0
        assert first.total_gap == pr.finish_tau(0, rows[0], ok[0]).total_gap
    finally:
        pr.close()
    plain = builder(ob, 3, "GroupA", reps=8).prepare()
    try:
        assert plain.n_taus == 0
        prow, pok = plain.boot(0, 8)
        assert code(lambda: plain.rifq_info()) == N.OB_E_INVALID
        assert code(lambda: plain.finish_tau(0, prow, pok)) == N.OB_E_INVALID
    finally:
        plain.close()


def test_c_decompose_entry_point_equals_python_route(ob, N):
    """ob_builder_decompose_quantiles_refit: out[t] is decompose_quantiles(refit=True)[t]."""
    from importlib import import_module

    api = import_module(ob.__name__ + ".api")
    b = builder(ob, 3, "Weighted", reps=16)
    want = b.decompose_quantiles(R.TAUS, refit=True)
    taus = np.ascontiguousarray(R.TAUS, dtype=np.float64)
    cols, ncol, nrow = b._frame.as_c()
    cfg, keep = b._config()
    hs = (C.c_void_p * 3)()
    N.check(N.lib().ob_builder_decompose_quantiles_refit(N.context(None), cols, ncol, nrow, C.byref(cfg),
                                                         taus.ctypes.data_as(C.POINTER(C.c_double)), 3,
                                                         C.cast(hs, C.POINTER(C.c_void_p))))
    got = [api._results_from_c(C.c_void_p(h)) for h in hs]
    for g, w in zip(got, want):
        assert g.total_gap == w.total_gap and g.n_failed == w.n_failed and len(g.residuals) == 0
        for cg, cw in zip(g.two_fold.aggregate + g.two_fold.detailed_explained + g.three_fold.aggregate,
                          w.two_fold.aggregate + w.two_fold.detailed_explained + w.three_fold.aggregate):
            assert cg == cw
