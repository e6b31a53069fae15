"""RIF statistics on the GPU: ob_rif_stat against the numpy reference of tests/rif_stat_ref.py
within 8 E per statistic (floor 1e-12; E is what `python tests/rif_stat_ref.py` measures against longdouble), the
host's ob_rif(tau_hi) - ob_rif(tau_lo) as the second yardstick of the quantile range, ties, row order, determinism,
and decompose_statistic(s) end to end. All tests need an MI355X.

Largest mixed errors seen on the MI355X beside the 1e-12 bound: variance 6.7e-16, gini 2.94e-14 (n = 70,001, the
reference's own cumsum error), iqr 8.9e-16, iqr against the host's ob_rif difference 1.25e-14."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rif_stat_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

STATS = [("variance", {}), ("gini", {})] + [("iqr", {"upper": u, "lower": l}) for u, l in R.IQR_PAIRS]
SEED = 0x51A7


@pytest.fixture(scope="module")
def data(ob):
    """The inputs for the library's scan block and their f64 references, computed once."""
    block = ob.rif_scan_block()
    ys = R.inputs(block)
    refs = {(name, i): R.rif_statistic(y, s, **kw) for name, y in ys.items() for i, (s, kw) in enumerate(STATS)}
    return block, ys, refs


def _check(ob, data, name):
    _, ys, refs = data
    y = ys[name]
    for i, (stat, kw) in enumerate(STATS):
        rif, value = ob.rif_statistic(y, stat, **kw)
        ref_rif, ref_value = refs[(name, i)]
        e = R.mixed_error(rif, value, ref_rif, ref_value)
        print(f"{name} n={len(y)} {stat} {kw}: mixed error {e:.3e} (bound {R.TOL[stat]:.1e})")
        assert np.all(np.isfinite(rif)) and e <= R.TOL[stat], (name, stat, kw, e)
        if stat == "iqr":  # the second yardstick: the host's quantile RIFs
            host = ob.rif(y, kw["upper"]) - ob.rif(y, kw["lower"])
            eh = float(np.max(np.abs(rif - host) / np.maximum(np.abs(host), abs(ref_value))))
            print(f"    against ob_rif(hi) - ob_rif(lo): {eh:.3e}")
            assert eh <= R.TOL[stat], (name, kw, eh)


@pytest.mark.parametrize("name", ["n2", "n3", "n64"])
def test_one_wave_no_carry(ob, data, name):
    _check(ob, data, name)


def test_first_block_boundary(ob, data):
    block = data[0]
    assert block == R.SCAN_BLOCK or f"n{block + 1}" in data[1]
    _check(ob, data, "n257")
    _check(ob, data, f"n{block + 1}")


def test_several_blocks_with_carries(ob, data):
    _check(ob, data, "n70001")


def test_heavy_ties(ob, data):
    """Integers in [0, 9] at n = 1,000, and a tie run across the scan-block boundary at n = block + 1: the ranks
    and GL of a run are those of its last element, so tied rows get one RIF value."""
    for name in ("ties", "straddle"):
        _check(ob, data, name)
        y = data[1][name]
        for stat, kw in STATS:
            rif, _ = ob.rif_statistic(y, stat, **kw)
            for v in np.unique(y)[:12]:
                assert len(np.unique(rif[y == v])) == 1, (name, stat, v)
    y = data[1]["straddle"]
    top = np.max(y)
    assert np.sum(y == top) == 5 and np.sum(np.sort(y)[: data[0]] == top) == 4  # four of the run before the boundary


def test_constant_outcome(ob, data):
    _check(ob, data, "constant")
    y = data[1]["constant"]
    rif, value = ob.rif_statistic(y, "variance")
    assert np.array_equal(rif, np.zeros(len(y))) and value == 0.0


def test_exact_zeros_among_positive_values(ob, data):
    _check(ob, data, "zeros")


def test_row_order_does_not_matter(ob, data):
    """Ascending, descending and shuffled input: the same statistic bytes and, after undoing the permutation, the
    same RIF bytes per row. Every sum runs over the sorted values."""
    block = data[0]
    rng = np.random.default_rng(3)
    y = np.sort(np.concatenate([R.wages(2 * block + 30, 5), np.full(7, 20.0)]))
    perm = rng.permutation(len(y))
    for stat, kw in STATS:
        asc, v_asc = ob.rif_statistic(y, stat, **kw)
        desc, v_desc = ob.rif_statistic(y[::-1].copy(), stat, **kw)
        shuf, v_shuf = ob.rif_statistic(y[perm], stat, **kw)
        assert v_asc == v_desc == v_shuf
        assert np.array_equal(asc, desc[::-1]) and np.array_equal(asc[perm], shuf)


def test_determinism(ob, data):
    for name in ("n257", "n70001"):
        y = data[1][name]
        for stat, kw in STATS:
            a, va = ob.rif_statistic(y, stat, **kw)
            b, vb = ob.rif_statistic(y, stat, **kw)
            assert a.tobytes() == b.tobytes() and va == vb
    t = ob.rif_last_timing()
    assert t["sort_ms"] > 0 and t["scan_ms"] > 0 and t["scatter_ms"] > 0 and t["kde_ms"] > 0


# ---- end to end -------------------------------------------------------------------------------------------
N_A, N_B = 400, 417


def _frame(clusters=None):
    rng = np.random.default_rng(11)
    n = N_A + N_B
    g = np.array(["A"] * N_A + ["B"] * N_B)
    order = rng.permutation(n)  # the groups interleaved, so that the frame order is not the panel order
    x = rng.normal(size=(n, 3))
    shift = np.where(g == "A", 0.25, 0.0)
    y = np.exp(2.5 + shift + x @ np.array([0.3, -0.2, 0.1]) + rng.normal(0, 0.4 + 0.2 * (g == "A"), n))
    f = {"y": y[order], "g": list(g[order]), "x0": x[order, 0], "x1": x[order, 1], "x2": x[order, 2]}
    if clusters:
        f["firm"] = rng.integers(0, clusters, n)
        f["firm"][:clusters] = np.arange(clusters)  # every cluster occurs
    return f


def _builder(ob, f, ref, reps=64):
    return (ob.OaxacaBuilder(f, "y", "g", "B").predictors(["x0", "x1", "x2"]).bootstrap_reps(reps)
            .reference_coefficients(ref).seed(SEED))


def _replaced(f, fn):
    """The frame with the outcome of each group replaced by fn(group's outcome), group by group in frame order."""
    y, g = np.asarray(f["y"], dtype=np.float64), np.array(f["g"])
    out = y.copy()
    for level in ("A", "B"):
        out[g == level] = fn(y[g == level])
    return dict(f, y=out)


def _numbers(res):
    tables = [res.two_fold.aggregate, res.two_fold.detailed_explained, res.two_fold.detailed_unexplained,
              res.three_fold.aggregate]
    comps = [c for t in tables for c in t]
    v = [[c.estimate, c.std_err, c.ci_lower, c.ci_upper, c.t_stat, c.p_value] for c in comps]
    return np.concatenate([np.ravel(v), [res.total_gap], res.residuals, res.beta_star, res.xa_mean, res.xb_mean])


def _bitwise(a, b):
    assert a.n_a == b.n_a and a.n_b == b.n_b and a.n_failed == b.n_failed
    assert np.array_equal(_numbers(a), _numbers(b), equal_nan=True)


def _close(res, ref):
    """The parity suite's bound: 1e-6 * max(|ref|, |total_gap|) on estimates, standard errors and interval ends."""
    tables = lambda r: [r.two_fold.aggregate, r.two_fold.detailed_explained, r.two_fold.detailed_unexplained,  # noqa: E731
                        r.three_fold.aggregate]
    assert abs(res.total_gap - ref.total_gap) <= 1e-6 * abs(ref.total_gap)
    for ta, tb in zip(tables(res), tables(ref)):
        assert [c.name for c in ta] == [c.name for c in tb]
        for a, b in zip(ta, tb):
            for fld in ("estimate", "std_err", "ci_lower", "ci_upper"):
                va, vb = getattr(a, fld), getattr(b, fld)
                assert abs(va - vb) <= 1e-6 * max(abs(vb), abs(ref.total_gap)), (a.name, fld, va, vb)


@pytest.mark.parametrize("ref", ["GroupA", "GroupB", "Pooled", "Weighted"])
def test_decompose_statistic_end_to_end(ob, ref):
    mode = ob.ReferenceCoefficients[ref]
    f = _frame()
    b = _builder(ob, f, mode)
    many = b.decompose_statistics([(s, kw) for s, kw in STATS])
    assert len(many) == len(STATS)
    for t, (stat, kw) in enumerate(STATS):
        res = b.decompose_statistic(stat, **kw)
        assert (res.n_a, res.n_b, res.n_failed, res.n_clusters) == (N_A, N_B, 0, None)
        _bitwise(res, _builder(ob, _replaced(f, lambda y: ob.rif_statistic(y, stat, **kw)[0]), mode).run())
        _close(res, _builder(ob, _replaced(f, lambda y: R.rif_statistic(y, stat, **kw)[0]), mode).run())
        _bitwise(many[t], res)
    via = ob.OaxacaBlinder(f, "y", "g", "B", ["x0", "x1", "x2"], bootstrap_reps=64, seed=SEED)
    if ref == "GroupA":  # the builder's default rule
        _bitwise(via.fit_statistic("iqr", upper=0.75, lower=0.25), many[3])


def _stacked(f):
    """A's rows over B's, each in frame order: the frame decompose_quantile(s) and decompose_statistic(s) hand to
    run(), as the reference's vstack does. Cluster ids are numbered by first appearance, so a clustered run
    draws the same clusters only on a frame in this order."""
    order = np.argsort(np.array(f["g"]), kind="stable")
    return {k: (list(np.array(v)[order]) if k == "g" else np.asarray(v)[order]) for k, v in f.items()}


@pytest.mark.parametrize("c", [5, 67])
def test_decompose_statistic_clustered(ob, c):
    f = _frame(clusters=c)
    mode = ob.ReferenceCoefficients.Pooled
    b = _builder(ob, f, mode).cluster("firm")
    many = b.decompose_statistics([(s, kw) for s, kw in STATS])
    for t, (stat, kw) in enumerate(STATS[:3]):
        res = b.decompose_statistic(stat, **kw)
        assert res.n_clusters == c
        replaced = _stacked(_replaced(f, lambda y: ob.rif_statistic(y, stat, **kw)[0]))
        want = _builder(ob, replaced, mode).cluster("firm").run()
        assert want.n_clusters == c
        _bitwise(res, want)
        _bitwise(many[t], res)
    plain = _builder(ob, f, mode).decompose_statistic("gini")
    assert plain.n_clusters is None and plain.total_gap == many[1].total_gap


def test_statistic_builder_serves_bca(ob):
    f = _frame()
    b = _builder(ob, f, ob.ReferenceCoefficients.GroupA)
    res = b.decompose_statistic("gini")
    sb = b.statistic_builder("gini")
    bca = sb.run_bca()
    for ta, tb in ((res.two_fold.aggregate, bca.two_fold.aggregate),
                   (res.two_fold.detailed_explained, bca.two_fold.detailed_explained),
                   (res.two_fold.detailed_unexplained, bca.two_fold.detailed_unexplained)):
        assert [(c.name, c.estimate, c.std_err) for c in ta] == [(c.name, c.estimate, c.std_err) for c in tb]
        assert all(np.isfinite(c.ci_lower) and np.isfinite(c.ci_upper) and c.ci_lower <= c.ci_upper for c in tb)
    assert bca.total_gap == res.total_gap and bca.jackknife
    _bitwise(sb.run(), res)
    jk = sb.jackknife()
    assert np.all(np.isfinite(jk.accel))


def test_variance_gap_sanity_panel(ob):
    """Two groups with the same mean log wage and the same predictor distribution, A with twice the residual
    variance: the variance gap sits in `unexplained`, with its sign, and the mean decomposition of the same panel
    shows a gap inside its own bootstrap interval of 0."""
    rng = np.random.default_rng(23)
    n = 3000
    g = np.array(["A", "B"] * n)
    x = rng.normal(size=(2 * n, 2))
    sd = np.where(g == "A", np.sqrt(0.5), 0.5)  # residual variance 0.5 against 0.25
    y = 3.0 + x @ np.array([0.4, -0.3]) + rng.normal(size=2 * n) * sd
    f = {"y": y, "g": list(g), "x0": x[:, 0], "x1": x[:, 1]}
    b = ob.OaxacaBuilder(f, "y", "g", "B").predictors(["x0", "x1"]).bootstrap_reps(200).seed(SEED)
    res = b.decompose_statistic("variance")
    va, vb = np.var(y[g == "A"]), np.var(y[g == "B"])
    assert abs(res.total_gap - (va - vb)) <= 1e-12 * va  # mean(RIF) = sigma^2 in each group
    un, ex = res.unexplained(), res.explained()
    assert un.estimate > 0 and un.estimate >= 0.9 * res.total_gap and abs(ex.estimate) <= 0.1 * res.total_gap
    assert un.ci_lower > 0
    mean = b.run()
    gap_se = np.sqrt(va / n + vb / n)
    assert abs(mean.total_gap) <= 4 * gap_se  # equal means by construction
    for c in mean.two_fold.aggregate:
        assert c.ci_lower <= 0.0 <= c.ci_upper or abs(c.estimate) <= 4 * gap_se
