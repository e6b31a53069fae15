"""Host pieces of the delete-one-cluster jackknife: every limit's error code before any device
work, the refusals, null handles, the numpy closed form against brute-force refits on the small panels, and the
statistics of one stratum against jackknife_ref.finish_direct. No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_jack_ref as R  # noqa: E402
import jackknife_ref as J  # noqa: E402


def _code(N, fn):
    with pytest.raises(N.OaxacaError) as e:
        fn()
    return e.value.code, str(e.value)


def test_check_shape_codes(ob, N):
    ob.cluster_jackknife_check_shape(32, 2)
    ob.cluster_jackknife_check_shape(1, 2 ** 24 - 1, want_rows=True)
    assert N.OB_CLUSTER_JACK_MAX_K == 32
    assert _code(N, lambda: ob.cluster_jackknife_check_shape(33, 67))[0] == N.OB_E_UNSUPPORTED          # K = 33
    assert _code(N, lambda: ob.cluster_jackknife_check_shape(5, 67, n_norm=1))[0] == N.OB_E_UNSUPPORTED  # normalize
    assert _code(N, lambda: ob.cluster_jackknife_check_shape(5, 67, heckman=True))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.cluster_jackknife_check_shape(5, 67, n_y=2))[0] == N.OB_E_UNSUPPORTED    # two outcomes
    assert _code(N, lambda: ob.cluster_jackknife_check_shape(5, 2 ** 24))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.cluster_jackknife_check_shape(5, 1))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.cluster_jackknife_check_shape(5, 0))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.cluster_jackknife_check_shape(0, 67))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.cluster_jackknife_check_shape(5, -1))[0] == N.OB_E_INVALID


def _frame(n=60, clusters=6):
    rng = np.random.default_rng(1)
    g = np.where(np.arange(n) % 2 == 0, "A", "B")
    x = rng.normal(size=n)
    return {"y": (x + rng.normal(size=n)).tolist(), "g": g.tolist(), "x": x.tolist(),
            "firm": [f"f{(i // 2) % clusters}" for i in range(n)], "sector": rng.choice(["a", "b", "c"], n).tolist(),
            "s": (rng.random(n) < 0.7).astype(float).tolist(), "z": rng.normal(size=n).tolist()}


def test_refusals_and_null_handles(ob, N):
    lib = N.lib()
    f = _frame()
    base = lambda: ob.OaxacaBuilder(f, "y", "g", "B").predictors(["x"]).seed(1)
    # an unclustered builder has no delete-one-cluster pass
    for call in (base().run_cluster_bca, base().cluster_jackknife):
        assert _code(N, call)[0] == N.OB_E_INVALID
    # a clustered builder keeps refusing the delete-one-row forms
    b = base().cluster("firm")
    assert _code(N, b.run_bca)[0] == N.OB_E_UNSUPPORTED and _code(N, b.jackknife)[0] == N.OB_E_UNSUPPORTED

    # ob_builder_run_clustered_bca reaches its refusals before it touches the context: a handle that is no context
    # at all (zeroed bytes) comes back untouched
    fake = C.create_string_buffer(4096)
    ctx = C.cast(fake, C.c_void_p)

    def run(builder, level=0.95, cluster=True):
        cols, ncol, nrow = builder._frame.as_c()
        cfg, keep = builder._config()
        cc = builder._cluster_config() if cluster else None
        h = C.c_void_p()
        rc = lib.ob_builder_run_clustered_bca(ctx, cols, ncol, nrow, C.byref(cfg), C.byref(cc) if cluster else None,
                                              level, C.byref(h))
        assert not h.value and fake.raw == bytes(4096)
        return rc

    assert run(base().cluster("firm").heckman_selection("s", ["z"])) == N.OB_E_UNSUPPORTED
    assert run(base().categorical_predictors(["sector"]).normalize(["sector"]).cluster("firm")) == N.OB_E_UNSUPPORTED
    assert run(base().cluster("firm"), level=1.0) == N.OB_E_INVALID
    assert run(base().cluster("firm"), level=0.0) == N.OB_E_INVALID
    assert run(ob.OaxacaBuilder(_frame(clusters=1), "y", "g", "B").predictors(["x"]).cluster("firm")) == N.OB_E_INSUFFICIENT
    plain = base()
    plain._cluster = "firm"
    assert run(plain, cluster=False) == N.OB_E_INVALID  # no cluster config
    h = C.c_void_p()
    cols, ncol, nrow = plain._frame.as_c()
    cfg, keep = plain._config()
    cc = plain._cluster_config()
    assert lib.ob_builder_run_clustered_bca(None, cols, ncol, nrow, C.byref(cfg), C.byref(cc), 0.95, C.byref(h)) == N.OB_E_INVALID
    assert lib.ob_builder_run_clustered_bca(ctx, cols, ncol, nrow, C.byref(cfg), C.byref(cc), 0.95, None) == N.OB_E_INVALID

    # null handles
    o = N.ob_jackknife_out()
    d = (C.c_double * 8)()
    u8 = (C.c_uint8 * 8)()
    assert lib.ob_prepared_cluster_jackknife(None, C.byref(o)) == N.OB_E_INVALID
    assert lib.ob_prepared_cluster_jackknife(None, None) == N.OB_E_INVALID
    assert lib.ob_prepared_cluster_jackknife_rows(None, d, u8, None, None) == N.OB_E_INVALID
    # the array entry points: the shape checks come first, then the null pointers, all before the context is read
    u32 = (C.c_uint32 * 8)()
    assert lib.ob_cluster_jackknife(ctx, d, u32, 67, 67, 0, 32, 0, 100, 100, d, d, 0, C.byref(o)) == N.OB_E_UNSUPPORTED  # K = 33
    assert lib.ob_cluster_jackknife(ctx, d, u32, 1, 1, 0, 2, 0, 100, 100, d, d, 0, C.byref(o)) == N.OB_E_INSUFFICIENT
    assert lib.ob_cluster_jackknife(None, d, u32, 2, 2, 0, 2, 0, 100, 100, d, d, 0, C.byref(o)) == N.OB_E_INVALID
    assert lib.ob_cluster_jackknife(ctx, None, u32, 2, 2, 0, 2, 0, 100, 100, d, d, 0, C.byref(o)) == N.OB_E_INVALID
    assert lib.ob_cluster_jackknife(ctx, d, u32, 2, 2, 0, 2, 0, 100, 100, d, d, 9, C.byref(o)) == N.OB_E_INVALID  # beta* rule
    assert lib.ob_cluster_jackknife(ctx, d, u32, 2, 3, 1, 2, 0, 100, 100, d, d, 0, C.byref(o)) == N.OB_E_INVALID  # C_A > C
    assert lib.ob_cluster_jackknife(ctx, d, u32, 2, 2, 0, 2, 0, 100, 100, d, d, 0, C.byref(o)) == N.OB_E_INVALID  # no capacity
    assert lib.ob_cluster_jackknife_rows(None, d, u32, 2, 2, 0, 0, d, u8, None, None) == N.OB_E_INVALID
    assert lib.ob_prepared_finish_cluster_bca(None, d, u8, 1, 0.95, C.byref(h)) == N.OB_E_INVALID
    assert lib.ob_prepared_finish_cluster_bca(None, None, None, 0, 0.95, None) == N.OB_E_INVALID
    assert lib.ob_cluster_jackknife_last_timing(None) == N.OB_OK
    assert ob.cluster_jackknife_last_timing() >= 0.0
    assert fake.raw == bytes(4096)


SMALL = [c for c in R.CASES if c[0][2] == 2]  # the (37 + 53, 2, C) panels, C = 5 and 2


@pytest.mark.parametrize("ref", R.REF_RULES)
@pytest.mark.parametrize("shape,weighted,stratified", SMALL)
def test_closed_form_against_brute_force(O, shape, weighted, stratified, ref):
    refb = R.reference(O, R.case_frame(shape, weighted, stratified), shape[2], ref, weighted, stratified)
    bt, bk = R.brute(refb)
    cf, ck = R.closed_form(refb, ref)
    dv, dk, hat = R.closed_form(refb, ref, deviations=True, with_point=True)
    assert np.array_equal(bk, ck) and np.array_equal(bk, dk)
    if shape[3] == 2:
        assert not bk.all()  # rows <= K without the cluster
    if bk.any():
        gap = refb.b.point(refb.prep)[0][5]
        assert R.mixed_error(cf[bk], bt[bk], gap) <= R.E_MEASURED
        assert R.mixed_error(dv[bk] + hat[None, :], bt[bk], gap) <= R.E_MEASURED


def test_special_panels_on_the_restatement(O):
    for weighted in (False, True):
        refb = R.reference(O, R.dummy_frame(weighted), 2, 2, weighted, False, extra=("d",))
        _, bk = R.brute(refb)
        _, ck = R.closed_form(refb, 2)
        assert (~bk).tolist() == [lab == "f3" for lab in refb.labels] and np.array_equal(bk, ck)
    refb = R.reference(O, R.zero_weight_frame(), 2, 4, True, False)
    d, kept = R.closed_form(refb, 4, deviations=True)
    z = refb.labels.index("f4")
    assert kept.all() and (d[z] == 0.0).all() and all((d[c] != 0.0).any() for c in range(5) if c != z)


def test_finish_one_stratum_against_direct(ob, O):
    """ob_jackknife_finish with the sums as stratum 0 and kept = {m, 0} against the statistics taken from
    u_c = thetabar - theta_(c) directly."""
    shape = (37, 53, 2, 5)
    refb = R.reference(O, R.case_frame(shape, True, False), 2, 2, True, False)
    theta, kept, hat = R.closed_form(refb, 2, with_point=True)
    d, _ = R.closed_form(refb, 2, deviations=True)
    sums, used, dropped = R.power_sums(d, kept, R.n_strata_ranges(refb))
    assert used == [5, 0] and dropped == [0, 0] and (sums[1] == 0.0).all()
    got = ob.jackknife_finish(sums, used)
    # jackknife_ref.finish_direct's formulas over one stratum (its second slice would be empty here)
    u = theta[kept].mean(0)[None, :] - theta[kept]
    scale = np.maximum(np.abs(hat), abs(hat[5]))
    live = np.sqrt((u ** 2).sum(0)) > 1e-9 * scale  # explained:intercept is 0 in every fit: no acceleration to compare
    assert live.sum() == len(hat) - 1 and not live[6]
    with np.errstate(invalid="ignore", divide="ignore"):
        accel, se = (u ** 3).sum(0) / (6 * (u ** 2).sum(0) ** 1.5), np.sqrt(4 / 5 * (u ** 2).sum(0))
    assert np.allclose(got[:, 1], se, rtol=1e-9, atol=1e-12 * scale.max())
    assert np.allclose(got[live, 0], accel[live], rtol=1e-6, atol=1e-9)
    assert np.allclose(got[:, 2], 4 * d.mean(0), rtol=1e-12, atol=1e-15)


def test_shock_panel_conditions_hold_for_the_restatements(O):
    """The two conditions of test_gpu_cluster_jack.py's shock test, on the CPU restatements alone: the cluster
    jackknife SE of total_gap exceeds the delete-one-row jackknife SE and lies closer (in log ratio) to the cluster
    bootstrap SE than to the row bootstrap SE."""
    import cluster_ref as CR

    f = R.shock_frame()
    refb = CR.ClusterRef(O, f, "y", "g", "B", "firm", False, predictors=["x0"], reps=200, ref_mode=0, seed=R.SEED)
    st, used, dropped, _ = R.stats(refb, 0)
    cj = st[5, 1]
    p = refb.prep
    theta, kept = J.closed_form(0, p["xa"][:, 1:], p["ya"], None, p["xb"][:, 1:], p["yb"], None)
    _, se_row = J.finish_direct(theta, kept, len(p["ya"]))
    rj = se_row[5]
    rows, ok = refb.rows(0, 200)
    se_c = rows[ok.astype(bool), 5].std(ddof=1)
    brows, bok = O.boot_ref(p["cfg"], p["xa"], p["ya"], None, p["xb"], p["yb"], None, R.SEED, 0, 200, full=False)
    se_r = brows[bok.astype(bool), 5].std(ddof=1)
    print(f"cluster jack {cj:.5f}, row jack {rj:.5f}, cluster boot {se_c:.5f}, row boot {se_r:.5f}")
    assert used == [40, 0] and cj > rj
    assert abs(np.log(cj / se_c)) < abs(np.log(cj / se_r))
