"""AKM on the GPU: ob_akm_demean, ob_akm_recover_fe and ob_akm_run / AkmBuilder against the NumPy
restatement (tests/akm_ref.py) and the reference's own tests (tests/golden/akm_kat.json).

Two conditions hold on the restatement alone for every input used here (tests/test_akm_host.py asserts
them without a GPU, and each test here re-checks the first before it compares): the stopping margin
(the last diff <= tol (1 - 1e-6), the earlier ones >= tol (1 + 1e-6)), so iteration counts must be
EQUAL, and the f64 restatement within 1/8 of each bar of its longdouble run.

Bars (first-order a-priori rounding bounds, valid for any summation order), with t the iteration
count, m the largest group, V the largest magnitude that entered a sum:
  demean      ||dev - ref||_2  <= 4 t (m + 2) 2^-53 sqrt(n) V   per column
  recover_fe  max|dev - ref|   <= 4 t (m + 3) 2^-53 V           over (alpha, psi)
  end to end  beta, effects, r2: 1e-6 of the largest magnitude (the bar of smoke() and matching's beta)
Batch, poll and repeat independence are bitwise. Each test prints its worst fraction of the bar
before it asserts.

The worst fractions measured on an MI355X are in DESIGN.md §5.6."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import akm_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu

KAT = json.load(open(os.path.join(HERE, "golden", "akm_kat.json")))
TOL = 1e-8


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_demean(ob, name, cols=None):
    d = A.case(name)
    b = A.batch(d) if cols is None else A.batch(d)[:, cols]
    refs = A.ref_demean(name, TOL)
    refs = refs if cols is None else [refs[c] for c in cols]
    assert all(A.margin_ok(r[2], TOL) for r in refs)
    out, iters, conv = ob.akm_demean(b, d["widx"], d["fidx"], d["nw"], d["nf"], TOL, 1000)
    n, m = len(d["y"]), A.max_group(d)
    worst = 0.0
    for c, (v, it, _, big) in enumerate(refs):
        err, bar = float(np.linalg.norm(out[:, c] - v)), A.demean_bar(it, m, n, big)
        worst = max(worst, err / bar)
    print(f"demean {name} {b.shape}: iterations {iters.tolist()[:6]} worst fraction of the bar {worst:.3g}")
    assert iters.tolist() == [r[1] for r in refs] and conv.all()
    assert worst <= 1.0
    return out, iters


@pytest.mark.parametrize("name", A.CASES)
def test_demean_against_restatement(ob, name):
    out, _ = _check_demean(ob, name)
    if name == "singletons":
        assert not out.any()  # every worker has one row: exactly 0 after the first half-step
    if name == "four":
        assert not out[:, 0].any()


@pytest.mark.parametrize("cols", [[0], [0, 1], [0, 1, 2, 3, 4, 5], list(range(65))], ids=["c1", "c2", "c6", "c65"])
def test_demean_column_counts(ob, cols):
    _check_demean(ob, "wide65", cols)


def test_demean_leading_dimension_and_padding(ob):
    d = A.case("p1000")
    b = A.batch(d)
    n, c = b.shape
    pad = np.full((c, n + 7), np.nan)
    pad[:, :n] = b.T
    out, iters, _ = ob.akm_demean(pad.T[:n], d["widx"], d["fidx"], d["nw"], d["nf"], TOL, 1000)
    ref, riters, _ = ob.akm_demean(b, d["widx"], d["fidx"], d["nw"], d["nf"], TOL, 1000)
    # a NaN read from the padding would have spread into its column's sums
    assert out.strides[1] == 8 * (n + 7) and np.array_equal(_bits(out), _bits(ref)) and iters.tolist() == riters.tolist()


def test_batch_poll_and_repeat_independence(ob, N):
    d = A.case("p1000")
    b = A.batch(d)
    refs = A.ref_demean("p1000", TOL)
    assert refs[0][1] != refs[1][1]  # the outcome and the control stop at different iterations
    args = (d["widx"], d["fidx"], d["nw"], d["nf"], TOL, 1000)
    both, it_both, _ = ob.akm_demean(b, *args)
    again, it_again, _ = ob.akm_demean(b, *args)
    assert np.array_equal(_bits(both), _bits(again)) and it_both.tolist() == it_again.tolist()
    for c in range(2):
        alone, it_alone, _ = ob.akm_demean(b[:, c], *args)
        assert np.array_equal(_bits(alone), _bits(both[:, c])) and it_alone[0] == it_both[c]
    swapped, it_sw, _ = ob.akm_demean(b[:, ::-1], *args)
    assert np.array_equal(_bits(swapped[:, ::-1]), _bits(both)) and it_sw.tolist() == it_both.tolist()[::-1]
    wide = A.batch(A.case("wide65"))
    w_out, w_it, _ = ob.akm_demean(wide, *args)
    assert np.array_equal(_bits(w_out[:, :2]), _bits(both)) and w_it[:2].tolist() == it_both.tolist()
    r = A.residual(d)
    fe = ob.akm_recover_fe(r, *args)
    for poll in (1, 3):
        with N.option("akm_poll", poll):
            p_out, p_it, _ = ob.akm_demean(b, *args)
            p_fe = ob.akm_recover_fe(r, *args)
        assert np.array_equal(_bits(p_out), _bits(both)) and p_it.tolist() == it_both.tolist()
        assert np.array_equal(_bits(p_fe[0]), _bits(fe[0])) and np.array_equal(_bits(p_fe[1]), _bits(fe[1]))
        assert p_fe[2] == fe[2]


def test_demean_max_iters_is_reported_not_raised(ob):
    d = A.case("p1000")
    b = A.batch(d)
    its = [r[1] for r in A.ref_demean("p1000", TOL)]
    args = (d["widx"], d["fidx"], d["nw"], d["nf"], TOL)
    full, _, _ = ob.akm_demean(b, *args, 1000)
    out, iters, conv = ob.akm_demean(b, *args, max(its))
    assert iters.tolist() == its and conv.tolist() == [it < max(its) for it in its]  # akm.rs:519
    assert np.array_equal(_bits(out), _bits(full))
    out, iters, conv = ob.akm_demean(b, *args, 0)
    assert iters.tolist() == [0, 0] and not conv.any() and np.array_equal(_bits(out), _bits(b))
    k = KAT["unit_demean"]
    out, iters, conv = ob.akm_demean(np.array(k["vec"]), k["worker_indices"], k["firm_indices"], k["n_workers"],
                                     k["n_firms"], k["tolerance"], k["max_iters"])
    assert iters[0] == 0 and not conv[0] and out.tolist() == k["vec"]


@pytest.mark.parametrize("name", A.CASES)
def test_recover_fe_against_restatement(ob, name):
    d = A.case(name)
    a, p, it, diffs, big = A.ref_recover(name, TOL)
    assert A.margin_ok(diffs, TOL)
    ga, gp, git, conv = ob.akm_recover_fe(A.residual(d), d["widx"], d["fidx"], d["nw"], d["nf"], TOL, 1000)
    err, bar = float(max(np.max(np.abs(ga - a)), np.max(np.abs(gp - p)))), A.recover_bar(it, A.max_group(d), big)
    print(f"recover_fe {name}: iterations {git} (restatement {it}), fraction of the bar {err / bar if bar else 0:.3g}")
    assert git == it and conv and gp[0] == 0.0 and not np.signbit(gp[0])
    assert err <= bar
    k = KAT["unit_recover_fe"]
    ga, gp, git, conv = ob.akm_recover_fe(np.array(k["r"]), k["worker_indices"], k["firm_indices"], k["n_workers"],
                                          k["n_firms"], k["tolerance"], k["max_iters"])
    assert git == 0 and not conv and not ga.any() and not gp.any()


def _frame(d, n_controls=None, ids="str"):
    k = d["x"].shape[1] if n_controls is None else n_controls
    w = [f"w{i}" for i in d["widx"]] if ids == "str" else d["widx"].astype(np.int64)
    f = [f"f{i}" for i in d["fidx"]] if ids == "str" else d["fidx"].astype(np.int64)
    fr = {"worker": w, "firm": f, "y": d["y"].copy()}
    for j in range(k):
        fr[f"x{j}"] = d["x"][:, j].copy()
    return fr, [f"x{j}" for j in range(k)]


def _ref_run(fr, controls, tol=TOL, max_iters=1000):
    def col(c):
        if isinstance(c, np.ma.MaskedArray):
            return [None if m else float(v) for v, m in zip(c.data, np.ma.getmaskarray(c))]
        return [None if v is None else v for v in (c.tolist() if isinstance(c, np.ndarray) else c)]

    return A.run([None if v is None else str(v) for v in col(fr["worker"])],
                 [None if v is None else str(v) for v in col(fr["firm"])], col(fr["y"]),
                 [col(fr[c]) for c in controls], tol, max_iters)


def _assert_run(got, ref, label):
    scale = max(1.0, float(np.max(np.abs(ref["beta"]))) if len(ref["beta"]) else 0.0,
                max(abs(v) for v in ref["worker_effects"].values()), max(abs(v) for v in ref["firm_effects"].values()))
    assert list(got.worker_effects) == list(ref["worker_effects"]) and list(got.firm_effects) == list(ref["firm_effects"])
    err = max([abs(g - r) for g, r in zip(got.beta, ref["beta"])] +
              [abs(got.worker_effects[k] - v) for k, v in ref["worker_effects"].items()] +
              [abs(got.firm_effects[k] - v) for k, v in ref["firm_effects"].items()] + [abs(got.r2 - ref["r2"])])
    print(f"run {label}: worst error {err / scale:.3g} of the scale (bar 1e-6); demean iterations "
          f"{got.info['demean_iterations']} recover {got.info['recover_iterations']}")
    assert err <= 1e-6 * scale
    assert got.info["demean_iterations"] == ref["demean_iterations"]
    assert got.info["recover_iterations"] == ref["recover_iterations"]


def test_run_synthetic_with_the_reference_bars(ob):
    s = KAT["synthetic"]
    fr, controls = _frame(A.case("p1000"))
    got = ob.AkmBuilder(fr, "y", "worker", "firm").controls(controls).tolerance(s["tolerance"]) \
        .max_iters(s["max_iters"]).run()
    assert abs(got.beta[0] - s["beta"]) < s["beta_abs_err_below"] and got.r2 > s["r2_above"]
    _assert_run(got, _ref_run(fr, controls, s["tolerance"], s["max_iters"]), "synthetic")
    assert got.info["n_components"] == 1 and got.info["launches_per_iteration"] <= 3


def test_run_lcs_kat_no_controls_five_controls_and_null_control(ob):
    k = KAT["lcs_filtering"]
    fr = {"worker": k["worker"], "firm": k["firm"], "y": k["y"]}
    got = ob.AkmBuilder(fr, "y", "worker", "firm").run()
    assert sorted(got.worker_effects) == k["kept_workers"] and "f2" not in got.firm_effects and got.beta == []
    assert got.info["n_rows_kept"] == 2 and got.info["n_components"] == 2
    _assert_run(got, _ref_run(fr, []), "lcs")
    fr, controls = _frame(A.case("p5000"))
    _assert_run(ob.AkmBuilder(fr, "y", "worker", "firm").run(), _ref_run(fr, []), "no controls")
    _assert_run(ob.AkmBuilder(fr, "y", "worker", "firm").controls(controls).run(), _ref_run(fr, controls), "5 controls")
    fr, controls = _frame(A.case("p1000"))
    mask = np.zeros(len(fr["y"]), dtype=bool)
    mask[::17] = True
    fr["x0"] = np.ma.MaskedArray(fr["x0"], mask=mask)
    _assert_run(ob.AkmBuilder(fr, "y", "worker", "firm").controls(controls).run(), _ref_run(fr, controls), "null control")


def test_run_second_component_is_dropped(ob):
    fr, controls = _frame(A.case("p1000"))
    fr["worker"] = fr["worker"] + ["wz1", "wz2", "wz1"]
    fr["firm"] = fr["firm"] + ["fz", "fz", "fz"]
    fr["y"] = np.concatenate([fr["y"], [5.0, 6.0, 7.0]])
    fr["x0"] = np.concatenate([fr["x0"], [1.0, 2.0, 3.0]])
    got = ob.AkmBuilder(fr, "y", "worker", "firm").controls(controls).run()
    assert "wz1" not in got.worker_effects and "fz" not in got.firm_effects and got.info["n_components"] == 2
    _assert_run(got, _ref_run(fr, controls), "two components")


def test_run_max_iters_quirk(ob, N):
    fr, controls = _frame(A.case("p1000"))
    ref = _ref_run(fr, controls)
    count = max(ref["demean_iterations"] + [ref["recover_iterations"]])
    with pytest.raises(N.OaxacaError) as e:
        ob.AkmBuilder(fr, "y", "worker", "firm").controls(controls).max_iters(count).run()
    assert e.value.code == N.OB_E_CONVERGENCE and f"failed to converge within {count} iterations" in str(e.value)
    _assert_run(ob.AkmBuilder(fr, "y", "worker", "firm").controls(controls).max_iters(count + 1).run(), ref, "count + 1")
    with pytest.raises(N.OaxacaError) as e:
        ob.AkmBuilder(fr, "y", "worker", "firm").controls(controls).max_iters(0).run()
    assert e.value.code == N.OB_E_CONVERGENCE
    assert "Convergence failed: demean_vector failed to converge within 0 iterations. Try increasing" in str(e.value)


def test_run_errors(ob, N):
    fr, controls = _frame(A.case("p1000"))

    def fails(frame, code, text, ctl=controls, outcome="y"):
        with pytest.raises(N.OaxacaError) as e:
            ob.AkmBuilder(frame, outcome, "worker", "firm").controls(ctl).run()
        assert e.value.code == code and text in str(e.value), (e.value.code, str(e.value))

    y = np.ma.MaskedArray(fr["y"], mask=np.arange(len(fr["y"])) == 3)
    fails(dict(fr, y=y), N.OB_E_INSUFFICIENT, "Null outcome encountered")
    fails(dict(fr, x0=np.arange(len(fr["y"]), dtype=np.int64)), N.OB_E_POLARS, "expected `Float64`")
    fails(fr, N.OB_E_COLUMN, "Column not found: nope", ctl=["nope"])
    fails(fr, N.OB_E_COLUMN, "Column not found: nope", outcome="nope")
    wide = dict(fr)
    for j in range(65):
        wide[f"c{j}"] = np.full(len(fr["y"]), float(j))
    fails(wide, N.OB_E_UNSUPPORTED, "at most 64", ctl=[f"c{j}" for j in range(65)])
    # a constant control is collinear with the worker effects: its demeaned column is exactly 0
    fails(dict(fr, x1=np.full(len(fr["y"]), 3.0)), N.OB_E_CONVERGENCE, "OLS design matrix is singular", ctl=["x0", "x1"])


def test_estimate_akm_from_csv_with_integer_ids(ob, tmp_path):
    d = A.case("p1000")
    fr, controls = _frame(d, ids="int")
    path = tmp_path / "akm.csv"
    with open(path, "w") as fh:
        fh.write("worker,firm,y,x0\n")
        for w, f, y, x in zip(fr["worker"], fr["firm"], fr["y"], fr["x0"]):
            fh.write(f"{w},{f},{float(y)!r},{float(x)!r}\n")
    got = ob.estimate_akm(str(path), "y", "worker", "firm", controls=["x0"])
    ref = _ref_run(fr, controls)
    _assert_run(got, ref, "csv")
    ids = list(got.worker_effects)
    assert ids.index("10") < ids.index("9")  # integer ids sort as decimal strings
