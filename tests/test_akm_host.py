"""AKM without a GPU: the NumPy restatement (tests/akm_ref.py) against the reference's own unit cases
(tests/golden/akm_kat.json), ob_akm_connected_set against the restatement, and the two conditions that
tests/test_gpu_akm.py relies on, shown here on the restatement alone for every input it uses:

* the stopping margin: each loop's last diff is <= tol (1 - 1e-6) and the ones before >= tol (1 + 1e-6),
  so a device norm added in another order (relative change <= n 2^-53) stops at the same iteration;
* the f64 restatement is within 1/8 of each a-priori bar of its own longdouble run, so the bars
  (demean: 4 t (m + 2) 2^-53 sqrt(n) V in the 2-norm; recover_fe: 4 t (m + 3) 2^-53 V in the max-norm)
  leave the device 7/8 of their width."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import akm_ref as A  # noqa: E402

KAT = json.load(open(os.path.join(HERE, "golden", "akm_kat.json")))
TOL = 1e-8


def test_restatement_unit_cases():
    k = KAT["unit_demean"]
    v, it, diffs, _ = A.demean(k["vec"], k["worker_indices"], k["firm_indices"], k["n_workers"], k["n_firms"],
                               k["tolerance"], k["max_iters"])
    assert it == 0 and it >= k["max_iters"] and diffs == [] and v.tolist() == k["vec"]  # ConvergenceFailed
    k = KAT["unit_recover_fe"]
    a, p, it, diffs, _ = A.recover_fe(k["r"], k["worker_indices"], k["firm_indices"], k["n_workers"], k["n_firms"],
                                      k["tolerance"], k["max_iters"])
    assert it == 0 and it >= k["max_iters"] and not a.any() and not p.any()
    # with iterations allowed the 2 x 2 case is exact: worker means 2 and 3, then firm means -1 and 1
    v, it, diffs, _ = A.demean([1.0, 2.0, 3.0, 4.0], [0, 1, 0, 1], [0, 0, 1, 1], 2, 2, 1e-10, 1000)
    assert it == 2 and diffs == [np.sqrt(30.0), 0.0] and not v.any()  # the first change is the vector itself


def test_restatement_lcs_and_synthetic():
    k = KAT["lcs_filtering"]
    r = A.run(k["worker"], k["firm"], k["y"], [])
    assert sorted(r["worker_effects"]) == k["kept_workers"] and sorted(r["firm_effects"]) == ["f1"]
    assert r["set"]["keep"].tolist() == [True, True, False] and r["set"]["n_components"] == 2
    assert r["firm_effects"]["f1"] == 0.0
    s = KAT["synthetic"]
    rng = np.random.default_rng(3)
    w, f = rng.integers(0, s["n_workers"], s["n_obs"]), rng.integers(0, s["n_firms"], s["n_obs"])
    x = rng.uniform(0, 10, s["n_obs"])
    y = s["beta"] * x + rng.uniform(-1, 1, s["n_workers"])[w] + rng.uniform(-.5, .5, s["n_firms"])[f] \
        + rng.uniform(-0.01, 0.01, s["n_obs"])
    r = A.run([f"w{i}" for i in w], [f"f{i}" for i in f], y.tolist(), [x.tolist()], s["tolerance"], s["max_iters"])
    assert abs(r["beta"][0] - s["beta"]) < s["beta_abs_err_below"] and r["r2"] > s["r2_above"]
    with pytest.raises(A.AkmRefError) as e:
        A.run([f"w{i}" for i in w], [f"f{i}" for i in f], y.tolist(), [x.tolist()], s["tolerance"], 0)
    assert e.value.kind == "convergence" and KAT["unit_demean"]["error"] in str(e.value)


SETS = {
    "strings": (["w1", "w2", "w3", "w2", "w9"], ["f1", "f1", "f2", "f3", "f2"]),
    "i64": ([9, 10, 10, 2, 9, 33], [1, 1, 10, 10, 9, 7]),
    "nulls": (["a", None, "b", "b", "c", None], ["x", "x", None, "y", "y", None]),
    # {a, b, x} and {c, d, y}: three nodes each; the tie goes to the component of the smallest worker id
    "tie": (["c", "d", "a", "b"], ["y", "y", "x", "x"]),
    # {p, q} joined by five rows loses against {a, b, x} with two rows
    "rows_lose": (["p", "p", "p", "p", "p", "a", "b"], ["q", "q", "q", "q", "q", "x", "x"]),
}


@pytest.mark.parametrize("name", sorted(SETS))
def test_connected_set_matches_restatement(ob, name):
    w, f = SETS[name]
    got = ob.akm_connected_set({"w": w, "f": f, "y": [1.0] * len(w)}, "w", "f")
    ref = A.connected_set([None if v is None else str(v) for v in w], [None if v is None else str(v) for v in f])
    assert got["keep"].tolist() == ref["keep"].tolist()
    assert got["worker_idx"].tolist() == ref["worker_idx"].tolist()
    assert got["firm_idx"].tolist() == ref["firm_idx"].tolist()
    assert got["worker_ids"] == ref["worker_ids"] and got["firm_ids"] == ref["firm_ids"]
    assert got["n_components"] == ref["n_components"]
    if name == "i64":
        assert got["worker_ids"].index("10") < got["worker_ids"].index("9")  # decimal strings, not numbers
    if name == "tie":
        assert got["worker_ids"] == ["a", "b"] and got["keep"].tolist() == [False, False, True, True]
    if name == "rows_lose":
        assert got["worker_ids"] == ["a", "b"] and got["keep"].sum() == 2
    if name == "nulls":
        assert got["keep"].tolist() == [False, False, False, True, True, False]


def test_connected_set_errors(ob, N):
    with pytest.raises(N.OaxacaError) as e:
        ob.akm_connected_set({"w": [1.0, 2.0], "f": ["a", "b"]}, "w", "f")
    assert e.value.code == N.OB_E_UNSUPPORTED
    with pytest.raises(N.OaxacaError) as e:
        ob.akm_connected_set({"w": np.zeros(0, np.int64), "f": np.zeros(0, np.int64)}, "w", "f")
    assert e.value.code == N.OB_E_INSUFFICIENT and "No connected set found" in str(e.value)
    with pytest.raises(N.OaxacaError) as e:
        ob.akm_connected_set({"w": [None, "a"], "f": ["x", None]}, "w", "f")
    assert e.value.code == N.OB_E_INSUFFICIENT
    with pytest.raises(N.OaxacaError) as e:
        ob.akm_connected_set({"w": ["a"], "f": ["x"]}, "w", "nope")
    assert e.value.code == N.OB_E_COLUMN and "Column not found: nope" in str(e.value)


def test_option_and_limits(N):
    assert N.get_option("akm_poll") is None
    with N.option("akm_poll", 3):
        assert N.get_option("akm_poll") == 3
    assert N.OB_E_CONVERGENCE == 12 and N.OB_AKM_MAX_CONTROLS == 64


@pytest.mark.parametrize("name", A.CASES)
def test_gpu_inputs_satisfy_margin_and_bars(name):
    d = A.case(name)
    n, m = len(d["y"]), A.max_group(d)
    b = A.batch(d)
    worst = 0.0
    for c, (v, it, diffs, big) in enumerate(A.ref_demean(name, TOL)):
        assert it < 1000 and A.margin_ok(diffs, TOL), (name, c, it, diffs[-2:])
        if c < 6:  # the longdouble run of every column of the 65-column case would only repeat this
            hv = A.demean(b[:, c], d["widx"], d["fidx"], d["nw"], d["nf"], hi=True, stop_at=it)[0]
            err = float(np.sqrt(np.sum((v.astype(np.longdouble) - hv) ** 2)))
            bar = A.demean_bar(it, m, n, big)
            worst = max(worst, err / bar if bar else 0.0)
            assert err <= bar / 8, (name, c, err, bar)
    a, p, it, diffs, big = A.ref_recover(name, TOL)
    assert it < 1000 and A.margin_ok(diffs, TOL), (name, it, diffs[-2:])
    ha, hp = A.recover_fe(A.residual(d), d["widx"], d["fidx"], d["nw"], d["nf"], hi=True, stop_at=it)[:2]
    err = float(max(np.max(np.abs(a - ha)), np.max(np.abs(p - hp))))
    bar = A.recover_bar(it, m, big)
    print(f"{name}: demean f64 vs longdouble worst {worst:.3g} of the bar; recover_fe {err / bar:.3g} (t = {it})")
    assert err <= bar / 8, (name, err, bar)


def test_batch_case_columns_stop_at_different_iterations():
    its = [r[1] for r in A.ref_demean("p1000", TOL)]
    assert its[0] != its[1], its
