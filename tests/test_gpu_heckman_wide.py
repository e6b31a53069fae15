"""Heckman selection equations of 9 to 32 columns (ks = 1 + selection predictors > 8): the f64 MFMA
probit and IMR-sums kernels of csrc/ob_heckman.hip against the oracle's restatement of math/probit.rs,
heckman.rs and estimation.rs:114-260 -- replicate rows at the first wide width, a full 16-column tile,
one column past a tile and the maximum; both count-image layouts and the library erfc; bitwise shard
invariance; the results tables; a probit that never converges; the limits; and the probit() piece."""
import numpy as np
import pytest

from test_gpu_parity import RTOL, SEED, close, compare_results

pytestmark = pytest.mark.gpu


def wide_arrays(n, nz, weighted=False):
    """The frame's columns as arrays; the generator's seed is n."""
    rng = np.random.default_rng(n)
    Z = rng.normal(size=(n, nz))
    x = Z[:, 0] + 0.5 * rng.normal(size=n)
    x2 = rng.uniform(0.0, 3.0, n)
    u, e0 = rng.normal(size=n), rng.normal(size=n)
    e = 0.8 * u + 0.6 * e0
    grp = np.where(rng.random(n) < 0.5, "A", "B")
    coef = 0.5 * (-0.8) ** np.arange(nz) / np.sqrt(1.0 + np.arange(nz))
    s = (0.3 + Z @ coef + 0.2 * x2 + 0.3 * (grp == "A") + u > 0).astype(float)
    y = 1.0 + 2.0 * x + 0.5 * x2 + 0.4 * (grp == "A") + e
    w = rng.uniform(0.5, 2.0, n) if weighted else None  # drawn last
    return Z, x, x2, grp, s, y, w


def wide_frame(n, nz, weighted=False, null_unselected=False):
    Z, x, x2, grp, s, y, w = wide_arrays(n, nz, weighted)
    out = [None if (null_unselected and si != 1.0) else float(v) for v, si in zip(y, s)]
    f = {"outcome": out, "x": x.tolist(), "x2": x2.tolist(), "selection": s.tolist(), "group": grp.tolist()}
    for j in range(nz):
        f[f"z{j}"] = Z[:, j].tolist()
    if weighted:
        f["w"] = w.tolist()
    return f


PREDS = ["x", "x2"]


def zcols(lo_hi, extra=()):
    return [f"z{j}" for j in range(*lo_hi)] + list(extra)


def builders(ob, O, f, zs, reps, ref, weighted):
    b = (ob.OaxacaBuilder(f, "outcome", "group", "B").predictors(PREDS).heckman_selection("selection", zs)
         .bootstrap_reps(reps).reference_coefficients(ref).seed(SEED))
    o = O.OracleBuilder(f, "outcome", "group", "B").set(PREDS, reps=reps, ref_mode=ref, seed=SEED,
                                                         weights="w" if weighted else None)
    if weighted:
        b = b.weights("w")
    return b, o.heckman("selection", zs)


CASES = [  # (rows, z columns in the frame, selection predictors, ref, weighted) -> ks = 9, 16, 17, 32
    (1500, 8, zcols((0, 7), ["x2"]), 0, False),
    (2500, 15, zcols((0, 14), ["x2"]), 1, True),
    (2000, 16, zcols((0, 15), ["x2"]), 3, False),
    (4000, 31, zcols((0, 31)), 4, True),
]
KS17 = CASES[2]

_oracle_rows = {}


def oracle_rows(O, case):
    """The oracle's 48 replicate rows of a case, computed once and shared (read-only)."""
    n, nz, zs, ref, weighted = case
    if n not in _oracle_rows:
        f = wide_frame(n, nz, weighted)
        o = O.OracleBuilder(f, "outcome", "group", "B").set(PREDS, reps=48, ref_mode=ref, seed=SEED,
                                                             weights="w" if weighted else None).heckman("selection", zs)
        want = o.run()
        want["rows"].setflags(write=False)
        _oracle_rows[n] = (f, want)
    return _oracle_rows[n]


def check_rows(ob, O, case):
    n, nz, zs, ref, weighted = case
    f, want = oracle_rows(O, case)
    b, _ = builders(ob, O, f, zs, 48, ref, weighted)
    pr = b.prepare()
    try:
        rows, ok = pr.boot(0, 48)
    finally:
        pr.close()
    assert rows.shape == want["rows"].shape == (48, O.heckman_row_len(len(PREDS) + 1, len(zs) + 1))
    assert want["ok"].astype(bool).all() and ok.astype(bool).all()
    good, worst = close(rows, want["rows"], want["total_gap"])
    assert good, worst


@pytest.mark.parametrize("case", CASES, ids=["ks9", "ks16", "ks17", "ks32"])
def test_wide_rows_match_oracle(ob, O, case):
    check_rows(ob, O, case)


def test_wide_rows_f64_gram_count_images(ob, O, N):
    """gram_path = 1: the f64 Gram's [replicate][row] count words instead of the i8 A fragments."""
    with N.option("gram_path", 1):
        check_rows(ob, O, KS17)


def test_wide_rows_library_erfc(ob, O, N):
    with N.option("hk_erfc", 0):
        check_rows(ob, O, KS17)


def test_wide_shard_invariant_and_deterministic(ob, N):
    """Bitwise: a replicate's row does not depend on its slot, its neighbours or the boot's size
    (200, 128, 72 and 1 are multiples of neither 64 nor 16)."""
    n, nz, zs = 5000, 16, KS17[2]
    b = (ob.OaxacaBuilder(wide_frame(n, nz), "outcome", "group", "B").predictors(PREDS)
         .heckman_selection("selection", zs).bootstrap_reps(200).seed(SEED))
    pr = b.prepare()
    try:
        r0, k0 = pr.boot(0, 200)
        r1, k1 = pr.boot(72, 128)
        r2, k2 = pr.boot(0, 200)
        r3, k3 = pr.boot(199, 1)
    finally:
        pr.close()
    assert r0.tobytes() == r2.tobytes() and np.array_equal(k0, k2)
    assert r0[72:200].tobytes() == r1.tobytes() and np.array_equal(k0[72:200], k1)
    assert r0[199:200].tobytes() == r3.tobytes() and np.array_equal(k0[199:200], k3)
    assert k0.astype(bool).any()
    # the engine runs a wide segment in replicate batches when its chunk partials would outgrow their
    # budget (16,384-replicate segments of a large panel): forced here to 64 and 128 replicates a batch
    for blocks in (1, 2):
        with N.option("hk_batch", blocks):
            pr = b.prepare()
            try:
                rb, kb = pr.boot(0, 200)
            finally:
                pr.close()
        assert r0.tobytes() == rb.tobytes() and np.array_equal(k0, kb), blocks


def test_wide_results_match_oracle(ob, O):
    n, nz, zs, ref, weighted = KS17
    f = wide_frame(n, nz, weighted)
    b, o = builders(ob, O, f, zs, 100, ref, weighted)
    r, want = b.run(), o.run()
    compare_results(r, want)
    names = [c.name for c in r.two_fold.detailed_explained]
    assert names[-1] == "IMR" and names == [c["name"] for c in want["two_fold"]["detailed_explained"]]
    got, exp = r.two_fold.detailed_selection, want["two_fold"]["detailed_selection"]
    assert [c.name for c in got] == ["__ob_intercept__"] + zs == [c["name"] for c in exp]
    scale = abs(want["total_gap"])
    for c, w in zip(got, exp):
        for fld in ("estimate", "std_err", "ci_lower", "ci_upper"):
            assert abs(getattr(c, fld) - w[fld]) <= RTOL * max(abs(w[fld]), scale), (c.name, fld)
    assert len(r.residuals) == len(want["residuals"]) and not np.any(r.residuals)


def test_wide_probit_that_never_converges(ob, O):
    """Outcome null where s != 1: every kept row has s = 1, the probit runs its 100 iterations."""
    zs = zcols((0, 7), ["x2"])
    f = wide_frame(2000, 8, null_unselected=True)
    r = (ob.OaxacaBuilder(f, "outcome", "group", "B").predictors(PREDS).heckman_selection("selection", zs)
         .bootstrap_reps(0).run())
    assert any(c.name == "IMR" for c in r.two_fold.detailed_explained)
    o = O.OracleBuilder(f, "outcome", "group", "B").set(PREDS, reps=0).heckman("selection", zs).run()
    assert r.n_a == o["n_a"] and r.n_b == o["n_b"] and len(r.residuals) == len(o["residuals"]) == r.n_b
    assert abs(r.total_gap - o["total_gap"]) <= 1e-9 * max(1.0, abs(o["total_gap"]))


def test_wide_limits(ob, N):
    assert N.OB_HECKMAN_MAX_ZSEL == 31
    f = wide_frame(3000, 32)
    r = (ob.OaxacaBuilder(f, "outcome", "group", "B").predictors(PREDS)
         .heckman_selection("selection", zcols((0, 31))).bootstrap_reps(0).run())
    assert len(r.two_fold.detailed_selection) == 32
    with pytest.raises(N.OaxacaError) as e:
        (ob.OaxacaBuilder(f, "outcome", "group", "B").predictors(PREDS)
         .heckman_selection("selection", zcols((0, 32))).bootstrap_reps(0).run())
    assert e.value.code == N.OB_E_UNSUPPORTED and "31" in str(e.value)


# (n, k): narrow (k <= 8) and wide kernels, one row short of a sub-tile, one past a tile, the maximum.
# oracle.probit converges on each in fewer than 100 iterations (6, 6, 7, 9 and 7; run on the CPU),
# so neither (63, 3) nor (257, 12) separates and no shape had to move.
PROBIT_SHAPES = [(63, 3), (1000, 8), (1000, 9), (257, 12), (3001, 32)]
# the edges of the wide pass kernel: a one-row last sub-tile at the first wide width,
# a one-row second tile where a wave owns two pair tiles (66 pairs), and 496 pairs without a padding lane; 10, 7 and
# 7 iterations of oracle.probit (run on the CPU)
PROBIT_SHAPES += [(65, 9), (257, 11), (2049, 31)]


def probit_xy(n, k):
    Z, _, _, _, s, _, _ = wide_arrays(n, k - 1)
    return np.column_stack([np.ones(n), Z]), s


@pytest.mark.parametrize("n,k", PROBIT_SHAPES)
def test_probit_piece_matches_oracle(ob, O, n, k):
    x, y = probit_xy(n, k)
    want = O.probit(y, x, full=True)
    assert want["converged"] and want["iterations"] < 100
    beta, conv, iters = ob.probit(x, y)
    assert conv == want["converged"] and iters == want["iterations"]
    assert np.all(np.abs(beta - want["coefficients"]) <= RTOL * np.maximum(np.abs(want["coefficients"]), 1.0))


def test_probit_piece_refuses_33_columns(ob, N):
    x, y = probit_xy(200, 33)
    with pytest.raises(N.OaxacaError) as e:
        ob.probit(x, y)
    assert e.value.code == N.OB_E_UNSUPPORTED
