"""Hot-path binding: the two groups' design resident in HBM (``ob_panel``) and the bootstrap
replicate kernel sequence (``ob_boot_run``). This is the layer a Rust ``run()`` would call in
place of builder.rs:808-847; ``api.OaxacaBuilder`` drives it for frame inputs.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from .api import ReferenceCoefficients, tobit_finish_rows  # noqa: F401 (tobit_finish_rows is served from here too)


def row_layout(k: int, n_base: int = 0) -> dict:
    """Offsets of the per-replicate row (include/oaxaca_boot.h OB_ROW_*)."""
    kd = k + n_base
    t = 6 + 2 * kd
    return {"explained": 0, "unexplained": 1, "endowments": 2, "coefficients": 3, "interaction": 4,
            "total_gap": 5, "detailed_explained": slice(6, 6 + kd), "detailed_unexplained": slice(6 + kd, 6 + 2 * kd),
            "beta_a": slice(t, t + k), "beta_b": slice(t + k, t + 2 * k), "xa_mean": slice(t + 2 * k, t + 3 * k),
            "xb_mean": slice(t + 3 * k, t + 4 * k), "beta_star": slice(t + 4 * k, t + 5 * k),
            "len": t + 5 * k}


class Panel:
    """Two-group design (predictors only; intercept implicit) copied into HBM.

    ``xa``/``xb``: (n_g, p) arrays; ``n_num`` numeric predictors precede dummy columns (the
    pooled group indicator is inserted after them); ``norm`` optionally carries the
    normalization lists (dict with start, idx, m, pstart, pidx, has_base). ``ya``/``yb`` may be
    (n_g, n_y) blocks of several outcomes (RIF multi-tau): every replicate then yields n_y rows
    from one Gram pass, and ``point_estimate``/``boot`` return an outcome axis first.
    """

    def __init__(self, xa, ya, xb, yb, wa=None, wb=None, n_num=None, norm=None, device=None, ctx=None):
        xa = np.asarray(xa, dtype=np.float64)
        xb = np.asarray(xb, dtype=np.float64)
        if xa.ndim != 2 or xb.ndim != 2 or xa.shape[1] != xb.shape[1]:
            raise ValueError("xa/xb must be 2-D with the same number of columns")
        self.p = xa.shape[1]
        self._xa = np.asfortranarray(xa)
        self._xb = np.asfortranarray(xb)
        ya = np.asarray(ya, dtype=np.float64)
        yb = np.asarray(yb, dtype=np.float64)
        self.n_y = 1 if ya.ndim == 1 else ya.shape[1]
        if (yb.ndim == 1 and self.n_y != 1) or (yb.ndim == 2 and yb.shape[1] != self.n_y):
            raise ValueError("ya/yb must carry the same number of outcomes")
        self._ya = np.asfortranarray(ya.reshape(ya.shape[0], self.n_y))  # ld = n_g, as x
        self._yb = np.asfortranarray(yb.reshape(yb.shape[0], self.n_y))
        if len(self._ya) != xa.shape[0] or len(self._yb) != xb.shape[0]:
            raise ValueError("y length mismatch")
        weighted = wa is not None
        if weighted != (wb is not None):
            raise ValueError("weights must be given for both groups or neither")
        self._wa = None if wa is None else np.ascontiguousarray(wa, dtype=np.float64)
        self._wb = None if wb is None else np.ascontiguousarray(wb, dtype=np.float64)
        d = N.ob_panel_desc()
        d.p = self.p
        d.n_num = self.p if n_num is None else int(n_num)
        d.weighted = 1 if weighted else 0
        d.n_y = self.n_y
        d.a = N.ob_group_desc(xa.shape[0], N.dp(self._xa), max(xa.shape[0], 1), N.dp(self._ya), N.dp(self._wa))
        d.b = N.ob_group_desc(xb.shape[0], N.dp(self._xb), max(xb.shape[0], 1), N.dp(self._yb), N.dp(self._wb))
        self._norm_keep = []
        if norm:
            arrs = [np.ascontiguousarray(norm[k], dtype=np.int32)
                    for k in ("start", "idx", "m", "pstart", "pidx", "has_base")]
            self._norm_keep = arrs
            d.n_norm = len(arrs[2])
            (d.norm_start, d.norm_idx, d.norm_m, d.pooled_start, d.pooled_idx, d.has_base) = [N.i32p(a) for a in arrs]
        self._h = C.c_void_p()
        self._ctx = ctx if ctx is not None else N.context(device)
        N.check(N.lib().ob_panel_create(self._ctx, C.byref(d), C.byref(self._h)))
        self.k = N.lib().ob_panel_k(self._h)
        self.n_base = N.lib().ob_panel_n_base(self._h)
        self.row_len = N.lib().ob_panel_row_len(self._h)
        self.layout = row_layout(self.k, self.n_base)
        self.n_a, self.n_b = xa.shape[0], xb.shape[0]

    def point_estimate(self, ref=ReferenceCoefficients.GroupA, residuals=False):
        row = np.empty((self.n_y, self.row_len))
        res = np.empty((self.n_y, self.n_b)) if residuals else None
        N.check(N.lib().ob_point_estimate(self._h, int(ref), N.dp(row), N.dp(res)))
        if self.n_y == 1:
            row = row[0]
            res = None if res is None else res[0]
        return (row, res) if residuals else row

    def jackknife(self, ref=ReferenceCoefficients.GroupA):
        """ob_jackknife: the leave-one-out pass's power sums and statistics (api.JackknifeResult)."""
        from .api import _jackknife_out, _jackknife_result

        o, bufs = _jackknife_out(self.k)
        N.check(N.lib().ob_jackknife(self._h, int(ref), C.byref(o)))
        return _jackknife_result(o, bufs, None)

    def jackknife_rows(self, ref=ReferenceCoefficients.GroupA):
        """ob_jackknife_rows -> (theta (n_a + n_b, 6 + 2K), kept, n_dropped (A, B))."""
        c = 6 + 2 * self.k
        theta = np.empty((self.n_a + self.n_b, c))
        kept = np.zeros(self.n_a + self.n_b, dtype=np.uint8)
        nd = (C.c_int64 * 2)()
        N.check(N.lib().ob_jackknife_rows(self._h, int(ref), N.dp(theta), N.u8p(kept), nd))
        return theta, kept, (int(nd[0]), int(nd[1]))

    def boot(self, seed: int, first_rep: int, n_reps: int, ref=ReferenceCoefficients.GroupA):
        rows = np.empty((self.n_y, n_reps, self.row_len))
        ok = np.zeros((self.n_y, n_reps), dtype=np.uint8)
        if n_reps:
            N.check(N.lib().ob_boot_run(self._h, seed & ((1 << 64) - 1), first_rep, n_reps, int(ref), N.dp(rows),
                                        N.u8p(ok)))
        return (rows[0], ok[0]) if self.n_y == 1 else (rows, ok)

    def mm(self, seed: int, simulations: int, quantiles, first_rep: int = 0, n_reps: int = 0, with_point=True):
        """Machado-Mata passes (ob_mm_run): rows [gap, characteristics, coefficients] per quantile,
        the point pass first when ``with_point``; ok = 0 where a pass failed."""
        q = np.ascontiguousarray(quantiles, dtype=np.float64)
        m = int(bool(with_point)) + n_reps
        rows = np.empty((m, 3 * q.size))
        ok = np.zeros(m, dtype=np.uint8)
        N.check(N.lib().ob_mm_run(self._h, seed & ((1 << 64) - 1), int(simulations), N.dp(q), int(q.size), first_rep,
                                  n_reps, int(bool(with_point)), N.dp(rows), N.u8p(ok)))
        return rows, ok

    def debug_mm_betas(self, seed: int, simulations: int, rep: int):
        """ob_debug_mm_betas: the 2 x simulations QR coefficient vectors of one MM pass (rep =
        OB_MM_POINT_REP = 2^32 - 1 for the point pass): (betas [2, S, K], converged [2, S])."""
        b = np.empty((2, int(simulations), self.k))
        done = np.zeros((2, int(simulations)), dtype=np.uint8)
        N.check(N.lib().ob_debug_mm_betas(self._h, seed & ((1 << 64) - 1), int(simulations), int(rep), N.dp(b),
                                          N.u8p(done)))
        return b, done

    def debug_mm_fail(self, mask=None):
        """ob_debug_mm_fail: mask[g][s] bit (rep & 7) forces fit (g, s) of pass rep to fail."""
        m = np.ascontiguousarray(np.zeros((2, 0)) if mask is None else mask, dtype=np.uint8)
        N.check(N.lib().ob_debug_mm_fail(self._h, N.u8p(m), m.shape[1]))

    def boot_device(self, seed: int, first_rep: int, n_reps: int, rows_ptr: int, ok_ptr: int,
                    ref=ReferenceCoefficients.GroupA, stream: int | None = None):
        N.check(N.lib().ob_boot_run_device(self._h, seed & ((1 << 64) - 1), first_rep, n_reps, int(ref),
                                           C.c_void_p(rows_ptr), C.c_void_p(ok_ptr), C.c_void_p(stream or 0)))

    def boot_sharded(self, seed: int, first_rep: int, n_reps: int, ref=ReferenceCoefficients.GroupA):
        """This rank's shard of [first_rep, first_rep + n_reps) plus the RCCL all-gather
        (ob_boot_run_sharded): every rank returns all rows. Collective over the panel's rank ctx."""
        rows = np.empty((self.n_y, n_reps, self.row_len))
        ok = np.zeros((self.n_y, n_reps), dtype=np.uint8)
        if n_reps:
            N.check(N.lib().ob_boot_run_sharded(self._h, seed & ((1 << 64) - 1), first_rep, n_reps, int(ref), N.dp(rows),
                                                N.u8p(ok)))
        return (rows[0], ok[0]) if self.n_y == 1 else (rows, ok)

    def boot_sharded_device(self, seed: int, first_rep: int, n_reps: int, rows_ptr: int, ok_ptr: int,
                            ref=ReferenceCoefficients.GroupA, stream: int | None = None):
        N.check(N.lib().ob_boot_run_sharded_device(self._h, seed & ((1 << 64) - 1), first_rep, n_reps, int(ref),
                                                   C.c_void_p(rows_ptr), C.c_void_p(ok_ptr), C.c_void_p(stream or 0)))

    def debug_counts(self, seed: int, first_rep: int, n_reps: int, group: int):
        """OBRS-3 counts as the Gram kernel consumes them (ob_debug_counts): (level-1 tile counts
        [n_reps, tiles], per-row counts [n_reps, n_g] uint8)."""
        ng = self.n_a if group == 0 else self.n_b
        tiles = -(-ng // 256)
        l1 = np.zeros((n_reps, tiles), dtype=np.uint32)
        rc = np.zeros((n_reps, ng), dtype=np.uint8)
        N.check(N.lib().ob_debug_counts(self._h, seed & ((1 << 64) - 1), first_rep, n_reps, group,
                                        N.u32p(l1),
                                        N.u8p(rc)))
        return l1, rc

    def debug_gram(self, seed: int, first_rep: int, n_reps: int, path: int = 0):
        """Reduced extended Grams [n_reps, 2, e_pad] (ob_debug_gram): path 1 = f64 MFMA,
        2 = exact integer-sliced i8 MFMA, 0 = the engine's default."""
        e_pad = -(-((self.k + self.n_y) * (self.k + self.n_y + 1) // 2) // 16) * 16
        g = np.empty((n_reps, 2, e_pad))
        N.check(N.lib().ob_debug_gram(self._h, int(path), seed & ((1 << 64) - 1), first_rep, n_reps, N.dp(g)))
        return g

    def debug_chunks(self):
        """The panel's row chunking (ob_debug_chunks): [(group, first tile, end tile), ...]."""
        n = C.c_int32(0)
        N.check(N.lib().ob_debug_chunks(self._h, None, 0, C.byref(n)))
        t = np.zeros(3 * n.value, dtype=np.uint32)
        N.check(N.lib().ob_debug_chunks(self._h, N.u32p(t), n.value, C.byref(n)))
        return [tuple(int(v) for v in t[3 * c: 3 * c + 3]) for c in range(n.value)]

    def set_gather_columns(self, cols=None):
        """Row columns the sharded entry points gather (ob_panel_set_gather_columns); None = all."""
        c = np.ascontiguousarray([] if cols is None else cols, dtype=np.int32)
        N.check(N.lib().ob_panel_set_gather_columns(self._h, N.i32p(c), len(c)))

    def component_columns(self):
        """The row columns the aggregation reads: two-fold, three-fold, total gap, detailed."""
        return list(range(6 + 2 * (self.k + self.n_base)))

    def debug_shard_sim(self, world: int, self_rank: int, seed: int, first_rep: int, n_reps: int,
                        ref=ReferenceCoefficients.GroupA):
        """ob_debug_shard_sim: a `world`-rank sharded run simulated on this GPU, as rank
        `self_rank` receives it."""
        rows = np.empty((self.n_y, n_reps, self.row_len))
        ok = np.zeros((self.n_y, n_reps), dtype=np.uint8)
        if n_reps:
            N.check(N.lib().ob_debug_shard_sim(self._h, world, self_rank, seed & ((1 << 64) - 1), first_rep, n_reps,
                                               int(ref), N.dp(rows), N.u8p(ok)))
        return (rows[0], ok[0]) if self.n_y == 1 else (rows, ok)

    def debug_gram_exceptions(self):
        """The i8 Gram's exception rows (ob_debug_gram_exceptions): (bits, [(group, row), ...])."""
        bits, n = C.c_int32(0), C.c_int32(0)
        buf = np.zeros(4096, dtype=np.uint32)
        N.check(N.lib().ob_debug_gram_exceptions(self._h, C.byref(bits), C.byref(n),
                                                 N.u32p(buf), len(buf)))
        ent = buf[: n.value]
        return bits.value, [(int(e >> 31), int(e & 0x7FFFFFFF)) for e in ent]

    def sync(self):
        N.check(N.lib().ob_panel_sync(self._h))

    def timing(self) -> dict:
        t = N.ob_timing()
        N.check(N.lib().ob_panel_last_timing(self._h, C.byref(t)))
        return N.struct_dict(t)

    def close(self):
        if self._h:
            N.lib().ob_panel_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def boot_multi(panels, seed: int, first_rep: int, n_reps: int, ref=ReferenceCoefficients.GroupA):
    """One process, several GPUs (ob_boot_run_multi): panels[i] (same design, distinct devices)
    runs shard i; the shards are all-gathered over an RCCL clique of those devices."""
    p0 = panels[0]
    rows = np.empty((p0.n_y, n_reps, p0.row_len))
    ok = np.zeros((p0.n_y, n_reps), dtype=np.uint8)
    hs = (C.c_void_p * len(panels))(*[p._h for p in panels])
    if n_reps:
        N.check(N.lib().ob_boot_run_multi(hs, len(panels), seed & ((1 << 64) - 1), first_rep, n_reps, int(ref),
                                          N.dp(rows), N.u8p(ok)))
    return (rows[0], ok[0]) if p0.n_y == 1 else (rows, ok)


def bootstrap_stats(values, point_estimate: float = 0.0):
    """inference.rs:4-34 -> (std_err, p_value, (ci_lower, ci_upper)) via the native routine."""
    v = np.ascontiguousarray(values, dtype=np.float64)
    out = np.empty(4)
    N.check(N.lib().ob_bootstrap_stats(N.dp(v), len(v), float(point_estimate), N.dp(out)))
    return out[0], out[1], (out[2], out[3])


def aggregate(rows, ok, cols):
    """ob_aggregate: bootstrap_stats of each row column over ok rows -> (n_cols, 4) array of
    (std_err, p_value, ci_lower, ci_upper)."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    ok = np.ascontiguousarray(ok, dtype=np.uint8)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    out = np.empty((len(cols), 4))
    N.check(N.lib().ob_aggregate(N.dp(rows), N.u8p(ok), len(ok), rows.shape[1],
                                 N.i32p(cols), len(cols), N.dp(out)))
    return out


def jackknife_rows(xa, ya, wa, xb, yb, wb, ref_mode=ReferenceCoefficients.GroupA, n_num=None, device=None):
    """theta_(i) of every row (A's first) for predictor-only designs xa, xb -> (theta, kept, n_dropped)."""
    panel = Panel(xa, ya, xb, yb, wa, wb, n_num=n_num, device=device)
    try:
        return panel.jackknife_rows(ref_mode)
    finally:
        panel.close()


def jackknife_last_timing() -> float:
    ms = C.c_double()
    N.check(N.lib().ob_jackknife_last_timing(C.byref(ms)))
    return ms.value


def jackknife_check_shape(k: int, n_a: int, n_b: int, n_norm: int = 0, n_y: int = 1, heckman: bool = False,
                          want_rows: bool = False) -> None:
    """ob_jackknife_check_shape: raises OaxacaError where the jackknife entry points would (host only)."""
    N.check(N.lib().ob_jackknife_check_shape(k, n_a, n_b, n_norm, n_y, int(heckman), int(want_rows)))


def jackknife_finish(sums, n_used):
    """ob_jackknife_finish: sums (2, C, 3), n_used (2,) -> (C, 3) = accel, jack_se, jack_bias."""
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    if sums.ndim != 3 or sums.shape[0] != 2 or sums.shape[2] != 3:
        raise ValueError("sums must be (2, C, 3)")
    m = (C.c_int64 * 2)(int(n_used[0]), int(n_used[1]))
    out = np.zeros((sums.shape[1], 3))
    N.check(N.lib().ob_jackknife_finish(N.dp(sums), m, sums.shape[1], N.dp(out)))
    return out


def bca_stats(estimates, point: float, accel: float, level: float = 0.95) -> dict:
    """ob_bca_stats -> dict(ci_lower, ci_upper, z0, alpha_lo, alpha_hi, flag)."""
    v = np.ascontiguousarray(estimates, dtype=np.float64)
    out = np.zeros(6)
    N.check(N.lib().ob_bca_stats(N.dp(v), len(v), float(point), float(accel), float(level), N.dp(out)))
    return {"ci_lower": out[0], "ci_upper": out[1], "z0": out[2], "alpha_lo": out[3], "alpha_hi": out[4],
            "flag": int(out[5])}


def aggregate_bca(rows, ok, cols, point, accel, level: float = 0.95):
    """ob_aggregate_bca -> (len(cols), 6)."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    ok = np.ascontiguousarray(ok, dtype=np.uint8)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    point = np.ascontiguousarray(point, dtype=np.float64)
    accel = np.ascontiguousarray(accel, dtype=np.float64)
    out = np.zeros((len(cols), 6))
    N.check(N.lib().ob_aggregate_bca(N.dp(rows), N.u8p(ok), len(ok), rows.shape[1],
                                     N.i32p(cols), len(cols), N.dp(point), N.dp(accel), float(level), N.dp(out)))
    return out


def rif(y, quantile: float):
    """math/rif.rs:14-88 via the native routine."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    out = np.empty_like(y)
    N.check(N.lib().ob_rif(N.dp(y), len(y), float(quantile), N.dp(out)))
    return out


def parse_rif_statistic(stat, **params) -> tuple:
    """The Python surface of ``ob_rif_spec`` -> (code, p0, p1). ``stat``: "variance", "gini" or "iqr" (with
    ``upper`` = 0.9 and ``lower`` = 0.1 by default); also a ``(stat, params)`` pair or a dict with a ``stat`` key,
    as ``decompose_statistics`` lists them. An unknown statistic is ``OB_E_INVALID``; the quantiles' range is
    checked by the library."""
    if isinstance(stat, dict):
        params = {**{k: v for k, v in stat.items() if k != "stat"}, **params}
        stat = stat.get("stat")
    elif isinstance(stat, (tuple, list)):
        if len(stat) != 2 or not isinstance(stat[1], dict):
            raise ValueError("a statistic is a name, a (name, params) pair or a dict with a 'stat' key")
        stat, params = stat[0], {**stat[1], **params}
    if not isinstance(stat, str) or stat not in N.OB_RIF_STATS:
        raise N.OaxacaError(N.OB_E_INVALID, f"unknown RIF statistic {stat!r} (variance, gini, iqr)")
    allowed = ("upper", "lower") if stat == "iqr" else ()
    extra = sorted(set(params) - set(allowed))
    if extra:
        raise ValueError(f"{stat}: unexpected parameter(s) {', '.join(extra)}")
    if stat == "iqr":
        return N.OB_RIF_IQR, float(params.get("upper", 0.9)), float(params.get("lower", 0.1))
    return N.OB_RIF_STATS[stat], 0.0, 0.0


def parse_weighted_rif_statistic(stat, **params) -> tuple:
    """``parse_rif_statistic`` for the weighted entry points (``ob_rif_stat_weighted``, the reweighted decomposition
    of a statistic): the same statistics and forms, plus ``"quantile"`` with ``tau`` (0.5 by default)."""
    name, kw = stat, dict(params)
    if isinstance(stat, dict):
        name, kw = stat.get("stat"), {**{k: v for k, v in stat.items() if k != "stat"}, **params}
    elif isinstance(stat, (tuple, list)) and len(stat) == 2 and isinstance(stat[1], dict):
        name, kw = stat[0], {**stat[1], **params}
    if name != "quantile":
        if isinstance(name, str) and name in N.OB_RIF_STATS or not isinstance(name, str):
            return parse_rif_statistic(stat, **params)
        raise N.OaxacaError(N.OB_E_INVALID, f"unknown RIF statistic {name!r} (variance, gini, iqr, quantile)")
    extra = sorted(set(kw) - {"tau"})
    if extra:
        raise ValueError(f"quantile: unexpected parameter(s) {', '.join(extra)}")
    return N.OB_RIF_QUANTILE, float(kw.get("tau", 0.5)), 0.0


def weighted_rif_name(parsed) -> tuple:
    """(code, p0, p1) -> (name, params), what ``ReweightedDecompositionResults.statistic`` holds."""
    code, p0, p1 = parsed
    name = {v: k for k, v in N.OB_RIF_WSTATS.items()}[code]
    if code == N.OB_RIF_IQR:
        return name, {"upper": p0, "lower": p1}
    return name, ({"tau": p0} if code == N.OB_RIF_QUANTILE else {})


def rif_specs(stats):
    """A ctypes array of ``ob_rif_spec`` for a list of statistics (``parse_rif_statistic`` each)."""
    parsed = [parse_rif_statistic(s) for s in stats]
    if not parsed:
        raise ValueError("statistics must be a non-empty sequence")
    return (N.ob_rif_spec * len(parsed))(*[N.ob_rif_spec(*p) for p in parsed])


def with_context(call, device: int | None = None):
    """``call(ctx)`` -> rc on the device's context. Without a GPU the call still runs once with a NULL context, so
    that its argument errors surface as they do on a GPU machine; good arguments leave the missing device as the
    error."""
    try:
        ctx = N.context(device)
    except (N.OaxacaError, ImportError):
        rc = call(None)
        if not (rc == N.OB_E_INVALID and b"null pointer" in N.lib().ob_last_error()):
            N.check(rc)
        raise
    N.check(call(ctx))


def _last_timing(symbol: str, struct) -> dict:
    """This thread's last timing record of one estimator: ``symbol`` fills a ``struct``."""
    t = struct()
    N.check(getattr(N.lib(), symbol)(C.byref(t)))
    return N.struct_dict(t)


# One group's rows as the array entry points take them. Each check raises ValueError(what).
def _design(x, what="x must be (n, k)"):
    """A design matrix: float64, column-major -> (array, n, k)."""
    xf = np.asfortranarray(x, dtype=np.float64)
    if xf.ndim != 2:
        raise ValueError(what)
    return (xf,) + xf.shape


def _per_row(v, n: int, what: str, optional: bool = False):
    """One float64 per row; an ``optional`` vector (weights) may be ``None`` and stays so."""
    if v is None and optional:
        return None
    v = np.ascontiguousarray(v, dtype=np.float64)
    if v.shape != (n,):
        raise ValueError(what)
    return v


def _counts_u8(counts, n: int, by_rep: bool = False):
    """Resample counts in [0, 255] as the kernels read them: uint8 (n,), or ``by_rep`` (n_reps, n) with a plain
    vector taken as one replicate; ``None`` (every row once) stays ``None``."""
    if counts is None:
        return None
    c = np.ascontiguousarray(counts)
    if by_rep:
        c = np.atleast_2d(c)
    if c.shape[1 if by_rep else 0:] != (n,) or (c < 0).any() or (c > 255).any():
        raise ValueError(f"counts must be {'(n_reps, n)' if by_rep else 'n'} integers in [0, 255]")
    return np.ascontiguousarray(c.astype(np.uint8))


def rif_statistic(y, stat, device: int | None = None, **params):
    """``ob_rif_stat``: the recentred influence function of ``stat`` ("variance", "gini", "iqr" with ``upper`` /
    ``lower``) over ``y`` on the GPU -> (rif in y's order, the statistic). Unweighted; n >= 2."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    if y.ndim != 1:
        raise ValueError("y must be one-dimensional")
    spec = N.ob_rif_spec(*parse_rif_statistic(stat, **params))
    out, value = np.empty_like(y), C.c_double()
    with_context(lambda ctx: N.lib().ob_rif_stat(ctx, N.dp(y), len(y), C.byref(spec), N.dp(out), C.byref(value)), device)
    return out, value.value


def rif_statistic_weighted(y, w, stat, device: int | None = None, **params):
    """``ob_rif_stat_weighted``: the weighted recentred influence function of ``stat`` ("variance", "gini",
    "quantile" with ``tau``, "iqr" with ``upper`` / ``lower``) over ``y`` with weights ``w`` >= 0 on the GPU ->
    (rif in y's order, the statistic). At w = 1 it is ``rif_statistic``'s definition."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    if y.ndim != 1 or w.shape != y.shape:
        raise ValueError("y and w must be one-dimensional and of one length")
    spec = N.ob_rif_spec(*parse_weighted_rif_statistic(stat, **params))
    out, value = np.empty_like(y), C.c_double()
    with_context(lambda ctx: N.lib().ob_rif_stat_weighted(ctx, N.dp(y), N.dp(w), len(y), C.byref(spec), N.dp(out),
                                                          C.byref(value)), device)
    return out, value.value


def rif_scan_block() -> int:
    """ob_rif_scan_block: sorted values per scan block of the RIF statistics pass."""
    return int(N.lib().ob_rif_scan_block())


def rif_last_timing() -> dict:
    """ob_rif_last_timing: sort / scan / kde / scatter ms of this thread's last RIF statistics call."""
    return _last_timing("ob_rif_last_timing", N.ob_rif_timing)


def logit(y, x, max_iter: int = 100, tol: float = 1e-6, device: int | None = None):
    """math/logit.rs:31-118 with the Newton passes on the GPU (``ob_logit``). ``x``: (n, k) with the
    intercept column included, ``k <= OB_LOGIT_MAX_K``. Returns (coefficients, predicted_probs,
    converged, iterations); on convergence the probabilities are those of the last iteration's
    start, as in the reference."""
    xf, n, k = _design(x)
    y = _per_row(y, n, "y must have one entry per row of x")
    beta, probs = np.empty(k), np.empty(n)
    conv, iters = C.c_int32(0), C.c_int32(0)
    N.check(N.lib().ob_logit(N.context(device), N.dp(xf), max(n, 1), N.dp(y), n, k, int(max_iter), float(tol),
                             N.dp(beta), N.dp(probs), C.byref(conv), C.byref(iters)))
    return beta, probs, bool(conv.value), int(iters.value)


def probit(x, y, max_iter: int = 100, tol: float = 1e-6, device: int | None = None):
    """math/probit.rs::probit with the Fisher-scoring passes on the GPU (``ob_probit``). ``x``: (n, k)
    with the intercept (all ones) as column 0, ``k <= 32``; ``y``: the 0/1 outcome. Returns
    (coefficients, converged, iterations); running out of iterations is not an error."""
    xf, n, k = _design(x)
    y = _per_row(y, n, "y must have one entry per row of x")
    beta = np.empty(k)
    conv, iters = C.c_int32(0), C.c_int32(0)
    N.check(N.lib().ob_probit(N.context(device), N.dp(xf), max(n, 1), N.dp(y), n, k, int(max_iter), float(tol),
                              N.dp(beta), C.byref(conv), C.byref(iters)))
    return beta, bool(conv.value), int(iters.value)


def binary_means(x, y, betas, counts=None, device: int | None = None) -> dict:
    """The mean-probability pass of the binary decomposition alone (``ob_binary_means``) over one group.
    ``x``: (n, k) with the intercept (all ones) as column 0, ``k <= 32``; ``y``: the outcome; ``betas``: (3, k);
    ``counts``: n resample counts below 256 (``None``: every row once). Returns ``probabilities`` (the three
    count-weighted means of Phi(x'beta)), ``y_mean``, ``n`` (the counts' sum) and ``x_mean`` (k)."""
    xf, n, k = _design(x)
    what = "y must have one entry per row of x and betas must be (3, k)"
    y = _per_row(y, n, what)
    b = np.ascontiguousarray(betas, dtype=np.float64)
    if b.shape != (3, k):
        raise ValueError(what)
    c8 = _counts_u8(counts, n)
    out = np.empty(5 + k)
    with_context(lambda ctx: N.lib().ob_binary_means(ctx, N.dp(xf), max(n, 1), N.dp(y), n, k, N.u8p(c8), N.dp(b),
                                                     N.dp(out)), device)
    return {"probabilities": out[:3].copy(), "y_mean": float(out[3]), "n": float(out[4]), "x_mean": out[5:].copy()}


def binary_check_shape(k: int, n_a: int, n_b: int) -> None:
    """ob_binary_check_shape: raises OaxacaError where a binary decomposition would (host only)."""
    N.check(N.lib().ob_binary_check_shape(int(k), int(n_a), int(n_b)))


def binary_row_len(k: int) -> int:
    """ob_binary_row_len: 6 + 7k + 8 doubles per replicate of a binary decomposition."""
    return int(N.lib().ob_binary_row_len(int(k)))


def binary_last_timing() -> dict:
    """ob_binary_last_timing: HIP-event ms of this thread's last binary boot (probit, means pass, rows)."""
    return _last_timing("ob_binary_last_timing", N.ob_binary_timing)


def _tobit_config(lower, upper):
    """ob_tobit_config of two optional limits."""
    tc = N.ob_tobit_config()
    tc.has_lower, tc.has_upper = int(lower is not None), int(upper is not None)
    tc.lower, tc.upper = float(lower or 0.0), float(upper or 0.0)
    return tc


def _tobit_group(x, y, w):
    """(x column-major, n, k, y, w) of one group for the Tobit array entry points."""
    xf, n, k = _design(x)
    what = "y (and w) must have one entry per row of x"
    return xf, n, k, _per_row(y, n, what), _per_row(w, n, what, optional=True)


def tobit_pass(x, y, etas, lower=None, upper=None, w=None, counts=None, device: int | None = None):
    """One Newton pass of the Tobit fit alone (``ob_tobit_pass``) over one group. ``x``: (n, k) with the intercept
    (all ones) as column 0, ``k <= 31``; ``y``: the censored outcome; ``etas``: (m, k + 1) parameter vectors
    [delta; theta], m <= 64; ``counts``: n resample counts below 256 (``None``: every row once). Returns
    (-Hessian (m, k + 1, k + 1), gradient (m, k + 1), N_unc (m,))."""
    xf, n, k, y, w = _tobit_group(x, y, w)
    e = np.ascontiguousarray(np.atleast_2d(np.asarray(etas, dtype=np.float64)))
    if e.shape[1:] != (k + 1,):
        raise ValueError("etas must be (m, k + 1)")
    c8, tc, m = _counts_u8(counts, n), _tobit_config(lower, upper), len(e)
    info, grad, nunc = np.empty((m, k + 1, k + 1)), np.empty((m, k + 1)), np.empty(m)
    with_context(lambda ctx: N.lib().ob_tobit_pass(ctx, N.dp(xf), max(n, 1), N.dp(y), N.dp(w), N.u8p(c8), n, k,
                                                   C.byref(tc), N.dp(e), m, N.dp(info), N.dp(grad), N.dp(nunc)), device)
    return info, grad, nunc


def tobit_fit(x, y, lower=None, upper=None, w=None, counts=None, n_reps: int = 1, eta0=None,
              device: int | None = None):
    """The Tobit fits alone (``ob_tobit_fit``) over one group: ``counts`` (n_reps, n) resample counts (``None``:
    ``n_reps`` fits of every row once), ``eta0`` (k + 1) the start of every fit (``None``: the least-squares start).
    Returns (eta (n_reps, k + 1), flags (n_reps) of ``OB_TOBIT_DONE | OB_TOBIT_FAILED``, passes (n_reps))."""
    xf, n, k, y, w = _tobit_group(x, y, w)
    c8 = _counts_u8(counts, n, by_rep=True)
    reps = int(n_reps) if c8 is None else len(c8)
    e0 = None if eta0 is None else np.ascontiguousarray(eta0, dtype=np.float64)
    if e0 is not None and e0.shape != (k + 1,):
        raise ValueError("eta0 must be (k + 1,)")
    tc = _tobit_config(lower, upper)
    eta = np.empty((max(reps, 0), k + 1))
    flags, passes = np.zeros(max(reps, 0), dtype=np.uint32), np.zeros(max(reps, 0), dtype=np.uint32)
    with_context(lambda ctx: N.lib().ob_tobit_fit(ctx, N.dp(xf), max(n, 1), N.dp(y), N.dp(w), n, k, C.byref(tc),
                                                  N.u8p(c8), reps, N.dp(e0), N.dp(eta), N.u32p(flags),
                                                  N.u32p(passes)), device)
    return eta, flags, passes


def tobit(x, y, lower=None, upper=None, w=None, device: int | None = None) -> dict:
    """The censored-normal (Tobit) maximum-likelihood fit of ``y`` on ``x`` on the GPU: ``tobit_fit`` of every row
    once from the least-squares start. Returns ``beta`` (k), ``sigma``, ``eta`` (k + 1), ``converged`` and
    ``passes``."""
    eta, flags, passes = tobit_fit(x, y, lower, upper, w, device=device)
    e = eta[0]
    return {"beta": e[:-1] / e[-1], "sigma": float(1.0 / e[-1]), "eta": e.copy(),
            "converged": int(flags[0]) == N.OB_TOBIT_DONE, "passes": int(passes[0])}


def tobit_means(x, y, etas, lower=None, upper=None, w=None, counts=None, device: int | None = None) -> dict:
    """The conditional-mean pass of the Tobit decomposition alone (``ob_tobit_means``) over one group and one
    replicate's ``counts``: ``etas`` (2, k + 1) the two fits whose parameters are applied. Returns ``means`` (2),
    ``y_mean``, ``n`` (sum c w), ``censored_share`` (left, right) and ``x_mean`` (k)."""
    xf, n, k, y, w = _tobit_group(x, y, w)
    e = np.ascontiguousarray(etas, dtype=np.float64)
    if e.shape != (2, k + 1):
        raise ValueError("etas must be (2, k + 1)")
    c8, tc = _counts_u8(counts, n), _tobit_config(lower, upper)
    out = np.empty(6 + k)
    with_context(lambda ctx: N.lib().ob_tobit_means(ctx, N.dp(xf), max(n, 1), N.dp(y), N.dp(w), N.u8p(c8), n, k,
                                                    C.byref(tc), N.dp(e), N.dp(out)), device)
    return {"means": out[:2].copy(), "y_mean": float(out[2]), "n": float(out[3]),
            "censored_share": (float(out[4]), float(out[5])), "x_mean": out[6:].copy()}


def tobit_rows(xa, ya, xb, yb, lower=None, upper=None, wa=None, wb=None, counts_a=None, counts_b=None,
               reference_coefficients=ReferenceCoefficients.GroupA, device: int | None = None):
    """Fits, means and rows of the Tobit decomposition over two groups of rows with given resample counts
    (``ob_tobit_rows``): ``counts_a`` (n_reps, n_a) and ``counts_b`` (n_reps, n_b), or both ``None`` for the point
    pass. Returns (rows (n_reps, tobit_row_len(k)), ok (n_reps))."""
    xfa, na, k, ya, wa = _tobit_group(xa, ya, wa)
    xfb, nb, kb, yb, wb = _tobit_group(xb, yb, wb)
    if kb != k:
        raise ValueError("xa and xb must have the same columns")
    ca, cb = _counts_u8(counts_a, na, by_rep=True), _counts_u8(counts_b, nb, by_rep=True)
    if (ca is None) != (cb is None) or (ca is not None and len(ca) != len(cb)):
        raise ValueError("counts_a and counts_b must be given together, for the same replicates")
    reps, tc = 1 if ca is None else len(ca), _tobit_config(lower, upper)
    rows, ok = np.empty((reps, tobit_row_len(k))), np.zeros(reps, dtype=np.uint8)
    with_context(lambda ctx: N.lib().ob_tobit_rows(
        ctx, k, C.byref(tc), int(reference_coefficients), N.dp(xfa), max(na, 1), N.dp(ya), N.dp(wa), na, N.u8p(ca),
        N.dp(xfb), max(nb, 1), N.dp(yb), N.dp(wb), nb, N.u8p(cb), reps, N.dp(rows), N.u8p(ok)), device)
    return rows, ok


def tobit_lambda(z) -> np.ndarray:
    """ob_tobit_lambda (host only): the inverse Mills ratio phi(z) / Phi(z) by the branches the kernels take."""
    z = np.ascontiguousarray(z, dtype=np.float64)
    out = np.empty_like(z)
    N.check(N.lib().ob_tobit_lambda(N.dp(z.ravel()), z.size, N.dp(out.ravel())))
    return out


def tobit_check_shape(k: int, n_a: int, n_b: int) -> None:
    """ob_tobit_check_shape: raises OaxacaError where a Tobit decomposition would (host only); ``n_a`` and ``n_b``
    are the groups' uncensored rows."""
    N.check(N.lib().ob_tobit_check_shape(int(k), int(n_a), int(n_b)))


def tobit_row_len(k: int) -> int:
    """ob_tobit_row_len: 6 + 7k + 17 doubles per replicate of a Tobit decomposition."""
    return int(N.lib().ob_tobit_row_len(int(k)))


def tobit_last_timing() -> dict:
    """ob_tobit_last_timing: the Newton rounds and the HIP-event ms of the pass kernels, the means pass and the rows
    of this thread's last Tobit boot (or prepare, ``tobit_fit`` or ``tobit_rows``)."""
    return _last_timing("ob_tobit_last_timing", N.ob_tobit_timing)


def _refit_pass_args(n: int, counts, x):
    """What ``rifq_pass`` and ``rifs_pass`` share: the optional (n, p) predictors and the (n_reps, n) counts of the n
    sorted rows -> (x column-major or None, p, uint8 counts or None, n_reps)."""
    xf, p = None, 0
    if x is not None:
        xf, rows, p = _design(x, "x must be (n, p)")
        if rows != n:
            raise ValueError("x must be (n, p)")
        if p == 0:
            xf = None
    c8 = _counts_u8(counts, n, by_rep=True)
    return xf, p, c8, 1 if c8 is None else len(c8)


def rifq_pass(y_sorted, taus, counts=None, x=None, device: int | None = None) -> dict:
    """The RIF of quantiles refitted on resamples of one group (``ob_rifq_pass``). ``y_sorted``: the
    group's outcome in ascending order; ``taus``: up to 8 strictly increasing quantiles in (0, 1); ``counts``:
    (n_reps, n) resample counts below 256 over the sorted rows, each replicate summing to n (``None``: the point
    pass, every row once); ``x``: (n, p) predictors in y's row order, ``p <= 31``. Returns ``q``, ``f``, ``n_le``,
    ``floored`` (n_reps, T), ``bw`` (n_reps), ``t`` (n_reps, T, p + 1) = the sums of c v over the rows with
    y <= q, v = [1, x], and ``gy`` (n_reps, T, p + 2) = the y-pairs G[a, y], then G[y, y], of the extended Gram."""
    y = np.ascontiguousarray(y_sorted, dtype=np.float64)
    tq = np.ascontiguousarray(np.atleast_1d(taus), dtype=np.float64)
    if y.ndim != 1 or tq.ndim != 1:
        raise ValueError("y_sorted and taus must be one-dimensional")
    n, nt = len(y), len(tq)
    xf, p, c8, reps = _refit_pass_args(n, counts, x)
    q, f, nle = np.empty((reps, nt)), np.empty((reps, nt)), np.empty((reps, nt))
    bw, t, gy = np.empty(reps), np.empty((reps, nt, p + 1)), np.empty((reps, nt, p + 2))
    fl = np.zeros((reps, nt), dtype=np.uint8)
    with_context(lambda ctx: N.lib().ob_rifq_pass(ctx, N.dp(y), n, N.u8p(c8), reps, N.dp(tq), nt, N.dp(xf), max(n, 1), p,
                                                  N.dp(q), N.dp(bw), N.dp(f), N.dp(nle), N.dp(t), N.dp(gy), N.u8p(fl)),
                 device)
    return {"q": q, "bw": bw, "f": f, "n_le": nle, "t": t, "gy": gy, "floored": fl.astype(bool)}


def rifq_check_shape(k: int, taus, n_a: int, n_b: int) -> None:
    """ob_rifq_check_shape: raises OaxacaError where a refitted quantile decomposition would (host only)."""
    tq = np.ascontiguousarray(np.atleast_1d(taus), dtype=np.float64)
    N.check(N.lib().ob_rifq_check_shape(int(k), len(tq), N.dp(tq), int(n_a), int(n_b)))


def rifq_row_len(k: int, n_base: int = 0) -> int:
    """ob_rifq_row_len: the OLS row followed by q_A, q_B, f_A, f_B, N_le,A, N_le,B."""
    return int(N.lib().ob_rifq_row_len(int(k), int(n_base)))


def rifq_last_timing() -> dict:
    """ob_rifq_last_timing: HIP-event ms of this thread's last rifq_pass, or prepare / boot of a refit handle: search,
    density, patch, and for a handle gram (resample, f64 Gram, reduce) and solve (y-pairs, solves, rows)."""
    return _last_timing("ob_rifq_last_timing", N.ob_rifq_timing)


def _rif_specs(stats):
    """names, (name, params) pairs, dicts or parsed (code, p0, p1) triples -> (ctypes array of ob_rif_spec, triples)."""
    stats = [stats] if isinstance(stats, (str, dict)) else list(stats)
    parsed = [s if isinstance(s, tuple) and len(s) == 3 else parse_rif_statistic(s) for s in stats]
    return (N.ob_rif_spec * max(len(parsed), 1))(*[N.ob_rif_spec(*p) for p in parsed]), parsed


def rifs_pass(y_sorted, stats, counts=None, x=None, device: int | None = None) -> dict:
    """The RIFs of the variance, the Gini and quantile ranges refitted on resamples of one group (``ob_rifs_pass``,
    DESIGN.md §5.19). ``y_sorted``: the group's outcome in ascending order; ``stats``: up to 8 statistics as
    ``decompose_statistics`` lists them (the ranges share at most 8 distinct quantiles); ``counts``: (n_reps, n)
    resample counts below 256 over the sorted rows, each replicate summing to n (``None``: the point pass, every row
    once); ``x``: (n, p) predictors in y's row order, ``p <= 31``. Returns ``nu`` (n_reps, S) = the statistics on the
    expanded resamples, ``gy`` (n_reps, S, p + 2) = the y-pairs G[a, RIF], then G[RIF, RIF], of the extended Gram,
    ``floored`` (n_reps, S) = a range's density floor flags and ``ok`` (n_reps, S), False where a Gini's resample has
    mean 0."""
    y = np.ascontiguousarray(y_sorted, dtype=np.float64)
    if y.ndim != 1:
        raise ValueError("y_sorted must be one-dimensional")
    specs, parsed = _rif_specs(stats)
    n, ns = len(y), len(parsed)
    xf, p, c8, reps = _refit_pass_args(n, counts, x)
    nu, gy = np.empty((reps, ns)), np.empty((reps, ns, p + 2))
    fl, ok = np.zeros((reps, ns), dtype=np.uint8), np.zeros((reps, ns), dtype=np.uint8)
    with_context(lambda ctx: N.lib().ob_rifs_pass(ctx, N.dp(y), n, N.u8p(c8), reps, specs, ns, N.dp(xf), max(n, 1), p,
                                                  N.dp(nu), N.dp(gy), N.u8p(fl), N.u8p(ok)), device)
    return {"nu": nu, "gy": gy, "floored": fl.astype(bool), "ok": ok.astype(bool)}


def rifs_check_shape(k: int, stats, n_a: int, n_b: int) -> None:
    """ob_rifs_check_shape: raises OaxacaError where a refitted statistics decomposition would (host only)."""
    specs, parsed = _rif_specs(stats)
    N.check(N.lib().ob_rifs_check_shape(int(k), specs, len(parsed), int(n_a), int(n_b)))


def rifs_row_len(k: int, n_base: int = 0) -> int:
    """ob_rifs_row_len: the OLS row followed by nu_A, nu_B."""
    return int(N.lib().ob_rifs_row_len(int(k), int(n_base)))


def rifs_last_timing() -> dict:
    """ob_rifs_last_timing: HIP-event ms of this thread's last rifs_pass, or prepare / boot of a statistics refit
    handle: moment, scan, gini, tie, finish, rifq (the ranges' quantile pass), and for a handle gram and solve."""
    return _last_timing("ob_rifs_last_timing", N.ob_rifs_timing)


def _coefficient_rows(coefs, k: int, what: str):
    """(m, k) coefficient vectors; a plain vector is one row."""
    c = np.ascontiguousarray(np.atleast_2d(coefs), dtype=np.float64)
    if c.ndim != 2 or c.shape[1] != k:
        raise ValueError(what)
    return c


def _reweight_args(x, second, w, counts, gammas):
    """The arrays of the two reweighting pieces as the C ABI takes them."""
    what = "d / y must have one entry per row of x and gammas must be (R, k)"
    xf, n, k = _design(x)
    second = _per_row(second, n, what)
    g = _coefficient_rows(gammas, k, what)
    wv = _per_row(w, n, "w must have one entry per row of x", optional=True)
    return xf, second, wv, _counts_u8(counts, n), g, n, k


def reweight_logit_pass(x, d, gammas, w=None, counts=None, device: int | None = None):
    """One Newton pass of the reweighted decomposition's propensity logit alone (``ob_reweight_logit_pass``).
    ``x``: (n, k) with the intercept (all ones) as column 0, ``k <= 32``; ``d``: n values 0.0 / 1.0; ``gammas``:
    (R, k) coefficient vectors, ``R <= 64``; ``w``: n weights (``None``: 1); ``counts``: n resample counts below
    256 (``None``: every row once). Returns ``(info, grad)``: (R, k, k) sums c w p (1 - p) x x' and (R, k) sums
    c w (d - p) x, p the sigmoid of x'gamma clamped to [1e-10, 1 - 1e-10]."""
    xf, dv, wv, c8, g, n, k = _reweight_args(x, d, w, counts, gammas)
    info, grad = np.empty((len(g), k, k)), np.empty((len(g), k))
    with_context(lambda ctx: N.lib().ob_reweight_logit_pass(ctx, N.dp(xf), max(n, 1), N.dp(dv), N.dp(wv), N.u8p(c8), n, k,
                                                           N.dp(g), len(g), N.dp(info), N.dp(grad)), device)
    return info, grad


def reweight_gram(x, y, gammas, w=None, counts=None, device: int | None = None):
    """The psi-weighted extended Gram of the reweighted decomposition alone (``ob_reweight_gram``) over one
    group: ``(gram, ess_den)`` with gram (R, k + 1, k + 1) = sum c w psi v v', v = [x, y], psi = p / (1 - p) of the
    clamped p at each of the (R, k) ``gammas``, and ess_den (R) = sum c (w psi)^2. Arguments as
    ``reweight_logit_pass``."""
    xf, yv, wv, c8, g, n, k = _reweight_args(x, y, w, counts, gammas)
    gram, den = np.empty((len(g), k + 1, k + 1)), np.empty(len(g))
    with_context(lambda ctx: N.lib().ob_reweight_gram(ctx, N.dp(xf), max(n, 1), N.dp(yv), N.dp(wv), N.u8p(c8), n, k,
                                                     N.dp(g), len(g), N.dp(gram), N.dp(den)), device)
    return gram, den


def reweight_check_shape(k: int, n_a: int, n_b: int) -> None:
    """ob_reweight_check_shape: raises OaxacaError where a reweighted decomposition would (host only)."""
    N.check(N.lib().ob_reweight_check_shape(int(k), int(n_a), int(n_b)))


def reweight_row_len(k: int) -> int:
    """ob_reweight_row_len: 7 + 11k + 5 doubles per replicate of a reweighted decomposition."""
    return int(N.lib().ob_reweight_row_len(int(k)))


def reweight_last_timing() -> dict:
    """ob_reweight_last_timing: logit passes and HIP-event ms (logit passes, Grams, rows) of this thread's last
    reweighted boot."""
    return _last_timing("ob_reweight_last_timing", N.ob_reweight_timing)


def _dr_args(x, w, counts, betas):
    """The arrays of the two distribution-regression pieces as the C ABI takes them."""
    xf, n, k = _design(x)
    b = _coefficient_rows(betas, k, "betas must be (m, k)")
    wv = _per_row(w, n, "w must have one entry per row of x", optional=True)
    return xf, wv, _counts_u8(counts, n), b, n, k


def dr_logit_pass(x, y, thresholds, betas, w=None, counts=None, device: int | None = None):
    """One Newton pass of the distribution regression's threshold logits alone (``ob_dr_logit_pass``). ``x``: (n, k)
    with the intercept (all ones) as column 0, ``k <= 32``; ``y``: n outcomes; ``thresholds``: T <= 64 values;
    ``betas``: (T, k), one coefficient vector per threshold; ``w``: n weights (``None``: 1); ``counts``: n resample
    counts below 256 (``None``: every row once). Returns ``(info, grad)``: (T, k, k) sums c w p (1 - p) x x' and
    (T, k) sums c w (1[y <= c_t] - p) x, p the sigmoid of x'beta_t clamped to [1e-10, 1 - 1e-10]."""
    xf, wv, c8, b, n, k = _dr_args(x, w, counts, betas)
    yv = np.ascontiguousarray(y, dtype=np.float64)
    thr = np.ascontiguousarray(thresholds, dtype=np.float64)
    if yv.shape != (n,) or thr.ndim != 1 or len(thr) != len(b):
        raise ValueError("y must have one entry per row of x and betas one row per threshold")
    info, grad = np.empty((len(b), k, k)), np.empty((len(b), k))
    with_context(lambda ctx: N.lib().ob_dr_logit_pass(ctx, N.dp(xf), max(n, 1), N.dp(yv), N.dp(wv), N.u8p(c8), n, k,
                                                     N.dp(thr), len(thr), N.dp(b), N.dp(info), N.dp(grad)), device)
    return info, grad


def dr_cdf(x, betas, w=None, counts=None, device: int | None = None):
    """The distribution pass alone (``ob_dr_cdf``): ``(sums, wsum)`` with sums (m) = sum c w L(x'beta_v) for the
    (m, k) ``betas``, m <= 128, L the clamped sigmoid, and wsum = sum c w. Arguments as ``dr_logit_pass``."""
    xf, wv, c8, b, n, k = _dr_args(x, w, counts, betas)
    sums, wsum = np.empty(len(b)), np.empty(1)
    with_context(lambda ctx: N.lib().ob_dr_cdf(ctx, N.dp(xf), max(n, 1), N.dp(wv), N.u8p(c8), n, k, N.dp(b), len(b),
                                              N.dp(sums), N.dp(wsum)), device)
    return sums, float(wsum[0])


def dr_thresholds(y, n_thresholds: int = 50, lo: float = 0.05, hi: float = 0.95) -> np.ndarray:
    """ob_dr_thresholds (host only): the sample quantiles of ``y`` at ``n_thresholds`` evenly spaced levels of
    [lo, hi], exact duplicates removed."""
    yv = np.ascontiguousarray(y, dtype=np.float64).ravel()
    out = np.empty(max(int(n_thresholds), 1))
    kept = C.c_int32()
    N.check(N.lib().ob_dr_thresholds(N.dp(yv), len(yv), int(n_thresholds), float(lo), float(hi), N.dp(out), C.byref(kept)))
    return out[:kept.value].copy()


def dr_quantiles(f, thresholds, taus):
    """ob_dr_quantiles (host only): rearranges the distribution ``f`` on the threshold grid and inverts it at
    ``taus`` -> (quantiles, rearranged f, edge codes: 0, 1 below the grid, 2 above it)."""
    fv = np.ascontiguousarray(f, dtype=np.float64)
    thr = np.ascontiguousarray(thresholds, dtype=np.float64)
    tv = np.ascontiguousarray(np.atleast_1d(taus), dtype=np.float64)
    if fv.ndim != 1 or fv.shape != thr.shape or tv.ndim != 1:
        raise ValueError("f and thresholds must be 1-D of one length and taus 1-D")
    q, re, edge = np.empty(len(tv)), np.empty(len(fv)), np.zeros(len(tv), dtype=np.uint8)
    N.check(N.lib().ob_dr_quantiles(N.dp(fv), N.dp(thr), len(fv), N.dp(tv), len(tv), N.dp(q), N.dp(re),
                                    N.u8p(edge)))
    return q, re, edge


def dr_check_shape(k: int, n_a: int, n_b: int, n_thresholds: int, n_quantiles: int) -> None:
    """ob_dr_check_shape: raises OaxacaError where a distribution-regression decomposition would (host only)."""
    N.check(N.lib().ob_dr_check_shape(int(k), int(n_a), int(n_b), int(n_thresholds), int(n_quantiles)))


def dr_row_len(n_thresholds: int, n_quantiles: int) -> int:
    """ob_dr_row_len: 6 n_q + 7 T + 1 doubles per replicate of a distribution-regression decomposition."""
    return int(N.lib().ob_dr_row_len(int(n_thresholds), int(n_quantiles)))


def dr_last_timing() -> dict:
    """ob_dr_last_timing: Newton passes and HIP-event ms (logit passes, distribution pass, rows) of this thread's
    last distribution-regression boot."""
    return _last_timing("ob_dr_last_timing", N.ob_dr_timing)


def density_pass(x, y, grid, bandwidth: float, gammas=None, w=None, counts=None, device: int | None = None):
    """The density pass of ``decompose_density`` alone (``ob_density_pass``) over one group's rows. ``x``: (n, k) with
    the intercept (all ones) as column 0, ``k <= 32``; ``y``: n outcomes; ``grid``: 2 to 256 finite points;
    ``gammas``: (m, k) logit coefficients, ``m <= 64``, or ``None`` (psi = 1, m = 1); ``w``: n weights (``None``: 1);
    ``counts``: n resample counts below 256 (``None``: every row once). With v = w psi, psi = p / (1 - p) of the
    clamped sigmoid of x'gamma, returns ``(num, den, den2)``: (m, G) sums c v phi((g_j - y) / h), (m) sums c v and
    (m) sums c v^2."""
    xf, n, k = _design(x)
    yv = _per_row(y, n, "y must have one entry per row of x")
    wv = _per_row(w, n, "w must have one entry per row of x", optional=True)
    g = None if gammas is None else _coefficient_rows(gammas, k, "gammas must be (m, k)")
    gr = np.ascontiguousarray(grid, dtype=np.float64)
    if gr.ndim != 1:
        raise ValueError("grid must be a 1-D sequence")
    m = 1 if g is None else len(g)
    num, den, den2 = np.empty((m, len(gr))), np.empty(m), np.empty(m)
    with_context(lambda ctx: N.lib().ob_density_pass(ctx, N.dp(xf), max(n, 1), N.dp(yv), N.dp(wv),
                                                    N.u8p(_counts_u8(counts, n)), n, k, N.dp(g), m, N.dp(gr), len(gr),
                                                    float(bandwidth), N.dp(num), N.dp(den), N.dp(den2)), device)
    return num, den, den2


def density_grid(y, grid_size: int = 100) -> np.ndarray:
    """ob_density_grid (host only): the default grid, g_j = min + j (max - min) / grid_size (dfl.rs:164-172)."""
    yv = np.ascontiguousarray(y, dtype=np.float64)
    out = np.empty(max(int(grid_size) or 100, 0))
    N.check(N.lib().ob_density_grid(N.dp(yv), len(yv), int(grid_size), N.dp(out)))
    return out


def density_check_shape(k: int, n_a: int, n_b: int, grid_size: int) -> None:
    """ob_density_check_shape: raises OaxacaError where a density decomposition would (host only)."""
    N.check(N.lib().ob_density_check_shape(int(k), int(n_a), int(n_b), int(grid_size)))


def density_row_len(k: int, grid_size: int) -> int:
    """ob_density_row_len: 6 G + k + 2 doubles per replicate of a density decomposition (0 outside the limits)."""
    return int(N.lib().ob_density_row_len(int(k), int(grid_size)))


def density_last_timing() -> dict:
    """ob_density_last_timing: logit passes and HIP-event ms (logit passes, the density pass, the rows) of this
    thread's last density boot."""
    return _last_timing("ob_density_last_timing", N.ob_density_timing)


def nopo_sums(y, cell, n_cells: int, w=None, counts=None, device: int | None = None):
    """The cell pass of the matching decomposition alone (``ob_nopo_sums``) over one group of rows in ascending
    order of ``cell`` (ids in [0, n_cells)). ``w``: weights or ``None`` for 1; ``counts``: (n_reps, n) resample
    counts below 256 (``None``: the point pass, one replicate). Returns (N, S), each (n_reps, n_cells): sum c w and
    sum c (w y) per cell."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    if y.ndim != 1:
        raise ValueError("y must be one-dimensional")
    n = len(y)
    what = "cell and w must have one entry per entry of y"
    wv = _per_row(w, n, what, optional=True)
    cv = np.ascontiguousarray(cell, dtype=np.int32)
    if cv.shape != (n,):
        raise ValueError(what)
    c8 = _counts_u8(counts, n, by_rep=True)
    reps = 1 if c8 is None else len(c8)
    ns, ss = np.empty((reps, max(int(n_cells), 0))), np.empty((reps, max(int(n_cells), 0)))
    with_context(lambda ctx: N.lib().ob_nopo_sums(ctx, N.dp(y), N.dp(wv), N.i32p(cv), n, int(n_cells), N.u8p(c8), reps,
                                                 N.dp(ns), N.dp(ss)), device)
    return ns, ss


def nopo_check_shape(n_cells: int, n_a: int, n_b: int) -> None:
    """ob_nopo_check_shape: raises OaxacaError where a matching decomposition would (host only)."""
    N.check(N.lib().ob_nopo_check_shape(int(n_cells), int(n_a), int(n_b)))


def nopo_row_len() -> int:
    """ob_nopo_row_len: 13 doubles per replicate of a matching decomposition."""
    return int(N.lib().ob_nopo_row_len())


def nopo_last_timing() -> dict:
    """ob_nopo_last_timing: HIP-event ms of the cell pass, the rows and the resample of this thread's last matching
    decomposition boot (or prepare, or ``nopo_sums``)."""
    return _last_timing("ob_nopo_last_timing", N.ob_nopo_timing)


def knn(queries, controls, k: int, device: int | None = None):
    """The min(k, n_c) nearest controls of each query (``ob_knn``): squared Euclidean distance summed
    in covariate order without FMA, ties by control position. ``queries``: (n_q, d), ``controls``:
    (n_c, d). Returns (idx int64 (n_q, k), dist2 (n_q, k)), ascending, -1 / +inf past min(k, n_c)."""
    q = np.asfortranarray(queries, dtype=np.float64)
    c = np.asfortranarray(controls, dtype=np.float64)
    if q.ndim != 2 or c.ndim != 2 or q.shape[1] != c.shape[1]:
        raise ValueError("queries and controls must be (n, d) with the same d")
    (n_q, d), n_c, k = q.shape, c.shape[0], int(k)
    idx, dist2 = np.empty((n_q, max(k, 0)), dtype=np.int64), np.empty((n_q, max(k, 0)))
    N.check(N.lib().ob_knn(N.context(device), N.dp(q), max(n_q, 1), n_q, N.dp(c), max(n_c, 1), n_c, d, k,
                           N.i64p(idx), N.dp(dist2)))
    return idx, dist2


def match_logistic(x, y, max_iter: int = 100, tol: float = 1e-6, device: int | None = None):
    """matching/logistic.rs:31-113 with the Newton passes on the GPU (``ob_match_logistic``): no
    probability clamp, a 1e-6 ridge, an LU solve. ``x``: (n, k) with the intercept column included.
    Returns (coefficients, scores at the final coefficients, converged, iterations)."""
    xf, n, k = _design(x)
    y = _per_row(y, n, "y must have one entry per row of x")
    beta, probs = np.empty(k), np.empty(n)
    conv, iters = C.c_int32(0), C.c_int32(0)
    N.check(N.lib().ob_match_logistic(N.context(device), N.dp(xf), max(n, 1), N.dp(y), n, k, int(max_iter), float(tol),
                                      N.dp(beta), N.dp(probs), C.byref(conv), C.byref(iters)))
    return beta, probs, bool(conv.value), int(iters.value)


def kde(data, grid, bandwidth: float, weights=None, device: int | None = None):
    """math/kde.rs:20-41 on the GPU (``ob_kde``): the weighted Gaussian kernel density of ``data``
    at the ``grid`` points."""
    data = np.ascontiguousarray(data, dtype=np.float64)
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    if w is not None and w.shape != data.shape:
        raise ValueError("weights must match data")
    out = np.empty(len(grid))
    N.check(N.lib().ob_kde(N.context(device), N.dp(data), N.dp(w), len(data), N.dp(grid), len(grid), float(bandwidth),
                           N.dp(out)))
    return out


def silverman_bandwidth(data) -> float:
    """math/kde.rs:44-59 via the native host routine (not the RIF bandwidth of math/rif.rs)."""
    data = np.ascontiguousarray(data, dtype=np.float64)
    out = C.c_double()
    N.check(N.lib().ob_silverman_bandwidth(N.dp(data), len(data), C.byref(out)))
    return out.value


def akm_connected_set(dataframe, worker_col: str, firm_col: str) -> dict:
    """akm.rs:151-303 on the host (``ob_akm_connected_set``, no GPU needed): the largest connected set
    of the worker-firm graph by node count; among equally large components the one holding the
    smallest sorted worker id. Returns ``keep`` (bool per row), ``worker_idx`` / ``firm_idx`` (int32
    per kept row, dense over the kept ids in sorted string order), ``worker_ids`` / ``firm_ids`` (the
    sorted id strings) and ``n_components``."""
    from .frame import Frame

    lib = N.lib()
    frame = dataframe if isinstance(dataframe, Frame) else Frame(dataframe)
    cols, ncol, nrow = frame.as_c()
    h = C.c_void_p()
    N.check(lib.ob_akm_connected_set(cols, ncol, nrow, worker_col.encode(), firm_col.encode(), C.byref(h)))
    try:
        n, kept, nw, nf, comps = (C.c_int64() for _ in range(5))
        keep = C.POINTER(C.c_uint8)()
        wi, fi = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        N.check(lib.ob_akm_set_get(h, C.byref(n), C.byref(keep), C.byref(kept), C.byref(wi), C.byref(fi),
                                   C.byref(nw), C.byref(nf), C.byref(comps)))
        return {"keep": N.array_copy(keep, (n.value,)).astype(bool), "worker_idx": N.array_copy(wi, (kept.value,)),
                "firm_idx": N.array_copy(fi, (kept.value,)),
                "worker_ids": [lib.ob_akm_set_id(h, 0, i).decode() for i in range(nw.value)],
                "firm_ids": [lib.ob_akm_set_id(h, 1, i).decode() for i in range(nf.value)],
                "n_components": int(comps.value)}
    finally:
        lib.ob_akm_set_free(h)


def akm_demean(v, worker_idx, firm_idx, n_workers: int, n_firms: int, tol: float = 1e-8, max_iters: int = 1000,
               device: int | None = None):
    """akm.rs:452-527 for a batch of columns on the GPU (``ob_akm_demean``). ``v``: (n,) or (n, c); a
    Fortran-ordered view with a longer leading dimension is passed as it is. Returns (demeaned,
    iterations int32 (c,), converged bool (c,)); a column is the same bytes alone or in a batch."""
    v = np.asarray(v, dtype=np.float64)
    one = v.ndim == 1
    v2 = v.reshape(-1, 1) if one else v
    if v2.ndim != 2:
        raise ValueError("v must be (n,) or (n, c)")
    n, c = v2.shape
    if not (v2.strides[0] == 8 and v2.strides[1] % 8 == 0 and v2.strides[1] >= 8 * max(n, 1)):
        v2 = np.asfortranarray(v2)
    ldv = v2.strides[1] // 8 if c > 1 and n > 0 else max(n, 1)
    wi = np.ascontiguousarray(worker_idx, dtype=np.int32)
    fi = np.ascontiguousarray(firm_idx, dtype=np.int32)
    if wi.shape != (n,) or fi.shape != (n,):
        raise ValueError("one worker and one firm index per row")
    out = np.full((c, ldv), np.nan).T[:n]  # the same leading dimension; the padding is never written
    iters, conv = np.zeros(c, np.int32), np.zeros(c, np.int32)
    N.check(N.lib().ob_akm_demean(N.context(device), N.dp(v2), ldv, n, c, N.i32p(wi), N.i32p(fi), int(n_workers),
                                  int(n_firms), float(tol), int(max_iters), N.dp(out), N.i32p(iters), N.i32p(conv)))
    return (out[:, 0] if one else out), iters, conv.astype(bool)


def akm_recover_fe(r, worker_idx, firm_idx, n_workers: int, n_firms: int, tol: float = 1e-8, max_iters: int = 1000,
                   device: int | None = None):
    """akm.rs:530-621 on the GPU (``ob_akm_recover_fe``), the psi[0] normalisation included. Returns
    (alpha, psi, iterations, converged)."""
    r = np.ascontiguousarray(r, dtype=np.float64)
    n = len(r)
    wi = np.ascontiguousarray(worker_idx, dtype=np.int32)
    fi = np.ascontiguousarray(firm_idx, dtype=np.int32)
    if wi.shape != (n,) or fi.shape != (n,):
        raise ValueError("one worker and one firm index per row")
    alpha, psi = np.zeros(int(n_workers)), np.zeros(int(n_firms))
    iters, conv = C.c_int32(0), C.c_int32(0)
    N.check(N.lib().ob_akm_recover_fe(N.context(device), N.dp(r), n, N.i32p(wi), N.i32p(fi), int(n_workers), int(n_firms),
                                      float(tol), int(max_iters), N.dp(alpha), N.dp(psi), C.byref(iters), C.byref(conv)))
    return alpha, psi, int(iters.value), bool(conv.value)


def _vif_x(x):
    """(n, K) predictors as the C ABI takes them: column-major, a Fortran-ordered view with a longer
    leading dimension passed as it is. Returns (array, ldx, n, K)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("x must be (n, K)")
    n, k = x.shape
    if not (x.strides[0] == 8 and x.strides[1] % 8 == 0 and x.strides[1] >= 8 * max(n, 1)):
        x = np.asfortranarray(x)
    ldx = x.strides[1] // 8 if k > 1 and n > 0 else max(n, 1)
    return x, ldx, n, k


def vif_gram(x, device: int | None = None):
    """The extended Gram of the VIF fits on the GPU (``ob_vif_gram``): G = Xe'Xe for Xe = [x, 1],
    (K + 1, K + 1) with both triangles filled; row and column K are the intercept's."""
    x, ldx, n, k = _vif_x(x)
    g = np.empty((k + 1, k + 1), order="F")
    N.check(N.lib().ob_vif_gram(N.context(device), N.dp(x), ldx, n, k, N.dp(g)))
    return g


def vif_solve(gram, n: int):
    """The K auxiliary fits of math/diagnostics.rs:43-66 from one Gram, on the host (``ob_vif_solve``,
    no GPU needed): each x_j on [the others in order, the intercept last] by nalgebra's Cholesky.
    Returns the (K + 1, K) coefficients at the positions of Xe, with B[j, j] = 0."""
    g = np.asfortranarray(gram, dtype=np.float64)
    if g.ndim != 2 or g.shape[0] != g.shape[1] or g.shape[0] < 1:
        raise ValueError("gram must be (K + 1, K + 1)")
    k = g.shape[0] - 1
    b = np.empty((k + 1, max(k, 0)), order="F")
    N.check(N.lib().ob_vif_solve(N.dp(g), int(n), k, N.dp(b)))
    return b


def vif_sums(x, coef, means, device: int | None = None):
    """Every fit's sums of squares in one pass over the rows on the GPU (``ob_vif_sums``): ss_res[j] =
    sum_i (x_ij - xe_i . coef[:, j])^2 from explicit residuals and ss_tot[j] = sum_i (x_ij -
    means[j])^2. Returns (ss_res, ss_tot)."""
    x, ldx, n, k = _vif_x(x)
    b = np.asfortranarray(coef, dtype=np.float64)
    m = np.ascontiguousarray(means, dtype=np.float64)
    if b.shape != (k + 1, k) or m.shape != (k,):
        raise ValueError("coef must be (K + 1, K) and means (K,)")
    ss_res, ss_tot = np.empty(k), np.empty(k)
    N.check(N.lib().ob_vif_sums(N.context(device), N.dp(x), ldx, n, k, N.dp(b), N.dp(m), N.dp(ss_res), N.dp(ss_tot)))
    return ss_res, ss_tot


def vif(x, device: int | None = None):
    """math/diagnostics.rs:29-109 on the GPU (``ob_vif``): the variance inflation factor of every
    column of the (n, K) array ``x``, +inf where the reference gives it. A Cholesky failure of any
    auxiliary fit raises OB_E_LINALG for the whole call, as in the reference."""
    x, ldx, n, k = _vif_x(x)
    out = np.empty(k)
    N.check(N.lib().ob_vif(N.context(device), N.dp(x), ldx, n, k, N.dp(out)))
    return out


def vif_last_timing() -> dict:
    """``ob_vif_last_timing``: this thread's last ``vif`` / ``calculate_vif`` call, in ms: the Gram pass
    and the residual pass by HIP events, the K solves by the host clock."""
    g, s, r = C.c_double(), C.c_double(), C.c_double()
    N.check(N.lib().ob_vif_last_timing(C.byref(g), C.byref(s), C.byref(r)))
    return {"gram_ms": g.value, "solve_ms": s.value, "sums_ms": r.value}


def normal_inverse_cdf(p: float) -> float:
    """statrs ``Normal::new(0, 1).inverse_cdf(p)`` term by term (``ob_normal_inverse_cdf``, host only): the
    z of the remediation's prediction intervals. NaN outside [0, 1]."""
    return float(N.lib().ob_normal_inverse_cdf(float(p)))


def remedy_solve(gram_a, gram_fit=None):
    """The fair-wage model of analysis.rs:434-500 from Grams, on the host (``ob_remedy_solve``, no GPU
    needed). ``gram_a`` is ``vif_gram(np.column_stack([features, y]))`` over the reference group's rows,
    ``gram_fit`` the same over the rows the model is fit on (None: the reference group; for the pooled
    target, both groups stacked). Returns (beta, cov) in the design's order, the intercept first: beta by
    nalgebra's Cholesky of the fit rows' normal equations, cov = (X_A'X_A)^-1 of the reference group."""
    ga = np.asfortranarray(gram_a, dtype=np.float64)
    if ga.ndim != 2 or ga.shape[0] != ga.shape[1] or ga.shape[0] < 2:
        raise ValueError("gram_a must be (K + 1, K + 1)")
    k = ga.shape[0] - 1
    gf = None
    if gram_fit is not None:
        gf = np.asfortranarray(gram_fit, dtype=np.float64)
        if gf.shape != ga.shape:
            raise ValueError("gram_fit must have gram_a's shape")
    beta, cov = np.empty(k), np.empty((k, k), order="F")
    N.check(N.lib().ob_remedy_solve(N.dp(ga), N.dp(gf), k, N.dp(beta), N.dp(cov)))
    return beta, cov


def remedy_score(x, beta, cov, y=None, contributions: bool = False, device: int | None = None):
    """One pass over the rows on the GPU (``ob_remedy_score``): for the (n, K - 1) features ``x`` and the
    design xe = [1, x], fair = xe . beta, leverage = xe' cov xe, and rss = sum (y_i - fair_i)^2 over the
    first len(y) rows from explicit residuals (0.0 without ``y``). Returns (fair, leverage, rss), and the
    (n, K) contributions xe_ij beta_j as a fourth item when asked for."""
    x, ldx, n, p = _vif_x(x)
    k = p + 1
    b = np.ascontiguousarray(beta, dtype=np.float64)
    c = np.asfortranarray(cov, dtype=np.float64)
    if b.shape != (k,) or c.shape != (k, k):
        raise ValueError("beta must be (K,) and cov (K, K) for K - 1 feature columns")
    yv = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    n_rss = 0 if yv is None else int(yv.shape[0])
    if yv is not None and (yv.ndim != 1 or n_rss > n):
        raise ValueError("y must be 1-D with at most n entries")
    fair, lev, rss = np.empty(n), np.empty(n), C.c_double(0.0)
    con = np.empty((n, k), order="F") if contributions else None
    N.check(N.lib().ob_remedy_score(N.context(device), N.dp(x), ldx, N.dp(yv), n, n_rss, k, N.dp(b), N.dp(c), N.dp(fair),
                                    N.dp(lev), C.byref(rss), N.dp(con)))
    return (fair, lev, rss.value, con) if contributions else (fair, lev, rss.value)


def remedy_allocate(y, fair, leverage, n_a: int, sigma_squared: float, budget: float = 0.0, strategy: str = "greedy",
                    min_gap_pct: float = 0.0, forensic_mode: bool = False, adjust_both_groups: bool = False,
                    confidence_level: float = 0.95, range_target: str = "midpoint", index=None,
                    device: int | None = None) -> dict:
    """analysis.rs:516-857 on the GPU (``ob_remedy_allocate``) over stacked rows, the reference group's
    ``n_a`` first and the target group's after them: prediction intervals, classification, the stable
    descending order of the gaps and the greedy or equitable allocation. ``index`` gives each stacked
    row's original index (default: its stacked position). Returns a dict of arrays with one entry per
    adjustment, ordered by index (index, adjustment, current_wage, new_wage, fair_wage, lower, upper,
    group with 0 = reference and 1 = target, row), and the scalars of ``ob_remedy_info``."""
    yv, fv, hv = (np.ascontiguousarray(a, dtype=np.float64) for a in (y, fair, leverage))
    n = yv.shape[0]
    if yv.ndim != 1 or fv.shape != (n,) or hv.shape != (n,) or not 0 <= int(n_a) <= n:
        raise ValueError("y, fair and leverage must be 1-D of one length, with 0 <= n_a <= n")
    iv = None
    if index is not None:
        iv = np.ascontiguousarray(index, dtype=np.int64)
        if iv.shape != (n,):
            raise ValueError("index must have one entry per row")
    rq = N.ob_remedy_request(float(budget), float(min_gap_pct), float(confidence_level),
                             N.OB_REMEDY_STRATEGIES[strategy], N.OB_REMEDY_RANGE_TARGETS[range_target],
                             int(bool(forensic_mode)), int(bool(adjust_both_groups)))
    lib = N.lib()
    h = C.c_void_p()
    N.check(lib.ob_remedy_allocate(N.context(device), N.dp(yv), N.dp(fv), N.dp(hv), int(n_a), n - int(n_a),
                                   N.i64p(iv), float(sigma_squared), C.byref(rq), C.byref(h)))
    try:
        info = N.ob_remedy_info()
        N.check(lib.ob_remedy_results_info(h, C.byref(info)))
        m = int(info.n_adjustments)
        pi, pr = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)()
        pg = C.POINTER(C.c_int32)()
        pd = [C.POINTER(C.c_double)() for _ in range(6)]
        N.check(lib.ob_remedy_results_get(h, C.byref(pi), *[C.byref(p) for p in pd], C.byref(pg), C.byref(pr)))
        out = {"index": N.array_copy(pi, (m,)), "group": N.array_copy(pg, (m,)), "row": N.array_copy(pr, (m,))}
        for name, p in zip(("adjustment", "current_wage", "new_wage", "fair_wage", "lower", "upper"), pd):
            out[name] = N.array_copy(p, (m,))
        return {**out, **N.struct_dict(info)}
    finally:
        lib.ob_remedy_results_free(h)


def remedy_defend_rows(y, fair, leverage, n_a: int, sigma_squared: float, rows, values, confidence_level: float = 0.95,
                       device: int | None = None) -> dict:
    """engine/src/defensibility.rs:199-365 on the GPU (``ob_remedy_defend_rows``) over stacked rows, the
    reference group's ``n_a`` first: ``rows`` and ``values`` are the proposed adjustments as (stacked row,
    raise) in request order. Returns, per adjustment and in that order, row, adjustment, current_wage,
    new_wage (one add), fair_wage, lower, upper and is_defensible (``new_wage >= lower - 1.0``), and the
    scalars of ``ob_defend_info``; ``sums`` holds the seven group sums behind the gaps. Where several
    adjustments name one row, the first decides that row's new wage in the sums."""
    yv, fv, hv = (np.ascontiguousarray(a, dtype=np.float64) for a in (y, fair, leverage))
    n = yv.shape[0]
    if yv.ndim != 1 or fv.shape != (n,) or hv.shape != (n,) or not 0 <= int(n_a) <= n:
        raise ValueError("y, fair and leverage must be 1-D of one length, with 0 <= n_a <= n")
    rv = np.ascontiguousarray(rows, dtype=np.int64)
    vv = np.ascontiguousarray(values, dtype=np.float64)
    if rv.ndim != 1 or vv.shape != rv.shape:
        raise ValueError("rows and values must be 1-D of one length")
    m = int(rv.shape[0])
    lib = N.lib()
    h = C.c_void_p()
    N.check(lib.ob_remedy_defend_rows(N.context(device), N.dp(yv), N.dp(fv), N.dp(hv), int(n_a), n - int(n_a), N.i64p(rv),
                                      N.dp(vv), m, float(sigma_squared), float(confidence_level), C.byref(h)))
    try:
        info = N.ob_defend_info()
        N.check(lib.ob_remedy_results_defend_info(h, C.byref(info)))
        pr, pf = C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)()
        pd = [C.POINTER(C.c_double)() for _ in range(6)]
        N.check(lib.ob_remedy_results_get(h, None, *[C.byref(p) for p in pd], None, C.byref(pr)))
        N.check(lib.ob_remedy_results_defensible(h, C.byref(pf)))
        out = {"row": N.array_copy(pr, (m,)), "is_defensible": N.array_copy(pf, (m,)).astype(bool)}
        for name, p in zip(("adjustment", "current_wage", "new_wage", "fair_wage", "lower", "upper"), pd):
            out[name] = N.array_copy(p, (m,))
        return {**out, **N.struct_dict(info), "sums": np.array(info.sums)}
    finally:
        lib.ob_remedy_results_free(h)


def remedy_resolve_overrides(index, overrides, predictors, n_rows: int) -> list:
    """engine/src/defensibility.rs:32-73 on the host (``ob_remedy_resolve_overrides``, no GPU needed).
    ``index``: each adjustment's original row index; ``overrides``: ``(adjustment position, column name,
    value)`` triples. Per index the last adjustment that carries overrides replaces every earlier set as a
    whole; names outside ``predictors`` and indices past ``n_rows`` have no effect. Returns the cells to
    change as ``(row, predictor name, value)``, predictor by predictor and by ascending row."""
    iv = np.ascontiguousarray(index, dtype=np.int64)
    ov = list(overrides)
    pos = np.array([o[0] for o in ov], dtype=np.int64)
    val = np.array([o[2] for o in ov], dtype=np.float64)
    names, keep_names = N.strs([str(o[1]) for o in ov])
    preds = [str(p) for p in predictors]
    pn, keep_preds = N.strs(preds)
    cap = max(len(ov), 1)
    orow, opred, oval, n_out = np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.zeros(cap), C.c_int64(0)
    N.check(N.lib().ob_remedy_resolve_overrides(N.i64p(iv), int(iv.shape[0]), N.i64p(pos), names, N.dp(val), len(ov),
                                                pn, len(preds), int(n_rows), N.i64p(orow), N.i32p(opred), N.dp(oval),
                                                C.byref(n_out)))
    del keep_names, keep_preds  # held until the call has returned
    return [(int(orow[i]), preds[opred[i]], float(oval[i])) for i in range(n_out.value)]


def remedy_apply_adjustments(wage, index, value, valid=None):
    """engine/src/analysis.rs:76-88 on the host (``ob_remedy_apply_adjustments``, no GPU needed): a copy
    of ``wage`` with ``wage[index[j]] += value[j]`` applied one by one in request order. ``valid`` marks
    the non-null wages; no raise touches a null. An index outside the frame raises ``OB_E_INVALID`` with
    the reference's text."""
    wv = np.ascontiguousarray(wage, dtype=np.float64)
    iv = np.ascontiguousarray(index, dtype=np.int64)
    vv = np.ascontiguousarray(value, dtype=np.float64)
    if wv.ndim != 1 or iv.ndim != 1 or vv.shape != iv.shape:
        raise ValueError("wage must be 1-D, index and value 1-D of one length")
    ok = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    out = np.empty_like(wv)
    N.check(N.lib().ob_remedy_apply_adjustments(N.dp(wv), N.u8p(ok),
                                                int(wv.shape[0]), N.i64p(iv), N.dp(vv), int(iv.shape[0]), N.dp(out)))
    return out


# ---- cluster bootstrap ------------------------------------------------------
def cluster_check_shape(n_clusters: int, k1: int) -> None:
    """ob_cluster_check_shape: raises OaxacaError where a clustered prepare would (host only)."""
    N.check(N.lib().ob_cluster_check_shape(int(n_clusters), int(k1)))


def cluster_index(ids, group, stratified: bool = False) -> dict:
    """ob_cluster_index (host only). ``ids``: one column (strings or integers, ``None`` = null);
    ``group``: per row 0 (A), 1 (B) or anything else for a row in neither group. Returns dense ids in
    order of first appearance (-1: dropped), each group's stable permutation by cluster id with its
    CSR offsets, and n_clusters / n_clusters_a / n_clusters_b / max_cluster_rows / stratified."""
    from .frame import Frame

    fr = Frame({"ids": ids})
    cols, _, n = fr.as_c()
    grp = np.ascontiguousarray(group, dtype=np.int32)
    if grp.shape != (n,):
        raise ValueError("group must have one entry per row")
    dense = np.full(n, -1, dtype=np.int32)
    perm = [np.zeros(max(n, 1), dtype=np.int64) for _ in range(2)]
    off = [np.zeros(n + 1, dtype=np.int64) for _ in range(2)]
    info = N.ob_cluster_info()
    N.check(N.lib().ob_cluster_index(cols, N.i32p(grp), n, int(bool(stratified)), N.i32p(dense), N.i64p(perm[0]), N.i64p(perm[1]),
                                     N.i64p(off[0]), N.i64p(off[1]), C.byref(info)))
    nc = int(info.n_clusters)
    kept = [int(((grp == g) & (dense >= 0)).sum()) for g in (0, 1)]
    return {"dense": dense, "perm_a": perm[0][:kept[0]].copy(), "perm_b": perm[1][:kept[1]].copy(),
            "off_a": off[0][:nc + 1].copy(), "off_b": off[1][:nc + 1].copy(), "n_clusters": nc,
            "n_clusters_a": int(info.n_clusters_a), "n_clusters_b": int(info.n_clusters_b),
            "max_cluster_rows": int(info.max_cluster_rows), "stratified": bool(info.stratified)}


def cluster_gram(x, y, w, perm, off, device=None):
    """ob_cluster_gram for one group: x (n, p) predictors without the intercept, y (n,), w (n,) or None,
    perm / off from ``cluster_index`` -> (Q (C, E) in ob_spec.h's pair order, rows (C,))."""
    x = np.asfortranarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    perm = np.ascontiguousarray(perm, dtype=np.int64)
    off = np.ascontiguousarray(off, dtype=np.int64)
    n, p = x.shape
    if y.shape != (n,) or perm.shape != (n,) or (w is not None and w.shape != (n,)) or off.ndim != 1 or off.size < 2:
        raise ValueError("cluster_gram: mismatched shapes")
    nc = off.size - 1
    e = (p + 2) * (p + 3) // 2
    e_pad = (e + 15) // 16 * 16
    q = np.zeros((nc, e_pad))
    rows = np.zeros(nc, dtype=np.uint32)
    N.check(N.lib().ob_cluster_gram(N.context(device), N.dp(x), n, max(n, 1), p, N.dp(y), N.dp(w),
                                    N.i64p(perm), N.i64p(off), nc, N.dp(q), N.u32p(rows)))
    return q[:, :e].copy(), rows


def cluster_counts(seed: int, first_rep: int, n_reps: int, n_clusters_a: int, n_clusters_b: int = 0,
                   stratified: bool = False, device=None):
    """ob_cluster_counts -> (n_reps, C) uint32 counts of the OBRC-1 stream (C = n_clusters_a + n_clusters_b)."""
    nc = int(n_clusters_a) + int(n_clusters_b)
    out = np.zeros((n_reps, max(nc, 0)), dtype=np.uint32)
    N.check(N.lib().ob_cluster_counts(N.context(device), int(seed) & (2 ** 64 - 1), int(first_rep), int(n_reps),
                                      int(n_clusters_a), int(n_clusters_b), int(bool(stratified)),
                                      N.u32p(out)))
    return out


def cluster_apply(counts, q, device=None):
    """ob_cluster_apply: counts (R, C) uint32 x q (C, W) -> (R, W) on the f64 matrix units (W is padded to a
    multiple of 16 on the way in)."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    q = np.ascontiguousarray(q, dtype=np.float64)
    if counts.ndim != 2 or q.ndim != 2 or counts.shape[1] != q.shape[0]:
        raise ValueError("cluster_apply: counts (R, C) and q (C, W)")
    w = q.shape[1]
    w_pad = max((w + 15) // 16 * 16, 16)
    qp = np.zeros((q.shape[0], w_pad))
    qp[:, :w] = q
    out = np.zeros((counts.shape[0], w_pad))
    N.check(N.lib().ob_cluster_apply(N.context(device), N.u32p(counts), counts.shape[0],
                                     counts.shape[1], N.dp(qp), w_pad, N.dp(out)))
    return out[:, :w].copy()


def cluster_last_timing() -> dict:
    """ob_cluster_last_timing: gram / counts / apply / solve ms of this thread's last clustered host boot."""
    return _last_timing("ob_cluster_last_timing", N.ob_cluster_timing)


# ---- delete-one-cluster jackknife ---------------------------------------------
def cluster_jackknife_check_shape(k: int, n_clusters: int, n_norm: int = 0, n_y: int = 1, heckman: bool = False,
                                  want_rows: bool = False) -> None:
    """ob_cluster_jackknife_check_shape: raises OaxacaError where the cluster jackknife entry points would
    (host only). ``k``: design columns with the intercept."""
    N.check(N.lib().ob_cluster_jackknife_check_shape(int(k), int(n_clusters), int(n_norm), int(n_y), int(heckman),
                                                     int(want_rows)))


def cluster_jackknife_last_timing() -> float:
    """ob_cluster_jackknife_last_timing: HIP-event ms of this thread's last delete-one-cluster pass."""
    ms = C.c_double()
    N.check(N.lib().ob_cluster_jackknife_last_timing(C.byref(ms)))
    return ms.value


def _cluster_q(q_a, q_b, rows_a, rows_b):
    """The two groups' ``cluster_gram`` outputs interleaved into Q (C, 2, e_pad) and rows (C, 2)."""
    q_a, q_b = np.asarray(q_a, dtype=np.float64), np.asarray(q_b, dtype=np.float64)
    if q_a.ndim != 2 or q_a.shape != q_b.shape or len(rows_a) != len(q_a) or len(rows_b) != len(q_a):
        raise ValueError("cluster_jackknife: q_a / q_b (C, E) and rows_a / rows_b (C,) of the same clusters")
    e = q_a.shape[1]
    q = np.zeros((len(q_a), 2, (e + 15) // 16 * 16))
    q[:, 0, :e], q[:, 1, :e] = q_a, q_b
    rows = np.ascontiguousarray(np.stack([rows_a, rows_b], axis=1), dtype=np.uint32)
    return q, rows, e


def cluster_jackknife(q_a, q_b, rows_a, rows_b, tail, n_a: int, n_b: int, weighted: bool,
                      ref_mode=ReferenceCoefficients.GroupA, n_clusters_a=None, gram=None, device=None):
    """ob_cluster_jackknife: the delete-one-cluster pass on arrays. ``q_a`` / ``q_b`` (C, E) and ``rows_a`` /
    ``rows_b`` (C,) from ``cluster_gram`` per group over the same C clusters; ``tail``: the point estimate's beta_A,
    beta_B, xbar_A, xbar_B, beta* (5K values, a point-estimate row's columns after its 6 + 2K components); ``gram``
    (2, E): its extended Grams, by default the sum of Q over the clusters; ``n_clusters_a``: A's clusters (they come
    first) for the stratified strata, ``None`` for joint mode. -> api.JackknifeResult, counts per stratum."""
    from .api import _jackknife_out, _jackknife_result

    q, rows, e = _cluster_q(q_a, q_b, rows_a, rows_b)
    k1 = int(round((np.sqrt(8 * e + 1) - 1) / 2))
    if k1 * (k1 + 1) // 2 != e or k1 < 2:
        raise ValueError("cluster_jackknife: E is not (p + 2)(p + 3) / 2")
    g = q.sum(0) if gram is None else np.zeros((2, q.shape[2]))
    if gram is not None:
        g[:, :e] = np.asarray(gram, dtype=np.float64)
    tail = np.ascontiguousarray(tail, dtype=np.float64)
    if tail.size != 5 * (k1 - 1):
        raise ValueError("cluster_jackknife: tail holds 5 K values")
    o, bufs = _jackknife_out(k1 - 1)
    N.check(N.lib().ob_cluster_jackknife(N.context(device), N.dp(q), N.u32p(rows), len(q),
                                         len(q) if n_clusters_a is None else int(n_clusters_a),
                                         0 if n_clusters_a is None else 1, k1 - 2, int(bool(weighted)), int(n_a), int(n_b),
                                         N.dp(np.ascontiguousarray(g)), N.dp(tail), int(ref_mode), C.byref(o)))
    return _jackknife_result(o, bufs, None)


def cluster_jackknife_rows(panel, q_a, q_b, rows_a, rows_b, ref_mode=ReferenceCoefficients.GroupA, n_clusters_a=None,
                           deviations: bool = False):
    """ob_cluster_jackknife_rows on a resident ``Panel`` (its point estimate and solve kernel) and the two groups'
    ``cluster_gram`` outputs -> (theta (C, row_len), kept, n_dropped per stratum[, d (C, 6 + 2K)])."""
    q, rows, e = _cluster_q(q_a, q_b, rows_a, rows_b)
    lib = N.lib()
    nc, k = len(q), lib.ob_panel_k(panel._h)
    theta = np.empty((nc, lib.ob_panel_row_len(panel._h)), dtype=np.float64)
    kept = np.zeros(nc, dtype=np.uint8)
    dev = np.empty((nc, 6 + 2 * k), dtype=np.float64) if deviations else None
    nd = (C.c_int64 * 2)()
    N.check(lib.ob_cluster_jackknife_rows(panel._h, N.dp(q), N.u32p(rows), nc,
                                          nc if n_clusters_a is None else int(n_clusters_a),
                                          0 if n_clusters_a is None else 1, int(ref_mode), N.dp(theta),
                                          N.u8p(kept), nd, N.dp(dev)))
    out = (theta, kept.astype(bool), (int(nd[0]), int(nd[1])))
    return out + (dev,) if deviations else out
