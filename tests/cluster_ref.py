"""numpy restatement of the cluster bootstrap, for the tests.

OBRC-1 (csrc/ob_spec.h) is restated on the oracle's ``philox`` (pinned by the Random123 vectors of
tests/golden/reference_kat.json). A replicate is decomposed the way the reference would decompose a resampled
frame: the drawn clusters' rows are GATHERED, in draw order, into the two groups' matrices and handed to the
oracle's ``single_pass`` (OLS, beta*, the OB terms; a pass that fails there is a dropped replicate). Q is never
formed here.
"""
import numpy as np

TAG_OBC = 0x4F424331  # "OBC1"


def draws(O, seed, rep, s, m, base=0):
    """Stratum s of replicate rep: m uniform draws over m clusters, Lemire's multiply-and-reject."""
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    thresh = ((1 << 32) - m) % m
    calls, out = {}, []
    for j in range(m):
        t = 0
        while True:
            if (j >> 2, t) not in calls:
                calls[(j >> 2, t)] = O.philox((j >> 2, rep, 2 * t + s, TAG_OBC), key)
            p = calls[(j >> 2, t)][j & 3] * m
            if (p & 0xFFFFFFFF) >= thresh:
                out.append((p >> 32) + base)
                break
            t += 1
    return out


def indices(O, seed, rep, c_a, c_b=0, stratified=False):
    """The clusters replicate rep draws, in draw order (joint: c_a + c_b draws over all clusters)."""
    if not stratified:
        return draws(O, seed, rep, 0, c_a + c_b)
    return draws(O, seed, rep, 0, c_a) + draws(O, seed, rep, 1, c_b, base=c_a)


def counts(O, seed, first_rep, n_reps, c_a, c_b=0, stratified=False):
    out = np.zeros((n_reps, c_a + c_b), dtype=np.uint32)
    for r in range(n_reps):
        out[r] = np.bincount(indices(O, seed, first_rep + r, c_a, c_b, stratified), minlength=c_a + c_b)
    return out


def dense_ids(values, group, stratified=False):
    """values / group per frame row (group 0 = A, 1 = B, else neither; a None value drops the row) -> (dense ids
    with -1 for dropped rows, C_A, C_B, labels): first appearance, stratified: A's clusters first."""
    present = [v for v in values if v is not None]
    if present and any(isinstance(v, (float, np.floating)) for v in present):
        raise ValueError("float cluster column")
    first, in_g = {}, []
    for v, g in zip(values, group):
        if v is None or g not in (0, 1):
            continue
        if v not in first:
            first[v] = len(first)
            in_g.append(0)
        in_g[first[v]] |= 1 << g
    labels = list(first)
    order = list(range(len(labels)))
    if stratified:
        for c in order:
            if in_g[c] == 3:
                raise ValueError(f"cluster {labels[c]} has rows in both groups")
        order = [c for c in order if in_g[c] == 1] + [c for c in order if in_g[c] == 2]
    renum = {c: i for i, c in enumerate(order)}
    dense = np.array([renum[first[v]] if (v is not None and g in (0, 1)) else -1 for v, g in zip(values, group)])
    c_a = sum(1 for c in order if in_g[c] & 1)
    c_b = sum(1 for c in order if in_g[c] & 2)
    return dense, c_a, c_b, [labels[c] for c in order]


class ClusterRef:
    """OracleBuilder with a cluster column: prepared matrices, the cluster members per group, gathered replicates."""

    def __init__(self, O, frame, outcome, group, reference_group, cluster, stratified=False, **settings):
        self.O, self.stratified = O, stratified
        keep = [i for i, v in enumerate(frame[cluster]) if v is not None]  # a null drops the row (clean_dataframe)
        fr = {k: [v[i] for i in keep] for k, v in frame.items()}
        self.b = O.OracleBuilder(fr, outcome, group, reference_group).set(**settings)
        df, _, _, _ = self.b._stage()
        ia, ib, _ = self.b.split_groups(df)
        self.prep = self.b.prepared()
        grp = np.full(len(df[cluster]), -1)
        grp[ia], grp[ib] = 0, 1
        dense, self.c_a, self.c_b, self.labels = dense_ids(df[cluster], grp.tolist(), stratified)
        self.n_clusters = len(self.labels)
        self.members = []
        for rows in (ia, ib):  # positions within the group, frame order kept
            ids = dense[rows]
            self.members.append([np.flatnonzero(ids == c) for c in range(self.n_clusters)])
        self.seed = self.b.seed

    def _draws(self, rep):
        if self.stratified:
            return indices(self.O, self.seed, rep, self.c_a, self.c_b, True)
        return indices(self.O, self.seed, rep, self.n_clusters)

    def replicate(self, rep):
        p, k = self.prep, self.prep["cfg"].k
        idx = self._draws(rep)
        take = [np.concatenate([self.members[g][c] for c in idx]).astype(np.int64) for g in (0, 1)]
        if len(take[0]) <= k or len(take[1]) <= k:  # ols.rs:98-105: InsufficientData -> the replicate is dropped
            return np.full(p["cfg"].row_len, np.nan), 0
        wa = None if p["wa"] is None else p["wa"][take[0]]
        wb = None if p["wb"] is None else p["wb"][take[1]]
        rc, row = self.O.single_pass(p["cfg"], p["xa"][take[0]], p["ya"][take[0]], wa, p["xb"][take[1]],
                                     p["yb"][take[1]], wb)
        if rc != 0:
            return np.full(p["cfg"].row_len, np.nan), 0
        return row, 1

    def rows(self, first_rep, n_reps):
        out = [self.replicate(first_rep + r) for r in range(n_reps)]
        return np.array([o[0] for o in out]).reshape(n_reps, -1), np.array([o[1] for o in out], dtype=np.uint8)

    def run(self):
        point_row, resid = self.b.point(self.prep)
        rows, ok = self.rows(0, self.b.reps)
        return self.b.aggregate(self.prep, point_row, rows, ok, resid)
