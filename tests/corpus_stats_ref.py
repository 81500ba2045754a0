"""Reference of the device-side corpus statistics (gt_op_corpus_stats; gantts_amd.data.ResidentCorpus.minmax / .meanvar).

Reference (``reference``): the two-pass statistic in extended precision (np.longdouble) over the valid rows -- utterance ``idx`` cut to
``lengths[idx]`` -- per column: n, mean_ref, var_ref = sum (x - mean_ref)^2 / n, amax = max |x|, dmax = max |x - mean_ref|.

Bound (``bounds``), derived, with u = 2^-53 and n the number of valid rows, per column:
    |mean - mean_ref| <= n u amax                                   any summation order of exactly representable terms
    |var  - var_ref|  <= n u (4 (var_ref + dmax^2) + 4 amax dmax)   the summation, plus what the mean's own error injects through (x - mean)^2
Every summation order in double stays inside it (the host's data.meanvar, sklearn's _incremental_mean_and_var, a per-thread Welford with a
Chan tree); a float32 accumulator is outside it by four to six orders of magnitude.  A constant column must be exact: mean the constant,
variance 0.0.

``kernel_model`` restates the kernel's order of operations (corpus_stats_kernels.hip.h) in numpy with the mistakes the comparators have
to reject (``MISTAKES``).  The inputs (``FAMILIES``, ``make_corpus``) are shared with the GPU test: what the host is shown to satisfy
here is what the device is asked there.
"""
import numpy as np

U = 2.0 ** -53
FAMILIES = ("normal", "five", "large_offset", "constant")
SLAB, FANIN = 256, 64      # gantts_amd._lib.CORPUS_STATS_SLAB / _FANIN (asserted equal in the tests)
WIDTHS = (1, 3, 4, 5, 63, 187)      # 3, 1, 0, 3, 1, 1 pad columns; 63 and 187 are the real static and acoustic widths
# rows: one; around one slab; several workgroups with a ragged last one; more partials than the merge has chains
ROWS = (1, SLAB - 1, SLAB, SLAB + 1, 3 * SLAB + 100, (FANIN + 1) * SLAB + 77)


def make_lengths(F, rs, longest=70):
    """Utterance lengths from 1 to ``longest`` that add up to exactly ``F`` rows."""
    out, left = [], int(F)
    while left > 0:
        n = min(left, int(rs.randint(1, longest + 1)))
        out.append(n)
        left -= n
    return out


def make_corpus(family, F, D, seed=0):
    """``(utterances, cut)``: float32 ``(T_i, D)`` arrays adding up to F rows, and a cut length per utterance in [1, T_i].
    normal: N(0, 1);  five: 5 +- 0.3;  large_offset: 1e4 +- 1e-2;  constant: N(0, 1) with column 0 the float32 nearest 0.1."""
    rs = np.random.RandomState(1000 * FAMILIES.index(family) + seed)
    lens = make_lengths(F, rs)
    X = []
    for n in lens:
        g = rs.randn(n, D)
        if family == "five":
            g = 5.0 + 0.3 * g
        elif family == "large_offset":
            g = 1e4 + 1e-2 * g
        x = g.astype(np.float32)
        if family == "constant":
            x[:, 0] = np.float32(0.1)
        X.append(x)
    cut = [int(rs.randint(1, n + 1)) for n in lens]
    return X, cut


def valid_rows(X, lengths=None):
    return np.concatenate([np.asarray(x)[:(None if lengths is None else lengths[i])] for i, x in enumerate(X)], axis=0)


def reference(X, lengths=None):
    """dict of per-column n, mean, var (np.longdouble), amax, dmax over the valid rows."""
    v = valid_rows(X, lengths).astype(np.longdouble)
    n = len(v)
    mean = v.sum(0) / n
    d = v - mean
    return dict(n=n, mean=mean, var=(d * d).sum(0) / n, amax=np.abs(v).max(0), dmax=np.abs(d).max(0))


def bounds(ref):
    n = float(ref["n"])
    amax, dmax, var = ref["amax"].astype(np.float64), ref["dmax"].astype(np.float64), ref["var"].astype(np.float64)
    return n * U * amax, n * U * (4.0 * (var + dmax ** 2) + 4.0 * amax * dmax)


def errors(mean, var, ref):
    """(|mean - mean_ref| / bound, |var - var_ref| / bound) per column; 0 / 0 (an exact result under a zero bound) counts as 0."""
    bm, bv = bounds(ref)
    em = np.abs(np.asarray(mean, dtype=np.longdouble) - ref["mean"]).astype(np.float64)
    ev = np.abs(np.asarray(var, dtype=np.longdouble) - ref["var"]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(em == 0, 0.0, em / bm), np.where(ev == 0, 0.0, ev / bv)


def mismatches(mean, var, n, ref, D):
    """What of (mean, var, n) is outside the bound of ``ref``: a list of names, empty when all is inside."""
    mean, var = np.asarray(mean), np.asarray(var)
    bad = []
    if mean.shape != (D,) or mean.dtype != np.float64 or var.shape != (D,) or var.dtype != np.float64:
        return ["shape or dtype"]
    if n is not None and int(n) != ref["n"]:
        bad.append("n")
    rm, rv = errors(mean, var, ref)
    if not (rm <= 1.0).all():
        bad.append("mean")
    if not (rv <= 1.0).all():
        bad.append("var")
    return bad


def constant_mismatches(mean, var, column, value):
    """A constant column has to be exact."""
    return [k for k, ok in (("mean", mean[column] == np.float64(value)), ("var", var[column] == 0.0)) if not ok]


def minmax_mismatches(lo, hi, X, lengths=None):
    """(lo, hi) against numpy's own min / max of the valid rows: float32 (D,), equal by value (NaN where numpy has NaN)."""
    v = valid_rows(X, lengths)
    bad = []
    for name, got, want in (("min", lo, v.min(0)), ("max", hi, v.max(0))):
        got = np.asarray(got)
        if got.dtype != np.float32 or got.shape != want.shape or not np.array_equal(got, want, equal_nan=True):
            bad.append(name)
    return bad


# ---- numpy model of the kernel -------------------------------------------------------------------------------------------------------
MISTAKES = ("sample_variance", "lengths_ignored", "rows_past_a_cut_utterance", "pad_column_folded_in", "float32_accumulation",
            "chan_weight_dropped", "prior_ignored")


def _chan(a, b, mistake=None):
    (n, m, M2), (k, mb, M2b) = a, b
    if k == 0:
        return a
    if n == 0:
        return b
    if mistake == "float32_accumulation":      # the folds as well: a lane of a narrow corpus holds a row or two of a slab
        m, M2, mb, M2b = [np.asarray(v, np.float32) for v in (m, M2, mb, M2b)]
    tot = n + k
    w = k / tot
    with np.errstate(invalid="ignore"):
        d = mb - m
        return tot, m + d * w, M2 + M2b + d * d * (n if mistake == "chan_weight_dropped" else n * w)


def kernel_model(X, lengths=None, prior=None, mistake=None, slab=SLAB, fanin=FANIN, waves=4):
    """(lo, hi, mean, var, n) as the two launches compute them: the corpus on its pitch, a slab of rows per workgroup, a lane per
    float4 and row residue (Welford in double, one reciprocal per row), Chan folds in ascending order inside the workgroup, ``fanin``
    chains over the partials and a halving tree over the chains, then the prior continued by the total."""
    D = X[0].shape[1]
    ld = (D + 3) // 4 * 4
    lens = np.array([len(x) for x in X], dtype=np.int64)
    A = np.zeros((int(lens.sum()), ld), np.float32)
    A[:, :D] = np.concatenate(X)
    F = len(A)
    offsets = np.cumsum(lens) - lens
    cut = lens if (lengths is None or mistake == "lengths_ignored") else np.minimum(np.asarray(lengths, dtype=np.int64), lens)
    if mistake == "rows_past_a_cut_utterance":      # the cut utterances taken as lying back to back
        offsets = np.cumsum(cut) - cut
    valid = np.zeros(F, bool)
    for s, n in zip(offsets, cut):
        valid[s:s + n] = True
    if mistake == "pad_column_folded_in" and ld != D:      # columns taken from a dense index into the pitched rows
        A = np.concatenate([A.reshape(-1), np.zeros((-F * ld) % D, np.float32)]).reshape(-1, D)
        valid = np.ones(len(A), bool)
        F, ld = len(A), D
    acc = np.float32 if mistake == "float32_accumulation" else np.float64
    nv = ld // 4
    lpr = 1
    while lpr < min(nv, 64):
        lpr *= 2
    step = waves * (64 // lpr)
    parts = []
    for r0 in range(0, F, slab):
        rows = min(slab, F - r0)
        total = (0.0, np.zeros(ld), np.zeros(ld))
        lo, hi = np.full(ld, np.inf, np.float32), np.full(ld, -np.inf, np.float32)
        for fold in range(step):
            n, mean, m2 = acc(0), np.zeros(ld, acc), np.zeros(ld, acc)
            for r in range(fold, rows, step):
                if not valid[r0 + r]:
                    continue
                x = A[r0 + r].astype(acc)
                n = acc(n + 1)
                inv = acc(1) / n
                with np.errstate(invalid="ignore"):      # inf - inf, NaN: what the columns that hold them come to
                    d = x - mean
                    mean = mean + d * inv
                    m2 = m2 + d * (x - mean)
                    lo, hi = np.minimum(lo, A[r0 + r]), np.maximum(hi, A[r0 + r])
            total = _chan(total, (float(n), mean.astype(np.float64), m2.astype(np.float64)), mistake)
        parts.append((total, lo, hi))
    chains = []
    for q in range(fanin):
        t = (0.0, np.zeros(ld), np.zeros(ld))
        lo, hi = np.full(ld, np.inf, np.float32), np.full(ld, -np.inf, np.float32)
        for p in range(q, len(parts), fanin):
            t = _chan(t, parts[p][0], mistake)
            lo, hi = np.minimum(lo, parts[p][1]), np.maximum(hi, parts[p][2])
        chains.append([t, lo, hi])
    h = fanin // 2
    while h >= 1:
        for q in range(h):
            a, b = chains[q], chains[q + h]
            chains[q] = [_chan(a[0], b[0], mistake), np.minimum(a[1], b[1]), np.maximum(a[2], b[2])]
        h //= 2
    (n, mean, m2), lo, hi = chains[0]
    if prior is not None and mistake != "prior_ignored":
        pm, pv, pn = [np.asarray(v, np.float64) for v in prior]
        pm, pv = [np.concatenate([np.broadcast_to(v, (D,)), np.zeros(ld - D)]) for v in (pm, pv)]
        n, mean, m2 = _chan((float(pn), pm, pv * float(pn)), (n, mean, m2), mistake)
    var = m2 / (max(n - 1.0, 1.0) if mistake == "sample_variance" else max(n, 1.0))
    return lo[:D], hi[:D], np.asarray(mean, np.float64)[:D].copy(), np.asarray(var, np.float64)[:D].copy(), int(n)
