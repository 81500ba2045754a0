"""Float64 host reference of variance-weighted MLPG (nnmnkwii.paramgen.mlpg), the comparator of tests/test_gpu_mlpg_var.py, and a
sequential float64 model of the device's column solve (gantts_amd/csrc/mlpg_var_kernels.hip.h) with seeded mistakes.

nnmnkwii's algorithm, restated: for each static dimension, with windows (W_w x)[t] = sum_k coef_w[k + l_w] x[t + k] (terms outside the
sequence dropped), precisions p_w = 1 / var_w and means mu_w,

    P = sum_w W_w^T diag(p_w) W_w        b = sum_w W_w^T (p_w mu_w)        P c = b

P is banded with half-bandwidth hb = max_w (l_w + u_w): `solve_column` builds its lower band and solves with scipy.linalg.solveh_banded.
`solve_column_dense` is the independent construction: explicit W matrices and np.linalg.solve.  Every sequence is solved over its own
length, as an utterance evaluated alone.

The bound of the comparator, for every dynamic output element:  |dev - ref| <= 2^-24 |ref| + 2^-40 peak,  peak the largest |ref| of the
element's column: one float32 rounding, and the float64 solve's error, which grows with cond(P); the inputs are chosen so that
cond(P) <= 2^11 (asserted by tests/test_mlpg_var_host.py for every case), where a backward-stable float64 solve is within
~ 2^-53 * 2^11 * (a small multiple of hb) of the solution -- more than 40 times under 2^-40.  Pass-through columns and the zero rows
beyond a length are compared bit for bit.
"""
import functools

import numpy as np
import scipy.linalg

U24, U40 = 2.0 ** -24, 2.0 ** -40
COND_LIMIT = 2.0 ** 11
T_VALUES = [1, 2, 3, 5, 17, 65, 200]
VAR_FORMS = ["ones", "row", "frame"]
SET_NAMES = ["std", "static", "delta", "asym", "four", "hb1"]       # of test_gpu_mlpg.WINDOW_SETS, and the hb = 1 pair
MISTAKES = ["edge", "wrong_window", "b_without_precision", "full_T", "row_frame_stride"]


def window_sets():
    import test_gpu_mlpg as M
    sets = {n: M.WINDOW_SETS[n] for n in SET_NAMES if n != "hb1"}
    sets["hb1"] = [(0, 0, np.array([1.0])), (0, 1, np.array([-1.0, 1.0]))]
    return sets


def half_bandwidth(windows):
    return max(int(l) + int(u) for (l, u, _) in windows)


def ragged_lengths(T):
    return [T, T // 2 + 1, 1]


def layout(n, nW):
    """the [3n, 3, 1, 3]-shaped layout of test_gpu_mlpg.streams scaled to nW windows: (stream sizes, has_dynamic, scol, sstride, D, Ds)"""
    ss, hd = [n * nW, nW, 1, nW], [True, True, False, True]
    scol, sst, col = [], [], 0
    for sz, dyn in zip(ss, hd):
        w = sz // nW if dyn else sz
        scol += [col + c for c in range(w)]
        sst += [w if dyn else 0] * w
        col += sz
    return ss, hd, np.array(scol), np.array(sst), col, len(scol)


def make_inputs(name, T, var_form, B=3, n=5, seed=None):
    """(y [B][T][D] float32, var float32 [D] or [B][T][D], lengths): normal means, variances 4^U(-1, 1) rounded to float32"""
    nW = len(window_sets()[name])
    D = layout(n, nW)[4]
    rs = np.random.RandomState(1000 * T + 10 * SET_NAMES.index(name) + VAR_FORMS.index(var_form) if seed is None else seed)
    y = rs.randn(B, T, D).astype(np.float32)
    if var_form == "ones":
        var = np.ones(D, np.float32)
    elif var_form == "row":
        var = (4.0 ** rs.uniform(-1, 1, D)).astype(np.float32)
    else:
        var = (4.0 ** rs.uniform(-1, 1, (B, T, D))).astype(np.float32)
    lengths = ragged_lengths(T) if B == 3 else [T] * B
    return y, var, lengths


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def band_system(mu, var, windows):
    """mu, var [n][nW] float64 -> (lower band ab [hb + 1][n] of P, b [n])"""
    n = mu.shape[0]
    hb = half_bandwidth(windows)
    ab, rhs = np.zeros((hb + 1, n)), np.zeros(n)
    t = np.arange(n)
    for w, (l, u, coef) in enumerate(windows):
        l, u, coef = int(l), int(u), np.asarray(coef, np.float64)
        p = 1.0 / var[:, w]
        for qa in range(-l, u + 1):
            ok_a = (t + qa >= 0) & (t + qa < n)
            np.add.at(rhs, t[ok_a] + qa, coef[qa + l] * p[ok_a] * mu[ok_a, w])
            for qb in range(-l, qa + 1):
                ok = ok_a & (t + qb >= 0) & (t + qb < n)
                np.add.at(ab[qa - qb], t[ok] + qb, p[ok] * coef[qa + l] * coef[qb + l])
    return ab, rhs


def solve_column(mu, var, windows):
    ab, rhs = band_system(mu, var, windows)
    ab = ab[:min(ab.shape[0], len(rhs))]      # diagonals beyond the matrix hold nothing (and LAPACK's tridiagonal driver refuses them at n = 1)
    if len(rhs) == 1:
        return rhs / ab[0]
    return scipy.linalg.solveh_banded(ab, rhs, lower=True, check_finite=False)


def dense_window(window, n):
    l, u, coef = int(window[0]), int(window[1]), np.asarray(window[2], np.float64)
    W = np.zeros((n, n))
    for t in range(n):
        for k in range(-l, u + 1):
            if 0 <= t + k < n:
                W[t, t + k] = coef[k + l]
    return W


def dense_system(mu, var, windows):
    n = mu.shape[0]
    P, rhs = np.zeros((n, n)), np.zeros(n)
    for w, win in enumerate(windows):
        W = dense_window(win, n)
        P += W.T @ np.diag(1.0 / var[:, w]) @ W
        rhs += W.T @ (mu[:, w] / var[:, w])
    return P, rhs


def solve_column_dense(mu, var, windows):
    P, rhs = dense_system(mu, var, windows)
    return np.linalg.solve(P, rhs)


def condition(mu, var, windows):
    w = np.linalg.eigvalsh(dense_system(mu, var, windows)[0])
    return float(w[-1] / w[0])


def columns_of(y, var, scol, sst, nW, b, c, n):
    """(mu, var) [n][nW] float64 of sequence b, static column c"""
    cols = scol[c] + np.arange(nW) * sst[c]
    mu = y[b, :n][:, cols].astype(np.float64)
    v = np.broadcast_to(var[cols], (n, nW)) if var.ndim == 1 else var[b, :n][:, cols]
    return mu, np.asarray(v, np.float64)


def reference(y, var, windows, scol, sst, lengths, solver=solve_column):
    """[B][T][Ds] float64: every sequence over its own length, 0 beyond it; pass-through columns copied"""
    B, T, _ = y.shape
    nW = len(windows)
    out = np.zeros((B, T, len(scol)))
    for b in range(B):
        n = int(lengths[b])
        for c in range(len(scol)):
            if sst[c] == 0:
                out[b, :n, c] = y[b, :n, scol[c]]
            else:
                out[b, :n, c] = solver(*columns_of(y, var, scol, sst, nW, b, c, n), windows)
    return out


@functools.lru_cache(maxsize=None)
def case(name, T, var_form):
    """a GPU case and its reference, computed once: (y, var, lengths, ref)"""
    windows = window_sets()[name]
    _, _, scol, sst, _, _ = layout(5, len(windows))
    y, var, lengths = make_inputs(name, T, var_form)
    ref = reference(y, var, windows, scol, sst, lengths)
    for a in (y, var, ref):
        a.setflags(write=False)
    return y, var, lengths, ref


# ---------------------------------------------------------------------------------------------------------------------
# the comparator
# ---------------------------------------------------------------------------------------------------------------------
def compare(dev, ref, y, scol, sst, lengths):
    """(worst |dev - ref| / bound over the dynamic elements inside the lengths, elements over the bound, elements that had to equal bit
    for bit and do not): the bound is 2^-24 |ref| + 2^-40 peak, peak the largest |ref| of the element's column (b, c)."""
    dev = np.asarray(dev, np.float32)
    B, T, Ds = ref.shape
    assert dev.shape == ref.shape
    worst, over, bad_bits = 0.0, 0, 0
    for b in range(B):
        n = int(lengths[b])
        bad_bits += int((dev[b, n:].view(np.uint32) != 0).sum())                      # +0.0 beyond the length
        for c in range(Ds):
            if sst[c] == 0:
                bad_bits += int((dev[b, :n, c].view(np.uint32) != np.ascontiguousarray(y[b, :n, scol[c]], np.float32).view(np.uint32)).sum())
                continue
            r = ref[b, :n, c]
            err = np.abs(dev[b, :n, c].astype(np.float64) - r)
            err[~np.isfinite(err)] = np.inf
            ratio = err / (U24 * np.abs(r) + U40 * np.abs(r).max())
            worst = max(worst, float(ratio.max()))
            over += int((ratio > 1.0).sum())
    return worst, over, bad_bits


# ---------------------------------------------------------------------------------------------------------------------
# a float64 model of the device's column solve, and its seeded mistakes
# ---------------------------------------------------------------------------------------------------------------------
def model_column(y, var, windows, scol, sst, b, c, n, mistake=None):
    """x [n] float64 as the kernels compute it: P and b of the column, a banded Cholesky column by column with the forward substitution
    riding along, the back substitution from the last row upwards.  `mistake`: one of MISTAKES."""
    T, D = y.shape[1], y.shape[2]
    nW, hb = len(windows), half_bandwidth(windows)
    if mistake == "full_T":
        n = T
    frames = T if mistake == "edge" else n      # "edge": frames beyond the length still contribute to the columns inside it

    def v_at(t, w):
        col = scol[c] + ((w + 1) % nW if mistake == "wrong_window" else w) * sst[c]
        if var.ndim == 1:
            return float(var[(col + t) % D]) if mistake == "row_frame_stride" else float(var[col])
        return float(var[b, t, col])

    P = np.zeros((n, hb + 1))
    rhs = np.zeros(n)
    for w, (l, u, coef) in enumerate(windows):
        l, u = int(l), int(u)
        for t in range(frames):
            p = 1.0 / v_at(t, w)
            m = float(y[b, t, scol[c] + w * sst[c]])
            for qa in range(-l, u + 1):
                i = t + qa
                if not 0 <= i < n:
                    continue
                rhs[i] += coef[qa + l] * (m if mistake == "b_without_precision" else p * m)
                for qb in range(-l, qa + 1):
                    j = t + qb
                    if 0 <= j < n:
                        P[j, i - j] += p * coef[qa + l] * coef[qb + l]
    L, z = np.zeros((n, hb + 1)), np.zeros(n)
    for j in range(n):
        for k in range(min(hb, n - 1 - j) + 1):
            i = j + k
            v = P[j, k] - sum(L[m, i - m] * L[m, j - m] for m in range(max(0, i - hb), j))
            L[j, k] = np.sqrt(v) if k == 0 else v / L[j, 0]
        z[j] = (rhs[j] - sum(L[m, j - m] * z[m] for m in range(max(0, j - hb), j))) / L[j, 0]
    x = np.zeros(n)
    for j in range(n - 1, -1, -1):
        x[j] = (z[j] - sum(L[j, k] * x[j + k] for k in range(1, min(hb, n - 1 - j) + 1))) / L[j, 0]
    return x


def model(y, var, windows, scol, sst, lengths, mistake=None):
    """the device's output as float32 [B][T][Ds]"""
    B, T, _ = y.shape
    out = np.zeros((B, T, len(scol)), np.float32)
    for b in range(B):
        n = int(lengths[b])
        for c in range(len(scol)):
            if sst[c] == 0:
                out[b, :n, c] = y[b, :n, scol[c]]
            else:
                x = model_column(y, var, windows, scol, sst, b, c, n, mistake)
                out[b, :len(x), c] = x.astype(np.float32)
    return out
