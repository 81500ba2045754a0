"""The seven distortion sums of one batch in numpy: what distortion_kernel<S> + distortion_finalize_kernel (frame_kernels.hip.h) and the
ledger path in front of them (ledger_lengths_kernel) must leave, with a COUNTED bound for each sum, the case list of
tests/test_gpu_distortion_sums.py, and the references of sequence_mask_kernel / pad_sequences_kernel.  Nothing here needs a GPU:
tests/test_distortion_host.py holds this module against tests/golden/distortions.npz and oracle/, and shows that the case list sees
ten seeded mistakes.

The definition (the kernel's header comment, restated).  Over the frames f = (b, t) with t < lengths[b], with S = float32 for float32
statistics and float64 for float64 ones:

    v(x)   = fl32(fl32(x * float32(std[k])) + float32(mean[k])) > 0.5,  k = stats[vuv_col]      always float32, two roundings
    a_c    = flS(flS(S(y[f][c]) * std[stats[c]]) + mean[stats[c]]),  h_c likewise from y_hat     two roundings in S, no fma
    z_c    = flS(a_c - h_c)                                      for the roles MCD, BAP, MSE
    z_c    = flS(flS(exp a_c) - flS(exp h_c))                    for the role LF0, only in frames voiced on both sides
    s_mcd  = sum_f sqrt(sum_{c in MCD} flS(z_c^2))   s_bap likewise   s_mse = sum_f sum_{c in MSE} flS(z_c^2)
    s_f0   = sum_{f voiced in both} sum_{c in LF0} flS(z_c^2)
    n_voiced = #{f: v(y) and v(y_hat)}   n_vuv_err = #{f: v(y) != v(y_hat)}   n_frames = #{f}

What is the same bits on the device, and so compared exactly: the inverse scaling (numpy multiplies and adds arrays of dtype S, one
rounding each, as inv_scale_rn does with contraction switched off), hence the three counts, and for S = float32 every flS(z^2) of MCD, BAP and MSE.

The bounds, u = 2^-53, every summand non-negative (so n terms added in ANY order are within (n - 1) u of their sum, relatively):

    s_mse: (n_role - 1) u   the device's sum of a frame's n_role terms (lane loop, wave reduction)
         + (N_valid - 1) u  its sum over the valid frames (per wave, per block, the partials, the finalize kernel)
         + 1 u              S = float64 only: the compiler may contract q += z * z into an fma, which leaves the product unrounded
         + 2 u              the reference's own two roundings (a frame's q in longdouble or fsum, rounded once; the total with fsum)
         + 1 u              second-order terms of the products (1 + u)^k
         = (n_role + N_valid + 2) u
    s_mcd, s_bap: the same (the square root halves the error of q, which is not claimed) + 2 u: the device's sqrt and numpy's, both
                  correctly rounded (IEEE) = (n_role + N_valid + 4) u.  All three stay below 2 (Ds + N_valid + 8) u, asserted in sums().
    s_f0: the reference takes exp in float64 of the S-rounded argument and forms z and z^2 in float64.  The device's expf / exp may be
          E ulp of S away from it: per element, from the reference's own a = exp a_c, h = exp h_c, z = a - h,
              |dz|     <= E ulp_S(a) + E ulp_S(h) + ulp_S(|z| + E ulp_S(a) + E ulp_S(h)) / 2
              |d(z^2)| <= 2 |z| |dz| + dz^2 + ulp_S(z^2 + 2 |z| |dz| + dz^2) / 2
          summed over the voiced frames, plus (n_lf0 + N_voiced + 2) u of (s_f0 + that sum) for the additions, plus 2^-51 s_f0 for the
          error of numpy's own float64 exp (below one ulp of float64 per operand).  The bound is a function of the inputs.

E = 1.  The HIP math API reference of the ROCm documentation ("HIP math API", tables "Single precision mathematical functions" and
"Double precision mathematical functions") states a maximum error of 1 ulp for expf and 1 ulp for exp.  The copy of ROCm this suite
was written on carries no statement of these errors: neither the installed documentation nor the HIP and clang math headers
(__clang_hip_math.h) contain one, so E could not be confirmed there and is taken from the published table.
"""
import math
from fractions import Fraction

import numpy as np

U64 = 2.0 ** -53
E_EXP = 1.0
ROLE_MCD, ROLE_BAP, ROLE_LF0, ROLE_VUV, ROLE_MSE, ROLE_NONE = 0, 1, 2, 3, 4, -1
NAMES = ("s_mcd", "s_bap", "s_f0", "n_voiced", "n_vuv_err", "s_mse", "n_frames")
I_MCD, I_BAP, I_F0, I_NV, I_VERR, I_MSE, I_N = range(7)
COUNTS = (I_NV, I_VERR, I_N)
F32, F64 = np.float32, np.float64
LOGDB_CONST = 10.0 / math.log(10.0) * math.sqrt(2.0)
# the seeded mistakes sums() can make (tests/test_distortion_host.py): each restates one way the kernel could be wrong
MISTAKES = ("vuv_fma", "col0_mcd", "ignore_lengths", "sqrt_after_sum", "no_exp", "va_or_vb", "stats_are_columns", "drop_cols_ge_64",
            "drop_tail_frames", "f32_stats_in_f64")


def cdiv(a, b):
    return (a + b - 1) // b


def _frame_sums(zz):
    """Row sums of non-negative float64 terms, each rounded to float64 once."""
    if zz.shape[1] == 0:
        return np.zeros(zz.shape[0], dtype=F64)
    if np.finfo(np.longdouble).nmant >= 63:      # 64-bit significand: the sum of < 2^10 doubles is within 2^-54 of exact before the rounding
        return zz.astype(np.longdouble).sum(axis=1).astype(F64)
    return np.array([math.fsum(r) for r in zz], dtype=F64)


def _ulp(x, S):
    with np.errstate(over="ignore"):
        return np.spacing(np.abs(np.asarray(x, dtype=F64)).astype(S)).astype(F64)


def clip_lengths(lengths, B, T):
    """What ledger_lengths_kernel makes of device lengths: None -> T, every entry cut to [0, T]."""
    if lengths is None:
        return [T] * B
    return [min(max(int(n), 0), T) for n in lengths]


def sums(y, yh, mean, std, roles, stats, vuv_col, lengths, stats_f64, mistake=None):
    """(values[7], bounds[7]) in the order of NAMES; bounds are absolute, 0.0 for the three counts.  ``y``, ``yh``: float32 [B][T][Ds];
    ``mean``, ``std``: the statistics table; ``lengths``: B entries in [0, T] or None.  ``mistake``: one of MISTAKES (tests only)."""
    assert mistake is None or mistake in MISTAKES
    y, yh = np.asarray(y, dtype=F32), np.asarray(yh, dtype=F32)
    B, T, Ds = y.shape
    assert yh.shape == y.shape and len(roles) == Ds and len(stats) == Ds and -1 <= vuv_col < Ds
    S = F64 if stats_f64 else F32
    mean_s, std_s = np.asarray(mean).astype(S), np.asarray(std).astype(S)
    if mistake == "f32_stats_in_f64":
        mean_s, std_s = mean_s.astype(F32).astype(S), std_s.astype(F32).astype(S)
    roles, stats = [int(r) for r in roles], [int(k) for k in stats]
    if mistake == "stats_are_columns":
        stats = list(range(Ds))
    if mistake == "col0_mcd":
        roles = [ROLE_MCD] + roles[1:]
    lens = clip_lengths(None if mistake == "ignore_lengths" else lengths, B, T)
    assert lengths is None or (len(lengths) == B and all(0 <= int(n) <= T for n in lengths))
    valid = (np.arange(T)[None, :] < np.asarray(lens)[:, None]).reshape(-1)
    if mistake == "drop_tail_frames":
        valid[len(valid) - len(valid) % 4:] = False
    yv, hv = y.reshape(B * T, Ds)[valid], yh.reshape(B * T, Ds)[valid]
    N = int(valid.sum())

    va = vb = np.zeros(N, dtype=bool)
    if vuv_col >= 0:
        vs, vm = F32(std_s[stats[vuv_col]]), F32(mean_s[stats[vuv_col]])
        if mistake == "vuv_fma":
            scale = lambda x: (x.astype(F64) * F64(vs) + F64(vm)).astype(F32)      # noqa: E731  (the product is exact in float64)
        else:
            scale = lambda x: (x * vs) + vm                                           # noqa: E731  two float32 roundings
        va, vb = scale(yv[:, vuv_col]) > F32(0.5), scale(hv[:, vuv_col]) > F32(0.5)
    both = (va | vb) if mistake == "va_or_vb" else (va & vb)

    def inv(x, c):
        p = x[:, c].astype(S) * std_s[stats[c]]       # rounded product ...
        return p + mean_s[stats[c]]                   # ... then rounded sum

    def cols_of(role):
        cs = [c for c in range(Ds) if roles[c] == role]
        return [c for c in cs if c < 64] if mistake == "drop_cols_ge_64" else cs

    vals, bounds = [0.0] * 7, [0.0] * 7
    for role, slot in ((ROLE_MCD, I_MCD), (ROLE_BAP, I_BAP), (ROLE_MSE, I_MSE)):
        cs = cols_of(role)
        if not cs or N == 0:
            continue
        z = np.stack([inv(yv, c) - inv(hv, c) for c in cs], axis=1)       # dtype S throughout
        q = _frame_sums((z * z).astype(F64))
        if slot == I_MSE:
            vals[slot], k = math.fsum(q), len(cs) + N + 2
        elif mistake == "sqrt_after_sum":
            vals[slot], k = math.sqrt(math.fsum(q)), len(cs) + N + 4
        else:
            vals[slot], k = math.fsum(np.sqrt(q)), len(cs) + N + 4
        assert k <= 2 * (Ds + N + 8)
        bounds[slot] = k * U64 * vals[slot]

    cs = cols_of(ROLE_LF0)
    nv = int(both.sum())
    if cs and nv:
        ex = (lambda v: v.astype(F64)) if mistake == "no_exp" else (lambda v: np.exp(v.astype(F64)))
        a = np.stack([ex(inv(yv[both], c)) for c in cs], axis=1)
        h = np.stack([ex(inv(hv[both], c)) for c in cs], axis=1)
        z = a - h
        zz = z * z
        ea = E_EXP * (_ulp(a, S) + _ulp(h, S))
        dz = ea + 0.5 * _ulp(np.abs(z) + ea, S)
        grow = 2.0 * np.abs(z) * dz + dz * dz
        dzz = grow + 0.5 * _ulp(zz + grow, S)
        vals[I_F0] = math.fsum(_frame_sums(zz))
        spread = math.fsum(dzz.reshape(-1))
        bounds[I_F0] = spread * (1.0 + 2.0 ** -40) + (len(cs) + nv + 2) * U64 * (vals[I_F0] + spread) + 2.0 ** -51 * vals[I_F0]
    vals[I_NV], vals[I_VERR], vals[I_N] = float(nv), float((va != vb).sum()), float(N)
    return vals, bounds


def outside(got, ref, bounds):
    """The names of the sums of ``got`` that are not within their bound of ``ref`` (NaN is outside; the counts must be equal)."""
    bad = []
    for i, name in enumerate(NAMES):
        g, r = float(got[i]), float(ref[i])
        ok = (g == r) if i in COUNTS else (abs(g - r) <= bounds[i])
        if not ok:
            bad.append(name)
    return bad


def metrics(vals, kind, Ds):
    """The logged metrics from the seven sums, as gantts_amd/train.py: compute_distortions forms them."""
    s_mcd, s_bap, s_f0, n_voiced, n_vuv_err, s_mse, n = vals
    if kind == "acoustic":
        return {"mcd": LOGDB_CONST * s_mcd / n, "bap_mcd": LOGDB_CONST * s_bap / n / 10.0,
                "f0_rmse": math.sqrt(s_f0 / n_voiced) if n_voiced > 0 else float("nan"), "vuv_err": n_vuv_err / n}
    if kind == "duration":
        return {"dur_rmse": math.sqrt(s_mse / (n * Ds))}
    return {"mcd": LOGDB_CONST * s_mcd / n}


# ---------------------------------------------------------------------------------------------------------------------
# the vuv threshold
# ---------------------------------------------------------------------------------------------------------------------
THRESHOLD_KINDS = ("rn_le_fma_gt", "rn_gt_fma_le", "on_half", "below_half", "above_half")
HALF = F32(0.5)
HALF_BELOW, HALF_ABOVE = np.nextafter(HALF, F32(0)), np.nextafter(HALF, F32(1))


def scale_rn(x, s, m):
    """fl32(fl32(x * s) + m) on float32 arrays or scalars."""
    return (np.asarray(x, dtype=F32) * F32(s)) + F32(m)


def fma_exceeds_half(x, s, m):
    """Whether the float32 fma(x, s, m) -- the exact x * s + m rounded ONCE to float32, ties to even -- is > 0.5: the exact value must
    exceed the midpoint of 0.5 and its upper neighbour (the tie goes to 0.5, whose significand is even).  Rational arithmetic."""
    exact = Fraction(float(x)) * Fraction(float(s)) + Fraction(float(m))
    return exact > (Fraction(float(HALF)) + Fraction(float(HALF_ABOVE))) / 2


def threshold_triples(n, seed, max_pairs=20000):
    """{kind: float32 array [n][3] of (x, s, m)} for the five THRESHOLD_KINDS, found by a deterministic search:
      rn_le_fma_gt   fl(fl(x s) + m) <= 0.5 <  fma(x, s, m)         rn_gt_fma_le   fl(fl(x s) + m) >  0.5 >= fma(x, s, m)
      on_half / below_half / above_half   fl(fl(x s) + m) is exactly 0.5 / its lower / its upper float32 neighbour.
    s and m are scalars of a column, so the search draws one (s, m) and walks the float32 x around (0.5 - m) / s for it; a pair gives at
    most a few x of the first two kinds (the window in which the two roundings disagree is narrower than one step of x), so the n
    triples of a kind come from n different pairs -- a case per pair (threshold_groups).  Raises if ``max_pairs`` pairs do not deliver n of
    every kind."""
    rs = np.random.RandomState(seed)
    found = {k: [] for k in THRESHOLD_KINDS}
    for _ in range(max_pairs):
        if all(len(v) >= n for v in found.values()):
            break
        # half of the pairs cancel a large product against a large mean: there the product's rounding is coarse next to 0.5
        if rs.rand() < 0.5:
            s, m = F32(0.05 + 1.95 * rs.rand()), F32(rs.randn() * 0.4)
        else:
            m = F32(-(2.0 ** rs.randint(0, 6)) * (1.0 + rs.rand()))
            s = F32(0.25 + 3.0 * rs.rand())
        x0 = F32((0.5 - float(m)) / float(s))
        if not np.isfinite(x0) or x0 == 0:
            continue
        xs = (np.asarray(x0).view(np.int32) + np.arange(-48, 49, dtype=np.int32)).view(F32)      # 97 consecutive float32 around x0
        rn = scale_rn(xs, s, m)
        got = set()
        near = np.abs(rn.astype(F64) - 0.5) <= 2.0 ** -16      # |x s| < 256: the product's rounding moves the sum by less than 2^-17
        for x, r in zip(xs[near], rn[near]):
            fma_gt = fma_exceeds_half(x, s, m)
            if r <= HALF and fma_gt:
                kind = "rn_le_fma_gt"
            elif r > HALF and not fma_gt:
                kind = "rn_gt_fma_le"
            elif r == HALF:
                kind = "on_half"
            elif r == HALF_BELOW:
                kind = "below_half"
            elif r == HALF_ABOVE:
                kind = "above_half"
            else:
                continue
            if kind not in got and len(found[kind]) < n:      # one x of a kind per pair: n triples, n pairs
                got.add(kind)
                found[kind].append((x, s, m))
    short = [k for k, v in found.items() if len(v) < n]
    if short:
        raise RuntimeError("threshold_triples(%d, %d): too few triples of %s" % (n, seed, short))
    return {k: np.array(v, dtype=F32) for k, v in found.items()}


def threshold_groups(n, seed):
    """The triples of threshold_triples(n, seed) grouped by their (s, m): [(s, m, [(kind, x), ...])], in a fixed order."""
    groups = {}
    for kind, arr in threshold_triples(n, seed).items():
        for x, s, m in arr:
            groups.setdefault((float(s), float(m)), []).append((kind, F32(x)))
    return [(F32(s), F32(m), groups[(s, m)]) for s, m in sorted(groups)]


# ---------------------------------------------------------------------------------------------------------------------
# layouts: (roles, stats, vuv_col, number of statistics)
# ---------------------------------------------------------------------------------------------------------------------
def acoustic_streams(Ds):
    """Static stream sizes (mgc, lf0, vuv, bap) of an acoustic layout with Ds static columns: lf0 is one column, vuv one (two from
    Ds = 9 on: a spare column nobody reads), bap one per 13 columns, mgc the rest (63 -> 60 + 1 + 1 + 1 would be the flagship's; this
    rule gives 63 -> 56, 1, 2, 4)."""
    svuv, sbap = (2 if Ds >= 9 else 1), max(1, Ds // 13)
    smgc = Ds - 1 - svuv - sbap
    assert smgc >= 2, "an acoustic layout needs the energy column and one MCD column"
    return smgc, 1, svuv, sbap


def layout(kind, Ds, seed=0, nw=3, streams=None):
    """kind = "acoustic": the layout of train._acoustic_columns for the static streams ``streams`` (default acoustic_streams(Ds)),
    mgc, lf0 and bap with ``nw`` windows, vuv without dynamic features -- statistics indexed in the static+dynamic domain;
    "mse" / "mcd": every column of that role, stats[c] = c, no vuv column (the duration and the vc layout);
    "general": every role and ROLE_NONE shuffled over the columns, LF0 and VUV above column 63 where Ds allows, stats a shuffled
    injection into a table of 2 Ds + 3 entries (not monotone, != c: static and static+dynamic indices cannot be swapped unseen);
    "nolf0": the general layout with its LF0 columns turned into MSE columns (a vuv column, no LF0 column)."""
    if kind in ("mse", "mcd"):
        return [ROLE_MSE if kind == "mse" else ROLE_MCD] * Ds, list(range(Ds)), -1, Ds
    if kind == "acoustic":
        smgc, slf0, svuv, sbap = streams or acoustic_streams(Ds)
        assert smgc + slf0 + svuv + sbap == Ds
        lf0_0, vuv_0, bap_0 = nw * smgc, nw * smgc + nw * slf0, nw * smgc + nw * slf0 + svuv
        roles = [ROLE_NONE] + [ROLE_MCD] * (smgc - 1) + [ROLE_LF0] * slf0 + [ROLE_VUV] + [ROLE_NONE] * (svuv - 1) + [ROLE_BAP] * sbap
        stats = list(range(smgc)) + [lf0_0 + j for j in range(slf0)] + [vuv_0] * svuv + [bap_0 + j for j in range(sbap)]
        return roles, stats, smgc + slf0, bap_0 + nw * sbap
    assert kind in ("general", "nolf0") and Ds >= 6
    rs = np.random.RandomState(1000 * Ds + seed)
    roles = [ROLE_MCD, ROLE_BAP, ROLE_MSE, ROLE_NONE] + [int(r) for r in rs.choice([ROLE_MCD, ROLE_BAP, ROLE_LF0, ROLE_MSE, ROLE_NONE], Ds - 6)]
    rs.shuffle(roles)
    roles += [ROLE_LF0, ROLE_VUV]                    # the last two columns: above 63 for Ds >= 66 ...
    if Ds == 65:
        roles[63], roles[64] = ROLE_VUV, ROLE_LF0    # ... and at 63 / 64, on either side of the lane loop's first trip, for Ds = 65
    vuv_col = roles.index(ROLE_VUV)
    assert roles.count(ROLE_VUV) == 1
    nstat = 2 * Ds + 3
    stats = [int(k) for k in rs.permutation(nstat)[:Ds]]
    for c in range(Ds):                              # no column may sit on its own index
        if stats[c] == c:
            stats[c], stats[(c + 1) % Ds] = stats[(c + 1) % Ds], stats[c]
    assert all(stats[c] != c for c in range(Ds)) and len(set(stats)) == Ds
    if kind == "nolf0":
        roles = [ROLE_MSE if r == ROLE_LF0 else r for r in roles]
    return roles, stats, vuv_col, nstat


# ---------------------------------------------------------------------------------------------------------------------
# the case list of tests/test_gpu_distortion_sums.py
# ---------------------------------------------------------------------------------------------------------------------
def ragged_lengths(B, T, rs):
    """Lengths with a 0 in the middle and a 0 at the end (B >= 3), the first sequence not empty."""
    if B == 1:
        return [max(1, T - 1)]
    if B == 2:
        return [max(1, T - 2), 0]
    n = [int(v) for v in rs.randint(0, T + 1, B)]
    n[0], n[B // 2], n[B - 1] = max(1, T - 1), 0, 0
    if B > 4:
        n[1] = T
    return n


def _len_of(kind, B, T, rs):
    if kind == "none":
        return None
    if kind == "full":
        return [T] * B
    if kind == "single":      # one valid frame in the whole batch, not in the first sequence where there is another
        n = [0] * B
        n[B // 2] = 1
        return n
    assert kind == "ragged"
    return ragged_lengths(B, T, rs)


# (B, T, Ds, layout, lengths): nblk = min(1024, cdiv(B T, 4)) is 1, 1, 13, 5, 1024 (4200 frames: 104 in the second trip),
# 1024 (4097 frames: one in the second trip), 258 and 290
_BASE = [
    (1, 1, 1, "mse", "none"), (1, 1, 1, "mcd", "full"),
    (1, 3, 5, "acoustic", "ragged"), (1, 3, 5, "mse", "none"),
    (3, 17, 63, "acoustic", "ragged"), (3, 17, 63, "general", "single"), (3, 17, 63, "mcd", "none"),
    (3, 17, 64, "acoustic", "full"), (3, 17, 64, "general", "ragged"), (3, 17, 64, "mcd", "none"),
    (3, 17, 65, "general", "none"), (3, 17, 65, "general", "ragged"), (3, 17, 65, "acoustic", "single"), (3, 17, 65, "mse", "ragged"),
    (2, 9, 130, "general", "ragged"), (2, 9, 130, "general", "none"), (2, 9, 130, "nolf0", "full"), (2, 9, 130, "mcd", "ragged"),
    (3, 1400, 5, "acoustic", "none"), (3, 1400, 5, "mse", "ragged"), (3, 1400, 5, "acoustic", "full"),
    (1, 4097, 63, "acoustic", "none"), (1, 4097, 63, "mcd", "ragged"),
    (1030, 1, 5, "acoustic", "none"), (1030, 1, 5, "acoustic", "ragged"), (1030, 1, 5, "mse", "single"),
    # Scratch::ensure keeps need + need / 8 bytes: the ledger's first 1024 lengths are room for 1152, so 1030 sequences do not make
    # its length buffer grow and 1160 do
    (1160, 1, 5, "acoustic", "ragged"),
]
THRESHOLD_N, THRESHOLD_SEED = 3, 20240917


def case_list():
    """Every case as a dict (id, B, T, Ds, layout, lengths, f64, and for the special ones `special`); both statistics types of each."""
    out = []
    for B, T, Ds, lay, lens in _BASE:
        for f64 in (False, True):
            out.append(dict(id="%dx%d-Ds%d-%s-%s-%s" % (B, T, Ds, lay, lens, "f64" if f64 else "f32"), B=B, T=T, Ds=Ds, layout=lay,
                            lengths=lens, f64=f64, special=None))
    for f64 in (False, True):
        out.append(dict(id="unvoiced-%s" % ("f64" if f64 else "f32"), B=3, T=17, Ds=63, layout="acoustic", lengths="ragged", f64=f64,
                        special="unvoiced"))
        for g in range(len(threshold_groups(THRESHOLD_N, THRESHOLD_SEED))):
            out.append(dict(id="threshold%d-%s" % (g, "f64" if f64 else "f32"), B=2, T=9, Ds=5, layout="acoustic", lengths="none", f64=f64,
                            special=("threshold", g)))
    return out


_THRESHOLD_CACHE = {}


def threshold_groups_cached():
    if "g" not in _THRESHOLD_CACHE:
        _THRESHOLD_CACHE["g"] = threshold_groups(THRESHOLD_N, THRESHOLD_SEED)
    return _THRESHOLD_CACHE["g"]


def make_case(case, poison=True):
    """The inputs of a case: dict(y, yh, mean, std, roles, stats, vuv_col, lengths, f64, B, T, Ds).  With ``poison`` every ROLE_NONE
    column, every frame at t >= lengths[b] (in y and y_hat) and every statistics entry no column indexes hold NaN; without, finite
    values drawn from the same generator state (so the rest of the inputs are the same bits)."""
    B, T, Ds = case["B"], case["T"], case["Ds"]
    rs = np.random.RandomState(sum((i + 1) * 7919 * v for i, v in enumerate((B, T, Ds, len(case["layout"]), len(case["lengths"])))) % (1 << 31))
    roles, stats, vuv_col, nstat = layout(case["layout"], Ds)
    y = rs.randn(B, T, Ds).astype(F32)
    yh = (y + 0.4 * rs.randn(B, T, Ds)).astype(F32)
    mean = rs.randn(nstat) * 0.5
    std = 0.5 + 1.5 * rs.rand(nstat)
    for c in range(Ds):
        if roles[c] == ROLE_LF0:                        # log-F0: around exp(5), a range of a few per cent
            mean[stats[c]], std[stats[c]] = 5.0 + 0.1 * rs.randn(), 0.25
    if vuv_col >= 0:
        mean[stats[vuv_col]], std[stats[vuv_col]] = 0.55, 0.45
    if case["f64"]:
        mean, std = mean.astype(F64), std.astype(F64)   # 53-bit values: not representable in float32
    else:
        mean, std = mean.astype(F32), std.astype(F32)
    lengths = _len_of(case["lengths"], B, T, rs)
    if case["special"] == "unvoiced":
        y[:, :, vuv_col] = -2.0                         # 0.55 - 0.9: no frame of y is voiced
    elif case["special"] is not None:
        s, m, xs = threshold_groups_cached()[case["special"][1]]
        k = stats[vuv_col]
        std[k], mean[k] = s, m                          # float32 values: exact in either table
        hi, lo = F32((2.0 - float(m)) / float(s)), F32((-1.0 - float(m)) / float(s))      # scale to about 2 and about -1
        yv, hv = y.reshape(B * T, Ds), yh.reshape(B * T, Ds)
        yv[:, vuv_col], hv[:, vuv_col] = hi, hi
        for i, (_, x) in enumerate(xs):                 # frame 2 i: x in y against a voiced y_hat; frame 2 i + 1: x in y_hat against a
            yv[2 * i, vuv_col] = x                      # voiced y (both move n_voiced and n_vuv_err the same way: nothing cancels)
            hv[2 * i + 1, vuv_col] = x
        yv[B * T - 1, vuv_col] = lo                     # and one frame that is unvoiced in y whatever happens
        assert 2 * len(xs) < B * T
    fill_y, fill_h, fill_s = rs.randn(B, T, Ds).astype(F32), rs.randn(B, T, Ds).astype(F32), rs.randn(nstat)
    if poison:
        fill_y, fill_h, fill_s = np.full_like(fill_y, np.nan), np.full_like(fill_h, np.nan), np.full_like(fill_s, np.nan)
    none_cols = [c for c in range(Ds) if roles[c] == ROLE_NONE]
    y[:, :, none_cols], yh[:, :, none_cols] = fill_y[:, :, none_cols], fill_h[:, :, none_cols]
    if lengths is not None:
        dead = np.arange(T)[None, :] >= np.asarray(lengths)[:, None]
        y[dead], yh[dead] = fill_y[dead], fill_h[dead]
    used = set(stats[c] for c in range(Ds) if roles[c] != ROLE_NONE)
    unused = [k for k in range(nstat) if k not in used]
    mean[unused], std[unused] = fill_s[unused].astype(mean.dtype), fill_s[unused].astype(std.dtype)
    return dict(y=y, yh=yh, mean=mean, std=std, roles=roles, stats=stats, vuv_col=vuv_col, lengths=lengths, f64=case["f64"],
                B=B, T=T, Ds=Ds)


_REF_CACHE = {}


def case_reference(case):
    """(inputs, values, bounds) of a case, computed once per process and not to be changed by the caller."""
    if case["id"] not in _REF_CACHE:
        d = make_case(case)
        v, b = sums(d["y"], d["yh"], d["mean"], d["std"], d["roles"], d["stats"], d["vuv_col"], d["lengths"], d["f64"])
        for a in (d["y"], d["yh"], d["mean"], d["std"]):
            a.setflags(write=False)
        _REF_CACHE[case["id"]] = (d, v, b)
    return _REF_CACHE[case["id"]]


# ---------------------------------------------------------------------------------------------------------------------
# sequence_mask_kernel, pad_sequences_kernel
# ---------------------------------------------------------------------------------------------------------------------
SEQ_SHAPES = [(1, 1), (15, 17), (16, 16), (1, 257)]      # B T = 1, 255, 256, 257: the last thread of a block, the first of the next


def seq_lengths(B, T, rs):
    """B lengths in [0, T + 3] holding 0, T and T + 3 where B allows (B = 1: the caller runs each of them)."""
    n = [int(v) for v in rs.randint(0, T + 4, B)]
    if B >= 3:
        n[0], n[B // 2], n[B - 1] = T + 3, 0, T
    return n


def sequence_mask_ref(lengths, T):
    return (np.arange(T)[None, :] < np.asarray(lengths)[:, None]).astype(F32)


def pad_sequences_ref(ragged, start, length, T, ld):
    """out[b][t][c] = ragged[start[b] + t][c] for t < min(len[b], T), c < D; +0.0 in every other word of the [B][T][ld] result."""
    D = ragged.shape[1]
    out = np.zeros((len(start), T, ld), dtype=F32)
    for b, (s0, n) in enumerate(zip(start, length)):
        n = min(int(n), T)
        out[b, :n, :D] = ragged[s0:s0 + n]
    return out
