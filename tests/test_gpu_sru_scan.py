"""Every SRU scan kernel and image output against float64 (gt_op_sru_scan, gt_sru_path_counts).

The recurrence has two sequential scans (sru_kernels.hip.h), eight cooperative-scan instantiations (sru_cs_kernels.hip.h: four or eight
waves per 64 columns x forward / backward x float32 results / bf16 images) and three helper kernels.  gt_op_sru_scan runs ONE scan
launch through the launch functions of the engine's stacks (sru_launch_fwd / _bwd), gt_sru_path_counts counts the launches per kernel,
so each case here asserts WHICH kernel ran (against `expected_counts`, a restatement of the 8 / 4-wave rule and the image conditions)
and compares every output element with a float64 evaluation of the recurrence in the header comment of sru_kernels.hip.h -- exact
sigmoid / tanh on the same float32 inputs, written here in numpy, independent of oracle/gantts_oracle.py.

Bound: next to each quantity the reference carries a running error scale S -- the same recurrence on absolute values, every operation
adding its own rounding (the per-operation constants SIG_ULPS, TANH_ULPS and one ulp per fmaf / multiply) -- and an element passes if
|got - ref| <= ULPS[kind] * 2^-24 * S; per tensor the rms of |got - ref| / S is limited as well.  ULPS / RMS_LIM are at most 4 x the
worst figure measured on an MI355X over the whole matrix (MEASURED below, profiles/sru_scan_parity.md).  The backward reference reads
the same float32 cell-state stash as the kernel, so act'(c) and c_prev are data: no relu kink, no element is excluded.

The bf16 images are judged exactly.  A float32 numpy model of the cooperative association, perturbed in five ways, shows on the CPU
that the limits are discriminating (test_limits_reject_mutations_of_the_cooperative_association)."""
import collections
import ctypes as Ct
import functools
import zlib

import numpy as np
import pytest
import torch

from test_gpu_gemm_f32 import SENT, U, _bf16, cdiv, philox4x32_10
from test_gpu_gemm_b16 import PAD16, _F32, _I16, pads_intact

NSLOTS = 13
FWD, FWD_CS, BWD, BWD_CS, INPUT_MASK, INPUT_DROPOUT, DX_ADV_FINISH = 0, 1, 5, 6, 10, 11, 12      # gt_sru_path_counts
KNOBS = dict(sru_coop=1, sru_cs_waves=0)       # GtTuning defaults
CUS = 256
ID, TANH, RELU = 0, 1, 2
KEYS = (0x1234ABCD, 0x9E3779B9)
P_DROP = 0.3
SEQ_MUL, SEQ_ADD = 2, 1

# per-operation constants of the running error scale, in float32 ulps
SIG_ULPS = 4.0        # fast_sigmoid: v_exp_f32 + v_rcp_f32 with the folded-in correction (fast_math.hip.h: "a few ulp")
TANH_ULPS = 4.0       # tanhf of the device library
# Limits, in units of 2^-24 * S: worst |got - ref| / (2^-24 * S) per element, and rms of it per tensor.  MEASURED: the worst figure over the
# whole matrix on an MI355X with the case that produced it; the limit is at most 4 x that (the margin of the other kernel suites; it covers the
# association differences between the sequential, 4- and 8-wave forms).
MEASURED = {      # kind: (worst ratio, case), (worst rms, case)
    "c": ((1.480, "cs8-fwd-B3H64x2-T208-k4-relu-m2-img-saturated"), (0.172, "cs4-fwd-B1H64x1-T1-k3-tanh-m0-normal")),
    "h": ((0.779, "cs8-fwd-B3H20x2-T256-k3-tanh-m1-normal"), (0.180, "cs4-fwd-B1H1x1-T7-k3-relu-m2-long")),
    "dU": ((0.712, "cs8-bwd-B3H20x2-T133-k4-relu-m0-ua-long"), (0.114, "cs4-bwd-B1H1x1-T8-k4-tanh-m2-um-ua-long")),
    "dx": ((0.685, "cs8-bwd-B3H20x2-T256-k3-relu-m1-ua-normal"), (0.159, "cs8-bwd-B3H64x2-T8-k3-relu-m0-ua-img-long")),
    "dbias": ((0.321, "cs4-bwd-B3H64x2-T8-k4-relu-m0-img-long"), (0.074, "seq-bwd-B1H64x1-T1-k4-tanh-m0-um-ua-normal")),
}
ULPS = {"c": 4.5, "h": 2.4, "dU": 2.2, "dx": 2.0, "dbias": 1.0}              # about 3 x MEASURED
RMS_LIM = {"c": 0.5, "h": 0.55, "dU": 0.35, "dx": 0.5, "dbias": 0.22}
MUTATION_MARGIN = 10.0
# Absolute floor of every limit: the gate functions flush float32 denormals (v_exp_f32 / v_rcp_f32), so a quantity below 2^-126 may
# become 0 -- fewer than 16 operations per frame, T frames behind any element.  Matters only where a saturated gate (f or 1 - f ~ 1e-44)
# makes an exact result denormal; the values of the cases are of order 1.
FTZ = 16 * 2.0 ** -126


# ---------------------------------------------------------------------------------------------------------------------
# the launcher's choice, restated
# ---------------------------------------------------------------------------------------------------------------------
class Invalid(Exception):
    pass


def waves_of(form, B, ncols, cus=CUS):
    """0 sequential, else waves per 64 columns: eng_sru.hip sru_coop / sru_coop_waves.  form: 0, 4, 8 or "auto" (sru_cs_waves = 0)."""
    if form == 0:
        return 0
    if form in (4, 8):
        return form
    return 8 if cdiv(B * ncols, 64) <= 2 * cus else 4


def knobs_of(form):
    return dict(sru_coop=0) if form == 0 else dict(sru_coop=1, sru_cs_waves=0 if form == "auto" else form)


def expected_counts(c, bwd, img, cus=CUS):
    """launches per slot of gt_sru_path_counts of one gt_op_sru_scan call."""
    w = waves_of(c["form"], c["B"], c["H"] * c["dirs"], cus)
    if img and not (w and c["T"] % 8 == 0 and c["H"] % 64 == 0):
        raise Invalid("images need a cooperative form, T % 8 == 0 and H % 64 == 0")
    counts = [0] * NSLOTS
    if w == 0:
        counts[BWD if bwd else FWD] = 1
    else:
        counts[(BWD_CS if bwd else FWD_CS) + 2 * (w == 8) + (1 if img else 0)] = 1
    return counts


# ---------------------------------------------------------------------------------------------------------------------
# the case matrix
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 64, 1), (3, 20, 2), (1, 1, 1)]            # one full workgroup / a partial second one, boundaries inside a wave / one lane
IMG_SHAPES = [(3, 64, 2), (2, 128, 1)]                  # every second workgroup in the flipped direction / two workgroups per sequence


def coop_T(nw):
    F = 8 * nw
    return [1, 7, 8, 9, F - 1, F, F + 1, 2 * F + 5, 4 * F]


def img_T(nw):
    F = 8 * nw
    return [8, F, F + 8, 3 * F + 16]


SEQ_T = {False: [1, 11, 12, 13, 25], True: [1, 7, 8, 9, 17]}      # unroll 12 forward, 8 backward


def case(form, bwd, shape, T, k, act, mask, up_mul, up_add, flavour, img=False, nx_mul=False):
    B, H, dirs = shape
    c = dict(form=form, bwd=bwd, B=B, H=H, dirs=dirs, T=T, k=k, act=act, mask=mask, up_mul=up_mul, up_add=up_add, flavour=flavour, img=img,
             nx_mul=nx_mul)
    c["id"] = "%s-%s-B%dH%dx%d-T%d-k%d-%s-m%d%s%s%s-%s" % (
        "seq" if form == 0 else "cs%s" % form, "bwd" if bwd else "fwd", B, H, dirs, T, k, ("id", "tanh", "relu")[act], mask,
        "-um" if up_mul else "", "-ua" if up_add else "", ("-img" + ("-nm" if nx_mul else "")) if img else "", flavour)
    return c


def _matrix():
    out = []
    n = 0
    for form in (0, 4, 8):
        for bwd in (False, True):
            Ts = SEQ_T[bwd] if form == 0 else coop_T(form)
            F = 8 * form
            for T in Ts:
                multi = form != 0 and T > F
                for k in (3, 4):
                    n += 1
                    # the covering design: shape, activation, mask mode, the two upstream riders and the flavour rotate with co-prime periods
                    flavour = ("long" if (n % 2 == 0 or T == 2 * F + 5) else "saturated" if n % 3 == 0 else "normal") if multi else \
                        ("normal", "saturated", "long")[n % 3]
                    shape = SHAPES[1] if (form != 0 and T == 2 * F + 5) else SHAPES[n % 3]      # the mutation check's shape: both directions
                    out.append(case(form, bwd, shape, T, k, (TANH, RELU)[(n // 2) % 2], n % 3, bwd and n % 4 < 2, bwd and (n // 3) % 2 == 0, flavour))
    return out


def _img_matrix():
    out = []
    n = 0
    for form in (4, 8):
        for bwd in (False, True):
            for T in img_T(form):
                for k in (3, 4):
                    for shape in IMG_SHAPES:
                        n += 1
                        out.append(case(form, bwd, shape, T, k, (TANH, RELU)[n % 2], (n // 2) % 3, bwd and n % 3 == 0, bwd and n % 4 == 1,
                                        ("normal", "long", "saturated")[n % 3], img=True, nx_mul=(not bwd) and n % 2 == 0))
    return out


MATRIX = _matrix()
IMG_MATRIX = _img_matrix()
# either side of the automatic 8 / 4-wave threshold (two workgroups per CU): 512 workgroups on 256 CUs, and one sequence more
THRESHOLD = [case("auto", bwd, (B, 512, 2), 8, 4, RELU, 0, False, False, "normal") for B in (32, 33) for bwd in (False, True)]
CHAINED = [case(form, True, SHAPES[1], {0: 25, 4: 69, 8: 133}[form], 3, act, 2, True, True, "long") for form in (0, 4, 8) for act in (RELU, TANH)]
_BY_ID = {}
for _c in MATRIX + IMG_MATRIX + THRESHOLD + CHAINED:
    assert _c["id"] not in _BY_ID, _c["id"]
    _BY_ID[_c["id"]] = _c

# census slots that no case of this file reaches (with the reason): must stay empty
UNREACHED = {}


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def f32(a):
    return np.asarray(a, dtype=np.float32)


def philox_keep_seq(key0, key1, p, B, n, seq_mul, seq_add):
    """[B][n] bool of the scans' Philox stream: (sequence seq_add + seq_mul * b, column) kept iff word 0 >= p * 2^32."""
    th = float(np.float32(p)) * 4294967296.0
    thresh = 4294967295 if th >= 4294967295.0 else int(th)
    seq = (seq_add + seq_mul * np.arange(B, dtype=np.uint64))[:, None]
    col = np.arange(n, dtype=np.uint64)[None, :]
    w = philox4x32_10(np.broadcast_to(seq, (B, n)), np.broadcast_to(col, (B, n)), 0x243F6A88, 0x85A308D3, key0, key1)
    return w[0] >= np.uint64(thresh)


KEEP_SCALE = np.float32(1.0) / (np.float32(1.0) - np.float32(P_DROP))      # 1.f / (1.f - p) of the launch code


@functools.lru_cache(maxsize=None)
def operands(key):
    """float32 operands of a case, logical layouts: U [B][T][ncols][k], x / dh / up_add [B][T][ncols], bias [2 ncols], tables [B][ncols]."""
    c = _BY_ID[key]
    B, T, H, dirs, k = c["B"], c["T"], c["H"], c["dirs"], c["k"]
    nc = H * dirs
    rs = np.random.RandomState(zlib.crc32(("%d-%d-%d-%d-%d-%s" % (B, T, H, dirs, k, c["flavour"])).encode()))
    Uu = rs.randn(B, T, nc, k)
    bias = 0.1 * rs.randn(2 * nc)
    if c["flavour"] == "long":            # f ~ 0.98: the carried state crosses every block boundary at nearly full weight
        Uu[..., 1] *= 0.1
        bias[:nc] = 4.0
    if c["flavour"] == "saturated":       # a third of the columns: pre-activations of exactly +-100 -> f = 1 / 0, r = 0 / 1
        cols = np.arange(nc)
        sat = cols % 3 == 0
        sf = np.where((cols // 3) % 2 == 0, 100.0, -100.0)
        sr = np.where((cols // 6) % 2 == 0, -100.0, 100.0)
        bias[:nc][sat] = 0.0
        bias[nc:][sat] = 0.0
        Uu[..., 1] = np.where(sat, sf, Uu[..., 1])
        Uu[..., 2] = np.where(sat, sr, Uu[..., 2])
    ops = dict(U=f32(Uu), bias=f32(bias), x=f32(rs.randn(B, T, nc)), dh=f32(rs.randn(B, T, nc)),
               mask=f32(rs.rand(B, nc) >= P_DROP), up_mul=f32(rs.rand(B, nc) >= 0.25) * np.float32(1.0 / 0.75),
               up_add=f32(rs.randn(B, T, nc)), nx_mul=f32(rs.rand(B, nc) >= 0.25) * np.float32(1.0 / 0.75))
    return ops


def mask_values(c, ops):
    """[B][ncols] float32 multipliers of the output dropout, as the kernels form them."""
    B, nc = c["B"], c["H"] * c["dirs"]
    if c["mask"] == 0:
        return np.ones((B, nc), np.float32)
    keep = ops["mask"] != 0 if c["mask"] == 1 else philox_keep_seq(KEYS[0], KEYS[1], P_DROP, B, nc, SEQ_MUL, SEQ_ADD)
    return np.where(keep, KEEP_SCALE, np.float32(0.0)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the float64 reference with its running error scale
# ---------------------------------------------------------------------------------------------------------------------
def walk(a, H):
    """[B][T][ncols]... <-> [T][B][ncols]... in the order the forward recurrence visits the frames (columns >= H: time reversed); an
    involution up to the transpose, `unwalk` undoes it."""
    w = np.array(np.moveaxis(a, 1, 0))
    w[:, :, H:] = w[::-1, :, H:]
    return w


def unwalk(w, H):
    a = np.array(w)
    a[:, :, H:] = a[::-1, :, H:]
    return np.moveaxis(a, 0, 1)


def sigmoid64(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def gate(u, b):
    """exact sigmoid(u + b) of the float32 inputs, and its error scale: SIG_ULPS of the value plus the float32 rounding of the pre-activation."""
    z = u.astype(np.float64) + b.astype(np.float64)
    g = sigmoid64(z)
    return g, SIG_ULPS * g + 0.5 * np.abs(z) * g * (1.0 - g)


def act64(c, act):
    """act(c), the scale of its own rounding given an exact argument, and |act'(c)|."""
    if act == TANH:
        v = np.tanh(c)
        return v, TANH_ULPS * np.abs(v), 1.0 - v * v
    if act == RELU:
        return np.maximum(c, 0.0), np.zeros_like(c), np.ones_like(c)      # (slope 1 on both sides: a kink moved by an error e moves the value by <= e)
    return c, np.zeros_like(c), np.ones_like(c)


def ref_forward(c, ops):
    """c, h [B][T][ncols] in float64 and their error scales."""
    H, k, T = c["H"], c["k"], c["T"]
    nc = H * c["dirs"]
    Uw = walk(ops["U"], H)
    u0 = Uw[..., 0].astype(np.float64)
    f, ef = gate(Uw[..., 1], ops["bias"][:nc])
    r, er = gate(Uw[..., 2], ops["bias"][nc:])
    xp = (walk(ops["x"], H) if k == 3 else Uw[..., 3]).astype(np.float64)
    mk = mask_values(c, ops).astype(np.float64)
    cs, hs, Sc, Sh = (np.zeros(u0.shape) for _ in range(4))
    cp, Sp = np.zeros(u0.shape[1:]), np.zeros(u0.shape[1:])
    for t in range(T):
        d = cp - u0[t]
        cc = d * f[t] + u0[t]
        S = f[t] * Sp + np.abs(d) * (ef[t] + f[t]) + np.abs(cc)
        a, Sa0, slope = act64(cc, c["act"])
        Sa = slope * S + Sa0
        val = a * mk
        Sval = mk * Sa + np.abs(val)
        hh = (val - xp[t]) * r[t] + xp[t]
        cs[t], Sc[t], hs[t] = cc, S, hh
        Sh[t] = r[t] * Sval + np.abs(val - xp[t]) * (er[t] + r[t]) + np.abs(hh)
        cp, Sp = cc, S
    return dict(c=unwalk(cs, H), h=unwalk(hs, H), S_c=unwalk(Sc, H), S_h=unwalk(Sh, H), r=unwalk(r, H), xp=unwalk(xp, H))


def ref_backward(c, ops, c32):
    """dU [B][T][ncols][k], dx [B][T][ncols] (k == 3), dbias [B][2 ncols] in float64 from the float32 stash c32, and their error scales."""
    H, k, T, B = c["H"], c["k"], c["T"], c["B"]
    nc = H * c["dirs"]
    Uw = walk(ops["U"], H)
    u0 = Uw[..., 0].astype(np.float64)
    f, ef = gate(Uw[..., 1], ops["bias"][:nc])
    r, er = gate(Uw[..., 2], ops["bias"][nc:])
    xp = (walk(ops["x"], H) if k == 3 else Uw[..., 3]).astype(np.float64)
    mk = mask_values(c, ops).astype(np.float64)
    cw = walk(np.asarray(c32, np.float32), H).astype(np.float64)
    um = ops["up_mul"].astype(np.float64) if c["up_mul"] else np.ones((B, nc))
    ua = walk(ops["up_add"], H).astype(np.float64) if c["up_add"] else np.zeros(u0.shape)
    dhw = walk(ops["dh"], H).astype(np.float64)
    out = {n: np.zeros(u0.shape) for n in ("du0", "du1", "du2", "dxp", "S0", "S1", "S2", "S3")}
    dc, Sdc = np.zeros(u0.shape[1:]), np.zeros(u0.shape[1:])
    db = [np.zeros((B, nc)) for _ in range(2)]
    Sdb = [np.zeros((B, nc)) for _ in range(2)]
    ab = [np.zeros((B, nc)) for _ in range(2)]
    for t in range(T - 1, -1, -1):
        dh = dhw[t] * um + ua[t]
        Sdh = np.abs(dh)
        cprev = cw[t - 1] if t > 0 else np.zeros(u0.shape[1:])
        val, Sv, _ = act64(cw[t], c["act"])
        if c["act"] == TANH:
            da = 1.0 - val * val
            Sda = 2.0 * np.abs(val) * Sv + val * val + np.abs(da)
        else:
            da = (cw[t] > 0).astype(np.float64) if c["act"] == RELU else np.ones_like(val)
            Sda = np.zeros_like(val)
        gm = dh * r[t] * mk
        Sgm = 2.0 * np.abs(gm) + (Sdh * r[t] + np.abs(dh) * er[t]) * mk
        dct = gm * da + dc
        Sdct = Sgm * np.abs(da) + np.abs(gm) * Sda + Sdc + np.abs(dct)
        omf, omr = 1.0 - f[t], 1.0 - r[t]
        du0 = dct * omf
        out["S0"][t] = Sdct * omf + np.abs(dct) * (ef[t] + omf) + np.abs(du0)
        dd = cprev - u0[t]
        df = dct * dd
        Sdf = Sdct * np.abs(dd) + np.abs(dct) * np.abs(dd) + np.abs(df)
        du1 = df * f[t] * omf
        out["S1"][t] = Sdf * f[t] * omf + np.abs(df) * (ef[t] * omf + f[t] * (ef[t] + omf)) + 2.0 * np.abs(du1)
        inner = val * mk - xp[t]
        Sin = Sv * mk + np.abs(inner)
        dr = dh * inner
        Sdr = Sdh * np.abs(inner) + np.abs(dh) * Sin + np.abs(dr)
        du2 = dr * r[t] * omr
        out["S2"][t] = Sdr * r[t] * omr + np.abs(dr) * (er[t] * omr + r[t] * (er[t] + omr)) + 2.0 * np.abs(du2)
        dxp = dh * omr
        out["S3"][t] = Sdh * omr + np.abs(dh) * (er[t] + omr) + np.abs(dxp)
        out["du0"][t], out["du1"][t], out["du2"][t], out["dxp"][t] = du0, du1, du2, dxp
        dc_new = dct * f[t]
        Sdc = Sdct * f[t] + np.abs(dct) * ef[t] + np.abs(dc_new)
        dc = dc_new
        for j, (v, S) in enumerate(((du1, out["S1"][t]), (du2, out["S2"][t]))):
            db[j] += v
            Sdb[j] += S
            ab[j] += np.abs(v)
    names = ["du0", "du1", "du2"] + (["dxp"] if k == 4 else [])
    res = dict(dU=np.stack([unwalk(out[n], H) for n in names], axis=-1),
               S_dU=np.stack([unwalk(out[s], H) for s in ("S0", "S1", "S2", "S3")[:k]], axis=-1))
    if k == 3:
        res["dx"], res["S_dx"] = unwalk(out["dxp"], H), unwalk(out["S3"], H)
    # a sum of T terms in any order: every term passes through at most T - 1 additions
    res["dbias"] = np.concatenate(db, axis=1)
    res["S_dbias"] = np.concatenate([Sdb[j] + (T - 1) * ab[j] for j in range(2)], axis=1)
    return res


@functools.lru_cache(maxsize=None)
def reference_fwd(key):
    return ref_forward(_BY_ID[key], operands(key))


def judge(tag, kind, got, ref, S, T, ulps=None, rms_lim=None):
    """Failure messages of one tensor against its float64 reference (prints the measured figures first).  T: frames of the case."""
    got = np.asarray(got, np.float64)
    fails = []
    if not np.isfinite(got).all():
        return ["%s: %s holds %d non-finite elements" % (tag, kind, int((~np.isfinite(got)).sum()))]
    ratio = np.abs(got - ref) / (U * S + FTZ * T)
    worst, rms = float(ratio.max()), float(np.sqrt(np.mean(ratio * ratio)))
    print("SRUSTAT %s %s worst %.4f rms %.4f" % (tag, kind, worst, rms))
    ulps = ULPS[kind] if ulps is None else ulps
    rms_lim = RMS_LIM[kind] if rms_lim is None else rms_lim
    if worst > ulps:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        fails.append("%s: %s%s = %.9g, float64 %.9g: %.2f x 2^-24 x S (limit %.2f)" % (tag, kind, list(i), got[i], ref[i], worst, ulps))
    if rms > rms_lim:
        fails.append("%s: %s rms %.3f x 2^-24 x S (limit %.3f)" % (tag, kind, rms, rms_lim))
    return fails


# ---------------------------------------------------------------------------------------------------------------------
# a float32 model of the cooperative association and its mutations (host)
# ---------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def act32(c, act):
    return np.tanh(c).astype(np.float32) if act == TANH else np.maximum(c, np.float32(0)) if act == RELU else c


MUTATIONS = ("carry", "order", "shift", "cprev", "tail")


def _model_inputs(c, ops, mut):
    H, k = c["H"], c["k"]
    nc = H * c["dirs"]
    U_, x_ = ops["U"], ops["x"]
    if mut == "shift":        # the flipped direction reads the frame next to the one it should (t = T - tt instead of T - 1 - tt)
        U_, x_ = U_.copy(), x_.copy()
        U_[:, :-1, H:] = ops["U"][:, 1:, H:]
        x_[:, :-1, H:] = ops["x"][:, 1:, H:]
    Uw = walk(U_, H)
    f = sigmoid64(Uw[..., 1].astype(np.float64) + ops["bias"][:nc].astype(np.float64)).astype(np.float32)
    r = sigmoid64(Uw[..., 2].astype(np.float64) + ops["bias"][nc:].astype(np.float64)).astype(np.float32)
    xp = walk(x_, H) if k == 3 else Uw[..., 3]
    return Uw[..., 0], f, r, xp, mask_values(c, ops)


def _compose(comps, carry, mut):
    """incoming state of every wave and the state behind the block, from the waves' (product, end state) composites"""
    cin, allv = [], carry
    order = range(len(comps))
    if mut == "order":        # the composites applied last wave first
        order = reversed(order)
    for w in order:
        cin.append(allv)
        allv = fma32(comps[w][0], allv, comps[w][1])
    if mut == "order":
        cin.reverse()
    return cin, allv


def model_forward(c, ops, nw, mut=None):
    """float32 c, h [B][T][ncols] by the association of sru_fwd_cs_kernel<nw>."""
    H, T = c["H"], c["T"]
    u0, f, r, xp, mk = _model_inputs(c, ops, mut)
    one, zero = np.ones(u0.shape[1:], np.float32), np.zeros(u0.shape[1:], np.float32)
    cs, hs = np.zeros(u0.shape, np.float32), np.zeros(u0.shape, np.float32)
    FBT = 8 * nw
    carry = zero
    for i in range(cdiv(T, FBT)):
        comps, loc = [], []
        for w in range(nw):
            cc, p, cl, P = zero, one, [], []
            for q in range(8):
                tt = i * FBT + w * 8 + q
                ix = min(tt, T - 1)
                fq = f[ix] if (tt < T or mut == "tail") else one      # (mutation: a frame past T is walked like a frame)
                cc = fma32(cc - u0[ix], fq, u0[ix])
                p = p * fq
                cl.append(cc)
                P.append(p)
            comps.append((p, cc))
            loc.append((cl, P))
        cin, allv = _compose(comps, zero if mut == "carry" else carry, mut)
        carry = allv
        for w in range(nw):
            for q in range(8):
                tt = i * FBT + w * 8 + q
                if tt >= T and mut != "tail":
                    continue
                ix = min(tt, T - 1)      # (mutation: ... and stored where its clamped loads came from)
                cq = fma32(loc[w][1][q], cin[w], loc[w][0][q])
                val = act32(cq, c["act"]) * mk
                hs[ix], cs[ix] = fma32(val - xp[ix], r[ix], xp[ix]), cq
    return unwalk(cs, H), unwalk(hs, H)


def model_backward(c, ops, c32, nw, mut=None):
    """float32 dU[.., 0..2] [B][T][ncols][3] by the association of sru_bwd_cs_kernel<nw>."""
    H, T, k, B = c["H"], c["T"], c["k"], c["B"]
    nc = H * c["dirs"]
    u0, f, r, xp, mk = _model_inputs(c, ops, mut)
    cw = walk(np.asarray(c32, np.float32), H)
    um = ops["up_mul"] if c["up_mul"] else np.ones((B, nc), np.float32)
    ua = walk(ops["up_add"], H) if c["up_add"] else np.zeros(u0.shape, np.float32)
    dhw = walk(ops["dh"], H)
    one, zero = np.ones(u0.shape[1:], np.float32), np.zeros(u0.shape[1:], np.float32)
    o = np.zeros(u0.shape + (4,), np.float32)
    FBT = 8 * nw
    carry = zero
    flip = np.arange(nc) >= H
    for i in range(cdiv(T, FBT)):
        comps, loc = [], []
        for w in range(nw):
            dc, p, rows = zero, one, []
            for q in range(8):
                s = i * FBT + w * 8 + q
                inn = s < T or mut == "tail"
                ix = max(T - 1 - s, 0)
                fq = f[ix] if inn else one
                dh = fma32(dhw[ix], um, ua[ix]) if inn else zero
                cprev = cw[ix - 1] if ix > 0 else zero
                if mut == "cprev" and ix + 1 < T:      # the flipped direction takes the frame on the other side
                    cprev = np.where(flip, cw[ix + 1], cprev)
                val = act32(cw[ix], c["act"])
                da = (one - val * val) if c["act"] == TANH else (cw[ix] > 0).astype(np.float32) if c["act"] == RELU else one
                gm = (dh * r[ix]) * mk
                Q = p
                dl = fma32(gm, da, dc)
                dc = dl * fq
                p = p * fq
                rows.append((ix, Q, dl, fq, dh, val, cprev, s))
            comps.append((p, dc))
            loc.append(rows)
        din, allv = _compose(comps, zero if mut == "carry" else carry, mut)
        carry = allv
        for w in range(nw):
            for ix, Q, dl, fq, dh, val, cprev, s in loc[w]:
                if s >= T and mut != "tail":
                    continue
                dct = fma32(Q, din[w], dl)
                dr = dh * fma32(val, mk, -xp[ix])
                df = dct * (cprev - u0[ix])
                o[ix, ..., 0] = dct * (one - fq)
                o[ix, ..., 1] = (df * fq) * (one - fq)
                o[ix, ..., 2] = (dr * r[ix]) * (one - r[ix])
                o[ix, ..., 3] = dh * (one - r[ix])
    return unwalk(o, H)[..., :3]


def _worst(got, ref, S, T):
    return float((np.abs(np.asarray(got, np.float64) - ref) / (U * S + FTZ * T)).max())


def mutation_ratios(nw):
    """{(mutation or None, tensor): worst |model - float64| / (2^-24 S)} on the long-memory 2F + 5 cases of the matrix."""
    F = 8 * nw
    res = {}
    for bwd in (False, True):
        cs_ = [c for c in MATRIX if c["form"] == nw and c["bwd"] == bwd and c["T"] == 2 * F + 5]
        assert cs_ and all(c["flavour"] == "long" and c["dirs"] == 2 for c in cs_)
        for c in cs_:
            ops = operands(c["id"])
            fw = reference_fwd(c["id"])
            c32 = fw["c"].astype(np.float32)
            rb = ref_backward(c, ops, c32) if bwd else None
            for mut in (None,) + MUTATIONS:
                if bwd:
                    res.setdefault((mut, "dU"), []).append(_worst(model_backward(c, ops, c32, nw, mut), rb["dU"][..., :3], rb["S_dU"][..., :3], c["T"]))
                elif mut != "cprev":
                    mc, mh = model_forward(c, ops, nw, mut)
                    res.setdefault((mut, "c"), []).append(_worst(mc, fw["c"], fw["S_c"], c["T"]))
                    res.setdefault((mut, "h"), []).append(_worst(mh, fw["h"], fw["S_h"], c["T"]))
    return {key: min(v) if key[0] else max(v) for key, v in res.items()}


# ---------------------------------------------------------------------------------------------------------------------
# host checks
# ---------------------------------------------------------------------------------------------------------------------
HELPER_SLOTS = [INPUT_MASK, INPUT_DROPOUT, DX_ADV_FINISH]      # reached by the helper tests below


def test_matrix_reaches_every_kernel():
    reached = collections.Counter()
    for c in MATRIX + IMG_MATRIX + CHAINED:
        for i, n in enumerate(expected_counts(c, c["bwd"], c["img"])):
            reached[i] += n
        if c in CHAINED or (c["img"] and c["bwd"]):      # the chained cases also run the forward, the backward image cases the float32 instantiation
            for i, n in enumerate(expected_counts(c, c["img"], False)):
                reached[i] += n
    for s in HELPER_SLOTS:
        reached[s] += 1
    assert UNREACHED == {}
    assert sorted(i for i in range(NSLOTS) if not reached[i]) == sorted(UNREACHED)
    # every (form, T) of the issue occurs with both k, in both passes; every image case with both k, both passes, both shapes
    for form in (0, 4, 8):
        for bwd in (False, True):
            for T in (SEQ_T[bwd] if form == 0 else coop_T(form)):
                assert {c["k"] for c in MATRIX if (c["form"], c["bwd"], c["T"]) == (form, bwd, T)} == {3, 4}, (form, bwd, T)
    for form in (4, 8):
        for T in img_T(form):
            got = {(c["bwd"], c["k"], c["B"]) for c in IMG_MATRIX if (c["form"], c["T"]) == (form, T)}
            assert len(got) == 8, (form, T)
        multi = [c for c in MATRIX if c["form"] == form and c["T"] > 8 * form]
        assert 2 * sum(c["flavour"] == "long" for c in multi) >= len(multi)
    for dims in ("mask", "act", "up_mul", "up_add", "flavour"):
        for form in (0, 4, 8):
            want = {"mask": {0, 1, 2}, "act": {TANH, RELU}, "up_mul": {False, True}, "up_add": {False, True},
                    "flavour": {"normal", "long", "saturated"}}[dims]
            assert {c[dims] for c in MATRIX if c["form"] == form and (c["bwd"] or dims not in ("up_mul", "up_add"))} == want, (dims, form)


def test_expected_counts_model_the_launcher():
    c = case("auto", False, (32, 512, 2), 8, 4, RELU, 0, False, False, "normal")
    assert expected_counts(c, False, False, 256)[FWD_CS + 2] == 1 and expected_counts(c, True, False, 256)[BWD_CS + 2] == 1
    assert expected_counts(dict(c, B=33), False, False, 256)[FWD_CS] == 1 and expected_counts(dict(c, B=33), False, False, 304)[FWD_CS + 2] == 1
    assert expected_counts(dict(c, form=0), True, False)[BWD] == 1
    assert expected_counts(dict(c, form=4), True, True)[BWD_CS + 1] == 1 and expected_counts(dict(c, form=8), False, True)[FWD_CS + 3] == 1
    for bad in (dict(c, form=0), dict(c, form=8, T=12), dict(c, form=4, H=96)):
        with pytest.raises(Invalid):
            expected_counts(bad, False, True)


def test_philox_stream_of_the_scans():
    k = philox_keep_seq(KEYS[0], KEYS[1], P_DROP, 64, 300, SEQ_MUL, SEQ_ADD)
    assert 0.67 < k.mean() < 0.73
    # sequence b of (mul 2, add 1) is sequence 2 b + 1 of the plain stream
    assert np.array_equal(k[:10], philox_keep_seq(KEYS[0], KEYS[1], P_DROP, 21, 300, 1, 0)[1::2])


@pytest.mark.parametrize("nw", [4, 8])
def test_limits_reject_mutations_of_the_cooperative_association(nw):
    """A float32 numpy model of the cooperative association passes the limits; with the block carry dropped, the wave composites composed
    in the wrong order, the flipped direction shifted by one frame, c_prev of the flipped direction taken from the wrong neighbour, or a
    frame past T walked (and stored) like a frame it exceeds them at least MUTATION_MARGIN-fold, on the long-memory inputs of the
    three-block ragged case (T = 2 F + 5)."""
    res = mutation_ratios(nw)
    for (mut, kind), v in sorted(res.items(), key=str):
        print("SRUMUT nw %d %s %s %.4g (limit %.2f)" % (nw, mut, kind, v, ULPS[kind]))
    for (mut, kind), v in res.items():
        if mut is None:
            assert v <= ULPS[kind], (kind, v)
        else:
            assert v >= MUTATION_MARGIN * ULPS[kind], (mut, kind, v)


# ---------------------------------------------------------------------------------------------------------------------
# running a case on the device
# ---------------------------------------------------------------------------------------------------------------------
def _set_knobs(kn):
    from gantts_amd import _lib as Lb
    for k, v in kn.items():
        Lb.check(Lb.lib.gt_set_tuning(k.encode(), int(v)))


def _stream():
    return Ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _census(fn, knobs):
    """Runs fn() with the knobs set and the census reset; (rc, counts)."""
    from gantts_amd import _lib as Lb
    counts = (Ct.c_int64 * Lb.SRU_PATH_SLOTS)()
    torch.cuda.synchronize()
    _set_knobs(dict(KNOBS, **knobs))
    try:
        Lb.check(Lb.lib.gt_sru_path_counts(None, 1))
        rc = fn()
        Lb.check(Lb.lib.gt_sru_path_counts(counts, 1))
    finally:
        _set_knobs(KNOBS)
    torch.cuda.synchronize()
    return rc, list(counts)


NAN = np.float32(np.nan)


def _in(a, cols, pad=3, off=1):
    """input matrix [rows][cols] at a pitch larger than its width, NaN in the pads"""
    a = np.ascontiguousarray(a, np.float32).reshape(-1, cols)
    return _F32(a, cols + pad, off, NAN)


def _out(rows, cols, ld=None, off=1):
    """result matrix filled with NaN inside a field of sentinels"""
    return _F32(np.full((rows, cols), NAN, np.float32), cols if ld is None else ld, off, SENT)


def run_scan(c, ops, bwd, img=False, c_stash=None, want_t=True, form=None):
    """One gt_op_sru_scan launch.  Returns (rc, counts, {name: (flat, logical, buffer)})."""
    from gantts_amd import _lib as Lb
    B, T, H, dirs, k = c["B"], c["T"], c["H"], c["dirs"], c["k"]
    nc, N = H * dirs, B * T
    g = Lb.SruScanCase()
    g.backward, g.B, g.T, g.H, g.dirs, g.k, g.act = int(bwd), B, T, H, dirs, k, c["act"]
    g.mask_mode, g.keep_scale, g.p = c["mask"], float(KEEP_SCALE), P_DROP
    g.key0, g.key1, g.seq_mul, g.seq_add = KEYS[0], KEYS[1], SEQ_MUL, SEQ_ADD
    ins = dict(U=_in(ops["U"], nc * k), bias=_in(ops["bias"], 2 * nc, pad=0, off=0))
    g.ldu = ins["U"].ld
    if k == 3:
        ins["x"] = _in(ops["x"], nc)
        g.ldx = ins["x"].ld
    if c["mask"] == 1:
        ins["mask"] = _in(ops["mask"], nc, pad=0, off=0)
    outs = {}
    if not bwd:
        outs["h"], outs["c"] = _out(N, nc), _out(N, nc)
        if img:
            outs["nx_b"] = _I16(N, nc, nc + 8)
            g.ld_nxb = nc + 8
            if want_t:
                outs["nx_bt"] = _I16(nc, N, N + 16)
                g.ld_nxbt = N + 16
            if c["nx_mul"]:
                ins["nx_mul"] = _in(ops["nx_mul"], nc, pad=0, off=0)
    else:
        ins["c"] = _in(c_stash, nc, pad=0, off=1)
        ins["dh"] = _in(ops["dh"], nc, pad=0, off=1)
        if c["up_mul"]:
            ins["up_mul"] = _in(ops["up_mul"], nc, pad=0, off=0)
        if c["up_add"]:
            ins["up_add"] = _in(ops["up_add"], nc)
            g.ld_up_add = ins["up_add"].ld
        outs["dU"] = _out(N, nc * k, ld=g.ldu)
        outs["dbias_part"] = _out(B, 2 * nc)
        if k == 3:
            outs["dx"] = _out(N, nc, ld=nc + 5)
            g.lddx = nc + 5
        if img:
            outs["dU_b"] = _I16(N, nc * k, nc * k + 8)
            g.ld_dub = nc * k + 8
            if want_t:
                outs["dU_bt"] = _I16(nc * k, N, N + 16)
                g.ld_dubt = N + 16
    for name, b in list(ins.items()) + list(outs.items()):
        setattr(g, name, b.ptr)
    rc, counts = _census(lambda: Lb.lib.gt_op_sru_scan(Ct.byref(g), _stream()), knobs_of(c["form"] if form is None else form))
    return rc, counts, {name: b.got() + (b,) for name, b in outs.items()}


def _sentinels(tag, out):
    return ["%s: %s written outside its result" % (tag, name) for name, (flat, _, buf) in out.items()
            if not pads_intact(flat, buf.inside(), SENT if flat.dtype == np.float32 else PAD16)]


def _ok(tag, rc):
    from gantts_amd import _lib as Lb
    if rc == Lb.GT_ERR_HIP:      # a device error: nothing more is launched in this session
        pytest.exit("%s: %s" % (tag, Lb.lib.gt_last_error()), returncode=3)
    assert rc == Lb.GT_OK, "%s: %s" % (tag, Lb.lib.gt_last_error())


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def check_forward(tag, c, ops, out, fw):
    B, T, nc = c["B"], c["T"], c["H"] * c["dirs"]
    fails = judge(tag, "c", out["c"][1].reshape(B, T, nc), fw["c"], fw["S_c"], T)
    fails += judge(tag, "h", out["h"][1].reshape(B, T, nc), fw["h"], fw["S_h"], T)
    if c["mask"] == 2:      # dropped columns of the numpy stream: h = x' (1 - r)
        drop = np.broadcast_to((mask_values(c, ops) == 0)[:, None, :], (B, T, nc))
        if drop.any():
            want = fw["xp"] * (1.0 - fw["r"])
            fails += judge(tag + "[dropped]", "h", out["h"][1].reshape(B, T, nc)[drop], want[drop], fw["S_h"][drop], T)
    return fails


def check_backward(tag, c, ops, out, rb, img=False):
    B, T, k, nc = c["B"], c["T"], c["k"], c["H"] * c["dirs"]
    fails = []
    if not img:
        dU = out["dU"][1].reshape(B, T, nc, k)
        fails += judge(tag, "dU", dU, rb["dU"], rb["S_dU"], T)
        if c["mask"] == 2 and not c["up_add"]:      # a dropped column passes no gradient into its cell: dU[.., 0..1] is exactly 0
            drop = mask_values(c, ops) == 0
            if drop.any() and not (np.broadcast_to(drop[:, None, :, None], dU[..., :2].shape) <= (dU[..., :2] == 0)).all():
                fails.append("%s: dU[.., 0..1] of a dropped column is not exactly 0" % tag)
    if k == 3:
        fails += judge(tag, "dx", out["dx"][1].reshape(B, T, nc), rb["dx"], rb["S_dx"], T)
    fails += judge(tag, "dbias", out["dbias_part"][1], rb["dbias"], rb["S_dbias"], T)
    return fails


def bf16_bits(a):
    """round-to-nearest-even bf16 of float32 values, as 16-bit patterns"""
    return (_bf16(np.ascontiguousarray(a, np.float32)).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


# ---------------------------------------------------------------------------------------------------------------------
# the scans against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", MATRIX, ids=[c["id"] for c in MATRIX])
def test_scan_case_vs_float64(c):
    tag, ops = c["id"], operands(c["id"])
    fw = reference_fwd(tag)
    stash = fw["c"].astype(np.float32)
    rc, counts, out = run_scan(c, ops, c["bwd"], c_stash=stash)
    _ok(tag, rc)
    assert counts == expected_counts(c, c["bwd"], False, _cus()), "%s: launches %s" % (tag, counts)
    fails = _sentinels(tag, out)
    fails += check_backward(tag, c, ops, out, ref_backward(c, ops, stash)) if c["bwd"] else check_forward(tag, c, ops, out, fw)
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CHAINED, ids=[c["id"] for c in CHAINED])
def test_backward_from_the_forward_kernels_own_stash(c):
    """forward kernel -> its float32 c -> backward kernel, judged against the reference evaluated on that same c"""
    tag, ops = c["id"], operands(c["id"])
    rc, counts, fo = run_scan(c, ops, False)
    _ok(tag, rc)
    assert counts == expected_counts(c, False, False, _cus()), counts
    fails = _sentinels(tag, fo) + check_forward(tag, c, ops, fo, reference_fwd(tag))
    stash = fo["c"][1].reshape(c["B"], c["T"], -1)
    rc, counts, out = run_scan(c, ops, True, c_stash=stash)
    _ok(tag, rc)
    assert counts == expected_counts(c, True, False, _cus()), counts
    fails += _sentinels(tag, out) + check_backward(tag, c, ops, out, ref_backward(c, ops, stash))
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("c", THRESHOLD, ids=[c["id"] for c in THRESHOLD])
def test_automatic_wave_count_either_side_of_two_workgroups_per_cu(c):
    if _cus() != CUS:
        pytest.skip("the threshold shapes are derived for %d CUs, this device has %d" % (CUS, _cus()))
    tag, ops = c["id"], operands(c["id"])
    assert waves_of("auto", c["B"], c["H"] * c["dirs"], _cus()) == (8 if c["B"] == 32 else 4)
    fw = reference_fwd(tag)
    stash = fw["c"].astype(np.float32)
    rc, counts, out = run_scan(c, ops, c["bwd"], c_stash=stash)
    _ok(tag, rc)
    assert counts == expected_counts(c, c["bwd"], False, _cus()), "%s: launches %s" % (tag, counts)
    fails = _sentinels(tag, out)
    fails += check_backward(tag, c, ops, out, ref_backward(c, ops, stash)) if c["bwd"] else check_forward(tag, c, ops, out, fw)
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("c", IMG_MATRIX, ids=[c["id"] for c in IMG_MATRIX])
def test_image_case_is_exact(c):
    """The bf16 images bit for bit: nx_b / nx_bt = bf16(float32(h * nx_mul)) of the h the same launch wrote; dU_b / dU_bt = bf16 of the
    float32 dU of the non-image instantiation with the same wave count (the same explicit fmaf / __fmul_rn chain); k = 3: the same dx."""
    tag, ops = c["id"], operands(c["id"])
    B, T, k, nc = c["B"], c["T"], c["k"], c["H"] * c["dirs"]
    N = B * T
    fw = reference_fwd(tag)
    stash = fw["c"].astype(np.float32)
    rc, counts, out = run_scan(c, ops, c["bwd"], img=True, c_stash=stash)
    _ok(tag, rc)
    assert counts == expected_counts(c, c["bwd"], True, _cus()), "%s: launches %s" % (tag, counts)
    fails = _sentinels(tag, out)
    if not c["bwd"]:
        fails += check_forward(tag, c, ops, out, fw)
        nm = ops["nx_mul"] if c["nx_mul"] else np.ones((B, nc), np.float32)
        want = bf16_bits(out["h"][1].reshape(B, T, nc) * nm[:, None, :]).reshape(N, nc)
        if not np.array_equal(out["nx_b"][1], want):
            fails.append("%s: nx_b differs from bf16(h * nx_mul) in %d elements" % (tag, int((out["nx_b"][1] != want).sum())))
        if not np.array_equal(out["nx_bt"][1], out["nx_b"][1].T):
            fails.append("%s: nx_bt is not nx_b transposed" % tag)
        rc, counts, o2 = run_scan(c, ops, False, img=True, want_t=False)      # the forward of a pass without weight gradients
        _ok(tag, rc)
        assert counts == expected_counts(c, False, True, _cus())
        fails += _sentinels(tag, o2)
        for name in ("h", "c", "nx_b"):
            if not np.array_equal(o2[name][1].view(np.uint16 if name == "nx_b" else np.uint32), out[name][1].view(np.uint16 if name == "nx_b" else np.uint32)):
                fails.append("%s: %s changes when nx_bt is not requested" % (tag, name))
    else:
        rb = ref_backward(c, ops, stash)
        fails += check_backward(tag, c, ops, out, rb, img=True)
        if not np.array_equal(out["dU"][0].view(np.uint32), out["dU"][2].host.view(np.uint32)):
            fails.append("%s: the float32 dU was written although the images were requested" % tag)
        rc, counts, plain = run_scan(c, ops, True, img=False, c_stash=stash)
        _ok(tag, rc)
        assert counts == expected_counts(c, True, False, _cus())
        fails += _sentinels(tag, plain) + check_backward(tag + "[f32]", c, ops, plain, rb)
        want = bf16_bits(plain["dU"][1])
        if not np.array_equal(out["dU_b"][1], want):
            fails.append("%s: dU_b differs from bf16(float32 dU) in %d elements" % (tag, int((out["dU_b"][1] != want).sum())))
        if not np.array_equal(out["dU_bt"][1], out["dU_b"][1].T):
            fails.append("%s: dU_bt is not dU_b transposed" % tag)
        for name in ("dx",) if k == 3 else ():
            if not np.array_equal(out[name][1].view(np.uint32), plain[name][1].view(np.uint32)):
                fails.append("%s: dx differs from the float32 instantiation's" % tag)
        # (dbias_part is judged against float64 in both instantiations, not bit-compared: its running sums dbf += du1 are plain additions
        #  behind a multiplication, which the compiler is free to contract per instantiation -- see profiles/sru_scan_parity.md)
        nd = int((out["dbias_part"][1].view(np.uint32) != plain["dbias_part"][1].view(np.uint32)).sum())
        print("SRUINFO %s dbias_part: %d of %d elements differ in bits from the float32 instantiation's" % (tag, nd, out["dbias_part"][1].size))
        rc, counts, o2 = run_scan(c, ops, True, img=True, c_stash=stash, want_t=False)      # want_w == false: no transposed image
        _ok(tag, rc)
        assert counts == expected_counts(c, True, True, _cus())
        fails += _sentinels(tag, o2)
        if not np.array_equal(o2["dU_b"][1], out["dU_b"][1]):
            fails.append("%s: dU_b changes when dU_bt is null" % tag)
        if k == 3 and not np.array_equal(o2["dx"][1].view(np.uint32), out["dx"][1].view(np.uint32)):
            fails.append("%s: dx changes when dU_bt is null" % tag)
        if not np.array_equal(o2["dU"][0].view(np.uint32), o2["dU"][2].host.view(np.uint32)):
            fails.append("%s: the float32 dU was written (dU_bt null)" % tag)
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------------
# the helper kernels
# ---------------------------------------------------------------------------------------------------------------------
def _one_launch(slot):
    return [1 if i == slot else 0 for i in range(NSLOTS)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,n,inject,seq_mul,seq_add", [(3, 70, False, 2, 1), (5, 257, False, 1, 0), (2, 300, False, 4, 3), (3, 70, True, 2, 1)])
def test_input_mask_is_the_philox_stream(B, n, inject, seq_mul, seq_add):
    from gantts_amd import _lib as Lb
    out = _out(B, n)
    inj = (np.random.RandomState(B * n).rand(B, n) >= 0.4).astype(np.float32)
    injb = _in(inj, n, pad=0, off=0)
    rc, counts = _census(lambda: Lb.lib.gt_op_sru_input_mask(out.ptr, B, n, P_DROP, KEYS[0], KEYS[1], injb.ptr if inject else None, seq_mul, seq_add,
                                                             _stream()), {})
    _ok("input_mask", rc)
    assert counts == _one_launch(INPUT_MASK), counts
    keep = inj != 0 if inject else philox_keep_seq(KEYS[0], KEYS[1], P_DROP, B, n, seq_mul, seq_add)
    want = np.where(keep, KEEP_SCALE, np.float32(0)).astype(np.float32)
    flat, got = out.got()
    assert pads_intact(flat, out.inside(), SENT)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,n", [(3, 5, 37), (2, 1, 300), (1, 260, 1)])
def test_input_dropout_is_the_float32_product(B, T, n):
    from gantts_amd import _lib as Lb
    rs = np.random.RandomState(B + T + n)
    x = rs.randn(B * T, n).astype(np.float32)
    mul = ((rs.rand(B, n) >= 0.3) * KEEP_SCALE).astype(np.float32)
    xb, mb, yb = _in(x, n, pad=4), _in(mul, n, pad=0, off=0), _out(B * T, n, ld=n + 3)
    rc, counts = _census(lambda: Lb.lib.gt_op_sru_input_dropout(xb.ptr, xb.ld, yb.ptr, yb.ld, B, T, n, mb.ptr, _stream()), {})
    _ok("input_dropout", rc)
    assert counts == _one_launch(INPUT_DROPOUT), counts
    flat, got = yb.got()
    want = (x.reshape(B, T, n) * mul[:, None, :]).reshape(B * T, n)
    assert pads_intact(flat, yb.inside(), SENT)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# rows * Da modulo 4 = 1, 2, 3, 0 at Da = 59 (T = 3: a group of four straddles row and sequence boundaries), Da = 1, Da = 60
DX_CASES = [(rows, Da, T, off, mul, hw) for rows, Da, T in ((3, 59, 3), (6, 59, 3), (9, 59, 3), (12, 59, 3), (9, 1, 3), (6, 1, 2), (7, 60, 1), (1030, 1, 5))
            for off, mul, hw in ((0, True, True), (1, True, True), (0, False, True), (1, True, False))]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,Da,T,off,mul,hw", DX_CASES)
def test_dx_adv_finish_vs_float64(rows, Da, T, off, mul, hw):
    """16-byte path (aligned buffer, whole groups) and scalar path (buffer offset by one float; the last, partial group)"""
    from gantts_amd import _lib as Lb
    rs = np.random.RandomState(rows * 64 + Da + off)
    g = rs.randn(rows, Da).astype(np.float32)
    m = ((rs.rand(rows // T, Da) >= 0.3) * KEEP_SCALE).astype(np.float32)
    h = rs.randn(rows, Da).astype(np.float32)
    buf = _F32(g, Da, 4 + off, SENT)      # (the allocation is 256-byte aligned: offset 4 keeps 16 bytes, 5 breaks them)
    mb, hb = _in(m, Da, pad=5), _in(h, Da, pad=2)
    rc, counts = _census(lambda: Lb.lib.gt_op_sru_dx_adv_finish(buf.ptr, rows, Da, T, mb.ptr if mul else None, mb.ld, hb.ptr if hw else None, hb.ld,
                                                                _stream()), {})
    _ok("dx_adv_finish", rc)
    assert buf.ptr % 16 == (0 if off == 0 else 4)
    assert counts == _one_launch(DX_ADV_FINISH), counts
    flat, got = buf.got()
    assert pads_intact(flat, buf.inside(), SENT)
    want = g.astype(np.float64) * (np.repeat(m, T, axis=0).astype(np.float64) if mul else 1.0) + (h.astype(np.float64) if hw else 0.0)
    assert np.isfinite(got).all()
    assert (np.abs(got - want) <= np.spacing(np.abs(want).astype(np.float32))).all()


@pytest.mark.gpu
def test_hooks_reject_malformed_cases():
    from gantts_amd import _lib as Lb
    lib = Lb.lib
    c = MATRIX[0]
    ops = operands(c["id"])
    assert lib.gt_op_sru_scan(None, None) == Lb.GT_ERR_INVALID
    assert lib.gt_sru_path_counts(None, 1) == Lb.GT_OK
    nc, N = c["H"] * c["dirs"], c["B"] * c["T"]
    buf = torch.zeros(max(N * nc * 4, 4096) + 64, dtype=torch.float32, device="cuda")

    def mk(**kw):
        g = Lb.SruScanCase()
        g.B, g.T, g.H, g.dirs, g.k, g.act = c["B"], c["T"], c["H"], c["dirs"], 4, TANH
        g.ldu = nc * 4
        for name in ("U", "bias", "h", "c"):
            setattr(g, name, buf.data_ptr())
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    p = buf.data_ptr()
    bad = [mk(k=2), mk(k=5), mk(dirs=3), mk(T=0), mk(act=3), mk(mask_mode=3), mk(U=None), mk(bias=None), mk(h=None), mk(c=None), mk(ldu=nc * 4 - 1),
           mk(k=3, ldu=nc * 3), mk(k=3, ldu=nc * 3, x=p, ldx=nc - 1), mk(mask_mode=1), mk(mask_mode=2, p=0.0), mk(U=p + 2),
           mk(backward=1), mk(backward=1, dh=p, dbias_part=p), mk(backward=1, dh=p, dbias_part=p, dU=p, up_add=p, ld_up_add=nc - 1),
           mk(backward=1, dh=p, dbias_part=p, dU=p, nx_b=p), mk(dU_b=p),
           # images: sequential form, T % 8, H % 64, pitch, alignment, transposed image alone
           mk(nx_b=p, ld_nxb=nc + 8), mk(nx_bt=p, ld_nxbt=N + 8)]
    for i, g in enumerate(bad):
        assert lib.gt_op_sru_scan(Ct.byref(g), None) == Lb.GT_ERR_INVALID, i
    img = dict(B=1, T=8, H=64, dirs=1, ldu=256, nx_b=p, ld_nxb=64)
    _set_knobs(dict(sru_coop=0))
    try:
        assert lib.gt_op_sru_scan(Ct.byref(mk(**img)), None) == Lb.GT_ERR_INVALID and b"cooperative" in lib.gt_last_error()
    finally:
        _set_knobs(KNOBS)
    for kw in (dict(T=12), dict(H=32, ldu=128, ld_nxb=32), dict(ld_nxb=60), dict(ld_nxb=68), dict(nx_b=p + 8), dict(nx_bt=p, ld_nxbt=4)):
        assert lib.gt_op_sru_scan(Ct.byref(mk(**dict(img, **kw))), None) == Lb.GT_ERR_INVALID, kw
    assert lib.gt_op_sru_dx_adv_finish(None, 4, 2, 2, None, 0, None, 0, None) == Lb.GT_ERR_INVALID
    assert lib.gt_op_sru_dx_adv_finish(p, 5, 2, 2, None, 0, None, 0, None) == Lb.GT_ERR_INVALID
    assert lib.gt_op_sru_dx_adv_finish(p, 4, 2, 2, p, 1, None, 0, None) == Lb.GT_ERR_INVALID
    assert lib.gt_op_sru_input_mask(None, 2, 2, 0.3, 1, 2, None, 1, 0, None) == Lb.GT_ERR_INVALID
    assert lib.gt_op_sru_input_mask(p, 2, 2, 1.0, 1, 2, None, 1, 0, None) == Lb.GT_ERR_INVALID
    assert lib.gt_op_sru_input_dropout(p, 3, p, 4, 1, 2, 4, p, None) == Lb.GT_ERR_INVALID
    assert lib.gt_op_sru_input_dropout(p, 4, p, 4, 1, 2, 4, None, None) == Lb.GT_ERR_INVALID
    counts = (Ct.c_int64 * Lb.SRU_PATH_SLOTS)()
    assert lib.gt_sru_path_counts(counts, 1) == Lb.GT_OK and sum(counts) == 0      # nothing was launched
