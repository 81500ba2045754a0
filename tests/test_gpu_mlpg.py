"""Banded MLPG (mlpg_forward_kernel / mlpg_backward_kernel, gantts_amd/csrc/mlpg_kernels.hip.h) against float64, every instantiation,
and the band cache (ensure_band, eng_mlpg.hip).

gt_op_mlpg runs ONE launch through ensure_band and mlpg_forward / mlpg_backward, the functions the step calls, with the step's freedom in
the arguments (column maps, pitches, the fused masked-MSE gradient).  Two judges:

  impulse   one impulse per (sequence, static column): the result is a scaled column (forward) or row (transpose) of float32 R inside the
            band and zero outside it, EXACTLY -- every fma has a zero operand or a zero accumulator.  This is the judge that sees the far
            taps, which are 1e-9 of the peak and invisible in random data.
  random    float32 normal data against the DENSE product with R promoted to float64 (the reference's definition, not the band).  Per
            element  |got - ref| <= n 2^-24 S + 1e-9 peak sum_outside |y|,  S = sum over the band of |R| |y|,  n = nW (2 kb + 1 + 3) the
            length of the longest fma chain (the textbook bound of a sequential fma sum; the second term is what ensure_band's own rule
            allows the band to leave out).  No element may exceed it.

Half-widths, LDS sizes and tile constants are computed here from the same rules and from the MLPG_* constants of frame_kernels.hip.h, never copied.
The CPU self-check at the end runs a numpy model of the tiled kernels through both judges, and six mutations of it that must be caught.
"""
import ctypes as Ct
import functools
import os
import re

import numpy as np
import pytest
import torch

import cases as C
from test_gpu_gemm_b16 import _F32, pads_intact
from test_gpu_gemm_f32 import SENT, U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = np.float32(np.nan)
BAND_EPS = np.float32(1e-9)          # ensure_band: what lies outside the band is <= 1e-9f * peak
MSE_ULPS = 6                         # float32 inv_tv, two products, the difference, two scalings, the final add


def _kernel_constants():
    src = open(os.path.join(ROOT, "gantts_amd", "csrc", "frame_kernels.hip.h")).read()
    return {n: int(re.search(r"constexpr int %s = (\d+);" % n, src).group(1)) for n in ("MLPG_TT", "MLPG_CC", "MLPG_PAD", "MLPG_MAXW", "MLPG_THREADS")}


K = _kernel_constants()
CC, PAD, MAXW = K["MLPG_CC"], K["MLPG_PAD"], K["MLPG_MAXW"]
INSTANCES = [(16, 2), (32, 1), (32, 2), (32, 4)]      # (mlpg_tt, mlpg_fpl): <2,16>, <1,32>, <2,32>, <4,32>
DEFAULT = (0, 2)                                      # GtTuning defaults: 32-frame tiles, two frames per lane


def lds_forward(tt, kb, nW):
    return ((tt + 2 * kb) * nW * CC + tt * nW * (2 * kb + 1 + 2 * PAD)) * 4


def lds_backward(tt, kb, nW):
    return ((tt + 2 * kb) * CC + (tt + 2 * kb) * nW * (2 * kb + 1 + 2 * PAD)) * 4


def band_accepted(kb, T):
    """ensure_band's acceptance rule"""
    return not (kb > 63 or (kb > 48 and kb > T // 4))


# ---------------------------------------------------------------------------------------------------------------------
# window sets
# ---------------------------------------------------------------------------------------------------------------------
def _static(c):
    return (0, 0, np.array([c]))


_D1, _D2 = C.WINDOWS[1], C.WINDOWS[2]
_D4 = (2, 2, np.array([-0.2, -0.1, 0.0, 0.1, 0.2]))
WINDOW_SETS = {
    "std": list(C.WINDOWS),
    "static": [_static(1.0)],
    "delta": [_static(1.0), _D1],
    "asym": [_static(1.0), (0, 1, np.array([-1.0, 1.0])), _D2],
    "four": list(C.WINDOWS) + [_D4],
    "slow3": [_static(0.5), _D1, _D2],
    "slow2": [_static(0.5), _D1],
    "wide4": [_static(0.3), _D1, _D2, _D4],
    "four_half": [_static(0.5), _D1, _D2, _D4],
}
# the half-widths the issue lists: (window set, T) -> kb
LISTED_KB = {("std", 97): 22, ("std", 31): 22, ("std", 17): 16, ("static", 97): 0, ("delta", 97): 23, ("asym", 97): 24, ("four", 97): 31,
             ("slow3", 39): 38, ("slow3", 97): 38, ("slow2", 44): 43, ("slow2", 90): 43, ("slow2", 97): 43, ("wide4", 40): 39,
             ("wide4", 49): 48, ("wide4", 50): 49, ("four_half", 236): 59}
KB_WIDE = {"std": 22, "static": 0, "delta": 23, "asym": 24, "four": 31, "slow3": 38, "slow2": 43}      # at large T (asserted below)


@functools.lru_cache(maxsize=None)
def matrix(name, T):
    from gantts_amd import paramgen
    return paramgen.unit_variance_mlpg_matrix(WINDOW_SETS[name], T)


def half_width(R, T, nW):
    """ensure_band's rule in its own arithmetic: the largest |offset| at which some |R[t][w*T + t + o]| > 1e-9f * peak (float32 product)."""
    A = np.abs(np.asarray(R, np.float32)).reshape(T, nW, T)
    peak = np.float32(A.max())
    t = np.arange(T)
    big = (A > BAND_EPS * peak).any(axis=1)
    return int(np.abs(t[None, :] - t[:, None])[big].max()), peak


@functools.lru_cache(maxsize=None)
def kb_of(name, T):
    return half_width(matrix(name, T), T, len(WINDOW_SETS[name]))[0]


def layout(ss, hd, nW):
    """the engine's static-column maps (gt_engine_create): scol, sstride, full width, static width"""
    scol, sst, col = [], [], 0
    for sz, dyn in zip(ss, hd):
        w = sz // nW if dyn else sz
        scol += [col + c for c in range(w)]
        sst += [w if dyn else 0] * w
        col += sz
    return np.array(scol), np.array(sst), col, len(scol)


def streams(n, nW):
    """[3n,3,1,3] with hd [T,T,F,T] at nW = 3, stream sizes scaled by nW / 3: Ds = n + 3"""
    return [n * nW, nW, 1, nW], [True, True, False, True]


EDGE_LAYOUTS = {      # pass-through columns 62..65 across the block boundary; the pass-through stream first
    "straddle": lambda nW: ([62 * nW, 4, nW], [True, False, True]),
    "pass_first": lambda nW: ([4, nW], [False, True]),
}
IMPULSE_LAYOUT = lambda nW: ([61 * nW, 2 * nW, 2, 3 * nW], [True, True, False, True])      # Ds = 68: two column blocks, pass-through 63, 64


# ---------------------------------------------------------------------------------------------------------------------
# cases and judges (shared by the GPU tests and the CPU self-check)
# ---------------------------------------------------------------------------------------------------------------------
def impulse_frames(T, kb):
    want = [0, 1, kb - 1, kb, kb + 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, T - kb - 1, T - 2, T - 1]
    return sorted({f for f in want if 0 <= f < T})


def impulse_case(R, T, nW, kb, scol, sst, Dout, B, backward):
    """(input, expected, exact-zero mask is implied): one impulse per (b, dynamic static column), random data in the pass-through columns"""
    Ds = len(scol)
    Rw = np.asarray(R, np.float32).reshape(T, nW, T)
    frames = impulse_frames(T, kb)
    rs = np.random.RandomState(1000 * T + 10 * nW + int(backward))
    t = np.arange(T)
    k = 0
    if not backward:
        x = np.zeros((B, T, Dout), np.float32)
        exp = np.zeros((B, T, Ds), np.float32)
    else:
        x = np.zeros((B, T, Ds), np.float32)
        exp = np.zeros((B, T, Dout), np.float32)
    for b in range(B):
        for c in range(Ds):
            if sst[c] == 0:
                v = rs.randn(T).astype(np.float32)
                if not backward:
                    x[b, :, scol[c]] = v
                    exp[b, :, c] = v
                else:
                    x[b, :, c] = v
                    exp[b, :, scol[c]] = v
                continue
            s, v = frames[k % len(frames)], np.float32(1.0 if k % 2 == 0 else -0.5)
            inband = np.abs(t - s) <= kb
            if not backward:
                w = (k // len(frames) + c + b) % nW
                x[b, s, scol[c] + w * sst[c]] = v
                exp[b, :, c] = np.where(inband, Rw[:, w, s] * v, np.float32(0))       # ys[t] = R[t][w T + s] v
            else:
                x[b, s, c] = v
                for w in range(nW):
                    exp[b, :, scol[c] + w * sst[c]] = np.where(inband, Rw[s, w, :] * v, np.float32(0))      # gy[t'] = R[s][w T + t'] v
            k += 1
    assert k >= len(frames), "too few dynamic columns to place every impulse frame"
    return x, exp


def fixture_band_is_negligible_outside(R, T, nW, kb):
    A = np.abs(np.asarray(R, np.float32)).reshape(T, nW, T)
    t = np.arange(T)
    outside = np.broadcast_to((np.abs(t[None, :] - t[:, None]) > kb)[:, None, :], A.shape)
    return bool((A[outside] <= BAND_EPS * np.float32(A.max())).all())


def judge_exact(got, exp):
    """number of elements that differ (as values: -0 equals +0); NaN never equals"""
    got, exp = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    assert got.shape == exp.shape
    return int((~(got == exp)).sum())


def random_case(T, Dout, Ds, B, backward, seed):
    rs = np.random.RandomState(seed)
    return rs.randn(B, T, Ds if backward else Dout).astype(np.float32)


def reference(R, T, nW, kb, scol, sst, Dout, x, backward):
    """float64 dense product and the per-element limit.  Returns (ref, limit, passthrough mask over the result)."""
    scol, sst = np.asarray(scol), np.asarray(sst)
    Rw = np.asarray(R, np.float32).reshape(T, nW, T).astype(np.float64)
    peak = float(np.float32(np.abs(Rw).max()))
    t = np.arange(T)
    inband = (np.abs(t[None, :] - t[:, None]) <= kb)[:, None, :]
    Rin, Rout = np.abs(Rw) * inband, np.broadcast_to((~inband).astype(np.float64), Rw.shape)
    n = nW * (2 * kb + 1 + 3)
    dyn = np.nonzero(sst > 0)[0]
    cols = scol[dyn][None, :] + np.arange(nW)[:, None] * sst[dyn][None, :]      # [w][dynamic column]
    x64 = x.astype(np.float64)
    B = x.shape[0]
    if not backward:
        Yw = x64[:, :, cols]                                                     # [b][u][w][c]
        ref = np.zeros((B, T, len(scol)))
        lim = np.zeros_like(ref)
        ref[:, :, dyn] = np.einsum("twu,buwc->btc", Rw, Yw)
        lim[:, :, dyn] = n * U * np.einsum("twu,buwc->btc", Rin, np.abs(Yw)) + 1e-9 * peak * np.einsum("twu,buwc->btc", Rout, np.abs(Yw))
        pt = np.zeros(ref.shape, bool)
        pt[:, :, sst == 0] = True
        ref[:, :, sst == 0] = x64[:, :, scol[sst == 0]]
    else:
        G = x64[:, :, dyn]                                                       # [b][t][c]
        ref = np.zeros((B, T, Dout))
        lim = np.zeros_like(ref)
        ref[:, :, cols] = np.einsum("twu,btc->buwc", Rw, G)
        lim[:, :, cols] = n * U * np.einsum("twu,btc->buwc", Rin, np.abs(G)) + 1e-9 * peak * np.einsum("twu,btc->buwc", Rout, np.abs(G))
        pt = np.zeros(ref.shape, bool)
        pt[:, :, scol[sst == 0]] = True
        ref[:, :, scol[sst == 0]] = x64[:, :, sst == 0]
    return ref, lim, pt


def judge_random(got, ref, lim, pt, extra=None):
    """(worst |got - ref| / limit over the computed elements, elements over the limit, pass-through elements that are no copy)"""
    got = np.asarray(got, np.float32)
    if extra is not None:
        lim = lim + extra
    err = np.abs(got.astype(np.float64) - ref)
    err[~np.isfinite(err)] = np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(lim > 0, err / lim, np.where(err == 0, 0.0, np.inf))
    ratio[pt] = 0.0
    bad_pt = int((~(got[pt] == ref[pt].astype(np.float32))).sum())
    return float(ratio.max()) if ratio.size else 0.0, int((ratio > 1.0).sum()), bad_pt


# ---------------------------------------------------------------------------------------------------------------------
# running the library
# ---------------------------------------------------------------------------------------------------------------------
_ENGINES, _R_DEV = {}, {}


def engine(ss, hd, nW, fresh=False):
    from gantts_amd.engine import StepEngine
    from gantts_amd.multistream import _HP
    key = (tuple(ss), tuple(hd), nW)
    if fresh:
        return StepEngine(_HP(ss, hd, nW))
    if key not in _ENGINES:
        _ENGINES[key] = StepEngine(_HP(ss, hd, nW))
    return _ENGINES[key]


def r_dev(name, T):
    """device copy of a window set's R, alive for the whole session: the band cache is keyed by its address"""
    if (name, T) not in _R_DEV:
        _R_DEV[(name, T)] = torch.from_numpy(np.array(matrix(name, T))).cuda()
    return _R_DEV[(name, T)]


def _stream():
    return Ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def set_instance(tt, fpl):
    from gantts_amd import _lib as Lb
    Lb.check(Lb.lib.gt_set_tuning(b"mlpg_tt", tt))
    Lb.check(Lb.lib.gt_set_tuning(b"mlpg_fpl", fpl))


def lds_limit():
    return int(torch.cuda.get_device_properties(0).shared_memory_per_block)


def fits(tt, kb, nW, backward):
    return (lds_backward if backward else lds_forward)(tt or K["MLPG_TT"], kb, nW) <= lds_limit()


def _dense(a, cols, fill=None):
    a = np.full((a, cols), fill, np.float32) if fill is not None else np.ascontiguousarray(a, np.float32).reshape(-1, cols)
    return _F32(a, cols, 0, SENT)


def call(eng, R, B, T, backward, src, dst, maps=None, Ds=0, mse=None, expect_kb=None):
    """One gt_op_mlpg call.  src / dst: _F32 buffers; maps: (scol, sstride) device int32 tensors or None (the engine's own);
    mse: (mse_w, yhat _F32, ytgt _F32, mask tensor).  Returns (rc, kb)."""
    from gantts_amd import _lib as Lb
    g = Lb.MlpgCase()
    kb = Ct.c_int32(-1)
    g.backward, g.B, g.T, g.Ds = int(backward), B, T, Ds
    g.e, g.R, g.kb = eng._h, R.data_ptr(), Ct.pointer(kb)
    if maps is not None:
        g.scol, g.sstride = [None if m is None else m.data_ptr() for m in maps]
    if not backward:
        g.y, g.ldy, g.ys, g.ldys = src.ptr, src.ld, dst.ptr, dst.ld
    else:
        g.gs, g.ldgs, g.gy, g.ldgy = src.ptr, src.ld, dst.ptr, dst.ld
    if mse is not None:
        g.mse_w = mse[0]
        if mse[1] is not None:
            g.yhat, g.ytgt, g.ldt, g.mask = mse[1].ptr, mse[2].ptr, mse[1].ld, mse[3].data_ptr()
    rc = Lb.lib.gt_op_mlpg(Ct.byref(g), _stream())
    if rc == Lb.GT_ERR_HIP:      # a device error: nothing more is launched in this session
        pytest.exit("gt_op_mlpg: %s" % Lb.lib.gt_last_error(), returncode=3)
    if rc == Lb.GT_OK and expect_kb is not None:
        assert kb.value == expect_kb, "the engine chose half-width %d, the rule gives %d" % (kb.value, expect_kb)
    return rc, kb.value


def run_dense(name, T, ss, hd, x, backward):
    """x [B][T][Dout] -> [B][T][Ds] (or the transpose) through the engine's own maps at dense pitches, the result pre-filled with NaN"""
    from gantts_amd import _lib as Lb
    nW = len(WINDOW_SETS[name])
    _, _, Dout, Ds = layout(ss, hd, nW)
    B = x.shape[0]
    src = _dense(x, Ds if backward else Dout)
    dst = _dense(B * T, Dout if backward else Ds, fill=NAN)
    rc, _ = call(engine(ss, hd, nW), r_dev(name, T), B, T, backward, src, dst, expect_kb=kb_of(name, T))
    assert rc == Lb.GT_OK, Lb.lib.gt_last_error()
    flat, got = dst.got()
    assert pads_intact(flat, dst.inside(), SENT), "written outside the result"
    return got.reshape(B, T, -1)


def check_random(tag, name, T, ss, hd, B, backward, got_fn=None, seed=0):
    """judge (b) for one shape; returns the result so that instantiations can be compared bit for bit"""
    nW = len(WINDOW_SETS[name])
    scol, sst, Dout, Ds = layout(ss, hd, nW)
    kb = kb_of(name, T)
    x = random_case(T, Dout, Ds, B, backward, seed + 7 * T + Ds)
    got = (got_fn or run_dense)(name, T, ss, hd, x, backward)
    ref, lim, pt = reference(matrix(name, T), T, nW, kb, scol, sst, Dout, x, backward)
    worst, over, bad_pt = judge_random(got, ref, lim, pt)
    print("%s %s %s T=%d B=%d Ds=%d kb=%d: worst |err| / bound %.4f, %d over, %d pass-through mismatches"
          % (tag, name, "bwd" if backward else "fwd", T, B, Ds, kb, worst, over, bad_pt))
    assert over == 0 and bad_pt == 0 and worst < 1.0, (tag, name, T, backward, worst, over, bad_pt)
    return got


def check_impulse(tag, name, T, B, backward, run=None):
    nW = len(WINDOW_SETS[name])
    ss, hd = IMPULSE_LAYOUT(nW)
    scol, sst, Dout, Ds = layout(ss, hd, nW)
    kb = kb_of(name, T)
    R = matrix(name, T)
    assert fixture_band_is_negligible_outside(R, T, nW, kb)
    x, exp = impulse_case(R, T, nW, kb, scol, sst, Dout, B, backward)
    got = (run or run_dense)(name, T, ss, hd, x, backward)
    diff = judge_exact(got, exp)
    assert diff == 0, "%s %s %s T=%d kb=%d: %d elements differ from float32 R" % (tag, name, "bwd" if backward else "fwd", T, kb, diff)
    return 1


FITTING_SETS = ["std", "static", "delta", "asym", "four", "slow3", "slow2", "wide4"]


def impulse_lengths(name):
    return sorted({1, 2, 17, 33, 2 * KB_WIDE.get(name, 0) + 1, 97} | ({40} if name == "wide4" else set()))


# ---------------------------------------------------------------------------------------------------------------------
# host checks of the fixtures (no GPU)
# ---------------------------------------------------------------------------------------------------------------------
def test_listed_half_widths_and_lds_sizes_hold():
    """The figures of the issue, from the rule and the formulas: half-widths of the window sets, and which tiles exceed 160 KiB."""
    for (name, T), kb in LISTED_KB.items():
        assert kb_of(name, T) == kb, (name, T, kb_of(name, T))
    for T in (1, 2, 17, 23, 24, 30, 31):      # every tap above the threshold until the band is as wide as it gets
        assert kb_of("std", T) == min(T - 1, 22)
    for name, kb in KB_WIDE.items():
        assert kb_of(name, 2 * kb + 1) == kb or name in ("slow2", "slow3"), name      # the slow sets reach their width a few frames later
    assert len(WINDOW_SETS["four"]) == MAXW and 2 * kb_of("four", 97) + 1 + 2 * PAD > 64          # the second jp pass
    assert (32 + 2 * kb_of("slow3", 97)) * 3 > 16 * (K["MLPG_THREADS"] // 64)                      # transpose staging beyond its 16 batches
    assert (32 + 2 * kb_of("std", 97)) * 3 <= 16 * (K["MLPG_THREADS"] // 64)
    lim = 160 * 1024
    assert lds_forward(32, 39, 4) == 156160 <= lim < lds_backward(32, 39, 4) == 177760
    assert lds_forward(32, 48, 4) == 183808 > lim and lds_forward(32, 59, 4) == 217600 > lim
    assert lds_forward(32, 43, 2) <= lim and lds_backward(32, 43, 2) <= lim                       # slow2: fits both kernels
    assert band_accepted(39, 40) and band_accepted(48, 49) and band_accepted(59, 236) and not band_accepted(49, 50) and not band_accepted(63, 64)


# ---------------------------------------------------------------------------------------------------------------------
# (a) impulse responses, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", FITTING_SETS)
def test_impulse_responses_are_float32_R_exactly(name):
    nW = len(WINDOW_SETS[name])
    done = skipped = 0
    try:
        for tt, fpl in INSTANCES:
            set_instance(tt, fpl)
            for T in impulse_lengths(name):
                kb = kb_of(name, T)
                if not band_accepted(kb, T):
                    skipped += 1
                    continue
                for backward in (False, True):
                    if not fits(tt, kb, nW, backward):
                        skipped += 1
                        continue
                    done += check_impulse("<%d,%d>" % (fpl, tt), name, T, 3, backward)
    finally:
        set_instance(*DEFAULT)
    print("impulse %s: %d cases exactly equal to float32 R, %d beyond the band rule or the LDS" % (name, done, skipped))
    assert done >= (32 if name != "wide4" else 24)


# ---------------------------------------------------------------------------------------------------------------------
# (b) random data against float64, (c) the instantiations agree bit for bit
# ---------------------------------------------------------------------------------------------------------------------
RANDOM_T = [1, 2, 15, 16, 17, 31, 32, 33, 45, 65, 97]
DS_N = [1, 60, 61, 62, 126]          # Ds = 4, 63, 64, 65, 129


@pytest.mark.gpu
@pytest.mark.parametrize("inst", INSTANCES, ids=lambda i: "fpl%d_tt%d" % (i[1], i[0]))
def test_random_every_instantiation_std_every_length(inst):
    """std, Ds = 65 (a second column block with one column: odd nc), every T, B = 1 and 3, and the two pass-through edge layouts"""
    try:
        set_instance(*inst)
        for T in RANDOM_T:
            for B in (1, 3):
                for backward in (False, True):
                    check_random("inst", "std", T, *streams(62, 3), B, backward)
        for lay in EDGE_LAYOUTS.values():
            for T in (33, 97):
                for backward in (False, True):
                    check_random("edge", "std", T, *lay(3), 3, backward)
    finally:
        set_instance(*DEFAULT)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["std", "four"])
def test_random_every_static_width(name):
    nW = len(WINDOW_SETS[name])
    for n in DS_N:
        for T in (33, 97):
            for backward in (False, True):
                check_random("Ds", name, T, *streams(n, nW), 3, backward)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FITTING_SETS)
def test_random_every_window_set(name):
    """every window set at two lengths (wide4: the forward at T = 40, both directions at T = 33 where its half-width is 32)"""
    nW = len(WINDOW_SETS[name])
    for T in ((33, 40) if name == "wide4" else (45, 97)):
        kb = kb_of(name, T)
        for lay in (streams(62, nW), EDGE_LAYOUTS["straddle"](nW)):
            for backward in (False, True):
                if fits(0, kb, nW, backward):
                    check_random("set", name, T, *lay, 3, backward)
                else:
                    assert name == "wide4" and T == 40 and backward


@pytest.mark.gpu
@pytest.mark.parametrize("name,T", [("std", 97), ("std", 17), ("four", 97), ("asym", 65), ("slow3", 45), ("static", 33)])
def test_instantiations_agree_bit_for_bit(name, T):
    """Same products in the same order, the padded taps add exact zeros: the four instantiations give the same bits."""
    nW = len(WINDOW_SETS[name])
    res = {}
    try:
        for inst in INSTANCES:
            set_instance(*inst)
            res[inst] = [check_random("bits", name, T, *streams(62, nW), 3, backward) for backward in (False, True)]
    finally:
        set_instance(*DEFAULT)
    first = res[INSTANCES[0]]
    for inst in INSTANCES[1:]:
        for d in (0, 1):
            assert np.array_equal(res[inst][d].view(np.uint32), first[d].view(np.uint32)), (inst, "bwd" if d else "fwd")


# ---------------------------------------------------------------------------------------------------------------------
# (d) pitches and untouched memory, (e) the fused masked-MSE gradient
# ---------------------------------------------------------------------------------------------------------------------
def _pitched(x, cols, ld):
    """input [rows][cols] at pitch ld, NaN in the pads"""
    return _F32(np.ascontiguousarray(x, np.float32).reshape(-1, cols), ld, 1, NAN)


def _result(rows, cols, ld, inner=None):
    """result [rows][cols] at pitch ld: the sentinel everywhere (`inner`: what the result's own columns hold first), guard words around it"""
    return _F32(np.full((rows, cols), SENT if inner is None else inner, np.float32), ld, 1, SENT)


def run_pitched(maps_of):
    """a run function for check_random / check_impulse: Dout + 3, Ds + 1, Ds + 5 and (Dout + 3) & ~3, every pad and guard word checked"""
    def run(name, T, ss, hd, x, backward):
        from gantts_amd import _lib as Lb
        nW = len(WINDOW_SETS[name])
        scol, sst, Dout, Ds = layout(ss, hd, nW)
        B = x.shape[0]
        eng, maps = maps_of(ss, hd, nW, scol, sst)
        if not backward:
            src, dst = _pitched(x, Dout, Dout + 3), _result(B * T, Ds, Ds + 1)
        else:
            src, dst = _pitched(x, Ds, Ds + 5), _result(B * T, Dout, (Dout + 3) & ~3)
        rc, _ = call(eng, r_dev(name, T), B, T, backward, src, dst, maps=maps, Ds=Ds if maps is not None else 0, expect_kb=kb_of(name, T))
        assert rc == Lb.GT_OK, Lb.lib.gt_last_error()
        flat, got = dst.got()
        assert pads_intact(flat, dst.inside(), SENT), "a pad column or a guard word was written"
        written = np.ones(got.shape[1], bool)
        if backward:      # the transpose writes the mapped columns only
            written[:] = False
            for w in range(nW):
                written[(scol + w * sst)[(sst > 0) | (w == 0)]] = True
            assert np.array_equal(got[:, ~written].view(np.uint32), np.full(got[:, ~written].shape, SENT, np.float32).view(np.uint32))
            got[:, ~written] = 0.0
        assert not (got[:, written].view(np.uint32) == SENT.view(np.uint32)).any(), "an element of the result was not written"
        return got.reshape(B, T, -1)
    return run


def _own_maps(ss, hd, nW, scol, sst):
    return engine(ss, hd, nW), None


def _given_maps(ss, hd, nW, scol, sst):
    """the same maps passed as the case's own device arrays, on an engine whose stream layout is another one"""
    dev = (torch.from_numpy(scol.astype(np.int32)).cuda(), torch.from_numpy(sst.astype(np.int32)).cuda())
    return engine([nW], [True], nW), dev


@pytest.mark.gpu
@pytest.mark.parametrize("name,T", [("std", 33), ("std", 97), ("four", 65), ("slow2", 97)])
@pytest.mark.parametrize("maps_of", [_own_maps, _given_maps], ids=["engine_maps", "case_maps"])
def test_pitched_operands_and_untouched_memory(name, T, maps_of):
    nW = len(WINDOW_SETS[name])
    run = run_pitched(maps_of)
    for lay in (streams(62, nW), EDGE_LAYOUTS["straddle"](nW)):
        for backward in (False, True):
            check_random("pitch", name, T, *lay, 3, backward, got_fn=run)
    for backward in (False, True):
        check_impulse("pitch", name, T, 3, backward, run=run)


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,sd", [("std", 33, 59), ("std", 97, 65), ("delta", 65, 64)])
def test_in2out_column_maps(name, T, sd):
    """The In2Out form: scol = identity, sstride = sd, one stream of sd static columns (eng_core.hip: d_scol_i2o / d_sstride_i2o)."""
    nW = len(WINDOW_SETS[name])
    ss, hd = [sd * nW], [True]
    scol, sst, Dout, Ds = layout(ss, hd, nW)
    assert np.array_equal(scol, np.arange(sd)) and (sst == sd).all() and Dout == nW * sd
    run = run_pitched(_given_maps)
    for backward in (False, True):
        check_random("i2o", name, T, ss, hd, 3, backward, got_fn=run)


@pytest.mark.gpu
@pytest.mark.parametrize("mse_w", [1.0, 0.5])
@pytest.mark.parametrize("name,T", [("std", 45), ("four", 97)])
def test_fused_masked_mse_gradient(name, T, mse_w):
    from gantts_amd import _lib as Lb
    nW = len(WINDOW_SETS[name])
    B = 3
    ss, hd = streams(62, nW)
    scol, sst, Dout, Ds = layout(ss, hd, nW)
    kb = kb_of(name, T)
    rs = np.random.RandomState(T + int(8 * mse_w))
    gs = rs.randn(B, T, Ds).astype(np.float32)
    yhat, ytgt = rs.randn(B, T, Dout).astype(np.float32), rs.randn(B, T, Dout).astype(np.float32)
    lengths = [T, 0, T // 2]
    m = (np.arange(T)[None, :] < np.array(lengths)[:, None]).astype(np.float32)
    src, dst = _pitched(gs, Ds, Ds + 5), _result(B * T, Dout, (Dout + 3) & ~3)
    hb, tb = _F32(yhat.reshape(-1, Dout), Dout, 0, NAN), _F32(ytgt.reshape(-1, Dout), Dout, 0, NAN)
    rc, _ = call(engine(ss, hd, nW), r_dev(name, T), B, T, True, src, dst, mse=(mse_w, hb, tb, torch.from_numpy(m).cuda()), expect_kb=kb)
    assert rc == Lb.GT_OK, Lb.lib.gt_last_error()
    flat, got = dst.got()
    assert pads_intact(flat, dst.inside(), SENT)
    ref, lim, pt = reference(matrix(name, T), T, nW, kb, scol, sst, Dout, gs, True)
    m64 = m.astype(np.float64)[:, :, None]
    tv = m64.sum()
    term = 2.0 * mse_w * (yhat * m64 - ytgt * m64) * m64 / tv
    ref = ref + term
    extra = MSE_ULPS * U * np.abs(term)
    # A pass-through column carries the copied gradient PLUS the term.  The bound of the copy alone is zero, so the rounding of the final
    # add, at most 2^-24 of the result, has nothing to hide in there: it is added for these columns (in the others the three spare
    # fused multiply-adds per window of n cover it, S being at least the MLPG part of the result).
    lim = lim + np.where(pt, U * np.abs(ref), 0.0)
    worst, over, _ = judge_random(got.reshape(B, T, Dout), ref, lim, np.zeros(ref.shape, bool), extra=extra)
    print("mse %s T=%d mse_w=%g kb=%d: worst |err| / bound %.4f, %d over" % (name, T, mse_w, kb, worst, over))
    assert over == 0 and worst < 1.0


@pytest.mark.gpu
def test_no_mse_weight_is_the_plain_transpose_bit_for_bit():
    """mse_w = 0 with null yhat, ytgt and mask through gt_op_mlpg == gt_op_mlpg_backward"""
    T, B, nW = 65, 3, 3
    ss, hd = streams(62, nW)
    _, _, Dout, Ds = layout(ss, hd, nW)
    gs = random_case(T, Dout, Ds, B, True, 5)
    a = run_dense("std", T, ss, hd, gs, True)
    b = engine(ss, hd, nW).mlpg_backward(torch.from_numpy(gs).cuda(), r_dev("std", T), Dout).cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    y = random_case(T, Dout, Ds, B, False, 6)
    a = run_dense("std", T, ss, hd, y, False)
    b = engine(ss, hd, nW).mlpg_forward(torch.from_numpy(y).cuda(), r_dev("std", T)).cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
def test_malformed_cases_are_refused_on_the_host():
    from gantts_amd import _lib as Lb
    T, B, nW = 17, 2, 3
    ss, hd = streams(1, nW)
    scol, sst, Dout, Ds = layout(ss, hd, nW)
    eng, R = engine(ss, hd, nW), r_dev("std", T)
    assert Lb.lib.gt_op_mlpg(None, None) == Lb.GT_ERR_INVALID
    maps = (torch.from_numpy(scol.astype(np.int32)).cuda(), torch.from_numpy(sst.astype(np.int32)).cuda())
    far = (torch.from_numpy((scol + 1).astype(np.int32)).cuda(), maps[1])          # the last window of the last stream reaches column Dout
    neg = (torch.from_numpy((scol - 1).astype(np.int32)).cuda(), maps[1])

    def go(backward, ld_full=Dout, ld_static=Ds, maps=None, Ds_=0, src=True, dst=True, mse=None, R_=R, eng_=eng):
        full, stat = _dense(B * T, ld_full, fill=0.0), _dense(B * T, max(ld_static, 1), fill=0.0)
        full.ld, stat.ld = ld_full, ld_static
        s, d = (stat, full) if backward else (full, stat)
        if not src:
            s = _NullBuf(s.ld)
        if not dst:
            d = _NullBuf(d.ld)
        return call(eng_, R_, B, T, backward, s, d, maps=maps, Ds=Ds_, mse=mse)[0]

    ok = Lb.GT_OK
    bad = Lb.GT_ERR_INVALID
    assert go(False) == ok and go(True) == ok and go(False, maps=maps, Ds_=Ds) == ok and go(True, maps=maps, Ds_=Ds) == ok
    for backward in (False, True):
        assert go(backward, src=False) == bad and go(backward, dst=False) == bad                      # null tensors
        assert go(backward, ld_static=Ds - 1) == bad and go(backward, ld_full=Dout - 1) == bad          # pitches below the widths
        assert go(backward, maps=far, Ds_=Ds) == bad and go(backward, maps=neg, Ds_=Ds) == bad          # maps beyond ldy / ldgy
        assert go(backward, maps=far, Ds_=Ds, ld_full=Dout + 1) == ok
        assert go(backward, maps=(maps[0], None), Ds_=Ds) == bad and go(backward, maps=maps, Ds_=0) == bad and go(backward, Ds_=Ds + 1) == bad
        assert go(backward, R_=_NullBuf(0)) == bad
    hb = _F32(np.zeros((B * T, Dout), np.float32), Dout, 0, NAN)
    m = torch.ones(B * T, device="cuda")
    assert go(True, mse=(1.0, hb, hb, m)) == ok
    assert go(True, mse=(1.0, None, None, None)) == bad                                               # the gradient without its operands
    short = _F32(np.zeros((B * T, Dout - 1), np.float32), Dout - 1, 0, NAN)
    assert go(True, mse=(1.0, short, short, m)) == bad                                                # ldt below the columns the maps reach
    g = Lb.MlpgCase()
    assert Lb.lib.gt_op_mlpg(Ct.byref(g), None) == bad                                                # null engine


class _NullBuf:
    def __init__(self, ld):
        self.ptr, self.ld = None, ld

    def data_ptr(self):
        return None


# ---------------------------------------------------------------------------------------------------------------------
# (f) the band cache, (g) the LDS guard
# ---------------------------------------------------------------------------------------------------------------------
def _std_still_served(eng, ss, hd, T=45, name="std"):
    """a std call on the same engine is right (an engine of four windows: `four`, which is std and a fourth window)"""
    nW = len(WINDOW_SETS[name])
    scol, sst, Dout, Ds = layout(ss, hd, nW)
    for backward in (False, True):
        x = random_case(T, Dout, Ds, 2, backward, 11)
        src, dst = _dense(x, Ds if backward else Dout), _dense(2 * T, Dout if backward else Ds, fill=NAN)
        rc, _ = call(eng, r_dev(name, T), 2, T, backward, src, dst, expect_kb=kb_of(name, T))
        assert rc == 0
        ref, lim, pt = reference(matrix(name, T), T, nW, kb_of(name, T), scol, sst, Dout, x, backward)
        worst, over, bad_pt = judge_random(dst.got()[1].reshape(2, T, -1), ref, lim, pt)
        assert over == 0 and bad_pt == 0, (worst, over, bad_pt)


def _judge_with(R_np, kb, T, nW, scol, sst, Dout, x, got, backward=False):
    ref, lim, pt = reference(R_np, T, nW, kb, scol, sst, Dout, x, backward)
    return judge_random(got, ref, lim, pt)


@pytest.mark.gpu
def test_band_cache_two_matrices_alive_and_rewrite():
    from gantts_amd import _lib as Lb
    T, B, nW = 97, 2, 3
    ss, hd = streams(5, nW)
    scol, sst, Dout, Ds = layout(ss, hd, nW)
    eng = engine(ss, hd, nW, fresh=True)
    Ra, Rb = np.array(matrix("std", T)), np.array(matrix("slow3", T))
    kba, kbb = kb_of("std", T), kb_of("slow3", T)
    assert kba != kbb
    da, db = torch.from_numpy(Ra).cuda(), torch.from_numpy(Rb).cuda()
    x = random_case(T, Dout, Ds, B, False, 3)
    src = _dense(x, Dout)

    def use(dev, R_np, kb):
        dst = _dense(B * T, Ds, fill=NAN)
        rc, _ = call(eng, dev, B, T, False, src, dst, expect_kb=kb)
        assert rc == Lb.GT_OK, Lb.lib.gt_last_error()
        worst, over, bad_pt = _judge_with(R_np, kb, T, nW, scol, sst, Dout, x, dst.got()[1].reshape(B, T, Ds))
        assert over == 0 and bad_pt == 0, (worst, over)
        return dst.got()[1]

    try:
        first = use(da, Ra, kba)
        for _ in range(2):      # alternately: each served from its own entry
            use(db, Rb, kbb)
            assert np.array_equal(use(da, Ra, kba).view(np.uint32), first.view(np.uint32))
        # the two differ by far more than the bound: a stale band would show
        assert _judge_with(Rb, kbb, T, nW, scol, sst, Dout, x, first.reshape(B, T, Ds))[1] > 0
        da.copy_(db)            # rewrite in place, then tell the engine
        torch.cuda.synchronize()
        eng.invalidate_mlpg_cache()
        use(da, Rb, kbb)
    finally:
        eng.invalidate_mlpg_cache()


@pytest.mark.gpu
def test_band_cache_recycles_the_least_recently_used_entry():
    from gantts_amd import _lib as Lb
    T, nW, N = 4, 3, 257      # MlpgCache::MAX_ENTRIES is 256
    src_text = open(os.path.join(ROOT, "gantts_amd", "csrc", "engine_internal.hip.h")).read()
    assert int(re.search(r"MAX_ENTRIES = (\d+)", src_text).group(1)) == N - 1
    ss, hd = streams(1, nW)
    scol, sst, Dout, Ds = layout(ss, hd, nW)
    eng = engine(ss, hd, nW, fresh=True)
    base = np.array(matrix("std", T))
    scales = (1.0 + np.arange(N) / 1024.0).astype(np.float32)
    allR = (base[None] * scales[:, None, None]).astype(np.float32)
    dev = torch.from_numpy(allR).cuda()
    kb = kb_of("std", T)
    x = random_case(T, Dout, Ds, 1, False, 9)
    src = _dense(x, Dout)

    def use(i):
        dst = _dense(T, Ds, fill=NAN)
        rc, _ = call(eng, dev[i], 1, T, False, src, dst, expect_kb=kb)
        assert rc == Lb.GT_OK, Lb.lib.gt_last_error()
        worst, over, bad_pt = _judge_with(allR[i], kb, T, nW, scol, sst, Dout, x, dst.got()[1].reshape(1, T, Ds))
        assert over == 0 and bad_pt == 0, (i, worst, over)
        return dst.got()[1].reshape(1, T, Ds)

    try:
        got0 = use(0)
        assert _judge_with(allR[1], kb, T, nW, scol, sst, Dout, x, got0)[1] > 0      # neighbours differ visibly: a stale band would show
        for i in range(1, N):
            use(i)              # the 257th recycles the first entry
        for i in (0, N - 1, N // 2):
            use(i)
    finally:
        eng.invalidate_mlpg_cache()


@pytest.mark.gpu
def test_ensure_band_rejections_leave_the_engine_usable():
    from gantts_amd import _lib as Lb
    ss, hd = streams(5, 3)
    eng = engine(ss, hd, 3, fresh=True)
    eng4 = engine(*streams(5, 4), 4, fresh=True)
    rs = np.random.RandomState(0)
    nan_R = np.array(matrix("std", 33))
    nan_R[7, 40] = np.nan                  # window 1, offset 0
    nan_far = np.array(matrix("std", 33))
    nan_far[0, 32] = np.nan                # window 0, offset 32: outside the band, where a max that drops NaN would also drop it from the result
    assert kb_of("wide4", 50) == 49 and not band_accepted(49, 50)
    dense = rs.randn(64, 3 * 64).astype(np.float32)
    assert half_width(dense, 64, 3)[0] == 63 and not band_accepted(63, 64)
    cases = [(eng, np.zeros((33, 99), np.float32), 33, "empty or not finite"), (eng, nan_R, 33, "empty or not finite"), (eng, nan_far, 33, "empty or not finite"),
             (eng, dense, 64, "not banded (half-width 63 of T=64)"), (eng4, np.array(matrix("wide4", 50)), 50, "not banded (half-width 49 of T=50)")]
    try:
        for e, R_np, T, msg in cases:
            nW = R_np.shape[1] // T
            _, _, Dout, Ds = layout(*streams(5, nW), nW)
            R = torch.from_numpy(R_np).cuda()
            for backward in (False, True):
                src, dst = _dense(2 * T, Ds if backward else Dout, fill=0.0), _dense(2 * T, Dout if backward else Ds, fill=NAN)
                rc, _ = call(e, R, 2, T, backward, src, dst)
                assert rc == Lb.GT_ERR_INVALID and msg in Lb.lib.gt_last_error().decode(), Lb.lib.gt_last_error()
                assert np.isnan(dst.got()[1]).all()                                  # no MLPG kernel ran
            _std_still_served(e, *streams(5, nW), name="std" if nW == 3 else "four")
            del R
            e.invalidate_mlpg_cache()
    finally:
        eng.invalidate_mlpg_cache()
        eng4.invalidate_mlpg_cache()


GUARD = re.compile(r"MLPG (forward|transpose): half-width (\d+) with (\d+) windows needs (\d+) bytes of LDS per (\d+)-frame tile, the device allows (\d+): "
                   r"this window set's R = \(W\^T W\)\^-1 W\^T decays too slowly for the banded kernels")


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,refused", [("wide4", 40, "transpose"), ("wide4", 49, "forward"), ("four_half", 236, "forward")])
def test_lds_guard_refuses_oversize_tiles_on_the_host(name, T, refused):
    """Nothing oversize is launched: the launchers compare the request with the device's limit first and return GT_ERR_INVALID."""
    from gantts_amd import _lib as Lb
    nW, B = 4, 2
    ss, hd = streams(5, nW)
    _, _, Dout, Ds = layout(ss, hd, nW)
    kb = kb_of(name, T)
    assert band_accepted(kb, T)
    eng = engine(ss, hd, nW)
    tt = K["MLPG_TT"]
    need = (lds_backward if refused == "transpose" else lds_forward)(tt, kb, nW)
    assert need > lds_limit()
    if refused == "transpose":      # the forward fits and serves inference: judges (a) and (b)
        assert lds_forward(tt, kb, nW) <= lds_limit()
        check_impulse("guard", name, T, 3, False)
        check_random("guard", name, T, ss, hd, 3, False)
    backward = refused == "transpose"
    src, dst = _dense(B * T, Ds if backward else Dout, fill=0.0), _dense(B * T, Dout if backward else Ds, fill=NAN)
    rc, got_kb = call(eng, r_dev(name, T), B, T, backward, src, dst)
    msg = Lb.lib.gt_last_error().decode()
    assert rc == Lb.GT_ERR_INVALID and got_kb == kb, (rc, got_kb, msg)
    m = GUARD.search(msg)
    assert m, msg
    assert (m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(6))) == (refused, kb, nW, need, tt, lds_limit()), msg
    with pytest.raises(ValueError, match="decays too slowly"):
        Lb.check(rc)
    assert np.isnan(dst.got()[1]).all()                                              # nothing ran
    # the engine still serves: an engine is bound to its number of windows, so on THIS one it is `four` (std and a fourth window), and
    # std itself on the three-window engine of the same process
    _std_still_served(eng, ss, hd, name="four")
    _std_still_served(engine(*streams(5, 3), 3), *streams(5, 3))


# ---------------------------------------------------------------------------------------------------------------------
# CPU self-check: a numpy float32 model of the two kernels with their tiling, through the same judges; six mutations
# ---------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """float32 fma up to a double rounding: the product of two float32 is exact in float64"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def extract_band(R, T, nW, kb):
    """mlpg_extract_band_kernel: band[t][w][j] = R[t][w T + t + j - kb], zero outside [0, T)"""
    Rw = np.asarray(R, np.float32).reshape(T, nW, T)
    band = np.zeros((T, nW, 2 * kb + 1), np.float32)
    for j in range(2 * kb + 1):
        t = np.arange(T)
        u = t + j - kb
        ok = (u >= 0) & (u < T)
        band[t[ok], :, j] = Rw[t[ok], :, u[ok]]
    return band


MUTATIONS = ["clamp", "reflect", "late", "droptap", "window", "colmap"]


def _staged_band(band, t_first, rows, T, mut):
    """band rows of frames t_first .. t_first + rows - 1, zero outside [0, T)"""
    nW, nb = band.shape[1:]
    sb = np.zeros((rows, nW, nb), np.float32)
    for r in range(rows):
        t = t_first + r + (1 if mut == "late" else 0)       # mutation: the rows of a tile staged one row late
        if 0 <= t < T:
            sb[r] = band[t]
        elif mut == "clamp":
            sb[r] = band[min(max(t, 0), T - 1)]
    if mut == "reflect":
        sb = sb[:, :, ::-1].copy()
    if mut == "droptap":
        sb[:, :, 0] = 0.0
    return sb


def _staged_rows(x, t_first, rows, T, mut):
    """frames t_first .. of x [B][T][D]: zero rows outside [0, T) (mutation: clamped to the edge frame)"""
    out = np.zeros((x.shape[0], rows) + x.shape[2:], np.float32)
    for r in range(rows):
        t = t_first + r
        if 0 <= t < T:
            out[:, r] = x[:, t]
        elif mut == "clamp":
            out[:, r] = x[:, min(max(t, 0), T - 1)]
    return out


def model(R, T, nW, kb, scol, sst, Dout, x, backward, TT=32, mut=None):
    """The banded forward (x = y [B][T][Dout]) or transpose (x = gs [B][T][Ds]) as the kernels tile it: TT output frames and CC static
    columns per workgroup, a halo of kb staged rows on both sides, zero rows outside [0, T), taps in ascending order."""
    band = extract_band(R, T, nW, kb)
    nb, Ds, B = 2 * kb + 1, len(scol), x.shape[0]
    rows = TT + 2 * kb
    out = np.zeros((B, T, Dout if backward else Ds), np.float32)
    for t0 in range(0, T, TT):
        nt = min(TT, T - t0)
        for c0 in range(0, Ds, CC):
            nc = min(CC, Ds - c0)
            m0 = 0 if (mut == "colmap" and c0 > 0) else c0      # mutation: the second block with the first block's map
            col, st = scol[m0:m0 + nc], sst[m0:m0 + nc]
            wcol = lambda w: (col + np.where(st > 0, (w + (1 if mut == "window" else 0)) * st, 0)) % Dout
            if not backward:
                tile = np.stack([_staged_rows(x[:, :, wcol(w)], t0 - kb, rows, T, mut) for w in range(nW)], axis=2)      # [B][rows][nW][nc]
                sb = _staged_band(band, t0, TT, T, mut)
                acc = np.zeros((B, TT, nc), np.float32)
                for w in range(nW):
                    for j in range(nb):
                        acc = fma32(sb[None, :, w, j, None], tile[:, j:j + TT, w], acc)
                res = np.where(st[None, None, :] == 0, tile[:, kb:kb + TT, 0], acc)
                out[:, t0:t0 + nt, c0:c0 + nc] = res[:, :nt]
            else:
                tile = _staged_rows(x[:, :, c0:c0 + nc], t0 - kb, rows, T, mut)                                         # [B][rows][nc]
                sb = _staged_band(band, t0 - kb, rows, T, mut)
                for w in range(nW):
                    acc = np.zeros((B, TT, nc), np.float32)
                    for q in range(nb):      # staged row tl + q reaches output frame tl through band[t][w][nb - 1 - q]
                        acc = fma32(sb[None, q:q + TT, w, nb - 1 - q, None], tile[:, q:q + TT], acc)
                    res = np.where(st[None, None, :] == 0, tile[:, kb:kb + TT], acc)
                    keep = (st > 0) | (w == 0)
                    out[:, t0:t0 + nt, wcol(w)[keep]] = res[:, :nt][:, :, keep]
    return out


def self_check(name, T, TT):
    """{(mutation or None, direction): (impulse mismatches, random elements over the bound + pass-through mismatches, worst ratio)}"""
    nW = len(WINDOW_SETS[name])
    ss, hd = IMPULSE_LAYOUT(nW)
    scol, sst, Dout, Ds = layout(ss, hd, nW)
    R, kb = matrix(name, T), kb_of(name, T)
    res = {}
    for backward in (False, True):
        xi, exp = impulse_case(R, T, nW, kb, scol, sst, Dout, 3, backward)
        xr = random_case(T, Dout, Ds, 2, backward, 1)
        ref, lim, pt = reference(R, T, nW, kb, scol, sst, Dout, xr, backward)
        for mut in [None] + MUTATIONS:
            a = judge_exact(model(R, T, nW, kb, scol, sst, Dout, xi, backward, TT, mut), exp)
            worst, over, bad_pt = judge_random(model(R, T, nW, kb, scol, sst, Dout, xr, backward, TT, mut), ref, lim, pt)
            res[(mut, backward)] = (a, over + bad_pt, worst)
    return res


@pytest.mark.parametrize("name,T,TT", [("asym", 70, 32), ("std", 50, 16)])
def test_self_check_model_passes_and_every_mutation_is_caught(name, T, TT):
    res = self_check(name, T, TT)
    for backward in (False, True):
        d = "bwd" if backward else "fwd"
        a, b, worst = res[(None, backward)]
        print("model %s %s T=%d TT=%d: impulse judge %d mismatches, random judge %d over, worst ratio %.4f" % (name, d, T, TT, a, b, worst))
        assert a == 0 and b == 0 and worst < 1.0
        for mut in MUTATIONS:
            a, b, worst = res[(mut, backward)]
            by = [j for j, n in (("impulse", a), ("random", b)) if n]
            print("mutation %-8s %s: caught by %s (impulse %d, random %d, worst ratio %.3g)" % (mut, d, " and ".join(by) or "nobody", a, b, worst))
            # Clamped halo rows cannot change the FORWARD result of finite data: the band taps that would meet a frame outside [0, T) are
            # zero already (mlpg_extract_band_kernel), so the zeroing of the forward data tile is a second line of defence.  In the
            # transpose the staged band rows of frames outside [0, T) are halo rows themselves, and clamping them is caught.
            assert by or (mut == "clamp" and not backward), (mut, d)
        # the dropped outer tap is 1e-9 of the peak: only the impulse judge can see it
        a, b, worst = res[("droptap", backward)]
        assert a > 0 and b == 0 and worst < 1.0
