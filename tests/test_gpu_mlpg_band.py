"""The MLPG band built on the device from the windows (gantts_amd/csrc/mlpg_band_kernels.hip.h, the GT_MLPG_R_FROM_WINDOWS path of ensure_band in eng_mlpg.hip)
against the committed host path paramgen.unit_variance_mlpg_matrix, the reference of every check here.

  taps        band read back through gt_op_mlpg_band: every tap  |dev - host| <= 2^-24 |host| + 2^-40 peak  (one float32 rounding, and
              ~4000 x the float64 noise of a system whose condition number is below 20), no element exempt; the same half-width
  kernels     the impulse and random judges of test_gpu_mlpg.py through gt_op_mlpg with the sentinel, against the dense matrix rebuilt
              from the read-back band
  refusals    what the dense path refuses, and what only this path can be asked; the engine serves afterwards
  cache       eviction and rebuild give the same bits; dense and built entries of one T coexist; another window set replaces the built ones
  step        apply_generator -> update_discriminator -> update_generator with a dense R and with an MLPGBand, from identical state
  no dense R  train_loop (hp.mlpg_device_band) and gen_parameters(device_band=True) with the host construction made to raise
"""
import ctypes as Ct
import types

import numpy as np
import pytest
import torch

import cases as C
import test_gpu_mlpg as M
from gantts_amd import paramgen

U24, U23, U40 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -40
TAP_CASES = [(n, T) for n, Ts in (("std", [1, 2, 3, 5, 17, 31, 65, 97, 200]), ("static", [33]), ("delta", [97]), ("asym", [97]), ("four", [4, 97]),
                                  ("slow3", [39, 97]), ("slow2", [44, 97]), ("wide4", [40, 49]), ("four_half", [120, 236])) for T in Ts]


class _Sentinel:
    """GT_MLPG_R_FROM_WINDOWS where the helpers of test_gpu_mlpg.py ask a tensor for its address"""

    def data_ptr(self):
        from gantts_amd import _lib as Lb
        return Lb.MLPG_R_FROM_WINDOWS


SENTINEL = _Sentinel()
_ENG = {}


def engine(nW, fresh=False):
    """an engine of nW windows on the [3n, 3, 1, 3]-shaped layout of test_gpu_mlpg.streams; its own, not that file's: windows get registered"""
    if fresh:
        return M.engine(*M.streams(5, nW), nW, fresh=True)
    if nW not in _ENG:
        _ENG[nW] = M.engine(*M.streams(5, nW), nW, fresh=True)
    return _ENG[nW]


def band_of(name, T):
    return paramgen.MLPGBand(M.WINDOW_SETS[name], T)


def host_band(name, T, kb):
    return M.extract_band(M.matrix(name, T), T, len(M.WINDOW_SETS[name]), kb)


def tap_errors(dev, host, peak):
    """(worst |dev - host| / bound, taps over the bound); bound = 2^-24 |host| + 2^-40 peak"""
    err = np.abs(dev.astype(np.float64) - host.astype(np.float64))
    err[~np.isfinite(err)] = np.inf
    ratio = err / (U24 * np.abs(host.astype(np.float64)) + U40 * float(peak))
    return float(ratio.max()), int((ratio > 1.0).sum())


def dense_from_band(band, kb):
    """(T, nW * T) float32 with the band's taps and zero outside: the matrix the kernels apply"""
    T, nW, nb = band.shape
    R = np.zeros((T, nW, T), np.float32)
    t = np.arange(T)
    for j in range(nb):
        u = t + j - kb
        ok = (u >= 0) & (u < T)
        R[t[ok], :, u[ok]] = band[t[ok], :, j]
    return R.reshape(T, nW * T)


def abs_product(R, T, nW, scol, sst, y):
    """sum |R| |y| per element of the static result [B][T][Ds] (0 in the pass-through columns)"""
    Rw = np.abs(np.asarray(R, np.float64)).reshape(T, nW, T)
    scol, sst = np.asarray(scol), np.asarray(sst)
    dyn = np.nonzero(sst > 0)[0]
    cols = scol[dyn][None, :] + np.arange(nW)[:, None] * sst[dyn][None, :]
    out = np.zeros(y.shape[:2] + (len(scol),))
    out[:, :, dyn] = np.einsum("twu,buwc->btc", Rw, np.abs(y.astype(np.float64))[:, :, cols])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. taps and half-width
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,T", TAP_CASES, ids=["%s_T%d" % c for c in TAP_CASES])
def test_taps_and_half_width_equal_the_host_path(name, T):
    nW = len(M.WINDOW_SETS[name])
    R = M.matrix(name, T)
    kb, peak = M.half_width(R, T, nW)
    # the host's own per-offset maxima stay clear of the threshold, so a tap that differs in its last bit cannot move the half-width
    A = np.abs(np.asarray(R, np.float32)).reshape(T, nW, T)
    thr = float(M.BAND_EPS * peak)
    offmax = np.array([float(np.diagonal(A, o, 0, 2).max()) for o in range(-(T - 1), T)])
    assert not ((offmax >= thr / 1.001) & (offmax <= thr * 1.001)).any(), "a per-offset maximum within 0.1 % of the threshold"
    if not M.band_accepted(kb, T):
        # four_half at T = 120: half-width 59 > 48 and > T / 4.  The acceptance rule, which the build keeps, refuses it on either path, so
        # there is no band to read back: the refusal must be the dense path's, with the host rule's half-width in it.  (Taps of this
        # half-width are read back at T = 236.)
        assert (name, T) == ("four_half", 120)
        with pytest.raises(ValueError, match=r"not banded \(half-width %d of T=%d\)" % (kb, T)):
            engine(nW).mlpg_band(band_of(name, T))
        with pytest.raises(ValueError, match=r"not banded \(half-width %d of T=%d\)" % (kb, T)):
            engine(nW).mlpg_band(M.r_dev(name, T))
        return
    dev, kb_dev = engine(nW).mlpg_band(band_of(name, T))
    host = host_band(name, T, kb)
    assert kb_dev == kb, "the device build chose half-width %d, the host rule gives %d" % (kb_dev, kb)
    assert dev.shape == host.shape == (T, nW, 2 * kb + 1)
    worst, over = tap_errors(dev, host, peak)
    print("%s T=%d kb=%d: worst |dev - host| / bound %.5f, %d over, %s" % (name, T, kb, worst, over,
                                                                          "bit-identical" if np.array_equal(dev.view(np.uint32), host.view(np.uint32)) else "not bit-identical"))
    assert over == 0 and worst <= 1.0
    u = np.arange(T)[:, None] + np.arange(2 * kb + 1)[None, :] - kb                                        # the frame a tap reads
    assert (dev[np.broadcast_to(((u < 0) | (u >= T))[:, None, :], dev.shape)] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the same kernels run on the built band
# ---------------------------------------------------------------------------------------------------------------------
def _run_sentinel(eng, T, nW, ss, hd, x, backward, kb):
    from gantts_amd import _lib as Lb
    _, _, Dout, Ds = M.layout(ss, hd, nW)
    B = x.shape[0]
    src = M._dense(x, Ds if backward else Dout)
    dst = M._dense(B * T, Dout if backward else Ds, fill=M.NAN)
    rc, _ = M.call(eng, SENTINEL, B, T, backward, src, dst, expect_kb=kb)
    assert rc == Lb.GT_OK, Lb.lib.gt_last_error()
    flat, got = dst.got()
    assert M.pads_intact(flat, dst.inside(), M.SENT), "written outside the result"
    return got.reshape(B, T, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["std", "asym"])
def test_step_kernels_apply_the_built_band(name):
    T, B, nW = 97, 3, 3
    ss, hd = M.IMPULSE_LAYOUT(nW)
    scol, sst, Dout, Ds = M.layout(ss, hd, nW)
    eng = M.engine(ss, hd, nW, fresh=True)
    band, kb = eng.mlpg_band(band_of(name, T))
    assert kb == M.kb_of(name, T)
    R = dense_from_band(band, kb)
    assert M.fixture_band_is_negligible_outside(R, T, nW, kb)
    for backward in (False, True):
        x, exp = M.impulse_case(R, T, nW, kb, scol, sst, Dout, B, backward)
        diff = M.judge_exact(_run_sentinel(eng, T, nW, ss, hd, x, backward, kb), exp)
        assert diff == 0, "%s %s: %d elements differ from the read-back band" % (name, "bwd" if backward else "fwd", diff)
        x = M.random_case(T, Dout, Ds, B, backward, 21)
        ref, lim, pt = M.reference(R, T, nW, kb, scol, sst, Dout, x, backward)
        worst, over, bad_pt = M.judge_random(_run_sentinel(eng, T, nW, ss, hd, x, backward, kb), ref, lim, pt)
        print("%s %s T=%d kb=%d: worst |err| / bound %.4f, %d over" % (name, "bwd" if backward else "fwd", T, kb, worst, over))
        assert over == 0 and bad_pt == 0 and worst < 1.0


# ---------------------------------------------------------------------------------------------------------------------
# 3. refusals
# ---------------------------------------------------------------------------------------------------------------------
def _served(eng, name, T):
    kb, peak = M.half_width(M.matrix(name, T), T, len(M.WINDOW_SETS[name]))
    dev, kb_dev = eng.mlpg_band(band_of(name, T))
    assert kb_dev == kb and tap_errors(dev, host_band(name, T, kb), peak)[1] == 0


def _raw_windows(eng, windows, n=None):
    from gantts_amd import _lib as Lb
    n = len(windows) if n is None else n
    coef = np.concatenate([np.asarray(c, np.float64).ravel() for _, _, c in windows])
    return Lb.lib.gt_set_mlpg_windows(eng._h, n, (Ct.c_int32 * len(windows))(*[int(l) for l, _, _ in windows]),
                                      (Ct.c_int32 * len(windows))(*[int(u) for _, u, _ in windows]), (Ct.c_double * coef.size)(*coef.tolist()))


def _raw_band(eng, T):
    from gantts_amd import _lib as Lb
    buf = np.full(T * eng.num_windows * 129, np.nan, np.float32)
    kb = Ct.c_int32(-1)
    rc = Lb.lib.gt_op_mlpg_band(eng._h, Lb.MLPG_R_FROM_WINDOWS, T, buf.ctypes.data_as(Ct.POINTER(Ct.c_float)), buf.size, Ct.byref(kb), M._stream())
    return rc, kb.value, buf


@pytest.mark.gpu
def test_refusals_leave_the_engine_usable():
    from gantts_amd import _lib as Lb
    bad = Lb.GT_ERR_INVALID
    # wide4 at T = 50: half-width 49 > 48 and > T / 4, refused as the dense path refuses it
    eng4 = engine(4, fresh=True)
    assert M.kb_of("wide4", 50) == 49 and not M.band_accepted(49, 50)
    with pytest.raises(ValueError, match=r"not banded \(half-width 49 of T=50\)"):
        eng4.mlpg_band(band_of("wide4", 50))
    ss, hd = M.streams(5, 4)
    _, _, Dout, Ds = M.layout(ss, hd, 4)
    for backward in (False, True):
        src, dst = M._dense(2 * 50, Ds if backward else Dout, fill=0.0), M._dense(2 * 50, Dout if backward else Ds, fill=M.NAN)
        rc, _ = M.call(eng4, SENTINEL, 2, 50, backward, src, dst)
        assert rc == bad and "not banded (half-width 49 of T=50)" in Lb.lib.gt_last_error().decode()
        assert np.isnan(dst.got()[1]).all()                                              # no MLPG kernel ran
    _served(eng4, "wide4", 40)
    _served(eng4, "four", 33)
    # the sentinel without registered windows
    eng = engine(3, fresh=True)
    rc, _, buf = _raw_band(eng, 17)
    assert rc == bad and "gt_set_mlpg_windows" in Lb.lib.gt_last_error().decode() and np.isnan(buf).all()
    y = torch.zeros(2, 17, M.layout(*M.streams(5, 3), 3)[2], device="cuda")
    out = torch.empty(2, 17, eng.static_dim, device="cuda")
    assert Lb.lib.gt_op_mlpg_forward(eng._h, Lb.ptr(y), Lb.MLPG_R_FROM_WINDOWS, 2, 17, Lb.ptr(out), M._stream()) == bad
    # another number of windows than the engine's; malformed windows
    assert _raw_windows(eng, M.WINDOW_SETS["delta"]) == bad and "num_windows" in Lb.lib.gt_last_error().decode()
    with pytest.raises(RuntimeError, match="2 windows, the engine 3"):
        eng.mlpg_forward(y, band_of("delta", 17))
    assert _raw_windows(eng, [(0, 0, [1.0]), (-1, 2, [1.0, 0.0]), (1, 1, [1.0, -2.0, 1.0])]) == bad
    assert _raw_windows(eng, [(0, 0, [1.0]), (20, 20, [0.1] * 41), (1, 1, [1.0, -2.0, 1.0])]) == bad       # l + u beyond GT_MLPG_MAX_WINDOW_SPAN
    assert Lb.MLPG_MAX_WINDOW_SPAN < 40
    assert _raw_windows(eng, [(0, 0, [1.0]), (1, 1, [-0.5, np.inf, 0.5]), (1, 1, [1.0, -2.0, 1.0])]) == bad
    assert _raw_windows(eng, [(0, 0, [np.nan]), (1, 1, [-0.5, 0.0, 0.5]), (1, 1, [1.0, -2.0, 1.0])]) == bad
    rc, _, _ = _raw_band(eng, 17)
    assert rc == bad                                                                     # none of them was registered
    # an MLPGBand made for another T than the batch's
    with pytest.raises(RuntimeError, match="made for T = 18, the batch has T = 17"):
        eng.mlpg_forward(y, band_of("std", 18))
    with pytest.raises(RuntimeError, match="made for T = 18"):
        eng.mlpg_backward(out, band_of("std", 18), y.size(-1))
    _served(eng, "std", 17)
    # a window set that does not determine the static features: W^T W = 0, the first pivot is no positive number
    eng1 = engine(1, fresh=True)
    with pytest.raises(ValueError, match="window set does not determine the static features"):
        eng1.mlpg_band(paramgen.MLPGBand([(0, 0, np.array([0.0]))], 17))
    with pytest.raises(ValueError, match="window set does not determine the static features"):      # nothing was cached: refused again
        eng1.mlpg_band(paramgen.MLPGBand([(0, 0, np.array([0.0]))], 17))
    _served(eng1, "static", 17)
    for e in (eng4, eng, eng1):
        e.invalidate_mlpg_cache()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the cache
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_evicted_entries_are_rebuilt_with_the_same_bits():
    import os
    import re
    src_text = open(os.path.join(M.ROOT, "gantts_amd", "csrc", "engine_internal.hip.h")).read()
    assert int(re.search(r"MAX_ENTRIES = (\d+)", src_text).group(1)) < 259      # T = 2 .. 260 are more entries than the cache holds
    eng = engine(2, fresh=True)
    try:
        first = {}
        for T in range(2, 261):
            first[T], kb = eng.mlpg_band(band_of("delta", T))
            assert first[T].shape == (T, 2, 2 * kb + 1)
        for T in (2, 3, 100, 260, 2):      # 2 and 3 were recycled and are built again; 100 and 260 are still there
            band, kb = eng.mlpg_band(band_of("delta", T))
            assert band.shape == first[T].shape and np.array_equal(band.view(np.uint32), first[T].view(np.uint32)), T
        for T in (2, 24, 129, 260):
            kb, peak = M.half_width(M.matrix("delta", T), T, 2)
            assert first[T].shape[2] == 2 * kb + 1 and tap_errors(first[T], host_band("delta", T, kb), peak)[1] == 0
    finally:
        eng.invalidate_mlpg_cache()


@pytest.mark.gpu
def test_dense_and_built_entries_coexist_and_a_new_window_set_replaces_the_built_ones():
    T, nW = 97, 3
    eng = engine(nW, fresh=True)
    R_dev = torch.from_numpy(np.array(M.matrix("std", T))).cuda()
    kb_std, peak_std = M.half_width(M.matrix("std", T), T, nW)
    kb_slow, peak_slow = M.half_width(M.matrix("slow3", T), T, nW)
    assert kb_std != kb_slow
    try:
        dense1, kd = eng.mlpg_band(R_dev)
        built1, kw = eng.mlpg_band(band_of("std", T))
        assert kd == kw == kb_std
        assert np.array_equal(dense1.view(np.uint32), host_band("std", T, kb_std).view(np.uint32))      # extraction copies
        assert tap_errors(built1, host_band("std", T, kb_std), peak_std)[1] == 0
        for _ in range(2):      # alternately, each from its own entry
            assert np.array_equal(eng.mlpg_band(R_dev)[0].view(np.uint32), dense1.view(np.uint32))
            assert np.array_equal(eng.mlpg_band(band_of("std", T))[0].view(np.uint32), built1.view(np.uint32))
        # slow3 after std at the same T: the built entry is slow3's, the dense one is still std's
        slow, ks = eng.mlpg_band(band_of("slow3", T))
        assert ks == kb_slow and tap_errors(slow, host_band("slow3", T, kb_slow), peak_slow)[1] == 0
        assert np.array_equal(eng.mlpg_band(R_dev)[0].view(np.uint32), dense1.view(np.uint32))
        again, kw = eng.mlpg_band(band_of("std", T))
        assert kw == kb_std and np.array_equal(again.view(np.uint32), built1.view(np.uint32))
    finally:
        eng.invalidate_mlpg_cache()


# ---------------------------------------------------------------------------------------------------------------------
# 5. one G + D step with a dense R and with an MLPGBand
# ---------------------------------------------------------------------------------------------------------------------
STEP = dict(ss=[9, 3, 1, 3], hd=[True, True, False, True], B=3, T=97, lengths=[97, 80, 61], din=8,
            g=dict(kind="MLP", in_dim=8, out_dim=16, num_hidden=2, hidden_dim=12, dropout=0.0, last_sigmoid=False),
            d=dict(kind="MLP", in_dim=6, out_dim=1, num_hidden=2, hidden_dim=10, dropout=0.0, last_sigmoid=True))


def _step_hp():
    from gantts_amd import hparams
    hp = types.SimpleNamespace(**hparams.tts_acoustic.values())
    hp.stream_sizes, hp.has_dynamic_features, hp.windows = STEP["ss"], STEP["hd"], list(C.WINDOWS)
    hp.adversarial_streams, hp.mask_nth_mgc_for_adv_loss, hp.discriminator_linguistic_condition = None, 0, False
    return hp


def _one_step(make_R):
    """apply_generator -> update_discriminator -> update_generator from the seeded state; everything the step produced"""
    import gantts_amd.train as T
    from gantts_amd import optim
    from gantts_amd.engine import engine_for
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model
    hp = _step_hp()
    saved = getattr(T, "hp", None)
    T.hp = hp
    try:
        mg, md = build_model(STEP["g"], 11), build_model(STEP["d"], 22)
        mg.train(), md.train()
        og, od = optim.Adagrad(mg.parameters(), lr=0.01, weight_decay=1e-7), optim.Adagrad(md.parameters(), lr=0.01, weight_decay=1e-7)
        rs = np.random.RandomState(5)
        B, Tn, lengths = STEP["B"], STEP["T"], STEP["lengths"]
        x = (0.01 + 0.98 * rs.rand(B, Tn, STEP["din"])).astype(np.float32)
        y = rs.randn(B, Tn, 16).astype(np.float32)
        for b, n in enumerate(lengths):
            x[b, n:] = 0
            y[b, n:] = 0
        x, y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        R = make_R(hp.windows, Tn)
        y_static = get_static_features(y, 3, hp.stream_sizes, hp.has_dynamic_features)
        mask = sequence_mask(torch.tensor(lengths).cuda(), max_len=Tn).unsqueeze(-1)
        og.zero_grad()
        od.zero_grad()
        y_hat, y_hat_static = T.apply_generator(mg, x, R, lengths)
        out = {"y_hat": y_hat.cpu().numpy(), "y_hat_static": y_hat_static.cpu().numpy()}
        out["d"] = np.array(T.update_discriminator(md, od, x, y_static, y_hat_static, lengths, mask, "train"), np.float64)
        out["g"] = np.array(T.update_generator(mg, md, og, x, y, y_hat, y_static, y_hat_static, 1.0, lengths, mask, "train", mse_w=0.5, mge_w=1.0),
                            np.float64)
        torch.cuda.synchronize()
        out["band"] = engine_for(hp, mg).mlpg_band(R, Tn)
        out["params"] = {t + "." + k: v.cpu().numpy() for t, m in (("G", mg), ("D", md)) for k, v in m.state_dict().items()}
        return out
    finally:
        T.hp = saved


def _compare_runs(a, b, bound_static, what):
    """a: dense R, b: MLPGBand.  Bit-identical bands -> bit-identical everything."""
    from test_gpu_parity import RTOL, _close
    assert np.array_equal(a["y_hat"].view(np.uint32), b["y_hat"].view(np.uint32)), what + ": y_hat does not depend on R"
    same_band = a["band"][1] == b["band"][1] and np.array_equal(a["band"][0].view(np.uint32), b["band"][0].view(np.uint32))
    err = np.abs(a["y_hat_static"].astype(np.float64) - b["y_hat_static"].astype(np.float64))
    print("%s: bands %s, worst |y_hat_static difference| / bound %.4f" % (what, "bit-identical" if same_band else "differ in their last bits",
                                                                       float((err / np.maximum(bound_static, 1e-300)).max())))
    assert (err <= bound_static).all()
    for k in ("d", "g"):
        if k in a:
            assert (np.abs(a[k] - b[k]) <= RTOL * np.maximum(np.abs(a[k]), 1e-3)).all(), (k, a[k], b[k])
    for k, v in a.get("params", {}).items():
        _close(b["params"][k], v, rtol=RTOL, atol=1e-6, msg=what + ":" + k)
    if same_band:
        assert np.array_equal(a["y_hat_static"].view(np.uint32), b["y_hat_static"].view(np.uint32))
        for k in ("d", "g"):
            if k in a:
                assert np.array_equal(a[k], b[k])
        for k, v in a.get("params", {}).items():
            assert np.array_equal(v.view(np.uint32), b["params"][k].view(np.uint32)), k


@pytest.mark.gpu
def test_one_step_with_a_dense_R_and_with_an_mlpg_band():
    dense = _one_step(paramgen.unit_variance_mlpg_matrix_cuda)
    built = _one_step(paramgen.unit_variance_mlpg_band)
    assert built["band"][1] == dense["band"][1] == 22
    scol, sst, Dout, Ds = M.layout(STEP["ss"], STEP["hd"], 3)
    S = abs_product(paramgen.unit_variance_mlpg_matrix(C.WINDOWS, STEP["T"]), STEP["T"], 3, scol, sst, dense["y_hat"])
    _compare_runs(dense, built, U23 * S, "MLP step")
    assert np.isfinite(dense["d"]).all() and np.isfinite(dense["g"]).all() and dense["g"][3] != 0


@pytest.mark.gpu
def test_in2out_highway_forward_with_a_dense_R_and_with_an_mlpg_band():
    """out2 = x_static + Tx * MLPG(G(x)), Tx in (0, 1): a difference d of the MLPG term reaches out2 as at most d, plus one rounding of the
    product (<= 2^-24 |MLPG term| <= 2^-24 sum |R||y|) and one of the sum (<= 2^-24 |out2|), each on either side."""
    from hip_runner import build_model
    Tn, B, sd = 97, 3, 3
    spec = dict(kind="In2OutHighwayNet", in_dim=9, out_dim=9, static_dim=sd, num_hidden=1, hidden_dim=8, dropout=0.0)
    rs = np.random.RandomState(8)
    x = torch.from_numpy(rs.randn(B, Tn, 9).astype(np.float32)).cuda()
    res = {}
    for tag, R in (("dense", paramgen.unit_variance_mlpg_matrix_cuda(C.WINDOWS, Tn)), ("band", paramgen.unit_variance_mlpg_band(C.WINDOWS, Tn))):
        m = build_model(spec, 31)
        m.eval()
        y_hat, out2 = m(x, R)
        res[tag] = {"y_hat": y_hat.cpu().numpy(), "y_hat_static": out2.cpu().numpy(), "band": m._own_engine().mlpg_band(R, Tn)}
    scol, sst = np.arange(sd), np.full(sd, sd)
    S = abs_product(paramgen.unit_variance_mlpg_matrix(C.WINDOWS, Tn), Tn, 3, scol, sst, res["dense"]["y_hat"])
    _compare_runs(res["dense"], res["band"], U23 * (2.0 * S + np.abs(res["dense"]["y_hat_static"])), "In2OutHighwayNet forward")


# ---------------------------------------------------------------------------------------------------------------------
# 6. no dense R anywhere
# ---------------------------------------------------------------------------------------------------------------------
def _train_loop_run(device_band):
    import gantts_amd.train as T
    from gantts_amd import hparams, optim
    from hip_runner import build_model
    case = dict(C.TRAIN_LOOP_CASES["train_loop_acoustic"], batches=dict(train=[(3, 29)], test=[(2, 21)]))
    hp = types.SimpleNamespace(**getattr(hparams, case["hp"]).values())
    hp.stream_sizes, hp.has_dynamic_features = case["stream_sizes"], case["has_dynamic_features"]
    hp.windows = C.WINDOWS[:case["windows"]]
    hp.adversarial_streams, hp.mask_nth_mgc_for_adv_loss = case["adversarial_streams"], case["mask_nth_mgc"]
    hp.discriminator_linguistic_condition = case["cond"]
    hp.nepoch, hp.lr_decay_schedule, hp.lr_decay_epoch = 1, False, 10
    hp.generator_add_noise = False
    hp.optimizer_g_params, hp.optimizer_d_params = dict(case["opt_g"][1]), dict(case["opt_d"][1])
    if device_band:
        hp.mlpg_device_band = True
    saved_hp, saved_epoch, saved_log = getattr(T, "hp", None), T.global_epoch, T.log_value
    T.hp, T.global_epoch = hp, 0
    mg, md = build_model(case["g"], 11), build_model(case["d"], 22)
    og = getattr(optim, case["opt_g"][0])(mg.parameters(), **case["opt_g"][1])
    od = getattr(optim, case["opt_d"][0])(md.parameters(), **case["opt_d"][1])
    data, mean, std = C.make_train_loop_data(case)

    class Loader(list):
        pass

    loaders = {}
    for phase in ("train", "test"):
        ld = Loader((torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(l)) for x, y, l in data[phase])
        ld.dataset = types.SimpleNamespace(Y_data_mean=mean, Y_data_std=std)
        loaders[phase] = ld
    logs = []
    T.log_value = lambda n, v, e: logs.append((n, float(v)))
    try:
        assert T.train_loop((mg, md), (og, od), loaders, w_d=1.0, mse_w=0.0, mge_w=1.0) == 0
    finally:
        T.log_value, T.hp, T.global_epoch = saved_log, saved_hp, saved_epoch
    return logs, {t + "." + k: v.cpu().numpy() for t, m in (("G", mg), ("D", md)) for k, v in m.state_dict().items()}


@pytest.mark.gpu
def test_training_and_inference_run_without_a_dense_R(monkeypatch):
    from gantts_amd import inference as INF
    from test_gpu_parity import RTOL, _close
    rs = np.random.RandomState(12)
    Tn = 53
    y_pred = rs.randn(Tn, 187).astype(np.float32)
    mean, std = rs.randn(187) * 0.4, 0.5 + rs.rand(187)
    ref_logs, ref_params = _train_loop_run(False)
    ref_streams = INF.gen_parameters(y_pred, mean, std)
    R53 = np.array(paramgen.unit_variance_mlpg_matrix(INF.hp_acoustic.windows, Tn))

    def no_dense(*a, **k):
        raise AssertionError("the dense MLPG matrix was asked for")

    monkeypatch.setattr(paramgen, "unit_variance_mlpg_matrix", no_dense)
    monkeypatch.setattr(paramgen, "unit_variance_mlpg_matrix_cuda", no_dense)
    monkeypatch.setattr(INF, "unit_variance_mlpg_matrix_cuda", no_dense)
    logs, params = _train_loop_run(True)
    assert [n for n, _ in logs] == [n for n, _ in ref_logs] and len(logs) > 10
    for (n, v), (_, g) in zip(logs, ref_logs):
        if np.isnan(g):
            assert np.isnan(v), (n, v, g)
        elif " acc" in n or "spoofing" in n or "vuv_err" in n:
            assert v == g, (n, v, g)
        else:
            assert abs(v - g) <= RTOL * max(abs(g), 1e-3), (n, v, g)
    for k, v in ref_params.items():
        _close(params[k], v, rtol=RTOL, atol=1e-6, msg="train_loop:" + k)
    got = INF.gen_parameters(y_pred, mean, std, device_band=True)
    hp = INF.hp_acoustic
    scol, sst, Dout, Ds = M.layout(hp.stream_sizes, hp.has_dynamic_features, 3)
    S = abs_product(R53, Tn, 3, scol, sst, y_pred[None])[0]                 # (T, Ds): mgc 60, lf0 1, vuv 1, bap 1
    scale = {"mgc": (S[:, :60], std[:60]), "lf0": (S[:, 60:61], std[180:181]), "bap": (S[:, 62:], std[184:185])}
    for n, v, g in zip(("mgc", "lf0", "vuv", "bap"), got, ref_streams):
        assert v.shape == g.shape
        if n == "vuv":
            assert np.array_equal(v, g)                                     # a copy of a column
        else:
            s, sd = scale[n]
            assert (np.abs(v - g) <= U23 * s * sd[None, :] + 1e-12).all(), n


@pytest.mark.gpu
def test_multi_stream_mlpg_and_vc_convert_accept_the_band():
    """The reference-shaped entry points: multi_stream_mlpg reads num_windows from R.size(1) // R.size(0); vc_convert(device_band=True)."""
    from gantts_amd import inference as INF
    from gantts_amd.multistream import multi_stream_mlpg
    from hip_runner import build_model
    from test_gpu_parity import RTOL, _close
    Tn, ss, hd = 45, [9, 3, 1, 3], [True, True, False, True]
    scol, sst, Dout, Ds = M.layout(ss, hd, 3)
    y = np.random.RandomState(4).randn(2, Tn, Dout).astype(np.float32)
    yd = torch.from_numpy(y).cuda()
    S = abs_product(paramgen.unit_variance_mlpg_matrix(C.WINDOWS, Tn), Tn, 3, scol, sst, y)
    for streams in ([True] * 4, [True, False, True, True]):
        a = multi_stream_mlpg(yd, paramgen.unit_variance_mlpg_matrix_cuda(C.WINDOWS, Tn), ss, hd, streams).cpu().numpy()
        b = multi_stream_mlpg(yd, paramgen.unit_variance_mlpg_band(C.WINDOWS, Tn), ss, hd, streams).cpu().numpy()
        keep = np.repeat(streams, [3, 1, 1, 1])
        assert a.shape == b.shape == (2, Tn, int(keep.sum())) and (np.abs(a.astype(np.float64) - b) <= U23 * S[:, :, keep]).all()
    inp = C.make_inference_inputs()
    mc = np.random.RandomState(6).randn(C.INFERENCE["T_vc"], 75).astype(np.float32)
    res = [INF.vc_convert(build_model(C.INFERENCE["vc"], 43), mc, inp["vc_mean"], inp["vc_std"], diffvc=True, device_band=db) for db in (False, True)]
    np.testing.assert_array_equal(res[0][0], res[1][0])
    _close(res[1][1], res[0][1], rtol=RTOL, atol=1e-6, msg="vc outputs")
    _close(res[1][2], res[0][2], rtol=RTOL, atol=1e-5, msg="vc diff")
