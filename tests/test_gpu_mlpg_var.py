"""Variance-weighted MLPG on the device (gt_op_mlpg_var, gantts_amd/csrc/mlpg_var_kernels.hip.h) against the float64 host reference of
tests/mlpg_var_ref.py (nnmnkwii.paramgen.mlpg restated; held against a dense construction by tests/test_mlpg_var_host.py).

Bound, for every dynamic output element:  |dev - ref| <= 2^-24 |ref| + 2^-40 peak  (peak: the largest |ref| of the element's column) -- one
float32 rounding and the float64 solve's error at cond(P) <= 2^11, which the host test asserts for every case used here.  No element is
exempt.  Pass-through columns and the zero rows beyond a length are compared bit for bit; outputs sit in NaN-filled buffers with
ldys > Ds, and the pad must stay NaN.

  cases       window sets std, static, delta, asym, four and the hb = 1 pair (hb 2, 0, 2, 2, 4, 1: both register forms and the generic
              kernel, shown by gt_mlpg_var_path_counts) x T in 1, 2, 3, 5, 17, 65, 200 x variances all ones / one row / per frame,
              B = 3 with lengths [T, T // 2 + 1, 1]
  groups      B = 9 on the 8-column layout (72 columns: a second workgroup with a part-filled wave), in one group and in three
  unit        all-ones variances against the banded mlpg_forward of the same input, within the bound test_gpu_mlpg.py derives for it
  refusals    a zero, a negative, a NaN, an infinite variance; the malformed cases; the engine serves afterwards
  surface     paramgen.mlpg / mlpg_batch, StepEngine.mlpg_var, inference.gen_parameters_without_mge; gen_parameters unchanged
"""
import ctypes as Ct
import hashlib

import numpy as np
import pytest
import torch

import mlpg_var_ref as V
import test_gpu_mlpg as M
from test_gpu_gemm_b16 import _F32, pads_intact

NAN = np.float32(np.nan)
SETS = V.window_sets()
SLOT_OF_HB = {1: 0, 2: 1}      # gt_mlpg_var_path_counts: solve<1>, solve<2>; everything else the generic kernel (2)
_ENG = {}


def engine(name, fresh=False):
    """an engine on the [3n, 3, 1, 3]-shaped 8-column layout of test_gpu_mlpg.streams with the set's windows registered"""
    from gantts_amd import paramgen
    if fresh or name not in _ENG:
        nW = len(SETS[name])
        eng = M.engine(*M.streams(5, nW), nW, fresh=True)
        eng._register_windows(paramgen.MLPGBand(SETS[name], 1))
        if fresh:
            return eng
        _ENG[name] = eng
    return _ENG[name]


def counts(reset=False):
    from gantts_amd import _lib as Lb
    if reset:
        Lb.check(Lb.lib.gt_mlpg_var_path_counts(None, 0))
        return None
    out = (Ct.c_int64 * Lb.MLPG_VAR_PATH_SLOTS)()
    Lb.check(Lb.lib.gt_mlpg_var_path_counts(out, Lb.MLPG_VAR_PATH_SLOTS))
    return list(out)


def call(eng, y, var, lengths, max_ws_bytes=0, edit=None):
    """One gt_op_mlpg_var call on the engine's own maps.  Returns (rc, result [B][T][Ds] or None, launches per kernel)."""
    from gantts_amd import _lib as Lb
    B, T, D = y.shape
    Ds = eng.static_dim
    src = _F32(np.ascontiguousarray(y).reshape(B * T, D), D, 0, NAN)
    vv = torch.from_numpy(np.array(var)).cuda()
    dst = _F32(np.full((B * T, Ds), NAN, np.float32), Ds + 3, 5, NAN)
    g = Lb.MlpgVarCase()
    g.e, g.B, g.T, g.Ds, g.ldy, g.ldv, g.ldys = eng._h, B, T, 0, D, 0 if var.ndim == 1 else D, dst.ld
    if lengths is not None:
        g.lengths = (Ct.c_int64 * B)(*lengths)
    g.y, g.var, g.ys, g.max_ws_bytes = src.ptr, vv.data_ptr(), dst.ptr, max_ws_bytes
    if edit:
        edit(g)
    counts(reset=True)
    rc = Lb.lib.gt_op_mlpg_var(Ct.byref(g), M._stream())
    if rc == Lb.GT_ERR_HIP:      # a device error: nothing more is launched in this session
        pytest.exit("gt_op_mlpg_var: %s" % Lb.lib.gt_last_error(), returncode=3)
    n = counts()
    if rc != Lb.GT_OK:
        return rc, None, n
    flat, got = dst.got()
    assert pads_intact(flat, dst.inside(), NAN), "written outside the result"
    return rc, got.reshape(B, T, Ds), n


def expect_launches(name, groups):
    want = [0, 0, 0]
    want[SLOT_OF_HB.get(V.half_bandwidth(SETS[name]), 2)] = groups
    return want


# ---------------------------------------------------------------------------------------------------------------------
# 1. every form against the reference
# ---------------------------------------------------------------------------------------------------------------------
CASES = [(n, T, f) for n in V.SET_NAMES for T in V.T_VALUES for f in V.VAR_FORMS]


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,form", CASES, ids=["%s_T%d_%s" % c for c in CASES])
def test_solve_against_float64(name, T, form):
    from gantts_amd import _lib as Lb
    _, _, scol, sst, _, _ = V.layout(5, len(SETS[name]))
    y, var, lengths, ref = V.case(name, T, form)
    rc, got, n = call(engine(name), y, var, lengths)
    assert rc == Lb.GT_OK, Lb.lib.gt_last_error()
    assert n == expect_launches(name, 1), "launch census %s" % n
    worst, over, bad = V.compare(got, ref, y, scol, sst, lengths)
    print("%s T=%d %s: worst |dev - ref| / bound %.4f, %d over, %d exact elements differ" % (name, T, form, worst, over, bad))
    assert over == 0 and bad == 0 and worst <= 1.0


@pytest.mark.gpu
def test_nine_sequences_in_one_group_and_in_three():
    from gantts_amd import _lib as Lb
    name, T, B = "std", 65, 9
    _, _, scol, sst, _, Ds = V.layout(5, 3)
    y, var, _ = V.make_inputs(name, T, "frame", B=B, seed=7)
    lengths = [65, 33, 1, 64, 2, 17, 65, 5, 40]
    ref = V.reference(y, var, SETS[name], scol, sst, lengths)
    rc, one, n = call(engine(name), y, var, lengths)
    assert rc == Lb.GT_OK and n == expect_launches(name, 1), (Lb.lib.gt_last_error(), n)
    worst, over, bad = V.compare(one, ref, y, scol, sst, lengths)
    print("B=9: worst |dev - ref| / bound %.4f" % worst)
    assert over == 0 and bad == 0
    per_seq = 8 * (V.half_bandwidth(SETS[name]) + 2) * T * Ds
    rc, three, n = call(engine(name), y, var, lengths, max_ws_bytes=3 * per_seq + per_seq // 2)
    assert rc == Lb.GT_OK and n == expect_launches(name, 3), (Lb.lib.gt_last_error(), n)
    assert np.array_equal(one.view(np.uint32), three.view(np.uint32))
    rc, _, n = call(engine(name), y, var, lengths, max_ws_bytes=per_seq - 1)      # not one sequence: refused before any launch
    assert rc == Lb.GT_ERR_INVALID and b"scratch" in Lb.lib.gt_last_error() and n == [0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# 2. unit variance: the R the step uses
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,T", [("std", 65), ("std", 200), ("delta", 17), ("four", 65)])
def test_unit_variance_equals_the_banded_forward(name, T):
    from gantts_amd import _lib as Lb
    nW = len(SETS[name])
    ss, hd = M.streams(5, nW)
    scol, sst, Dout, Ds = M.layout(ss, hd, nW)
    y = M.random_case(T, Dout, Ds, 2, False, 31 * T + nW)
    kb = M.kb_of(name, T)
    ref, lim, pt = M.reference(M.matrix(name, T), T, nW, kb, scol, sst, Dout, y, False)
    eng = engine(name)
    banded = eng.mlpg_forward(torch.from_numpy(y).cuda(), M.r_dev(name, T)).cpu().numpy()
    rc, got, _ = call(eng, y, np.ones(Dout, np.float32), None)
    assert rc == Lb.GT_OK, Lb.lib.gt_last_error()
    err = np.abs(got.astype(np.float64) - banded.astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(pt, 0.0, err / lim)
    print("%s T=%d: worst |var - banded| / limit %.4f" % (name, T, ratio.max()))
    assert np.isfinite(got).all() and (ratio <= 1.0).all()
    assert np.array_equal(got[pt].view(np.uint32), banded[pt].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 3. refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")], ids=["zero", "negative", "nan", "inf"])
@pytest.mark.parametrize("name", ["std", "hb1", "four"])
def test_bad_variances_are_refused_and_the_engine_serves_afterwards(name, bad):
    _, _, scol, sst, D, _ = V.layout(5, len(SETS[name]))
    eng = engine(name)
    y, var, lengths, ref = V.case(name, 17, "frame")
    yd = torch.from_numpy(np.array(y)).cuda()
    dyn = np.nonzero(sst > 0)[0]
    last = int(scol[dyn[-1]] + (len(SETS[name]) - 1) * sst[dyn[-1]])
    for (b, t, c) in ((0, 16, 0), (1, lengths[1] - 1, last), (2, 0, int(scol[dyn[1]]))):      # first and last frames and columns of a sequence
        v = np.array(var)
        v[b, t, c] = bad
        with pytest.raises(ValueError, match="variances must be finite and positive"):
            eng.mlpg_var(yd, torch.from_numpy(v).cuda(), lengths=lengths, windows=SETS[name])
    y1, row, _, ref1 = V.case(name, 17, "row")
    v = np.array(row)
    v[last] = bad
    with pytest.raises(ValueError, match="variances must be finite and positive"):
        eng.mlpg_var(torch.from_numpy(np.array(y1)).cuda(), torch.from_numpy(v).cuda(), lengths=lengths, windows=SETS[name])
    got = eng.mlpg_var(yd, torch.from_numpy(np.array(var)).cuda(), lengths=lengths, windows=SETS[name]).cpu().numpy()
    _, over, wrong = V.compare(got, ref, y, scol, sst, lengths)
    assert over == 0 and wrong == 0


@pytest.mark.gpu
def test_malformed_cases_are_refused_before_any_launch():
    from gantts_amd import _lib as Lb
    name = "std"
    eng = engine(name)
    y, var, lengths, ref = V.case(name, 17, "frame")
    _, _, scol, sst, D, Ds = V.layout(5, 3)
    maps = [torch.from_numpy(np.asarray(a, np.int32)).cuda() for a in (scol, sst)]

    def own_maps(g):
        g.scol, g.sstride, g.Ds = maps[0].data_ptr(), maps[1].data_ptr(), Ds

    edits = {
        "null y": lambda g: setattr(g, "y", None),
        "null var": lambda g: setattr(g, "var", None),
        "null ys": lambda g: setattr(g, "ys", None),
        "null engine": lambda g: setattr(g, "e", None),
        "scol alone": lambda g: setattr(g, "scol", maps[0].data_ptr()),
        "T = 0": lambda g: setattr(g, "T", 0),
        "B = 0": lambda g: setattr(g, "B", 0),
        "length 0": lambda g: setattr(g, "lengths", (Ct.c_int64 * 3)(17, 0, 1)),
        "length T + 1": lambda g: setattr(g, "lengths", (Ct.c_int64 * 3)(17, 18, 1)),
        "ldys < Ds": lambda g: setattr(g, "ldys", Ds - 1),
        "ldy below the maps": lambda g: setattr(g, "ldy", D - 1),
        "ldv below the maps": lambda g: setattr(g, "ldv", D - 1),
        "ldv below its own maps": lambda g: (own_maps(g), setattr(g, "ldv", D - 1)),
        "Ds against the engine's maps": lambda g: setattr(g, "Ds", Ds + 1),
        "negative cap": lambda g: setattr(g, "max_ws_bytes", -1),
    }
    for what, edit in edits.items():
        rc, _, n = call(eng, y, var, lengths, edit=edit)
        assert rc == Lb.GT_ERR_INVALID and n == [0, 0, 0], "%s: rc %d, launches %s" % (what, rc, n)
    bare = M.engine(*M.streams(5, 3), 3, fresh=True)      # no registered windows
    rc, _, n = call(bare, y, var, lengths)
    assert rc == Lb.GT_ERR_INVALID and b"gt_set_mlpg_windows" in Lb.lib.gt_last_error() and n == [0, 0, 0]
    rc, got, n = call(eng, y, var, lengths, edit=own_maps)      # the caller's maps, and the engine after the refusals
    assert rc == Lb.GT_OK and n == [0, 1, 0], Lb.lib.gt_last_error()
    _, over, wrong = V.compare(got, ref, y, scol, sst, lengths)
    assert over == 0 and wrong == 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. the public surface
# ---------------------------------------------------------------------------------------------------------------------
def _single_stream(name, T, form, B=None, seed=3):
    """(means, variances) of one stream with dynamic features, static width 4, and the maps of that layout"""
    nW = len(SETS[name])
    D = 4 * nW
    rs = np.random.RandomState(seed + T)
    shape = (T, D) if B is None else (B, T, D)
    y = rs.randn(*shape).astype(np.float32)
    var = (4.0 ** rs.uniform(-1, 1, D if form == "row" else shape)).astype(np.float32)
    return y, var, np.arange(4), np.full(4, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["row", "frame"])
@pytest.mark.parametrize("kind", ["numpy", "numpy64", "tensor"])
def test_paramgen_mlpg(kind, form):
    from gantts_amd import paramgen
    T = 33
    y, var, scol, sst = _single_stream("std", T, form)
    ref = V.reference(y[None], var if form == "row" else var[None], SETS["std"], scol, sst, [T])
    if kind == "tensor":
        out = paramgen.mlpg(torch.from_numpy(y).cuda(), torch.from_numpy(var).cuda(), SETS["std"])
        assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32
        got = out.cpu().numpy()
    elif kind == "numpy64":
        out = paramgen.mlpg(y.astype(np.float64), var.astype(np.float64), SETS["std"])
        assert isinstance(out, np.ndarray) and out.dtype == np.float64
        got = out.astype(np.float32)
        assert np.array_equal(got.astype(np.float64), out)      # float32 values: the device's rounding, nothing on top
    else:
        got = paramgen.mlpg(y, var, SETS["std"])
        assert isinstance(got, np.ndarray) and got.dtype == np.float32
    assert got.shape == (T, 4)
    _, over, wrong = V.compare(got[None], ref, y[None], scol, sst, [T])
    assert over == 0 and wrong == 0


@pytest.mark.gpu
def test_paramgen_mlpg_refuses_bad_variances_with_a_value_error():
    from gantts_amd import paramgen
    y, var, _, _ = _single_stream("std", 9, "row")
    var[5] = 0.0
    with pytest.raises(ValueError, match="finite and positive"):
        paramgen.mlpg(y, var, SETS["std"])


@pytest.mark.gpu
def test_paramgen_mlpg_batch_with_ragged_lengths():
    from gantts_amd import paramgen
    B, T = 3, 21
    lengths = V.ragged_lengths(T)
    for name in ("std", "hb1", "four"):
        y, var, scol, sst = _single_stream(name, T, "frame", B=B)
        got = paramgen.mlpg_batch(y, var, SETS[name], lengths=lengths)
        assert got.shape == (B, T, 4) and got.dtype == np.float32
        _, over, wrong = V.compare(got, V.reference(y, var, SETS[name], scol, sst, lengths), y, scol, sst, lengths)
        assert over == 0 and wrong == 0, name
    t = paramgen.mlpg_batch(torch.from_numpy(y).cuda(), torch.from_numpy(var).cuda(), SETS["four"], lengths=torch.tensor(lengths))
    assert np.array_equal(t.cpu().numpy().view(np.uint32), got.view(np.uint32))


def _acoustic_input(T=50):
    rs = np.random.RandomState(1234)
    y = rs.randn(T, 187).astype(np.float32)
    mean = rs.randn(187)
    std = 4.0 ** rs.uniform(-1, 1, 187)
    return y, mean, std


@pytest.mark.gpu
def test_gen_parameters_without_mge_against_the_reference_stream_by_stream():
    from gantts_amd import hparams, inference
    hp = hparams.tts_acoustic
    assert list(hp.stream_sizes) == [180, 3, 1, 3] and len(hp.windows) == 3
    y, mean, std = _acoustic_input()
    T = len(y)
    mgc, lf0, vuv, bap = inference.gen_parameters_without_mge(y, {"acoustic": mean}, {"acoustic": std})
    plain = inference.gen_parameters_without_mge(torch.from_numpy(y), mean, std)
    den = (y.astype(np.float64) * std + mean).astype(np.float32)      # what the device is given
    var = (std * std).astype(np.float32)
    for got, again, (start, size) in zip((mgc, lf0, bap), (plain[0], plain[1], plain[3]), ((0, 180), (180, 3), (184, 3))):
        w = size // 3
        assert got.shape == (T, w) and got.dtype == np.float64 and np.array_equal(got, again)
        scol, sst = np.arange(w), np.full(w, w)
        ref = V.reference(den[None, :, start:start + size], var[start:start + size], hp.windows, scol, sst, [T])
        _, over, wrong = V.compare(got[None].astype(np.float32), ref, den[None, :, start:start + size], scol, sst, [T])
        assert over == 0 and wrong == 0
        assert np.array_equal(got.astype(np.float32).astype(np.float64), got)
    assert vuv.shape == (T,) and np.array_equal(vuv, y[:, 183].astype(np.float64) * std[183] + mean[183]) and np.array_equal(vuv, plain[2])


# sha256 over the float64 bytes of (mgc, lf0, vuv, bap) of _acoustic_input(), from a run of the commit BEFORE variance-weighted MLPG
MGE_DIGEST = "5ff41de8e9f556e47eaa5baa737ff64dcf34c9307e0da7193e940c76d6ff4a03"


@pytest.mark.gpu
def test_gen_parameters_with_mge_keeps_its_bits():
    from gantts_amd import inference
    y, mean, std = _acoustic_input()
    out = inference.gen_parameters(y, {"acoustic": mean}, {"acoustic": std}, mge_training=True)
    h = hashlib.sha256()
    for a in out:
        assert a.dtype == np.float64
        h.update(np.ascontiguousarray(a).tobytes())
    assert h.hexdigest() == MGE_DIGEST
