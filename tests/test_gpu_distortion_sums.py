"""The kernels behind the logged metrics -- distortion_kernel<float>, distortion_kernel<double>, distortion_finalize_kernel
(frame_kernels.hip.h), ledger_lengths_kernel (ledger_kernels.hip.h) -- and the two sequence helpers beside them, sequence_mask_kernel and
pad_sequences_kernel, against float64, one sum at a time.

Every case of tests/distortion_ref.py: case_list() runs through train._distortion_sums (gt_compute_distortions: host lengths, per-call
tables) and through StepEngine.ledger_configure / ledger_add / ledger_buffers (device lengths, resident tables); all seven sums are
compared with the reference under ITS bounds (counted in roundings, never measured: the module's docstring), the three counts exactly;
each case runs twice and the two runs agree bit for bit.  Every case carries NaN in its ROLE_NONE columns, in every frame at
t >= lengths[b] of y and y_hat and in every statistics entry no column indexes.  tests/test_distortion_host.py shows on the CPU that
this case list sees ten seeded mistakes.  E = 1 ulp for expf / exp (distortion_ref's docstring says where that was read).

Which case reaches which kernel / branch:

| cases                                         | kernel, branch                                                                              |
|-----------------------------------------------|---------------------------------------------------------------------------------------------|
| every case, -f32 / -f64                       | distortion_kernel<float> / <double>; the vuv column in float32 in both                      |
| 1x1-Ds1, 1x3-Ds5                              | nblk = cdiv(N, 4) = 1 with N < 4: waves without a frame; finalize with nblk = 1             |
| 3x17 (N = 51), 2x9 (N = 18)                   | N not a multiple of 4: the last block's idle waves; finalize with nblk = 13 and 5 (< 64)    |
| Ds63 / Ds64 / Ds65 / Ds130                    | lane loop: one trip with a lane idle / all lanes / a second trip of one lane / three trips  |
| 3x1400-Ds5 (N = 4200)                         | the 1024-block cap, second trip of the frame loop with 104 frames; finalize nblk = 1024     |
| 1x4097-Ds63                                   | the cap with ONE frame in the second trip (wave 0 of block 0), 16 trips of the finalize loop |
| 1030x1-Ds5, 1160x1-Ds5                        | T = 1: b = f; finalize with nblk = 258 / 290 (not multiples of 64); ledger_lengths_kernel's  |
|                                               | second to fifth block; 1160 > 1152 entries: the ledger's length buffer grows                |
| -general- at Ds65 / Ds130, -nolf0-            | roles shuffled, stats[c] != c not monotone, LF0 and VUV above lane 63; a vuv column, no LF0 |
| -mse- / -mcd-                                 | vuv_col = -1: va = vb = false, no LF0 column                                                |
| -none / -full / -ragged / -single             | lengths == null (ledger: in == null) / all T / a 0 in the middle and at the end / one frame  |
| threshold*                                    | inv_scale_rn(float): x with fl(fl(x s) + m) on the other side of 0.5 than fma(x, s, m), on   |
|                                               | 0.5 and on its two neighbours -- in y and in y_hat                                          |
| unvoiced-*                                    | no frame voiced on both sides: the LF0 branch never taken, s_f0 = n_voiced = 0, ledger NaN  |
| test_ledger_cuts_lengths_to_0_T               | ledger_lengths_kernel: n < 0 and n > T, its only branches; the host path refuses the same    |
| test_ledger_after_its_length_buffer_grew      | EpochLedger::len regrown between two adds; the record after four batches                    |
| test_poison_is_not_read                       | both paths: NaN against finite values in the unread places, same bits                       |
| test_sequence_mask, test_pad_sequences        | sequence_mask_kernel, pad_sequences_kernel on guarded buffers                               |
"""
import numpy as np
import pytest
import torch

import distortion_ref as R
import ledger_ref as LR
import resident_ref as RR
from frame_kernels_ref import SENT
from test_gpu_frame_kernels import Buf, inp, rs_of, twice

pytestmark = pytest.mark.gpu

CASES = R.case_list()
BY_ID = {c["id"]: c for c in CASES}
PATHS = ("host", "ledger")


def _lib():
    from gantts_amd import _lib as Lb
    return Lb


def _f64_view(addr, n):
    class _Arr(object):
        __cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (addr, False), "version": 2}
    return torch.as_tensor(_Arr(), device="cuda")


def _kind_of(d):
    """The ledger kind whose slots the layout fills: acoustic with a vuv column, duration for all-MSE, vc for all-MCD."""
    if d["vuv_col"] >= 0:
        return LR.ACOUSTIC
    return LR.DURATION if d["roles"][0] == R.ROLE_MSE else LR.VC


class Device(object):
    """The inputs of a case on the device, uploaded once."""

    def __init__(self, d):
        self.d = d
        self.y, self.yh = torch.from_numpy(np.array(d["y"])).cuda(), torch.from_numpy(np.array(d["yh"])).cuda()
        self.mean, self.std = torch.from_numpy(np.array(d["mean"])).cuda(), torch.from_numpy(np.array(d["std"])).cuda()
        assert self.mean.dtype == (torch.float64 if d["f64"] else torch.float32)

    def host_path(self, lengths="case"):
        import gantts_amd.train as T
        d = self.d
        r = T._distortion_sums(self.y, self.yh, self.mean, self.std, d["roles"], d["stats"], d["vuv_col"], d["lengths"] if lengths == "case" else lengths)
        return [r.s_mcd, r.s_bap, r.s_f0, r.n_voiced, r.n_vuv_err, r.s_mse, r.n_frames]

    def configure(self, eng):
        import gantts_amd.train as T
        d = self.d
        eng.ledger_configure(_kind_of(d), d["roles"], d["stats"], d["vuv_col"], self.mean, self.std, T._LOGDB_CONST)
        eng.ledger_reset()

    def ledger_add(self, eng, lengths="case"):
        """One ledger_add of the batch -> its seven sums, read where gt_ledger_buffers says they are.  No host wait in the add."""
        Lb = _lib()
        lengths = self.d["lengths"] if lengths == "case" else lengths
        lens = None if lengths is None else torch.tensor(lengths, dtype=torch.int64).cuda()
        waits = eng.host_waits()
        eng.ledger_add(Lb.LEDGER_HAS_DIST, self.y, self.yh, lens)
        assert eng.host_waits() == waits, "ledger_add waited for the device"
        torch.cuda.synchronize()
        rec, dist = eng.ledger_buffers()
        assert dist - rec == Lb.LEDGER_SLOTS * 8, "the distortion sums sit behind the record's 32 doubles"
        got = _f64_view(dist, 8).cpu().tolist()
        assert got[7] == 0.0, "the eighth double behind the seven sums was written"
        return got[:7]


@pytest.fixture(scope="module")
def engine():
    from gantts_amd.engine import StepEngine
    return StepEngine(RR.make_hp(RR.SMALL))


def _check(got, case, what, vals=None, bounds=None):
    """Prints every figure, then asserts: the three counts equal, the four sums within the reference's bounds."""
    if vals is None:
        _, vals, bounds = R.case_reference(case)
    lines = ["%-10s got %-24r ref %-24r diff %.3e bound %.3e" % (n, g, v, abs(g - v), b) for n, g, v, b in zip(R.NAMES, got, vals, bounds)]
    print("%s %s\n  %s" % (case["id"], what, "\n  ".join(lines)))
    bad = R.outside(got, vals, bounds)
    assert not bad, "%s %s: %s outside\n  %s" % (case["id"], what, bad, "\n  ".join(lines))


def _slots_of(eng):
    led = eng.ledger_read()
    return [led[k] for k in LR.KEYS]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_sums_against_float64(cid, path, engine):
    import gantts_amd.train as T
    case = BY_ID[cid]
    d, vals, bounds = R.case_reference(case)
    dev = Device(d)
    if path == "host":
        got, again = dev.host_path(), dev.host_path()
    else:
        dev.configure(engine)
        got = dev.ledger_add(engine)
        slots = _slots_of(engine)
        dev.configure(engine)
        again = dev.ledger_add(engine)
    assert LR.same_bits(got, again), "two runs differ: %r %r" % (got, again)
    _check(got, case, path)
    if case["special"] == "unvoiced":
        assert got[R.I_F0] == 0.0 and got[R.I_NV] == 0.0 and not np.signbit(got[R.I_F0])
    if path == "ledger":
        # the record holds this one batch's metrics, formed from the sums just checked; a batch without a voiced frame leaves NaN in
        # f0_rmse and in no other slot
        want = LR.Ledger().add([0.0] * 12, got, LR.HAS_DIST, _kind_of(d), case["Ds"], T._LOGDB_CONST).slots[:len(LR.KEYS)]
        assert LR.same_bits(slots, want), (slots, want)
        nan = [k for k, v in zip(LR.KEYS, slots) if v != v]
        assert nan == (["f0_rmse"] if case["special"] == "unvoiced" or (_kind_of(d) == LR.ACOUSTIC and got[R.I_NV] == 0.0) else []), nan


@pytest.mark.parametrize("cid", ["3x17-Ds63-acoustic-ragged-f32", "3x17-Ds65-general-ragged-f64", "1030x1-Ds5-acoustic-ragged-f32",
                                 "2x9-Ds130-general-ragged-f64", "1x4097-Ds63-mcd-ragged-f32"])
def test_poison_is_not_read(cid, engine):
    """NaN against finite values in the ROLE_NONE columns, the frames beyond the lengths and the unused statistics: the same bits."""
    case = BY_ID[cid]
    d, vals, bounds = R.case_reference(case)
    clean = R.make_case(case, poison=False)
    assert np.isnan(d["y"]).any() and not np.isnan(clean["y"]).any() and not np.isnan(clean["mean"]).any()
    a, b = Device(d), Device(clean)
    got, ref = a.host_path(), b.host_path()
    assert all(np.isfinite(got)) and LR.same_bits(got, ref), (got, ref)
    _check(got, case, "host, poisoned")
    a.configure(engine)
    got = a.ledger_add(engine)
    b.configure(engine)
    ref = b.ledger_add(engine)
    assert all(np.isfinite(got)) and LR.same_bits(got, ref), (got, ref)
    _check(got, case, "ledger, poisoned")


@pytest.mark.parametrize("cid", ["3x17-Ds63-acoustic-none-f32", "1030x1-Ds5-acoustic-none-f64"])
def test_ledger_cuts_lengths_to_0_T(cid, engine):
    """Device lengths of -3 and T + 5 give the sums of 0 and T (ledger_lengths_kernel's two branches); gt_compute_distortions, which
    sees the lengths on the host, refuses them with GT_ERR_INVALID."""
    B, T, Ds = (3, 17, 63) if cid.startswith("3x17") else (1030, 1, 5)
    case = dict(id=cid, B=B, T=T, Ds=Ds, layout="acoustic", lengths="none", f64=cid.endswith("f64"), special=None)
    d = R.make_case(case)
    rs = rs_of(B, T, 5)
    raw = [int(v) for v in rs.randint(0, T + 1, B)]
    raw[0], raw[1], raw[2] = -3, T + 5, max(1, T // 2)
    if B > 3:
        raw[B - 1], raw[B - 2], raw[700] = T + 5, -3, -(1 << 40)
    cut = R.clip_lengths(raw, B, T)
    assert cut[0] == 0 and cut[1] == T and cut != raw
    dead = np.arange(T)[None, :] >= np.asarray(cut)[:, None]
    d["y"][dead], d["yh"][dead] = np.nan, np.nan
    vals, bounds = R.sums(d["y"], d["yh"], d["mean"], d["std"], d["roles"], d["stats"], d["vuv_col"], cut, d["f64"])
    assert vals[R.I_N] == sum(cut) > 0
    dev = Device(d)
    dev.configure(engine)
    got = dev.ledger_add(engine, raw)
    dev.configure(engine)
    again = dev.ledger_add(engine, raw)
    assert LR.same_bits(got, again)
    _check(got, case, "ledger, lengths outside [0, T]", vals, bounds)
    _check(dev.host_path(cut), case, "host, the cut lengths", vals, bounds)
    Lb = _lib()
    for bad in (raw, [-3] + cut[1:], cut[:1] + [T + 5] + cut[2:]):
        with pytest.raises(ValueError):        # _lib.check: GT_ERR_INVALID
            dev.host_path(bad)
        assert b"outside [0, T=" in Lb.lib.gt_last_error()


def test_ledger_after_its_length_buffer_grew():
    """A fresh engine: 51 frames, then 1030 sequences (inside the first 1152 entries), then 1160 (the buffer is freed and allocated
    anew between two adds), then 51 frames again.  Every batch's sums are checked against the reference, and the record after the
    four adds is the sum of ledger_ref.batch_metrics of those checked sums, bit for bit."""
    import gantts_amd.train as T
    from gantts_amd.engine import StepEngine
    eng = StepEngine(RR.make_hp(RR.SMALL))
    order = ["1x3-Ds5-acoustic-ragged-f32", "1030x1-Ds5-acoustic-ragged-f32", "1160x1-Ds5-acoustic-ragged-f32", "1030x1-Ds5-acoustic-none-f32",
             "1x3-Ds5-acoustic-ragged-f32"]
    devs = [Device(R.case_reference(BY_ID[i])[0]) for i in order]
    # one layout, one pair of statistics tables for the whole phase: the cases share Ds = 5 and the acoustic layout; the tables differ
    # by case, so each batch is re-referenced with the first case's tables
    first = devs[0].d
    devs[0].configure(eng)
    ref = LR.Ledger()
    for cid, dv in zip(order, devs):
        d = dv.d
        assert (d["roles"], d["stats"], d["vuv_col"]) == (first["roles"], first["stats"], first["vuv_col"])
        vals, bounds = R.sums(d["y"], d["yh"], first["mean"], first["std"], d["roles"], d["stats"], d["vuv_col"], d["lengths"], False)
        got = dv.ledger_add(eng)
        _check(got, BY_ID[cid], "ledger, one phase", vals, bounds)
        ref.add([0.0] * 12, got, LR.HAS_DIST, LR.ACOUSTIC, 5, T._LOGDB_CONST)
    waits = eng.host_waits()
    slots = _slots_of(eng)
    assert eng.host_waits() == waits + 1
    assert LR.same_bits(slots, ref.slots[:len(LR.KEYS)]), (slots, ref.slots)
    assert slots[LR.KEYS.index("mcd")] > 0 and slots[LR.KEYS.index("vuv_err")] > 0 and slots[LR.KEYS.index("f0_rmse")] > 0


# ---------------------------------------------------------------------------------------------------------------------
# the sequence helpers
# ---------------------------------------------------------------------------------------------------------------------
def _i64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int64)).cuda()


def _seq_length_sets(B, T):
    if B == 1:
        return [[0], [T], [T + 3]] + ([[T - 1]] if T > 1 else [])
    return [R.seq_lengths(B, T, rs_of(B, T, s)) for s in (1, 2)] + [[T] * B, [0] * B]


@pytest.mark.parametrize("lead", [8, 9], ids=["aligned", "plus1float"])
@pytest.mark.parametrize("B,T", R.SEQ_SHAPES)
def test_sequence_mask(B, T, lead):
    Lb = _lib()
    for lengths in _seq_length_sets(B, T):
        def run():
            out = Buf(np.full((1, B * T), np.nan, dtype=np.float32), None, SENT, lead=lead)
            assert (out.ptr % 16 == 0) == (lead == 8)
            lens = _i64(lengths)
            assert Lb.lib.gt_op_sequence_mask(Lb.ptr(lens), B, T, out.ptr, Lb.current_stream()) == 0, Lb.lib.gt_last_error()
            torch.cuda.synchronize()
            return (out.result("sequence_mask %dx%d" % (B, T)),)
        got, = twice(run)
        want = R.sequence_mask_ref(lengths, T).reshape(1, B * T)
        assert got.tobytes() == want.tobytes(), (B, T, lengths)


@pytest.mark.parametrize("lead", [8, 9], ids=["aligned", "plus1float"])
@pytest.mark.parametrize("D,pad", [(1, 0), (1, 3), (5, 0), (5, 3)], ids=["D1", "D1-ld4", "D5", "D5-ld8"])
@pytest.mark.parametrize("B,T", R.SEQ_SHAPES)
def test_pad_sequences(B, T, D, pad, lead):
    """Utterances back to back in one order, asked for in another (start not ascending); a length of T + 3 copies T frames; every pad
    column and pad frame is +0.0; nothing around the [B T][ld] result is written."""
    Lb = _lib()
    ld = D + pad
    for lengths in _seq_length_sets(B, T):
        rs = rs_of(B, T, D, sum(lengths))
        order = rs.permutation(B)                            # where each utterance lies in the ragged buffer
        start = np.zeros(B, dtype=np.int64)
        pos = 2                                              # two frames nobody asks for in front
        for b in order[::-1] if B > 1 else order:
            start[b] = pos
            pos += lengths[b]
        ragged = rs.randn(pos + 2, D).astype(np.float32)
        ragged[ragged == 0] = 1.0
        if B > 2 and sum(lengths) > 0:
            assert any(start[b] > start[b + 1] for b in range(B - 1))

        def run():
            rg = inp(ragged)
            out = Buf(np.full((B * T, ld), np.nan, dtype=np.float32), None, SENT, lead=lead)
            assert (out.ptr % 16 == 0) == (lead == 8)
            st, ln = _i64(start), _i64(lengths)
            assert Lb.lib.gt_op_pad_sequences(rg.ptr, D, Lb.ptr(st), Lb.ptr(ln), B, T, out.ptr, ld, Lb.current_stream()) == 0, Lb.lib.gt_last_error()
            torch.cuda.synchronize()
            return (out.result("pad_sequences %dx%dx%d ld %d" % (B, T, D, ld)),)
        got, = twice(run)
        want = R.pad_sequences_ref(ragged, start, lengths, T, ld).reshape(B * T, ld)
        assert got.tobytes() == want.tobytes(), (B, T, D, ld, lengths)      # bytes: a pad of -0.0 is not +0.0


def test_sequence_helpers_refuse_bad_arguments():
    Lb = _lib()
    st = Lb.current_stream()
    lens, out, rg = _i64([1, 2]), torch.zeros(64, device="cuda"), torch.ones(64, device="cuda")
    p = Lb.ptr
    assert Lb.lib.gt_op_sequence_mask(p(lens), 0, 4, p(out), st) == Lb.GT_ERR_INVALID
    assert Lb.lib.gt_op_sequence_mask(p(lens), 2, 0, p(out), st) == Lb.GT_ERR_INVALID
    assert Lb.lib.gt_op_sequence_mask(None, 2, 4, p(out), st) == Lb.GT_ERR_INVALID
    assert Lb.lib.gt_op_pad_sequences(p(rg), 3, p(lens), p(lens), 2, 4, p(out), 2, st) == Lb.GT_ERR_INVALID      # ld_out < D
    assert Lb.lib.gt_op_pad_sequences(p(rg), 0, p(lens), p(lens), 2, 4, p(out), 2, st) == Lb.GT_ERR_INVALID
    assert Lb.lib.gt_op_pad_sequences(None, 1, p(lens), p(lens), 2, 4, p(out), 2, st) == Lb.GT_ERR_INVALID
    torch.cuda.synchronize()
    assert not out.any()
