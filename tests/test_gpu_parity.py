"""-m gpu parity tests: the HIP path (through the C ABI, via the reference-shaped Python API)
against (a) the golden fixtures generated from the REAL reference and (b) the CPU oracle on the
same seeded inputs.  Tolerance: 1e-4 relative on float32 (BASELINE.json north_star); counts and
stream-split / vuv indexing bit-exact."""
import os

import numpy as np
import pytest
import torch

import cases as C
import gantts_oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL = 1e-4


def _scale_of(b, msg):
    """Comparison scale of every element: tensors with a feature axis are judged PER COLUMN of their last dimension
    (each stream column of a (B,T,D) frame tensor against that column's own magnitude, so the small lf0 / bap columns
    are not hidden behind mgc), weight matrices additionally per row (output unit): scale[i,j] = min(row_i, col_j).
    Vectors and scalars use their own max."""
    ab = np.abs(b)
    if b.ndim < 2 or b.shape[-1] == 1 or (b.ndim == 2 and b.shape[0] == 1):      # (a (1, K) weight -- out_dim 1 -- is a vector)
        return np.full(b.shape, max(1e-30, float(ab.max()) if b.size else 1e-30))
    col = ab.reshape(-1, b.shape[-1]).max(0)
    scale = np.broadcast_to(col, b.shape).copy()
    if b.ndim == 2 and "weight" in msg:
        scale = np.minimum(scale, ab.max(1, keepdims=True))
    return np.maximum(scale, 1e-30)


_REPORT = os.environ.get("GT_PARITY_REPORT")     # dev aid: append "msg worst-ratio" lines instead of judging blind


def _close(a, b, rtol=RTOL, atol=1e-6, msg="", frac_ok=0.0):
    """|a - b| <= atol + rtol * scale element-wise, scale per column / row (see _scale_of).  frac_ok > 0 tolerates that
    fraction of outliers (only for documented discontinuities such as the first Adagrad step, lr * sign(g))."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    if not a.size:
        return
    err = np.abs(a - b)
    lim = atol + rtol * _scale_of(b, msg)
    ratio = err / lim
    worst = float(ratio.max())
    if _REPORT:
        with open(_REPORT, "a") as f:
            f.write("%-60s worst %.3f  frac>1 %.2e  rtol %.0e atol %.0e shape %s\n" % (msg, worst, float((ratio > 1).mean()), rtol, atol, a.shape))
        return                       # report mode collects every comparison of a run and judges none
    bad = float((ratio > 1).mean())
    assert bad <= frac_ok, "%s: %.3e of the elements outside tolerance, worst error %.2fx the limit (rtol %.0e, atol %.0e)" % (
        msg, bad, worst, rtol, atol)


def _kink_frac(case):
    """Fraction of a parameter tensor's elements that may sit outside the flat 1e-4 because of LeakyReLU slope flips, for the
    small-case comparisons that have no float64 arbiter.  LeakyReLU is differentiated by the sign of its stored output
    (gantts/models.py:132): a pre-activation within rounding (~1e-7 relative) of 0 picks slope 1 or 0.01, so two correct float32
    evaluations with different summation orders disagree on a given activation with probability p ~ 1e-7 (measured by the slope
    census of the at-size fixtures, tests/golden/at_size.py), and each disagreement moves the gradient of ONE unit's bias (and its
    weight row) by about one frame's dZ -- about 1 % of an element that is a sum over thousands of frames with random signs.  A case
    with more than 1e6 LeakyReLU activations (cfg3 / cfg4 widths at T ~ 64 .. 96: 1.4e7) expects about one flip per run; cases
    below that get the flat rule.  Returns (frac_ok, worst_ok)."""
    acts = 0
    for spec, passes in ((case["g"], 1), (case["d"], 3)):
        if spec["kind"] in ("MLP", "In2OutHighwayNet"):
            acts += case["B"] * case["T"] * spec["hidden_dim"] * spec["num_hidden"] * passes * case["steps"]
    return (0.01, 20.0) if acts > 1e6 else (0.0, 0.0)


def _close_kink(a, b, msg, frac_ok, worst_ok, **kw):
    """_close with the documented LeakyReLU-flip allowance: at most frac_ok of the elements outside, none by more than worst_ok x."""
    if frac_ok <= 0.0:
        return _close(a, b, msg=msg, **kw)
    _close(a, b, msg=msg, frac_ok=frac_ok, **kw)
    kw = dict(kw)
    _close(a, b, msg=msg + " (worst element)", rtol=kw.pop("rtol", RTOL) * worst_ok, **kw)


def _close_state(got, ref, msg):
    """Optimizer state at the suite's 1e-4: first moments (Adam exp_avg) directly; second moments (Adagrad `sum`, Adam
    `exp_avg_sq`) are sums of SQUARED gradients -- a gradient that is right to 1e-4 gives a second moment that is right to
    2e-4 -- so they are compared on the scale the update uses them on, their square root (p -= lr * g / (sqrt(sum) + eps))."""
    if ".opt.sum." in msg or ".opt.exp_avg_sq." in msg:
        _close(np.sqrt(np.maximum(np.asarray(got, dtype=np.float64), 0.0)), np.sqrt(np.maximum(np.asarray(ref, dtype=np.float64), 0.0)),
               rtol=RTOL, atol=1e-9, msg=msg + " (sqrt)")
    else:
        _close(got, ref, rtol=RTOL, atol=1e-9, msg=msg)


def test_library_loaded_is_the_hip_one():
    import gantts_amd._lib as L
    assert os.path.isfile(L.LIB_PATH)
    assert b"gfx950" in L.lib.gt_version()


# reference goldens whose discriminator the fused stack takes (MLP, hidden_dim 128 / 256): run a second time with the fused launches
# forced (GT_OPT_FUSED_DSTACK = 2; the default takes them only for passes with a panel per CU, which no small golden has)
_FUSED_GOLDENS = [n for n, c in sorted(C.CASES.items()) if c["d"]["kind"] == "MLP" and c["d"]["hidden_dim"] in (128, 256)]


@pytest.mark.parametrize("name,fused", [(n, 0) for n in sorted(C.CASES)] + [(n, 2) for n in _FUSED_GOLDENS])
def test_step_matches_reference_golden(name, fused):
    from hip_runner import run_hip_case
    case = C.CASES[name]
    gold = np.load(os.path.join(GOLDEN, name + ".npz"))
    got = run_hip_case(case, engine_options={"fused_dstack": 2} if fused else None)
    for k in gold.files:
        if k.startswith("g_leak_norm"):
            continue
        assert k in got, k
        g, o = gold[k], got[k]
        if "scalars" in k:
            _close(o, g, rtol=RTOL, atol=1e-6, msg=k)
            if k.startswith("d_scalars"):
                assert o[3] == g[3] and o[4] == g[4], (k, o, g)   # classification counts exact
        elif ".opt." in k:
            _close_state(o, g, k)
        else:
            _close(o, g, rtol=RTOL, atol=1e-6, msg=k)
    # vuv stream is a pass-through copy: bit-exact
    if case["stream_sizes"] == [180, 3, 1, 3]:
        assert np.array_equal(got["y_hat_static"][:, :, 61], got["y_hat"][:, :, 183])


def test_leak_gradient_matches_reference():
    """||G.grad|| right after update_discriminator alone (the un-detached D-loss leak, train.py:265,274)."""
    import gantts_amd.train as T
    from gantts_amd import optim, paramgen
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model, make_hp
    name = "acoustic_d_warmup"
    case = C.CASES[name]
    gold = np.load(os.path.join(GOLDEN, name + ".npz"))
    T.hp = make_hp(case)
    mg, md = build_model(case["g"], 11).eval(), build_model(case["d"], 22).eval()
    od = optim.Adagrad(md.parameters(), **case["opt_d"][1])
    x_np, y_np, lengths = C.make_batch(case)
    x, y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
    R = paramgen.unit_variance_mlpg_matrix_cuda(T.hp.windows, case["T"])
    y_static = get_static_features(y, 3, T.hp.stream_sizes, T.hp.has_dynamic_features)
    mask = sequence_mask(torch.from_numpy(lengths).cuda()).unsqueeze(-1)
    y_hat, y_hat_static = T.apply_generator(mg, x, R, list(lengths))
    T.update_discriminator(md, od, x, y_static, y_hat_static, list(lengths), mask, "train")
    y_hat_static._gt_engine.flush_generator_grads()
    gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in mg.parameters())))
    assert gn == pytest.approx(float(gold["g_leak_norm_0"]), rel=2e-4)


@pytest.mark.parametrize("rows,din,dout,act", [(77, 425, 512, 1), (1000, 512, 187, 0), (300, 483, 256, 1),
                                               (129, 25, 25, 2), (4096, 256, 58, 0), (33, 7, 3, 1)])
def test_linear_forward_backward_vs_torch(rows, din, dout, act):
    import ctypes as Ct
    from gantts_amd._lib import check, lib, ptr
    rs = np.random.RandomState(rows + din)
    X = torch.from_numpy(rs.randn(rows, din).astype(np.float32))
    W = torch.from_numpy((rs.randn(dout, din) / np.sqrt(din)).astype(np.float32))
    b = torch.from_numpy(rs.randn(dout).astype(np.float32))
    p = 0.5 if act == 1 else 0.0
    keep = torch.from_numpy((rs.rand(rows, dout) >= 0.5).astype(np.float32)) if act == 1 else None
    # torch reference
    Xr, Wr, br = X.clone().requires_grad_(True), W.clone().requires_grad_(True), b.clone().requires_grad_(True)
    z = torch.nn.functional.linear(Xr, Wr, br)
    if act == 1:
        ref = torch.nn.functional.leaky_relu(z, 0.01) * keep / (1 - p)
    elif act == 2:
        ref = torch.sigmoid(z)
    else:
        ref = z
    gY = torch.from_numpy(rs.randn(rows, dout).astype(np.float32))
    ref.backward(gY)
    Xd, Wd, bd = X.cuda(), W.cuda(), b.cuda()
    Y = torch.empty(rows, dout, device="cuda")
    s = Ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    kd = keep.cuda() if keep is not None else None
    check(lib.gt_op_linear_forward(ptr(Xd), din, ptr(Wd), ptr(bd), ptr(Y), dout, rows, din, dout, act, ptr(kd), p, s))
    _close(Y.cpu().numpy(), ref.detach().numpy(), msg="Y")
    # backward of the *linear* part: feed dZ = gY * f'(out) computed on the host, check dX/dW/db
    with torch.no_grad():
        if act == 1:
            dZ = gY * torch.where(ref > 0, torch.ones_like(ref), torch.full_like(ref, 0.01)) * keep / (1 - p)
        elif act == 2:
            dZ = gY * ref * (1 - ref)
        else:
            dZ = gY
    dZd = dZ.contiguous().cuda()
    dX, dW, db = torch.empty_like(Xd), torch.empty_like(Wd), torch.empty_like(bd)
    check(lib.gt_op_linear_backward(ptr(dZd), dout, ptr(Xd), din, ptr(Wd), rows, din, dout, ptr(dX), din, None, 0, None,
                                    0.0, ptr(dW), ptr(db), s))
    torch.cuda.synchronize()
    _close(dX.cpu().numpy(), Xr.grad.numpy(), msg="dX")
    _close(dW.cpu().numpy(), Wr.grad.numpy(), msg="dW")
    _close(db.cpu().numpy(), br.grad.numpy(), msg="db")


@pytest.mark.parametrize("rows,din,dout,act", [(300, 425, 512, 1), (1000, 512, 187, 0), (77, 483, 256, 1), (16384, 512, 512, 1),
                                               (32768, 256, 256, 1), (129, 25, 25, 2), (33, 7, 3, 1), (4096, 256, 58, 0),
                                               (16384, 512, 512, 0), (16320, 640, 1152, 2), (16384, 1024, 768, -1),
                                               (32768, 512, 1024, 1), (8192, 1024, 2048, -1)])
def test_linear_bf16_storage_products_vs_float64_on_rounded_operands(rows, din, dout, act):
    """The bf16-STORAGE product family of GT_OPT_MATMUL_BF16 (gemm_bf16s.hip.h) in isolation: forward (bias + LeakyReLU +
    injected dropout / sigmoid), backward-data with the producer's f', weight gradient with split-K slabs and the bias
    gradient from the loader, 64 x 64 and 128 x 128 tiles, ragged edges, K tails that are not multiples of 8 / 64.  Operands
    are rounded to bfloat16 on the host the way the engine's images hold them; against float64 arithmetic on those rounded
    values only float32 accumulation error remains (1e-5 of the column scale).  The two bf16 result images the forward
    epilogue writes ([frame][out] and its transposed twin) must be the bf16 rounding of the float32 result, bit for bit."""
    import ctypes as Ct
    from gantts_amd._lib import check, lib, ptr
    # shapes 9 - 11 take the LDS-DMA form of the 128 x 128 tile (K a multiple of 64, >= 512 tiles) in the forward and
    # backward-data products with every epilogue (none / sigmoid / LeakyReLU + mask) and a ragged M; act = -1: no bias gradient
    # is asked for, so the weight gradient (128 x 128 tiles, whole rounds of slabs) goes through the DMA loader as well.
    # The last two fill whole rounds of CUs with 256 x 256 tiles (8-wave workgroups): forward and backward-data with the
    # LeakyReLU + mask epilogue, and (2048 x 1024 weights, no bias gradient) the weight gradient
    want_db = act >= 0
    act = max(act, 0)
    rs = np.random.RandomState(rows + 3 * din)
    bf = lambda t: t.bfloat16().double()
    X = torch.from_numpy(rs.randn(rows, din).astype(np.float32))
    W = torch.from_numpy((rs.randn(dout, din) / np.sqrt(din)).astype(np.float32))
    b = torch.from_numpy(rs.randn(dout).astype(np.float32))
    p = 0.5 if act == 1 else 0.0
    keep = torch.from_numpy((rs.rand(rows, dout) >= 0.5).astype(np.float32)) if act == 1 else None
    z = bf(X) @ bf(W).t() + b.double()
    if act == 1:
        ref = torch.nn.functional.leaky_relu(z, 0.01) * keep.double() / (1 - p)
    elif act == 2:
        ref = torch.sigmoid(z)
    else:
        ref = z
    dY = torch.from_numpy(rs.randn(rows, dout).astype(np.float32))
    Hp = torch.from_numpy(rs.randn(rows, din).astype(np.float32))               # stored activation of a producing layer
    keep_p = torch.from_numpy((rs.rand(rows, din) >= 0.5).astype(np.float32))
    Hp = Hp * keep_p
    fprime = torch.where(bf(Hp) > 0, 1.0, 0.01) * keep_p.double() * 2.0
    ref_dX = (bf(dY) @ bf(W)) * fprime
    ref_dW = bf(dY).t() @ bf(X)
    ref_db = bf(dY).sum(0)
    s = Ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    c = lambda t: None if t is None else t.cuda()
    Xd, Wd, bd, kd, dYd, Hd, kpd = c(X), c(W), c(b), c(keep), c(dY), c(Hp), c(keep_p)
    Y = torch.empty(rows, dout, device="cuda")
    Yi, YTi = torch.empty(rows, dout, device="cuda"), torch.empty(dout, rows, device="cuda")
    dX, dW, db = torch.empty(rows, din, device="cuda"), torch.empty(dout, din, device="cuda"), torch.empty(dout, device="cuda")
    check(lib.gt_op_linear_bf16(ptr(Xd), ptr(Wd), ptr(bd), rows, din, dout, act, ptr(kd), p, ptr(Y), ptr(dYd), ptr(Hd), 1, ptr(kpd), 0.5,
                                ptr(dX), ptr(dW), ptr(db) if want_db else None, ptr(Yi), ptr(YTi), s))
    torch.cuda.synchronize()
    _close(Y.cpu().numpy(), ref.numpy(), rtol=1e-5, msg="bf16-storage Y")
    assert torch.equal(Yi.cpu(), Y.cpu().bfloat16().float()), "bf16 result image != bf16(float32 result)"
    assert torch.equal(YTi.cpu(), Yi.cpu().t()), "transposed bf16 image differs from the row-major one"
    _close(dX.cpu().numpy(), ref_dX.numpy(), rtol=1e-5, msg="bf16-storage dX")
    _close(dW.cpu().numpy(), ref_dW.numpy(), rtol=2e-5, msg="bf16-storage dW")
    if want_db:
        _close(db.cpu().numpy(), ref_db.numpy(), rtol=2e-5, msg="bf16-storage db")


def test_linear_backward_fused_activation_derivative():
    """dX epilogue multiplies by f'(H_prev) of the producing layer (LeakyReLU + dropout keep mask)."""
    import ctypes as Ct
    from gantts_amd._lib import check, lib, ptr
    rs = np.random.RandomState(5)
    rows, din, dout = 200, 96, 40
    H = rs.randn(rows, din).astype(np.float32)
    keep = (rs.rand(rows, din) >= 0.5).astype(np.float32)
    H = np.where(keep > 0, H, 0).astype(np.float32)
    W = (rs.randn(dout, din) / 10).astype(np.float32)
    dZ = rs.randn(rows, dout).astype(np.float32)
    ref = (dZ.astype(np.float64) @ W.astype(np.float64)) * np.where(H > 0, 1.0, 0.01) * keep * 2.0
    s = Ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    t = lambda a: torch.from_numpy(a).cuda()
    dX = torch.empty(rows, din, device="cuda")
    Hd, Wd, dZd, kd = t(H), t(W), t(dZ), t(keep)
    check(lib.gt_op_linear_backward(ptr(dZd), dout, None, 0, ptr(Wd), rows, din, dout, ptr(dX), din, ptr(Hd), 1, ptr(kd),
                                    0.5, None, None, s))
    torch.cuda.synchronize()
    _close(dX.cpu().numpy(), ref, msg="dX fused")


@pytest.mark.parametrize("tile_frames", [16, 32])
@pytest.mark.parametrize("B,T", [(1, 1), (2, 2), (3, 7), (2, 100), (4, 513)])
def test_multi_stream_mlpg_forward_backward_vs_dense(B, T, tile_frames):
    """Banded MLPG (both tile heights of the kernels: 16 and 32 output frames per workgroup) against the dense R of the oracle."""
    from gantts_amd import _lib as L
    L.check(L.lib.gt_set_tuning(b"mlpg_tt", tile_frames))
    try:
        _mlpg_vs_dense(B, T)
    finally:
        L.check(L.lib.gt_set_tuning(b"mlpg_tt", 0))


def _mlpg_vs_dense(B, T):
    from gantts_amd import paramgen
    from gantts_amd.engine import engine_for
    from gantts_amd.multistream import _HP, multi_stream_mlpg
    ss, hd = [180, 3, 1, 3], [True, True, False, True]
    R_np = paramgen.unit_variance_mlpg_matrix(C.WINDOWS, T)
    R = torch.from_numpy(np.array(R_np)).cuda()
    rs = np.random.RandomState(T)
    y = torch.from_numpy(rs.randn(B, T, 187).astype(np.float32))
    yr = y.clone().requires_grad_(True)
    ref = O.multi_stream_mlpg(yr, torch.from_numpy(np.array(R_np)), ss, hd)
    got = multi_stream_mlpg(y.cuda(), R, ss, hd)
    _close(got.cpu().numpy(), ref.detach().numpy(), msg="mlpg fwd")
    assert torch.equal(got[:, :, 61].cpu(), y[:, :, 183])          # vuv pass-through bit-exact
    g = torch.from_numpy(rs.randn(B, T, 63).astype(np.float32))
    ref.backward(g)
    eng = engine_for(_HP(ss, hd, 3))
    gy = eng.mlpg_backward(g.cuda(), R, 187)
    _close(gy.cpu().numpy(), yr.grad.numpy(), msg="mlpg bwd")
    with pytest.raises(RuntimeError):
        multi_stream_mlpg(y[:, :, :100].cuda(), R, ss, hd)


def test_stream_gathers_are_bit_exact():
    # mirrors reference tests/test_gantts.py:60-129
    from gantts_amd.multistream import get_static_features, get_static_stream_sizes, select_streams
    ss = [60, 1, 1, 1]
    x = torch.arange(0, 63).float().expand(32, 100, 63).contiguous().cuda()
    assert select_streams(x, ss, [True, True, True, True]).shape == (32, 100, 63)
    assert select_streams(x, ss, [True, False, False, False]).shape == (32, 100, 60)
    assert select_streams(x, ss, [True, False, False, True]).shape == (32, 100, 61)
    assert (select_streams(x, ss, [False, False, False, True]).squeeze(-1) == x[:, :, -1]).all()
    assert (select_streams(x, ss, [False, False, True, False]).squeeze(-1) == x[:, :, -2]).all()
    assert (select_streams(x, ss, [False, True, False, False]).squeeze(-1) == x[:, :, -3]).all()
    y = select_streams(x, ss, [True, False, False, True])
    assert (y[:, :, :60] == x[:, :, :60]).all() and (y[:, :, -1] == x[:, :, -1]).all()
    assert np.all(get_static_stream_sizes([180, 3, 1, 3], [True, True, False, True], 3) == [60, 1, 1, 1])
    z = torch.rand(8, 50, 187).cuda()
    sf = get_static_features(z, 3, [180, 3, 1, 3], [True, True, False, True])
    assert sf.shape == (8, 50, 63)
    ref = O.get_static_features(z.cpu(), 3, [180, 3, 1, 3], [True, True, False, True])
    assert torch.equal(sf.cpu(), ref)
    assert get_static_features(z, 3, [180, 3, 1, 3], [True, True, False, True],
                               streams=[True, False, False, True]).shape == (8, 50, 61)


def test_sequence_mask_and_masked_mse():
    from gantts_amd.seqloss import MaskedMSELoss, sequence_mask
    lengths = torch.tensor([7, 5, 1, 0, 7])
    m = sequence_mask(lengths.cuda())
    assert torch.equal(m.cpu(), O.sequence_mask(lengths, 7))
    a, b = torch.randn(5, 7, 11), torch.randn(5, 7, 11)
    crit = MaskedMSELoss(compute_grad=True)
    loss = crit(a.cuda(), b.cuda(), lengths=lengths.cuda())
    ar = a.clone().requires_grad_(True)
    ref = O.masked_mse(ar, b, O.sequence_mask(lengths, 7).unsqueeze(-1))
    ref.backward()
    assert float(loss) == pytest.approx(float(ref), rel=1e-5)
    _close(crit.grad_input.cpu().numpy(), ar.grad.numpy(), msg="mse grad")
    with pytest.raises(RuntimeError):
        MaskedMSELoss()(a.cuda(), b.cuda())


def test_model_forward_eval_matches_oracle_and_errors():
    from gantts_amd import models
    spec = dict(kind="MLP", in_dim=425, out_dim=187, num_hidden=3, hidden_dim=512, dropout=0.5, last_sigmoid=False)
    m = models.MLP(**{k: v for k, v in spec.items() if k != "kind"})
    sd = C.make_weights(spec, 7)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    with pytest.raises(RuntimeError):
        m(torch.rand(2, 5, 425))          # CPU tensors: fail loudly, no fallback
    m = m.cuda().eval()
    o = O.OracleMLP(**{k: v for k, v in spec.items() if k != "kind"})
    o.load_state_dict(sd)
    o.training = False
    x = torch.rand(3, 41, 425)
    _close(m(x.cuda()).cpu().numpy(), o(x).detach().numpy(), msg="MLP eval forward")
    assert list(m.state_dict().keys()) == o.names


@pytest.mark.parametrize("pitch_x", [False, True])
def test_device_side_collate_equals_host_collate(pitch_x):
    """SURVEY 8(f)2 / VERDICT r3 missing #7: padding (train.py:139-159) and the length sort (train.py:494-501) on the device.
    A collate_ragged batch (un-padded utterances back to back) through DevicePrefetcher -> gt_op_pad_sequences must be the
    bit-identical (B, T, D) batch, in the same order, that the reference-shaped host collate + sort + trim produces."""
    from gantts_amd import data as D
    rs = np.random.RandomState(9)
    lens = [37, 120, 5, 120, 64, 1, 99]
    batch = [(rs.rand(n, 425).astype(np.float32), rs.randn(n, 187).astype(np.float32)) for n in lens]
    host = list(D.DevicePrefetcher([D.collate_fn(batch)], pitch_x=pitch_x))[0]
    dev = list(D.DevicePrefetcher([D.collate_ragged(batch)], pitch_x=pitch_x))[0]
    torch.cuda.synchronize()
    assert host.cpu_lengths == dev.cpu_lengths == sorted(lens, reverse=True)
    assert torch.equal(host.lengths.cpu(), dev.lengths.cpu())
    assert dev.x.shape == host.x.shape == (7, 120, 425) and dev.y.shape == (7, 120, 187)
    assert torch.equal(host.x.contiguous(), dev.x.contiguous()) and torch.equal(host.y, dev.y)
    if pitch_x:
        assert dev.x.stride(1) == 428 and not dev.x.is_contiguous()


@pytest.mark.parametrize("name", ["acoustic_mlp", "acoustic_mlp_dropout", "acoustic_chain_d"])
def test_pitched_x_is_bit_identical_to_dense_x(name):
    """gt_set_x_pitch (include/gantts_hip.h): x handed over with rows on a 16-byte pitch -- what DevicePrefetcher(pitch_x=True)
    stages -- must give the very same step as dense rows: the forward products read the same values in the same order, and
    the weight gradients read the caller's rows instead of the engine's own pitched copy of them."""
    from hip_runner import run_hip_case
    case = C.CASES[name]
    dense, pitched = run_hip_case(case), run_hip_case(case, pitch_x=True)
    assert set(dense) == set(pitched)
    for k in dense:
        assert np.array_equal(dense[k], pitched[k]), k


@pytest.mark.parametrize("name,options", [("acoustic_lstm_d", None), ("acoustic_lstm", None), ("vc_in2out", None), ("acoustic_grurnn_uni", None),
                                          ("acoustic_chain_d", {"split_first_layer": 0}), ("acoustic_mlp_dropout", {"matmul_bf16": 1})])
def test_pitched_x_is_accepted_by_every_network(name, options):
    """a batch staged by DevicePrefetcher(pitch_x=True) -- what train_loop hands over by default -- must be a valid
    input for EVERY network, not only for the float32 MLP pair whose kernels read pitched rows in place: a recurrent generator or
    discriminator (LSTMRNN in the discriminator slot), In2OutHighwayNet, a discriminator with the split first layer switched off,
    bf16 storage.  The engine makes the dense copy those paths read (eng_step.hip: dense_gx / dense_cx); results are bit-identical
    to handing over dense rows."""
    from hip_runner import run_hip_case
    case = C.CASES[name]
    dense, pitched = run_hip_case(case, engine_options=options), run_hip_case(case, engine_options=options, pitch_x=True)
    assert set(dense) == set(pitched)
    for k in dense:
        assert np.array_equal(dense[k], pitched[k]), k


@pytest.mark.parametrize("name", ["acoustic_mlp", "acoustic_mlp_dropout", "acoustic_chain_d", "acoustic_lstm"])
def test_split_first_layer_matches_the_concatenated_image(name):
    """GT_OPT_SPLIT_FIRST_LAYER (x . W_x^T once per D step + adv . W_adv^T, weight gradient with the two halves summed in the
    loader) against the concatenated [x | adv] image: the reference golden holds for BOTH settings
    (test_step_matches_reference_golden runs the defaults); here the two settings are compared with each other at the same 1e-4,
    counts exactly."""
    from hip_runner import run_hip_case
    case = C.CASES[name]
    on = run_hip_case(case, engine_options={"split_first_layer": 1})
    off = run_hip_case(case, engine_options={"split_first_layer": 0})
    for k in off:
        if "scalars" in k:
            _close(on[k], off[k], msg=k)
            if k.startswith("d_scalars"):
                assert on[k][3] == off[k][3] and on[k][4] == off[k][4], k
        elif ".opt." in k:
            _close_state(on[k], off[k], k)
        else:
            _close(on[k], off[k], msg=k)


@pytest.mark.parametrize("name,philox", [("acoustic_chain_d", False), ("acoustic_chain_d", True), ("acoustic_chain_d_uncond", False),
                                         ("acoustic_sru_at_size", False), ("acoustic_lstm_at_size", False)])
def test_fused_discriminator_stack_matches_the_per_layer_launches(name, philox):
    """GT_OPT_FUSED_DSTACK (dstack_f32.hip.h): the MLP discriminator's layers above the first one + head (+ the generator step's
    backward-data chain down to the adversarial columns) as ONE launch per pass, against one launch per layer + d_head_kernel.
    The reference goldens hold for the default (fused) setting (test_step_matches_reference_golden, the at-size fixtures); here the
    two settings are compared with each other at 1e-4, counts exactly: injected masks (3 x 128 conditioned, ragged last panel of
    10 rows), the engine's own Philox bits (the same bits must be drawn whatever the tiling), no dropout (2 x 128 unconditioned),
    3 x 256 behind recurrent generators."""
    from hip_runner import run_hip_case
    case = (C.CASES if name in C.CASES else C.ORACLE_ONLY_CASES)[name]
    on = run_hip_case(case, engine_options={"fused_dstack": 2}, philox=philox)
    off = run_hip_case(case, engine_options={"fused_dstack": 0}, philox=philox)
    assert set(on) == set(off)
    frac_ok, worst_ok = _kink_frac(case)      # the two settings sum the pre-activations in different orders: LeakyReLU flips at these sizes
    for k in off:
        if "scalars" in k:
            _close(on[k], off[k], msg=k)
            if k.startswith("d_scalars"):
                assert on[k][3] == off[k][3] and on[k][4] == off[k][4], k
        elif ".opt." in k and frac_ok > 0.0:
            sq = ".opt.sum." in k or ".opt.exp_avg_sq." in k
            _close_kink(np.sqrt(np.maximum(on[k], 0.0)) if sq else on[k], np.sqrt(np.maximum(off[k], 0.0)) if sq else off[k], k, frac_ok, worst_ok, atol=1e-9)
        elif ".opt." in k:
            _close_state(on[k], off[k], k)
        elif k.startswith(("G.", "D.")):
            _close_kink(on[k], off[k], k, frac_ok, worst_ok)
        else:
            _close(on[k], off[k], msg=k)


@pytest.mark.parametrize("num_hidden,hidden_dim,cond", [(1, 128, True), (1, 256, False), (2, 256, True), (4, 128, True)])
def test_fused_discriminator_stack_depths_and_widths_vs_oracle(num_hidden, hidden_dim, cond):
    """Shapes of the fused discriminator stack no fixture has: ONE hidden layer (no product inside the kernel: head on the first layer's
    output, seed, the adversarial-column product alone), the maximum of four, 256-wide with and without conditioning (col0 = 0),
    injected masks, 69-row passes (ragged last panel) -- two G+D steps against the CPU oracle, fused launches forced."""
    from hip_runner import run_hip_case
    from oracle_runner import run_oracle_case
    base = C.CASES["acoustic_chain_d"]
    din = base["din"]
    d = dict(base["d"], num_hidden=num_hidden, hidden_dim=hidden_dim, in_dim=58 + (din if cond else 0))
    case = dict(base, d=d, cond=cond, steps=2)
    got, ref = run_hip_case(case, engine_options={"fused_dstack": 2}), run_oracle_case(case)
    for k, r in ref.items():
        if k.startswith("g_leak_norm"):
            continue
        if "scalars" in k:
            _close(got[k], r, msg=k)
            if k.startswith("d_scalars"):
                assert got[k][3] == r[3] and got[k][4] == r[4], k
        elif ".opt." in k:
            _close_state(got[k], r, k)
        else:
            _close(got[k], r, msg=k)


def test_fused_discriminator_stack_eval_phase_reports_the_same_losses():
    """phase != "train" (the "test" phase of train_loop, train.py:528-585: losses and counts, no gradients, no update, eval-mode
    networks: no dropout): the fused stack runs with want_grad = 0 and must report the scalars the per-layer launches report; nothing
    may be written to the parameters."""
    import gantts_amd.train as T
    from gantts_amd import optim, paramgen
    from gantts_amd.engine import engine_for
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model, make_hp
    case = C.CASES["acoustic_chain_d"]
    hp = make_hp(case)
    x_np, y_np, lengths = C.make_batch(case)
    res = {}
    for fused in (2, 0):
        T.hp = hp
        mg, md = build_model(case["g"], 11).eval(), build_model(case["d"], 22).eval()
        og = optim.Adagrad(mg.parameters(), **case["opt_g"][1])
        od = optim.Adagrad(md.parameters(), **case["opt_d"][1])
        engine_for(hp, mg).set_option("fused_dstack", fused)
        x, y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
        R = paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, case["T"])
        ys = get_static_features(y, len(hp.windows), hp.stream_sizes, hp.has_dynamic_features)
        mask = sequence_mask(torch.from_numpy(np.ascontiguousarray(lengths)).cuda(), max_len=case["T"]).unsqueeze(-1)
        w0 = md.flat_params().clone()
        yh, yhs = T.apply_generator(mg, x, R, list(lengths))
        d = T.update_discriminator(md, od, x, ys, yhs, list(lengths), mask, "test")
        g = T.update_generator(mg, md, og, x, y, yh, ys, yhs, 1.0, list(lengths), mask, "test", mse_w=0.0, mge_w=1.0)
        assert torch.equal(w0, md.flat_params())
        res[fused] = (np.array(d, dtype=np.float64), np.array(g, dtype=np.float64))
    _close(res[2][0], res[0][0], msg="eval D scalars")
    assert res[2][0][3] == res[0][0][3] and res[2][0][4] == res[0][0][4]
    _close(res[2][1], res[0][1], msg="eval G scalars")


@pytest.mark.parametrize("name", ["acoustic_mlp_dropout", "acoustic_chain_d", "acoustic_lstm", "duration_mlp", "vc_in2out"])
def test_launch_riders_match_the_separate_launches(name):
    """GT_OPT_LAUNCH_RIDERS: the valid-frame count as an extra workgroup of the adversarial-column gather, the generator step's two
    sums of squares in one launch, the head's scalar reduction and the step's finalisation as an extra workgroup of the
    gradient-assembly launch.  No gradient depends on where those sums are formed: parameters and optimizer state must be
    BIT-IDENTICAL to the separate launches, the reported scalars equal to double-precision summation order (counts exactly)."""
    from hip_runner import run_hip_case
    case = C.CASES[name]
    on = run_hip_case(case, engine_options={"launch_riders": 1})
    off = run_hip_case(case, engine_options={"launch_riders": 0})
    assert set(on) == set(off)
    for k in off:
        if "scalars" in k:
            _close(on[k], off[k], rtol=1e-6, atol=1e-9, msg=k)
            if k.startswith("d_scalars"):
                assert on[k][3] == off[k][3] and on[k][4] == off[k][4], k
        else:
            assert np.array_equal(on[k], off[k]), k


@pytest.mark.parametrize("name", ["acoustic_mlp_dropout", "acoustic_chain_d"])
def test_head_16_byte_accesses_match_the_4_byte_form(name):
    """The discriminator head with lane <-> four consecutive hidden units (16-byte loads of the row, 16-byte stores of the seed
    gradient; gt_set_tuning("head_vec")) against lane <-> every 64th unit: the same products, the row's dot product summed in a
    different order -- a whole run agrees at 1e-4 (counts exactly), with the engine's own Philox dropout (bits keyed by unit index)."""
    from gantts_amd import _lib as L
    from hip_runner import run_hip_case
    case = C.CASES[name]
    scalar = run_hip_case(case, philox=True)
    try:
        L.check(L.lib.gt_set_tuning(b"head_vec", 1))
        vec = run_hip_case(case, philox=True)
    finally:
        L.check(L.lib.gt_set_tuning(b"head_vec", 0))
    for k in scalar:
        if "scalars" in k:
            _close(vec[k], scalar[k], msg=k)
            if k.startswith("d_scalars"):
                assert vec[k][3] == scalar[k][3] and vec[k][4] == scalar[k][4], k
        elif ".opt." in k:
            _close_state(vec[k], scalar[k], k)
        else:
            _close(vec[k], scalar[k], msg=k)


def test_split_first_layer_one_launch_equals_two_launches():
    """The split first layer's forward as ONE two-segment launch with two result halves (GEMM_A_LEAKY_PHILOX_SEG: the production
    path with Philox dropout) against its two-launch form (x product, then the K = 58 pass that adds it: GEMM_A_LEAKY_PHILOX_ADDM):
    same Philox bits (keyed by site and row, not by launch), same sums up to float32 association -- a whole two-step run with the
    engine's own dropout must agree at 1e-4, counts exactly."""
    from gantts_amd import _lib as L
    from hip_runner import run_hip_case
    case = dict(C.CASES["acoustic_mlp_dropout"], B=4, T=80)       # 320 rows: five 64-row tiles per half
    try:
        L.check(L.lib.gt_set_tuning(b"split_fused", 0))
        two = run_hip_case(case, philox=True)
    finally:
        L.check(L.lib.gt_set_tuning(b"split_fused", 1))
    one = run_hip_case(case, philox=True)
    for k in two:
        if "scalars" in k:
            _close(one[k], two[k], msg=k)
            if k.startswith("d_scalars"):
                assert one[k][3] == two[k][3] and one[k][4] == two[k][4], k
        elif ".opt." in k:
            _close_state(one[k], two[k], k)
        else:
            _close(one[k], two[k], msg=k)
    assert not np.array_equal(one["D.layers.0.weight"], C.make_weights(case["d"], 22)["layers.0.weight"])     # (the steps did run)


def test_philox_dropout_statistics_and_determinism():
    from gantts_amd import models
    m = models.MLP(in_dim=16, out_dim=8, num_hidden=1, hidden_dim=2048, dropout=0.5, last_sigmoid=False).cuda().train()
    with torch.no_grad():
        for p in m.parameters():
            p.zero_()
        m.layers[0].bias.fill_(1.0)
        m.last_linear.weight.fill_(1.0 / 2048)
    x = torch.zeros(4, 64, 16, device="cuda")
    out = m(x)                 # each output = mean over hidden of keep*2  -> ~1.0
    assert abs(float(out.mean()) - 1.0) < 0.02
    assert float(out.std()) > 1e-4          # masks differ between frames
    out2 = m(x)
    assert not torch.equal(out, out2)       # fresh mask per call


def test_checkpoint_roundtrip_and_torch_compat(tmp_path):
    import gantts_amd.train as T
    from gantts_amd import models, optim
    m = models.MLP(in_dim=12, out_dim=5, num_hidden=2, hidden_dim=16, last_sigmoid=False).cuda()
    opt = optim.Adagrad(m.parameters(), lr=0.01, weight_decay=1e-7)
    path = T.save_checkpoint(m, opt, 10, str(tmp_path), "Generator")
    ck = torch.load(path, map_location="cpu")
    # loadable by a plain torch module with the reference's layout
    ref = torch.nn.ModuleDict({"layers": torch.nn.ModuleList([torch.nn.Linear(12, 16), torch.nn.Linear(16, 16)]),
                               "last_linear": torch.nn.Linear(16, 5)})
    ref.load_state_dict(ck["state_dict"])
    topt = torch.optim.Adagrad(ref.parameters(), lr=0.01, weight_decay=1e-7)
    topt.load_state_dict(ck["optimizer"])
    m2 = models.MLP(in_dim=12, out_dim=5, num_hidden=2, hidden_dim=16, last_sigmoid=False).cuda()
    opt2 = optim.Adagrad(m2.parameters())
    assert T.load_checkpoint(m2, opt2, path) == 10
    for a, b in zip(m.parameters(), m2.parameters()):
        assert torch.equal(a, b)
    assert opt2.param_groups[0]["weight_decay"] == 1e-7


def _dp_objects(case, rows):
    """(backend, batch) of one emulated rank holding sequences `rows` of the case's batch."""
    from gantts_amd import optim, paramgen
    from gantts_amd.engine import HipStepBackend
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model, make_hp
    hp = make_hp(case)
    mg, md = build_model(case["g"], 11).eval(), build_model(case["d"], 22).eval()
    og = getattr(optim, case["opt_g"][0])(mg.parameters(), **case["opt_g"][1])
    od = getattr(optim, case["opt_d"][0])(md.parameters(), **case["opt_d"][1])
    x_np, y_np, lengths = C.make_batch(case)
    x, y = torch.from_numpy(x_np[rows]).cuda(), torch.from_numpy(y_np[rows]).cuda()
    lens = torch.from_numpy(lengths[rows]).cuda()
    batch = dict(x=x, y=y, R=paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, case["T"]),
                 y_static=get_static_features(y, len(hp.windows), hp.stream_sizes, hp.has_dynamic_features),
                 mask=sequence_mask(lens, case["T"]).unsqueeze(-1))
    return HipStepBackend(hp, mg, md, og, od), batch


def test_data_parallel_shards_equal_whole_batch_on_one_gpu():
    """Two emulated ranks (B/2 sequences each, own engine + replicas) with the all-reduce done by
    hand == the plain single-engine step on the whole batch: the split-phase C ABI keeps additive
    sums, normalises by the GLOBAL valid-frame count and leaves identical replicas."""
    from gantts_amd.parallel import DataParallelStep
    from hip_runner import run_hip_case
    case = C.CASES["acoustic_mlp"]
    whole = run_hip_case(case)
    ranks = [_dp_objects(case, np.arange(case["B"])[r::2]) for r in range(2)]
    tv = float(sum(b["mask"].sum().item() for _, b in ranks))
    hist = []
    for step in range(case["steps"]):
        for be, b in ranks:
            be.set_loss_normalizer(tv)
            be.zero_grad()
            be.apply_generator(b)
            be.update_discriminator_begin(b, "train")
        for which, phase_end in (("D", "update_discriminator_end"),):
            g = sum(be.flat_grads(which) for be, _ in ranks)
            s = sum(be.scalar_sums(which) for be, _ in ranks)
            for be, _ in ranks:
                be.flat_grads(which).copy_(g)
                be.scalar_sums(which).copy_(s)
        d = [be.update_discriminator_end(b, "train") for be, b in ranks]
        for be, b in ranks:
            be.update_generator_begin(b, case["adv_w"], case["mse_w"], case["mge_w"], "train")
        g = sum(be.flat_grads("G") for be, _ in ranks)
        s = sum(be.scalar_sums("G") for be, _ in ranks)
        for be, _ in ranks:
            be.flat_grads("G").copy_(g)
            be.scalar_sums("G").copy_(s)
        gr = [be.update_generator_end(b, case["adv_w"], case["mse_w"], case["mge_w"], "train") for be, b in ranks]
        assert d[0] == d[1] and gr[0] == gr[1]
        hist.append((d[0], gr[0]))
    for i, (d, g) in enumerate(hist):
        _close(d, whole["d_scalars_%d" % i], msg="dp d step %d" % i)
        _close(g, whole["g_scalars_%d" % i], msg="dp g step %d" % i)
    for tag, idx in (("G", 0), ("D", 1)):
        m0 = (ranks[0][0].mg, ranks[0][0].md)[idx]
        m1 = (ranks[1][0].mg, ranks[1][0].md)[idx]
        for (k, v0), v1 in zip(m0.state_dict().items(), m1.state_dict().values()):
            assert torch.equal(v0, v1), k                       # replicas bit-identical
            _close(v0.cpu().numpy(), whole["%s.%s" % (tag, k)], msg=k)
    # world = 1 through the DP orchestrator == the plain path as well
    be, b = _dp_objects(case, np.arange(case["B"]))
    dp = DataParallelStep(be)
    for i in range(case["steps"]):
        d, g = dp.step(b, adv_w=case["adv_w"], mse_w=case["mse_w"], mge_w=case["mge_w"])
        _close(d, whole["d_scalars_%d" % i], msg="dp1 d")
        _close(g, whole["g_scalars_%d" % i], msg="dp1 g")


def test_full_size_cfg2_step_vs_oracle_and_determinism():
    """BASELINE.json configs[1] at full size (B=32, T=512, 425->187, fp32), dropout off: one G+D step
    against the CPU oracle, plus run-to-run bit-reproducibility of the HIP path."""
    import gantts_amd.train as T
    from gantts_amd import hparams, optim, paramgen
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model
    import types
    B, Tn = 32, 512
    gs = dict(kind="MLP", in_dim=425, out_dim=187, num_hidden=3, hidden_dim=512, dropout=0.5, last_sigmoid=False)
    ds = dict(kind="MLP", in_dim=483, out_dim=1, num_hidden=3, hidden_dim=256, dropout=0.5, last_sigmoid=True)
    case = dict(B=B, T=Tn, din=425, dout=187, stream_sizes=[180, 3, 1, 3])
    x_np, y_np, lengths = C.make_batch(case, seed=7)
    hp = types.SimpleNamespace(**hparams.tts_acoustic.values())
    T.hp = hp
    R_np = np.array(paramgen.unit_variance_mlpg_matrix(hp.windows, Tn))

    def hip_once():
        mg, md = build_model(gs, 1).eval(), build_model(ds, 2).eval()
        og, od = optim.Adagrad(mg.parameters(), lr=0.01, weight_decay=1e-7), optim.Adagrad(md.parameters(), lr=0.01, weight_decay=1e-7)
        x, y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
        R = torch.from_numpy(R_np).cuda()
        ys = get_static_features(y, 3, hp.stream_sizes, hp.has_dynamic_features)
        mask = sequence_mask(torch.from_numpy(lengths).cuda()).unsqueeze(-1)
        og.zero_grad(), od.zero_grad()
        yh, yhs = T.apply_generator(mg, x, R, list(lengths))
        d = T.update_discriminator(md, od, x, ys, yhs, list(lengths), mask, "train")
        d_grads = md.flat_grads().cpu().clone()   # D.grad as left by the D step (the G step's additions to it
        # are discarded by the next zero_grad in the reference, train.py:538-539, and are not computed here)
        g = T.update_generator(mg, md, og, x, y, yh, ys, yhs, 1.0, list(lengths), mask, "train", mse_w=0.0, mge_w=1.0)
        return (d, g, yhs.cpu(), mg.flat_params().cpu().clone(), md.flat_params().cpu().clone(),
                mg.flat_grads().cpu().clone(), d_grads)

    a, b = hip_once(), hip_once()
    assert a[0] == b[0] and a[1] == b[1]
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])   # bit-reproducible

    mg = O.OracleMLP(**{k: v for k, v in gs.items() if k != "kind"})
    md = O.OracleMLP(**{k: v for k, v in ds.items() if k != "kind"})
    mg.load_state_dict(C.make_weights(gs, 1)), md.load_state_dict(C.make_weights(ds, 2))
    mg.training = md.training = False
    og, od = O.OracleAdagrad(mg.params, lr=0.01, weight_decay=1e-7), O.OracleAdagrad(md.params, lr=0.01, weight_decay=1e-7)
    cfg = O.StreamConfig([180, 3, 1, 3], [True, True, False, True], 3, [True, False, False, False], 2, True)
    x, y = torch.from_numpy(x_np), torch.from_numpy(y_np)
    omask = O.sequence_mask(lengths, Tn).unsqueeze(-1)
    oys = O.get_static_features(y, 3, cfg.stream_sizes, cfg.has_dynamic_features)
    oyh, oyhs = O.apply_generator(cfg, mg, x, torch.from_numpy(R_np), list(lengths))
    out = {"y_hat_static": oyhs.detach()}
    out["d"] = O.update_discriminator(cfg, md, od, x, oys, oyhs, list(lengths), omask, "train")
    ref_d_grads = torch.cat([p.grad.reshape(-1) for p in md.params]).numpy().copy()
    out["g"] = O.update_generator(cfg, mg, md, og, x, y, oyh, oys, oyhs, 1.0, list(lengths), omask, "train",
                                  mse_w=0.0, mge_w=1.0)
    _close(a[0], out["d"], msg="full-size D scalars")
    assert a[0][3] == out["d"][3] and a[0][4] == out["d"][4]
    _close(a[1], out["g"], msg="full-size G scalars")
    _close(a[2].numpy(), out["y_hat_static"].numpy(), msg="full-size y_hat_static")
    # gradients (clipped in place by clip_grad_norm_, like torch) agree to 1e-4 of their scale
    _close(a[5].numpy(), torch.cat([p.grad.reshape(-1) for p in mg.params]).numpy(), rtol=2e-4, atol=1e-9, msg="G grads")
    _close(a[6].numpy(), ref_d_grads, rtol=2e-4, atol=1e-9, msg="D grads")
    # parameters after the step: the FIRST Adagrad step is lr*sign(g) (sum == g^2), i.e. discontinuous
    # at g == 0, so the handful of entries whose gradient cancels to rounding noise may land 2*lr
    # apart; everything else must agree tightly.
    for got, params in ((a[3].numpy(), mg.params), (a[4].numpy(), md.params)):
        ref = torch.cat([p.detach().reshape(-1) for p in params]).numpy()
        gref = torch.cat([p.grad.reshape(-1) for p in params]).numpy()
        bad = np.abs(got - ref) > 1e-5
        assert bad.mean() < 1e-3, "too many mismatching parameters: %g" % bad.mean()
        if bad.any():
            assert np.abs(gref[bad]).max() < 1e-3 * np.abs(gref).max(), "mismatch on a well-conditioned gradient"


def _rms(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.sqrt((a * a).mean())) if a.size else 0.0


ARBITER_FACTOR, ARBITER_FLOOR = 3.0, 2e-6


def _close_arbiter(got, ref32, ref64, msg, factor=ARBITER_FACTOR, floor=ARBITER_FLOOR, kink=0.0):
    """The float64 arbiter (same rule as tests/golden/at_size.py): the oracle is run twice on identical inputs and masks,
    in float32 (the reference's arithmetic) and in float64 (exact to 1e-16); per tensor the engine must be no further from
    the exact result than `factor` x the reference's own float32 arithmetic is:

        rms(got - ref64) <= factor * rms(ref32 - ref64) + floor * rms(ref64)

    No hand-set per-layer tolerance: where float32 itself is ill-conditioned -- a pre-activation within rounding of 0 picks
    LeakyReLU slope 1 or 0.01 (in-place LeakyReLU, gantts/models.py:132: the derivative follows the sign of the stored output)
    and moves a rank-one piece of every lower weight gradient -- rms(ref32 - ref64) shows it, tensor by tensor, and where it is
    well-conditioned the limit is a few float32 ulps.  `kink` (for gradient tensors downstream of a LeakyReLU layer only): whether
    a given run HAS such a flip on a given tensor is a Poisson draw with a mean of order one per network, so the reference's
    single float32 run may show none where the engine shows one.  The allowance is MEASURED per case: the oracle's float32 and
    float64 runs are compared activation by activation (make_at_size.SlopeCensus) and n = flips + 3 sqrt(flips) + 5 flips -- the
    upper end of that Poisson draw -- are allowed, i.e. sqrt(n / activations) relative rms (tests/golden/at_size.py).  A wrong keep bit or tile shows at 1e-1..1.  The worst
    single element must stay within 10x the limit (relative to the tensor's largest magnitude)."""
    g, r32, r64 = (np.asarray(a, dtype=np.float64) for a in (got, ref32, ref64))
    den = max(_rms(r64), 1e-300)
    err, e32 = _rms(g - r64) / den, _rms(r32 - r64) / den
    lim = factor * e32 + floor + kink
    worst = float(np.abs(g - r64).max()) / max(float(np.abs(r64).max()), 1e-300) if g.size else 0.0
    if _REPORT:
        with open(_REPORT, "a") as f:
            f.write("%-60s rel-rms err %.3e  ref32-vs-ref64 %.3e  limit %.3e  worst element %.3e\n" % (msg, err, e32, lim, worst))
        return
    assert err <= lim and worst <= 10 * lim, "%s: relative rms distance to the float64 result %.3e > %.3e (the reference's own float32: %.3e); worst element %.3e" % (
        msg, err, lim, e32, worst)


@pytest.mark.parametrize("tag,B,Tn,gh,dh,x_layout", [("cfg2-full-size", 32, 512, 512, 256, "dense"),
                                                      ("cfg2-full-size-pitched-x", 32, 512, 512, 256, "pitched"),
                                                      ("ragged-tiles-narrow-epilogue", 3, 171, 130, 250, "dense"),
                                                      ("64-row-tiles", 4, 200, 256, 128, "dense")])
def test_philox_dropout_step_matches_oracle_with_dumped_masks(tag, B, Tn, gh, dh, x_layout):
    """The path bench.py times: dropout 0.5 ON through the engine's own Philox stream (no injected masks on the HIP
    side).  The keep masks the engine is about to use are dumped through gt_op_philox_mask -- the layout-independent
    definition philox_keep(row, col) -- and handed to the CPU oracle as its nn.Dropout masks (the oracle is pinned to
    the reference with masks injected the same way, tests/golden/make_golden.py); the whole step must then agree:
    forward epilogues AND the keep bits every backward kernel regenerates (wide 16-byte and narrow epilogues, 64 / 128
    row and column tiles, partial tiles, 2N-row discriminator pass, fused head).  Two steps, Adagrad with a warm
    accumulator (1e-4: as after some training, where the update is smooth in g).
    Forward quantities of the first step and all scalars: 1e-4 per column.  Gradients and what follows from them
    (parameters, the second step's forward): per tensor under the float64 arbiter (_close_arbiter): the oracle runs a second
    time in float64 with the same masks, and the engine may be 3x as far from that as the float32 oracle is.
    Reference semantics: gantts/models.py:132-139, train.py:245-320."""
    import types
    import gantts_amd.train as T
    from gantts_amd import _lib as L
    from gantts_amd import hparams, optim, paramgen
    from gantts_amd.engine import engine_for
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model
    N, steps, acc0, p = B * Tn, 2, 1e-4, 0.5
    gs = dict(kind="MLP", in_dim=425, out_dim=187, num_hidden=3, hidden_dim=gh, dropout=p, last_sigmoid=False)
    ds = dict(kind="MLP", in_dim=483, out_dim=1, num_hidden=3, hidden_dim=dh, dropout=p, last_sigmoid=True)
    case = dict(B=B, T=Tn, din=425, dout=187, stream_sizes=[180, 3, 1, 3])
    x_np, y_np, lengths = C.make_batch(case, seed=11)
    hp = types.SimpleNamespace(**hparams.tts_acoustic.values())
    T.hp = hp
    R_np = np.array(paramgen.unit_variance_mlpg_matrix(hp.windows, Tn))
    okw = dict(lr=0.01, weight_decay=1e-7)

    # ---- HIP: train mode, Philox dropout; dump the masks of the coming step first ----
    mg, md = build_model(gs, 1).train(), build_model(ds, 2).train()
    og = optim.Adagrad(mg.parameters(), initial_accumulator_value=acc0, **okw)
    od = optim.Adagrad(md.parameters(), initial_accumulator_value=acc0, **okw)
    eng = engine_for(hp, mg)
    eng.set_seed(1234)
    x, y, R = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda(), torch.from_numpy(R_np).cuda()
    if x_layout == "pitched":       # the layout bench.py times and train_loop stages (DevicePrefetcher(pitch_x=True); gt_set_x_pitch)
        from gantts_amd.engine import pitched_empty
        xp = pitched_empty(B, Tn, 425)
        xp.copy_(x)
        x = xp
        assert x.stride(1) == 428 and not x.is_contiguous()
    ys = get_static_features(y, 3, hp.stream_sizes, hp.has_dynamic_features)
    mask = sequence_mask(torch.from_numpy(lengths).cuda()).unsqueeze(-1)
    hip, masks = [], []
    for st in range(steps):
        gm = [eng.philox_mask(L.ROLE_G, 0, l, p, N, gh).cpu().view(B, Tn, gh) for l in range(3)]
        d0 = [eng.philox_mask(L.ROLE_D, 0, l, p, 2 * N, dh).cpu() for l in range(3)]
        d2 = [eng.philox_mask(L.ROLE_D, 2, l, p, N, dh).cpu().view(B, Tn, dh) for l in range(3)]
        masks.append((gm, [m[:N].view(B, Tn, dh) for m in d0] + [m[N:].view(B, Tn, dh) for m in d0] + d2))
        og.zero_grad(), od.zero_grad()
        yh, yhs = T.apply_generator(mg, x, R, list(lengths))
        d = T.update_discriminator(md, od, x, ys, yhs, list(lengths), mask, "train")
        dgrad = md.flat_grads().cpu().clone()
        g = T.update_generator(mg, md, og, x, y, yh, ys, yhs, 1.0, list(lengths), mask, "train", mse_w=0.0, mge_w=1.0)
        hip.append(dict(d=d, g=g, yh=yh.cpu().numpy(), yhs=yhs.cpu().numpy(), dgrad=dgrad.numpy(),
                        ggrad=mg.flat_grads().cpu().numpy().copy()))
    for gm, _ in masks:                       # the dumped masks are Bernoulli(0.5) and differ between sites / steps
        assert all(abs(float(m.mean()) - 0.5) < 0.02 for m in gm)
    assert not torch.equal(masks[0][0][0], masks[1][0][0]) and not torch.equal(masks[0][0][0], masks[0][0][1])

    # ---- oracle: the same masks injected; run twice -- as is, and with every weight moved by ~1 ulp ----
    cfg = O.StreamConfig([180, 3, 1, 3], [True, True, False, True], 3, [True, False, False, False], 2, True)
    xc32, yc32, Rc32 = torch.from_numpy(x_np), torch.from_numpy(y_np), torch.from_numpy(R_np)
    omask32 = O.sequence_mask(lengths, Tn).unsqueeze(-1)
    oys32 = O.get_static_features(yc32, 3, cfg.stream_sizes, cfg.has_dynamic_features)
    wg0, wd0 = C.make_weights(gs, 1), C.make_weights(ds, 2)

    def oracle_run(dtype):
        omg = O.OracleMLP(**{k: v for k, v in gs.items() if k != "kind"})
        omd = O.OracleMLP(**{k: v for k, v in ds.items() if k != "kind"})
        omg.load_state_dict(wg0), omd.load_state_dict(wd0)
        O.cast_model(omg, dtype), O.cast_model(omd, dtype)
        xc, yc, Rc, omask, oys = (t.to(dtype) for t in (xc32, yc32, Rc32, omask32, oys32))
        omg.training = omd.training = True
        init_g, init_d = [q.detach().numpy().copy() for q in omg.params], [q.detach().numpy().copy() for q in omd.params]
        oog, ood = O.OracleAdagrad(omg.params, initial_accumulator_value=acc0, **okw), O.OracleAdagrad(omd.params, initial_accumulator_value=acc0, **okw)
        rec = []
        for st in range(steps):
            gm, dm = ([m.to(dtype) for m in q] for q in masks[st])
            dd = O._DropoutSource(dm)
            oog.zero_grad(), ood.zero_grad()
            oyh, oyhs = O.apply_generator(cfg, omg, xc, Rc, list(lengths), drop=O._DropoutSource(gm))
            od_ = O.update_discriminator(cfg, omd, ood, xc, oys, oyhs, list(lengths), omask, "train", drop=dd)
            dgr = [q.grad.numpy().copy() for q in omd.params]
            og_ = O.update_generator(cfg, omg, omd, oog, xc, yc, oyh, oys, oyhs, 1.0, list(lengths), omask, "train",
                                     mse_w=0.0, mge_w=1.0, drop=dd)
            assert not dd.masks, "oracle consumed %d of 9 discriminator masks" % (9 - len(dd.masks))
            rec.append(dict(d=od_, g=og_, yh=oyh.detach().numpy().copy(), yhs=oyhs.detach().numpy().copy(), dgrad=dgr,
                            ggrad=[q.grad.numpy().copy() for q in omg.params]))
        return rec, [q.detach().numpy() - i for q, i in zip(omg.params, init_g)], [q.detach().numpy() - i for q, i in zip(omd.params, init_d)], omg.names, omd.names

    from make_at_size import SlopeCensus
    with SlopeCensus() as c32:
        ref, ref_gu, ref_du, gnames, dnames = oracle_run(torch.float32)     # records of both steps, total parameter updates
    with SlopeCensus() as c64:
        alt, alt_gu, alt_du, _, _ = oracle_run(torch.float64)               # the arbiter: same inputs and masks, float64
    calls = len(c32.signs) // steps

    def kink_of(first_call, last_call):      # measured allowance from the flips among calls [first, last)
        a, b = SlopeCensus(), SlopeCensus()
        a.signs, b.signs = c32.signs[first_call:last_call], c64.signs[first_call:last_call]
        cen = SlopeCensus.compare(a, b, 3, calls)
        flips, acts = cen["G"][0] + cen["D"][0], cen["G"][1] + cen["D"][1]
        return float(np.sqrt((flips + 3.0 * np.sqrt(flips) + 5.0) / acts)), cen

    # the first step's gradients see the first step's flips only; whatever follows the first update sees many more (the two
    # precisions' parameters differ after it, so every pre-activation within that difference of 0 flips)
    kink_by_step = [kink_of(0, calls)[0]] + [kink_of(0, calls * (st + 1))[0] for st in range(1, steps)]
    KINK_ALLOWANCE = kink_by_step[-1]
    if _REPORT:
        with open(_REPORT, "a") as f:
            f.write("%s: LeakyReLU slope census, all steps: %s -> kink allowance by step %s\n" % (tag, kink_of(0, calls * steps)[1], kink_by_step))

    def split(flat, like):
        out, off = [], 0
        for r in like:
            out.append(flat[off:off + r.size].reshape(r.shape))
            off += r.size
        return out

    for st in range(steps):
        h, r, a = hip[st], ref[st], alt[st]
        t = "%s step %d " % (tag, st)
        _close(h["d"], r["d"], msg=t + "D scalars")
        assert h["d"][3] == r["d"][3] and h["d"][4] == r["d"][4], (h["d"], r["d"])
        _close(h["g"], r["g"], msg=t + "G scalars")
        if st == 0:
            _close(h["yh"], r["yh"], msg=t + "y_hat")
            _close(h["yhs"], r["yhs"], msg=t + "y_hat_static")
        else:       # inherits the parameter differences of the step before
            _close_arbiter(h["yh"], r["yh"], a["yh"], t + "y_hat", kink=KINK_ALLOWANCE)
            _close_arbiter(h["yhs"], r["yhs"], a["yhs"], t + "y_hat_static", kink=KINK_ALLOWANCE)
        for nm, got, rr, aa in zip(dnames, split(h["dgrad"], r["dgrad"]), r["dgrad"], a["dgrad"]):
            _close_arbiter(got, rr, aa, t + "D.grad " + nm, kink=0.0 if nm.startswith("last_linear") and st == 0 else kink_by_step[st])
        for nm, got, rr, aa in zip(gnames, split(h["ggrad"], r["ggrad"]), r["ggrad"], a["ggrad"]):
            _close_arbiter(got, rr, aa, t + "G.grad " + nm, kink=kink_by_step[st])
    # parameters after both steps: the UPDATE each tensor received
    for tagm, m, ru, au, w0 in (("G", mg, ref_gu, alt_gu, wg0), ("D", md, ref_du, alt_du, wd0)):
        for (k, v), r_, a_ in zip(m.state_dict().items(), ru, au):
            _close_arbiter(v.cpu().numpy() - w0[k], r_, a_, "%s %s.%s update after 2 steps" % (tag, tagm, k), kink=KINK_ALLOWANCE)


@pytest.mark.parametrize("B,T,din,H,L,bi", [(5, 13, 20, 40, 2, True), (2, 30, 7, 8, 1, False), (37, 9, 12, 33, 3, True),
                                            (3, 17, 10, 300, 1, True)])
def test_lstmrnn_forward_matches_oracle_unsorted_lengths(B, T, din, H, L, bi):
    """LSTMRNN.forward(sequence, lengths) vs the oracle's masked time loop (== nn.LSTM over packed
    sequences, pinned by the golden case); lengths deliberately NOT sorted, B = 37 runs five
    8-sequence batch tiles, the last one ragged.  (16-sequence tiles, every unit count and precision: test_gpu_lstm_recurrence.py.)"""
    from gantts_amd import models
    spec = dict(kind="LSTMRNN", in_dim=din, out_dim=11, num_hidden=L, hidden_dim=H, bidirectional=bi, dropout=0.0,
                last_sigmoid=False)
    sd = C.make_weights(spec, B + T)
    m = models.LSTMRNN(**{k: v for k, v in spec.items() if k != "kind"})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda().eval()
    o = O.OracleLSTMRNN(**{k: v for k, v in spec.items() if k != "kind"})
    o.load_state_dict(sd)
    o.training = False
    rs = np.random.RandomState(B)
    x = torch.from_numpy(rs.randn(B, T, din).astype(np.float32))
    lengths = rs.randint(1, T + 1, size=B)
    lengths[rs.randint(B)] = T
    got = m(x.cuda(), list(lengths)).cpu().numpy()
    ref = o(x, list(lengths)).detach().numpy()
    _close(got, ref, msg="LSTMRNN forward")
    # frames beyond each length see zero LSTM output -> exactly the hidden2out bias
    b = int(np.argmin(lengths))
    if lengths[b] < T:
        np.testing.assert_allclose(got[b, lengths[b]:], np.broadcast_to(sd["hidden2out.bias"], got[b, lengths[b]:].shape),
                                   rtol=0, atol=1e-7)
    with pytest.raises(RuntimeError):
        m(x.cuda(), list(lengths[:-1]))


@pytest.mark.parametrize("name", sorted(C.ORACLE_ONLY_CASES))
def test_oracle_only_step_matches_oracle(name):
    """Full G+D steps against the CPU oracle where no reference-generated fixture can exist: SRURNN
    (un-vendored third-party CUDA cell -> parity unpinned) and nn.LSTM inter-layer
    dropout in training mode (masks cannot be injected into _VF.lstm; eval mode is pinned in CASES)."""
    from hip_runner import run_hip_case
    from oracle_runner import run_oracle_case
    case = C.ORACLE_ONLY_CASES[name]
    got, ref = run_hip_case(case), run_oracle_case(case)
    frac_ok, worst_ok = _kink_frac(case)      # (parameters / optimizer state of the at-size cases: see _kink_frac)
    for k, r in ref.items():
        if k.startswith("g_leak_norm"):
            continue
        if "scalars" in k:
            _close(got[k], r, msg=k)
        elif ".opt." in k:
            if frac_ok > 0.0 and (".opt.sum." in k or ".opt.exp_avg_sq." in k):
                _close_kink(np.sqrt(np.maximum(got[k], 0.0)), np.sqrt(np.maximum(r, 0.0)), k + " (sqrt)", frac_ok, worst_ok, atol=1e-9)
            elif frac_ok > 0.0:
                _close_kink(got[k], r, k, frac_ok, worst_ok, atol=1e-9)
            else:
                _close_state(got[k], r, k)
        elif k.startswith(("G.", "D.")):
            _close_kink(got[k], r, k, frac_ok, worst_ok)
        else:
            _close(got[k], r, msg=k)


def test_matmul_bf16_step_tracks_the_float32_oracle():
    """GT_OPT_MATMUL_BF16 (BASELINE.json configs[2]: bf16 products, float32 accumulation, float32 master weights and
    state) on cfg3 at its real widths (BiLSTM 3 x 256, 425 -> 187, conditioned MLP D, B = 32, T = 96): one G+D step against
    the FLOAT32 CPU oracle.  Tolerances are the measured bf16 rounding level (operands carry 8 mantissa bits: 4e-3
    relative per value, averaged down by the K ~ 256..512 long sums), an order of magnitude above the float32 path's and
    two below what a wrong operand layout produces: forward outputs and losses 2e-2 of their scale, gradients 5e-2
    relative rms per tensor."""
    from hip_runner import run_hip_case
    from oracle_runner import run_oracle_case
    case = dict(C.ORACLE_ONLY_CASES["acoustic_lstm_at_size"])
    case["steps"] = 1
    got, objs = run_hip_case(case, return_objects=True, engine_options={"matmul_bf16": 1})
    ref = run_oracle_case(case)
    for k in ("y_hat", "y_hat_static"):
        err = _rms(got[k] - ref[k]) / _rms(ref[k])
        if _REPORT:
            open(_REPORT, "a").write("bf16 %-20s rel-rms %.3e\n" % (k, err))
        assert err < 2e-2, (k, err)
    for k in ("d_scalars_0", "g_scalars_0"):
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        rel = np.abs(a - b) / np.maximum(np.abs(b), 1e-3)
        if _REPORT:
            open(_REPORT, "a").write("bf16 %-20s %s vs %s\n" % (k, a, b))
        assert (rel[:3] < 2e-2).all(), (k, a, b)
    # parameters after one warm-accumulator Adagrad step: the update is ~ the gradient; compare updates per tensor
    w0g, w0d = C.make_weights(case["g"], 11), C.make_weights(case["d"], 22)
    worst = 0.0
    for tag, w0 in (("G.", w0g), ("D.", w0d)):
        for name, init in w0.items():
            ug, ur = got[tag + name] - init, ref[tag + name] - init
            err = _rms(ug - ur) / max(_rms(ur), 1e-30)
            worst = max(worst, err)
            if _REPORT:
                open(_REPORT, "a").write("bf16 update %-40s rel-rms %.3e\n" % (tag + name, err))
            assert err < 8e-2, (tag + name, err)
    assert worst > 1e-4, "suspiciously exact: the bf16 path did not run"


@pytest.mark.parametrize("name", ["acoustic_mlp", "acoustic_mlp_dropout", "acoustic_chain_d", "acoustic_multistream_adam", "duration_mlp"])
def test_bf16_storage_mlp_steps_track_the_float32_oracle(name):
    """GT_OPT_MATMUL_BF16 on MLP generators / discriminators = bf16 STORAGE (gemm_bf16s.hip.h): activations, dZ, input
    images and weight shadows are bfloat16 in HBM, in both orientations, every product is the k-contiguous bf16 form with
    float32 accumulation; master weights, gradients and optimizer state stay float32.  Reference-shaped cases (conditioned
    and unconditioned D, injected dropout masks, multi-stream selection, R = None duration model, Adagrad with a warm
    accumulator / Adam) against the FLOAT32 oracle at the measured bf16 rounding level: outputs and losses 2e-2, counts
    within 2 %, parameter updates 0.25 relative rms per tensor (measured: up to 0.17 at these tiny hidden widths -- 32 .. 64
    units, few terms to average the rounding over; 3e-3 .. 1.4e-2 at the real widths, tests/test_gpu_at_size.py)."""
    from hip_runner import run_hip_case
    from oracle_runner import run_oracle_case
    case = dict(C.CASES[name])
    if case["opt_g"][0] == "Adagrad":
        case["opt_g"] = ("Adagrad", dict(case["opt_g"][1], initial_accumulator_value=1e-4))
        case["opt_d"] = ("Adagrad", dict(case["opt_d"][1], initial_accumulator_value=1e-4))
    case["steps"] = 2
    got = run_hip_case(case, engine_options={"matmul_bf16": 1})
    ref = run_oracle_case(case)
    for k in ("y_hat", "y_hat_static"):
        err = _rms(got[k] - ref[k]) / _rms(ref[k])
        assert err < 2e-2, (k, err)
    assert _rms(got["y_hat"] - ref["y_hat"]) > 0, "suspiciously exact: the bf16 path did not run"
    for st in range(2):
        for k, nl in (("d_scalars_%d" % st, 3), ("g_scalars_%d" % st, 4)):
            a, b = np.asarray(got[k]), np.asarray(ref[k])
            rel = np.abs(a - b) / np.maximum(np.abs(b), 1e-2)
            assert (rel[:nl] < 3e-2).all(), (k, a, b)
            if k.startswith("d_"):
                assert (np.abs(a[3:] - b[3:]) <= 0.02 * max(1.0, float(case["B"] * case["T"]))).all(), (k, a, b)
    if case["opt_g"][0] == "Adagrad":      # Adam's first steps are sign-like (m / sqrt(v)): updates are not comparable at bf16 noise
        w0g, w0d = C.make_weights(case["g"], 11), C.make_weights(case["d"], 22)
        for tag, w0 in (("G.", w0g), ("D.", w0d)):
            for nm, init in w0.items():
                ug, ur = got[tag + nm] - init, ref[tag + nm] - init
                err = _rms(ug - ur) / max(_rms(ur), 1e-30)
                assert err < 0.25, (tag + nm, err)


def test_bf16_storage_sru_step_tracks_the_float32_oracle():
    """GT_OPT_MATMUL_BF16 on the hparams-default SRU generator at its real widths (6 x 512 bidirectional, both variational
    dropouts, 425 -> 187; B = 16, T = 64): the layer inputs, dU and W go through bf16 images / shadows in both orientations
    (U = xin . W, dW = xin^T . dU, d in = dU . W^T as k-contiguous bf16 products), the scans stay float32.  Against the
    FLOAT32 oracle (the SRU cell is un-vendored: parity unpinned) at the bf16 rounding level."""
    from hip_runner import run_hip_case
    from oracle_runner import run_oracle_case
    case = dict(C.ORACLE_ONLY_CASES["acoustic_sru_at_size"])
    got = run_hip_case(case, engine_options={"matmul_bf16": 1})
    ref = run_oracle_case(case)
    for k in ("y_hat", "y_hat_static"):
        err = _rms(got[k] - ref[k]) / _rms(ref[k])
        assert 1e-5 < err < 2e-2, (k, err)
    for k in ("d_scalars_0", "g_scalars_0"):
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        rel = np.abs(a - b) / np.maximum(np.abs(b), 1e-3)
        assert (rel[:3] < 2e-2).all(), (k, a, b)
    w0g, w0d = C.make_weights(case["g"], 11), C.make_weights(case["d"], 22)
    for tag, w0 in (("G.", w0g), ("D.", w0d)):
        for name, init in w0.items():
            ug, ur = got[tag + name] - init, ref[tag + name] - init
            err = _rms(ug - ur) / max(_rms(ur), 1e-30)
            assert err < 8e-2, (tag + name, err)


@pytest.mark.parametrize("waves", [8, 4])
@pytest.mark.parametrize("name,bf16", [("acoustic_sru_at_size", 0), ("acoustic_sru_uni_k3_dropout", 0), ("vc_sru_multistream", 0), ("acoustic_sru_uni_k3", 0),
                                       ("acoustic_sru_bi_saturated", 0), ("acoustic_sru_at_size", 1), ("acoustic_sru_dropout", 1),
                                       ("acoustic_sru_dropout@T133", 0), ("acoustic_sru_dropout@T133", 1)])
def test_sru_cooperative_block_scans_match_the_sequential_scans(name, bf16, waves):
    """The cooperative block scans (sru_cs_kernels.hip.h, the default: every wave of a workgroup walks eight frames of a block from a
    zero state, the waves' composites (prod f, end state) are combined through LDS, each wave corrects its frames by prefix
    product x incoming state) against the sequential one-wave scans (sru_kernels.hip.h, gt_set_tuning("sru_coop", 0)): the same linear recurrence under another association of the
    products, so a whole G+D step agrees to rounding -- 1e-4 like every float32 comparison of the suite (bf16 storage: the products
    around the scans round their operands to bf16, where a last-bit difference of a scan output can flip a rounding: 2e-2) --
    forward and backward, both directions, k = 3 and 4, tanh / relu, saturated gates, ragged T (partial blocks: frames past T are
    the identity), partial workgroups, dU as float32 and as bf16 images.  "@T133": the case at T = 133, three ragged blocks for both
    wave counts (2 x 32 + 5 + 64, 2 x 64 + 5) -- the carried state crosses two block boundaries, the trailing block has no pair; built here,
    not in ORACLE_ONLY_CASES (the oracle's python time loop is not needed for a comparison of two kernels)."""
    from hip_runner import run_hip_case
    name, _, t_over = name.partition("@T")
    case = C.ORACLE_ONLY_CASES[name]
    if t_over:
        case = dict(case, T=int(t_over))
    from gantts_amd import _lib as L
    opts = {"matmul_bf16": 1} if bf16 else None
    try:
        L.check(L.lib.gt_set_tuning(b"sru_coop", 0))
        ref = run_hip_case(case, engine_options=opts)
        L.check(L.lib.gt_set_tuning(b"sru_coop", 1))
        L.check(L.lib.gt_set_tuning(b"sru_cs_waves", waves))      # both instantiations (8 / 4 waves per 64 columns) on every shape
        got = run_hip_case(case, engine_options=opts)
    finally:
        L.check(L.lib.gt_set_tuning(b"sru_coop", 1))
        L.check(L.lib.gt_set_tuning(b"sru_cs_waves", 0))
    assert set(got) == set(ref)
    rtol = 2e-2 if bf16 else RTOL
    frac_ok, worst_ok = _kink_frac(case)
    for k in ref:
        if "scalars" in k:
            _close(got[k], ref[k], rtol=rtol, msg=k)
            if k.startswith("d_scalars") and not bf16:
                assert got[k][3] == ref[k][3] and got[k][4] == ref[k][4], k
        elif ".opt." in k:
            sq = ".opt.sum." in k or ".opt.exp_avg_sq." in k
            _close_kink(np.sqrt(np.maximum(got[k], 0.0)) if sq else got[k], np.sqrt(np.maximum(ref[k], 0.0)) if sq else ref[k], k, frac_ok, worst_ok,
                        rtol=(8e-2 if bf16 else RTOL), atol=1e-9)
        elif k.startswith(("G.", "D.")):
            _close_kink(got[k], ref[k], k, frac_ok, worst_ok, rtol=(8e-2 if bf16 else RTOL))
        else:
            _close(got[k], ref[k], rtol=rtol, msg=k)


def test_lstm_full_size_persistent_equals_per_step_kernels():
    """cfg3 at full size (B=32, T=1024, BiLSTM 3x256, variable lengths): the persistent recurrence kernels (one launch
    per layer, W_hh resident on chip, h / dG exchanged between workgroups) against the per-step kernels the small
    reference-pinned goldens also run through -- same engine, option flipped -- on one whole G+D step; the persistent
    path must not raise its fault word."""
    import types
    import gantts_amd.train as T
    from gantts_amd import hparams, optim, paramgen
    from gantts_amd.engine import engine_for
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model
    B, Tn = 32, 1024
    gs = dict(kind="LSTMRNN", in_dim=425, out_dim=187, num_hidden=3, hidden_dim=256, bidirectional=True, dropout=0.0,
              last_sigmoid=False)
    ds = dict(kind="MLP", in_dim=483, out_dim=1, num_hidden=3, hidden_dim=256, dropout=0.0, last_sigmoid=True)
    case = dict(B=B, T=Tn, din=425, dout=187, stream_sizes=[180, 3, 1, 3])
    x_np, y_np, lengths = C.make_batch(case, seed=3)
    lengths = lengths[np.random.RandomState(0).permutation(B)]          # NOT sorted (pack_padded_sequence would need it)
    lengths[5] = 1
    hp = types.SimpleNamespace(**hparams.tts_acoustic.values())
    T.hp = hp
    R = paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, Tn)
    x, y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
    ys = get_static_features(y, 3, hp.stream_sizes, hp.has_dynamic_features)
    mask = sequence_mask(torch.from_numpy(lengths).cuda()).unsqueeze(-1)
    res = {}
    for persistent in (1, 0):
        mg, md = build_model(gs, 1).eval(), build_model(ds, 2).eval()
        og = optim.Adagrad(mg.parameters(), lr=0.01, weight_decay=1e-7, initial_accumulator_value=1e-4)
        od = optim.Adagrad(md.parameters(), lr=0.01, weight_decay=1e-7, initial_accumulator_value=1e-4)
        eng = engine_for(hp, mg)
        eng.set_option("lstm_persistent", persistent)
        og.zero_grad(), od.zero_grad()
        yh, yhs = T.apply_generator(mg, x, R, list(lengths))
        d = T.update_discriminator(md, od, x, ys, yhs, list(lengths), mask, "train")
        g = T.update_generator(mg, md, og, x, y, yh, ys, yhs, 1.0, list(lengths), mask, "train", mse_w=0.0, mge_w=1.0)
        eng.check_faults()
        res[persistent] = (d, g, yh.cpu().numpy(), mg.flat_grads().cpu().numpy().copy(), mg.flat_params().cpu().numpy().copy())
    a, b = res[1], res[0]
    assert np.isfinite(a[2]).all() and np.isfinite(a[3]).all()
    _close(a[0], b[0], msg="cfg3 D scalars persistent vs per-step")
    _close(a[1], b[1], msg="cfg3 G scalars persistent vs per-step")
    _close(a[2], b[2], msg="cfg3 y_hat persistent vs per-step")
    _close(a[3], b[3], rtol=RTOL, atol=1e-9, msg="cfg3 G grads persistent vs per-step")
    _close(a[4], b[4], rtol=RTOL, atol=1e-7, msg="cfg3 G params persistent vs per-step")
    # frames beyond a length: zero LSTM output -> exactly the hidden2out bias (pad_packed_sequence)
    bshort = 5
    bias = build_model(gs, 1).state_dict()["hidden2out.bias"].cpu().numpy()
    np.testing.assert_allclose(a[2][bshort, 1:], np.broadcast_to(bias, a[2][bshort, 1:].shape), rtol=0, atol=1e-7)


def test_sru_full_size_cfg4_step_is_finite_and_reproducible():
    """BASELINE.json configs[3] at full size (hparams-default SRU 6 x 512 bidirectional with both dropouts, B = 16,
    T = 2048): the oracle's python time loop is out of reach there (its parity case runs at T = 64, same widths), so the
    full-size run is checked through properties: finite outputs and losses, loss_mge / loss_mse of a fresh network near the
    per-frame dimension counts (y ~ N(0,1): 63 and 187), frames beyond a length DO change the output (the reference's SRU
    ignores lengths, models.py:161-164), run-to-run bit-reproducibility."""
    import types
    import gantts_amd.train as T
    from gantts_amd import hparams, models, optim, paramgen
    from gantts_amd.engine import engine_for
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    B, Tn = 16, 2048
    hp = types.SimpleNamespace(**hparams.tts_acoustic.values())
    T.hp = hp
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, Tn, 425, generator=g).cuda()
    y = torch.randn(B, Tn, 187, generator=g).cuda()
    lengths = [Tn] + [int(v) for v in torch.randint(Tn // 2, Tn, (B - 1,), generator=g)]
    R = paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, Tn)
    ys = get_static_features(y, 3, hp.stream_sizes, hp.has_dynamic_features)
    mask = sequence_mask(torch.tensor(lengths).cuda(), max_len=Tn).unsqueeze(-1)

    def once():
        torch.manual_seed(3)
        mg = models.SRURNN(in_dim=425, out_dim=187, num_hidden=6, hidden_dim=512, bidirectional=True, dropout=0.2,
                           use_relu=1, rnn_dropout=0.2).cuda().train()
        md = models.MLP(in_dim=483, out_dim=1, num_hidden=3, hidden_dim=256, dropout=0.5, last_sigmoid=True).cuda().train()
        og, od = optim.Adagrad(mg.parameters(), lr=0.01), optim.Adagrad(md.parameters(), lr=0.01)
        engine_for(hp, mg).set_seed(99)
        og.zero_grad(), od.zero_grad()
        yh, yhs = T.apply_generator(mg, x, R, lengths)
        d = T.update_discriminator(md, od, x, ys, yhs, lengths, mask, "train")
        gg = T.update_generator(mg, md, og, x, y, yh, ys, yhs, 1.0, lengths, mask, "train", mse_w=0.0, mge_w=1.0)
        return d, gg, yh.cpu(), mg.flat_params().cpu().clone()

    a, b = once(), once()
    assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert all(np.isfinite(v) for v in a[0] + a[1]) and torch.isfinite(a[2]).all() and torch.isfinite(a[3]).all()
    assert 0.5 * 63 < a[1][1] < 6 * 63 and 0.5 * 187 < a[1][0] < 6 * 187, a[1]
    assert 0 <= a[0][3] <= sum(lengths) and 0 <= a[0][4] <= sum(lengths)
    short = int(np.argmin(lengths))
    assert a[2][short, lengths[short]:].abs().max() > 0          # padded frames run through the recurrence like real ones


def _dist_hp(case):
    import types
    from gantts_amd import hparams
    hp = types.SimpleNamespace(**getattr(hparams, case["hp"]).values())
    hp.stream_sizes, hp.has_dynamic_features = case["stream_sizes"], case["has_dynamic_features"]
    hp.windows = C.WINDOWS[:case["windows"]]
    hp.order = sum(C.static_sizes(case))
    return hp


@pytest.mark.parametrize("name", sorted(C.DISTORTION_CASES))
def test_compute_distortions_matches_reference_golden(name):
    """Fused device reduction (gt_compute_distortions) vs the real train.compute_distortions fixture;
    the binarised vuv stream and the vuv error COUNT are bit-exact."""
    import gantts_amd.train as T
    gold = np.load(os.path.join(GOLDEN, "distortions.npz"))
    case = C.DISTORTION_CASES[name]
    T.hp = _dist_hp(case)
    y, yh, mean, std, lengths = C.make_distortion_inputs(case)
    ty, tyh = torch.from_numpy(y).cuda(), torch.from_numpy(yh).cuda()
    tm, ts = torch.from_numpy(mean).cuda(), torch.from_numpy(std).cuda()
    for lens in (torch.from_numpy(lengths), list(lengths)):
        got = T.compute_distortions(ty, tyh, tm, ts, lens)
        keys = [k for k in gold.files if k.startswith(name + ".") and ".split." not in k]
        assert sorted(k.split(".", 1)[1] for k in keys) == sorted(got)
        for k in keys:
            g, o = float(gold[k]), got[k.split(".", 1)[1]]
            if np.isnan(g):
                assert np.isnan(o), k
            elif k.endswith("vuv_err"):
                assert o == g, (k, o, g)                       # integer count / integer frames
            else:
                assert abs(o - g) <= 1e-5 * abs(g), (k, o, g)
    if case["name"] == "acoustic":
        for tag, t in (("y", ty), ("yh", tyh)):
            _, lf0, vuv, _ = T.split_streams(t, tm, ts)
            assert vuv.dtype == torch.int64
            np.testing.assert_array_equal(vuv.cpu().numpy(), gold["%s.split.%s.vuv" % (name, tag)])


def test_compute_distortions_full_size_properties():
    """cfg2 size (B=32, T=512, Ds=63): identical inputs -> all-zero distortions; no lengths == full
    lengths; the kernel's vuv mismatch count equals a host count over the binarised streams; the
    result does not depend on what lies beyond the lengths."""
    import types
    import gantts_amd.train as T
    from gantts_amd import hparams
    T.hp = types.SimpleNamespace(**hparams.tts_acoustic.values())
    g = torch.Generator().manual_seed(5)
    B, Tn = 32, 512
    y = torch.randn(B, Tn, 63, generator=g)
    yh = y + 0.3 * torch.randn(B, Tn, 63, generator=g)
    mean, std = torch.randn(187, generator=g) * 0.3, 0.5 + torch.rand(187, generator=g)
    mean[180], std[180], mean[183], std[183] = 5.0, 0.2, 0.5, 0.5
    lengths = torch.randint(Tn // 2, Tn + 1, (B,), generator=g)
    yc, yhc, mc, sc = y.cuda(), yh.cuda(), mean.cuda(), std.cuda()
    same = T.compute_distortions(yc, yc, mc, sc, lengths)
    assert same["mcd"] == 0 and same["bap_mcd"] == 0 and same["vuv_err"] == 0 and same["f0_rmse"] == 0
    full = T.compute_distortions(yc, yhc, mc, sc, None)
    assert full == T.compute_distortions(yc, yhc, mc, sc, [Tn] * B)
    d = T.compute_distortions(yc, yhc, mc, sc, lengths)
    ref = O.compute_distortions(O.StreamConfig([180, 3, 1, 3], [True, True, False, True], 3), "acoustic", y, yh, mean, std,
                                lengths.tolist())
    for k in ref:
        assert abs(d[k] - ref[k]) <= 1e-5 * abs(ref[k]), (k, d[k], ref[k])
    assert d["vuv_err"] == ref["vuv_err"]
    _, _, va, _ = T.split_streams(yc, mc, sc)
    _, _, vb, _ = T.split_streams(yhc, mc, sc)
    m = (torch.arange(Tn)[None, :] < lengths[:, None]).cuda()
    assert d["vuv_err"] == float(((va != vb) & m).sum().item()) / float(lengths.sum().item())
    yh2 = yhc.clone()
    yh2[~m] = 1e6
    assert T.compute_distortions(yc, yh2, mc, sc, lengths) == d


@pytest.mark.parametrize("name", sorted(C.TRAIN_LOOP_CASES))
def test_train_loop_matches_reference_golden(name):
    """gantts_amd.train.train_loop (prefetcher + cached R + HIP steps + fused distortions) against the
    log stream and final weights of the REAL reference train_loop (train.py:435-643) on the same
    in-memory dataset: same log names in the same order, values within 1e-4, accuracies exact."""
    import types
    import gantts_amd.train as T
    from gantts_amd import hparams, optim
    from hip_runner import build_model
    case = C.TRAIN_LOOP_CASES[name]
    gold = np.load(os.path.join(GOLDEN, name + ".npz"))
    hp = types.SimpleNamespace(**getattr(hparams, case["hp"]).values())
    hp.stream_sizes, hp.has_dynamic_features = case["stream_sizes"], case["has_dynamic_features"]
    hp.windows = C.WINDOWS[:case["windows"]]
    hp.adversarial_streams, hp.mask_nth_mgc_for_adv_loss = case["adversarial_streams"], case["mask_nth_mgc"]
    hp.discriminator_linguistic_condition = case["cond"]
    hp.nepoch, hp.lr_decay_schedule, hp.lr_decay_epoch = case["nepoch"], case["lr_decay_schedule"], case["lr_decay_epoch"]
    hp.generator_add_noise = False
    hp.optimizer_g_params, hp.optimizer_d_params = dict(case["opt_g"][1]), dict(case["opt_d"][1])
    if "order" in case:
        hp.order = case["order"]
    T.hp, T.global_epoch = hp, 0
    mg, md = build_model(case["g"], 11), build_model(case["d"], 22)
    ref_d = build_model(case["d"], 33) if case["reference_d"] else None
    og = getattr(optim, case["opt_g"][0])(mg.parameters(), **case["opt_g"][1])
    od = getattr(optim, case["opt_d"][0])(md.parameters(), **case["opt_d"][1])
    data, mean, std = C.make_train_loop_data(case)

    class Loader(list):
        pass

    loaders = {}
    for phase in ("train", "test"):
        ld = Loader((torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(l)) for x, y, l in data[phase])
        ld.dataset = types.SimpleNamespace(data_mean=mean, data_std=std) if case["hp"] == "vc" \
            else types.SimpleNamespace(Y_data_mean=mean, Y_data_std=std)
        loaders[phase] = ld
    logs = []
    saved_log = T.log_value
    T.log_value = lambda n, v, e: logs.append((n, float(v), int(e)))
    try:
        rc = T.train_loop((mg, md), (og, od), loaders, w_d=case["w_d"], mse_w=case["mse_w"], mge_w=case["mge_w"],
                          update_d=case["update_d"], update_g=case["update_g"], reference_discriminator=ref_d)
    finally:
        T.log_value = saved_log
    assert rc == 0 and T.global_epoch == case["nepoch"]
    assert [n for n, _, _ in logs] == [str(n) for n in gold["log.names"]]
    assert [e for _, _, e in logs] == [int(e) for e in gold["log.epochs"]]
    for (n, v, e), g in zip(logs, gold["log.values"]):
        if np.isnan(g):
            assert np.isnan(v), (n, e, v, g)                 # f0_rmse of a batch without co-voiced frames
        elif " acc" in n or "spoofing" in n or "vuv_err" in n:
            assert v == g, (n, e, v, g)                      # integer counts / integer frames
        else:
            assert abs(v - g) <= 1e-4 * max(abs(g), 1e-3), (n, e, v, g)
    assert og.param_groups[0]["lr"] == float(gold["lr_g"]) and od.param_groups[0]["lr"] == float(gold["lr_d"])
    for tag, m in (("G", mg), ("D", md)):
        for k, v in m.state_dict().items():
            _close(v.cpu().numpy(), gold[tag + "." + k], rtol=2e-4, atol=2e-6, msg=name + ":" + tag + "." + k)


def test_inference_path_matches_reference_golden():
    """gantts_amd.inference (eval-mode forwards + banded multi-stream MLPG + inverse scaling) against
    outputs of the real reference models / evaluation_tts.gen_parameters / evaluation_vc lines."""
    from gantts_amd import inference as INF
    from hip_runner import build_model
    gold = np.load(os.path.join(GOLDEN, "inference.npz"))
    I, inp = C.INFERENCE, C.make_inference_inputs()
    X_min = {"acoustic": inp["X_min_acoustic"], "duration": inp["X_min_duration"]}
    X_max = {"acoustic": inp["X_max_acoustic"], "duration": inp["X_max_duration"]}
    Y_mean = {"acoustic": inp["Y_mean_acoustic"], "duration": inp["Y_mean_duration"]}
    Y_std = {"acoustic": inp["Y_std_acoustic"], "duration": inp["Y_std_duration"]}
    for tag, spec in (("lstm", I["acoustic"]), ("mlp", I["acoustic_mlp"])):
        model = build_model(spec, 41)
        pred = INF.predict_acoustic(model, inp["feats_acoustic"], X_min, X_max)
        _close(pred, gold["acoustic_predicted." + tag], msg="acoustic_predicted." + tag)
        assert not model.training
        got = INF.gen_parameters(pred, Y_mean, Y_std)
        for n, v in zip(("mgc", "lf0", "vuv", "bap"), got):
            g = gold["%s.%s" % (n, tag)]
            assert v.shape == g.shape, n
            _close(v, g, msg="%s.%s" % (n, tag))
        # from the reference's own prediction: isolates MLPG + inverse scaling
        got = INF.gen_parameters(gold["acoustic_predicted." + tag], Y_mean, Y_std)
        for n, v in zip(("mgc", "lf0", "vuv", "bap"), got):
            _close(v, gold["%s.%s" % (n, tag)], rtol=2e-5, msg="%s.%s (ref input)" % (n, tag))
    d = INF.predict_duration(build_model(I["duration"], 42), inp["feats_duration"], X_min, X_max, Y_mean, Y_std)
    assert d.shape == gold["durations"].shape and d.min() >= 1
    assert (d != gold["durations"]).sum() <= 1, "rounded durations differ in more than one borderline entry"
    inputs, outputs, diff = INF.vc_convert(build_model(I["vc"], 43), gold["vc_mc"], inp["vc_mean"], inp["vc_std"], diffvc=True)
    np.testing.assert_array_equal(inputs, gold["vc_mc"][:, :25])
    _close(outputs, gold["vc_outputs"], msg="vc_outputs")
    _close(diff, gold["vc_diff"], rtol=1e-4, atol=1e-5, msg="vc_diff")
    with pytest.raises(NotImplementedError):
        INF.gen_parameters(gold["acoustic_predicted.mlp"], Y_mean, Y_std, mge_training=False)


_DP_SCHEDULES = {
    "default": None,        # count with the D loss sums (unnormalised seeds), closing messages on the step stream, riders
    "round3": {"comm_tv_in_sums": 0, "comm_close_inline": 0, "launch_riders": 0},      # six collectives, all on the communicator's stream
    "count_ahead": {"comm_tv_in_sums": 0},                                              # the count all-reduced ahead of the head
}


@pytest.mark.parametrize("schedule", sorted(_DP_SCHEDULES))
@pytest.mark.parametrize("name", ["acoustic_mlp_dropout", "acoustic_lstm", "vc_in2out", "acoustic_chain_d+fused"])
def test_engine_communicator_world_1_matches_reference_golden(name, schedule):
    """gt_comm_init with one rank: the step goes through the engine's data-parallel path (global valid-frame count,
    per-layer gradient buckets handed to RCCL on the communicator's stream under the backward pass, loss sums, join,
    clip + optimizer on the reduced gradient) and must reproduce the reference-generated fixture exactly like the
    plain path does -- in every message schedule (GT_OPT_COMM_*): the default one (the count leaves with the D loss sums, the
    backward pass runs on the unnormalised loss and the optimizer kernel applies 1 / Tv), the round-3 one, and the one in between."""
    from hip_runner import run_hip_case
    opts = dict(_DP_SCHEDULES[schedule] or {})
    if name.endswith("+fused"):      # the fused discriminator stack under the communicator (unnormalised seeds, the count from the collective, deferred head sums)
        name, opts["fused_dstack"] = name[:-6], 2
    case = C.CASES[name]
    gold = np.load(os.path.join(GOLDEN, name + ".npz"))
    got = run_hip_case(case, comm_world_1=True, engine_options=opts or None)
    for k in gold.files:
        if k.startswith("g_leak_norm"):
            continue
        if "scalars" in k:
            _close(got[k], gold[k], msg=k)
            if k.startswith("d_scalars"):
                assert got[k][3] == gold[k][3] and got[k][4] == gold[k][4]
        elif ".opt." in k:
            _close_state(got[k], gold[k], k)
        else:
            _close(got[k], gold[k], msg=k)


def test_engine_communicator_schedule_trace_accounts_for_every_gradient_byte():
    """gt_comm_trace (bench.py --comm-trace): with one rank and forced collectives every step's messages carry each network's whole
    gradient exactly once plus its loss sums; every record is a well-formed interval, and the traced run still reproduces the fixture."""
    from hip_runner import run_hip_case
    name = "acoustic_mlp_dropout"
    case = C.CASES[name]
    gold = np.load(os.path.join(GOLDEN, name + ".npz"))
    held = {}

    def start(eng):
        eng.comm_trace(True)
        held["eng"] = eng
    got = run_hip_case(case, comm_world_1=True, extra={"after_comm": start})
    rec = held["eng"].comm_trace_read()
    held["eng"].comm_trace(False)
    assert rec.shape[1] == 5 and len(rec) > 0
    assert set(np.unique(rec[:, 0])) <= {0.0, 1.0}
    assert (rec[:, 4] >= rec[:, 3]).all() and rec[0, 3] == 0.0
    msgs, waits = rec[rec[:, 0] == 0], rec[rec[:, 0] == 1]
    assert len(waits) >= 2 * case["steps"]                      # each backward pass ends with the step stream joining the communicator
    n_g = sum(v.size for k, v in gold.items() if k.startswith("G.") and ".opt." not in k)
    n_d = sum(v.size for k, v in gold.items() if k.startswith("D.") and ".opt." not in k)
    grad_bytes = msgs[msgs[:, 1] > 64][:, 1].sum()               # (the sums are a few doubles)
    assert grad_bytes == 4.0 * (n_g + n_d) * case["steps"], (grad_bytes, n_g, n_d)
    small = msgs[msgs[:, 1] <= 64]
    assert len(small) >= 2 * case["steps"] and (small[:, 1] % 8 == 0).all()
    for k in gold.files:
        if "scalars" in k:
            _close(got[k], gold[k], msg=k)


def _dp2_hip_worker(rank, world, port, q):
    """One of two processes sharing cuda:0: HipStepBackend on its shard, DataParallelStep over a gloo group (device
    tensors staged through the host -- two RCCL ranks cannot share one GPU)."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import gantts_amd.train as T
    from gantts_amd import optim, paramgen
    from gantts_amd.engine import HipStepBackend
    from gantts_amd.multistream import get_static_features
    from gantts_amd.parallel import DataParallelStep
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model, make_hp
    case = C.CASES["acoustic_mlp"]
    hp = make_hp(case)
    T.hp = hp
    mg, md = build_model(case["g"], 11).eval(), build_model(case["d"], 22).eval()
    og = getattr(optim, case["opt_g"][0])(mg.parameters(), **case["opt_g"][1])
    od = getattr(optim, case["opt_d"][0])(md.parameters(), **case["opt_d"][1])
    x_np, y_np, lengths = C.make_batch(case)
    rows = np.arange(case["B"])[rank::world]
    x, y = torch.from_numpy(x_np[rows]).cuda(), torch.from_numpy(y_np[rows]).cuda()
    lens = lengths[rows]
    batch = dict(x=x, y=y, R=paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, case["T"]), lengths=list(lens),
                 y_static=get_static_features(y, 3, hp.stream_sizes, hp.has_dynamic_features),
                 mask=sequence_mask(torch.from_numpy(lens).cuda(), max_len=case["T"]).unsqueeze(-1))
    dp = DataParallelStep(HipStepBackend(hp, mg, md, og, od), reduce_via_host=True)
    hist = []
    for _ in range(case["steps"]):
        d, g = dp.step(batch, adv_w=case["adv_w"], mse_w=case["mse_w"], mge_w=case["mge_w"])
        hist.append((tuple(d), tuple(g)))
    torch.cuda.synchronize()
    params = {"G." + k: v.cpu().numpy() for k, v in mg.state_dict().items()}
    params.update({"D." + k: v.cpu().numpy() for k, v in md.state_dict().items()})
    q.put((rank, hist, params))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_dp2_hip_backend_two_processes_equal_whole_batch_golden():
    """world_size 2 through a REAL process group with the HIP split-phase backend on both ranks (one GPU, two
    processes, two engines): sharded batch == the reference's result on the whole batch, replicas bit-identical."""
    import socket
    import torch.multiprocessing as mp
    case = C.CASES["acoustic_mlp"]
    gold = np.load(os.path.join(GOLDEN, "acoustic_mlp.npz"))
    s_ = socket.socket()
    s_.bind(("127.0.0.1", 0))
    port = s_.getsockname()[1]
    s_.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp2_hip_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = sorted([q.get(timeout=500) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank, hist, params in results:
        for i, (d, g) in enumerate(hist):
            _close(d, gold["d_scalars_%d" % i], msg="dp2 rank %d step %d D" % (rank, i))
            assert d[3] == gold["d_scalars_%d" % i][3] and d[4] == gold["d_scalars_%d" % i][4]
            _close(g, gold["g_scalars_%d" % i], msg="dp2 rank %d step %d G" % (rank, i))
    for k in results[0][2]:
        _close(results[0][2][k], gold[k], msg="dp2 " + k)
    for k in results[0][2]:
        assert np.array_equal(results[0][2][k], results[1][2][k]), k       # replicas bit-identical


def test_data_parallel_step_through_rccl_world_1():
    """DataParallelStep with a real process group (backend "nccl" == RCCL, one rank, every collective executed:
    async all-reduce of the device-resident valid-frame count, coalesced gradient + loss-sum all-reduces) ==
    the plain step.  The multi-rank semantics are covered by the gloo test and the two-engine emulation."""
    import socket
    import torch.distributed as dist
    from gantts_amd.parallel import DataParallelStep
    from hip_runner import run_hip_case
    if dist.is_initialized():
        pytest.skip("a process group is already initialised in this process")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        case = C.CASES["acoustic_mlp"]
        whole = run_hip_case(case)
        be, b = _dp_objects(case, np.arange(case["B"]))
        dp = DataParallelStep(be, always_reduce=True)
        assert dp._coalesce
        for i in range(case["steps"]):
            d, g = dp.step(b, adv_w=case["adv_w"], mse_w=case["mse_w"], mge_w=case["mge_w"])
            _close(d, whole["d_scalars_%d" % i], msg="rccl dp d")
            _close(g, whole["g_scalars_%d" % i], msg="rccl dp g")
        for tag, m in (("G", be.mg), ("D", be.md)):
            for k, v in m.state_dict().items():
                _close(v.cpu().numpy(), whole["%s.%s" % (tag, k)], msg=k)
        # test phase: only the loss sums travel
        d, g = dp.step(b, adv_w=case["adv_w"], mse_w=case["mse_w"], mge_w=case["mge_w"], phase="test")
        assert np.isfinite(d[0]) and np.isfinite(g[3])
        # lazy generator scalars: same numbers, fetched on first use (here: by the following step, then explicitly)
        from gantts_amd.parallel import LazyResult
        d1, g1 = dp.step(b, adv_w=case["adv_w"], mse_w=case["mse_w"], mge_w=case["mge_w"], phase="test", lazy_g=True)
        d2, g2 = dp.step(b, adv_w=case["adv_w"], mse_w=case["mse_w"], mge_w=case["mge_w"], phase="test", lazy_g=True)
        assert isinstance(g1, LazyResult) and g1._value is not None and g2._value is None
        assert tuple(g1) == tuple(g) and tuple(g2) == tuple(g) and d1 == d and d2 == d
    finally:
        dist.destroy_process_group()


def test_generator_noise_step_matches_oracle_values():
    """cfg5's data path by VALUE: generator_add_noise feeds G with cat(x, z) (train.py:504-506, 542) while the
    conditioned discriminator still sees x alone (train.py:254-256) -- G's first layer is in_dim + noise_dim wide, D's
    conditioning width differs from G's input width, and G's weight gradient must be taken against cat(x, z).  Same z
    on both sides, dropout masks injected, two steps, against the CPU oracle."""
    import types
    import gantts_amd.train as T
    from gantts_amd import hparams, optim, paramgen
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model
    B, Tn, din, nz = 4, 30, 40, 9
    gs = dict(kind="MLP", in_dim=din + nz, out_dim=187, num_hidden=2, hidden_dim=48, dropout=0.5, last_sigmoid=False)
    ds = dict(kind="MLP", in_dim=58 + din, out_dim=1, num_hidden=2, hidden_dim=24, dropout=0.5, last_sigmoid=True)
    case = dict(B=B, T=Tn, din=din, dout=187, stream_sizes=[180, 3, 1, 3], g=gs, d=ds)
    x_np, y_np, lengths = C.make_batch(case, seed=21)
    rs = np.random.RandomState(77)
    z_np = rs.rand(B, Tn, nz).astype(np.float32)
    hp = types.SimpleNamespace(**hparams.tts_acoustic.values())
    hp.generator_add_noise, hp.generator_noise_dim = True, nz
    T.hp = hp
    R_np = np.array(paramgen.unit_variance_mlpg_matrix(hp.windows, Tn))
    okw = dict(lr=0.01, weight_decay=1e-7, initial_accumulator_value=1e-4)
    mg, md = build_model(gs, 3).train(), build_model(ds, 4).train()
    og, od = optim.Adagrad(mg.parameters(), **okw), optim.Adagrad(md.parameters(), **okw)
    omg = O.OracleMLP(**{k: v for k, v in gs.items() if k != "kind"})
    omd = O.OracleMLP(**{k: v for k, v in ds.items() if k != "kind"})
    omg.load_state_dict(C.make_weights(gs, 3)), omd.load_state_dict(C.make_weights(ds, 4))
    oog, ood = O.OracleAdagrad(omg.params, **okw), O.OracleAdagrad(omd.params, **okw)
    cfg = O.StreamConfig([180, 3, 1, 3], [True, True, False, True], 3, [True, False, False, False], 2, True)
    x, y, z, R = (torch.from_numpy(a).cuda() for a in (x_np, y_np, z_np, R_np))
    ys = get_static_features(y, 3, hp.stream_sizes, hp.has_dynamic_features)
    mask = sequence_mask(torch.from_numpy(lengths).cuda()).unsqueeze(-1)
    xc, yc, zc, Rc = (torch.from_numpy(a) for a in (x_np, y_np, z_np, R_np))
    omask = O.sequence_mask(lengths, Tn).unsqueeze(-1)
    oys = O.get_static_features(yc, 3, cfg.stream_sizes, cfg.has_dynamic_features)
    for st in range(2):
        gm = [(rs.rand(B, Tn, 48) >= 0.5).astype(np.float32) for _ in range(2)]
        dm = [(rs.rand(B, Tn, 24) >= 0.5).astype(np.float32) for _ in range(6)]
        mg.set_dropout_masks(0, [torch.from_numpy(m) for m in gm])
        for p_ in range(3):
            md.set_dropout_masks(p_, [torch.from_numpy(m) for m in dm[2 * p_:2 * p_ + 2]])
        og.zero_grad(), od.zero_grad()
        yh, yhs = T.apply_generator(mg, torch.cat((x, z), -1), R, list(lengths))
        d = T.update_discriminator(md, od, x, ys, yhs, list(lengths), mask, "train")
        g = T.update_generator(mg, md, og, x, y, yh, ys, yhs, 1.0, list(lengths), mask, "train", mse_w=0.2, mge_w=1.0)
        dd = O._DropoutSource([torch.from_numpy(m) for m in dm])
        oog.zero_grad(), ood.zero_grad()
        oyh, oyhs = O.apply_generator(cfg, omg, torch.cat((xc, zc), -1), Rc, list(lengths), drop=O._DropoutSource([torch.from_numpy(m) for m in gm]))
        od_ = O.update_discriminator(cfg, omd, ood, xc, oys, oyhs, list(lengths), omask, "train", drop=dd)
        og_ = O.update_generator(cfg, omg, omd, oog, xc, yc, oyh, oys, oyhs, 1.0, list(lengths), omask, "train",
                                 mse_w=0.2, mge_w=1.0, drop=dd)
        _close(yh.cpu().numpy(), oyh.detach().numpy(), msg="noise step %d y_hat" % st)
        _close(d, od_, msg="noise step %d D scalars" % st)
        _close(g, og_, msg="noise step %d G scalars" % st)
    for (k, v), r in list(zip(mg.state_dict().items(), omg.params)) + list(zip(md.state_dict().items(), omd.params)):
        _close(v.cpu().numpy(), r.detach().numpy(), msg="noise " + k)


def test_train_loop_with_generator_noise_and_two_engines_in_one_process():
    """cfg5 plumbing: generator_add_noise=True (G in_dim += noise_dim, z ~ U[0,1) drawn on the device,
    train.py:504-506, 542) and two independent engines (duration: R=None / Adam; acoustic) alive in one process.
    No reference fixture can exist (torch's CPU RNG stream): checks the mechanics -- finite logs, weights move,
    the two engines do not disturb each other, the noise stream is reproducible for a fixed seed."""
    import types
    import gantts_amd.train as T
    from gantts_amd import hparams, optim
    from hip_runner import build_model

    def run(case_name, noise_dim, seed):
        case = dict(C.TRAIN_LOOP_CASES[case_name])
        hp = types.SimpleNamespace(**getattr(hparams, case["hp"]).values())
        hp.stream_sizes, hp.has_dynamic_features = case["stream_sizes"], case["has_dynamic_features"]
        hp.windows = C.WINDOWS[:case["windows"]]
        hp.adversarial_streams, hp.mask_nth_mgc_for_adv_loss = case["adversarial_streams"], case["mask_nth_mgc"]
        hp.discriminator_linguistic_condition = case["cond"]
        hp.nepoch, hp.lr_decay_schedule, hp.lr_decay_epoch = 1, False, 10
        hp.generator_add_noise, hp.generator_noise_dim, hp.generator_noise_seed = True, noise_dim, seed
        hp.optimizer_g_params, hp.optimizer_d_params = dict(case["opt_g"][1]), dict(case["opt_d"][1])
        T.hp, T.global_epoch = hp, 0
        g_spec = dict(case["g"], in_dim=case["g"]["in_dim"] + noise_dim)
        mg, md = build_model(g_spec, 11), build_model(case["d"], 22)
        w0 = mg.flat_params().clone()
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
        saved = T.log_value
        T.log_value = lambda n, v, e: logs.append((n, float(v)))
        try:
            assert T.train_loop((mg, md), (og, od), loaders, w_d=1.0, mse_w=0.0, mge_w=1.0) == 0
        finally:
            T.log_value = saved
        assert all(np.isfinite(v) or "f0_rmse" in n for n, v in logs), logs
        assert not torch.equal(w0, mg.flat_params())
        return mg.flat_params().clone(), md.flat_params().clone(), logs

    a1 = run("train_loop_acoustic", 7, 123)
    d1 = run("train_loop_d_warmup", 5, 9)           # a second (G, D, hp) set: its own engines
    a2 = run("train_loop_acoustic", 7, 123)         # same seed after the other engines ran: identical
    a3 = run("train_loop_acoustic", 7, 124)
    assert torch.equal(a1[0], a2[0]) and torch.equal(a1[1], a2[1])
    assert not torch.equal(a1[0], a3[0])
    assert len(d1[2]) > 0


@pytest.mark.parametrize("B,T", [(1, 1), (1, 2), (2, 1), (3, 1), (1, 33)])
def test_tiny_batches_match_oracle(B, T):
    """Degenerate shapes (one sequence, one or two frames, one frame past a 32-row tile): one full G+D step vs the
    oracle.  Outputs, the 9 scalars and the squared-gradient accumulators are compared tightly.  The first Adagrad
    step is lr * sign(g): with a handful of frames a few gradient entries are pure rounding noise around zero, so
    the updated weights are allowed a few entries that differ by (at most) 2 * lr -- measured: <= 5 of 27 200."""
    from hip_runner import run_hip_case
    from oracle_runner import run_oracle_case
    case = dict(C.CASES["acoustic_mlp"], B=B, T=T, steps=1)
    lr = case["opt_g"][1]["lr"]
    got, ref = run_hip_case(case), run_oracle_case(case)
    for k, r in ref.items():
        if k.startswith("g_leak_norm"):
            continue
        a, b = np.asarray(got[k], dtype=np.float64), np.asarray(r, dtype=np.float64)
        if ".opt." in k:
            _close_state(a, b, k)
        elif k.startswith(("G.", "D.")):
            bad = np.abs(a - b) > 1e-4 * max(1e-30, float(np.abs(b).max())) + 1e-6
            assert bad.sum() <= max(1, a.size // 2000), (k, int(bad.sum()), a.size)
            assert np.abs(a - b).max() <= 2.1 * lr, (k, float(np.abs(a - b).max()))
        else:
            _close(a, b, msg=k)


def _adv_term_cases():
    from test_gpu_sru_discriminator import SRUD_CASES
    srud = SRUD_CASES["srud_uni_k4_cond"]
    return {"mlp_split": (C.CASES["acoustic_chain_d"], None), "mlp_cat": (C.CASES["acoustic_chain_d"], {"split_first_layer": 0}),
            "mlp_bf16": (C.CASES["acoustic_mlp_dropout"], {"matmul_bf16": 1}), "lstm": (C.CASES["acoustic_lstm_d"], None),
            "sru": (srud, None), "sru_bf16": (srud, {"sru_d_bf16": 1})}


@pytest.mark.parametrize("backend", ["mlp_split", "mlp_cat", "mlp_bf16", "lstm", "sru", "sru_bf16"])
def test_adversarial_term_without_a_d_step_equals_the_one_behind_a_d_step(backend):
    """The generator step's adversarial term builds the generated half of D's input itself when no D step of the same batch left it
    behind (a miss of the engine's image cache), and reuses it otherwise.  Eval phase, eval-mode networks (no dropout, no update),
    every discriminator backend: apply_generator + update_generator on a fresh engine against apply_generator +
    update_discriminator + update_generator on a second fresh engine with the same seed.  Both builders only copy (or round to bf16)
    the same values and an eval D step changes no weight, so loss_adv and loss_g are bit-identical."""
    import gantts_amd.train as T
    from gantts_amd import optim, paramgen
    from gantts_amd.engine import engine_for
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model, make_hp
    case, options = _adv_term_cases()[backend]
    hp = make_hp(case)
    x_np, y_np, lengths = C.make_batch(case)
    res = {}
    for with_d in (False, True):
        T.hp = hp
        mg, md = build_model(case["g"], 11).eval(), build_model(case["d"], 22).eval()
        og = getattr(optim, case["opt_g"][0])(mg.parameters(), **case["opt_g"][1])
        od = getattr(optim, case["opt_d"][0])(md.parameters(), **case["opt_d"][1])
        eng = engine_for(hp, mg)
        eng.set_seed(4711)
        for k, v in (options or {}).items():
            eng.set_option(k, v)
        x, y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
        R = paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, case["T"])
        ys = get_static_features(y, len(hp.windows), hp.stream_sizes, hp.has_dynamic_features)
        mask = sequence_mask(torch.from_numpy(np.ascontiguousarray(lengths)).cuda(), max_len=case["T"]).unsqueeze(-1)
        yh, yhs = T.apply_generator(mg, x, R, list(lengths))
        if with_d:
            T.update_discriminator(md, od, x, ys, yhs, list(lengths), mask, "test")
        g = T.update_generator(mg, md, og, x, y, yh, ys, yhs, case["adv_w"], list(lengths), mask, "test", mse_w=case["mse_w"],
                               mge_w=case["mge_w"])
        res[with_d] = np.array(g, dtype=np.float64)
    print("%s G scalars alone %s behind a D step %s" % (backend, res[False], res[True]))
    assert np.isfinite(res[False]).all() and res[False][2] > 0
    assert res[False][2] == res[True][2] and res[False][3] == res[True][3], (backend, res[False], res[True])
