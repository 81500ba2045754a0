"""Every instantiation of the LSTM recurrence kernels against a float64 oracle.

lstm_launch_seq (gantts_amd/csrc/eng_lstm.hip) runs one layer's forward or backward recurrence as ONE persistent launch,
picking one of 24 kernel instantiations -- forward: HP (hidden units padded to 256 / 512) x UPC (8 / 16 hidden units per
workgroup) x BT (8 / 16 sequences per batch tile) x f32 / bf16 products; backward: HP x BT x f32 / bf16 -- and falls back to
the per-step kernels when no grid is co-resident.  The engine counts the layer-passes of every instantiation
(gt_lstm_path_counts), so each case here asserts WHICH kernels ran as well as what they computed.

A case is one generator step (zero_grad, apply_generator, update_generator with adv_w = 0, so no LeakyReLU of the
discriminator enters the generator's gradient): y_hat and every gradient tensor are compared with the oracle run in float64
on the same inputs (computed once per shape).  Lengths are unsorted and include 1 and T; the last batch tile is ragged
unless the shape says otherwise.  The discriminator case does the same for a recurrent discriminator's step, whose one
pass over 2B sequences is what picks 16-sequence tiles at B = 32.

The per-step kernels beyond one batch tile and two K chunks, hidden widths that are no multiple of 4 and the adversarial
term through a recurrent discriminator are tests/test_gpu_lstm_steps.py, on this module's helpers and shapes.
"""
import functools

import numpy as np
import pytest
import torch

import cases as C
import gantts_oracle as O
from test_gpu_parity import _close

STREAMS = [180, 3, 1, 3]
DYN = [True, True, False, True]
ADV = [True, False, False, False]
DOUT = sum(STREAMS)
NXCD = 8                      # MI355X: 8 XCDs of 32 CUs (eng_lstm.hip: seq_xcds)

# bf16 limits (GT_OPT_MATMUL_BF16: operands rounded to 8 mantissa bits, float32 accumulation), measured on the MI355X over
# every bf16 case of MATRIX against the float64 oracle.  Per tensor: relative rms, and the worst single error relative to
# the tensor's largest magnitude -- for y_hat the worst of any one sequence over its valid frames, for a gradient (one
# tensor per layer and direction) the worst element.  Each limit is 4x its measured worst value at most and stays under
# the caps of test_matmul_bf16_step_tracks_the_float32_oracle (2e-2 outputs, 8e-2 gradients).  h37-bf16 (test_gpu_lstm_steps.py)
# is the mixed state of matmul_bf16 with H % 8 != 0 -- the bf16 recurrence over float32 products -- and stays below each.
Y_RMS_LIM = 1e-2              # measured worst 2.60e-3 (h256-bf16-btauto-upcauto); h37-bf16 1.20e-3
Y_SEQ_LIM = 1.2e-2            # measured worst 3.11e-3 (h256-bf16-btauto-upcauto, h264-bf16); h37-bf16 2.22e-3
G_RMS_LIM = 2e-2              # measured worst 5.91e-3 (h24t2-bf16); h37-bf16 3.23e-3
G_WORST_LIM = 2.5e-2          # measured worst 6.59e-3 (h24t2-bf16); h37-bf16 4.38e-3

# Shapes of the matrix: (H, layers, bidirectional, B, T, in_dim)
SHAPES = {
    "h40": (40, 2, True, 5, 13, 20),          # HP 256; with BT 16 one tile of 5 sequences and 11 empty rows
    "h256": (256, 2, True, 64, 20, 425),      # B = 64 bidirectional: 16-sequence tiles chosen automatically, all full
    "h264": (264, 1, True, 20, 17, 31),       # HP 512 with 248 padded units; H % 8 == 0, so the bf16 products apply
    "h512": (512, 1, False, 3, 9, 17),        # the largest HP 512 layer
    "h24t2": (24, 2, True, 4, 2, 9),          # the shortest sequence the persistent kernels take
    "h24t1": (24, 2, True, 4, 1, 9),          # T = 1: per-step kernels
    # odd hidden widths and the per-step route beyond one batch tile / two K chunks (cases: tests/test_gpu_lstm_steps.py)
    "h37": (37, 2, True, 37, 7, 11),          # H % 4 = 1; per-step unit tiles 4 x 8 + 5 forward, 32 + 5 backward; batch tiles 32 + 5
    "h3": (3, 1, True, 2, 3, 5),              # H < 4: one partial tile everywhere, K = 12 in the backward
    "h260u": (260, 2, False, 33, 5, 9),       # H % 4 = 0 with a 4-wide K tail; unidirectional stack; batch tiles 32 + 1
    "h520": (520, 1, True, 3, 4, 9),          # H > 512: forward K chunks 256 + 256 + 8, backward K = 2080 = 8 chunks + 32
    "h515": (515, 1, False, 3, 4, 9),         # H > 512 with H % 4 = 3
}

# Instantiations MI355X refuses for a shape (the grid is not co-resident: eng_lstm.hip launch_seq): key (shape, pass, HP,
# UPC, BT, bf16) -> why.  The launcher's forward then tries UPC 16; where nothing fits the pass runs on the per-step kernels.
# MI355X: the forward HP 512 kernels with 8 units per workgroup get one workgroup per CU (the launcher keeps a margin of one
# block below what the occupancy API reports), so the cdiv(H, 8) >= 33 workgroups of a group never fit the 32 CUs of one XCD:
# the launcher takes UPC 16 instead.  The h264 / h512 cases that force UPC 8 assert exactly that fall-through.
_HP512_UPC8 = "forward HP 512 x UPC 8: cdiv(H, 8) >= 33 workgroups per group, one per CU, 32 CUs per XCD"
REFUSED = {(s, "fwd", 512, 8, bt, p): _HP512_UPC8 for s in ("h264", "h512") for bt in (8, 16) for p in (0, 1)}
REFUSED[("h260u", "fwd", 512, 8, 8, 0)] = _HP512_UPC8          # cdiv(260, 8) = 33 as well (tests/test_gpu_lstm_steps.py)
# Instantiations no case of MATRIX reaches, with the reason: slot -> why.  Which case reaches each of the other 20 slots
# (forward 16 * 0 + ..., backward 16 + ...):
#   0 / 1   fwd 256 UPC 8  BT 8   f32 / bf16   h40-bt8-upc8, h24t2          16 / 17  bwd 256 BT 8   h40-bt8-*, h24t2
#   2 / 3   fwd 256 UPC 8  BT 16               h40-bt16-upc8, h256-upcauto   18 / 19  bwd 256 BT 16  h40-bt16-*, h256-*
#   4 / 5   fwd 256 UPC 16 BT 8                h40-bt8-upc16                 24 / 25  bwd 512 BT 8   h264-bt8-*, h512-*
#   6 / 7   fwd 256 UPC 16 BT 16               h40-bt16-upc16, h256-upc16    26 / 27  bwd 512 BT 16  h264-bt16-*
#   12 / 13 fwd 512 UPC 16 BT 8                h264-bt8-*, h512-*
#   14 / 15 fwd 512 UPC 16 BT 16               h264-bt16-*
# (slots 2 and 18 also by the recurrent discriminator's step)
UNREACHED = {16 * 0 + 8 + 2 * bt16 + p: _HP512_UPC8 for bt16 in (0, 1) for p in (0, 1)}


def _case(shape, bf16=0, bt=0, upc=0, persistent=1, xcd_local=1):
    return dict(shape=shape, bf16=bf16, bt=bt, upc=upc, persistent=persistent, xcd_local=xcd_local)


MATRIX = ([_case("h40", p, bt, upc) for p in (0, 1) for bt in (8, 16) for upc in (8, 16)]
          + [_case("h256", p, 0, upc) for p in (0, 1) for upc in (0, 16)] + [_case("h256", xcd_local=0)]
          + [_case("h264", p, bt, upc) for p in (0, 1) for bt in (8, 16) for upc in (8, 16)]
          + [_case("h512", p, 0, upc) for p in (0, 1) for upc in (0, 16)]
          + [_case("h24t2", p) for p in (0, 1)] + [_case("h24t1")]
          + [_case("h40", persistent=0), _case("h264", persistent=0)])


def _case_id(c):
    return "%s-%s-bt%s-upc%s%s%s" % (c["shape"], "bf16" if c["bf16"] else "f32", c["bt"] or "auto", c["upc"] or "auto",
                                     "" if c["persistent"] else "-steps", "" if c["xcd_local"] else "-agent-scope")


def _slot(backward, hp, upc, bt, bf16):
    return 16 * int(backward) + 8 * int(hp == 512) + 4 * int(upc == 16 and not backward) + 2 * int(bt == 16) + int(bool(bf16))


ALL_SLOTS = sorted({_slot(bw, hp, upc, bt, p) for bw in (0, 1) for hp in (256, 512) for upc in (8, 16) for bt in (8, 16)
                    for p in (0, 1)})
STEPS_SLOT, DECLINED_SLOT, NSLOTS = 32, 33, 34


def expected_counts(shape, H, L, bi, B, T, bf16=0, bt=0, upc=0, persistent=1, xcd_local=1):
    """The launcher's choice (eng_lstm.hip: lstm_launch_seq) for every layer-pass of one step: L forward + L backward
    passes, each in ONE launch for all directions and batch tiles."""
    counts = [0] * NSLOTS
    dirs = 2 if bi else 1
    for backward in (0, 1):
        for _ in range(L):
            if not persistent or H > 512 or T < 2:
                counts[STEPS_SLOT] += 1
                continue
            hp = 256 if H <= 256 else 512
            tile = bt or (16 if dirs * -(-B // 16) >= NXCD else 8)
            tries = [8] if backward else [u for u in (8, 16) if u >= (upc if upc in (8, 16) else 8)]
            for u in tries:
                if (shape, "bwd" if backward else "fwd", hp, None if backward else u, tile, bf16) not in REFUSED:
                    counts[_slot(backward, hp, u, tile, bf16)] += 1
                    break
            else:
                counts[DECLINED_SLOT] += 1
                counts[STEPS_SLOT] += 1
    return counts


def _expected(c):
    H, L, bi, B, T, _ = SHAPES[c["shape"]]
    return expected_counts(c["shape"], H, L, bi, B, T, **{k: c[k] for k in ("bf16", "bt", "upc", "persistent", "xcd_local")})


def _lengths(B, T, seed):
    """Unsorted, with 1 and T."""
    rs = np.random.RandomState(seed)
    n = rs.randint(1, T + 1, size=B)
    i1, iT = rs.permutation(B)[:2] if B > 1 else (0, 0)
    n[i1] = 1
    n[iT] = T
    return n.astype(np.int64)


def _batch(B, T, din, seed):
    rs = np.random.RandomState(seed)
    x = (0.01 + 0.98 * rs.rand(B, T, din)).astype(np.float32)
    y = rs.randn(B, T, DOUT).astype(np.float32)
    lengths = _lengths(B, T, seed + 1)
    for b, n in enumerate(lengths):
        x[b, n:] = 0
        y[b, n:] = 0
    return x, y, lengths


def _gspec(shape):
    H, L, bi, B, T, din = SHAPES[shape]
    return dict(kind="LSTMRNN", in_dim=din, out_dim=DOUT, num_hidden=L, hidden_dim=H, bidirectional=bi, dropout=0.0,
                last_sigmoid=False)


def _ocfg():
    return O.StreamConfig(STREAMS, DYN, 3, ADV, 2, False)


def _hp():
    from hip_runner import make_hp
    return make_hp(dict(hp="tts_acoustic", stream_sizes=STREAMS, has_dynamic_features=DYN, windows=3, adversarial_streams=ADV,
                        mask_nth_mgc=2, cond=False))


_DSPEC_MLP = dict(kind="MLP", in_dim=58, out_dim=1, num_hidden=1, hidden_dim=16, dropout=0.0, last_sigmoid=True)


def oracle_step(spec, weights, x, y, lengths, model_cls=None, **model_kw):
    """The float64 oracle's generator step (adv_w = 0) of an LSTMRNN with `weights` on one batch: y_hat and the gradient of
    every parameter tensor.  model_cls: an OracleLSTMRNN subclass (the mutated recurrences of test_gpu_lstm_steps.py)."""
    from gantts_amd import paramgen
    T = x.shape[1]
    o = (model_cls or O.OracleLSTMRNN)(**{k: v for k, v in spec.items() if k != "kind"}, **model_kw)
    o.load_state_dict(weights)
    O.cast_model(o, torch.float64)
    o.training = False
    opt = O.OracleAdagrad(o.params, lr=0.01, initial_accumulator_value=1e-4)
    cfg = _ocfg()
    f64 = torch.float64
    xc, yc = torch.from_numpy(x).to(f64), torch.from_numpy(y).to(f64)
    R = torch.from_numpy(np.array(paramgen.unit_variance_mlpg_matrix(C.WINDOWS[:3], T))).to(f64)
    mask = O.sequence_mask(list(lengths), T).unsqueeze(-1).to(f64)
    ys = O.get_static_features(yc, 3, STREAMS, DYN)
    opt.zero_grad()
    yh, yhs = O.apply_generator(cfg, o, xc, R, list(lengths))
    O.update_generator(cfg, o, None, opt, xc, yc, yh, ys, yhs, 0.0, list(lengths), mask, "train", mse_w=1.0, mge_w=1.0)
    return dict(x=x, y=y, lengths=lengths, y_hat=yh.detach().numpy().copy(), names=list(o.names),
                grads=[p.grad.numpy().copy() for p in o.params], model=o)


@functools.lru_cache(maxsize=None)
def reference(shape):
    """The float64 oracle's generator step on the shape's inputs: y_hat and the gradient of every parameter tensor."""
    H, L, bi, B, T, din = SHAPES[shape]
    x, y, lengths = _batch(B, T, din, seed=H + B + T)
    return oracle_step(_gspec(shape), C.make_weights(_gspec(shape), 7), x, y, lengths)


def make_engine(c):
    """The case's generator (weights of seed 7), an MLP discriminator, the optimizer and the engine with the case's kernel
    selection."""
    import gantts_amd.train as T
    from gantts_amd import optim
    from gantts_amd.engine import engine_for
    from hip_runner import build_model
    hp = _hp()
    T.hp = hp
    mg, md = build_model(_gspec(c["shape"]), 7).eval(), build_model(_DSPEC_MLP, 8).eval()
    og = optim.Adagrad(mg.parameters(), lr=0.01, initial_accumulator_value=1e-4)
    eng = engine_for(hp, mg)
    eng.set_option("matmul_bf16", c["bf16"])
    eng.set_option("lstm_persistent", c["persistent"])
    eng.set_option("lstm_fwd_units", c["upc"])
    eng.set_option("lstm_xcd_local", c["xcd_local"])
    return dict(hp=hp, mg=mg, md=md, og=og, eng=eng)


def engine_step(e, c, ref):
    """One generator step (zero_grad, apply_generator, update_generator with adv_w = 0) of make_engine's objects on the
    batch of `ref` (x, y, lengths; its gradients give the split of the flat gradient)."""
    import gantts_amd.train as T
    from gantts_amd import _lib as L
    from gantts_amd import paramgen
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    hp, mg, md, og, eng = e["hp"], e["mg"], e["md"], e["og"], e["eng"]
    T.hp = hp
    Tn = ref["x"].shape[1]
    bias0 = mg.state_dict()["hidden2out.bias"].cpu().numpy().copy()      # what y_hat was computed with (the step updates it)
    L.check(L.lib.gt_set_tuning(b"lstm_bt", c["bt"]))
    try:
        x, y = torch.from_numpy(ref["x"]).cuda(), torch.from_numpy(ref["y"]).cuda()
        lengths = list(ref["lengths"])
        R = paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, Tn)
        ys = get_static_features(y, 3, hp.stream_sizes, hp.has_dynamic_features)
        mask = sequence_mask(torch.from_numpy(ref["lengths"]).cuda(), max_len=Tn).unsqueeze(-1)
        eng.lstm_path_counts(reset=True)
        og.zero_grad()
        yh, yhs = T.apply_generator(mg, x, R, lengths)
        T.update_generator(mg, md, og, x, y, yh, ys, yhs, 0.0, lengths, mask, "train", mse_w=1.0, mge_w=1.0)
        eng.check_faults()
        counts = eng.lstm_path_counts()
    finally:
        L.check(L.lib.gt_set_tuning(b"lstm_bt", 0))
    flat = mg.flat_grads().cpu().numpy().astype(np.float64)
    grads, off = [], 0
    for r in ref["grads"]:
        grads.append(flat[off:off + r.size].reshape(r.shape))
        off += r.size
    assert off == flat.size and list(mg.state_dict().keys()) == ref["names"]
    return dict(counts=counts, y_hat=yh.cpu().numpy(), grads=grads, bias=bias0)


def run_engine(c):
    """One generator step of the engine with the case's kernel selection; returns the path counts, y_hat, the gradients
    split like the oracle's parameters, and hidden2out.bias as y_hat saw it."""
    return engine_step(make_engine(c), c, reference(c["shape"]))


def bf16_errors(got, ref, lengths=None):
    """(relative rms, worst single error relative to max |ref|).  With `lengths` (a (B, T, ...) frame tensor) the worst
    error is taken per sequence over its valid frames, so that one broken sequence cannot average away."""
    g, r = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if lengths is not None:
        valid = np.arange(r.shape[1])[None, :] < np.asarray(lengths)[:, None]
        g, r = g[valid], r[valid]
    d = np.abs(g - r)
    scale = max(float(np.abs(r).max()), 1e-300)
    rms = float(np.sqrt((d * d).mean()) / max(float(np.sqrt((r * r).mean())), 1e-300))
    return rms, float(d.max()) / scale


def assert_bf16(got, ref, msg, rms_lim, worst_lim, lengths=None):
    rms, worst = bf16_errors(got, ref, lengths)
    assert rms <= rms_lim and worst <= worst_lim, "%s: bf16 vs float64 relative rms %.3e (limit %.1e), worst %s %.3e (limit %.1e)" % (
        msg, rms, rms_lim, "sequence" if lengths is not None else "element", worst, worst_lim)


def _assert_padding_is_bias(y_hat, lengths, bias, msg):
    for b, n in enumerate(lengths):
        tail = y_hat[b, n:]
        assert np.array_equal(tail, np.broadcast_to(bias, tail.shape)), "%s: frames past length %d of sequence %d are not hidden2out.bias" % (msg, n, b)


def assert_step(got, ref, expect, tag, bf16=False):
    """What every case asserts of one step: the path counts, padding frames, y_hat and every gradient tensor."""
    assert got["counts"] == expect, "%s: kernel path counts %s, expected %s" % (
        tag, {i: n for i, n in enumerate(got["counts"]) if n}, {i: n for i, n in enumerate(expect) if n})
    _assert_padding_is_bias(got["y_hat"], ref["lengths"], got["bias"], tag)
    if bf16:
        figs = [bf16_errors(got["y_hat"], ref["y_hat"], ref["lengths"])] + [bf16_errors(g, r) for g, r in zip(got["grads"], ref["grads"])]
        print("%s bf16 vs float64: y_hat rms %.3e worst sequence %.3e; gradients worst rms %.3e worst element %.3e" % (
            tag, figs[0][0], figs[0][1], max(f[0] for f in figs[1:]), max(f[1] for f in figs[1:])))
        assert_bf16(got["y_hat"], ref["y_hat"], tag + " y_hat", Y_RMS_LIM, Y_SEQ_LIM, ref["lengths"])
        for nm, g, r in zip(ref["names"], got["grads"], ref["grads"]):
            assert_bf16(g, r, tag + " grad " + nm, G_RMS_LIM, G_WORST_LIM)
    else:
        _close(got["y_hat"], ref["y_hat"], msg=tag + " y_hat")
        for nm, g, r in zip(ref["names"], got["grads"], ref["grads"]):
            _close(g, r, msg=tag + " grad " + nm)


# ---------------------------------------------------------------------------------------------------------------------
# host checks of the matrix itself
# ---------------------------------------------------------------------------------------------------------------------
def test_matrix_reaches_every_instantiation():
    """The union of the persistent slots the cases expect is all 24 instantiations, minus the named unreachable ones."""
    assert len(ALL_SLOTS) == 24
    reached = set()
    for c in MATRIX:
        counts = _expected(c)
        reached |= {s for s in ALL_SLOTS if counts[s]}
    reached |= {s for s in ALL_SLOTS if DSTEP_EXPECT[s]}
    assert sorted(set(ALL_SLOTS) - reached) == sorted(UNREACHED), (sorted(set(ALL_SLOTS) - reached), sorted(UNREACHED))
    # every forced tile / unit count that is refused falls through as the launcher does, and the two non-persistent routes
    # are in the matrix as well
    assert any(_expected(c)[STEPS_SLOT] and not _expected(c)[DECLINED_SLOT] for c in MATRIX if SHAPES[c["shape"]][4] == 1)
    assert any(not c["persistent"] for c in MATRIX)


def test_bf16_criterion_catches_one_corrupted_frame():
    """One sequence's output corrupted at one frame by an amount the relative-rms limit alone accepts must fail."""
    ref = reference("h40")
    yh, lengths = ref["y_hat"], ref["lengths"]
    assert_bf16(yh, yh, "exact", Y_RMS_LIM, Y_SEQ_LIM, lengths)
    b = int(np.argmax(lengths))
    t = int(lengths[b]) // 2
    bad = yh.copy()
    bad[b, t, 0] += 1.5 * Y_SEQ_LIM * np.abs(yh[np.arange(yh.shape[1])[None, :] < lengths[:, None]]).max()
    rms, worst = bf16_errors(bad, yh, lengths)
    assert rms <= Y_RMS_LIM and worst > Y_SEQ_LIM, (rms, worst)
    with pytest.raises(AssertionError):
        assert_bf16(bad, yh, "corrupted", Y_RMS_LIM, Y_SEQ_LIM, lengths)


def test_lstm_bt_knob_and_path_counts_reject_bad_arguments():
    from gantts_amd import _lib as L
    for v in (8, 16, 0):
        assert L.lib.gt_set_tuning(b"lstm_bt", v) == L.GT_OK
    for v in (-1, 1, 4, 12, 32):
        assert L.lib.gt_set_tuning(b"lstm_bt", v) == L.GT_ERR_INVALID and b"lstm_bt" in L.lib.gt_last_error()
    assert L.lib.gt_lstm_path_counts(None, None, 0) == L.GT_ERR_INVALID


def test_expected_counts_model_the_launcher():
    """Spot checks of the launcher model against eng_lstm.hip's rules."""
    # bidirectional B = 32: four 16-sequence groups < 8 XCDs -> 8-sequence tiles; B = 49 -> 2 x 4 = 8 groups -> 16
    assert expected_counts("x", 256, 1, True, 32, 10)[_slot(0, 256, 8, 8, 0)] == 1
    assert expected_counts("x", 256, 1, True, 49, 10)[_slot(0, 256, 8, 16, 0)] == 1
    assert expected_counts("x", 256, 1, False, 113, 10)[_slot(1, 256, 8, 16, 0)] == 1
    assert expected_counts("x", 256, 1, False, 112, 10)[_slot(1, 256, 8, 8, 0)] == 1
    assert expected_counts("x", 600, 2, True, 4, 10)[STEPS_SLOT] == 4
    assert expected_counts("x", 8, 3, True, 4, 1)[STEPS_SLOT] == 6 and sum(expected_counts("x", 8, 3, True, 4, 1)) == 6


# ---------------------------------------------------------------------------------------------------------------------
# the kernels against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", MATRIX, ids=[_case_id(c) for c in MATRIX])
def test_generator_step_vs_float64(case):
    assert_step(run_engine(case), reference(case["shape"]), _expected(case), _case_id(case), bf16=case["bf16"])


# recurrent discriminator: MLP generator, bidirectional 2 x 32 LSTMRNN discriminator, B = 32.  The D step runs the natural
# and the generated sequences as ONE batch of 2B = 64: 2 directions x 4 tiles = 8 groups -> 16-sequence tiles
DSTEP = dict(B=32, T=11, din=23)
_DSPEC_RNN = dict(kind="LSTMRNN", in_dim=58, out_dim=1, num_hidden=2, hidden_dim=32, bidirectional=True, dropout=0.0,
                  last_sigmoid=True)
_GSPEC_MLP = dict(kind="MLP", in_dim=DSTEP["din"], out_dim=DOUT, num_hidden=2, hidden_dim=32, dropout=0.0, last_sigmoid=False)
DSTEP_EXPECT = expected_counts("dstep", 32, 2, True, 2 * DSTEP["B"], DSTEP["T"])


def dstep_vs_float64(dspec, B, Tn, expect, persistent=1):
    """The discriminator gradients of one D step against the float64 oracle's update_discriminator, fed the engine's own
    y_hat_static (the generator is not under test here)."""
    import gantts_amd.train as T
    from gantts_amd import optim, paramgen
    from gantts_amd.engine import engine_for
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model
    x_np, y_np, lengths = _batch(B, Tn, DSTEP["din"], seed=5)
    hp = _hp()
    T.hp = hp
    mg, md = build_model(_GSPEC_MLP, 3).eval(), build_model(dspec, 4).eval()
    od = optim.Adagrad(md.parameters(), lr=0.01, initial_accumulator_value=1e-4)
    og = optim.Adagrad(mg.parameters(), lr=0.01, initial_accumulator_value=1e-4)
    eng = engine_for(hp, mg)
    eng.set_option("lstm_persistent", persistent)
    x, y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
    R = paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, Tn)
    ys = get_static_features(y, 3, hp.stream_sizes, hp.has_dynamic_features)
    mask = sequence_mask(torch.from_numpy(lengths).cuda(), max_len=Tn).unsqueeze(-1)
    eng.lstm_path_counts(reset=True)
    og.zero_grad(), od.zero_grad()
    _, yhs = T.apply_generator(mg, x, R, list(lengths))
    T.update_discriminator(md, od, x, ys, yhs, list(lengths), mask, "train")
    eng.check_faults()
    counts = eng.lstm_path_counts()
    got = md.flat_grads().cpu().numpy().astype(np.float64)
    assert counts == expect, ({i: n for i, n in enumerate(counts) if n}, {i: n for i, n in enumerate(expect) if n})

    f64 = torch.float64
    o = O.OracleLSTMRNN(**{k: v for k, v in dspec.items() if k != "kind"})
    o.load_state_dict(C.make_weights(dspec, 4))
    O.cast_model(o, f64)
    o.training = False
    opt = O.OracleAdagrad(o.params, lr=0.01, initial_accumulator_value=1e-4)
    yc = torch.from_numpy(y_np).to(f64)
    oys = O.get_static_features(yc, 3, STREAMS, DYN)
    oyhs = yhs.detach().cpu().to(f64)
    omask = O.sequence_mask(list(lengths), Tn).unsqueeze(-1).to(f64)
    opt.zero_grad()
    O.update_discriminator(_ocfg(), o, opt, torch.from_numpy(x_np).to(f64), oys, oyhs, list(lengths), omask, "train")
    assert list(md.state_dict().keys()) == o.names
    off = 0
    for nm, p in zip(o.names, o.params):
        r = p.grad.numpy()
        _close(got[off:off + r.size].reshape(r.shape), r, msg="recurrent D grad " + nm)
        off += r.size
    assert off == got.size


@pytest.mark.gpu
def test_recurrent_discriminator_step_vs_float64():
    """The bidirectional 2 x 32 discriminator at B = 32 on the persistent kernels (16-sequence tiles)."""
    dstep_vs_float64(_DSPEC_RNN, DSTEP["B"], DSTEP["T"], DSTEP_EXPECT)
