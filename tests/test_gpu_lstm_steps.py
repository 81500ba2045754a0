"""The per-step LSTM kernels, odd hidden widths and the recurrent discriminator's backward-data route against float64.

The harness is tests/test_gpu_lstm_recurrence.py's (one generator step, the float64 oracle once per shape, path counts,
padding == hidden2out.bias bit for bit, y_hat and every gradient tensor); this file adds the shapes that module's matrix
never takes: hidden widths that are no multiple of 4 (lstm_fwd_step_kernel / lstm_bwd_step_kernel then stage through
lstm_stage_kc(vec = false) and the backward's scalar W_hh loop), H < 4, H > 512 (per-step kernels only, a third K chunk),
more than 32 sequences (blockIdx.z > 0, the Bpad state rows, a ragged last batch tile), a unidirectional stack and a
recurrent discriminator on the per-step route, and lstm_stack_backward(want_w = false, dx0) -- the generator's adversarial
term through a recurrent discriminator.

Which case reaches which kernel and path (K chunks of LSTM_KC = 256 staged per launch; batch tiles of 32 sequences):

  kernel / path                          case                       K chunks                      sequences     units
                                                                                                  per batch     per unit
                                                                                                  tile          tile
  lstm_fwd_step_kernel, vector (H%4=0)   h260u-steps                2: 256 + 4 (clamp at H - 4)   32 + 1        32 x 8 + 4
                                         h520                       3: 256 + 256 + 8              3             65 x 8
                                         adversarial term, G H=12   1: 12                         32 + 5        8 + 4
                                         (h40-steps, h264-steps, h24t1 of the recurrence matrix: 1 / 2 / 1 chunks, one tile)
  lstm_fwd_step_kernel, scalar           h37-steps, shrinking batch 1: 37                         32 + 5; 3     4 x 8 + 5
                                         h3-steps                   1: 3                          2             3
                                         h515                       3: 256 + 256 + 3              3             64 x 8 + 3
                                         D H=13 (D step / adv term) 1: 13                         32 + 8 / + 5  8 + 5
  lstm_bwd_step_kernel, vector           h260u-steps                5: 4 x 256 + 16 (K = 1040)    32 + 1        8 x 32 + 4
                                         h520                       9: 8 x 256 + 32 (K = 2080)    3             16 x 32 + 8
                                         adversarial term, G H=12   1: 48                         32 + 5        12
                                         (h40-steps, h264-steps, h24t1: 1 / 5 / 1 chunks, one tile)
  lstm_bwd_step_kernel, scalar           h37-steps, shrinking batch 1: 148                        32 + 5; 3     32 + 5
                                         h3-steps                   1: 12                         2             3
                                         h515                       9: 8 x 256 + 12 (K = 2060)    3             16 x 32 + 3
                                         D H=13 (D step / adv term) 1: 52                         32 + 8 / + 5  13
  lstm_shift_kernel, d = 0 and d = 1     every bidirectional case above whose step wants weight gradients (h37, h3, h520,
                                         D step H=13, adversarial term's generator); d = 0 alone: h260u, h515.  The
                                         discriminator's backward inside the adversarial term (want_w = false) launches none.

The persistent kernels see the same odd widths (h37: forward UPC 8 with a 5-unit last workgroup, UPC 16 likewise, backward
2 x 16 + 5; h3; h260u), h37 also with the bf16 recurrence over float32 products (matmul_bf16 with H % 8 != 0) and with the
agent-scope exchange.

The host tests at the end prove that the comparison discriminates: the float64 oracle with one of the errors such a kernel
can make (a lost K chunk or K tail, a wrong reverse start, a batch-tile offset, a unit tile without recurrent input) misses
_close by at least 10 x its limit.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases as C
import gantts_oracle as O
import test_gpu_lstm_recurrence as R
from test_gpu_lstm_recurrence import DECLINED_SLOT, DOUT, SHAPES, STEPS_SLOT, _batch, _case, _case_id, _expected, _slot, expected_counts, reference
from test_gpu_parity import RTOL, _close, _scale_of

CASES = ([_case(s, persistent=p) for s in ("h37", "h3", "h260u") for p in (0, 1)]
         + [_case("h37", bt=bt, upc=upc) for bt in (8, 16) for upc in (8, 16)]
         + [_case("h37", bf16=1), _case("h37", xcd_local=0)]
         + [_case("h520"), _case("h515")])


# ---------------------------------------------------------------------------------------------------------------------
# host checks of the cases
# ---------------------------------------------------------------------------------------------------------------------
def test_cases_take_the_routes_they_are_named_for():
    by_id = {_case_id(c): _expected(c) for c in CASES}
    assert len(by_id) == len(CASES)
    for c in CASES:
        H, L, _, _, _, _ = SHAPES[c["shape"]]
        e = _expected(c)
        assert sum(e) == 2 * L + e[DECLINED_SLOT]
        if not c["persistent"] or H > 512:
            assert e[STEPS_SLOT] == 2 * L and e[DECLINED_SLOT] == 0, _case_id(c)
        else:
            assert e[STEPS_SLOT] == 0, _case_id(c)
    # h37: both forward unit counts and both batch tiles, f32 and the bf16 recurrence; h260u: HP 512 falls through to UPC 16
    for bt in (8, 16):
        for upc in (8, 16):
            e = by_id["h37-f32-bt%d-upc%d" % (bt, upc)]
            assert e[_slot(0, 256, upc, bt, 0)] == 2 and e[_slot(1, 256, 8, bt, 0)] == 2
    assert by_id["h37-bf16-btauto-upcauto"][_slot(0, 256, 8, 8, 1)] == 2 and by_id["h37-bf16-btauto-upcauto"][_slot(1, 256, 8, 8, 1)] == 2
    assert by_id["h260u-f32-btauto-upcauto"][_slot(0, 512, 16, 8, 0)] == 2 and by_id["h260u-f32-btauto-upcauto"][_slot(1, 512, 8, 8, 0)] == 2
    # the shapes are what the docstring's table says of them
    assert [SHAPES[s][0] % 4 for s in ("h37", "h3", "h260u", "h520", "h515")] == [1, 3, 0, 0, 3]
    assert all(SHAPES[s][3] > 32 for s in ("h37", "h260u")) and all(SHAPES[s][0] > 512 for s in ("h520", "h515"))


# ---------------------------------------------------------------------------------------------------------------------
# the kernels against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_generator_step_vs_float64(case):
    R.assert_step(R.run_engine(case), reference(case["shape"]), _expected(case), _case_id(case), bf16=case["bf16"])


@pytest.mark.gpu
def test_shrinking_batch_on_one_engine_vs_float64():
    """The per-step kernels' state scratch only grows and is laid out by Bpad: a step on 37 sequences of 7 frames, then --
    same model, same engine -- one on its first 3 sequences cut to 4 frames.  The second step is compared with the float64
    oracle on that sub-batch, run with the weights the first step left in the model."""
    case = _case("h37", persistent=0)
    ref = reference("h37")
    e = R.make_engine(case)
    R.assert_step(R.engine_step(e, case, ref), ref, _expected(case), "h37-steps first step")
    B2, T2 = 3, 4
    lengths = np.minimum(ref["lengths"][:B2], T2)
    lengths[int(np.argmax(ref["lengths"][:B2]))] = T2
    x, y = ref["x"][:B2, :T2].copy(), ref["y"][:B2, :T2].copy()
    for b, n in enumerate(lengths):
        x[b, n:] = 0
        y[b, n:] = 0
    weights = {k: v.cpu().numpy() for k, v in e["mg"].state_dict().items()}
    assert any(not np.array_equal(weights[k], v) for k, v in C.make_weights(R._gspec("h37"), 7).items())     # the first step did update
    sub = R.oracle_step(R._gspec("h37"), weights, x, y, lengths)
    R.assert_step(R.engine_step(e, case, sub), sub, _expected(case), "h37-steps second step, 3 sequences of 4 frames")


DSPEC13 = dict(kind="LSTMRNN", in_dim=58, out_dim=1, num_hidden=2, hidden_dim=13, bidirectional=True, dropout=0.0, last_sigmoid=True)


@pytest.mark.gpu
def test_recurrent_discriminator_step_on_the_step_kernels_vs_float64():
    """A D step of a bidirectional 2 x 13 LSTMRNN on the per-step kernels: its one pass over 2B = 40 sequences spans two
    batch tiles (32 + 8), on the scalar staging path."""
    B, T = 20, 6
    R.dstep_vs_float64(DSPEC13, B, T, expected_counts("dstep13", 13, 2, True, 2 * B, T, persistent=0), persistent=0)


ADV = dict(B=37, T=6, din=9)
_GSPEC12 = dict(kind="LSTMRNN", in_dim=ADV["din"], out_dim=DOUT, num_hidden=2, hidden_dim=12, bidirectional=True, dropout=0.0,
                last_sigmoid=False)


def _adv_expected(persistent):
    g = expected_counts("advg", 12, 2, True, ADV["B"], ADV["T"], persistent=persistent)
    d = expected_counts("advd", 13, 2, True, ADV["B"], ADV["T"], persistent=persistent)        # the generated half alone: B sequences
    return [a + b for a, b in zip(g, d)]


def test_adversarial_term_expected_counts():
    assert _adv_expected(0)[STEPS_SLOT] == 8 and sum(_adv_expected(0)) == 8
    e = _adv_expected(1)
    assert e[_slot(0, 256, 8, 8, 0)] == 4 and e[_slot(1, 256, 8, 8, 0)] == 4 and sum(e) == 8


@pytest.mark.gpu
@pytest.mark.parametrize("persistent", [0, 1], ids=["steps", "persistent"])
def test_adversarial_term_through_a_recurrent_discriminator_vs_float64(persistent):
    """One generator step with adv_w = mse_w = mge_w = 1 of an LSTMRNN generator against an LSTMRNN discriminator: the
    discriminator's backward runs without weight gradients and hands the gradient of its input back (lstm_stack_backward:
    want_w = false, dx0).  y_hat and the generator's gradients against the oracle's update_generator with the same
    discriminator in float64 (no LeakyReLU in either network: no kink allowance); the discriminator's gradient buffer
    must come out of the step as it went in."""
    import gantts_amd.train as T
    from gantts_amd import optim, paramgen
    from gantts_amd.engine import engine_for
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model
    B, Tn = ADV["B"], ADV["T"]
    tag = "adversarial term, %s" % ("persistent" if persistent else "steps")
    x_np, y_np, lengths = _batch(B, Tn, ADV["din"], seed=11)
    hp = R._hp()
    T.hp = hp
    mg, md = build_model(_GSPEC12, 7).eval(), build_model(DSPEC13, 4).eval()
    og = optim.Adagrad(mg.parameters(), lr=0.01, initial_accumulator_value=1e-4)
    bias0 = mg.state_dict()["hidden2out.bias"].cpu().numpy().copy()
    eng = engine_for(hp, mg)
    eng.set_option("lstm_persistent", persistent)
    x, y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
    Rm = paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, Tn)
    ys = get_static_features(y, 3, hp.stream_sizes, hp.has_dynamic_features)
    mask = sequence_mask(torch.from_numpy(lengths).cuda(), max_len=Tn).unsqueeze(-1)
    dgrad = md.flat_grads()
    dgrad.copy_(torch.arange(dgrad.numel(), dtype=torch.float32, device=dgrad.device).mul_(0.25).sub_(7.0))
    dgrad0 = dgrad.clone()
    eng.lstm_path_counts(reset=True)
    og.zero_grad()
    yh, yhs = T.apply_generator(mg, x, Rm, list(lengths))
    T.update_generator(mg, md, og, x, y, yh, ys, yhs, 1.0, list(lengths), mask, "train", mse_w=1.0, mge_w=1.0)
    eng.check_faults()
    counts = eng.lstm_path_counts()
    flat = mg.flat_grads().cpu().numpy().astype(np.float64)
    assert torch.equal(md.flat_grads(), dgrad0), tag + ": the generator step wrote to the discriminator's gradients"

    f64 = torch.float64
    og64 = O.OracleLSTMRNN(**{k: v for k, v in _GSPEC12.items() if k != "kind"})
    og64.load_state_dict(C.make_weights(_GSPEC12, 7))
    od64 = O.OracleLSTMRNN(**{k: v for k, v in DSPEC13.items() if k != "kind"})
    od64.load_state_dict(C.make_weights(DSPEC13, 4))
    for o in (og64, od64):
        O.cast_model(o, f64)
        o.training = False
    opt = O.OracleAdagrad(og64.params, lr=0.01, initial_accumulator_value=1e-4)
    cfg = R._ocfg()
    xc, yc = torch.from_numpy(x_np).to(f64), torch.from_numpy(y_np).to(f64)
    R64 = torch.from_numpy(np.array(paramgen.unit_variance_mlpg_matrix(C.WINDOWS[:3], Tn))).to(f64)
    omask = O.sequence_mask(list(lengths), Tn).unsqueeze(-1).to(f64)
    oys = O.get_static_features(yc, 3, R.STREAMS, R.DYN)
    opt.zero_grad()
    oyh, oyhs = O.apply_generator(cfg, og64, xc, R64, list(lengths))
    O.update_generator(cfg, og64, od64, opt, xc, yc, oyh, oys, oyhs, 1.0, list(lengths), omask, "train", mse_w=1.0, mge_w=1.0)
    assert list(mg.state_dict().keys()) == og64.names
    ref = dict(lengths=lengths, y_hat=oyh.detach().numpy(), names=og64.names, grads=[p.grad.numpy() for p in og64.params])
    grads, off = [], 0
    for r in ref["grads"]:
        grads.append(flat[off:off + r.size].reshape(r.shape))
        off += r.size
    assert off == flat.size
    R.assert_step(dict(counts=counts, y_hat=yh.cpu().numpy(), grads=grads, bias=bias0), ref, _adv_expected(persistent), tag)


# ---------------------------------------------------------------------------------------------------------------------
# host: the comparisons discriminate
# ---------------------------------------------------------------------------------------------------------------------
class MutatedLSTMRNN(O.OracleLSTMRNN):
    """OracleLSTMRNN._recurrent restated with one kernel error switched on (every layer and direction alike):
      whh_cols_from = k    the recurrent product stops at column k of W_hh (a lost K chunk / K tail)
      rev_full = b         the reverse direction of sequence b starts at frame T - 1 instead of its own last frame
      state_from = (b, s)  sequence b's recurrent state (h and c) is read from sequence s (a batch-tile offset)
      no_rec_units = u0    hidden units >= u0 get no recurrent input (a unit tile that was never staged)
    With none of them it is the oracle (checked below).  dtanh: mean of tanh'(c) over the active (layer, direction, b, t, unit)."""

    def __init__(self, whh_cols_from=None, rev_full=None, state_from=None, no_rec_units=None, **kw):
        O.OracleLSTMRNN.__init__(self, **kw)
        self.mut = (whh_cols_from, rev_full, state_from, no_rec_units)
        self.dtanh = None

    def _recurrent(self, x, lengths, drop, idx=0):
        whh_cols_from, rev_full, state_from, no_rec_units = self.mut
        B, T, _ = x.shape
        lens = torch.as_tensor([int(v) for v in lengths])
        H = self.H
        inp = x
        dts, n_act = 0.0, 0.0
        for l in range(self.L):
            outs = []
            for d in range(self.dirs):
                Wih, Whh, bih, bhh = self.params[idx:idx + 4]
                idx += 4
                if whh_cols_from is not None:
                    Whh = Whh * (torch.arange(H) < whh_cols_from).to(x.dtype)
                xp = F.linear(inp, Wih, bih + bhh)
                h, c = x.new_zeros(B, H), x.new_zeros(B, H)
                seq = [None] * T
                for t in (range(T - 1, -1, -1) if d else range(T)):
                    act = (t < lens).to(x.dtype).unsqueeze(1)
                    run = act.clone()                      # whether the state runs at this frame
                    if rev_full is not None and d == 1:
                        run[rev_full] = 1.0
                    if state_from is not None:
                        sel = torch.arange(B)
                        sel[state_from[0]] = state_from[1]
                        h, c = h[sel], c[sel]
                    rec = F.linear(h, Whh)
                    if no_rec_units is not None:
                        rec = rec * (torch.arange(4 * H) % H < no_rec_units).to(x.dtype)
                    g = xp[:, t] + rec
                    i, f, gg, o = g[:, :H].sigmoid(), g[:, H:2 * H].sigmoid(), g[:, 2 * H:3 * H].tanh(), g[:, 3 * H:].sigmoid()
                    c = run * (f * c + i * gg)
                    h = run * (o * c.tanh())
                    seq[t] = act * h
                    dts += float((act * (1.0 - c.detach().tanh() ** 2)).sum())
                    n_act += float(act.sum()) * H
                outs.append(torch.stack(seq, 1))
            inp = torch.cat(outs, -1)
        self.dtanh = dts / n_act
        return inp


def _worst_violation(mut, ref, tag):
    """Largest error of the mutated step in units of _close's limit, over y_hat and every gradient tensor; each tensor that
    is outside must make _close itself fail."""
    worst = 0.0
    for msg, a, b in [(tag + " y_hat", mut["y_hat"], ref["y_hat"])] + [(tag + " grad " + nm, g, r) for nm, g, r in
                                                                        zip(ref["names"], mut["grads"], ref["grads"])]:
        ratio = float((np.abs(a - b) / (1e-6 + RTOL * _scale_of(b, msg))).max())
        if ratio > 1.0:
            with pytest.raises(AssertionError):
                _close(a, b, msg=msg)
        else:
            _close(a, b, msg=msg)
        worst = max(worst, ratio)
    return worst


def _second_tile_short_sequence(shape):
    lengths, T = reference(shape)["lengths"], SHAPES[shape][4]
    b = 32 + int(np.argmin(lengths[32:]))
    assert lengths[b] < T
    return b


MUTATIONS = {
    "a-h520-third-k-chunk-lost": ("h520", lambda: dict(whh_cols_from=512)),
    "b-h37-scalar-k-tail-lost": ("h37", lambda: dict(whh_cols_from=37 - 37 % 4)),
    "b-h515-scalar-k-tail-lost": ("h515", lambda: dict(whh_cols_from=515 - 515 % 4)),
    "c-h37-reverse-start-at-T-1": ("h37", lambda: dict(rev_full=_second_tile_short_sequence("h37"))),
    "d-h37-sequence-32-reads-the-state-of-sequence-0": ("h37", lambda: dict(state_from=(32, 0))),
    "e-h37-last-unit-tile-without-recurrent-input": ("h37", lambda: dict(no_rec_units=32)),
}


@pytest.mark.parametrize("shape", sorted({s for s, _ in MUTATIONS.values()}))
def test_mutation_harness_without_a_mutation_is_the_oracle(shape):
    ref = reference(shape)
    same = R.oracle_step(R._gspec(shape), C.make_weights(R._gspec(shape), 7), ref["x"], ref["y"], ref["lengths"], model_cls=MutatedLSTMRNN)
    assert np.array_equal(same["y_hat"], ref["y_hat"]) and all(np.array_equal(g, r) for g, r in zip(same["grads"], ref["grads"]))
    # the gates are unsaturated: a saturated cell would hide the recurrent input from the output and from every gradient
    assert same["model"].dtanh > 0.1, same["model"].dtanh


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_comparison_fails_a_mutated_recurrence_by_10x(name):
    shape, kw = MUTATIONS[name]
    ref = reference(shape)
    mut = R.oracle_step(R._gspec(shape), C.make_weights(R._gspec(shape), 7), ref["x"], ref["y"], ref["lengths"], model_cls=MutatedLSTMRNN, **kw())
    worst = _worst_violation(mut, ref, name)
    print("%s: worst error %.1f x the limit" % (name, worst))
    assert worst >= 10.0, (name, worst)
