"""-m gpu: SRURNN in the DISCRIMINATOR slot (train.py:773-774 builds the discriminator from any model class).

The engine runs the role-generic SRU stack (gantts_amd/csrc/eng_sru.hip: sru_stack_forward / sru_stack_backward) for role D: D(real) and
D(fake) of the D step as ONE batch of 2B sequences, each half with its own variational masks, its own stashes beside the generator's, the
fused head on the top layer's h, and the gradient w.r.t. the generated rows' adversarial columns (the un-detached leak of the D step,
train.py:265,274, and the adversarial gradient of the G step, train.py:307-308).  Everything is judged against the CPU oracle
(oracle/gantts_oracle.py: OracleSRURNN) -- the SRU cell is un-vendored third-party code, so like every SRU path this one is PARITY UNPINNED.

hip_runner.run_hip_case slices a discriminator's injected masks by len(hidden_sites(d)) per pass, which is not the number of masks an
SRURNN with both dropouts draws per pass: the injected-mask runs use the step driver below (the same loop, `dm` cut in thirds)."""
import copy

import numpy as np
import pytest
import torch

import cases as C

pytestmark = pytest.mark.gpu

ADG = ("Adagrad", dict(lr=0.01, weight_decay=1e-7, initial_accumulator_value=1e-4))
ADAM = ("Adam", dict(lr=1e-3, betas=(0.5, 0.9), weight_decay=0))
GMLP = dict(kind="MLP", in_dim=20, out_dim=187, num_hidden=2, hidden_dim=32, dropout=0.0, last_sigmoid=False)


def _case(B, T, din, cond, steps, dropout_on, opt, g, d):
    d = dict(dict(kind="SRURNN", out_dim=1, last_sigmoid=True, dropout=0.0, rnn_dropout=0.0), **d)
    return dict(hp="tts_acoustic", B=B, T=T, din=din, dout=187, stream_sizes=[180, 3, 1, 3], has_dynamic_features=[True, True, False, True],
                adversarial_streams=[True, False, False, False], mask_nth_mgc=2, windows=3, cond=cond, g=dict(g), d=d,
                opt_g=opt, opt_d=opt, steps=steps, adv_w=1.0, mse_w=0.0, mge_w=1.0, dropout_on=dropout_on, update_d=True, update_g=True)


SRUD_CASES = {
    # in_dim == ncols: k = 3 in layer 0, the highway gradient reaches the D input; 2B * ncols = 348 columns (partial 64-column workgroup)
    "srud_bi_k3": _case(3, 19, 20, False, 2, False, ADG, GMLP,
                        dict(in_dim=58, num_hidden=2, hidden_dim=29, bidirectional=True, use_relu=1)),
    # conditioned input (col0 = 20), k = 4 then k = 3, one direction
    "srud_uni_k4_cond": _case(2, 23, 20, True, 2, False, ADAM, GMLP,
                              dict(in_dim=78, num_hidden=3, hidden_dim=16, bidirectional=False, use_relu=0)),
    # both variational sites on three passes; an SRU generator's stash beside the discriminator's
    "srud_bi_dropout": _case(5, 26, 30, True, 2, True, ADAM,
                             dict(kind="SRURNN", in_dim=30, out_dim=187, num_hidden=2, hidden_dim=20, bidirectional=True, dropout=0.2,
                                  last_sigmoid=False, use_relu=1, rnn_dropout=0.2),
                             dict(in_dim=88, num_hidden=3, hidden_dim=12, bidirectional=True, dropout=0.3, rnn_dropout=0.25, use_relu=1)),
    # layer-0 input dropout on the input gradient while the k = 3 highway term by-passes it
    "srud_k3_dropout": _case(3, 19, 20, False, 2, True, ADG, GMLP,
                             dict(in_dim=58, num_hidden=2, hidden_dim=58, bidirectional=False, use_relu=0, dropout=0.3, rnn_dropout=0.25)),
    # several block passes of the cooperative scans with a ragged tail (150 = 2 * 64 + 22 = 4 * 32 + 22)
    "srud_long": _case(2, 150, 20, True, 1, False, ADG, GMLP,
                       dict(in_dim=78, num_hidden=2, hidden_dim=24, bidirectional=True, use_relu=1)),
}


# ---------------------------------------------------------------------------------------------
# drivers
# ---------------------------------------------------------------------------------------------
def run_srud_case(case, philox=False, engine_options=None, seed=None, frame_mask=None, stop_after_d=False):
    """hip_runner.run_hip_case's loop with a discriminator's injected masks cut in thirds (one third per D pass).
    frame_mask: a (B, T) 0/1 array instead of the lengths' mask.  stop_after_d: the first step ends behind update_discriminator and the
    generator's gradient (the leak alone) is flushed; returns its norm under "g_leak_norm_0"."""
    import gantts_amd.train as T
    from gantts_amd import optim, paramgen
    from gantts_amd.engine import engine_for
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model, make_hp
    hp = make_hp(case)
    T.hp = hp
    mg, md = build_model(case["g"], 11), build_model(case["d"], 22)
    if case["dropout_on"]:
        mg.train(), md.train()
    else:
        mg.eval(), md.eval()
    og = getattr(optim, case["opt_g"][0])(mg.parameters(), **case["opt_g"][1])
    od = getattr(optim, case["opt_d"][0])(md.parameters(), **case["opt_d"][1])
    eng = engine_for(hp, mg)
    for k, v in (engine_options or {}).items():
        eng.set_option(k, v)
    if seed is not None:
        eng.set_seed(seed)
    x_np, y_np, lengths = C.make_batch(case)
    x, y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
    Tn = case["T"]
    R = paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, Tn)
    sl = torch.from_numpy(np.ascontiguousarray(lengths)).cuda()
    cpu_lengths = list(lengths)
    out = {}
    for step in range(case["steps"]):
        if case["dropout_on"] and not philox:
            gm, dm = C.make_dropout_masks(case, step)
            assert len(dm) % 3 == 0
            third = len(dm) // 3
            mg.set_dropout_masks(0, [torch.from_numpy(m) for m in gm])
            for p in range(3):
                md.set_dropout_masks(p, [torch.from_numpy(m) for m in dm[p * third:(p + 1) * third]])
        y_static = get_static_features(y, len(hp.windows), hp.stream_sizes, hp.has_dynamic_features)
        if frame_mask is None:
            mask = sequence_mask(sl, max_len=Tn).unsqueeze(-1)
        else:
            mask = torch.from_numpy(np.ascontiguousarray(frame_mask, dtype=np.float32)).cuda().unsqueeze(-1)
        og.zero_grad()
        od.zero_grad()
        y_hat, y_hat_static = T.apply_generator(mg, x, R, cpu_lengths)
        if step == 0:
            out["y_hat"] = y_hat.cpu().numpy()
            out["y_hat_static"] = y_hat_static.cpu().numpy()
        if case["update_d"]:
            res = T.update_discriminator(md, od, x, y_static, y_hat_static, cpu_lengths, mask, "train")
            out["d_scalars_%d" % step] = np.array(res, dtype=np.float64)
            if stop_after_d:
                y_hat_static._gt_engine.flush_generator_grads()
                out["g_leak_norm_0"] = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in mg.parameters())))
                return out
        if case["update_g"]:
            res = T.update_generator(mg, md, og, x, y, y_hat, y_static, y_hat_static, case["adv_w"], cpu_lengths, mask, "train",
                                     mse_w=case["mse_w"], mge_w=case["mge_w"])
            out["g_scalars_%d" % step] = np.array(res, dtype=np.float64)
    torch.cuda.synchronize()
    for k, v in mg.state_dict().items():
        out["G." + k] = v.cpu().numpy()
    for k, v in md.state_dict().items():
        out["D." + k] = v.cpu().numpy()
    for tag, opt, model in (("G", og, mg), ("D", od, md)):
        names = list(model.state_dict().keys())
        for i, st in opt.state_dict()["state"].items():
            for key in ("sum", "exp_avg", "exp_avg_sq"):
                if key in st:
                    out["%s.opt.%s.%s" % (tag, key, names[i])] = st[key].cpu().numpy()
    return out


class _RecordingD(object):
    """An oracle discriminator that keeps every output it returns (the classification margin of the D step is read from them)."""

    def __init__(self, model):
        self.model, self.seen = model, []
        self.params = model.params

    def __call__(self, x, lengths=None, drop=None):
        out = self.model(x, lengths=lengths, drop=drop)
        self.seen.append(out.detach().numpy().copy())
        return out


_ORACLE = {}


def oracle_of(name, case):
    """run_oracle_case (computed once per case and shared, never modified) + "d_margin": the distance from 0.5 of the D-step output
    nearest to it over the valid frames, per step."""
    if name not in _ORACLE:
        import gantts_oracle as O
        from oracle_runner import run_oracle_case
        seen = []
        real_ud = O.update_discriminator

        def recording_ud(cfg, model_d, *a, **kw):
            rec = _RecordingD(model_d)
            res = real_ud(cfg, rec, *a, **kw)
            seen.append(rec.seen)
            return res
        O.update_discriminator = recording_ud
        try:
            ref = run_oracle_case(case)
        finally:
            O.update_discriminator = real_ud
        _, _, lengths = C.make_batch(case)
        valid = (np.arange(case["T"])[None, :] < np.asarray(lengths)[:, None])
        margins = []
        for outs in seen:
            assert len(outs) == 2      # D(real), D(fake)
            margins.append(min(float(np.abs(o[..., 0] - 0.5)[valid].min()) for o in outs))
        ref["d_margin"] = np.asarray(margins)
        for v in ref.values():
            v.setflags(write=False)
        _ORACLE[name] = ref
    return _ORACLE[name]


def _compare(got, ref, tag, counts=True):
    """The rule of test_oracle_only_step_matches_oracle without the LeakyReLU-kink allowance (these cases have far fewer than 1e6
    LeakyReLU activations): _close at the suite's RTOL, _close_state for optimizer state, classification counts exact."""
    from test_gpu_parity import _close, _close_state
    for k, r in ref.items():
        if k.startswith("g_leak_norm") or k == "d_margin":
            continue
        assert k in got, (tag, k)
        msg = "%s %s" % (tag, k)
        if "scalars" in k:
            print("%-50s got %s ref %s" % (msg, np.asarray(got[k]), np.asarray(r)))
            _close(got[k], r, msg=msg)
        elif ".opt." in k:
            _close_state(got[k], r, msg)
        else:
            _close(got[k], r, msg=msg)
    if counts:
        steps = [k for k in ref if k.startswith("d_scalars")]
        if steps:
            print("%s oracle D-step margins to 0.5: %s" % (tag, ref["d_margin"]))
            assert (ref["d_margin"] > 2e-5).all(), (tag, ref["d_margin"])      # else the count comparison below could be vacuous or ill-posed
        for k in steps:
            assert got[k][3] == ref[k][3] and got[k][4] == ref[k][4], (tag, k, got[k], ref[k])


def _run(name, case):
    """Injected-mask cases through the driver above; dropout-off cases through hip_runner.run_hip_case as it is."""
    from hip_runner import run_hip_case
    return run_srud_case(case) if case["dropout_on"] else run_hip_case(case)


# ---------------------------------------------------------------------------------------------
# 1. step parity
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SRUD_CASES))
def test_sru_discriminator_step_matches_oracle(name):
    """Whole G+D steps of every case: outputs, scalars, parameters and optimizer state of both networks at the suite's 1e-4, the
    classification counts exact (the oracle's margin to 0.5 is asserted first)."""
    case = SRUD_CASES[name]
    _compare(_run(name, case), oracle_of(name, case), name)


# ---------------------------------------------------------------------------------------------
# 2. the leak alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["srud_bi_k3", "srud_k3_dropout"])
def test_sru_discriminator_leak_gradient_matches_oracle(name):
    """||G.grad|| right after update_discriminator alone (the un-detached D-loss leak, train.py:265,274): the gradient w.r.t. the generated
    rows' adversarial columns through the SRU stack, k = 3 highway term included (and by-passing layer 0's input dropout)."""
    case = SRUD_CASES[name]
    got = run_srud_case(case, stop_after_d=True)
    ref = float(oracle_of(name, case)["g_leak_norm_0"])
    print("%s leak norm got %.9g ref %.9g" % (name, got["g_leak_norm_0"], ref))
    assert ref > 0
    assert got["g_leak_norm_0"] == pytest.approx(ref, rel=1e-4)


# ---------------------------------------------------------------------------------------------
# 3. partial steps
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", ["g_only", "d_only"])
def test_sru_discriminator_partial_steps_match_oracle(part):
    """update_d=False: the G step alone goes through an un-stepped SRU D (no D-step stash to reuse); update_g=False: the D step alone."""
    case = dict(SRUD_CASES["srud_uni_k4_cond"])
    case["update_d" if part == "g_only" else "update_g"] = False
    name = "srud_uni_k4_cond/" + part
    _compare(_run(name, case), oracle_of(name, case), name)


# ---------------------------------------------------------------------------------------------
# 4. scan families
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["srud_bi_dropout", "srud_long", "srud_bi_k3"])
def test_sru_discriminator_cooperative_scans_match_the_sequential_scans(name):
    """The comparison test_sru_cooperative_block_scans_match_the_sequential_scans makes for the generator, for the discriminator's
    launches (2B sequences in the D step, B in the G step): sequential one-wave scans vs the cooperative block scans with 4 and with 8
    waves per 64 columns."""
    from gantts_amd import _lib as L
    from test_gpu_parity import RTOL, _close
    case = SRUD_CASES[name]
    try:
        L.check(L.lib.gt_set_tuning(b"sru_coop", 0))
        ref = _run(name, case)
        L.check(L.lib.gt_set_tuning(b"sru_coop", 1))
        gots = {}
        for waves in (4, 8):
            L.check(L.lib.gt_set_tuning(b"sru_cs_waves", waves))
            gots[waves] = _run(name, case)
    finally:
        L.check(L.lib.gt_set_tuning(b"sru_coop", 1))
        L.check(L.lib.gt_set_tuning(b"sru_cs_waves", 0))
    for waves, got in gots.items():
        assert set(got) == set(ref)
        for k in ref:
            msg = "%s waves %d %s" % (name, waves, k)
            if "scalars" in k:
                _close(got[k], ref[k], rtol=RTOL, msg=msg)
                if k.startswith("d_scalars"):
                    assert got[k][3] == ref[k][3] and got[k][4] == ref[k][4], msg
            elif ".opt." in k:
                sq = ".opt.sum." in k or ".opt.exp_avg_sq." in k
                _close(np.sqrt(np.maximum(got[k], 0.0)) if sq else got[k], np.sqrt(np.maximum(ref[k], 0.0)) if sq else ref[k], rtol=RTOL, atol=1e-9, msg=msg)
            else:
                _close(got[k], ref[k], rtol=RTOL, msg=msg)


# ---------------------------------------------------------------------------------------------
# 5. Philox
# ---------------------------------------------------------------------------------------------
def test_sru_discriminator_philox_is_reproducible_and_seeded():
    """The engine's own dropout stream: the same seed twice is bit-identical, another seed is not."""
    case = SRUD_CASES["srud_bi_dropout"]
    a = run_srud_case(case, philox=True, seed=1234)
    b = run_srud_case(case, philox=True, seed=1234)
    c = run_srud_case(case, philox=True, seed=4321)
    assert set(a) == set(b) == set(c)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert any(not np.array_equal(a[k], c[k]) for k in a if k.startswith("D."))
    assert not np.array_equal(a["d_scalars_0"], c["d_scalars_0"])


def test_sru_discriminator_train_mode_without_dropout_equals_the_dropout_off_oracle():
    """dropout = rnn_dropout = 0 in both networks, training mode, Philox path: the dropout-off oracle's step -- with the test above
    (which shows that the masks are drawn) the two directions of every site are applied consistently or not at all."""
    case = copy.deepcopy(SRUD_CASES["srud_bi_dropout"])
    for net in ("g", "d"):
        case[net]["dropout"] = 0.0
        case[net]["rnn_dropout"] = 0.0
    name = "srud_bi_dropout/p0"
    off = dict(case, dropout_on=False)
    _compare(run_srud_case(case, philox=True, seed=77), oracle_of(name, off), name)


def _one_frame_probabilities(case):
    """D(fake) at ONE frame from the D step (pass 1) and from the G step (pass 2) of one step with lr = 0 for D: with a single valid
    frame the two losses are -log(1 - p1) and -log(p2) of that frame alone."""
    fm = np.zeros((case["B"], case["T"]), dtype=np.float32)
    fm[0, 3] = 1.0
    got = run_srud_case(case, philox=True, seed=99, frame_mask=fm)
    loss_fake, loss_adv = float(got["d_scalars_0"][1]), float(got["g_scalars_0"][2])
    return -np.expm1(-loss_fake), np.exp(-loss_adv)


def test_sru_discriminator_third_pass_draws_fresh_bits():
    """The G step's D pass (pass 2) against the D step's fake half (pass 1) with D's weights held (lr = 0): without dropout the two
    evaluate the same function of the same rows (control: equal to rounding); with dropout they differ, so pass 2 has its own bits."""
    case = copy.deepcopy(SRUD_CASES["srud_bi_dropout"])
    case["steps"] = 1
    case["opt_d"] = ("Adam", dict(lr=0.0, betas=(0.5, 0.9), weight_decay=0))
    p1, p2 = _one_frame_probabilities(case)
    print("with dropout: D(fake) pass 1 %.8f pass 2 %.8f" % (p1, p2))
    ctrl = copy.deepcopy(case)
    ctrl["d"]["dropout"] = 0.0
    ctrl["d"]["rnn_dropout"] = 0.0
    c1, c2 = _one_frame_probabilities(ctrl)
    print("without dropout: D(fake) pass 1 %.8f pass 2 %.8f" % (c1, c2))
    assert 0.0 < c1 < 1.0 and abs(c1 - c2) < 1e-5 * max(c1, 1 - c1) + 2e-7, (c1, c2)
    assert abs(p1 - p2) > 1e-4, (p1, p2)


# ---------------------------------------------------------------------------------------------
# 6. model_forward
# ---------------------------------------------------------------------------------------------
def test_sru_discriminator_shaped_model_forward_matches_oracle():
    """An eval-mode D-shaped SRURNN (out_dim 1, sigmoid) called as md(x) through the forward-only engine."""
    import gantts_oracle as O
    from hip_runner import build_model
    from oracle_runner import build_oracle_model
    from test_gpu_parity import _close
    spec = SRUD_CASES["srud_bi_k3"]["d"]
    md = build_model(spec, 22).eval()
    mo = build_oracle_model(spec, 22)
    mo.training = False
    x = torch.from_numpy((np.random.RandomState(5).rand(3, 19, 58) * 2 - 1).astype(np.float32))
    with torch.no_grad():
        ref = mo(x).numpy()
    got = md(x.cuda()).cpu().numpy()
    assert got.shape == (3, 19, 1)
    _close(got, ref, msg="SRURNN D forward")
    assert isinstance(mo, O.OracleSRURNN)
    # the same network bound in the DISCRIMINATOR role (gt_model_forward(GT_ROLE_D): what a C caller scoring frames with its D runs)
    from gantts_amd import _lib as L
    from gantts_amd.engine import StepEngine
    eng = StepEngine.for_forward_only(md)
    eng.bind_model(L.ROLE_D, md, with_grads=False)
    xd = x.cuda().contiguous()
    out = torch.empty(3, 19, 1, device="cuda", dtype=torch.float32)
    L.check(L.lib.gt_model_forward(eng._h, L.ROLE_D, L.ptr(xd), None, 3, 19, L.ptr(out), None, L.current_stream()))
    torch.cuda.synchronize()
    _close(out.cpu().numpy(), ref, msg="SRURNN D forward, role D")


# ---------------------------------------------------------------------------------------------
# 7. bf16 option
# ---------------------------------------------------------------------------------------------
def test_sru_discriminator_under_the_bf16_option_tracks_the_float32_oracle():
    """GT_OPT_MATMUL_BF16 with an SRU generator and an SRU discriminator: the discriminator keeps float32 products and stashes, the
    generator's rounding moves the discriminator's inputs.  Bounds of test_bf16_storage_mlp_steps_track_the_float32_oracle: outputs 2e-2
    relative rms, scalars 3e-2, counts within 2 %."""
    from test_gpu_parity import _rms
    name = "srud_bi_dropout"
    case = SRUD_CASES[name]
    got = run_srud_case(case, engine_options={"matmul_bf16": 1})
    ref = oracle_of(name, case)
    for k in ("y_hat", "y_hat_static"):
        err = _rms(got[k] - ref[k]) / _rms(ref[k])
        print("bf16 %s rel-rms %.3e" % (k, err))
        assert err < 2e-2, (k, err)
    assert _rms(got["y_hat"] - ref["y_hat"]) > 0, "suspiciously exact: the bf16 option was not on"
    for st in range(case["steps"]):
        for k, nl in (("d_scalars_%d" % st, 3), ("g_scalars_%d" % st, 4)):
            a, b = np.asarray(got[k]), np.asarray(ref[k])
            print("bf16 %s got %s ref %s" % (k, a, b))
            rel = np.abs(a - b) / np.maximum(np.abs(b), 1e-2)
            assert (rel[:nl] < 3e-2).all(), (k, a, b)
            if k.startswith("d_"):
                assert (np.abs(a[3:] - b[3:]) <= 0.02 * max(1.0, float(case["B"] * case["T"]))).all(), (k, a, b)


# ---------------------------------------------------------------------------------------------
# 8. data parallel
# ---------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_sru_discriminator_world_2_equals_world_1():
    """Two ranks on one device over the RCCL test double (tests/fake_rccl.cpp), two sequences each, Philox on: sequence ids stay global
    in all three D passes (the fake half of the D step continues the count behind the whole minibatch's real half), so both ranks
    reproduce the one-process run -- the comparison of test_gpu_comm2."""
    from hip_runner import run_hip_case
    from test_gpu_comm2 import _check, _run_world2
    case = dict(SRUD_CASES["srud_bi_dropout"], B=4)
    r0, r1 = _run_world2(case, philox=True)      # two child processes, each under the driver's own time limits
    extra = {}
    ref = run_hip_case(case, extra=extra, philox=True)
    _check("srud_bi_dropout/world2", r0, r1, ref)


# ---------------------------------------------------------------------------------------------
# 9. limits
# ---------------------------------------------------------------------------------------------
def _bind_d(md):
    """Binds `md` as the discriminator of a small acoustic configuration (the first call that describes it to the engine)."""
    import gantts_amd.train as T
    from gantts_amd import optim, paramgen
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model, make_hp
    case = SRUD_CASES["srud_bi_k3"]
    T.hp = make_hp(case)
    mg = build_model(case["g"], 11).eval()
    od = optim.Adagrad(md.parameters(), lr=0.01)
    x_np, y_np, lengths = C.make_batch(case)
    x, y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
    R = paramgen.unit_variance_mlpg_matrix_cuda(T.hp.windows, case["T"])
    y_static = get_static_features(y, 3, T.hp.stream_sizes, T.hp.has_dynamic_features)
    mask = sequence_mask(torch.from_numpy(lengths).cuda(), max_len=case["T"]).unsqueeze(-1)
    y_hat, y_hat_static = T.apply_generator(mg, x, R, list(lengths))
    return T.update_discriminator(md, od, x, y_static, y_hat_static, list(lengths), mask, "train")


def test_sru_discriminator_limits_are_refused_by_message():
    from gantts_amd import models
    kw = dict(in_dim=58, out_dim=1, last_sigmoid=True, use_relu=1)
    with pytest.raises(ValueError, match="1024"):
        _bind_d(models.SRURNN(num_hidden=1, hidden_dim=516, bidirectional=True, **kw).cuda().eval())
    with pytest.raises(ValueError, match="at most 8 layers"):
        _bind_d(models.SRURNN(num_hidden=9, hidden_dim=8, bidirectional=False, **kw).cuda().eval())
    with pytest.raises(ValueError, match="last_sigmoid"):
        _bind_d(models.SRURNN(num_hidden=2, hidden_dim=8, bidirectional=False, **dict(kw, last_sigmoid=False)).cuda().eval())
    with pytest.raises(ValueError, match="MLP, LSTMRNN or SRURNN"):
        _bind_d(models.In2OutHighwayNet(in_dim=58, out_dim=58, static_dim=58, num_hidden=2, hidden_dim=16, dropout=0.0).cuda().eval())
    # and what is inside the limits binds and runs
    res = _bind_d(models.SRURNN(num_hidden=8, hidden_dim=8, bidirectional=True, **kw).cuda().eval())
    assert np.isfinite(np.asarray(res, dtype=np.float64)).all()
