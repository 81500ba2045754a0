"""-m gpu: the generator's weight average (gt_set_param_ema; the EMA rider of optim_step_kernel, gantts_amd/csrc/optim_kernels.hip.h) from
the stand-alone hook up to train_loop.

Every comparison is bit for bit and nothing has a tolerance: parameters, gradients, optimizer state and losses are compared with the engine's
own run without the average, and the average with torch's AveragedModel on the CPU (tests/generator_ema_ref.py: ``torch_chain``) fed the
device's own parameter snapshots.  tests/test_generator_ema_host.py shows that this comparator tells the plausible mistakes apart."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import generator_ema_ref as R
import test_gpu_optim_family as F1
import test_gpu_optim_family2 as F2

pytestmark = pytest.mark.gpu

K = R.K_UPDATES
GUARD = 64                       # floats in front of and behind the average buffer
SENTINEL = 12345.0
RULES = [("f1", n) for n in F1.CASES] + [("f2", n) for n in F2.CASES]
# a decay on either lerp branch, alternating over the rules' table; w = 1 and w = 0.5 in a test of their own
BRANCH_DECAYS = (0.999, 0.3)

_inputs = {}


def _make_inputs(n):
    if n not in _inputs:
        _inputs[n] = F1.make_inputs(n, 4000 + n)
    return _inputs[n]


class _Run(object):
    """One chain of updates through the stand-alone hook: the caller's buffers of one optimizer rule (either family's descriptor)."""

    def __init__(self, fam, name, p0):
        self.fam = fam
        self.tname, self.kw = (F1.CASES if fam == "f1" else F2.CASES)[name]
        self.p = p0.cuda()
        self.g = torch.empty_like(self.p)
        if fam == "f1":
            self.states = [None if k is None else torch.zeros_like(self.p) for k in F1.STATE_SLOTS[self.tname](self.kw)]
        else:
            self.states = [torch.zeros_like(self.p) for _ in F2.STATE_KEYS[self.tname]]
            self.h, _ = F2._hyper(self.tname, self.kw)
            if self.tname == "Rprop":
                self.states[1].fill_(self.h["lr"])
            self.scalars = F2._initial_scalars(self.tname, self.kw)

    def step(self, k, gk, ema=None, decay=0.0):
        from gantts_amd import _lib as L
        from gantts_amd.optim_full import host_scalars
        self.g.copy_(gk)
        if self.fam == "f1":
            desc = F1.make_desc(self.tname, self.kw, k, k > 0, self.states)
        else:
            desc = F2.make_desc(self.tname, self.kw, k, self.scalars, self.states)
        if ema is None:
            L.check(L.lib.gt_op_optim_step(C.byref(desc), L.ptr(self.p), L.ptr(self.g), self.p.numel(), None, None, L.current_stream()))
        else:
            L.check(L.lib.gt_op_optim_step_ema(C.byref(desc), L.ptr(self.p), L.ptr(self.g), self.p.numel(), None, None, L.ptr(ema), k,
                                               float(decay), L.current_stream()))
        if self.fam == "f2":
            self.scalars = host_scalars(F2._kind(self.tname), k, k + 1, self.scalars, **self.h)

    def tensors(self):
        return [("param", self.p), ("grad", self.g)] + [("state%d" % i, s) for i, s in enumerate(self.states) if s is not None]


def _guarded(n):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda", dtype=torch.float32)
    ema = buf[GUARD:GUARD + n]
    ema.fill_(7.0)               # never a copy of the parameters here: the first update must not read it
    return buf, ema


def _guards_intact(buf, n):
    g = torch.cat([buf[:GUARD], buf[GUARD + n:]]).cpu().numpy()
    return R.same_bits(g, np.full(2 * GUARD, SENTINEL, dtype=np.float32))


def _hook_chain(fam, name, n, decay):
    """K updates twice, in lockstep: gt_op_optim_step and gt_op_optim_step_ema on the same inputs.  Everything the plain hook writes is
    the same after every update; the average follows torch's chain over the snapshots of the parameters; the guard words stay."""
    p0, gs = _make_inputs(n)
    plain, avg = _Run(fam, name, p0), _Run(fam, name, p0)
    buf, ema = _guarded(n)
    snaps, emas = [], []
    for k in range(K):
        plain.step(k, gs[k])
        avg.step(k, gs[k], ema, decay)
        for (key, a), (_, b) in zip(plain.tensors(), avg.tensors()):
            assert R.same_bits(a.cpu().numpy(), b.cpu().numpy()), "%s n=%d update %d: %s differs with the average on" % (name, n, k + 1, key)
        snaps.append(avg.p.cpu().numpy().copy())
        emas.append(ema.cpu().numpy().copy())
    assert bool(np.isfinite(snaps[-1]).all())
    want = R.torch_chain(snaps, decay)
    for k in range(K):
        assert R.same_bits(emas[k], want[k]), "%s n=%d decay %g update %d: %d of %d elements of the average differ" % (
            name, n, decay, k + 1, R.differing(emas[k], want[k]), n)
    assert _guards_intact(buf, n), "%s n=%d: a guard word of the average buffer was written" % (name, n)


# ------------------------------------------------------------------------------------------
# 1. the hook, every rule of both optimizer-family tables, the kernel frame's three sizes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,name", RULES, ids=[n for _, n in RULES])
def test_hook_average_rides_every_rule(fam, name):
    decay = BRANCH_DECAYS[[n for _, n in RULES].index(name) % 2]
    for n in R.SIZES:
        _hook_chain(fam, name, n, decay)


def test_hook_both_branches_and_every_rule_are_covered():
    assert len(RULES) == len(F1.CASES) + len(F2.CASES) == 17
    ws = [float(R.lerp_weight(d)) for d in BRANCH_DECAYS]
    assert min(ws) < 0.5 <= max(ws) < 1.0


@pytest.mark.parametrize("decay", [0.0, 0.5, 0.25, 0.9, 0.99])
def test_hook_other_decays(decay):
    """w = 1 (every update a copy, through the lerp), the branch boundary w = 0.5, and the rest of the host test's list, on Adagrad."""
    for n in R.SIZES:
        _hook_chain("f1", "adagrad_lr_decay", n, decay)


def test_hook_refusals():
    from gantts_amd import _lib as L
    p0, gs = _make_inputs(4099)
    run = _Run("f1", "sgd", p0)
    run.g.copy_(gs[0])
    desc = F1.make_desc(run.tname, run.kw, 0, False, run.states)
    _, ema = _guarded(4099)
    for args, word in (((None, 0, 0.9), "ema"), ((L.ptr(ema), -1, 0.9), "n_averaged"), ((L.ptr(ema), 0, 1.5), "decay"),
                       ((L.ptr(ema), 0, -0.1), "decay"), ((L.ptr(ema), 0, float("nan")), "decay")):
        rc = L.lib.gt_op_optim_step_ema(C.byref(desc), L.ptr(run.p), L.ptr(run.g), 4099, None, None, args[0], args[1], args[2], L.current_stream())
        assert rc == L.GT_ERR_INVALID and word in L.lib.gt_last_error().decode(), (args[1:], L.lib.gt_last_error())
    torch.cuda.synchronize()
    assert torch.equal(run.p.cpu(), p0)      # refused before any launch


# ------------------------------------------------------------------------------------------
# 3. the engine, every generator architecture
# ------------------------------------------------------------------------------------------
def _case(name):
    import cases as Cs
    return Cs.CASES[name] if name in Cs.CASES else Cs.ORACLE_ONLY_CASES[name]


GENERATORS = {
    "MLP": lambda og, od: F1._mini_case(og, od),
    "In2OutHighwayNet": lambda og, od: dict(_case("vc_in2out"), opt_g=og, opt_d=od),
    "In2OutRNNHighwayNet": lambda og, od: dict(_case("vc_in2out_rnn"), opt_g=og, opt_d=od),
    "LSTMRNN": lambda og, od: dict(_case("acoustic_lstm"), opt_g=og, opt_d=od),
    "SRURNN": lambda og, od: dict(_case("vc_sru_multistream"), opt_g=og, opt_d=od),
}
OPTS = {"adagrad": ("Adagrad", dict(lr=0.01)), "adamw_amsgrad": ("AdamW", dict(lr=1e-3, amsgrad=True))}
DECAY = 0.9


def _step(pair, phase="train", update_g=True):
    """One batch as train_loop runs it -> the scalars both update calls return."""
    c, e = pair.case, pair.eng
    pair.T.hp = pair.hp
    pair.og.zero_grad()
    pair.od.zero_grad()
    y_hat, y_hat_static = e.apply_generator(pair.mg, pair.x, pair.R, pair.lengths)
    out = list(e.update_discriminator(pair.md, pair.od, pair.x, pair.y_static, y_hat_static, pair.mask, phase, lengths=pair.lengths))
    if update_g:
        out += list(e.update_generator(pair.mg, pair.md, pair.og, pair.x, pair.y, y_hat, pair.y_static, y_hat_static, c["adv_w"],
                                       pair.mask, phase, c["mse_w"], c["mge_w"], lengths=pair.lengths))
    torch.cuda.synchronize()
    return np.array(out, dtype=np.float64)


def _same_runs(a, b, what):
    assert R.same_bits(np.float32(a), np.float32(b)) and np.array_equal(a, b, equal_nan=True), "%s: %s != %s" % (what, a, b)


def _same_snapshots(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs" % (what, k)


def _average(model):
    return model._ema.detach().cpu().numpy().copy()


def _params(model):
    return model.flat_params().detach().cpu().numpy().copy()


@pytest.mark.parametrize("opt", list(OPTS))
@pytest.mark.parametrize("gen", list(GENERATORS))
def test_engine_average_for_every_generator(gen, opt):
    case = GENERATORS[gen](OPTS[opt], OPTS[opt])
    assert case["g"]["kind"] == gen and not case["dropout_on"]
    off, on = F1._Pair(case), F1._Pair(case)
    on.mg.enable_weight_average(DECAY)
    assert on.mg.n_averaged == 0 and on.mg.ema_decay == DECAY and R.same_bits(_average(on.mg), _params(on.mg))
    snaps = []
    for k in range(2):
        _same_runs(_step(off), _step(on), "%s step %d scalars" % (gen, k + 1))
        _same_snapshots(off.snapshot(), on.snapshot(), "%s step %d" % (gen, k + 1))
        snaps.append(_params(on.mg))
        assert on.mg.n_averaged == k + 1 == on.eng.param_ema_count()
        assert R.same_bits(_average(on.mg), R.torch_chain(snaps, DECAY)[-1]), "%s: the average after update %d" % (gen, k + 1)
    assert not R.same_bits(_average(on.mg), snaps[-1])      # (a lerp has happened: the average is not the parameters)
    held = _average(on.mg)
    # the test phase and a discriminator-only step (D warm-up: update_g=False) leave average and count alone
    _same_runs(_step(off, "test"), _step(on, "test"), "%s test-phase scalars" % gen)
    _same_runs(_step(off, update_g=False), _step(on, update_g=False), "%s D-only scalars" % gen)
    _same_snapshots(off.snapshot(), on.snapshot(), "%s after the D-only step" % gen)
    assert R.same_bits(_average(on.mg), held) and on.mg.n_averaged == 2 == on.eng.param_ema_count()
    assert on.og._step == 2
    on.eng.check_faults()


# ------------------------------------------------------------------------------------------
# 4. off is off
# ------------------------------------------------------------------------------------------
def test_switched_off_the_buffer_is_no_longer_written():
    from gantts_amd import _lib as L
    case = GENERATORS["MLP"](OPTS["adamw_amsgrad"], OPTS["adamw_amsgrad"])
    off, on = F1._Pair(case), F1._Pair(case)
    on.mg.enable_weight_average(DECAY)
    for _ in range(2):
        _same_runs(_step(off), _step(on), "scalars")
    held, version = _average(on.mg), on.mg._version
    L.check(L.lib.gt_set_param_ema(on.eng._h, L.ROLE_G, None, 0, 0.0))      # behind the model's back: no re-bind sends the buffer again
    _same_runs(_step(off), _step(on), "third step's scalars")
    assert on.mg._version == version
    _same_snapshots(off.snapshot(), on.snapshot(), "third step")
    assert R.same_bits(_average(on.mg), held)
    assert not R.same_bits(_params(on.mg), held)


# ------------------------------------------------------------------------------------------
# 5. the averaged forward
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("gen", ["MLP", "In2OutHighwayNet", "LSTMRNN", "SRURNN"])
def test_forward_inside_averaged_weights(gen, bf16):
    from hip_runner import build_model
    case = GENERATORS[gen](OPTS["adagrad"], OPTS["adagrad"])
    pair = F1._Pair(case)
    pair.mg.enable_weight_average(DECAY)
    for _ in range(2):
        _step(pair)
    params, average = _params(pair.mg), _average(pair.mg)
    plain = build_model(case["g"], 77).eval()
    plain.load_state_dict(pair.mg.ema_state_dict())
    assert list(pair.mg.ema_state_dict().keys()) == list(pair.mg.state_dict().keys())
    assert R.same_bits(_params(plain), average)

    def forward(m):
        if bf16:
            m._own_engine().set_option("matmul_bf16", 1)
        if gen == "In2OutHighwayNet":
            return [t.cpu().numpy() for t in m(pair.x, pair.R)]
        return [(m(pair.x, pair.lengths) if getattr(m, "needs_lengths", False) else m(pair.x)).cpu().numpy()]

    own = forward(pair.mg)                                     # (on the parameters: the shadows of this pass must not survive the swap)
    pair.mg.train()
    with pytest.raises(RuntimeError, match="model.eval"):
        with pair.mg.averaged_weights():
            pass
    pair.mg.eval()
    with pair.mg.averaged_weights():
        inside = forward(pair.mg)
        assert R.same_bits(_params(pair.mg), average)
        assert all(R.same_bits(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(pair.mg.ema_state_dict().values(), plain.state_dict().values()))
        with pytest.raises(RuntimeError, match="averaged_weights"):
            _step(pair)                                        # a train-phase step on the average
    want = forward(plain)
    assert len(inside) == len(want) and all(R.same_bits(a, b) for a, b in zip(inside, want))
    assert not all(R.same_bits(a, b) for a, b in zip(inside, own))
    assert R.same_bits(_params(pair.mg), params) and R.same_bits(_average(pair.mg), average) and pair.mg.n_averaged == 2
    assert all(R.same_bits(a, b) for a, b in zip(forward(pair.mg), own))


# ------------------------------------------------------------------------------------------
# 6. checkpoints
# ------------------------------------------------------------------------------------------
def test_checkpoint_resume_and_cross_loading(tmp_path):
    import gantts_amd.train as T
    opt = OPTS["adamw_amsgrad"]
    case = GENERATORS["MLP"](opt, opt)
    straight = F1._Pair(case)
    straight.mg.enable_weight_average(DECAY)
    for _ in range(4):
        _step(straight)
    first = F1._Pair(case)
    first.mg.enable_weight_average(DECAY)
    for _ in range(2):
        _step(first)
    paths = {tag: T.save_checkpoint(m, o, 2, str(tmp_path), tag) for tag, m, o in (("G", first.mg, first.og), ("D", first.md, first.od))}
    g_ckpt, d_ckpt = (torch.load(paths[t], map_location="cpu") for t in ("G", "D"))
    assert set(g_ckpt) == {"state_dict", "optimizer", "global_epoch", "ema_state_dict", "ema_n_averaged"} and g_ckpt["ema_n_averaged"] == 2
    assert set(d_ckpt) == {"state_dict", "optimizer", "global_epoch"}                      # no average: exactly the three keys
    assert list(g_ckpt["ema_state_dict"]) == list(g_ckpt["state_dict"])
    # both have one: restored, and the run continues as if uninterrupted
    resumed = F1._Pair(case, seeds=(33, 44))
    resumed.mg.enable_weight_average(DECAY)
    assert T.load_checkpoint(resumed.mg, resumed.og, paths["G"]) == 2 and T.load_checkpoint(resumed.md, resumed.od, paths["D"]) == 2
    assert resumed.mg.n_averaged == 2 and R.same_bits(_average(resumed.mg), _average(first.mg))
    for _ in range(2):
        _step(resumed)
    _same_snapshots(straight.snapshot(), resumed.snapshot(), "resumed run")
    assert resumed.mg.n_averaged == 4 == straight.mg.n_averaged
    assert R.same_bits(_average(resumed.mg), _average(straight.mg))
    # a checkpoint with an average into a plain model: ignored
    plain = F1._Pair(case, seeds=(55, 66))
    assert T.load_checkpoint(plain.mg, plain.og, paths["G"]) == 2
    assert plain.mg.ema_decay is None and plain.mg._ema is None and R.same_bits(_params(plain.mg), _params(first.mg))
    # a checkpoint without one into an averaging model: the average restarts from the loaded parameters
    bare = T.save_checkpoint(plain.mg, plain.og, 2, str(tmp_path), "Gplain")
    assert set(torch.load(bare, map_location="cpu")) == {"state_dict", "optimizer", "global_epoch"}
    restart = F1._Pair(case, seeds=(33, 44))
    restart.mg.enable_weight_average(DECAY)
    _step(restart)
    assert restart.mg.n_averaged == 1
    assert T.load_checkpoint(restart.mg, restart.og, bare) == 2 and T.load_checkpoint(restart.md, restart.od, paths["D"]) == 2
    assert restart.mg.n_averaged == 0 and R.same_bits(_average(restart.mg), _params(first.mg))
    _step(restart)
    assert restart.mg.n_averaged == 1 and R.same_bits(_average(restart.mg), _params(restart.mg))      # the first update copies again


# ------------------------------------------------------------------------------------------
# 7. train_loop
# ------------------------------------------------------------------------------------------
def _train_loop_run(tmp_path, ema):
    import cases as Cs
    import gantts_amd.train as T
    from gantts_amd import hparams, optim
    from hip_runner import build_model
    case = dict(Cs.TRAIN_LOOP_CASES["train_loop_acoustic"], batches=dict(train=[(3, 29), (2, 24)], test=[(2, 21)]))
    hp = types.SimpleNamespace(**getattr(hparams, case["hp"]).values())
    hp.stream_sizes, hp.has_dynamic_features = case["stream_sizes"], case["has_dynamic_features"]
    hp.windows = Cs.WINDOWS[:case["windows"]]
    hp.adversarial_streams, hp.mask_nth_mgc_for_adv_loss = case["adversarial_streams"], case["mask_nth_mgc"]
    hp.discriminator_linguistic_condition = case["cond"]
    hp.nepoch, hp.lr_decay_schedule, hp.lr_decay_epoch = 1, False, 10
    hp.generator_add_noise = False
    hp.optimizer_g_params, hp.optimizer_d_params = dict(case["opt_g"][1]), dict(case["opt_d"][1])
    if ema:
        hp.generator_ema_decay, hp.generator_ema_eval = 0.9, True
    mg, md = build_model(case["g"], 11), build_model(case["d"], 22)
    og = getattr(optim, case["opt_g"][0])(mg.parameters(), **case["opt_g"][1])
    od = getattr(optim, case["opt_d"][0])(md.parameters(), **case["opt_d"][1])
    data, mean, std = Cs.make_train_loop_data(case)

    class Loader(list):
        pass

    loaders = {}
    for phase in ("train", "test"):
        ld = Loader((torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(l)) for x, y, l in data[phase])
        ld.dataset = types.SimpleNamespace(Y_data_mean=mean, Y_data_std=std)
        loaders[phase] = ld
    logs = []
    saved = getattr(T, "hp", None), T.global_epoch, T.log_value, T.checkpoint_dir, T.checkpoint_interval
    T.hp, T.global_epoch, T.log_value = hp, 0, lambda n, v, e: logs.append((n, float(v)))
    tmp_path.mkdir(exist_ok=True)
    T.checkpoint_dir, T.checkpoint_interval = str(tmp_path), 1
    try:
        assert T.train_loop((mg, md), (og, od), loaders, w_d=1.0, mse_w=0.0, mge_w=1.0) == 0
        torch.cuda.synchronize()
        mge = None
        if ema:
            # the test batch once more, as the loop stages it, through a PLAIN generator that loaded the checkpoint's average
            from gantts_amd.data import DevicePrefetcher
            from gantts_amd.multistream import get_static_features
            from gantts_amd.paramgen import unit_variance_mlpg_matrix_cuda
            from gantts_amd.seqloss import sequence_mask
            ckpt = torch.load(str(tmp_path / "checkpoint_epoch1_Generator.pth"), map_location="cpu")
            assert ckpt["ema_n_averaged"] == 2 == mg.n_averaged
            plain = build_model(case["g"], 99).eval()
            plain.load_state_dict(ckpt["ema_state_dict"])
            assert R.same_bits(_params(plain), _average(mg)) and not R.same_bits(_params(plain), _params(mg))
            (batch,) = list(DevicePrefetcher(loaders["test"], pitch_x=True))
            Rm = unit_variance_mlpg_matrix_cuda(hp.windows, batch.max_len)
            y_static = get_static_features(batch.y, len(hp.windows), hp.stream_sizes, hp.has_dynamic_features)
            mask = sequence_mask(batch.lengths).unsqueeze(-1)
            md.eval()
            y_hat, y_hat_static = T.apply_generator(plain, batch.x, Rm, batch.cpu_lengths)
            T.update_discriminator(md, od, batch.x, y_static, y_hat_static, batch.cpu_lengths, mask, "test")
            _, mge, _, _ = T.update_generator(plain, md, og, batch.x, batch.y, y_hat, y_static, y_hat_static, 1.0, batch.cpu_lengths, mask,
                                              "test", mse_w=0.0, mge_w=1.0)
    finally:
        T.hp, T.global_epoch, T.log_value, T.checkpoint_dir, T.checkpoint_interval = saved
    return dict(logs), mge, mg


def test_train_loop_switches(tmp_path):
    off, _, mg_off = _train_loop_run(tmp_path / "off", False)
    on, mge, mg_on = _train_loop_run(tmp_path / "on", True)
    assert mg_off.ema_decay is None and mg_on.ema_decay == 0.9 and mg_on.n_averaged == 2
    train_keys = [k for k in off if k.startswith("train ") or k.startswith("E(") or k.startswith("Real train") or k.startswith("Fake train")]
    assert "train mge loss" in train_keys and len(train_keys) >= 8 and sorted(on) == sorted(off)
    for k in train_keys:
        assert off[k] == on[k] or (np.isnan(off[k]) and np.isnan(on[k])), "%s: %r without the average, %r with it" % (k, off[k], on[k])
    assert R.same_bits(_params(mg_off), _params(mg_on))                 # the test phase left the parameters where they were
    assert on["test mge loss"] == float(mge), (on["test mge loss"], mge)
    assert on["test mge loss"] != off["test mge loss"]                  # (the test phase did run on other weights)


# ------------------------------------------------------------------------------------------
# 8. refusals
# ------------------------------------------------------------------------------------------
def test_engine_refusals():
    from gantts_amd import _lib as L
    case = GENERATORS["MLP"](OPTS["adagrad"], OPTS["adagrad"])
    pair = F1._Pair(case)
    _step(pair)                                                         # (binds both networks)
    n = pair.mg.num_flat_params()
    buf = torch.zeros(n + 8, device="cuda")
    h = pair.eng._h

    def refused(role, ema, count, decay, word):
        rc = L.lib.gt_set_param_ema(h, role, L.ptr(ema), count, decay)
        msg = L.lib.gt_last_error().decode()
        assert rc == L.GT_ERR_INVALID and "gt_set_param_ema" in msg and word in msg, (rc, msg)

    refused(L.ROLE_D, buf[:n], n, 0.9, "role")
    for decay in (-0.1, 1.5, float("nan")):
        refused(L.ROLE_G, buf[:n], n, decay, "decay")
    refused(L.ROLE_G, buf[:n + 4], n + 4, 0.9, "n = ")
    refused(L.ROLE_G, buf[:n], 0, 0.9, "n = ")
    refused(L.ROLE_G, None, 0, 0.9, "ema is null")
    cnt = C.c_int64(-1)
    assert L.lib.gt_get_param_ema_count(h, L.ROLE_D, C.byref(cnt)) == L.GT_ERR_INVALID
    assert L.lib.gt_set_param_ema_count(h, L.ROLE_G, -1) == L.GT_ERR_INVALID
    L.check(L.lib.gt_get_param_ema_count(h, L.ROLE_G, C.byref(cnt)))
    assert cnt.value == 0
    # nothing stuck: the next step is the plain one
    before = pair.snapshot()
    ref = F1._Pair(case)
    _step(ref)
    _same_snapshots(before, ref.snapshot(), "after the refusals")
    _same_runs(_step(ref), _step(pair), "a step after the refusals")
    # a wrong n that could not be checked at the call (no generator bound yet) is refused at the step, before any launch
    fresh = F1._Pair(case)
    L.check(L.lib.gt_set_param_ema(fresh.eng._h, L.ROLE_G, L.ptr(buf), n + 8, 0.9))
    held = fresh.mg.flat_params().detach().cpu().clone()
    assert not fresh.eng._ema_on      # (set behind the Python handle's back: its bind does not switch the stray setting off)
    with pytest.raises(ValueError, match="gt_set_param_ema: n = "):
        _step(fresh)
    torch.cuda.synchronize()
    assert torch.equal(held, fresh.mg.flat_params().detach().cpu()) and bool((buf == 0).all())
