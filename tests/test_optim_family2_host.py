"""CPU checks of the second optimizer family, gantts_amd.optim_full (NAdam, RAdam, Rprop, ASGD beside the names of gantts_amd.optim): torch.optim's constructor
signatures, defaults and error texts, its checkpoint layout in both directions, the re-bind trigger, the descriptor's
validation, and the host scalar state -- NAdam's float32 running product ``mu_product`` and ASGD's ``eta`` / ``mu`` -- against
torch's own 0-dim float32 state tensors, through the library's routine (``gt_op_optim_scalars``: no device needed).  The
element-wise arithmetic runs on the GPU only: tests/test_gpu_optim_family2.py."""
import ctypes as C
import inspect

import pytest
import torch

PLUMBING = ("params", "foreach", "fused", "capturable", "differentiable")
NAMES = ("NAdam", "RAdam", "Rprop", "ASGD")

# (class name, keyword arguments, state keys torch keeps after one step, in torch's order)
CASES = [
    ("NAdam", dict(lr=2e-3, momentum_decay=1e-2, weight_decay=1e-5), ("step", "mu_product", "exp_avg", "exp_avg_sq")),
    ("NAdam", dict(lr=2e-3, weight_decay=1e-2, decoupled_weight_decay=True), ("step", "mu_product", "exp_avg", "exp_avg_sq")),
    ("RAdam", dict(lr=1e-3), ("step", "exp_avg", "exp_avg_sq")),
    ("RAdam", dict(lr=1e-3, betas=(0.5, 0.9), weight_decay=1e-4, decoupled_weight_decay=True), ("step", "exp_avg", "exp_avg_sq")),
    ("Rprop", dict(lr=0.02, etas=(0.3, 1.5), step_sizes=(1e-4, 0.05)), ("step", "prev", "step_size")),
    ("ASGD", dict(lr=0.01, t0=4, lambd=1e-3, weight_decay=1e-5), ("step", "eta", "mu", "ax")),
]
IDS = ["nadam", "nadam-decoupled", "radam", "radam-decoupled", "rprop", "asgd"]


def _mlp():
    from gantts_amd import models
    return models.MLP(in_dim=6, out_dim=2, num_hidden=1, hidden_dim=4, last_sigmoid=False)


def _torch_after_steps(tname, kw, steps=1):
    ref = torch.nn.Sequential(torch.nn.Linear(6, 4), torch.nn.Linear(4, 2))
    t = getattr(torch.optim, tname)(ref.parameters(), foreach=False, **kw)
    torch.manual_seed(3)
    for _ in range(steps):
        t.zero_grad()
        ref(torch.randn(5, 6)).pow(2).sum().backward()
        t.step()
    return ref, t


def test_every_first_order_name_resolves_and_lbfgs_does_not():
    from gantts_amd import optim as first
    from gantts_amd import optim_full as optim
    for n in NAMES:
        assert getattr(optim, n).__name__ == n and issubclass(getattr(optim, n), first._FlatOptimizer)
    for n in ("Adagrad", "Adam", "AdamW", "SGD", "RMSprop", "Adadelta", "Adamax"):      # the drop-in has the first family's names too
        assert getattr(optim, n) is getattr(first, n)
    assert not hasattr(optim, "LBFGS")


@pytest.mark.parametrize("name,kw,keys", CASES, ids=IDS)
def test_state_dict_round_trip_with_torch(name, kw, keys):
    """Keys (and their order), dtypes and shapes of state_dict() equal those of the torch class stepped three times on tensors of the
    same shapes; torch's checkpoint loads and comes back out unchanged, the 0-dim float32 scalars included; ours loads into torch."""
    from gantts_amd import optim_full as optim
    m = _mlp()
    o = getattr(optim, name)(m.parameters(), **kw)
    sd = o.state_dict()
    ref, t = _torch_after_steps(name, kw, steps=3)
    tsd = t.state_dict()
    assert sd["state"] == {}                                   # torch creates the state on the first step
    assert sd["param_groups"][0]["params"] == tsd["param_groups"][0]["params"]
    for k in kw:
        assert sd["param_groups"][0][k] == kw[k]
    for k in sd["param_groups"][0]:                            # nothing torch does not know
        assert k in tsd["param_groups"][0], k
    assert tuple(tsd["state"][0]) == keys
    getattr(torch.optim, name)(ref.parameters(), **kw).load_state_dict(sd)      # torch accepts our (empty) checkpoint
    o2 = getattr(optim, name)(m.parameters())
    o2.load_state_dict(tsd)
    assert o2.param_groups[0]["lr"] == kw["lr"] and o2._step == 3
    sd2 = o2.state_dict()
    assert sorted(sd2["state"]) == sorted(tsd["state"])
    shapes = [p.shape for p in m.parameters()]
    assert shapes == [p.shape for p in ref.parameters()]
    for i, st in tsd["state"].items():
        assert tuple(sd2["state"][i]) == keys                   # torch's key order
        for k, v in st.items():
            ours = sd2["state"][i][k]
            assert torch.is_tensor(ours) and ours.dtype == v.dtype == torch.float32, k
            assert ours.shape == v.shape and (ours.shape == shapes[i] or ours.dim() == 0), k
            assert torch.equal(ours.cpu(), v), k
    t2 = getattr(torch.optim, name)(ref.parameters(), foreach=False, **kw)
    t2.load_state_dict(sd2)                                     # a populated checkpoint of ours goes back into torch
    for i, st in tsd["state"].items():
        for k, v in st.items():
            assert torch.equal(torch.as_tensor(t2.state_dict()["state"][i][k]).cpu(), v)
    with pytest.raises(RuntimeError):
        o.step()


def test_never_bound_optimizer_reports_initial_then_loaded_scalars():
    from gantts_amd import optim_full as optim
    m = _mlp()
    o = optim.NAdam(m.parameters())
    assert o.state_dict()["state"] == {} and o._step == 0
    _, t = _torch_after_steps("NAdam", dict(momentum_decay=1e-2), steps=5)
    o.load_state_dict(t.state_dict())
    want = float(t.state_dict()["state"][0]["mu_product"])
    assert want < 1.0 and float(o.state_dict()["state"][0]["mu_product"]) == want == o._scalars[0]
    a = optim.ASGD(m.parameters(), lr=0.03)
    # (the descriptor itself needs device buffers; the scalars it would carry at step 0 do not)
    assert a._initial_scalars() == [float(torch.tensor(0.03, dtype=torch.float32)), 1.0]
    a.param_groups[0]["lr"] = 0.5      # torch forms eta from the group's lr at the FIRST step
    assert a._initial_scalars() == [0.5, 1.0]
    _, ta = _torch_after_steps("ASGD", dict(lr=0.01, t0=1, lambd=1e-3), steps=4)
    a.load_state_dict(ta.state_dict())
    st = ta.state_dict()["state"][0]
    assert a._scalars == [float(st["eta"]), float(st["mu"])] and float(st["mu"]) != 1.0
    # a checkpoint whose parameters disagree on a scalar is not one of this optimizer
    bad = ta.state_dict()
    bad["state"][1]["mu"] = torch.tensor(0.125)
    with pytest.raises(ValueError, match="differ"):
        optim.ASGD(m.parameters()).load_state_dict(bad)


@pytest.mark.parametrize("name", NAMES)
def test_constructor_signature_and_defaults_match_torch(name):
    from gantts_amd import optim_full as optim
    ours = inspect.signature(getattr(optim, name).__init__).parameters
    theirs = inspect.signature(getattr(torch.optim, name).__init__).parameters
    arithmetic = [k for k in theirs if k not in PLUMBING and k != "self"]
    assert arithmetic
    for k in arithmetic:
        assert k in ours, "%s lacks %s" % (name, k)
        assert ours[k].default == theirs[k].default, (name, k)
    for k in ours:                                             # nothing torch does not take
        assert k in theirs, k
    # the leading arithmetic arguments can be passed by position in torch's order
    lead = [k for k in theirs if theirs[k].kind == inspect.Parameter.POSITIONAL_OR_KEYWORD and k in arithmetic and k != "maximize"]
    assert [k for k in ours if k in lead] == lead
    for k in lead:
        assert ours[k].kind == inspect.Parameter.POSITIONAL_OR_KEYWORD
    m = _mlp()
    o = getattr(optim, name)(m.parameters())
    for k in arithmetic:
        if k != "maximize":
            assert o.param_groups[0][k] == theirs[k].default, (name, k)
    with pytest.raises(ValueError):
        getattr(optim, name)(m.parameters(), maximize=True)
    getattr(optim, name)(m.parameters(), maximize=False)


INVALID = [
    ("NAdam", dict(lr=-1.0)), ("NAdam", dict(eps=-1.0)), ("NAdam", dict(betas=(1.0, 0.9))), ("NAdam", dict(betas=(0.9, -0.1))),
    ("NAdam", dict(weight_decay=-1.0)), ("NAdam", dict(momentum_decay=-1.0)),
    ("RAdam", dict(lr=-1.0)), ("RAdam", dict(eps=-1.0)), ("RAdam", dict(betas=(-0.5, 0.9))), ("RAdam", dict(betas=(0.9, 1.0))),
    ("RAdam", dict(weight_decay=-1.0)),
    ("Rprop", dict(lr=-1.0)), ("Rprop", dict(etas=(0.0, 1.2))), ("Rprop", dict(etas=(1.0, 1.2))), ("Rprop", dict(etas=(0.5, 1.0))),
    ("Rprop", dict(etas=(1.2, 0.5))),
    ("ASGD", dict(lr=-1.0)), ("ASGD", dict(weight_decay=-1.0)),
]


@pytest.mark.parametrize("name,kw", INVALID, ids=["%s-%s" % (n, "-".join("%s=%s" % kv for kv in sorted(k.items()))) for n, k in INVALID])
def test_invalid_values_raise_torchs_error(name, kw):
    from gantts_amd import optim_full as optim
    with pytest.raises(ValueError) as theirs:
        getattr(torch.optim, name)(torch.nn.Linear(2, 2).parameters(), **kw)
    with pytest.raises(ValueError) as ours:
        getattr(optim, name)(_mlp().parameters(), **kw)
    assert str(ours.value) == str(theirs.value)


def test_editing_a_hyper_parameter_changes_the_bind_key():
    from gantts_amd import optim_full as optim
    m = _mlp()
    for name, key, new in (("NAdam", "momentum_decay", 1e-2), ("NAdam", "decoupled_weight_decay", True), ("NAdam", "betas", (0.5, 0.9)),
                           ("NAdam", "weight_decay", 0.1), ("RAdam", "decoupled_weight_decay", True), ("RAdam", "eps", 1e-6),
                           ("Rprop", "etas", (0.3, 1.5)), ("Rprop", "step_sizes", (1e-4, 0.05)),
                           ("ASGD", "lambd", 1e-3), ("ASGD", "alpha", 0.5), ("ASGD", "t0", 4), ("ASGD", "weight_decay", 1e-5)):
        o = getattr(optim, name)(m.parameters())
        before = o._hyper()
        o.param_groups[0][key] = new
        after = o._hyper()
        assert after[1:] != before[1:], (name, key)            # StepEngine.bind_optimizer re-binds
        o.param_groups[0]["lr"] = 0.123
        if name != "ASGD":      # (Rprop reads no lr after the fill of step_size: gt_set_lr is as good as anything)
            assert o._hyper()[1:] == after[1:] and o._hyper()[0] == 0.123      # lr alone: the gt_set_lr path
        else:
            assert o._hyper()[1:] != after[1:]      # ASGD keeps lr as a double: a re-bind, not gt_set_lr's float


def test_descriptor_growth_and_validation():
    from gantts_amd import _lib as L
    D = L.OptimDescEx2
    # every field of the first family keeps its offset; the new ones follow state2
    assert (D.kind.offset, D.flags.offset, D.lr.offset, D.alpha.offset, D.max_grad_norm.offset, D.step.offset) == (0, 4, 8, 72, 80, 88)
    assert (D.state0.offset, D.state1.offset, D.state2.offset) == (96, 104, 112)
    names = ("momentum_decay", "etaminus", "etaplus", "step_size_min", "step_size_max", "lambd", "t0", "host_state0", "host_state1")
    assert [getattr(D, n).offset for n in names] == [120 + 8 * i for i in range(9)] and C.sizeof(D) == 192
    assert issubclass(D, L.OptimDescEx) and C.sizeof(L.OptimDescEx) == 120      # the head alone: all the first family's kinds are read for
    assert (L.OPT_NADAM, L.OPT_RADAM, L.OPT_RPROP, L.OPT_ASGD) == (7, 8, 9, 10)
    assert L.OPTF_DECOUPLED_WD not in (L.OPTF_NESTEROV, L.OPTF_CENTERED, L.OPTF_AMSGRAD, L.OPTF_BUFFER_LIVE, 16)
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    good = {
        L.OPT_NADAM: dict(kind=L.OPT_NADAM, state0=p, state1=p, beta1=0.9, beta2=0.999, host_state0=1.0),
        L.OPT_RADAM: dict(kind=L.OPT_RADAM, state0=p, state1=p, beta1=0.9, beta2=0.999),
        L.OPT_RPROP: dict(kind=L.OPT_RPROP, state0=p, state1=p, etaminus=0.5, etaplus=1.2, step_size_min=1e-6, step_size_max=50.0),
        L.OPT_ASGD: dict(kind=L.OPT_ASGD, state0=p, host_state0=0.01, host_state1=1.0),
    }

    def rc(base, **kw):
        d = D()
        d.lr, d.max_grad_norm = 0.01, 1.0
        for k, v in dict(base, **kw).items():
            setattr(d, k, v)
        # validation comes before any device work: no GPU is needed to be told what is wrong
        return L.lib.gt_op_optim_step(C.byref(d), p, p, 4, None, None, None), L.lib.gt_last_error().decode()

    N, R, P, A = (good[k] for k in (L.OPT_NADAM, L.OPT_RADAM, L.OPT_RPROP, L.OPT_ASGD))
    for base, kw, text in (
            ({}, dict(kind=11), "unknown optimizer kind"),
            (N, dict(momentum_decay=-1.0), "Invalid momentum_decay value"), (N, dict(beta1=1.0), "Invalid beta parameter at index 0"),
            (N, dict(beta2=-0.1), "Invalid beta parameter at index 1"), (N, dict(eps=-1.0), "Invalid epsilon value"),
            (N, dict(weight_decay=-1.0), "Invalid weight_decay value"), (N, dict(lr=-1.0), "Invalid learning rate"),
            (N, dict(state1=None), "state buffer is null"), (N, dict(host_state0=0.5), "mu_product"), (N, dict(host_state0=1.5, step=3), "mu_product"), (N, dict(host_state0=-0.1, step=3), "mu_product"),
            (N, dict(flags=L.OPTF_AMSGRAD), "do not belong"),
            (R, dict(beta2=1.0), "Invalid beta parameter at index 1"), (R, dict(state0=None), "state buffer is null"),
            (R, dict(flags=L.OPTF_NESTEROV), "do not belong"),
            (P, dict(etaminus=0.0), "Invalid eta values"), (P, dict(etaminus=1.0), "Invalid eta values"), (P, dict(etaplus=1.0), "Invalid eta values"),
            (P, dict(state1=None), "state buffer is null"), (P, dict(flags=L.OPTF_DECOUPLED_WD), "do not belong"),
            (A, dict(weight_decay=-1.0), "Invalid weight_decay value"), (A, dict(state0=None), "state buffer is null"),
            (A, dict(host_state1=0.0), "mu"), (A, dict(flags=L.OPTF_DECOUPLED_WD), "do not belong")):
        code, msg = rc(base, **kw)
        assert code == L.GT_ERR_INVALID and text in msg, (kw, msg)
    # the decoupled flag belongs to NAdam and RAdam only
    for k in (L.OPT_ADAM, L.OPT_ADAMW, L.OPT_ADAMAX, L.OPT_SGD, L.OPT_RMSPROP, L.OPT_ADADELTA, L.OPT_ADAGRAD):
        code, msg = rc(dict(kind=k, state0=p, state1=p, state2=p, beta1=0.9, beta2=0.999, flags=L.OPTF_DECOUPLED_WD))
        assert code == L.GT_ERR_INVALID and "do not belong" in msg, k


def test_nadam_mu_product_underflows_to_zero_as_in_torch_and_binds_from_there():
    """The float32 running product of factors near 0.45 is exactly 0.0 after some 135 updates; torch goes on with 1 - 0 = 1.  The
    library's product equals torch's through the denormal range and at 0, a descriptor that carries 0 (a checkpoint of a long run, a
    re-bind after a param_groups edit) is valid, and the scalars derived from it stay 0."""
    from gantts_amd import _lib as L
    from gantts_amd.optim_full import host_scalars
    p = torch.zeros(3, requires_grad=True)
    t = torch.optim.NAdam([p], foreach=False)
    hyper = dict(lr=2e-3, beta1=0.9, beta2=0.999, momentum_decay=4e-3)
    carried, denormal = (1.0, 0.0), 0
    for k in range(1, 201):
        p.grad = torch.ones(3)
        t.step()
        carried = host_scalars(L.OPT_NADAM, k - 1, k, carried, **hyper)
        assert carried[0] == float(t.state[p]["mu_product"]), k
        denormal += 0.0 < carried[0] < 1.1754944e-38
    assert carried[0] == 0.0 and denormal > 0 and bool(torch.isfinite(p).all())
    assert host_scalars(L.OPT_NADAM, 0, 200, (1.0, 0.0), **hyper) == (0.0, 0.0)
    assert host_scalars(L.OPT_NADAM, 200, 201, (0.0, 0.0), **hyper) == (0.0, 0.0)      # bound at step 200 with mu_product = 0
    # gt_op_optim_scalars applies every check of gt_bind_optimizer_ex but the one of the state buffers: 0 is valid, what torch cannot hold is not
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="mu_product"):
            host_scalars(L.OPT_NADAM, 200, 201, (bad, 0.0), **hyper)
    # a checkpoint of that run loads, and the class then carries 0 into its descriptor
    from gantts_amd import optim_full as optim
    m = _mlp()
    ref, tt = _torch_after_steps("NAdam", {}, steps=200)
    o = optim.NAdam(m.parameters())
    o.load_state_dict(tt.state_dict())
    assert o._step == 200 and o._scalars[0] == 0.0 == float(tt.state_dict()["state"][0]["mu_product"])


STEPS = 50


@pytest.mark.parametrize("kw", [dict(), dict(momentum_decay=1e-2), dict(betas=(0.5, 0.9), momentum_decay=0.3)], ids=["default", "decay1e-2", "beta0.5"])
def test_nadam_mu_product_is_torchs_float32_state_exactly(kw):
    """50 steps of torch.optim.NAdam; after each, the library's mu_product -- carried step by step, re-derived in one call from the
    start, and re-derived from a mid-run bind -- equals the 0-dim float32 tensor torch keeps, bit for bit."""
    from gantts_amd import _lib as L
    from gantts_amd.optim_full import host_scalars
    p = torch.zeros(3, requires_grad=True)
    t = torch.optim.NAdam([p], foreach=False, **kw)
    hyper = dict(lr=2e-3, beta1=kw.get("betas", (0.9, 0.999))[0], beta2=kw.get("betas", (0.9, 0.999))[1],
                 momentum_decay=kw.get("momentum_decay", 4e-3))
    carried, mid = (1.0, 0.0), None
    for k in range(1, STEPS + 1):
        p.grad = torch.ones(3)
        t.step()
        want = t.state[p]["mu_product"]
        assert want.dtype == torch.float32 and want.dim() == 0
        carried = host_scalars(L.OPT_NADAM, k - 1, k, carried, **hyper)
        assert carried == (float(want), 0.0), k
        assert host_scalars(L.OPT_NADAM, 0, k, (1.0, 0.0), **hyper) == carried, k
        if k == 17:
            mid = carried
        if mid is not None:
            assert host_scalars(L.OPT_NADAM, 17, k, mid, **hyper) == carried, k
    assert 0.0 < carried[0] < 1e-3      # the product has moved far from 1


@pytest.mark.parametrize("kw", [dict(), dict(lr=0.01, t0=4, lambd=1e-3), dict(lr=0.3, t0=0, lambd=0.5, alpha=0.9)],
                         ids=["default", "t0=4", "large"])
def test_asgd_eta_and_mu_are_torchs_float32_state_exactly(kw):
    from gantts_amd import _lib as L
    from gantts_amd.optim_full import host_scalars
    p = torch.zeros(3, requires_grad=True)
    t = torch.optim.ASGD([p], foreach=False, **kw)
    d = dict(lr=1e-2, lambd=1e-4, alpha=0.75, t0=1e6)
    d.update(kw)
    start = (float(torch.tensor(d["lr"], dtype=torch.float32)), 1.0)
    averaged = 0
    for k in range(1, STEPS + 1):
        p.grad = torch.ones(3)
        t.step()
        st = t.state[p]
        assert st["eta"].dtype == st["mu"].dtype == torch.float32
        got = host_scalars(L.OPT_ASGD, 0, k, start, **d)
        assert got == (float(st["eta"]), float(st["mu"])), k
        assert host_scalars(L.OPT_ASGD, k, k, got, **d) == got      # at the bound step: the bind values themselves
        averaged += got[1] != 1.0
    assert averaged > 0 or "t0" not in kw
    assert host_scalars(L.OPT_ASGD, 0, 0, start, **d) == start


def test_scalars_of_the_other_kinds_are_zero_and_bad_calls_are_reported():
    from gantts_amd import _lib as L
    from gantts_amd.optim_full import host_scalars
    assert host_scalars(L.OPT_RADAM, 0, 5, (0.0, 0.0), lr=1e-3, beta1=0.9, beta2=0.999) == (0.0, 0.0)
    assert host_scalars(L.OPT_ADAMW, 3, 5, (0.0, 0.0), lr=1e-3) == (0.0, 0.0)
    with pytest.raises(ValueError):
        host_scalars(L.OPT_NADAM, 5, 4, (0.5, 0.0), lr=1e-3, beta1=0.9)      # before the descriptor's step
    with pytest.raises(ValueError):
        host_scalars(11, 0, 1, (0.0, 0.0))
