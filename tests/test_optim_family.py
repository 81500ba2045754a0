"""CPU checks of the optimizer family of gantts_amd.optim (SGD, RMSprop, Adadelta, AdamW, Adamax, amsgrad): torch.optim's
constructor defaults and errors, its checkpoint layout in both directions, and the re-bind trigger.  The arithmetic runs
on the GPU only: tests/test_gpu_optim_family.py."""
import ctypes as C
import inspect

import pytest
import torch

PLUMBING = ("params", "foreach", "fused", "capturable", "differentiable")

# (our class name, torch class name, keyword arguments, state keys torch keeps after one step)
CASES = [
    ("SGD", "SGD", dict(lr=0.05), ()),
    ("SGD", "SGD", dict(lr=0.05, momentum=0.9, dampening=0.1, weight_decay=1e-4), ("momentum_buffer",)),
    ("SGD", "SGD", dict(lr=0.05, momentum=0.9, nesterov=True), ("momentum_buffer",)),
    ("RMSprop", "RMSprop", dict(lr=0.01), ("step", "square_avg")),
    ("RMSprop", "RMSprop", dict(lr=0.01, alpha=0.9, momentum=0.9, centered=True, weight_decay=1e-5),
     ("step", "square_avg", "momentum_buffer", "grad_avg")),
    ("Adadelta", "Adadelta", dict(lr=1.0, rho=0.95, weight_decay=1e-5), ("step", "square_avg", "acc_delta")),
    ("AdamW", "AdamW", dict(lr=1e-3, betas=(0.5, 0.9)), ("step", "exp_avg", "exp_avg_sq")),
    ("AdamW", "AdamW", dict(lr=1e-3, amsgrad=True), ("step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")),
    ("Adam", "Adam", dict(lr=1e-3, amsgrad=True), ("step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")),
    ("Adam", "Adam", dict(lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True), ("step", "exp_avg", "exp_avg_sq")),
    ("Adamax", "Adamax", dict(lr=2e-3, weight_decay=1e-5), ("step", "exp_avg", "exp_inf")),
]
IDS = ["sgd", "sgd-momentum-dampening-wd", "sgd-nesterov", "rmsprop", "rmsprop-momentum-centered-wd", "adadelta", "adamw",
       "adamw-amsgrad", "adam-amsgrad", "adam-decoupled", "adamax"]


def _mlp():
    from gantts_amd import models
    return models.MLP(in_dim=6, out_dim=2, num_hidden=1, hidden_dim=4, last_sigmoid=False)


def _torch_after_one_step(tname, kw):
    ref = torch.nn.Sequential(torch.nn.Linear(6, 4), torch.nn.Linear(4, 2))
    t = getattr(torch.optim, tname)(ref.parameters(), **kw)
    torch.manual_seed(3)
    ref(torch.randn(5, 6)).pow(2).sum().backward()
    t.step()
    return ref, t


@pytest.mark.parametrize("name,tname,kw,keys", CASES, ids=IDS)
def test_state_dict_round_trip_with_torch(name, tname, kw, keys):
    from gantts_amd import optim
    m = _mlp()
    o = getattr(optim, name)(m.parameters(), **kw)
    sd = o.state_dict()
    ref, t = _torch_after_one_step(tname, kw)
    tsd = t.state_dict()
    assert sd["state"] == {}                                   # torch creates the state on the first step
    assert sd["param_groups"][0]["params"] == tsd["param_groups"][0]["params"]
    for k in kw:
        assert sd["param_groups"][0][k] == kw[k]
    for k in sd["param_groups"][0]:                            # nothing torch does not know
        assert k in tsd["param_groups"][0], k
    assert sorted(tsd["state"][0]) == sorted(keys) if keys else tsd["state"] == {}
    getattr(torch.optim, tname)(ref.parameters(), **kw).load_state_dict(sd)      # torch accepts our checkpoint format
    o2 = getattr(optim, name)(m.parameters())
    o2.load_state_dict(tsd)                                    # and we accept torch's, state included
    assert o2.param_groups[0]["lr"] == kw["lr"]
    sd2 = o2.state_dict()
    assert sorted(sd2["state"]) == sorted(tsd["state"])
    for i, st in tsd["state"].items():
        assert sorted(sd2["state"][i]) == sorted(st)
        for k, v in st.items():
            assert torch.equal(torch.as_tensor(sd2["state"][i][k]).float().reshape(-1), torch.as_tensor(v).float().reshape(-1)), k
    t2 = getattr(torch.optim, tname)(ref.parameters(), **kw)
    t2.load_state_dict(sd2)                                    # a populated checkpoint of ours goes back into torch
    for i, st in tsd["state"].items():
        for k, v in st.items():
            assert torch.equal(torch.as_tensor(t2.state_dict()["state"][i][k]), torch.as_tensor(v))
    with pytest.raises(RuntimeError):
        o.step()


@pytest.mark.parametrize("name,tname,kw,keys", [c for c in CASES if c[3]], ids=[i for i, c in zip(IDS, CASES) if c[3]])
def test_loading_a_checkpoint_without_state_empties_a_populated_optimizer(name, tname, kw, keys):
    """torch's load_state_dict REPLACES the state: a checkpoint written before the first step, loaded into an optimizer that has stepped
    (resume into live objects), leaves no state and step 0 -- not the old moments under the old step count."""
    from gantts_amd import optim
    m = _mlp()
    empty = getattr(optim, name)(m.parameters(), **kw).state_dict()
    assert empty["state"] == {}
    _, t = _torch_after_one_step(tname, kw)
    o = getattr(optim, name)(m.parameters())
    o.load_state_dict(t.state_dict())
    assert o.state_dict()["state"] != {} and o._version > 0
    version = o._version
    o.load_state_dict(empty)
    assert o.state_dict()["state"] == {} and o._step == 0 and o._step0 == 0 and not o._live()
    assert all(s is None for s in o._state) and o._version > version        # buffers are made anew (zeros) at the next bind, engines re-bind
    t.load_state_dict(empty)
    assert t.state_dict()["state"] == {}                                     # (torch does the same)


@pytest.mark.parametrize("name", ["SGD", "RMSprop", "Adadelta", "AdamW", "Adamax", "Adam", "Adagrad"])
def test_constructor_defaults_match_torch(name):
    from gantts_amd import optim
    ours = inspect.signature(getattr(optim, name).__init__).parameters
    theirs = inspect.signature(getattr(torch.optim, name).__init__).parameters
    arithmetic = [k for k in theirs if k not in PLUMBING and k != "self"]
    assert arithmetic
    for k in arithmetic:
        assert k in ours, "%s lacks %s" % (name, k)
        assert ours[k].default == theirs[k].default, (name, k)
    for k in PLUMBING[1:]:
        assert k not in ours                                   # the plumbing keywords stay unaccepted
    # the leading arguments can be passed by position in torch's order
    lead = [k for k in theirs if theirs[k].kind == inspect.Parameter.POSITIONAL_OR_KEYWORD and k in ours
            and ours[k].kind == inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert [k for k in ours if k in lead] == lead
    m = _mlp()
    o = getattr(optim, name)(m.parameters())
    for k in arithmetic:
        if k != "maximize":
            assert o.param_groups[0][k] == theirs[k].default, (name, k)


INVALID = [
    ("SGD", dict(lr=-1.0)), ("SGD", dict(momentum=-0.1)), ("SGD", dict(weight_decay=-1.0)),
    ("SGD", dict(nesterov=True)), ("SGD", dict(nesterov=True, momentum=0.9, dampening=0.1)),
    ("RMSprop", dict(lr=-1.0)), ("RMSprop", dict(eps=-1.0)), ("RMSprop", dict(momentum=-0.1)),
    ("RMSprop", dict(weight_decay=-1.0)), ("RMSprop", dict(alpha=-0.1)),
    ("Adadelta", dict(lr=-1.0)), ("Adadelta", dict(rho=1.5)), ("Adadelta", dict(rho=-0.1)), ("Adadelta", dict(eps=-1.0)),
    ("Adadelta", dict(weight_decay=-1.0)),
    ("AdamW", dict(lr=-1.0)), ("AdamW", dict(eps=-1.0)), ("AdamW", dict(betas=(1.0, 0.9))), ("AdamW", dict(betas=(0.9, 1.0))),
    ("AdamW", dict(weight_decay=-1.0)),
    ("Adam", dict(betas=(-0.1, 0.9), amsgrad=True)),
    ("Adamax", dict(lr=-1.0)), ("Adamax", dict(eps=-1.0)), ("Adamax", dict(betas=(1.0, 0.9))), ("Adamax", dict(betas=(0.9, -0.1))),
    ("Adamax", dict(weight_decay=-1.0)),
]


@pytest.mark.parametrize("name,kw", INVALID, ids=["%s-%s" % (n, "-".join("%s=%s" % kv for kv in sorted(k.items()))) for n, k in INVALID])
def test_invalid_values_raise_where_torch_raises(name, kw):
    from gantts_amd import optim
    with pytest.raises(ValueError):
        getattr(torch.optim, name)(torch.nn.Linear(2, 2).parameters(), **kw)
    with pytest.raises(ValueError):
        getattr(optim, name)(_mlp().parameters(), **kw)


@pytest.mark.parametrize("name", ["SGD", "RMSprop", "Adadelta", "AdamW", "Adamax", "Adam"])
def test_maximize_is_rejected_and_plumbing_is_not_accepted(name):
    from gantts_amd import optim
    with pytest.raises(ValueError):
        getattr(optim, name)(_mlp().parameters(), maximize=True)
    for k in PLUMBING[1:]:
        with pytest.raises(TypeError):
            getattr(optim, name)(_mlp().parameters(), **{k: False})


def test_other_torch_names_stay_absent():
    from gantts_amd import optim
    for n in ("NAdam", "RAdam", "Rprop", "ASGD", "LBFGS"):
        assert not hasattr(optim, n)


def test_editing_a_hyper_parameter_changes_the_bind_key():
    from gantts_amd import optim
    m = _mlp()
    for name, kw, key, new in (("SGD", dict(momentum=0.9), "momentum", 0.5), ("SGD", dict(momentum=0.9), "dampening", 0.1),
                               ("SGD", dict(momentum=0.9), "nesterov", True),
                               ("RMSprop", {}, "alpha", 0.9), ("RMSprop", {}, "momentum", 0.9), ("RMSprop", {}, "centered", True),
                               ("Adadelta", {}, "rho", 0.5), ("AdamW", {}, "betas", (0.5, 0.9)), ("AdamW", {}, "amsgrad", True),
                               ("Adamax", {}, "betas", (0.9, 0.9)), ("Adamax", {}, "eps", 1e-6)):
        o = getattr(optim, name)(m.parameters(), **kw)
        before = o._hyper()
        o.param_groups[0][key] = new
        after = o._hyper()
        assert after[1:] != before[1:], (name, key)            # StepEngine.bind_optimizer re-binds
        o.param_groups[0]["lr"] = 0.123
        assert o._hyper()[1:] == after[1:] and o._hyper()[0] == 0.123      # lr alone: the gt_set_lr path


def test_descriptor_layout_and_validation():
    from gantts_amd import _lib as L
    assert C.sizeof(L.OptimDescEx) == 120 and L.OptimDescEx.lr.offset == 8 and L.OptimDescEx.alpha.offset == 72
    assert L.OptimDescEx.step.offset == 88 and L.OptimDescEx.state2.offset == 112
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)

    def rc(**kw):
        d = L.OptimDescEx()
        d.lr, d.max_grad_norm = 0.01, 1.0
        for k, v in kw.items():
            setattr(d, k, v)
        # validation comes before any device work: no GPU is needed to be told what is wrong
        return L.lib.gt_op_optim_step(C.byref(d), p, p, 4, None, None, None), L.lib.gt_last_error()

    for bad in (dict(kind=7), dict(kind=L.OPT_SGD, flags=L.OPTF_NESTEROV),
                dict(kind=L.OPT_SGD, flags=L.OPTF_NESTEROV, momentum=0.9, dampening=0.1, state0=p),
                dict(kind=L.OPT_SGD, momentum=0.9), dict(kind=L.OPT_SGD, flags=L.OPTF_CENTERED),
                dict(kind=L.OPT_RMSPROP, state0=p, momentum=0.9), dict(kind=L.OPT_RMSPROP, state0=p, flags=L.OPTF_CENTERED),
                dict(kind=L.OPT_RMSPROP, state0=p, alpha=-1.0), dict(kind=L.OPT_ADADELTA, state0=p),
                dict(kind=L.OPT_ADADELTA, state0=p, state1=p, alpha=1.5),
                dict(kind=L.OPT_ADAMW, state0=p, state1=p, beta1=1.0),
                dict(kind=L.OPT_ADAM, state0=p, state1=p, beta1=0.9, beta2=0.999, flags=L.OPTF_AMSGRAD),
                dict(kind=L.OPT_ADAMAX, state0=p, beta1=0.9, beta2=0.999), dict(kind=L.OPT_ADAMAX, state0=p, state1=p, lr=-1.0)):
        code, msg = rc(**bad)
        assert code == L.GT_ERR_INVALID and msg, bad
