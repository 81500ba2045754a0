"""-m gpu: gt_bind_optimizer, the C ABI's first bind entry (gt_optim_desc: Adagrad and Adam, float hyper-parameters).  The Python
classes bind through gt_bind_optimizer_ex; a caller of the first entry must get the same update, bit for bit."""
import ctypes as C

import pytest
import torch

from test_gpu_optim_family import _Pair, _mini_case

pytestmark = pytest.mark.gpu

OPTS = {
    "adagrad": ("Adagrad", dict(lr=1e-2, lr_decay=1e-3, weight_decay=1e-4)),
    "adam": ("Adam", dict(lr=1e-3, betas=(0.8, 0.99), weight_decay=1e-4)),
}


def _bind_through_the_first_entry(pair):
    """Replaces the engine's bind of `pair` by gt_bind_optimizer with a hand-built gt_optim_desc (once per optimizer: nothing here
    edits a hyper-parameter between the steps)."""
    from gantts_amd import _lib as L
    eng, calls = pair.eng, []

    def bind(role, opt):
        if any(o is opt for _, o in calls):
            return
        opt._ensure_state()
        g = opt.param_groups[0]
        d = L.OptimDesc()
        d.kind = opt.KIND
        d.lr, d.weight_decay, d.eps, d.lr_decay = g["lr"], g["weight_decay"], g["eps"], g.get("lr_decay", 0.0)
        d.beta1, d.beta2 = g.get("betas", (0.0, 0.0))
        d.max_grad_norm = opt.max_grad_norm
        d.step = opt._step
        d.state0 = opt._state[0].data_ptr()
        d.state1 = opt._state[1].data_ptr() if len(opt.STATE_KEYS) > 1 else None
        L.check(L.lib.gt_bind_optimizer(eng._h, role, C.byref(d)))
        calls.append((role, opt))

    eng.bind_optimizer = bind
    return calls


@pytest.mark.parametrize("name", list(OPTS))
def test_the_first_bind_entry_updates_like_the_python_path(name):
    case = _mini_case(OPTS[name], OPTS[name])
    normal, first = _Pair(case), _Pair(case)
    calls = _bind_through_the_first_entry(first)
    for _ in range(2):
        normal.step()
        first.step()
    assert sorted(role for role, _ in calls) == [0, 1] and {id(o) for _, o in calls} == {id(first.og), id(first.od)}
    assert first.og._step == 2 and first.od._step == 2
    a, b = normal.snapshot(), first.snapshot()
    assert sorted(a) == sorted(b) and len(a) == 2 * (1 + len(normal.og.STATE_KEYS))
    for k in a:
        assert bool(a[k].abs().sum() > 0) and torch.equal(a[k], b[k]), "%s: %s differs (max |d| %.3e)" % (name, k, float((a[k] - b[k]).abs().max()))
