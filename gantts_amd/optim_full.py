"""The whole first-order list of torch.optim as a drop-in: every name of ``gantts_amd.optim`` (``Adagrad``, ``Adam``, ``AdamW``,
``SGD``, ``RMSprop``, ``Adadelta``, ``Adamax``) and ``NAdam``, ``RAdam``, ``Rprop``, ``ASGD``.

    from gantts_amd import optim_full as optim
    optimizer_g = getattr(optim, hp.optimizer_g)(model_g.parameters(), **hp.optimizer_g_params)      # reference train.py:796-799

``gantts_amd.optim`` itself keeps the seven names it has (its tests pin that list); the four classes here use the same base
class, the same fused clip + update launch and the same checkpoint layout.  The 0-dim float32 state tensors torch keeps beside
``step`` (NAdam ``mu_product``, ASGD ``eta`` and ``mu``) are host values that the engine advances with its step counter.
Not covered: ``LBFGS`` (a closure and a line search), ``maximize``, more than one parameter group.
"""
import ctypes as C

import torch

from . import _lib as L
from .optim import SGD, Adadelta, Adagrad, Adam, Adamax, AdamW, RMSprop      # noqa: F401 -- re-exported: the drop-in's other names
from .optim import _check_betas, _FlatOptimizer, _reject

__all__ = ["Adagrad", "Adam", "AdamW", "SGD", "RMSprop", "Adadelta", "Adamax", "NAdam", "RAdam", "Rprop", "ASGD", "host_scalars"]


def host_scalars(kind, step, t, scalars, **hyper):
    """The host scalar state of ``kind`` after ``t`` updates, given ``scalars`` as they stand after ``step <= t`` updates
    (``gt_op_optim_scalars``: the library's own routine, no device needed).  ``hyper``: fields of ``OptimDescEx`` (``lr``, ``beta1``,
    ``momentum_decay``; ``lr``, ``lambd``, ``alpha``, ``t0``).  NAdam: (mu_product, 0); ASGD: (eta, mu)."""
    d = L.OptimDescEx2()
    d.kind, d.step = kind, int(step)
    d.host_state0, d.host_state1 = float(scalars[0]), float(scalars[1])
    for k, v in hyper.items():
        setattr(d, k, float(v))
    out = (C.c_double * 2)()
    L.check(L.lib.gt_op_optim_scalars(C.byref(d), int(t), out))
    return out[0], out[1]


def _decoupled_flag(g):
    return L.OPTF_DECOUPLED_WD if g.get("decoupled_weight_decay") else 0


class NAdam(_FlatOptimizer):
    """torch.optim.NAdam semantics (Nesterov momentum with the mu_t schedule; ``mu_product`` is a float32 running product)."""
    KIND = L.OPT_NADAM
    STATE_KEYS = ("exp_avg", "exp_avg_sq")
    SCALAR_KEYS = ("mu_product",)

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, momentum_decay=4e-3,
                 decoupled_weight_decay=False, *, maximize=False):
        _reject(maximize)
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %s" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %s" % (eps,))
        _check_betas(betas)
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %s" % (weight_decay,))
        if not 0.0 <= momentum_decay:
            raise ValueError("Invalid momentum_decay value: %s" % (momentum_decay,))
        super(NAdam, self).__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                                                 momentum_decay=momentum_decay, decoupled_weight_decay=bool(decoupled_weight_decay)))

    def _initial_scalars(self):
        return [1.0, 0.0]

    def _desc(self):
        g = self.param_groups[0]
        return self._desc_ex(L.OPT_NADAM, _decoupled_flag(g), momentum_decay=g["momentum_decay"])


class RAdam(_FlatOptimizer):
    """torch.optim.RAdam semantics (the variance rectification is on from the step at which rho_t exceeds 5)."""
    KIND = L.OPT_RADAM
    STATE_KEYS = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, decoupled_weight_decay=False, *,
                 maximize=False):
        _reject(maximize)
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %s" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %s" % (eps,))
        _check_betas(betas)
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %s" % (weight_decay,))
        super(RAdam, self).__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                                                 decoupled_weight_decay=bool(decoupled_weight_decay)))

    def _desc(self):
        return self._desc_ex(L.OPT_RADAM, _decoupled_flag(self.param_groups[0]))


class Rprop(_FlatOptimizer):
    """torch.optim.Rprop semantics.  ``lr`` is only the value ``step_size`` is filled with when the state is created (the
    first update, or a ``load_state_dict``); writing ``param_groups[0]["lr"]`` later changes nothing, as in torch."""
    KIND = L.OPT_RPROP
    STATE_KEYS = ("prev", "step_size")

    def __init__(self, params, lr=1e-2, etas=(0.5, 1.2), step_sizes=(1e-6, 50), *, maximize=False):
        _reject(maximize)
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %s" % (lr,))
        if not 0.0 < etas[0] < 1.0 < etas[1]:
            raise ValueError("Invalid eta values: %s, %s" % (etas[0], etas[1]))
        super(Rprop, self).__init__(params, dict(lr=lr, etas=tuple(etas), step_sizes=tuple(step_sizes)))

    def _ensure_state(self):
        fresh = self._state[1] is None
        super(Rprop, self)._ensure_state()
        if fresh:
            self._state[1].fill_(float(self.param_groups[0]["lr"]))      # torch.full_like(grad, lr) at the state's creation

    def _desc(self):
        g = self.param_groups[0]
        return self._desc_ex(L.OPT_RPROP, etaminus=g["etas"][0], etaplus=g["etas"][1], step_size_min=g["step_sizes"][0],
                             step_size_max=g["step_sizes"][1])


class ASGD(_FlatOptimizer):
    """torch.optim.ASGD semantics (``ax`` is the running average; ``eta`` and ``mu`` are float32 scalars re-derived every step)."""
    KIND = L.OPT_ASGD
    STATE_KEYS = ("ax",)
    SCALAR_KEYS = ("eta", "mu")
    LR_REBINDS = True     # eta is a float32 rounding of a double expression in lr: lr must reach the engine unrounded

    def __init__(self, params, lr=1e-2, lambd=1e-4, alpha=0.75, t0=1e6, weight_decay=0, foreach=None, maximize=False):
        _reject(maximize)
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %s" % (lr,))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %s" % (weight_decay,))
        super(ASGD, self).__init__(params, dict(lr=lr, lambd=lambd, alpha=alpha, t0=t0, weight_decay=weight_decay))

    def _initial_scalars(self):
        return [float(torch.tensor(float(self.param_groups[0]["lr"]), dtype=torch.float32)), 1.0]      # eta = float32(lr), mu = 1

    def _desc(self):
        g = self.param_groups[0]
        return self._desc_ex(L.OPT_ASGD, alpha=g["alpha"], lambd=g["lambd"], t0=g["t0"])
