"""torch.optim's first-order family -- ``Adagrad``, ``Adam`` (``amsgrad``, ``decoupled_weight_decay``), ``AdamW``, ``SGD``,
``RMSprop``, ``Adadelta``, ``Adamax`` -- with torch.optim's constructor signatures, ``param_groups`` and ``state_dict``
layout (reference train.py:796-799 builds them with
``getattr(optim, hp.optimizer_g)(model.parameters(), **hp.optimizer_g_params)``; checkpoints
store ``optimizer.state_dict()``, train.py:162-171).

The update itself is the fused clip-norm + optimizer HIP kernel over the network's flat
parameter buffer (one launch per network, executed inside ``update_discriminator`` /
``update_generator`` exactly where the reference calls ``clip_grad_norm_`` + ``step()``,
train.py:275-276, 317-318).  State lives in flat float32 device buffers owned here; the 0-dim float32 state tensors torch
keeps beside ``step`` (NAdam ``mu_product``, ASGD ``eta`` and ``mu``) are host values that the engine advances with its step
counter (``gt_get_optimizer_scalars``).  ``NAdam``, ``RAdam``, ``Rprop`` and ``ASGD`` are in ``gantts_amd.optim_full``, which has
every name of this module as well.  Not covered: ``LBFGS``, ``maximize``, more than one parameter group.
"""
import torch

from . import _lib as L


def _owner_of(params):
    params = list(params)
    if not params:
        raise ValueError("optimizer got an empty parameter list")
    if isinstance(params[0], dict):
        if len(params) != 1:
            raise ValueError("gantts_amd optimizers support a single param group")
        params = list(params[0]["params"])
    owners = {id(getattr(p, "_gt_owner", lambda: None)()) for p in params}
    owner = getattr(params[0], "_gt_owner", lambda: None)()
    if owner is None or len(owners) != 1:
        raise TypeError("gantts_amd.optim optimizers take model.parameters() of ONE gantts_amd network")
    if len(params) != len(list(owner.parameters())):
        raise ValueError("pass all parameters of the network (the update runs over its flat buffer)")
    return owner, params


class _FlatOptimizer(object):
    KIND = None
    STATE_KEYS = ()
    SCALAR_KEYS = ()      # 0-dim float32 state tensors of torch's class, in state_dict order behind "step": host values here
    LR_REBINDS = False    # a changed lr re-binds (the kind keeps lr as a double) instead of taking gt_set_lr
    HAS_STEP = True       # torch keeps a "step" entry in the per-parameter state (every class but SGD)

    def __init__(self, params, defaults):
        self.model, self._params = _owner_of(params)
        self.defaults = dict(defaults)
        group = dict(defaults)
        group["params"] = list(range(len(self._params)))
        self.param_groups = [group]
        self._state = [None, None, None]
        self._step = 0
        self._step0 = 0               # step count at construction / load_state_dict
        self._scalars = [0.0, 0.0]    # values of SCALAR_KEYS after self._step updates (set by _desc_ex / _note_step / load_state_dict)
        self._live0 = False           # SGD: a loaded checkpoint carried momentum_buffer
        self._version = 0
        self._engines = {}
        self.max_grad_norm = 1.0      # clip_grad_norm_(params, 1.0), train.py:275,317

    # -- flat state -------------------------------------------------------------------------
    def _slots(self):
        """State buffer index (state0..2 of the descriptor) of every key of ``STATE_KEYS``."""
        return list(range(len(self.STATE_KEYS)))

    def _ensure_state(self):
        flat = self.model.flat_params()
        for i in self._slots():
            st = self._state[i]
            if st is None:
                self._state[i] = torch.zeros_like(flat)
                self._version += 1
            elif st.device != flat.device:
                self._state[i] = st.to(flat.device)
                self._version += 1

    def _hyper(self):
        """(lr, everything else the fused update kernel reads) -- compared by StepEngine.bind_optimizer on every step."""
        g = self.param_groups[0]
        b1, b2 = g.get("betas", (0.0, 0.0))
        return (float(g["lr"]), float(g.get("weight_decay", 0.0)), float(g.get("eps", 0.0)), float(g.get("lr_decay", 0.0)),
                float(b1), float(b2), float(self.max_grad_norm),
                float(g.get("momentum", 0.0)), float(g.get("dampening", 0.0)), bool(g.get("nesterov", False)),
                float(g.get("alpha", g.get("rho", 0.0))), bool(g.get("centered", False)), bool(g.get("amsgrad", False)),
                bool(g.get("decoupled_weight_decay", False)), float(g.get("momentum_decay", 0.0)),
                tuple(float(v) for v in g.get("etas", ())), tuple(float(v) for v in g.get("step_sizes", ())),
                float(g.get("lambd", 0.0)), float(g.get("t0", 0.0)), float(g["lr"]) if self.LR_REBINDS else 0.0)

    def _initial_scalars(self):
        return [0.0, 0.0]

    def _note_step(self, engine, role):
        self._step = engine.optimizer_step_count(role)
        if self.SCALAR_KEYS:
            self._scalars = list(engine.optimizer_scalars(role))

    # -- torch.optim API --------------------------------------------------------------------
    def zero_grad(self, set_to_none=True):
        """Marks the gradients as cleared (the next backward overwrites them) and drops the
        pending D-loss -> G gradient, like ``optimizer_g.zero_grad()`` at train.py:538."""
        for key, (ref, role) in list(self.model._bound_engines.items()):
            eng = ref()
            if eng is None:
                del self.model._bound_engines[key]
            else:
                eng.zero_grad(role)

    def step(self, closure=None):
        raise RuntimeError("gantts_amd optimizers step inside update_discriminator/update_generator "
                           "(fused clip-norm + update kernel); a separate step() would apply the update twice")

    def _views(self, flat):
        out, off = [], 0
        for p in self._params:
            n = p.numel()
            out.append(flat[off:off + n].view(p.shape))
            off += n
        return out

    def _has_state(self):
        """torch creates the per-parameter state on the first step() (Adagrad: at construction)."""
        return self._step > 0

    def _live(self):
        """SGD's "momentum_buffer holds a value": a step was taken since construction / load, or the loaded checkpoint had it."""
        return self._live0 or self._step > self._step0

    def _desc_ex(self, kind, flags=0, momentum=0.0, dampening=0.0, alpha=0.0, **more):
        self._ensure_state()
        g = self.param_groups[0]
        d = L.OptimDescEx2() if more else L.OptimDescEx()      # the kinds of gantts_amd.optim_full carry the descriptor's tail
        d.kind, d.flags = kind, flags
        d.lr = float(g["lr"])
        d.weight_decay = float(g.get("weight_decay", 0.0))
        d.eps = float(g.get("eps", 0.0))
        d.lr_decay = float(g.get("lr_decay", 0.0))
        b1, b2 = g.get("betas", (0.0, 0.0))
        d.beta1, d.beta2 = float(b1), float(b2)
        d.momentum, d.dampening, d.alpha = float(momentum), float(dampening), float(alpha)
        d.max_grad_norm = float(self.max_grad_norm)
        d.step = int(self._step)
        if not self._has_state():      # torch creates them on the first step(), from the group's lr of that moment
            self._scalars = self._initial_scalars()
        if more:                       # the tail fields of the four last kinds, and the host scalar state
            d.host_state0, d.host_state1 = float(self._scalars[0]), float(self._scalars[1])
            for k, v in more.items():
                setattr(d, k, float(v))
        slots = self._slots()
        for k in range(3):
            setattr(d, "state%d" % k, self._state[k].data_ptr() if k in slots else None)
        return d

    def state_dict(self):
        state = {}
        if self.KIND == L.OPT_ADAGRAD:
            self._ensure_state()      # torch.optim.Adagrad creates "sum" at construction
        keys, slots = self.STATE_KEYS, self._slots()
        if self._has_state() and all(self._state[k] is not None for k in slots):
            views = [self._views(self._state[k]) for k in slots]
            for i in range(len(self._params)):
                st = {"step": torch.tensor(float(self._step))} if self.HAS_STEP else {}
                for k, key in enumerate(self.SCALAR_KEYS):
                    st[key] = torch.tensor(self._scalars[k], dtype=torch.float32)
                for k, key in enumerate(keys):
                    st[key] = views[k][i].clone()
                state[i] = st
        return {"state": state, "param_groups": [dict(g) for g in self.param_groups]}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self._params):
            raise ValueError("loaded state dict has a different number of parameter groups / parameters")
        g = dict(groups[0])
        g["params"] = list(range(len(self._params)))
        self.param_groups = [g]
        state = sd.get("state", {})
        self._live0 = False
        if state:
            self._ensure_state()
            keys, slots = self.STATE_KEYS, self._slots()
            views = [self._views(self._state[k]) for k in slots]
            steps, scalars = set(), set()
            for i in range(len(self._params)):
                st = state[i]
                if self.HAS_STEP:
                    steps.add(int(float(st["step"])))
                scalars.add(tuple(float(torch.as_tensor(st[key], dtype=torch.float32)) for key in self.SCALAR_KEYS))
                for k, key in enumerate(keys):
                    views[k][i].copy_(st[key])
            if self.HAS_STEP:
                if len(steps) != 1:
                    raise ValueError("per-parameter step counts differ; not a checkpoint of this optimizer")
                self._step = steps.pop()
            if self.SCALAR_KEYS:
                if len(scalars) != 1:
                    raise ValueError("per-parameter %s differ; not a checkpoint of this optimizer" % " / ".join(self.SCALAR_KEYS))
                self._scalars = (list(scalars.pop()) + [0.0])[:2]
            self._live0 = len(keys) > 0
        else:
            # torch replaces the state by the loaded one: an optimizer that has stepped goes back to "no state yet" -- step 0, and
            # buffers that _ensure_state() makes anew at the next bind, as after construction
            self._state = [None, None, None]
            self._step = 0
            self._scalars = self._initial_scalars()
        self._step0 = self._step
        self._version += 1


class Adagrad(_FlatOptimizer):
    """p -= lr/(1+(t-1)*lr_decay) * g / (sqrt(sum g^2) + eps)   (torch.optim.Adagrad semantics)."""
    KIND = L.OPT_ADAGRAD
    STATE_KEYS = ("sum",)

    def __init__(self, params, lr=1e-2, lr_decay=0, weight_decay=0, initial_accumulator_value=0, eps=1e-10, *, maximize=False):
        _reject(maximize)
        if lr < 0 or lr_decay < 0 or weight_decay < 0 or eps < 0:
            raise ValueError("invalid Adagrad hyper-parameter")
        super(Adagrad, self).__init__(params, dict(lr=lr, lr_decay=lr_decay, eps=eps, weight_decay=weight_decay,
                                                   initial_accumulator_value=initial_accumulator_value))
        self._init_acc = float(initial_accumulator_value)

    def _has_state(self):
        return True

    def _ensure_state(self):
        fresh = self._state[0] is None
        super(Adagrad, self)._ensure_state()
        if fresh and self._init_acc != 0.0:
            self._state[0].fill_(self._init_acc)

    def _desc(self):
        return self._desc_ex(L.OPT_ADAGRAD)


def _reject(maximize):
    if maximize:
        raise ValueError("maximize is not supported")


def _check_betas(betas):
    if not 0.0 <= betas[0] < 1.0:
        raise ValueError("Invalid beta parameter at index 0: %s" % (betas[0],))
    if not 0.0 <= betas[1] < 1.0:
        raise ValueError("Invalid beta parameter at index 1: %s" % (betas[1],))


class Adam(_FlatOptimizer):
    """torch.optim.Adam semantics (bias-corrected; ``amsgrad`` keeps ``max_exp_avg_sq``; ``decoupled_weight_decay`` is AdamW)."""
    KIND = L.OPT_ADAM

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 decoupled_weight_decay=False):
        _reject(maximize)
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameter")
        super(Adam, self).__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                                                amsgrad=bool(amsgrad), decoupled_weight_decay=bool(decoupled_weight_decay)))

    @property
    def STATE_KEYS(self):
        return ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if self.param_groups[0].get("amsgrad") else ())

    def _desc(self):
        g = self.param_groups[0]
        dec = bool(g.get("decoupled_weight_decay"))
        return self._desc_ex(L.OPT_ADAMW if dec else L.OPT_ADAM, L.OPTF_AMSGRAD if g.get("amsgrad") else 0)


class AdamW(Adam):
    """torch.optim.AdamW: ``param *= 1 - lr * weight_decay``, then Adam without weight decay."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False):
        super(AdamW, self).__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize, decoupled_weight_decay=True)


class SGD(_FlatOptimizer):
    """torch.optim.SGD semantics (momentum, dampening, nesterov, weight_decay)."""
    KIND = L.OPT_SGD
    HAS_STEP = False

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False):
        _reject(maximize)
        if lr < 0.0:
            raise ValueError("Invalid learning rate: %s" % (lr,))
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: %s" % (momentum,))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: %s" % (weight_decay,))
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super(SGD, self).__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                               nesterov=bool(nesterov)))

    @property
    def STATE_KEYS(self):
        return ("momentum_buffer",) if self.param_groups[0]["momentum"] != 0 else ()

    def _has_state(self):
        return self._live()

    def _desc(self):
        g = self.param_groups[0]
        flags = (L.OPTF_NESTEROV if g["nesterov"] else 0) | (L.OPTF_BUFFER_LIVE if self._live() else 0)
        return self._desc_ex(L.OPT_SGD, flags, momentum=g["momentum"], dampening=g["dampening"])


class RMSprop(_FlatOptimizer):
    """torch.optim.RMSprop semantics (alpha, momentum, centered)."""
    KIND = L.OPT_RMSPROP

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, *, maximize=False):
        _reject(maximize)
        if lr < 0.0:
            raise ValueError("Invalid learning rate: %s" % (lr,))
        if eps < 0.0:
            raise ValueError("Invalid epsilon value: %s" % (eps,))
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: %s" % (momentum,))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: %s" % (weight_decay,))
        if alpha < 0.0:
            raise ValueError("Invalid alpha value: %s" % (alpha,))
        super(RMSprop, self).__init__(params, dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=bool(centered),
                                                   weight_decay=weight_decay))

    @property
    def STATE_KEYS(self):
        g = self.param_groups[0]
        return ("square_avg",) + (("momentum_buffer",) if g["momentum"] > 0 else ()) + (("grad_avg",) if g["centered"] else ())

    def _slots(self):
        g = self.param_groups[0]
        return [0] + ([1] if g["momentum"] > 0 else []) + ([2] if g["centered"] else [])

    def _desc(self):
        g = self.param_groups[0]
        return self._desc_ex(L.OPT_RMSPROP, L.OPTF_CENTERED if g["centered"] else 0, momentum=max(float(g["momentum"]), 0.0),
                             alpha=g["alpha"])


class Adadelta(_FlatOptimizer):
    """torch.optim.Adadelta semantics (rho, eps, lr)."""
    KIND = L.OPT_ADADELTA
    STATE_KEYS = ("square_avg", "acc_delta")

    def __init__(self, params, lr=1.0, rho=0.9, eps=1e-6, weight_decay=0, *, maximize=False):
        _reject(maximize)
        if lr < 0.0:
            raise ValueError("Invalid learning rate: %s" % (lr,))
        if not 0.0 <= rho <= 1.0:
            raise ValueError("Invalid rho value: %s" % (rho,))
        if eps < 0.0:
            raise ValueError("Invalid epsilon value: %s" % (eps,))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: %s" % (weight_decay,))
        super(Adadelta, self).__init__(params, dict(lr=lr, rho=rho, eps=eps, weight_decay=weight_decay))

    def _desc(self):
        return self._desc_ex(L.OPT_ADADELTA, alpha=self.param_groups[0]["rho"])


class Adamax(_FlatOptimizer):
    """torch.optim.Adamax semantics (exponentially weighted infinity norm)."""
    KIND = L.OPT_ADAMAX
    STATE_KEYS = ("exp_avg", "exp_inf")

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, maximize=False):
        _reject(maximize)
        if lr < 0.0:
            raise ValueError("Invalid learning rate: %s" % (lr,))
        if eps < 0.0:
            raise ValueError("Invalid epsilon value: %s" % (eps,))
        _check_betas(betas)
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: %s" % (weight_decay,))
        super(Adamax, self).__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))

    def _desc(self):
        return self._desc_ex(L.OPT_ADAMAX)
