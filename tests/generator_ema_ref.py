"""Reference of the generator's weight average (gt_set_param_ema; the EMA rider of optim_step_kernel, gantts_amd/csrc/optim_kernels.hip.h).

The DEFINITION is torch's: ``AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay))`` with ``update_parameters(model)`` called once after
every applied update (``torch_chain``).  ``numpy_chain`` restates it operation by operation -- the first update copies; every later one is
``ema.lerp_(p, w)`` with ``w = float32(1.0 - decay)`` (the subtraction in double), which this torch build's CPU path evaluates as ONE fused
multiply-add per element, ``fmaf(w, p - ema, ema)`` for ``w < 0.5`` and ``fmaf(-(1 - w), p - ema, p)`` otherwise -- and takes the seeded
mistakes of tests/test_generator_ema_host.py as switches.  Comparisons are bit for bit (``same_bits``): nothing here has a tolerance."""
import numpy as np
import torch

K_UPDATES = 12
SIZES = (1, 4099, 839355)      # tests/test_gpu_optim_family.py's: one element, the predicated tail, the cfg2 generator (several grid strides)


def same_bits(a, b):
    """The comparator: two float32 arrays are the same iff every element has the same 32 bits (-0.0 is not 0.0; a NaN equals itself)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def differing(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def fma32(a, b, c):
    """fmaf(a, b, c) of float32 operands, correctly rounded: the product is exact in float64; the sum is rounded to ODD in float64 (its
    error from TwoSum), which makes the second rounding, 53 -> 24 bits, the only one."""
    a64, b64, c64 = np.broadcast_arrays(*[np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c)])
    prod = a64 * b64
    s = prod + c64
    bb = s - prod
    err = (prod - (s - bb)) + (c64 - bb)
    bits = np.ascontiguousarray(s).view(np.int64)
    inexact = err != 0
    bits = np.where(inexact & ((err < 0) != (s < 0)), bits - 1, bits)      # truncate the exact sum towards zero ...
    bits = np.where(inexact, bits | 1, bits)                                 # ... and keep what was cut off as a sticky last bit
    return np.ascontiguousarray(bits).view(np.float64).astype(np.float32)


def lerp_weight(decay):
    return np.float32(1.0 - float(decay))


def lerp32(ema, p, w, fused=True):
    """Tensor.lerp_(p, w) on float32: fused (what torch computes) or with the product and the sum rounded separately (a seeded mistake)."""
    ema, p, w = np.asarray(ema, np.float32), np.asarray(p, np.float32), np.float32(w)
    d = p - ema
    if w < np.float32(0.5):
        return fma32(w, d, ema) if fused else (ema + w * d).astype(np.float32)
    omw = np.float32(1.0) - w
    return fma32(-omw, d, p) if fused else (p - d * omw).astype(np.float32)


def numpy_chain(stored, decay, initial=None, mistake=None, before=None, raw=None):
    """The average after each of the updates whose stored parameters are ``stored[0], stored[1], ...`` -> list of float32 arrays.
    ``initial``: the buffer before the first update (a copy of the parameters; read by the mistake "no_copy" only).  Mistakes:
    "no_copy" (lerp from ``initial`` at the first update), "two_roundings", "w_from_float_decay" (w = 1 - float32(decay)),
    "before_update" (averages ``before[k]``, the parameters ahead of update k), "before_clamp" (averages ``raw[k]``, the rule's value ahead
    of the clamp)."""
    w = np.float32(1.0) - np.float32(decay) if mistake == "w_from_float_decay" else lerp_weight(decay)
    src = {"before_update": before, "before_clamp": raw}.get(mistake, stored)
    ema = None if initial is None else np.asarray(initial, np.float32).copy()
    out = []
    for k, p in enumerate(src):
        p = np.asarray(p, np.float32)
        if k == 0 and mistake != "no_copy":
            ema = p.copy()
        else:
            ema = lerp32(ema, p, w, fused=mistake != "two_roundings")
        out.append(ema)
    return out


class _Flat(torch.nn.Module):
    def __init__(self, n):
        super(_Flat, self).__init__()
        self.p = torch.nn.Parameter(torch.zeros(n, dtype=torch.float32))


def torch_chain(stored, decay):
    """The definition: torch.optim.swa_utils.AveragedModel over the snapshots, on the CPU -> list of float32 numpy arrays."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    model = _Flat(int(np.asarray(stored[0]).size))
    avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(float(decay)))
    out = []
    for p in stored:
        with torch.no_grad():
            model.p.copy_(torch.as_tensor(np.asarray(p, np.float32)).view(-1))
        avg.update_parameters(model)
        out.append(avg.module.p.detach().numpy().copy())
    assert int(avg.n_averaged) == len(out)
    return out


def snapshots(n, seed, clamp=None):
    """K_UPDATES + 1 random parameter vectors (index 0: the parameters before the first update) -> (raw, stored): float32 N(0, 1) draws, and
    the same clamped to [-clamp, clamp]."""
    rng = np.random.RandomState(seed)
    raw = [rng.standard_normal(n).astype(np.float32) for _ in range(K_UPDATES + 1)]
    stored = raw if clamp is None else [np.clip(r, -np.float32(clamp), np.float32(clamp)) for r in raw]
    return raw, stored
