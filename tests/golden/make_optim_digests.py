"""Digests of the fused clip + update step, case by case: what tests/test_gpu_optim_digests.py demands bit for bit.

    python tests/golden/make_optim_digests.py [out.json]        (needs the GPU; default: optim_step_digests.json beside this file)

Every case runs consecutive updates through ``gt_op_optim_step`` (the production launches: squared-norm partials, then the
clip + update kernel) and records the SHA-256 of the bytes of params, grads and every live state buffer after the last
update, plus the bits of the reported norm of every update.  The host scalar state of NAdam and ASGD between two updates
comes from ``gt_op_optim_scalars`` (host arithmetic only), as a caller of the stand-alone operator keeps it.

The inputs are a closed integer formula over the element index (a 64-bit Weyl sequence through the splitmix64 finaliser,
in numpy's wrapping uint64 arithmetic) mapped to float32 by exact scaling: no library's random generator, so the digests depend
on no library version.  Parameters lie in [-2, 2); a gradient is a 24-bit fraction in [-0.5, 0.5) times 2^-k, k = 0..10 per
element: three decades of magnitude.

The recorded file is the behaviour of the commit that recorded it; it is re-recorded only by a change that means to change
a bit of the update."""
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
DEFAULT_OUT = os.path.join(HERE, "optim_step_digests.json")

# 1: the tail alone; 4099: one predicated trip of the stride loop (3 past 16 x 256); 4 * 1024 * 256 + 259: the grid is capped at
# 1024 workgroups of 256, so this is the smallest class of n that takes a second trip and ends it predicated (4 MB a buffer)
SIZES = (1, 4099, 4 * 1024 * 256 + 259)
STATE_FILL = {"RPROP": {1: "lr"}}      # Rprop's step_size starts filled with lr (torch creates it so)

# name -> kind, hyper-parameters (fields of gt_optim_desc_ex), flags, and optionally: start (updates already taken), updates,
# max_grad_norm, gscale.  `rows`: the rows of the variant table (eng_ops.hip) the case is there to launch, in the order it
# reaches them.  weight_decay is non-zero wherever the kind has one.
CLIP = 1.0
CASES = {
    "sgd": dict(kind="SGD", h=dict(lr=1e-2, weight_decay=1e-4), rows=["SGD"]),
    "sgd_momentum_dampening": dict(kind="SGD", h=dict(lr=1e-2, weight_decay=1e-4, momentum=0.9, dampening=0.1), rows=["SGD|MOMENTUM"]),
    "sgd_nesterov": dict(kind="SGD", flags=["NESTEROV"], h=dict(lr=1e-2, weight_decay=1e-4, momentum=0.9), rows=["SGD|NESTEROV|MOMENTUM"]),
    "rmsprop": dict(kind="RMSPROP", h=dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=1e-5), rows=["RMSPROP"]),
    "rmsprop_centered": dict(kind="RMSPROP", flags=["CENTERED"], h=dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=1e-5),
                             rows=["RMSPROP|CENTERED"]),
    "rmsprop_momentum": dict(kind="RMSPROP", h=dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=1e-5, momentum=0.9),
                             rows=["RMSPROP|MOMENTUM"]),
    "rmsprop_momentum_centered": dict(kind="RMSPROP", flags=["CENTERED"],
                                      h=dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=1e-5, momentum=0.9),
                                      rows=["RMSPROP|CENTERED|MOMENTUM"]),
    "adadelta": dict(kind="ADADELTA", h=dict(lr=1.0, alpha=0.9, eps=1e-6, weight_decay=1e-5), rows=["ADADELTA"]),
    "adagrad_lr_decay_wd": dict(kind="ADAGRAD", h=dict(lr=1e-2, lr_decay=1e-3, eps=1e-10, weight_decay=1e-4), rows=["ADAGRAD|ORIGINAL"]),
    "adam": dict(kind="ADAM", h=dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-4), rows=["ADAM|ORIGINAL"]),
    "adam_amsgrad": dict(kind="ADAM", flags=["AMSGRAD"], h=dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-4),
                         rows=["ADAM|AMSGRAD"]),
    "adamw": dict(kind="ADAMW", h=dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2), rows=["ADAMW"]),
    "adamw_amsgrad": dict(kind="ADAMW", flags=["AMSGRAD"], h=dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2),
                          rows=["ADAMW|AMSGRAD"]),
    "adamax": dict(kind="ADAMAX", h=dict(lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-5), rows=["ADAMAX"]),
    "nadam": dict(kind="NADAM", h=dict(lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-5, momentum_decay=4e-3), rows=["NADAM"]),
    "nadam_decoupled": dict(kind="NADAM", flags=["DECOUPLED_WD"],
                            h=dict(lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, momentum_decay=4e-3),
                            rows=["NADAM|DECOUPLED"]),
    # default betas from step 4 on: update 5 is unrectified (rho_5 = 4.99), updates 6 to 8 are rectified
    "radam": dict(kind="RADAM", h=dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-4), start=4, updates=4,
                  rows=["RADAM", "RADAM|RECTIFIED"]),
    "radam_decoupled": dict(kind="RADAM", flags=["DECOUPLED_WD"], h=dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2),
                            start=4, updates=4, rows=["RADAM|DECOUPLED", "RADAM|DECOUPLED|RECTIFIED"]),
    "rprop": dict(kind="RPROP", h=dict(lr=1e-2, etaminus=0.5, etaplus=1.2, step_size_min=1e-6, step_size_max=50.0), rows=["RPROP"]),
    # t0 = 1: mu = 1 / max(1, t - t0) is the value the update AFTER update t averages with, so updates 1 to 3 copy (mu == 1) and
    # update 4 is the first that averages (mu = 0.5): four updates, to launch both rows
    "asgd": dict(kind="ASGD", h=dict(lr=1e-2, lambd=1e-4, alpha=0.75, t0=1.0, weight_decay=1e-5), updates=4, rows=["ASGD", "ASGD|AVERAGE"]),
    # the clip: every case above clips (the norm of these gradients is far above 1)
    "adagrad_norm_below_max": dict(kind="ADAGRAD", h=dict(lr=1e-2, lr_decay=1e-3, eps=1e-10, weight_decay=1e-4), max_grad_norm=1e6,
                                   rows=["ADAGRAD|ORIGINAL"]),
    "adam_clip_off": dict(kind="ADAM", h=dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-4), max_grad_norm=0.0,
                          rows=["ADAM|ORIGINAL"]),
    "adagrad_gscale": dict(kind="ADAGRAD", h=dict(lr=1e-2, lr_decay=1e-3, eps=1e-10, weight_decay=1e-4), gscale=1.0 / 37.0,
                           rows=["ADAGRAD|ORIGINAL"]),
}
N_STATES = dict(SGD=1, RMSPROP=3, ADADELTA=2, ADAGRAD=1, ADAM=2, ADAMW=2, ADAMAX=2, NADAM=2, RADAM=2, RPROP=2, ASGD=1)


def _mix(x):
    """splitmix64's finaliser on a uint64 array (numpy wraps modulo 2^64)."""
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _bits(n, stream):
    with np.errstate(over="ignore"):
        idx = np.arange(n, dtype=np.uint64)
        return _mix((idx + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(stream) * np.uint64(0xD1B54A32D192ED03))


_cache = {}


def inputs(n, update):
    """(params, gradient of update number `update`) for size n; update < 0: the initial parameters only.  Computed once per (n, update)."""
    key = (n, update)
    if key not in _cache:
        z = _bits(n, 2 * update + 2)
        frac = (z >> np.uint64(40)).astype(np.float64) / 2.0 ** 24 - 0.5       # 24 bits: exact in float32
        if update < 0:
            _cache[key] = (frac * 4.0).astype(np.float32)
        else:
            k = (_bits(n, 2 * update + 3) >> np.uint64(32)) % np.uint64(11)
            _cache[key] = (frac * np.ldexp(1.0, -k.astype(np.int64))).astype(np.float32)
    return _cache[key]


def case_states(case):
    """Indices of the state buffers the case's kind and flags use (state0..2 of the descriptor)."""
    kind, h, flags = case["kind"], case["h"], case.get("flags", ())
    if kind == "SGD":
        return [0] if h.get("momentum", 0.0) != 0.0 else []
    if kind == "RMSPROP":
        return [0] + ([1] if h.get("momentum", 0.0) != 0.0 else []) + ([2] if "CENTERED" in flags else [])
    return list(range(N_STATES[kind])) + ([2] if "AMSGRAD" in flags else [])


def reached_rows(case, L):
    """The variant-table rows the case's updates launch, by the host's own rule for the per-step flags."""
    kind, h, flags = case["kind"], case["h"], list(case.get("flags", ()))
    base = [kind] + [f.replace("DECOUPLED_WD", "DECOUPLED") for f in flags]
    if kind in ("SGD", "RMSPROP") and h.get("momentum", 0.0) != 0.0:
        base.append("MOMENTUM")
    if kind == "ADAGRAD" or (kind == "ADAM" and "AMSGRAD" not in flags):
        base.append("ORIGINAL")
    start, rows = case.get("start", 0), []
    scal = _initial_scalars(case)
    for t in range(start + 1, start + 1 + case.get("updates", 3)):
        row = list(base)
        if kind == "RADAM":
            b2t = h["beta2"] ** t
            rho_inf = 2.0 / (1.0 - h["beta2"]) - 1.0
            if rho_inf - 2.0 * t * b2t / (1.0 - b2t) > 5.0:
                row.append("RECTIFIED")
        if kind == "ASGD":
            if scal[1] != 1.0:
                row.append("AVERAGE")
            scal = _host_scalars(L, case, t - 1, t, scal)
        name = "|".join(row)
        if name not in rows:
            rows.append(name)
    return rows


def _initial_scalars(case):
    if case["kind"] == "NADAM":
        return (1.0, 0.0)
    if case["kind"] == "ASGD":
        return (float(np.float32(case["h"]["lr"])), 1.0)
    return (0.0, 0.0)


def _fill(desc, L, case, step, scalars):
    kind = case["kind"]
    desc.kind = getattr(L, "OPT_" + kind)
    desc.flags = 0
    for f in case.get("flags", ()):
        desc.flags |= getattr(L, "OPTF_" + f)
    for k, v in case["h"].items():
        setattr(desc, k, float(v))
    desc.max_grad_norm = float(case.get("max_grad_norm", CLIP))
    desc.step = int(step)
    desc.host_state0, desc.host_state1 = scalars


def _host_scalars(L, case, step, t, scalars):
    if case["kind"] not in ("NADAM", "ASGD"):
        return scalars
    desc = L.OptimDescEx2()
    _fill(desc, L, case, step, scalars)
    out = (C.c_double * 2)()
    L.check(L.lib.gt_op_optim_scalars(C.byref(desc), int(t), out))
    return (out[0], out[1])


def run_case(name, n):
    """-> {"params": sha256, "grads": ..., "state<k>": ..., "norm_bits": [hex of the float32 norm of every update]}"""
    import torch
    from gantts_amd import _lib as L
    case = CASES[name]
    live = case_states(case)
    p = torch.from_numpy(inputs(n, -1)).cuda()
    g = torch.empty_like(p)
    states = {k: torch.zeros_like(p) for k in live}
    for k, what in STATE_FILL.get(case["kind"], {}).items():
        states[k].fill_(float(case["h"][what]))
    gscale = torch.tensor([case["gscale"]], dtype=torch.float32).cuda() if "gscale" in case else None
    start, scalars, norms = case.get("start", 0), _initial_scalars(case), []
    for u in range(case.get("updates", 3)):
        g.copy_(torch.from_numpy(inputs(n, u)))
        desc = L.OptimDescEx2()
        _fill(desc, L, case, start + u, scalars)
        if case["kind"] == "SGD" and u > 0:
            desc.flags |= L.OPTF_BUFFER_LIVE      # the first update creates momentum_buffer, the later ones continue it
        for k in range(3):
            setattr(desc, "state%d" % k, states[k].data_ptr() if k in states else None)
        norm = C.c_float()
        L.check(L.lib.gt_op_optim_step(C.byref(desc), L.ptr(p), L.ptr(g), n, None if gscale is None else L.ptr(gscale), C.byref(norm),
                                       L.current_stream()))
        norms.append(np.float32(norm.value).view(np.uint32).item())
        scalars = _host_scalars(L, case, start + u, start + u + 1, scalars)
    torch.cuda.synchronize()
    out = {"params": p, "grads": g}
    out.update({"state%d" % k: s for k, s in states.items()})
    out = {k: hashlib.sha256(v.cpu().numpy().tobytes()).hexdigest() for k, v in out.items()}
    out["norm_bits"] = ["%08x" % b for b in norms]
    return out


def hipcc_version():
    exe = os.environ.get("HIPCC") or shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    try:
        return subprocess.check_output([exe, "--version"], stderr=subprocess.STDOUT).decode().strip().splitlines()
    except (OSError, subprocess.CalledProcessError):
        return ["unknown"]


def main(argv):
    sys.path.insert(0, ROOT)
    from gantts_amd import _lib as L
    record = {"hipcc_version": hipcc_version(), "sizes": list(SIZES), "cases": {}}
    for name, case in CASES.items():
        rows = reached_rows(case, L)
        assert rows == case["rows"], "%s launches the rows %s, not the %s it is there for" % (name, rows, case["rows"])
        record["cases"][name] = {"rows": rows, "digests": {str(n): run_case(name, n) for n in SIZES}}
    out = argv[1] if len(argv) > 1 else DEFAULT_OUT
    with open(out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases x %d sizes" % (out, len(CASES), len(SIZES)))


if __name__ == "__main__":
    main(sys.argv)
