"""Digests of one G + D step through the MLPG path, case by case: what tests/test_gpu_mlpg_digests.py demands bit for bit.

    python tests/golden/make_mlpg_digests.py [out.json]        (needs the GPU; default: mlpg_step_digests.json beside this file)

Every case runs apply_generator -> update_discriminator -> update_generator once from seeded state and records the SHA-256 of the
bytes of y_hat_static, of the D and the G loss tuples (as float64) and of every parameter afterwards (sorted by name), and one digest
over all of them in that order.

  step_dense, step_band   the STEP case of tests/test_gpu_mlpg_band.py (B = 3, T = 97, lengths 97 / 80 / 61), with a dense R and with an MLPGBand
  vc_in2out_dense         one step of the parity case vc_in2out (In2OutHighwayNet, B = 3, T = 48), with a dense R

The recorded file is the behaviour of the commit that recorded it -- the one before MLPG moved into eng_mlpg.hip and a launch began to
take its band as an argument; it is re-recorded only by a change that means to change a bit of the step."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
DEFAULT_OUT = os.path.join(HERE, "mlpg_step_digests.json")
CASES = ("step_dense", "step_band", "vc_in2out_dense")


def _step_arrays(name):
    """-> (y_hat_static, d tuple, g tuple, {name: parameter})"""
    if name == "vc_in2out_dense":
        import cases as C
        import gantts_amd.train as T
        from hip_runner import run_hip_case
        saved = getattr(T, "hp", None)
        try:
            out = run_hip_case(dict(C.CASES["vc_in2out"], steps=1))
        finally:
            T.hp = saved
        params = {k: v for k, v in out.items() if k[:2] in ("G.", "D.") and ".opt." not in k}
        return out["y_hat_static"], out["d_scalars_0"], out["g_scalars_0"], params
    import test_gpu_mlpg_band as S
    from gantts_amd import paramgen
    out = S._one_step(paramgen.unit_variance_mlpg_matrix_cuda if name == "step_dense" else paramgen.unit_variance_mlpg_band)
    return out["y_hat_static"], out["d"], out["g"], out["params"]


def run_case(name):
    """-> {"y_hat_static": sha256, "d": ..., "g": ..., "params": ..., "all": ...}"""
    yhs, d, g, params = _step_arrays(name)
    assert yhs.dtype == np.float32 and len(d) == 5 and len(g) == 4 and params
    parts = {"y_hat_static": [yhs], "d": [np.asarray(d, np.float64)], "g": [np.asarray(g, np.float64)],
             "params": [params[k] for k in sorted(params)]}
    out, whole = {}, hashlib.sha256()
    for part in ("y_hat_static", "d", "g", "params"):
        h = hashlib.sha256()
        for a in parts[part]:
            b = np.ascontiguousarray(a).tobytes()
            h.update(b)
            whole.update(b)
        out[part] = h.hexdigest()
    out["all"] = whole.hexdigest()
    return out


def main(argv):
    for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    record = {"cases": {name: run_case(name) for name in CASES}}
    out = argv[1] if len(argv) > 1 else DEFAULT_OUT
    with open(out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases" % (out, len(CASES)))


if __name__ == "__main__":
    main(sys.argv)
