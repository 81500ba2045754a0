#!/usr/bin/env python
"""First sight of a new padded length T on the MLPG path: what one multi_stream_mlpg call costs when neither a dense R nor a band for T exists yet.

  dense    paramgen.unit_variance_mlpg_matrix (host, float64 banded solve of nW*T right-hand sides) + upload + ensure_band's extraction
  device   paramgen.MLPGBand: ensure_band builds the band on the device from hp.windows (gantts_amd/csrc/mlpg_band_kernels.hip.h)

Both end in the same forward launch over one sequence and a device synchronise; the host clock runs around all of it.  Every T is timed
`--rounds` times per path in one process, the two paths in alternating order, with the host and device caches dropped before each
timing; `--processes` fresh child processes repeat the whole thing.  One JSON line per process; record only, nothing is asserted.

    python tools/mlpg_first_sight.py --processes 3
"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def one_process(lengths, rounds):
    import torch
    from gantts_amd import hparams, paramgen
    from gantts_amd.engine import StepEngine
    hp = hparams.tts_acoustic
    eng = StepEngine(hp)
    D = sum(hp.stream_sizes)

    def first_sight(T, device):
        paramgen._cache.clear()
        paramgen._dev_cache.clear()
        eng.invalidate_mlpg_cache()
        y = torch.randn(1, T, D, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        R = paramgen.unit_variance_mlpg_band(hp.windows, T) if device else paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, T)
        eng.mlpg_forward(y, R)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for device in (False, True):          # code objects, allocator, the library's first launches
        first_sight(96, device)
    out = {"windows": "hp.windows", "unit": "ms", "rounds": rounds, "T": {}}
    for T in lengths:
        res = {"dense": [], "device": []}
        for r in range(rounds):
            for device in ((False, True) if r % 2 == 0 else (True, False)):
                res["device" if device else "dense"].append(round(first_sight(T, device), 3))
        out["T"][str(T)] = res
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lengths", type=int, nargs="+", default=[512, 1024, 2048])
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--processes", type=int, default=0, help="run this many fresh child processes one after the other (0: measure in this one)")
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds a child may take")
    a = ap.parse_args()
    if a.processes > 0:
        cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--lengths"] + [str(t) for t in a.lengths]
        for _ in range(a.processes):
            rc = subprocess.run(cmd, timeout=a.timeout).returncode
            if rc != 0:          # nothing more is started on the device after a failure
                sys.exit(rc)
        return
    print(json.dumps(one_process(a.lengths, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
