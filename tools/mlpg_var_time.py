#!/usr/bin/env python
"""What variance-weighted MLPG (paramgen.mlpg, StepEngine.mlpg_var) costs on the device, beside the float64 host reference on this CPU.

  device   StepEngine.mlpg_var on the tts_acoustic layout (187 columns -> 63 static, one launch for mgc, lf0, vuv and bap) with the data
           variance as one row: one utterance at each --lengths T, and a batch of --batch sequences at --batch-length frames.  Host clock
           around the call to a device synchronise; median, min and max of --runs runs after two warm-up calls.
  host     tests/mlpg_var_ref.py (scipy.linalg.solveh_banded per static dimension, nnmnkwii's algorithm) on the same inputs, once per
           shape (--host-runs).

`--processes` fresh child processes repeat the whole thing.  One JSON line per process; record only, nothing is asserted.

    python tools/mlpg_var_time.py --processes 3
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)


def one_process(lengths, batch, batch_length, runs, host_runs):
    import numpy as np
    import torch
    import mlpg_var_ref as V
    from gantts_amd import hparams
    from gantts_amd.engine import StepEngine
    hp = hparams.tts_acoustic
    eng = StepEngine(hp)
    nW = len(hp.windows)
    D = sum(hp.stream_sizes)
    scol, sst, col = [], [], 0
    for sz, dyn in zip(hp.stream_sizes, hp.has_dynamic_features):
        w = sz // nW if dyn else sz
        scol += [col + c for c in range(w)]
        sst += [w if dyn else 0] * w
        col += sz
    scol, sst = np.array(scol), np.array(sst)
    rs = np.random.RandomState(0)
    var = (4.0 ** rs.uniform(-1, 1, D)).astype(np.float32)
    var_dev = torch.from_numpy(var).cuda()

    def shape(B, T):
        y = rs.randn(B, T, D).astype(np.float32)
        y_dev = torch.from_numpy(y).cuda()
        ms = []
        for r in range(runs + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.mlpg_var(y_dev, var_dev)
            torch.cuda.synchronize()
            if r >= 2:
                ms.append((time.perf_counter() - t0) * 1e3)
        host = []
        for _ in range(host_runs):
            t0 = time.perf_counter()
            V.reference(y, var, hp.windows, scol, sst, [T] * B)
            host.append((time.perf_counter() - t0) * 1e3)
        return {"B": B, "T": T, "device_ms": {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)},
                "host_reference_ms": round(min(host), 1) if host else None}

    shape(1, 96)          # code objects, allocator, the library's first launches
    return {"layout": "tts_acoustic", "variances": "one row", "unit": "ms", "runs": runs,
            "shapes": [shape(1, T) for T in lengths] + [shape(batch, batch_length)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lengths", type=int, nargs="+", default=[512, 1024, 2048])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--batch-length", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--host-runs", type=int, default=1)
    ap.add_argument("--processes", type=int, default=0, help="run this many fresh child processes one after the other (0: measure in this one)")
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds a child may take")
    a = ap.parse_args()
    if a.processes > 0:
        cmd = [sys.executable, os.path.abspath(__file__), "--runs", str(a.runs), "--host-runs", str(a.host_runs), "--batch", str(a.batch),
               "--batch-length", str(a.batch_length), "--lengths"] + [str(t) for t in a.lengths]
        for _ in range(a.processes):
            rc = subprocess.run(cmd, timeout=a.timeout).returncode
            if rc != 0:          # nothing more is started on the device after a failure
                sys.exit(rc)
        return
    print(json.dumps(one_process(a.lengths, a.batch, a.batch_length, a.runs, a.host_runs)), flush=True)


if __name__ == "__main__":
    main()
