#!/usr/bin/env python
"""Measurements of the device-resident batch path (gantts_amd.data.ResidentLoader, gt_op_assemble_batch) at cfg2 size; needs a GPU.

1. The assembly kernel: B=32, T=512 (all utterances 512 frames), 425 (+0 noise) / 187 columns, a corpus larger than the 256 MB
   Infinity Cache, batches drawn at random, output buffers rotated; HIP events around LAUNCHES launches.  Reported: the time, the rate
   algorithmic bytes / time (B T (428 + 188) 4 read + B T (428 + 187 + 63 + 1) 4 written), and -- in the same process -- a device
   copy moving the same number of bytes (half read, half written; buffers rotated the same way) and the ratio of the two.
2. The normalisation statistics of that corpus (gt_op_corpus_stats, ResidentCorpus.minmax / .meanvar): one device pass per side between
   HIP events against the host's data.minmax + data.meanvar on the same arrays and against the device copy's rate of part 1.
3. Batches per second on the same corpus through DevicePrefetcher(DataLoader) -- collate_fn and hp.device_collate -- and through
   ResidentLoader: each loader alone (a device synchronise at the end), then each inside train_loop's G+D step (one epoch:
   train phase + a short test phase, host clock around the call, which ends in the epoch's read-back).
4. --world N [N ...]: one data-parallel rank's launch (gt_op_assemble_shard, rank 0 of a world of N: 32 / N sequences) beside
   gt_op_assemble_batch on the whole batch, in the same process and in alternating rounds: launch time and the bytes each moves.

5. --ledger: only this part.  train_loop on the resident corpus with hp.device_epoch_ledger off and on, alternating epoch by epoch in
   one process (one corpus, one pair of networks; the first epoch of each setting warms up), in --processes fresh processes; medians
   and the spread over all timed epochs.  --layout cfg2 (this tool's corpus) or cfg1 (the VC layout, B = 8, T = 256).

    python tools/resident_bench.py [--utterances 1024] [--workers 1] [--world 2 4 8] [--no-loaders] [--out FILE]
    python tools/resident_bench.py --ledger [--layout cfg1] [--processes 3] [--rounds 5] [--out FILE]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, T, DX, DY = 32, 512, 425, 187
G_SPEC = dict(in_dim=425, out_dim=187, num_hidden=3, hidden_dim=512, dropout=0.5, last_sigmoid=False)
D_SPEC = dict(in_dim=483, out_dim=1, num_hidden=3, hidden_dim=256, dropout=0.5, last_sigmoid=True)


def make_hp(workers):
    from gantts_amd import hparams
    hp = types.SimpleNamespace(**hparams.tts_acoustic.values())
    hp.batch_size, hp.num_workers, hp.nepoch, hp.lr_decay_schedule = B, workers, 1, False
    hp.generator_add_noise = False
    return hp


def make_corpus(n, seed=0):
    """n utterances of T frames; float32 min / max of x, float64 mean / std of y (what minmax() and meanvar() return)."""
    rng = np.random.default_rng(seed)
    X = [rng.random((T, DX), dtype=np.float32) for _ in range(n)]
    Y = [rng.standard_normal((T, DY), dtype=np.float32) for _ in range(n)]
    return X, Y, np.zeros(DX, np.float32), np.ones(DX, np.float32), rng.standard_normal(DY) * 0.3, 0.5 + rng.random(DY)


def kernel_time(ds, hp, launches, nbuf=8):
    import torch
    from gantts_amd import data as D
    loader = D.ResidentLoader(ds, B, True, hp)
    Ds = len(loader.scol_host)
    bufs = [(torch.empty(B, T, 428, device="cuda"), torch.empty(B, T, DY, device="cuda"), torch.empty(B, T, Ds, device="cuda"),
             torch.empty(B, T, 1, device="cuda"), torch.empty(B, device="cuda", dtype=torch.int64)) for _ in range(nbuf)]
    nbytes = B * T * (428 + 188) * 4 + B * T * (428 + DY + Ds + 1) * 4
    half = nbytes // 2 // 16 * 4                                       # floats: the copy reads `half` floats and writes as many
    src = [torch.rand(half, device="cuda") for _ in range(nbuf)]
    dst = [torch.empty(half, device="cuda") for _ in range(nbuf)]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

    case, plan = loader.begin_epoch()                                  # one random epoch; its full batches are launched in turn
    plan = [p for p in plan if p[1] == B]
    busy = torch.rand(8192, 8192, device="cuda")

    def occupy():                                                      # keeps the device busy while the host enqueues the window,
        for _ in range(2):                                             # so that the events bracket back-to-back launches
            torch.mm(busy, busy)

    def run_kernel(n, record):
        occupy()
        if record:
            ev[0].record()
        for k in range(n):
            first, b, t, _ = plan[k % len(plan)]
            loader.assemble(case, first, b, t, out=bufs[k % nbuf])
        if record:
            ev[1].record()

    def run_copy(n, record):
        occupy()
        if record:
            ev[2].record()
        for k in range(n):
            dst[k % nbuf].copy_(src[k % nbuf])
        if record:
            ev[3].record()

    res = {}
    for rep in range(3):                                               # alternating; the first round is the warm-up
        run_kernel(launches, True)
        run_copy(launches, True)
        torch.cuda.synchronize()
        res.update(kernel_us=ev[0].elapsed_time(ev[1]) * 1e3 / launches, copy_us=ev[2].elapsed_time(ev[3]) * 1e3 / launches)
        res["round_%d" % rep] = [round(res["kernel_us"], 2), round(res["copy_us"], 2)]
    res.update(algorithmic_bytes=nbytes, launches=launches, kernel_TBps=nbytes / res["kernel_us"] * 1e-6,
               copy_TBps=2 * half * 4 / res["copy_us"] * 1e-6)
    res["kernel_over_copy_rate"] = res["kernel_TBps"] / res["copy_TBps"]
    return res


def shard_time(ds, hp, launches, worlds, nbuf=8):
    """One data-parallel rank's launch (gt_op_assemble_shard: rank 0 of each world in `worlds`, B / world sequences padded to the same
    T, tv_global written) beside gt_op_assemble_batch on the whole batch: one corpus, one process, alternating rounds as in kernel_time
    (HIP events around `launches` back-to-back launches behind a busy device; the first round warms up).  A rank's launch at 4 sequences
    is 128 workgroups on 256 CUs -- latency-bound --, so the figure to read is the launch time; the bytes each moves are reported beside it."""
    import torch
    from gantts_amd import data as D
    corpus = D.ResidentCorpus(ds)
    row_bytes = (428 + 188) * 4 + (428 + DY + 63 + 1) * 4
    busy = torch.rand(8192, 8192, device="cuda")
    runs = {}
    for w in [1] + list(worlds):
        loader = D.ResidentLoader(corpus, B, True, hp, rank=0, world=w, short_batch="drop")
        Ds, b = len(loader.scol_host), B // w
        bufs = [(torch.empty(b, T, 428, device="cuda"), torch.empty(b, T, DY, device="cuda"), torch.empty(b, T, Ds, device="cuda"),
                 torch.empty(b, T, 1, device="cuda"), torch.empty(b, device="cuda", dtype=torch.int64)) for _ in range(nbuf)]
        case, plan = loader.begin_epoch()
        plan = [p for p in plan if p[1] == B]                      # the full batches: (first, B, T, ..) / (first, B_global, B_local, T, ..)
        tv = torch.zeros(1, device="cuda", dtype=torch.float64)
        runs[w] = (loader, case, plan, bufs, tv, [torch.cuda.Event(enable_timing=True) for _ in range(2)])

    def run(w):
        loader, case, plan, bufs, tv, ev = runs[w]
        for _ in range(2):
            torch.mm(busy, busy)
        ev[0].record()
        for k in range(launches):
            p = plan[k % len(plan)]
            if w == 1:
                loader.assemble(case, p[0], p[1], p[2], out=bufs[k % nbuf])
            else:
                loader.assemble(case, p[0], p[2], p[3], out=bufs[k % nbuf], B_global=p[1], tv_global=tv)
        ev[1].record()

    res = {"launches": launches, "rounds_us": {}}
    for rep in range(3):
        for w in runs:
            run(w)
        torch.cuda.synchronize()
        for w in runs:
            ev = runs[w][5]
            res["rounds_us"].setdefault("world_%d" % w, []).append(round(ev[0].elapsed_time(ev[1]) * 1e3 / launches, 2))
    for w in runs:
        if w > 1:
            assert float(runs[w][4]) == float(B * T)               # every utterance of this corpus has T frames
        res["world_%d" % w] = {"sequences": B // w, "workgroups": (B // w) * T // 16, "algorithmic_bytes": (B // w) * T * row_bytes,
                               "launch_us": res["rounds_us"]["world_%d" % w][-1]}
    return res


def stats_time(X, Y, copy_TBps, passes=20):
    """The normalisation statistics of the same corpus: host data.minmax / data.meanvar per side (host clock) against one
    gt_op_corpus_stats pass per side (min, max, count, mean and M2 of every column in one read of the side; HIP events around `passes`
    back-to-back passes behind a busy device, the last of three rounds).  Rates are algorithmic bytes F * ld * 4 over the time; the
    corpus is larger than the Infinity Cache, so every pass reads HBM.  `copy_TBps` is kernel_time's device copy in this process."""
    import ctypes as C
    import torch
    from gantts_amd import _lib as L
    from gantts_amd import data as D
    res, host = {}, {}
    for side, arrays in (("x", X), ("y", Y)):
        t0 = time.perf_counter()
        lo, hi = D.minmax(arrays)
        t1 = time.perf_counter()
        mean, var = D.meanvar(arrays)
        t2 = time.perf_counter()
        host[side] = (lo, hi, mean, var)
        res[side] = {"host_minmax_s": t1 - t0, "host_meanvar_s": t2 - t1}
    t0 = time.perf_counter()
    corpus = D.ResidentCorpus.from_arrays(X, Y)
    torch.cuda.synchronize()
    res["upload_s"] = time.perf_counter() - t0
    busy = torch.rand(8192, 8192, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for side, ld in (("x", corpus.ldX), ("y", corpus.ldY)):
        case, out_f, out_d = corpus.stats_case(side)
        nbytes = corpus.F * ld * 4
        rounds = []
        for rep in range(3):
            for _ in range(2):
                torch.mm(busy, busy)
            ev[0].record()
            for _ in range(passes):
                L.check(L.lib.gt_op_corpus_stats(C.byref(case), L.current_stream()))
            ev[1].record()
            torch.cuda.synchronize()
            rounds.append(ev[0].elapsed_time(ev[1]) * 1e3 / passes)
        lo, hi, mean, var = host[side]
        f, d = out_f.cpu().numpy(), out_d.cpu().numpy()
        assert np.array_equal(f[0], lo) and np.array_equal(f[1], hi) and d[0][0] == corpus.F
        assert np.allclose(d[1], mean, rtol=1e-9, atol=1e-12) and np.allclose(d[2] / corpus.F, var, rtol=1e-9, atol=1e-12)
        r = res[side]
        r.update(algorithmic_bytes=nbytes, device_us=rounds[-1], rounds_us=[round(v, 2) for v in rounds], device_TBps=nbytes / rounds[-1] * 1e-6)
        r["device_over_copy_rate"] = r["device_TBps"] / copy_TBps
        r["host_over_device"] = (r["host_minmax_s"] + r["host_meanvar_s"]) / (rounds[-1] * 1e-6)
    # what the start-up of a TTS run computes: minmax of x and meanvar of y
    res["tts_startup"] = {"host_s": res["x"]["host_minmax_s"] + res["y"]["host_meanvar_s"],
                          "device_s": (res["x"]["device_us"] + res["y"]["device_us"]) * 1e-6}
    return res


def loader_alone(make_batches, n_batches):
    """Batches per second of an iterable of DeviceBatches, nothing else on the device; the first epoch warms up."""
    import torch
    out = None
    for rep in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for batch in make_batches():
            n += 1
        torch.cuda.synchronize()
        out = n / (time.perf_counter() - t0)
        assert n == n_batches
    return out


def with_step(loaders, hp):
    """Batches per second of train_loop's epoch (train + test phase) on these loaders; the first epoch warms up."""
    import torch
    import gantts_amd.train as TR
    from gantts_amd import models, optim
    TR.hp = hp
    torch.manual_seed(0)
    mg, md = models.MLP(**G_SPEC).cuda(), models.MLP(**D_SPEC).cuda()
    og = optim.Adagrad(mg.parameters(), lr=0.01, weight_decay=1e-7)
    od = optim.Adagrad(md.parameters(), lr=0.01, weight_decay=1e-7)
    n = len(loaders["train"]) + len(loaders["test"])
    out = None
    for rep in range(2):
        TR.global_epoch = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        TR.train_loop((mg, md), (og, od), loaders, w_d=1.0, mse_w=0.0, mge_w=1.0)
        torch.cuda.synchronize()
        out = n / (time.perf_counter() - t0)
    return out


# ---- 5. --ledger: train_loop on a resident corpus with hp.device_epoch_ledger off and on ------------------------------------------
CFG1 = dict(B=8, T=256, D=75, order=25,
            g=dict(in_dim=75, out_dim=75, static_dim=25, num_hidden=3, hidden_dim=512, dropout=0.5),
            d=dict(in_dim=25, out_dim=1, num_hidden=2, hidden_dim=256, dropout=0.5, last_sigmoid=True))


def ledger_leg(layout, utterances, test_utterances, rounds):
    """One process: epochs of train_loop (train + test phase, host clock around the call, a device synchronise on either side) on ONE
    resident corpus, ONE pair of networks, the switch alternating off, on, off, on, ...; the first epoch of each setting warms up and
    is not reported.  layout "cfg2": this tool's corpus and networks; "cfg1": the VC layout (In2OutHighwayNet 75 -> 512 x 3 -> 75,
    MLP D 25 -> 256 x 2 -> 1, B = 8, T = 256)."""
    import torch
    import gantts_amd.train as TR
    from gantts_amd import data as D
    from gantts_amd import hparams, models, optim
    torch.manual_seed(0)
    if layout == "cfg2":
        hp = make_hp(1)
        X, Y, lo, hi, mean, std = make_corpus(utterances)
        hp.resident_corpus = True
        loaders = D.get_tts_data_loaders({"train": X, "test": X[:test_utterances]}, {"train": Y, "test": Y[:test_utterances]}, lo, hi, mean, std, hp)
        mg, md = models.MLP(**G_SPEC).cuda(), models.MLP(**D_SPEC).cuda()
    else:
        c = CFG1
        hp = types.SimpleNamespace(**hparams.vc.values())
        hp.batch_size, hp.num_workers, hp.nepoch, hp.lr_decay_schedule = c["B"], 1, 1, False
        hp.stream_sizes, hp.has_dynamic_features, hp.order, hp.adversarial_streams = [c["D"]], [True], c["order"], None
        hp.generator_add_noise, hp.resident_corpus = False, True
        rng = np.random.default_rng(0)
        X = [rng.standard_normal((c["T"], c["D"]), dtype=np.float32) for _ in range(utterances)]
        Y = [rng.standard_normal((c["T"], c["D"]), dtype=np.float32) for _ in range(utterances)]
        mean, std = rng.standard_normal(c["D"]) * 0.3, 0.5 + rng.random(c["D"])
        loaders = D.get_vc_data_loaders({"train": X, "test": X[:test_utterances]}, {"train": Y, "test": Y[:test_utterances]}, mean, std, hp)
        mg, md = models.In2OutHighwayNet(**c["g"]).cuda(), models.MLP(**c["d"]).cuda()
    TR.hp = hp
    og = optim.Adagrad(mg.parameters(), lr=0.01, weight_decay=1e-7)
    od = optim.Adagrad(md.parameters(), lr=0.01, weight_decay=1e-7)
    n = len(loaders["train"]) + len(loaders["test"])
    rates = {"off": [], "on": []}
    for rep in range(rounds + 1):
        for tag in ("off", "on"):
            hp.device_epoch_ledger = tag == "on"
            TR.global_epoch = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            TR.train_loop((mg, md), (og, od), loaders, w_d=1.0, mse_w=0.0, mge_w=1.0)
            torch.cuda.synchronize()
            if rep:
                rates[tag].append(n / (time.perf_counter() - t0))
    return {"layout": layout, "batches_per_epoch": n, "B": hp.batch_size, "off_batches_per_s": rates["off"], "on_batches_per_s": rates["on"]}


def ledger_processes(a):
    """--ledger: `--processes` fresh processes in turn, each one ledger_leg(); medians and spread over every timed epoch of every process."""
    import subprocess
    runs = []
    for _ in range(a.processes):
        cmd = [sys.executable, os.path.abspath(__file__), "--ledger-child", "--layout", a.layout, "--utterances", str(a.utterances),
               "--test-utterances", str(a.test_utterances), "--rounds", str(a.rounds)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.child_timeout)
        if p.returncode != 0:      # nothing more is started on the device behind a failed process
            raise SystemExit("resident_bench: a --ledger process ended with status %d" % p.returncode)
        runs.append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
    res = {"layout": a.layout, "processes": a.processes, "rounds": a.rounds, "batches_per_epoch": runs[0]["batches_per_epoch"], "B": runs[0]["B"]}
    for tag in ("off", "on"):
        v = sorted(r for run in runs for r in run[tag + "_batches_per_s"])
        res[tag] = {"median_batches_per_s": float(np.median(v)), "min": v[0], "max": v[-1],
                    "per_process_median": [float(np.median(run[tag + "_batches_per_s"])) for run in runs]}
    res["on_over_off"] = res["on"]["median_batches_per_s"] / res["off"]["median_batches_per_s"]
    res["ms_per_batch_saved"] = 1e3 / res["off"]["median_batches_per_s"] - 1e3 / res["on"]["median_batches_per_s"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ledger", action="store_true", help="only part 5: train_loop with hp.device_epoch_ledger off and on, alternating, in fresh processes")
    ap.add_argument("--ledger-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--layout", choices=["cfg2", "cfg1"], default="cfg2")
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5, help="timed epochs per setting and process (one more warms up)")
    ap.add_argument("--child-timeout", type=float, default=300.0)
    ap.add_argument("--utterances", type=int, default=1024, help="utterances of 512 frames (1024: a 1.3 GB corpus)")
    ap.add_argument("--test-utterances", type=int, default=64)
    ap.add_argument("--workers", type=int, default=1, help="DataLoader workers of the host pipeline (hp.num_workers)")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--stats-passes", type=int, default=20)
    ap.add_argument("--world", type=int, nargs="+", default=[], help="also time one rank's launch of a world of N (a divisor of 32)")
    ap.add_argument("--no-loaders", action="store_true", help="the kernel and the statistics only (parts 1 and 2)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if any(w < 2 or B % w for w in a.world):
        raise SystemExit("resident_bench: --world takes divisors of %d above 1" % B)
    if a.ledger and not a.ledger_child:      # this process starts the measuring ones and never opens the device itself
        line = json.dumps({"ledger": ledger_processes(a)})
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("resident_bench: needs a GPU (no CPU path)")
    if a.ledger_child:
        print(json.dumps(ledger_leg(a.layout, a.utterances, a.test_utterances, a.rounds)))
        return
    from gantts_amd import data as D
    hp = make_hp(a.workers)
    X, Y, lo, hi, mean, std = make_corpus(a.utterances)
    Xs = {"train": X, "test": X[:a.test_utterances]}
    Ys = {"train": Y, "test": Y[:a.test_utterances]}
    res = {"B": B, "T": T, "utterances": a.utterances, "corpus_bytes": a.utterances * T * (428 + 188) * 4, "workers": a.workers}
    ds = D.TTSDataset(X, Y, lo, hi, mean, std, hp=hp)
    res["kernel"] = kernel_time(ds, hp, a.launches)
    if a.world:
        res["shard"] = shard_time(ds, hp, a.launches, a.world)
    res["stats"] = stats_time(X, Y, res["kernel"]["copy_TBps"], a.stats_passes)
    n_train = (a.utterances + B - 1) // B
    for tag, flags in () if a.no_loaders else (("host_collate", {}), ("host_device_collate", {"device_collate": True}), ("resident", {"resident_corpus": True})):
        for k in ("device_collate", "resident_corpus"):
            setattr(hp, k, bool(flags.get(k, False)))
        loaders = D.get_tts_data_loaders(Xs, Ys, lo, hi, mean, std, hp)
        train = loaders["train"]
        if flags.get("resident_corpus"):
            alone = loader_alone(lambda: iter(train), n_train)
        else:
            alone = loader_alone(lambda: iter(D.DevicePrefetcher(train, pitch_x=True)), n_train)
        res[tag] = {"loader_alone_batches_per_s": alone, "with_step_batches_per_s": with_step(loaders, hp)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
