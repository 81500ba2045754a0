"""The cfg2-size G+D step with the generator's weight average (model_g.enable_weight_average / hp.generator_ema_decay) off and on (GPU box).

Both settings live in ONE process and alternate round by round, so that clock state and neighbours hit both alike; a round is
`--steps` steps between two HIP events on the step stream, after `--warmup` steps of its own.  The figure of a setting is the median
of `--rounds` rounds with their min - max.  The generator's fused clip + update launch is timed apart by the engine's launch profiler
(gt_profile_enable(2 + 8), slot 15 of gt_profile_read), switched on around update_generator alone for `--launches` steps per round: it
shows whether the average's four extra loads per thread were hidden.  "off" never called enable_weight_average, so its step figure is
comparable with bench.py's headline.  One JSON line; record only (profiles/generator_ema.md).

    python tools/generator_ema_bench.py [--steps 50] [--warmup 10] [--rounds 5] [--decay 0.999] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPTIM_SLOT, OPTIM_KIND = 15, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--spinup-ms", type=float, default=400.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import bench as B
    import gantts_amd.train as T
    from gantts_amd import _lib as L
    from gantts_amd import models, optim, paramgen
    from gantts_amd.engine import pitched_empty
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask

    dev = torch.device("cuda", 0)
    Bn, Tn = args.batch, args.frames
    x, y = B.synthetic_batch(Bn, Tn, 1000, dev)
    xp = pitched_empty(Bn, Tn, 425, dev)
    xp.copy_(x)
    x = xp
    lengths = torch.full((Bn,), Tn, dtype=torch.long, device=dev)
    cpu_lengths = [Tn] * Bn
    mask = sequence_mask(lengths).unsqueeze(-1)

    def setting(on):
        hp = B.make_hp()
        torch.manual_seed(0)
        mg = models.MLP(**B.G_SPEC).cuda().train()
        md = models.MLP(**B.D_SPEC).cuda().train()
        if on:
            mg.enable_weight_average(args.decay)
        og, od = optim.Adagrad(mg.parameters(), **B.OPT), optim.Adagrad(md.parameters(), **B.OPT)
        R = paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, Tn, dev)
        y_static = get_static_features(y, len(hp.windows), hp.stream_sizes, hp.has_dynamic_features)

        def step(profile_update=False):
            T.hp = hp
            og.zero_grad()
            od.zero_grad()
            y_hat, y_hat_static = T.apply_generator(mg, x, R, cpu_lengths)
            T.update_discriminator(md, od, x, y_static, y_hat_static, cpu_lengths, mask, "train")
            if profile_update:
                L.check(L.lib.gt_profile_enable(2 + OPTIM_KIND))
            T.update_generator(mg, md, og, x, y, y_hat, y_static, y_hat_static, 1.0, cpu_lengths, mask, "train", mse_w=0.0, mge_w=1.0)
            if profile_update:
                L.check(L.lib.gt_profile_enable(0))
        return step, mg

    steps = {False: setting(False), True: setting(True)}

    def spin_up():      # bench.py's: the device to its working clocks on a generic product, nothing of the workload
        ba, bw, bo = torch.rand(8192, 512, device=dev), torch.rand(512, 512, device=dev), torch.empty(8192, 512, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.spinup_ms:
            for _ in range(32):
                L.check(L.lib.gt_op_linear_forward(L.ptr(ba), 512, L.ptr(bw), None, L.ptr(bo), 512, 8192, 512, 512, 0, None, C.c_float(0.0),
                                                   L.current_stream()))
            torch.cuda.synchronize()

    def read_update_us():
        ms, fl, cnt = (C.c_double * L.PROFILE_SLOTS)(), (C.c_double * L.PROFILE_SLOTS)(), (C.c_int64 * L.PROFILE_SLOTS)()
        L.check(L.lib.gt_profile_read(ms, fl, cnt))
        by = (C.c_double * L.PROFILE_SLOTS)()
        L.check(L.lib.gt_profile_bytes(by))
        n = cnt[OPTIM_SLOT]
        return ms[OPTIM_SLOT] * 1e3 / n, by[OPTIM_SLOT] / n, n

    for on in (False, True):
        steps[on][0]()
    spin_up()
    ms = {False: [], True: []}
    upd = {False: [], True: []}
    upd_bytes = {}
    for _ in range(args.rounds):
        for on in (False, True):
            step = steps[on][0]
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            ms[on].append(e0.elapsed_time(e1) / args.steps)
            # the generator's update launch alone (two events around it: these steps are not part of the figure above)
            for _ in range(args.launches):
                step(profile_update=True)
            torch.cuda.synchronize()
            us, nbytes, n = read_update_us()
            assert n == args.launches, (n, args.launches)
            upd[on].append(us)
            upd_bytes[on] = nbytes

    def fig(v):
        return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=list(v))

    mg = steps[True][1]
    rec = dict(tool="generator_ema_bench", batch=Bn, frames=Tn, steps=args.steps, warmup=args.warmup, decay=args.decay,
               step_ms=dict(off=fig(ms[False]), on=fig(ms[True])),
               g_update_launch_us=dict(off=fig(upd[False]), on=fig(upd[True])),
               g_update_launch_bytes=dict(off=upd_bytes[False], on=upd_bytes[True]),
               g_params=int(mg.num_flat_params()), n_averaged=int(mg.n_averaged))
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
