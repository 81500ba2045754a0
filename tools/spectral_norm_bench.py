"""The cfg2-size G+D step with hp.discriminator_spectral_norm off and on (GPU box).

Both settings live in ONE process and alternate round by round, so that clock state and neighbours hit both alike; a round is
`--steps` steps between two HIP events on the step stream, after `--warmup` steps of its own.  The figure of a setting is the median
of `--rounds` rounds with their min - max.  The added kernels are timed apart, through the hooks that share the step's launch
functions: gt_op_spectral_norm (three launches) and gt_op_sn_project (two) on the discriminator's own flat buffers, by events
over `--launches` calls.  "off" issues exactly the launches of an engine that never saw the option (tests/test_gpu_spectral_norm.py),
so its figure is comparable with bench.py's headline.  One JSON line; record only (profiles/spectral_norm.md).

    python tools/spectral_norm_bench.py [--steps 50] [--warmup 10] [--rounds 5] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
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
    from gantts_amd.engine import StepEngine, pitched_empty
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
        hp.discriminator_spectral_norm = on
        torch.manual_seed(0)
        mg = models.MLP(**B.G_SPEC).cuda().train()
        md = models.MLP(spectral_norm=on, **B.D_SPEC).cuda().train()
        og, od = optim.Adagrad(mg.parameters(), **B.OPT), optim.Adagrad(md.parameters(), **B.OPT)
        R = paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, Tn, dev)
        y_static = get_static_features(y, len(hp.windows), hp.stream_sizes, hp.has_dynamic_features)

        def step():
            T.hp = hp
            og.zero_grad()
            od.zero_grad()
            y_hat, y_hat_static = T.apply_generator(mg, x, R, cpu_lengths)
            T.update_discriminator(md, od, x, y_static, y_hat_static, cpu_lengths, mask, "train")
            T.update_generator(mg, md, og, x, y, y_hat, y_static, y_hat_static, 1.0, cpu_lengths, mask, "train", mse_w=0.0, mge_w=1.0)
        return step, md

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

    for on in (False, True):
        steps[on][0]()
    spin_up()
    StepEngine.sn_path_counts(reset=True)
    ms = {False: [], True: []}
    launches = {}
    for _ in range(args.rounds):
        for on in (False, True):
            step = steps[on][0]
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            StepEngine.sn_path_counts(reset=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            ms[on].append(e0.elapsed_time(e1) / args.steps)
            launches[on] = sum(StepEngine.sn_path_counts(reset=True)) / float(args.steps)

    # the added kernels alone, on the discriminator's own buffers
    md = steps[True][1]
    flat, grads = md.flat_params(), md.flat_grads().clone()
    c = L.SnCase()
    off = 0
    holders = md._holders()
    c.n_layers, c.iterate, c.n_flat = len(holders), 1, flat.numel()
    for q, h in enumerate(holders):
        c.w_off[q], c.out[q], c.in_[q] = off, h.out_features, h.in_features
        off += h.out_features * h.in_features + h.out_features
    u, v, weff = md.sn_u.clone(), md.sn_v.clone(), flat.clone()
    sigma = torch.zeros(len(holders), device=dev)
    s = torch.zeros(len(holders), dtype=torch.float64, device=dev)
    parts = torch.zeros(2048, dtype=torch.float64, device=dev)
    n_parts = C.c_int32(0)
    c.W, c.u, c.v, c.weff, c.sigma, c.G, c.s, c.norm_partials = (t.data_ptr() for t in (flat, u, v, weff, sigma, grads, s, parts))
    c.norm_cap, c.n_norm_partials = 2048, C.pointer(n_parts)

    def timed(fn):
        out = []
        for _ in range(args.rounds):
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / args.launches)
        return out

    prep = timed(lambda: L.check(L.lib.gt_op_spectral_norm(C.byref(c), L.current_stream())))
    proj = timed(lambda: L.check(L.lib.gt_op_sn_project(C.byref(c), L.current_stream())))

    def fig(v):
        return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=list(v))

    rec = dict(tool="spectral_norm_bench", batch=Bn, frames=Tn, steps=args.steps, warmup=args.warmup,
               step_ms=dict(off=fig(ms[False]), on=fig(ms[True])),
               sn_launches_per_step=dict(off=launches[False], on=launches[True]),
               added_us=dict(prepare_3_launches=fig(prep), project_2_launches=fig(proj)),
               d_params=int(flat.numel()))
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
