"""The cfg2-size G+D step with hp.discriminator_grad_penalty off, "r1" and "wgan-gp" (GPU box).

The three settings live in ONE process and alternate round by round, so that clock state and neighbours hit all alike; a round is
`--steps` steps between two HIP events on the step stream, after `--warmup` steps of its own.  The figure of a setting is the median
of `--rounds` rounds with their min - max.  The added stage is timed apart through the hook that shares the step's launch function
(gt_op_grad_penalty: the second-order pass over N rows at the discriminator's shape, without WGAN-GP's extra forward), and the
launch census of a step is recorded beside it: gt_gp_path_counts and the product family's launches.  "off" issues exactly the
launches of an engine that never saw the option (tests/test_gpu_grad_penalty.py), so its figure is comparable with bench.py's
headline.  One JSON line; record only (profiles/grad_penalty.md).

    python tools/grad_penalty_bench.py [--steps 50] [--warmup 10] [--rounds 5] [--hook-only] [--out FILE]
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

KINDS = (None, "r1", "wgan-gp")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--spinup-ms", type=float, default=400.0)
    ap.add_argument("--hook-only", action="store_true", help="only the second-order pass through the hook (what a kernel trace is taken of)")
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

    def setting(kind):
        hp = B.make_hp()
        if kind is not None:
            hp.discriminator_grad_penalty = kind
        torch.manual_seed(0)
        mg = models.MLP(**B.G_SPEC).cuda().train()
        md = models.MLP(**B.D_SPEC).cuda().train()
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
        return step

    steps = {k: setting(k) for k in KINDS}

    def spin_up():      # bench.py's: the device to its working clocks on a generic product, nothing of the workload
        ba, bw, bo = torch.rand(8192, 512, device=dev), torch.rand(512, 512, device=dev), torch.empty(8192, 512, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.spinup_ms:
            for _ in range(32):
                L.check(L.lib.gt_op_linear_forward(L.ptr(ba), 512, L.ptr(bw), None, L.ptr(bo), 512, 8192, 512, 512, 0, None, C.c_float(0.0),
                                                   L.current_stream()))
            torch.cuda.synchronize()

    def gemm_launches(reset):
        g = (C.c_int64 * L.GEMM_PATH_SLOTS)()
        L.check(L.lib.gt_gemm_path_counts(g, 1 if reset else 0))
        return sum(g)

    if not args.hook_only:
        for k in KINDS:
            steps[k]()
    spin_up()
    ms = {k: [] for k in KINDS}
    census = {}
    for _ in range(0 if args.hook_only else args.rounds):
        for k in KINDS:
            step = steps[k]
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            StepEngine.gp_path_counts(reset=True)
            gemm_launches(True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.steps)
            gp = StepEngine.gp_path_counts(reset=True)
            census[str(k)] = dict(gp_path_counts=[c / float(args.steps) for c in gp], gp_kernel_launches=sum(gp[:5]) / float(args.steps),
                                  product_family_launches=gemm_launches(True) / float(args.steps))

    # the second-order pass alone, through the hook, at the discriminator's shape (N rows, Philox sites)
    N, Hd, Ld, cd, Da = Bn * Tn, B.D_SPEC["hidden_dim"], B.D_SPEC["num_hidden"], 425, 58
    ld_g = (Da + 3) & ~3
    ins = [cd + Da] + [Hd] * (Ld - 1)
    c = L.GpCase()
    keep = []
    c.L, c.H, c.cd, c.Da, c.ld_g, c.rows, c.weight, c.inv_tv = Ld, Hd, cd, Da, ld_g, N, 10.0, 1.0 / N
    for l, i in enumerate(ins):
        W, dW = torch.randn(Hd, i, device=dev) / i ** 0.5, torch.zeros(Hd, i, device=dev)
        Hact, a, cc = torch.randn(N, Hd, device=dev), torch.empty(N, Hd, device=dev), torch.empty(N, Hd, device=dev)
        keep += [W, dW, Hact, a, cc]
        c.W[l], c.dW[l], c.Hact[l], c.a[l], c.c[l] = (t.data_ptr() for t in (W, dW, Hact, a, cc))
        c.drop[l].mode, c.drop[l].p, c.drop[l].key0, c.drop[l].key1 = 1, 0.5, 1234 + l, 5678
    w_last, dw_last = torch.randn(Hd, device=dev) / Hd ** 0.5, torch.zeros(Hd, device=dev)
    g, phi, nrm = torch.empty(N, ld_g, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev)
    sums = torch.zeros(2, dtype=torch.float64, device=dev)
    c.w_last, c.dw_last, c.mask, c.g, c.phi, c.nrm, c.sums = (t.data_ptr() for t in (w_last, dw_last, mask.reshape(-1).contiguous(), g, phi, nrm, sums))

    def timed(fn):
        out = []
        for _ in range(args.rounds):
            for _ in range(10):
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

    hook = {}
    for kind, kid in (("r1", 1), ("wgan-gp", 2)):
        c.kind = kid
        hook[kind] = timed(lambda: L.check(L.lib.gt_op_grad_penalty(C.byref(c), L.current_stream())))

    def fig(v):
        return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=list(v))

    rec = dict(tool="grad_penalty_bench", batch=Bn, frames=Tn, steps=args.steps, warmup=args.warmup,
               step_ms={str(k): fig(ms[k]) for k in KINDS if ms[k]}, census_per_step=census,
               second_order_pass_us={k: fig(v) for k, v in hook.items()})
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
