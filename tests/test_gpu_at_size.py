"""-m gpu: one G+D step at the sizes BASELINE.json's configs name, against committed digests of the REAL reference
(cfg1 VC In2OutHighwayNet B = 8 T = 256, cfg2 cold, cfg3 BiLSTM T = 1024, cfg5 B = 64 acoustic + duration pairs) or of the oracle's restated SRU (cfg4 T = 2048, parity
unpinned).  Format and tolerance rule: tests/golden/at_size.py -- the engine may be as far from the float64 result as
the reference's own float32 arithmetic is (x ARBITER_FACTOR), tensor by tensor; counts exact."""
import os
import types

import numpy as np
import pytest
import torch

import at_size as A
import cases as C

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_REPORT = os.environ.get("GT_PARITY_REPORT")

# Ratchet.  The arbiter's limits are orders of magnitude above what the engine achieves on most tensors (D gradients of
# cfg2_cold sit at 2e-7 against 5.5e-4): a change that costs three digits there would stay green.  tests/golden/at_size_ratchet.json holds, per
# (case label, tensor), the distance to the float64 reference MEASURED on the GPU with the build that was committed with it; a tensor must stay
# within RATCHET_FACTOR x that (never below RATCHET_FLOOR: a few float32 ulps) AND within the arbiter's limit.  The engine is bit-reproducible run
# to run, so the ratchet only moves with the code: a change that trips it is looked at, and -- if it is a legitimate re-association (a LeakyReLU
# slope flip moves a gradient tensor by ~1e-4 at once, at_size.py) -- the file is regenerated in the same commit:
#     GT_RATCHET_WRITE=tests/golden/at_size_ratchet.json python -m pytest tests/test_gpu_at_size.py -m gpu -q
RATCHET_FACTOR, RATCHET_FLOOR = 4.0, 4e-7
_RATCHET_PATH = os.path.join(GOLDEN, "at_size_ratchet.json")
_RATCHET_WRITE = os.environ.get("GT_RATCHET_WRITE")


def _load_ratchet():
    import json
    return json.load(open(_RATCHET_PATH)) if os.path.isfile(_RATCHET_PATH) else {}


_RATCHET = _load_ratchet()
_RATCHET_SEEN = {}


def run_hip_at_size(case, engine_options=None):
    """The HIP engine on one at-size case, through the reference-shaped API; same record layout as make_at_size.py."""
    import gantts_amd.train as T
    from gantts_amd import optim, paramgen
    from gantts_amd.engine import engine_for
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model, make_hp
    hp = make_hp(case)
    if case["noise_dim"]:
        hp.generator_add_noise, hp.generator_noise_dim = True, case["noise_dim"]
    T.hp = hp
    mg, md = build_model(case["g"], 11).train(), build_model(case["d"], 22).train()
    w0 = {"G." + k: v.cpu().numpy().copy() for k, v in mg.state_dict().items()}
    w0.update({"D." + k: v.cpu().numpy().copy() for k, v in md.state_dict().items()})
    og = getattr(optim, case["opt_g"][0])(mg.parameters(), **case["opt_g"][1])
    od = getattr(optim, case["opt_d"][0])(md.parameters(), **case["opt_d"][1])
    eng = engine_for(hp, mg)
    for k, v in (engine_options or {}).items():
        eng.set_option(k, v)
    x_np, y_np, lengths, z_np = A.make_inputs(case)
    x, y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
    gin = torch.cat((x, torch.from_numpy(z_np).cuda()), -1) if z_np is not None else x      # train.py:542
    Tn = case["T"]
    R = paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, Tn) if np.any(case["has_dynamic_features"]) else None
    mask = sequence_mask(torch.from_numpy(lengths).cuda()).unsqueeze(-1)
    cl = list(lengths)
    nh = case["d"]["num_hidden"]
    out = {}

    def split(model, flat):
        res, off = {}, 0
        for k, v in model.state_dict().items():
            res[k] = flat[off:off + v.numel()].reshape(tuple(v.shape))
            off += v.numel()
        return res

    for step in range(case["steps"]):
        gm, dm = C.make_dropout_masks(case, step)
        mg.set_dropout_masks(0, [torch.from_numpy(m) for m in gm])
        for p in range(3):
            md.set_dropout_masks(p, [torch.from_numpy(m) for m in dm[p * nh:(p + 1) * nh]])
        del gm, dm
        y_static = get_static_features(y, len(hp.windows), hp.stream_sizes, hp.has_dynamic_features)
        og.zero_grad(), od.zero_grad()
        y_hat, y_hat_static = T.apply_generator(mg, gin, R, cl)
        if step == 0:
            out["y_hat"], out["y_hat_static"] = y_hat.cpu().numpy(), y_hat_static.cpu().numpy()
        res = T.update_discriminator(md, od, x, y_static, y_hat_static, cl, mask, "train")
        out["d_scalars_%d" % step] = np.array(res, dtype=np.float64)
        if step == 0:      # D.grad as the D step leaves it (clipped in place like clip_grad_norm_, train.py:275)
            for k, v in split(md, md.flat_grads().cpu().numpy().copy()).items():
                out["Dgrad." + k] = v
        res = T.update_generator(mg, md, og, x, y, y_hat, y_static, y_hat_static, case["adv_w"], cl, mask, "train",
                                 mse_w=case["mse_w"], mge_w=case["mge_w"])
        out["g_scalars_%d" % step] = np.array(res, dtype=np.float64)
        if step == 0:
            for k, v in split(mg, mg.flat_grads().cpu().numpy().copy()).items():
                out["Ggrad." + k] = v
    eng.check_faults()
    for k, v in mg.state_dict().items():
        out["Gupd." + k] = v.cpu().numpy() - w0["G." + k]
    for k, v in md.state_dict().items():
        out["Dupd." + k] = v.cpu().numpy() - w0["D." + k]
    return out


COLD_ELEMENT_RTOL = 1e-4      # north_star's float32 tolerance, per element, for the updates of a cold-accumulator case
COLD_OUTLIERS = 1e-3          # fraction of unambiguous sampled elements that may miss it (LeakyReLU slope flips, at_size.KINK_ALLOWANCE)


def judge_cold_update(k, got, fx, grad_err):
    """Update tensor of a cold-accumulator case (cfg2_cold: Adagrad with initial accumulator 0, hparams.py:223-227).  The first
    update is lr * g / (|g| + 1e-10) = lr * sign(g): a gradient element that is zero WITHIN ROUNDING gets either sign, in the
    reference's float32 run as in the engine's, and that parameter then differs by 2 * lr.  Such elements are identified, not
    averaged away: element i of the sample is *ambiguous* when its first-step gradient -- the float64 reference's (kept in the
    digest at the same positions) or the engine's -- is below 20 x the engine's typical (median) element error on that gradient,
    measured on the same sample (the median, not the rms: the rms is dominated by the few elements a LeakyReLU slope flip moves).
    Every unambiguous element must match the float64 reference to COLD_ELEMENT_RTOL of the tensor's largest update (2 steps);
    at most COLD_OUTLIERS of them may miss.  Returns (ambiguous fraction, outlier fraction, worst unambiguous error / limit)."""
    ref = fx[k + ".sample"].astype(np.float64)
    g = A.sample_of(k, np.asarray(got[k], dtype=np.float64))
    gname = k[0] + "grad." + k[5:]
    g1_ref = fx[k + ".g1"].astype(np.float64)
    g1_eng = A.sample_of(k, np.asarray(got[gname], dtype=np.float64))
    # The ambiguity threshold may not grow with the error of the engine under test: it is capped by the REFERENCE's own
    # float32-vs-float64 distance on this gradient tensor, which the digest records (relative rms over the full tensor x its rms).
    ref_level = float(fx[gname + ".err32"]) * float(fx[k + ".g1rms"]) if (gname + ".err32") in fx.files else float("inf")
    thr = 20.0 * max(min(float(np.median(np.abs(g1_eng - g1_ref))), ref_level), 1e-7 * float(fx[k + ".g1rms"]))
    ambiguous = (np.abs(g1_ref) <= thr) | (np.abs(g1_eng) <= thr)
    top = max(float(np.abs(ref).max()), 1e-30)
    lim = COLD_ELEMENT_RTOL * top + 1e-9
    ratio = np.abs(g - ref) / lim
    clear = ~ambiguous
    out_frac = float((ratio[clear] > 1).mean()) if clear.any() else 0.0
    median = float(np.median(ratio[clear])) if clear.any() else 0.0
    # hard bound on every unambiguous element: the cold update is lr * sign(g), so the worst a slope-flipped element can be off by is
    # a sign, i.e. twice the largest update; anything beyond that is a wrong value, not a flip
    hard = float(np.abs(g - ref)[clear].max()) / top if clear.any() else 0.0
    assert hard <= 2.0 * (1.0 + 1e-3), "%s: an unambiguous element is off by %.3f x the largest update" % (k, hard)
    assert median <= 0.5, "%s: the typical unambiguous element sits at %.3f x the 1e-4 limit" % (k, median)
    return float(ambiguous.mean()), out_frac, median


# Later steps of a long run (cfg3_lstm_10: ten G+D steps): a GAN step with dropout 0.5 in D amplifies a rounding-level perturbation by x3 .. x5 per
# step, so two CORRECT float32 evaluations with different summation orders separate from the float64 run by the same law with a random prefactor.
# [r6] That prefactor is MEASURED, not asserted (VERDICT r5 / ADVICE r5): tests/golden/make_drift_spread.py runs the REAL reference's ten steps in
# float32 under other summation orders (thread counts; the discriminator's hidden units relabelled) and records, per variant, the late-step
# scalars' distance to the float64 run over the reference's own float32 envelope, and every update tensor's distance over the network's float32
# level (tests/golden/drift_spread_cfg3_lstm_10.json).  The limits are TWICE the upper end of that spread for the scalars and 1.5 x for the
# update tensors -- never below the pre-round-5 values (15 x the envelope, the arbiter's own 3 x level); without the file, those old values.
def _drift_limits():
    import json
    path = os.path.join(GOLDEN, "drift_spread_cfg3_lstm_10.json")
    scal, upd = 15.0, 1.0
    if os.path.isfile(path):
        v = json.load(open(path))["variants"]
        ratios = [r for rec in v.values() for r in rec["scalar_over_envelope"] if r is not None]
        upds = [rec[k] for rec in v.values() for k in ("worst_over_level_Dupd", "worst_over_level_Gupd") if rec.get(k) is not None]
        if ratios:
            scal = max(scal, 2.0 * max(ratios))
        if upds:
            upd = max(upd, 1.5 * max(upds) / A.ARBITER_FACTOR)
    return scal, upd


SCALAR_DRIFT_FACTOR, LONG_RUN_FACTOR = _drift_limits()      # LONG_RUN_FACTOR multiplies the arbiter's factor for update tensors of runs > 2 steps


def reference_drift_envelope(fx):
    """Per step: the largest relative distance between the reference's own float32 and float64 LOSSES (counts excluded) seen in
    that step or an earlier one -- how far two exact-arithmetic-equivalent runs of the reference itself have separated by then."""
    env, out, st = 0.0, [], 0
    while "d_scalars_%d.f64" % st in fx.files:
        for k, n in (("d_scalars_%d" % st, 3), ("g_scalars_%d" % st, 4)):
            a, b = fx[k + ".f32"][:n].astype(np.float64), fx[k + ".f64"][:n].astype(np.float64)
            env = max(env, float((np.abs(a - b) / np.maximum(np.abs(b), 1e-3)).max()))
        out.append(env)
        st += 1
    return out


def compare_with_fixture(name, got, fx, factor=A.ARBITER_FACTOR, floor=A.ARBITER_FLOOR, scalar_rtol=1e-4, measure=None, cold=False):
    """The arbiter rule of at_size.py.  `measure` (dict): collect the observed relative rms distances instead of judging
    (used to MEASURE the bf16 tolerance).  cold: update tensors are judged element-wise by judge_cold_update."""
    lines, bad = [], []
    grad_err = {}
    keys = sorted(k[:-7] for k in fx.files if k.endswith(".sample"))
    e32_of = {k: max(float(fx[k + ".err32"]), float(fx[k + ".err32_sample"])) for k in keys}
    level = {}
    for k in keys:
        level[k.split(".")[0]] = max(level.get(k.split(".")[0], 0.0), e32_of[k])
    for k in keys:
        ref = fx[k + ".sample"].astype(np.float64)
        g_full = np.asarray(got[k], dtype=np.float64)
        g = A.sample_of(k, g_full).astype(np.float64)
        assert g.shape == ref.shape, (k, g.shape, ref.shape)
        den = max(A.rms(ref), 1e-300)
        err = A.rms(g - ref) / den
        kind = k.split(".")[0]
        if kind in ("Dgrad", "Ggrad"):
            grad_err[k] = err
        if cold and kind in ("Dupd", "Gupd") and measure is None:
            continue                                       # judged below, once every gradient's error is known
        exposed = kind in ("Dgrad", "Ggrad", "Dupd", "Gupd") and not k.startswith("Dgrad.last_linear")
        e32 = max(e32_of[k], level[kind]) if exposed else e32_of[k]
        kink = A.kink_allowance(fx, "G" if kind[0] == "G" else "D", first_step=kind.endswith("grad")) if exposed else 0.0
        # Long runs (cfg3_lstm_10: ten steps): the parameter update is the integral of a trajectory that separates from the float64
        # one by the chaotic law described at SCALAR_DRIFT_FACTOR -- a random prefactor per implementation.  Measured distance of the
        # worst ten-step D update to the float64 run: the reference's own float32 7.0e-3, this engine with per-layer discriminator
        # launches 1.9e-2 (2.7x), with the fused discriminator stack 4.0e-2 (5.7x), the REAL reference with relabelled hidden units 4.1x / 5.2x / 5.9x (three seeds)
        # (drift_spread_cfg3_lstm_10.json): update tensors of runs longer than two steps get LONG_RUN_FACTOR x the arbiter's factor.
        long_run = kind in ("Dupd", "Gupd") and ("d_scalars_2.f64" in fx.files)
        lim = (LONG_RUN_FACTOR * factor if long_run else factor) * e32 + floor + kink
        # the whole tensor, through its norm: nothing outside the sample can be far off without moving it
        norm_ref = float(fx[k + ".norm"])
        norm_err = abs(float(np.sqrt((g_full * g_full).sum())) - norm_ref) / max(norm_ref, 1e-300)
        worst = float(np.abs(g - ref).max()) / max(float(np.abs(ref).max()), 1e-300)
        # EVERY element, through seeded random projections of the whole tensor ([r6], at_size.proj_of): the rms of the projection
        # differences estimates |engine - ref64| over the full tensor (chi-square with PROJ_K degrees of freedom: limit x 1.5 = four sigma)
        full_err = None
        if (k + ".proj") in fx.files:
            full_err = A.rms(A.proj_of(k, g_full) - fx[k + ".proj"]) / max(norm_ref, 1e-300)
        lines.append("%-14s %-44s rel-rms %.2e  limit %.2e (ref32 %.2e, kink %.1e)  margin x%.1f  |norm| %.2e  worst elem %.2e  full-tensor estimate %s"
                     % (name, k, err, lim, e32, kink, lim / max(err, 1e-300), norm_err, worst, "-" if full_err is None else "%.2e" % full_err))
        if measure is not None:
            measure[k] = (err, norm_err, e32)
        else:
            _RATCHET_SEEN.setdefault(name, {})[k] = err
            held = _RATCHET.get(name, {}).get(k)
            if held is not None and not _RATCHET_WRITE:
                lim_r = RATCHET_FACTOR * max(held, RATCHET_FLOOR / RATCHET_FACTOR)
                if err > lim_r:
                    bad.append(lines[-1] + "   RATCHET: held %.2e, allowed %.2e (tests/golden/at_size_ratchet.json)" % (held, lim_r))
                    continue
            if not (err <= lim and norm_err <= max(lim, 10 * floor) and worst <= 10 * lim):
                bad.append(lines[-1])
            elif full_err is not None and full_err > 1.5 * lim:
                bad.append(lines[-1] + "   FULL TENSOR: projections say %.2e > 1.5 x limit" % full_err)
    if cold and measure is None:
        for k in keys:
            if k.split(".")[0] not in ("Dupd", "Gupd"):
                continue
            amb, out_frac, med = judge_cold_update(k, got, fx, grad_err)
            lines.append("%-14s %-44s cold update: ambiguous %.2e of the sample, outliers %.2e of the rest (allowed %.0e), median error %.3f x limit"
                         % (name, k, amb, out_frac, COLD_OUTLIERS, med))
            if not (out_frac <= COLD_OUTLIERS and amb <= 0.05):
                bad.append(lines[-1])
    drift_env = reference_drift_envelope(fx)
    count_env, _c = [], 0.0
    for st in range(len(drift_env)):
        a, b = fx["d_scalars_%d.f32" % st][3:5].astype(np.float64), fx["d_scalars_%d.f64" % st][3:5].astype(np.float64)
        _c = max(_c, float((np.abs(a - b) / np.maximum(b, 1.0)).max()))
        count_env.append(_c)
    for k in sorted(k[:-4] for k in fx.files if k.endswith(".f64")):
        r64, r32, g = fx[k + ".f64"], fx[k + ".f32"], np.asarray(got[k], dtype=np.float64)
        if k.startswith("d_scalars"):
            losses, counts = slice(0, 3), slice(3, 5)
            st = int(k.rsplit("_", 1)[1])
            if measure is None and not np.array_equal(g[counts], r64[counts]):
                if len(drift_env) <= 2:
                    # a count can only differ where the reference's own float32 and float64 runs differ (D == 0.5 within rounding)
                    if np.array_equal(r32[counts], r64[counts]):
                        bad.append("%s %s counts %s != %s" % (name, k, g[counts], r64[counts]))
                else:
                    # long runs: D(x) sits within 1e-2 of 0.5 for most frames at this stage of training, so a count moves with the
                    # parameters' rounding-level drift: up to 3 frames, or SCALAR_DRIFT_FACTOR x the reference's own count drift so far
                    allowed = np.maximum(3.0, SCALAR_DRIFT_FACTOR * count_env[st] * r64[counts])
                    if st == 0 or (np.abs(g[counts] - r64[counts]) > allowed).any():
                        bad.append("%s %s counts %s vs %s (allowed +-%s)" % (name, k, g[counts], r64[counts], allowed))
        else:
            losses = slice(0, 4)
        rel = np.abs(g[losses] - r64[losses]) / np.maximum(np.abs(r64[losses]), 1e-3)
        # The scalars of LATER steps of a long run (cfg3_lstm_10): a GAN step with dropout 0.5 in D amplifies a rounding-level
        # perturbation by x3..x5 per step -- the reference's OWN float32 and float64 runs agree to 1e-7 on the first steps, to 3e-5
        # on the 6th and to 1.6e-3 on the 10th (reference_drift_envelope).  Two float32 implementations with different summation
        # orders separate by the same law with a random prefactor, so from the step on where that envelope exceeds 1e-5 the limit is
        # SCALAR_DRIFT_FACTOR x the envelope (measured: this engine sits at 1x..9x); before that, and in every one- or two-step
        # case, it is the plain 1e-4.
        ref_drift = drift_env[int(k.rsplit("_", 1)[1])]
        s_lim = max(scalar_rtol, SCALAR_DRIFT_FACTOR * ref_drift if ref_drift > 1e-5 else 0.0)
        lines.append("%-14s %-44s %s vs %s (max rel %.2e, limit %.1e)" % (name, k, np.array2string(g, precision=6), np.array2string(r64, precision=6), rel.max(), s_lim))
        if measure is not None:
            measure[k] = (float(rel.max()), 0.0, ref_drift)
        elif rel.max() > s_lim:
            bad.append(lines[-1])
    if _REPORT:
        with open(_REPORT, "a") as f:
            f.write("\n".join(lines) + "\n")
    if _RATCHET_WRITE and measure is None:
        import json
        held = json.load(open(_RATCHET_WRITE)) if os.path.isfile(_RATCHET_WRITE) else {}
        held[name] = {k: float("%.3e" % v) for k, v in sorted(_RATCHET_SEEN.get(name, {}).items())}
        with open(_RATCHET_WRITE, "w") as f:
            json.dump(held, f, indent=0, sort_keys=True)
    assert not bad, "%d quantities outside the arbiter's limit or the ratchet:\n%s" % (len(bad), "\n".join(bad))


@pytest.mark.parametrize("name", sorted(A.AT_SIZE_CASES))
def test_at_size_step_matches_fixture(name):
    """cfg3 (BiLSTM 3 x 256, B = 32, T = 1024) / cfg4 (SRU 6 x 512, B = 16, T = 2048) / cfg5 (B = 64, generator noise,
    conditioned D; acoustic pair with Adagrad and duration pair with Adam) at full size, float32 engine."""
    case = A.AT_SIZE_CASES[name]
    path = os.path.join(GOLDEN, "at_size_%s.npz" % name)
    assert os.path.isfile(path), "declared at-size case %s has no committed fixture (tests/golden/make_at_size.py %s)" % (name, name)
    fx = np.load(path)
    got = run_hip_at_size(case)
    compare_with_fixture(name, got, fx, cold=bool(case.get("cold")))


def test_cfg1_at_size_with_the_fused_discriminator_stack_forced():
    """cfg1 (VC: MLP D 25 -> 256 x 2 -> 1, unconditioned, injected masks, B = 8, T = 256) has 128 panels per D pass: below the size at
    which the fused discriminator stack is taken by default (one panel per CU).  Forced (GT_OPT_FUSED_DSTACK = 2) it must meet the
    REAL reference's fixture under the same arbiter: two hidden layers, no conditioning columns (col0 = 0), mask-buffer dropout."""
    case = A.AT_SIZE_CASES["cfg1_vc"]
    fx = np.load(os.path.join(GOLDEN, "at_size_cfg1_vc.npz"))
    got = run_hip_at_size(case, engine_options={"fused_dstack": 2})
    compare_with_fixture("cfg1_vc/fused", got, fx)


# Relative rms distance to the float64 reference with bf16 storage, per case, network and kind: MEASURED on MI355X (round 4,
# GT_PARITY_REPORT run of these tests, committed as profiles/r04_parity_report.txt) and limited at <= 2x the measurement:
#                      measured:  y_hat    y_hat_static  Ggrad    Gupd     Dgrad    Dupd     losses
#   cfg3_lstm (T = 1024)          2.3e-3   2.2e-3        3.8e-3   4.3e-3   2.1e-2   2.0e-2   < 1e-3
#   cfg5_acoustic (B = 64)        4.3e-3   3.4e-3        2.1e-2   3.8e-2   1.9e-2   1.5e-2   < 1e-3
#   cfg4_sru (B = 16, T = 2048)   3.0e-3   2.3e-3        8.9e-3   7.0e-3   9.6e-3   9.3e-3   7.1e-5   (round 5: profiles/r05_parity_report.txt;
#                                 against the ORACLE's float64 digest -- un-vendored SRU cell, parity unpinned)
BF16_LIMITS = {
    "cfg4_sru": {"y_hat": 5.9e-3, "y_hat_static": 4.6e-3, "Ggrad": 1.8e-2, "Gupd": 1.4e-2, "Dgrad": 1.9e-2, "Dupd": 1.9e-2, "scalars": 5e-3},
    "cfg3_lstm": {"y_hat": 4.6e-3, "y_hat_static": 4.4e-3, "Ggrad": 7.6e-3, "Gupd": 8.6e-3, "Dgrad": 4.2e-2, "Dupd": 4.0e-2, "scalars": 5e-3},
    "cfg5_acoustic": {"y_hat": 8.6e-3, "y_hat_static": 6.8e-3, "Ggrad": 4.2e-2, "Gupd": 7.6e-2, "Dgrad": 3.9e-2, "Dupd": 3.1e-2, "scalars": 5e-3},
}


def _judge_bf16(case_name, seen):
    worst = {}
    lim = BF16_LIMITS[case_name]
    for k, (err, norm_err, _) in seen.items():
        kind = "scalars" if "scalars" in k else k.split(".")[0]
        worst[kind] = max(worst.get(kind, 0.0), err)
        assert err <= lim[kind], "bf16 %s %s: distance %.3e > %.1e" % (case_name, k, err, lim[kind])
    assert worst["y_hat"] > 1e-5, "suspiciously exact: the bf16 path did not run"
    return worst


def test_cfg3_full_length_bf16_tracks_the_reference():
    """BASELINE.json configs[2] as it is stated: bf16 (GT_OPT_MATMUL_BF16: bf16 operands / storage of GEMM-only tensors,
    float32 accumulation, float32 master weights and state) at T = 1024 -- 1024 recurrent steps of bf16-rounded h is where
    rounding would accumulate -- against the REAL reference's float64 digest, with measured limits (BF16_LIMITS)."""
    case = A.AT_SIZE_CASES["cfg3_lstm"]
    fx = np.load(os.path.join(GOLDEN, "at_size_cfg3_lstm.npz"))
    got = run_hip_at_size(case, engine_options={"matmul_bf16": 1})
    seen = {}
    compare_with_fixture("cfg3_lstm/bf16", got, fx, measure=seen)
    _judge_bf16("cfg3_lstm", seen)


def test_cfg4_full_size_bf16_tracks_the_fixture():
    """BASELINE.json configs[3] in the dtype bench.py reports it in (VERDICT r4 missing #1): the SRU generator 6 x 512 bidirectional
    at B = 16, T = 2048 with GT_OPT_MATMUL_BF16 -- bf16-storage products for U / dW / d(input), the dropped layer input as bf16
    images only (seqdrop_cast_transpose), dU written as bf16 images by the cooperative backward scan itself (sru_bwd_cs_kernel<NW, true>),
    float32 scans -- against the float64 digest of at_size_cfg4_sru.npz (the oracle's restated cell: parity unpinned), with
    measured limits (BF16_LIMITS)."""
    case = A.AT_SIZE_CASES["cfg4_sru"]
    fx = np.load(os.path.join(GOLDEN, "at_size_cfg4_sru.npz"))
    got = run_hip_at_size(case, engine_options={"matmul_bf16": 1})
    seen = {}
    compare_with_fixture("cfg4_sru/bf16", got, fx, measure=seen)
    _judge_bf16("cfg4_sru", seen)


def test_cfg5_acoustic_bf16_storage_tracks_the_reference():
    """The MLP pair of BASELINE.json configs[4] (B = 64, T = 512, generator noise, conditioned D) with GT_OPT_MATMUL_BF16:
    bf16 storage of activations / dZ / input images / weight shadows in both networks, against the REAL reference's float64
    digest with the measured limits."""
    case = A.AT_SIZE_CASES["cfg5_acoustic"]
    fx = np.load(os.path.join(GOLDEN, "at_size_cfg5_acoustic.npz"))
    got = run_hip_at_size(case, engine_options={"matmul_bf16": 1})
    seen = {}
    compare_with_fixture("cfg5_acoustic/bf16", got, fx, measure=seen)
    _judge_bf16("cfg5_acoustic", seen)


# Ten steps of cfg3 with bf16 storage, distance of the losses to the float64 reference by step and of the parameter updates after the
# tenth: MEASURED on MI355X (round 4, profiles/r04_parity_report.txt), limits at 2x the measurement:
#   losses by step   3.3e-5  3.9e-5  4.8e-5  3.7e-5  4.9e-5  2.4e-4  5.1e-4  1.6e-3  6.2e-3  3.3e-2      Gupd 8.1e-3   Dupd 7.5e-2
#   the reference's own float32-vs-float64 envelope (reference_drift_envelope):
#                    9.6e-8  1.1e-7  1.3e-7  2.0e-6  2.0e-6  2.8e-5  3.3e-5  3.3e-5  1.4e-4  1.6e-3
# Both grow by x3..x5 per step from the 5th step on: the step amplifies ANY perturbation at that rate (dropout 0.5 in D, Adagrad on
# fresh accumulators); bf16's 2^-8 roundings enter ~350x above float32's drift and stay 10x..50x above it -- they do not compound faster.
TEN_STEP_LIMITS = {"scalars_by_step": [7e-5, 8e-5, 1e-4, 8e-5, 1e-4, 5e-4, 1.1e-3, 3.2e-3, 1.3e-2, 6.6e-2], "Gupd": 1.7e-2, "Dupd": 1.5e-1,
                   "over_reference_drift": 100.0}


@pytest.mark.skipif(not os.path.isfile(os.path.join(GOLDEN, "at_size_cfg3_lstm_10.npz")), reason="ten-step digest not generated")
def test_cfg3_ten_steps_bf16_error_growth():
    """TEN G+D steps of cfg3 at T = 1024 with bf16 storage against the REAL reference's ten-step float64
    digest -- where a rounding bias of the bf16 path would compound: 10 240 recurrent steps of bf16-rounded h, ten optimizer
    updates built on bf16-rounded gradients.  Judged: the losses of EVERY step and the parameter updates after the tenth, with
    limits at about 2x the measured distances; the float32 engine on the same ten steps must stay under the arbiter's rule."""
    case = A.AT_SIZE_CASES["cfg3_lstm_10"]
    fx = np.load(os.path.join(GOLDEN, "at_size_cfg3_lstm_10.npz"))
    got = run_hip_at_size(case, engine_options={"matmul_bf16": 1})
    seen = {}
    compare_with_fixture("cfg3_lstm_10/bf16", got, fx, measure=seen)
    by_step = []
    for st in range(case["steps"]):
        by_step.append(max(seen["d_scalars_%d" % st][0], seen["g_scalars_%d" % st][0]))
    upd = {k: max(v[0] for q, v in seen.items() if q.startswith(k + ".")) for k in ("Gupd", "Dupd")}
    if _REPORT:
        with open(_REPORT, "a") as f:
            f.write("cfg3_lstm_10/bf16 loss distance by step: %s; updates after 10 steps: %s\n" % (["%.2e" % v for v in by_step], upd))
    env = reference_drift_envelope(fx)
    for st, v in enumerate(by_step):
        assert v <= TEN_STEP_LIMITS["scalars_by_step"][st], "step %d: loss distance %.2e: %s" % (st, v, by_step)
        # no faster than float32's own drift: once that drift is above the float32 rounding floor, bf16 stays within two orders of magnitude of it
        assert st < 3 or v <= TEN_STEP_LIMITS["over_reference_drift"] * env[st], "step %d: %.2e vs the reference's own drift %.2e" % (st, v, env[st])
    assert upd["Gupd"] <= TEN_STEP_LIMITS["Gupd"] and upd["Dupd"] <= TEN_STEP_LIMITS["Dupd"], upd
