"""References of the adversarial objectives (GT_OPT_GAN_OBJECTIVE: "bce", "ls", "hinge", "wgan") for tests/test_gan_objective_host.py
and tests/test_gpu_gan_objective.py.  Nothing here needs a GPU.

Two levels:
  * per frame, in float64: phi (the frame's loss term), its derivative in z, D(x) and the "correct" threshold -- the table of
    include/gantts_hip.h -- with the error bounds of the float32 sequences of gantts_amd/csrc/gan_objective.hip.h carried beside them
    (`head_math`: the drop-in for tests/test_gpu_d_tail.py's head_math, same keys);
  * per step, in torch on the CPU: `update_discriminator` / `update_generator` restate oracle/gantts_oracle.py's two functions
    (reference train.py:245-320: generated features not detached, retain_graph, the G step on the updated D) with phi swapped and the
    WGAN clamp behind optimizer_d.step(); models, MLPG, masks, clip_grad_norm_ and optimizers are the oracle's own.  With "bce" these are
    the oracle's torch operations one for one (tests/test_gan_objective_host.py ties them bit for bit).
`mistake=` plants one of MISTAKES in either level: what the comparators of the GPU test must reject."""
import numpy as np
import torch

import cases as C
import gantts_oracle as O

OBJECTIVES = ("bce", "ls", "hinge", "wgan")
IDS = {"bce": 0, "ls": 1, "hinge": 2, "wgan": 3}
THRESHOLD = {"bce": 0.5, "ls": 0.5, "hinge": 0.0, "wgan": 0.0}
U = 2.0 ** -24          # half an ulp of a float32, relative
MISTAKES = ("fake_sign_flipped", "ls_half_missing", "hinge_derivative_beyond_kink", "g_rows_scored_as_generated", "wgan_threshold_half",
            "clamp_before_update")


# ---------------------------------------------------------------------------------------------------------------------
# per frame, float64
# ---------------------------------------------------------------------------------------------------------------------
def _kind(real, g_mode, mistake):
    """0: scored against the "natural" label in the D step, 1: a generated row of the D step, 2: a row of the G step."""
    real = np.asarray(real, dtype=bool)
    if g_mode:
        return np.full(real.shape, 1 if mistake == "g_rows_scored_as_generated" else 2)
    return np.where(real, 0, 1)


def phi(obj, z, real, g_mode, eps=1e-20, mistake=None):
    """The frame's loss term (numpy float64, or torch float64 when z is a tensor: the autograd check differentiates this very function)."""
    tz = isinstance(z, torch.Tensor)
    k = _kind(real, g_mode, mistake)
    k = torch.from_numpy(np.ascontiguousarray(k)) if tz else k
    where = torch.where if tz else np.where
    relu = (lambda t: torch.clamp(t, min=0.0)) if tz else (lambda t: np.maximum(t, 0.0))
    half = 1.0 if mistake == "ls_half_missing" else 0.5
    sgn = -1.0 if mistake == "fake_sign_flipped" else 1.0
    if obj == "bce":
        D = torch.sigmoid(z) if tz else 1.0 / (1.0 + np.exp(-z))
        log = torch.log if tz else np.log
        return where(k == 1, -sgn * log(1.0 - D + eps), -log(D + eps))
    if obj == "ls":
        return where(k == 1, sgn * half * z * z, half * (z - 1.0) * (z - 1.0))
    if obj == "hinge":
        return where(k == 0, relu(1.0 - z), where(k == 1, relu(1.0 + sgn * z), -z))
    if obj == "wgan":
        return where(k == 1, sgn * z, -z)
    raise ValueError(obj)


def dphi(obj, z, real, g_mode, eps=1e-20, mistake=None):
    """d phi / d z, closed form, numpy float64 (the hinge's derivative at a kink is 0, as torch's relu)."""
    z = np.asarray(z, dtype=np.float64)
    k = _kind(real, g_mode, mistake)
    sgn = -1.0 if mistake == "fake_sign_flipped" else 1.0
    half = 1.0 if mistake == "ls_half_missing" else 0.5
    if obj == "bce":
        D = 1.0 / (1.0 + np.exp(-z))
        return np.where(k == 1, sgn / (1.0 - D + eps), -1.0 / (D + eps)) * D * (1.0 - D)
    if obj == "ls":
        return np.where(k == 1, sgn * 2.0 * half * z, 2.0 * half * (z - 1.0))
    if obj == "hinge":
        beyond = mistake == "hinge_derivative_beyond_kink"
        dr = np.where((z < 1.0) | beyond, -1.0, 0.0)
        df = np.where((sgn * z > -1.0) | beyond, sgn, 0.0)
        return np.where(k == 0, dr, np.where(k == 1, df, -1.0))
    if obj == "wgan":
        return np.where(k == 1, sgn, -1.0)
    raise ValueError(obj)


def threshold(obj, mistake=None):
    return 0.5 if (obj == "wgan" and mistake == "wgan_threshold_half") else THRESHOLD[obj]


def kinks(obj, real, g_mode):
    """Per frame, the z values at which something the GPU test compares exactly (a count) or without an either-side allowance (the
    hinge's derivative) jumps: rows x points, NaN where a frame has fewer points.  The G step has no counts and no kink."""
    real = np.asarray(real, dtype=bool)
    n = real.shape[0]
    pts = np.full((n, 2), np.nan)
    if g_mode:
        return pts
    pts[:, 0] = THRESHOLD[obj] if obj != "bce" else 0.0          # D = sigmoid(z) crosses 0.5 at z = 0
    if obj == "hinge":
        pts[:, 1] = np.where(real, 1.0, -1.0)
    return pts


def head_math(obj, mode_g, n_real, n_mask, h, Eh, w, bias, mask, inv_tv, mistake=None):
    """The head of objectives 1 .. 3 on h [rows][K] (float64, carrying the bound Eh), with the keys tests/test_gpu_d_tail.py's head_math
    returns: z = <h, w> + b with E_z from the product; D = z; lt = -phi m (the addend of s_real / s_fake) and dz = phi' m inv_tv with
    bounds |phi'| E_z (+ E_z^2 / 2 for the squares) plus one float32 rounding per operation of the kernel's sequence:
      ls     d = z - 1; addend = -(0.5 (d d)) m: 2 roundings (0.5 x and x m, m in {0, 1}, are exact);  dz = d u: 2 (d, the product)
      hinge  t = 1 -+ z; addend = -max(0, t) m: 1;  dz = -+u or 0: exact given u
      wgan   addend = -+z m, dz = -+u: exact given z and u
    u = m inv_tv is exact for a 0 / 1 mask.  Away from the kinks (the input condition) the hinge's bound holds on its own side."""
    assert obj in ("ls", "hinge", "wgan")
    f8 = np.float64
    rows, K = h.shape
    m = mask[np.arange(rows) % n_mask].astype(f8)
    z = h @ w + bias
    Sz = np.abs(h) @ np.abs(w) + abs(bias)
    Ez = (K + 2) * U * Sz + Eh @ np.abs(w)
    real = np.ones(rows, dtype=bool) if mode_g else (np.arange(rows) < n_real)
    p = phi(obj, z, real, mode_g, mistake=mistake)
    dp = dphi(obj, z, real, mode_g, mistake=mistake)
    lt = -p * m
    dz = dp * m * inv_tv
    curv = 0.5 if obj == "ls" else 0.0                                   # |phi''| / 2
    Ephi = np.abs(dp) * Ez + curv * Ez * Ez + 3 * U * (np.abs(p) + np.abs(dp) * Ez)
    El = m * Ephi
    Edz = np.abs(m * inv_tv) * (2.0 * curv * Ez) + 3 * U * np.abs(dz)
    return dict(z=z, Ez=Ez, D=z, ED=Ez, m=m, real=real, lt=lt, El=El, dz=dz, Edz=Edz)


def counts(obj, q, mode_g, mistake=None):
    """(n_real_ok, n_fake_ok) of a D-step pass from head_math's dict."""
    if mode_g:
        return None
    thr = threshold(obj, mistake)
    return float(((q["D"] > thr) * q["m"])[q["real"]].sum()), float(((q["D"] < thr) * q["m"])[~q["real"]].sum())


# ---------------------------------------------------------------------------------------------------------------------
# per step, torch on the CPU (the oracle's operations with phi swapped)
# ---------------------------------------------------------------------------------------------------------------------
def _phi_real(obj, D, eps, mistake=None):
    half = 1.0 if mistake == "ls_half_missing" else 0.5
    if obj == "bce":
        return -torch.log(D + eps)
    if obj == "ls":
        return half * (D - 1) ** 2
    if obj == "hinge":
        return torch.relu(1 - D)
    return -D


def _phi_fake(obj, D, eps, mistake=None):
    half = 1.0 if mistake == "ls_half_missing" else 0.5
    sgn = -1.0 if mistake == "fake_sign_flipped" else 1.0
    if obj == "bce":
        return -torch.log(1 - D + eps) if sgn > 0 else torch.log(1 - D + eps)
    if obj == "ls":
        return sgn * half * D ** 2
    if obj == "hinge":
        return torch.relu(1 + sgn * D)
    return sgn * D


def _phi_g(obj, D, eps, mistake=None):
    if mistake == "g_rows_scored_as_generated":
        return _phi_fake(obj, D, eps)
    if obj == "bce":
        return -torch.log(D + eps)
    if obj == "ls":
        return 0.5 * (D - 1) ** 2
    return -D


def clamp_(params, c):
    if c > 0:
        with torch.no_grad():
            for p in params:
                p.clamp_(-c, c)


def update_discriminator(obj, cfg, model_d, optimizer_d, x, y_static, y_hat_static, lengths, mask, phase, eps=1e-20, drop=None, clip=0.0,
                         mistake=None):
    """oracle.update_discriminator (train.py:245-279) with the objective's terms; the WGAN clamp follows optimizer_d.step()."""
    real_in = O._adv_input(cfg, x, y_static)
    fake_in = O._adv_input(cfg, x, y_hat_static)
    Tv = mask.sum().item()
    thr = threshold(obj, mistake)
    D_real = model_d(real_in, lengths=lengths, drop=drop)
    real_correct = ((D_real > thr).float() * mask).sum().item()
    D_fake = model_d(fake_in, lengths=lengths, drop=drop)
    fake_correct = ((D_fake < thr).float() * mask).sum().item()
    if obj == "bce" and mistake is None:        # the oracle's own expressions, operation for operation
        loss_real = -(torch.log(D_real + eps) * mask).sum() / Tv
        loss_fake = -(torch.log(1 - D_fake + eps) * mask).sum() / Tv
    else:
        loss_real = (_phi_real(obj, D_real, eps, mistake) * mask).sum() / Tv
        loss_fake = (_phi_fake(obj, D_fake, eps, mistake) * mask).sum() / Tv
    loss_d = loss_real + loss_fake
    if phase == "train":
        loss_d.backward(retain_graph=True)
        if mistake == "clamp_before_update":
            clamp_(model_d.params, clip)
        O.clip_grad_norm_(model_d.params, 1.0)
        optimizer_d.step()
        if mistake != "clamp_before_update":
            clamp_(model_d.params, clip)
    return loss_d.item(), loss_fake.item(), loss_real.item(), real_correct, fake_correct


def update_generator(obj, cfg, model_g, model_d, optimizer_g, x, y, y_hat, y_static, y_hat_static, adv_w, lengths, mask, phase, mse_w=None,
                     mge_w=None, eps=1e-20, drop=None, mistake=None):
    """oracle.update_generator (train.py:282-320) with the objective's adversarial term, through the ALREADY UPDATED (and clamped) D."""
    local_tv = mask.sum()
    Tv = local_tv.item()
    loss_mge = O.masked_mse(y_hat_static, y_static, mask) * (local_tv / Tv)
    loss_mse = O.masked_mse(y_hat, y, mask) * (local_tv / Tv)
    if adv_w > 0:
        fake_in = O._adv_input(cfg, x, y_hat_static)
        D = model_d(fake_in, lengths=lengths, drop=drop)
        if obj == "bce" and mistake is None:
            loss_adv = -(torch.log(D + eps) * mask).sum() / Tv
        else:
            loss_adv = (_phi_g(obj, D, eps, mistake) * mask).sum() / Tv
    else:
        loss_adv = torch.zeros(1)
    loss_g = (mse_w * loss_mse + mge_w * loss_mge) + adv_w * loss_adv
    if phase == "train":
        loss_g.backward()
        O.clip_grad_norm_(model_g.params, 1.0)
        optimizer_g.step()
    return loss_mse.item(), loss_mge.item(), loss_adv.item(), loss_g.item()


def run_step_reference(case, obj="bce", clip=0.0, mistake=None, snapshots=None):
    """tests/oracle_runner.py's run_oracle_case with the two update functions above; same keys.  snapshots: a list that receives the
    discriminator's state_dict (numpy) behind every D step."""
    from oracle_runner import build_oracle_model, stream_config
    cfg = stream_config(case)
    mg, md = build_oracle_model(case["g"], 11, case.get("saturate_gates", False)), build_oracle_model(case["d"], 22)
    mg.training = md.training = bool(case["dropout_on"])
    og = O.make_optimizer(case["opt_g"][0], mg.params, **case["opt_g"][1])
    od = O.make_optimizer(case["opt_d"][0], md.params, **case["opt_d"][1])
    x_np, y_np, lengths = C.make_batch(case)
    x, y = torch.from_numpy(x_np), torch.from_numpy(y_np)
    T = case["T"]
    has_dyn = bool(np.any(case["has_dynamic_features"]))
    R = torch.from_numpy(O.unit_variance_mlpg_matrix(C.WINDOWS[:case["windows"]], T)) if has_dyn else None
    mask = O.sequence_mask(lengths).unsqueeze(-1)
    out = {}
    for step in range(case["steps"]):
        dg = dd = None
        if case["dropout_on"]:
            gm, dm = C.make_dropout_masks(case, step)
            dg = O._DropoutSource([torch.from_numpy(m) for m in gm])
            dd = O._DropoutSource([torch.from_numpy(m) for m in dm])
        y_static = O.get_static_features(y, cfg.num_windows, cfg.stream_sizes, cfg.has_dynamic_features)
        og.zero_grad(), od.zero_grad()
        y_hat, y_hat_static = O.apply_generator(cfg, mg, x, R, list(lengths), drop=dg)
        if step == 0:
            out["y_hat"] = y_hat.detach().numpy().copy()
            out["y_hat_static"] = y_hat_static.detach().numpy().copy()
        if case["update_d"]:
            res = update_discriminator(obj, cfg, md, od, x, y_static, y_hat_static, list(lengths), mask, "train", drop=dd, clip=clip,
                                       mistake=mistake)
            out["d_scalars_%d" % step] = np.array(res, dtype=np.float64)
            gn = [p.grad for p in mg.params if p.grad is not None]
            out["g_leak_norm_%d" % step] = np.array(float(torch.sqrt(sum((g ** 2).sum() for g in gn))) if gn else 0.0)
            if snapshots is not None:
                snapshots.append({"D." + k: v.numpy().copy() for k, v in md.state_dict().items()})
        if case["update_g"]:
            res = update_generator(obj, cfg, mg, md, og, x, y, y_hat, y_static, y_hat_static, case["adv_w"], list(lengths), mask, "train",
                                   mse_w=case["mse_w"], mge_w=case["mge_w"], drop=dd, mistake=mistake)
            out["g_scalars_%d" % step] = np.array(res, dtype=np.float64)
    for k, v in mg.state_dict().items():
        out["G." + k] = v.numpy()
    for k, v in md.state_dict().items():
        out["D." + k] = v.numpy()
    for tag, opt, model in (("G", og, mg), ("D", od, md)):
        for i, name in enumerate(model.names):
            if isinstance(opt, O.OracleAdagrad):
                out["%s.opt.sum.%s" % (tag, name)] = opt.sum[i].numpy()
            elif opt.step_count:
                out["%s.opt.exp_avg.%s" % (tag, name)] = opt.m[i].numpy()
                out["%s.opt.exp_avg_sq.%s" % (tag, name)] = opt.v[i].numpy()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the step cases of the GPU test: generator MLP; B = 3, T = 24, ragged lengths, injected dropout masks
# ---------------------------------------------------------------------------------------------------------------------
_G = dict(kind="MLP", in_dim=30, out_dim=187, num_hidden=2, hidden_dim=32, dropout=0.5, last_sigmoid=False)
# Adagrad with a non-zero initial accumulator (as the at-size goldens of tests/golden/cases.py): with 0 the first update is
# lr * sign(g), discontinuous at g = 0 -- and under "hinge" / "wgan" every row's seed is +-m / Tv, so the gradient of a top-layer unit is
# m / Tv * w_k times a difference of two sums of activation slopes, which is exactly 0 whenever they balance: its float32 sign is noise.
_ADG = ("Adagrad", dict(lr=0.01, weight_decay=1e-7, initial_accumulator_value=1e-4))


def _step_case(d, cond, fused=False):
    in_dim = 58 + (30 if cond else 0)
    return dict(hp="tts_acoustic", B=3, T=24, din=30, dout=187, stream_sizes=[180, 3, 1, 3], has_dynamic_features=[True, True, False, True],
                adversarial_streams=[True, False, False, False], mask_nth_mgc=2, cond=cond, g=dict(_G),
                d=dict(dict(out_dim=1, last_sigmoid=False, in_dim=in_dim), **d), opt_g=_ADG, opt_d=_ADG, windows=3, steps=2, adv_w=1.0,
                mse_w=0.0, mge_w=1.0, dropout_on=True, update_d=True, update_g=True, fused=fused)


STEP_CASES = {
    "mlp32": _step_case(dict(kind="MLP", num_hidden=3, hidden_dim=32, dropout=0.5), False),                  # the per-layer head
    "mlp128_fused": _step_case(dict(kind="MLP", num_hidden=3, hidden_dim=128, dropout=0.5), False, fused=True),
    "lstm": _step_case(dict(kind="LSTMRNN", num_hidden=2, hidden_dim=12, bidirectional=True, dropout=0.0), False),
    "sru": _step_case(dict(kind="SRURNN", num_hidden=2, hidden_dim=12, bidirectional=True, dropout=0.0, rnn_dropout=0.0, use_relu=1), False),
    "mlp32_cond": _step_case(dict(kind="MLP", num_hidden=3, hidden_dim=32, dropout=0.5), True),                # discriminator_linguistic_condition
}


def bce_twin(case):
    """The same case with the reference's discriminator (last_sigmoid=True): what "bce" runs."""
    return dict(case, d=dict(case["d"], last_sigmoid=True))


def step_close(got, ref, rtol=1e-4):
    """The suite's comparison of a whole run (tests/test_gpu_parity.py: 1e-4 relative on each tensor's scale, second moments on the
    scale of their square root, classification counts exactly); returns the list of keys that miss."""
    from test_gpu_parity import _scale_of
    bad = []
    for k, r in ref.items():
        if k.startswith("g_leak_norm"):
            continue
        if k not in got:
            bad.append(k + " (missing)")
            continue
        g, r = np.asarray(got[k], dtype=np.float64), np.asarray(r, dtype=np.float64)
        atol = 1e-6
        if ".opt.sum." in k or ".opt.exp_avg_sq." in k:
            g, r, atol = np.sqrt(np.maximum(g, 0.0)), np.sqrt(np.maximum(r, 0.0)), 1e-9
        elif ".opt." in k:
            atol = 1e-9
        if g.shape != r.shape or not np.all(np.abs(g - r) <= atol + rtol * _scale_of(r, k)):
            bad.append(k)
        if k.startswith("d_scalars") and (g[3] != r[3] or g[4] != r[4]):
            bad.append(k + " (counts)")
    return bad
