"""References of the f-GAN divergences (GT_OPT_GAN_OBJECTIVE 4 kl, 5 rkl, 6 js; Nowozin et al. 2016) for tests/test_gan_fdiv_host.py and
tests/test_gpu_gan_fdiv.py, in the layout of tests/gan_objective_ref.py.  Nothing here needs a GPU.

With z the frame's output pre-activation, sp(x) = max(x, 0) + log(1 + exp(-|x|)):
    name   real row phi      generated row, D step   generated row, G step   threshold on z
    kl     -z                exp(z - 1)              -z                      1
    rkl    exp(-z)           z - 1                   exp(-z)                 0
    js     sp(-z) - ln 2     sp(z) - ln 2            sp(-z) - ln 2           0
which is the negative of the variational bound E_real g_f(v) - E_fake f*(g_f(v)) with the paper's output activations g_f and conjugates
f* (GF, FSTAR, F below restate them; tests/test_gan_fdiv_host.py ties the table to them), the G step in the non-saturating form.

Two levels, as in gan_objective_ref:
  * per frame, in float64: phi, dphi, threshold, kinks, counts, and `head_math` with the error bounds of the float32 sequences of
    gantts_amd/csrc/gan_objective.hip.h carried beside the values;
  * per step: `update_discriminator` / `update_generator` restate gan_objective_ref's two functions with phi swapped;
    `run_step_reference` runs gan_objective_ref.run_step_reference with them put in its place (`installed`, the way
    tests/grad_penalty_ref.py wraps the same function), so models, MLPG, masks, clip_grad_norm_, optimizers and the clamp are the oracle's own,
    and the references of the spectral normalisation and the gradient penalties, which call through gan_objective_ref, compose with it.
`mistake=` plants one of MISTAKES."""
import contextlib
import math

import numpy as np
import torch

import gan_objective_ref as G
import gantts_oracle as O
from test_gpu_d_tail import LOG_ULPS, SIG_ULPS

OBJECTIVES = ("kl", "rkl", "js")
IDS = {"kl": 4, "rkl": 5, "js": 6}
THRESHOLD = {"kl": 1.0, "rkl": 0.0, "js": 0.0}
U = G.U
LN2 = math.log(2.0)
MISTAKES = ("kl_exp_unshifted", "rkl_generated_unshifted", "js_ln2_missing", "kl_threshold_zero", "g_rows_scored_as_generated",
            "js_generated_derivative_sign")

# f-GAN's own ingredients (Nowozin et al. 2016, tables 1, 2 and 6): the generator function f of D_f(P || Q) = sum Q f(P / Q), its derivative, its
# conjugate f*, the output activation g_f and g_f's inverse.  float64 numpy.
F = {"kl": lambda u: u * np.log(u), "rkl": lambda u: -np.log(u), "js": lambda u: u * np.log(u) - (u + 1.0) * np.log(0.5 * (u + 1.0))}
FPRIME = {"kl": lambda u: 1.0 + np.log(u), "rkl": lambda u: -1.0 / u, "js": lambda u: np.log(2.0 * u / (1.0 + u))}
FSTAR = {"kl": lambda t: np.exp(t - 1.0), "rkl": lambda t: -1.0 - np.log(-t), "js": lambda t: -np.log(2.0 - np.exp(t))}
GF = {"kl": lambda v: v, "rkl": lambda v: -np.exp(-v), "js": lambda v: LN2 - np.log1p(np.exp(-v))}
GF_INV = {"kl": lambda t: t, "rkl": lambda t: -np.log(-t), "js": lambda t: -np.log(np.expm1(LN2 - t))}


# ---------------------------------------------------------------------------------------------------------------------
# per frame, float64
# ---------------------------------------------------------------------------------------------------------------------
def _sp(x):
    if isinstance(x, torch.Tensor):      # torch's own softplus: autograd of max(x, 0) + log1p(exp(-|x|)) is a subgradient at x = 0, not 1 / 2
        return torch.nn.functional.softplus(x, threshold=700.0 if x.dtype == torch.float64 else 30.0)      # (beyond it: x itself, exactly)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def phi(obj, z, real, g_mode, mistake=None):
    """The frame's loss term (numpy float64, or torch float64 when z is a tensor: the autograd check differentiates this very function)."""
    tz = isinstance(z, torch.Tensor)
    k = G._kind(real, g_mode, mistake)           # 0 real row of the D step, 1 generated row of the D step, 2 row of the G step
    k = torch.from_numpy(np.ascontiguousarray(k)) if tz else k
    where, exp = (torch.where, torch.exp) if tz else (np.where, np.exp)
    if obj == "kl":
        return where(k == 1, exp(z if mistake == "kl_exp_unshifted" else z - 1.0), -z)
    if obj == "rkl":
        return where(k == 1, z if mistake == "rkl_generated_unshifted" else z - 1.0, exp(-z))
    if obj == "js":
        c = 0.0 if mistake == "js_ln2_missing" else LN2
        return where(k == 1, _sp(z) - c, _sp(-z) - c)
    raise ValueError(obj)


def dphi(obj, z, real, g_mode, mistake=None):
    """d phi / d z, closed form, numpy float64."""
    z = np.asarray(z, dtype=np.float64)
    k = G._kind(real, g_mode, mistake)
    if obj == "kl":
        return np.where(k == 1, np.exp(z if mistake == "kl_exp_unshifted" else z - 1.0), -1.0)
    if obj == "rkl":
        return np.where(k == 1, 1.0, -np.exp(-z))
    if obj == "js":
        sgn = -1.0 if mistake == "js_generated_derivative_sign" else 1.0
        return np.where(k == 1, sgn * _sigmoid(z), -_sigmoid(-z))
    raise ValueError(obj)


def threshold(obj, mistake=None):
    return 0.0 if (obj == "kl" and mistake == "kl_threshold_zero") else THRESHOLD[obj]


def kinks(obj, real, g_mode):
    """Per frame, the z values at which a count (compared exactly) jumps: rows x 1, NaN for the G step, which counts nothing.  kl's
    jumps at z = 1.  No phi of this family has a kink."""
    n = np.asarray(real).shape[0]
    return np.full((n, 1), np.nan if g_mode else THRESHOLD[obj])


def head_math(obj, mode_g, n_real, n_mask, h, Eh, w, bias, mask, inv_tv, mistake=None):
    """The head of objectives 4 .. 6 on h [rows][K] (float64, carrying the bound Eh), with the keys of gan_objective_ref.head_math:
    z = <h, w> + b with E_z from the product; D = z; lt = -phi m and dz = phi' m inv_tv, each with an ABSOLUTE bound: the
    exact function's change over E_z plus one float32 rounding (U relative) per operation of the kernel's sequence, expf within
    SIG_ULPS U of its result and logf within LOG_ULPS U (1 + |log|) -- the allowances tests/test_gpu_d_tail.py grants objective 0 for the
    same two functions (LOG_ULPS covers the rounding of logf's argument as well).  u = m inv_tv and x m are exact for a 0 / 1 mask.
      kl   generated  t = z - 1 (d = E_z + U |z - 1|); e = expf(t): E_e = e expm1(d) + SIG_ULPS U e exp(d); phi = e; dz = e u: + U
           real / G   phi = -z: E_z; dz = -u: exact
      rkl  real / G   e = expf(-z): the same with d = E_z; dz = -(e u): + U
           generated  phi = z - 1: E_z + U (|z - 1| + E_z); dz = u: exact
      js   x = -+z; l = logf(1 + expf(-|z|)); r = max(x, 0); phi = (r + l) - ln2f.  sp is 1-Lipschitz with |sp''| <= 1 / 4: the exact
           function moves by at most sigmoid(x) E_z + E_z^2 / 8.  Roundings at the float32 point: expf SIG_ULPS U e (the log's slope at
           1 + e is below 1), logf LOG_ULPS U (1 + l), the sum U (r + l), the difference U (r + l + ln 2), ln2f itself U ln 2 -- on
           the magnitudes of the terms, NOT on phi, which is 0 at z = 0 by cancellation.
           dz = -+u / (1 + expf(-x)): the sigmoid's sequence, 0.25 E_z |u| + SIG_ULPS U |dz| as test_gpu_d_tail bounds D."""
    assert obj in OBJECTIVES
    f8 = np.float64
    rows, K = h.shape
    m = mask[np.arange(rows) % n_mask].astype(f8)
    z = h @ w + bias
    Sz = np.abs(h) @ np.abs(w) + abs(bias)
    Ez = (K + 2) * U * Sz + Eh @ np.abs(w)
    real = np.ones(rows, dtype=bool) if mode_g else (np.arange(rows) < n_real)
    k = G._kind(real, mode_g, None)
    p = phi(obj, z, real, mode_g, mistake=mistake)
    dp = dphi(obj, z, real, mode_g, mistake=mistake)
    u = np.abs(m * inv_tv)
    if obj in ("kl", "rkl"):
        expo = (k == 1) if obj == "kl" else (k != 1)                # the rows that go through expf
        t = z - 1.0 if obj == "kl" else -z
        d = Ez + (U * np.abs(t) if obj == "kl" else 0.0)
        e = np.exp(t)
        Ee = e * np.expm1(d) + SIG_ULPS * U * e * np.exp(d)
        lin = U * (np.abs(z - 1.0) + Ez) if obj == "rkl" else 0.0   # the linear rows: rkl's z - 1 is one rounding, kl's -z none
        Ephi = np.where(expo, Ee, Ez + lin)
        Edz = np.where(expo, u * Ee + U * u * (e + Ee), 0.0)
    else:
        x = np.where(k == 1, z, -z)
        a = np.abs(z)
        e, r = np.exp(-a), np.maximum(x, 0.0)
        l = np.log1p(e)
        Ephi = _sigmoid(x) * Ez + 0.125 * Ez * Ez \
            + (1.0 + 4.0 * U) * (SIG_ULPS * U * e + LOG_ULPS * U * (1.0 + l) + U * (r + l + Ez) + U * (r + l + Ez + LN2) + U * LN2)
        Edz = u * 0.25 * Ez + SIG_ULPS * U * u * _sigmoid(x)
    lt = -p * m
    dz = dp * m * inv_tv
    return dict(z=z, Ez=Ez, D=z, ED=Ez, m=m, real=real, lt=lt, El=m * Ephi, dz=dz, Edz=Edz)


def counts(obj, q, mode_g, mistake=None):
    """(n_real_ok, n_fake_ok) of a D-step pass from head_math's dict."""
    if mode_g:
        return None
    thr = threshold(obj, mistake)
    return float(((q["D"] > thr) * q["m"])[q["real"]].sum()), float(((q["D"] < thr) * q["m"])[~q["real"]].sum())


# ---------------------------------------------------------------------------------------------------------------------
# per step, torch on the CPU: gan_objective_ref's two functions with phi swapped
# ---------------------------------------------------------------------------------------------------------------------
def _t_phi(obj, D, kind, mistake=None):
    """phi on a torch tensor D = z for rows of one kind (0 real, 1 generated in the D step, 2 G step)."""
    if kind == 2 and mistake == "g_rows_scored_as_generated":
        kind = 1
    if obj == "kl":
        return torch.exp(D if mistake == "kl_exp_unshifted" else D - 1) if kind == 1 else -D
    if obj == "rkl":
        return (D if mistake == "rkl_generated_unshifted" else D - 1) if kind == 1 else torch.exp(-D)
    if obj == "js":
        c = 0.0 if mistake == "js_ln2_missing" else LN2
        return _sp(D if kind == 1 else -D) - c
    raise ValueError(obj)


_G_UPDATE_D, _G_UPDATE_G = G.update_discriminator, G.update_generator


def update_discriminator(obj, cfg, model_d, optimizer_d, x, y_static, y_hat_static, lengths, mask, phase, eps=1e-20, drop=None, clip=0.0,
                         mistake=None):
    """gan_objective_ref.update_discriminator with the divergence's terms (any other objective goes to that function itself)."""
    if obj not in OBJECTIVES:
        return _G_UPDATE_D(obj, cfg, model_d, optimizer_d, x, y_static, y_hat_static, lengths, mask, phase, eps=eps, drop=drop, clip=clip,
                           mistake=mistake)
    real_in = O._adv_input(cfg, x, y_static)
    fake_in = O._adv_input(cfg, x, y_hat_static)
    Tv = mask.sum().item()
    thr = threshold(obj, mistake)
    D_real = model_d(real_in, lengths=lengths, drop=drop)
    real_correct = ((D_real > thr).float() * mask).sum().item()
    D_fake = model_d(fake_in, lengths=lengths, drop=drop)
    fake_correct = ((D_fake < thr).float() * mask).sum().item()
    loss_real = (_t_phi(obj, D_real, 0, mistake) * mask).sum() / Tv
    loss_fake = (_t_phi(obj, D_fake, 1, mistake) * mask).sum() / Tv
    loss_d = loss_real + loss_fake
    if phase == "train":
        loss_d.backward(retain_graph=True)
        O.clip_grad_norm_(model_d.params, 1.0)
        optimizer_d.step()
        G.clamp_(model_d.params, clip)
    return loss_d.item(), loss_fake.item(), loss_real.item(), real_correct, fake_correct


def update_generator(obj, cfg, model_g, model_d, optimizer_g, x, y, y_hat, y_static, y_hat_static, adv_w, lengths, mask, phase, mse_w=None,
                     mge_w=None, eps=1e-20, drop=None, mistake=None):
    """gan_objective_ref.update_generator with the divergence's non-saturating term, through the already updated D."""
    if obj not in OBJECTIVES:
        return _G_UPDATE_G(obj, cfg, model_g, model_d, optimizer_g, x, y, y_hat, y_static, y_hat_static, adv_w, lengths, mask, phase,
                           mse_w=mse_w, mge_w=mge_w, eps=eps, drop=drop, mistake=mistake)
    local_tv = mask.sum()
    Tv = local_tv.item()
    loss_mge = O.masked_mse(y_hat_static, y_static, mask) * (local_tv / Tv)
    loss_mse = O.masked_mse(y_hat, y, mask) * (local_tv / Tv)
    if adv_w > 0:
        D = model_d(O._adv_input(cfg, x, y_hat_static), lengths=lengths, drop=drop)
        loss_adv = (_t_phi(obj, D, 2, mistake) * mask).sum() / Tv
    else:
        loss_adv = torch.zeros(1)
    loss_g = (mse_w * loss_mse + mge_w * loss_mge) + adv_w * loss_adv
    if phase == "train":
        loss_g.backward()
        O.clip_grad_norm_(model_g.params, 1.0)
        optimizer_g.step()
    return loss_mse.item(), loss_mge.item(), loss_adv.item(), loss_g.item()


@contextlib.contextmanager
def installed():
    """For the duration, gan_objective_ref's two update functions are the ones above: whatever runs its step loop (its own
    run_step_reference, spectral_norm_ref's, grad_penalty_ref's) then knows "kl", "rkl" and "js" too, and nothing else changes."""
    before = G.update_discriminator, G.update_generator
    G.update_discriminator, G.update_generator = update_discriminator, update_generator
    try:
        yield
    finally:
        G.update_discriminator, G.update_generator = before


def run_step_reference(case, obj, clip=0.0, mistake=None, snapshots=None):
    """gan_objective_ref.run_step_reference under an f-GAN divergence; same keys."""
    with installed():
        return G.run_step_reference(case, obj, clip=clip, mistake=mistake, snapshots=snapshots)
