"""Host checks of the f-GAN divergence references (tests/gan_fdiv_ref.py) and of the comparators tests/test_gpu_gan_fdiv.py judges the kernels
with.  Nothing here needs a GPU, and nothing here runs the engine."""
import copy
import math

import numpy as np
import pytest
import torch

import gan_fdiv_ref as F
import gan_objective_ref as G
import test_gpu_gan_fdiv as M

T = M.T


# ---------------------------------------------------------------------------------------------------------------------
# the per-frame functions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obj", F.OBJECTIVES)
@pytest.mark.parametrize("g_mode", [False, True])
def test_closed_form_derivative_is_autograd_of_phi(obj, g_mode):
    rs = np.random.RandomState(5)
    z_np = np.concatenate([rs.randn(200) * 3.0, [-20.0, -1.0, 0.0, 1.0, 20.0]])
    real = np.arange(z_np.size) % 2 == 0
    z = torch.tensor(z_np, dtype=torch.float64, requires_grad=True)
    F.phi(obj, z, real, g_mode).sum().backward()
    want = F.dphi(obj, z_np, real, g_mode)
    assert np.allclose(z.grad.numpy(), want, rtol=1e-12, atol=1e-14), (obj, g_mode)
    assert np.allclose(F.phi(obj, z_np, real, g_mode), F.phi(obj, z.detach(), real, g_mode).numpy(), rtol=1e-14, atol=1e-15)


def test_table_values():
    """The table of include/gantts_hip.h at hand-computed points, and the package's tables."""
    one, zero = np.array([True]), np.array([False])
    z = np.array([0.25])
    assert F.phi("kl", z, one, False)[0] == -0.25 and F.phi("kl", z, zero, False)[0] == math.exp(-0.75) and F.phi("kl", z, zero, True)[0] == -0.25
    assert F.phi("rkl", z, one, False)[0] == math.exp(-0.25) and F.phi("rkl", z, zero, False)[0] == -0.75
    assert F.phi("rkl", z, zero, True)[0] == math.exp(-0.25)
    assert abs(F.phi("js", z, one, False)[0] - (math.log(1.0 + math.exp(-0.25)) - math.log(2.0))) < 1e-15
    assert abs(F.phi("js", z, zero, False)[0] - (math.log(1.0 + math.exp(0.25)) - math.log(2.0))) < 1e-15
    for g_mode in (False, True):
        assert abs(F.phi("js", np.array([0.0]), one, g_mode)[0]) < 1e-16        # sp(0) = ln 2
    assert F.dphi("kl", z, zero, False)[0] == math.exp(-0.75) and abs(F.dphi("js", z, one, False)[0] + 1.0 / (1.0 + math.exp(0.25))) < 1e-15
    # saturated rows: finite values and derivatives that go to 0, in the overflow-safe form
    big = np.array([800.0])
    assert F.phi("js", big, one, False)[0] == -math.log(2.0) and F.dphi("js", big, one, False)[0] == 0.0
    assert F.phi("js", big, zero, False)[0] == 800.0 - math.log(2.0) and F.dphi("js", -big, zero, False)[0] == 0.0
    from gantts_amd import _lib as Lb
    assert Lb.GAN_F_DIVERGENCES == F.IDS == {"kl": 4, "rkl": 5, "js": 6}
    assert Lb.GAN_F_DIVERGENCE_THRESHOLD == F.THRESHOLD == {"kl": 1.0, "rkl": 0.0, "js": 0.0}
    assert not set(Lb.GAN_F_DIVERGENCES) & set(Lb.GAN_OBJECTIVES) and not set(Lb.GAN_F_DIVERGENCES.values()) & set(Lb.GAN_OBJECTIVES.values())
    from gantts_amd.engine import gan_objective_id, gan_objective_of, gan_objective_threshold
    for name in F.OBJECTIVES:
        assert gan_objective_of(type("HP", (), dict(gan_objective=name))()) == name
        assert gan_objective_id(name) == F.IDS[name] and gan_objective_threshold(name) == F.THRESHOLD[name]
    for name in G.OBJECTIVES:
        assert gan_objective_id(name) == G.IDS[name] and gan_objective_threshold(name) == G.THRESHOLD[name]
    with pytest.raises(ValueError, match="^hp.gan_objective"):
        gan_objective_of(type("HP", (), dict(gan_objective="chi2"))())


@pytest.mark.parametrize("obj", F.OBJECTIVES)
def test_table_is_the_f_gan_bound(obj):
    """The variational identity: at v* = g_f^-1(f'(P / Q)) the bound -sum P phi_real - sum Q phi_generated equals D_f(P || Q) = sum Q f(P / Q),
    and it is a maximum -- from f, f', f* and g_f of the paper, not from this project's table; the threshold is g_f(z) > f'(1)."""
    rs = np.random.RandomState(11)
    n = 8
    real, fake = np.ones(n, dtype=bool), np.zeros(n, dtype=bool)

    def bound(v):
        return -(P * F.phi(obj, v, real, False)).sum() - (Q * F.phi(obj, v, fake, False)).sum()
    for _ in range(5):
        P, Q = rs.rand(n) + 0.05, rs.rand(n) + 0.05
        P, Q = P / P.sum(), Q / Q.sum()
        v = F.GF_INV[obj](F.FPRIME[obj](P / Q))
        div = (Q * F.F[obj](P / Q)).sum()
        assert div > 0 and abs(bound(v) - div) <= 1e-12, (obj, bound(v), div)
        # the table's two columns are -g_f and f*(g_f)
        assert np.allclose(F.phi(obj, v, real, False), -F.GF[obj](v), rtol=0, atol=1e-13)
        assert np.allclose(F.phi(obj, v, fake, False), F.FSTAR[obj](F.GF[obj](v)), rtol=0, atol=1e-13)
        for _ in range(200):
            assert bound(v + rs.randn(n) * rs.choice([1e-3, 0.1, 1.0])) <= div + 1e-12
    zs = np.linspace(-3.0, 3.0, 25) + 1e-3
    assert np.array_equal(F.GF[obj](zs) > F.FPRIME[obj](1.0), zs > F.THRESHOLD[obj])
    # the G step is the non-saturating form: its rows are scored as real ones
    assert np.array_equal(F.phi(obj, zs, np.zeros(25, dtype=bool), True), F.phi(obj, zs, np.ones(25, dtype=bool), False))


# ---------------------------------------------------------------------------------------------------------------------
# the step reference
# ---------------------------------------------------------------------------------------------------------------------
def test_js_step_reference_is_the_bce_one_shifted_by_ln2():
    """js is the logistic loss minus 2 ln 2: on a case whose D stays away from 0 and 1 (eps = 1e-20 is then invisible) the step reference under
    "js" gives the pinned "bce" reference's losses minus ln 2 per column (2 ln 2 for loss_d), the same counts and the same parameters.  Ties the
    new step reference to the pinned one."""
    case = G.STEP_CASES["mlp32"]
    a, b = G.run_step_reference(G.bce_twin(case), "bce"), F.run_step_reference(case, "js")
    ln2 = math.log(2.0)
    for step in range(case["steps"]):
        da, db = a["d_scalars_%d" % step], b["d_scalars_%d" % step]
        assert np.all(np.abs(da[:3] - db[:3] - np.array([2 * ln2, ln2, ln2])) <= 1e-6), (step, da, db)
        assert da[3] == db[3] and da[4] == db[4]
        ga, gb = a["g_scalars_%d" % step], b["g_scalars_%d" % step]
        assert abs(ga[2] - gb[2] - ln2) <= 1e-6, (step, ga, gb)      # loss_adv (loss_g, near 64 in float32, has no sixth decimal)
    assert not [k for k in G.step_close(b, a) if "scalars" not in k]
    # any other objective passes through to the pinned functions, bit for bit
    c, d = G.run_step_reference(case, "ls"), F.run_step_reference(case, "ls")
    assert sorted(c) == sorted(d)
    assert all(np.array_equal(np.atleast_1d(np.asarray(c[k])).view(np.uint8), np.atleast_1d(np.asarray(d[k])).view(np.uint8)) for k in c)
    assert G.update_discriminator is F._G_UPDATE_D and G.update_generator is F._G_UPDATE_G      # `installed` put everything back


@pytest.mark.parametrize("mistake,obj", [("kl_exp_unshifted", "kl"), ("rkl_generated_unshifted", "rkl"), ("js_ln2_missing", "js"),
                                         ("kl_threshold_zero", "kl"), ("g_rows_scored_as_generated", "kl"),
                                         ("g_rows_scored_as_generated", "rkl"), ("g_rows_scored_as_generated", "js")])
def test_step_comparator_rejects_seeded_mistakes(mistake, obj):
    """step_close (1e-4, counts exactly) rejects a step reference with the mistake planted and accepts the reference against itself.  (The
    step reference differentiates by autograd: a wrong derivative sign can only be planted at the hook level.)"""
    case = G.STEP_CASES["mlp32"]
    good = F.run_step_reference(case, obj)
    assert G.step_close(copy.deepcopy(good), good) == []
    wrong = F.run_step_reference(case, obj, mistake=mistake)
    assert G.step_close(wrong, good), mistake


# ---------------------------------------------------------------------------------------------------------------------
# the hook matrix, its inputs and its criterion
# ---------------------------------------------------------------------------------------------------------------------
def test_matrix_is_what_the_kernels_need():
    heads = {(c["form"], c["K"], c["rows"]) for c in M.HEAD}
    assert heads >= {("f32", K, r) for K in (1, 65, 130) for r in (1, 17, 33)} | {("vec", 256, r) for r in (1, 17, 33)}
    assert ("f32", 1024, 33) in heads and ("img", 130, 17) in heads
    stacks = {(c["hd"], c["rows"], c["L"]) for c in M.DSTACK}
    assert stacks >= {(hd, r, L) for hd in (128, 256) for r in (33, 74) for L in (2, 3)}
    assert any(c["mode"] == M.MODE_G and c["want_grad"] and c["Da"] == 58 for c in M.DSTACK)
    for cases in (M.HEAD, M.DSTACK):
        combos = {(c["objective"], c["mode"], c["want_grad"], c["norm"] == "unit") for c in cases}
        assert combos == {(o, m, g, u) for o in F.OBJECTIVES for m in (0, 1) for g in (0, 1) for u in (False, True)}
        assert any(c["norm"] == "tv_dev" for c in cases if c["entry"] == "head") or cases is M.DSTACK
        for obj in F.OBJECTIVES:      # every shape under every objective in both modes
            assert {(c.get("K", c.get("hd")), c["rows"], c["mode"]) for c in cases if c["objective"] == obj} == \
                   {(c.get("K", c.get("hd")), c["rows"], c["mode"]) for c in cases}
    assert len({c["id"] for c in M.MATRIX}) == len(M.MATRIX) and max(c["rows"] for c in M.MATRIX) <= 74
    # the same matrix as the objectives 1 .. 3, case for case
    assert len(M.MATRIX) == len(M.GO.MATRIX)
    same = ("entry", "mode", "want_grad", "norm", "rows", "n_real", "n_mask", "acc")
    for a, b in zip(M.MATRIX, M.GO.MATRIX):
        assert all(a[k] == b[k] for k in same) and a.get("K", a.get("hd")) == b.get("K", b.get("hd")), (a["id"], b["id"])
        assert F.OBJECTIVES.index(a["objective"]) == M.GO.OBJS.index(b["objective"]) and a["id"] != b["id"]
    for c in M.MATRIX:
        assert sum(T.expected_counts(c)) in (1, 2)
    assert M.GO.OBJS == ("ls", "hinge", "wgan") and M.GO.G is G      # the borrowed builder was handed back


@pytest.mark.parametrize("c", M.MATRIX, ids=[c["id"] for c in M.MATRIX])
def test_input_conditions(c):
    """No row of the float64 reference within 64x its own z bound of its count threshold (kl's at z = 1 included), none within T's own 1.5
    bounds of a LeakyReLU kink; |z| <= 20, so that no exp is anywhere near overflow; and the criterion accepts the reference rounded to the
    storage type."""
    res = M.reference(c["id"])
    assert M.condition_margin(c["id"]) > 64.0
    if c["mode"] == M.MODE_D:
        k = res["_cond"]["kinks"]
        assert np.all(k == F.THRESHOLD[c["objective"]]) and k.shape[0] == c["rows"]
    ops = M.conditioned_operands(c["id"])
    x = ops["H"] if c["entry"] == "head" else ops["H0"]
    keeps = [ops["keep"]] if c["entry"] == "head" else ops["keeps"]
    assert not T._ambiguous_rows(c, ops, x, keeps).any()
    assert np.abs(res["_cond"]["z"]).max() <= 20.0
    got = T.rounded(res)
    for name in T.tensors(res):
        bad, rms, worst = T.criterion(got[name], res[name])
        assert bad == 0 and worst <= 1.0, (c["id"], name, bad, worst)


def test_bounds_hold_for_a_float32_emulation_of_the_kernel_sequence():
    """The sequences of gan_objective.hip.h's comment, evaluated in numpy float32 (one rounding per operation, numpy's exp and log in place of
    expf and logf) on float32 inputs with E_z = 0, stay inside head_math's bounds -- including js around its zero at z = 0, where the bound
    is absolute."""
    f4 = np.float32
    rs = np.random.RandomState(3)
    z = np.concatenate([rs.randn(4000) * 4.0, rs.randn(500) * 1e-3, [0.0, 1.0, -1.0, 20.0, -20.0]]).astype(f4)
    n = z.size
    m, u = np.ones(n, f4), f4(1.0) / f4(37.0)
    one, ln2f = f4(1.0), f4(math.log(2.0))
    h, w = z.astype(np.float64)[:, None], np.ones(1)
    for obj in F.OBJECTIVES:
        for mode_g, n_real in ((False, n // 2), (True, n)):
            q = F.head_math(obj, mode_g, n_real, n, h, np.zeros_like(h), w, 0.0, m.astype(np.float64), float(u))
            gen = ~q["real"]
            if obj == "kl":
                e = np.exp(z - one)
                ph, dz = np.where(gen, e, -z), np.where(gen, e * u, -u)
            elif obj == "rkl":
                e = np.exp(-z)
                ph, dz = np.where(gen, z - one, e), np.where(gen, u, -(e * u))
            else:
                x = np.where(gen, z, -z)
                l = np.log(one + np.exp(-np.abs(z)))
                ph = (np.maximum(x, f4(0.0)) + l) - ln2f
                s = u / (one + np.exp(-x))
                dz = np.where(gen, s, -s)
            assert ph.dtype == f4 and dz.dtype == f4
            Ez0 = q["Ez"]       # (the bound of a one-term product: 3 U |z|, part of every bound below)
            assert np.all(np.abs(-ph.astype(np.float64) - q["lt"]) <= q["El"] + T.TINY), (obj, mode_g)
            assert np.all(np.abs(dz.astype(np.float64) - q["dz"]) <= q["Edz"] + T.TINY), (obj, mode_g)
            assert np.all(q["El"] <= 64 * F.U * (1.0 + np.abs(q["lt"])) + 4.0 * (1.0 + np.abs(q["lt"])) * Ez0)      # ... and are no blank cheques


def _rejects(c, res, got):
    for name in T.tensors(res):
        if name in got and T.criterion(got[name], res[name])[0]:
            return True
    return any(name in res and got.get(name, res[name]) != res[name] for name in ("n_real_ok", "n_fake_ok"))


@pytest.mark.parametrize("mistake,obj,mode", [("kl_exp_unshifted", "kl", 0), ("rkl_generated_unshifted", "rkl", 0), ("js_ln2_missing", "js", 0),
                                              ("js_ln2_missing", "js", 1), ("kl_threshold_zero", "kl", 0),
                                              ("g_rows_scored_as_generated", "kl", 1), ("g_rows_scored_as_generated", "rkl", 1),
                                              ("g_rows_scored_as_generated", "js", 1), ("js_generated_derivative_sign", "js", 0)])
def test_hook_criterion_rejects_seeded_mistakes(mistake, obj, mode):
    """Each planted mistake, applied to the float64 reference's own outputs, is rejected by the bounds or the exact counts for at least one
    case of either entry; the unmutated reference is accepted everywhere (test_input_conditions)."""
    for entry in ("head", "dstack"):
        hit = []
        for c in M.MATRIX:
            if c["entry"] != entry or c["objective"] != obj or c["mode"] != mode:
                continue
            if mistake == "js_generated_derivative_sign" and not c["want_grad"]:
                continue
            if _rejects(c, M.reference(c["id"]), T.rounded(M.reference(c["id"], mistake))):
                hit.append(c["id"])
        assert hit, "no %s case rejects %r under %s" % (entry, mistake, obj)
