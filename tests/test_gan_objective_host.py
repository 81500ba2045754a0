"""Host checks of the adversarial-objective references (tests/gan_objective_ref.py) and of the comparators tests/test_gpu_gan_objective.py
judges the kernels with.  Nothing here needs a GPU, and nothing here runs the engine."""
import copy

import numpy as np
import pytest
import torch

import cases as C
import gan_objective_ref as G
import test_gpu_gan_objective as M

T = M.T


# ---------------------------------------------------------------------------------------------------------------------
# the per-frame functions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obj", G.OBJECTIVES)
@pytest.mark.parametrize("g_mode", [False, True])
def test_closed_form_derivative_is_autograd_of_phi(obj, g_mode):
    """Every phi' of the reference equals torch autograd of phi in float64 (the kinks themselves included: 0 there, as torch's relu)."""
    rs = np.random.RandomState(5)
    z_np = np.concatenate([rs.randn(200) * 2.0, [-1.0, 0.0, 0.5, 1.0, -1.0, 1.0]])
    real = np.arange(z_np.size) % 2 == 0
    z = torch.tensor(z_np, dtype=torch.float64, requires_grad=True)
    G.phi(obj, z, real, g_mode).sum().backward()
    want = G.dphi(obj, z_np, real, g_mode)
    assert np.allclose(z.grad.numpy(), want, rtol=1e-12, atol=1e-14), (obj, g_mode)
    # the numpy and the torch evaluation of phi are one function (torch's sigmoid and log may round their last bit differently)
    assert np.allclose(G.phi(obj, z_np, real, g_mode), G.phi(obj, z.detach(), real, g_mode).numpy(), rtol=1e-14, atol=1e-15)


def test_table_values():
    """The table of include/gantts_hip.h at hand-computed points."""
    one = np.array([True])
    zero = np.array([False])
    z = np.array([0.25])
    assert G.phi("ls", z, one, False)[0] == 0.5 * 0.75 ** 2 and G.phi("ls", z, zero, False)[0] == 0.5 * 0.25 ** 2
    assert G.phi("ls", z, one, True)[0] == 0.5 * 0.75 ** 2
    assert G.phi("hinge", z, one, False)[0] == 0.75 and G.phi("hinge", z, zero, False)[0] == 1.25 and G.phi("hinge", z, one, True)[0] == -0.25
    assert G.phi("hinge", np.array([1.5]), one, False)[0] == 0.0 and G.phi("hinge", np.array([-1.5]), zero, False)[0] == 0.0
    assert G.phi("wgan", z, one, False)[0] == -0.25 and G.phi("wgan", z, zero, False)[0] == 0.25 and G.phi("wgan", z, one, True)[0] == -0.25
    assert G.dphi("hinge", np.array([1.0]), one, False)[0] == 0.0 and G.dphi("hinge", np.array([-1.0]), zero, False)[0] == 0.0
    assert G.THRESHOLD == {"bce": 0.5, "ls": 0.5, "hinge": 0.0, "wgan": 0.0} and G.IDS == {"bce": 0, "ls": 1, "hinge": 2, "wgan": 3}
    from gantts_amd import _lib as Lb
    assert Lb.GAN_OBJECTIVES == G.IDS and Lb.GAN_OBJECTIVE_THRESHOLD == G.THRESHOLD and Lb.OPT_GAN_OBJECTIVE == 21


# ---------------------------------------------------------------------------------------------------------------------
# the step reference
# ---------------------------------------------------------------------------------------------------------------------
def test_bce_step_reference_is_the_oracle_bit_for_bit():
    """With "bce" the step reference performs the oracle's torch operations one for one: identical bits on an existing golden case.
    (Passes without the feature by construction: it ties the new reference to the pinned one.)"""
    from oracle_runner import run_oracle_case
    case = C.CASES["acoustic_mlp_dropout"]
    a, b = run_oracle_case(case), G.run_step_reference(case, "bce")
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = np.atleast_1d(np.asarray(a[k])), np.atleast_1d(np.asarray(b[k]))
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


def test_step_cases_cover_the_discriminators():
    kinds = {(c["d"]["kind"], c["d"]["hidden_dim"], bool(c.get("fused")), c["cond"]) for c in G.STEP_CASES.values()}
    assert kinds >= {("MLP", 32, False, False), ("MLP", 128, True, False), ("LSTMRNN", 12, False, False), ("SRURNN", 12, False, False),
                     ("MLP", 32, False, True)}
    for c in G.STEP_CASES.values():
        assert (c["B"], c["T"], c["steps"], c["dropout_on"]) == (3, 24, 2, True) and not c["d"]["last_sigmoid"]
        assert len(set(C.make_batch(c)[2])) > 1          # ragged lengths


@pytest.mark.parametrize("mistake,obj", [("fake_sign_flipped", "wgan"), ("ls_half_missing", "ls"), ("g_rows_scored_as_generated", "hinge"),
                                         ("wgan_threshold_half", "wgan"), ("clamp_before_update", "wgan")])
def test_step_comparator_rejects_seeded_mistakes(mistake, obj):
    """The whole-run comparison of the GPU test (step_close: 1e-4, counts exactly) rejects a step reference with the mistake planted --
    and accepts the reference against itself.  (The step reference differentiates by autograd: a wrong hinge derivative can only be
    planted at the hook level, test_hook_criterion_rejects_seeded_mistakes.)"""
    case = G.STEP_CASES["mlp32"]
    clip = 0.01 if obj == "wgan" else 0.0
    good = G.run_step_reference(case, obj, clip=clip)
    assert G.step_close(copy.deepcopy(good), good) == []
    wrong = G.run_step_reference(case, obj, clip=clip, mistake=mistake)
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
        assert combos == {(o, m, g, u) for o in M.OBJS for m in (0, 1) for g in (0, 1) for u in (False, True)}
        for obj in M.OBJS:      # every shape under every objective in both modes
            assert {(c.get("K", c.get("hd")), c["rows"], c["mode"]) for c in cases if c["objective"] == obj} == \
                   {(c.get("K", c.get("hd")), c["rows"], c["mode"]) for c in cases}
    assert len({c["id"] for c in M.MATRIX}) == len(M.MATRIX) and max(c["rows"] for c in M.MATRIX) <= 74
    # same launches: the census model is the one of the "bce" cases of the same form
    for c in M.MATRIX:
        assert sum(T.expected_counts(c)) in (1, 2)


@pytest.mark.parametrize("c", M.MATRIX, ids=[c["id"] for c in M.MATRIX])
def test_input_conditions(c):
    """No row of the float64 reference within 64x its own z bound of a hinge kink (+-1) or of its count threshold, none within T's own
    1.5 bounds of a LeakyReLU kink; and the criterion accepts the reference rounded to the storage type."""
    res = M.reference(c["id"])
    assert M.condition_margin(c["id"]) > 64.0
    ops = M.conditioned_operands(c["id"])
    x = ops["H"] if c["entry"] == "head" else ops["H0"]
    keeps = [ops["keep"]] if c["entry"] == "head" else ops["keeps"]
    assert not T._ambiguous_rows(c, ops, x, keeps).any()
    assert np.abs(res["_cond"]["z"]).max() <= 10.0
    got = T.rounded(res)
    for name in T.tensors(res):
        bad, rms, worst = T.criterion(got[name], res[name])
        assert bad == 0 and worst <= 1.0, (c["id"], name, bad, worst)


def _rejects(c, res, got):
    for name in T.tensors(res):
        if name in got and T.criterion(got[name], res[name])[0]:
            return True
    return any(name in res and got.get(name, res[name]) != res[name] for name in ("n_real_ok", "n_fake_ok"))


@pytest.mark.parametrize("mistake,obj,mode", [("fake_sign_flipped", "ls", 0), ("fake_sign_flipped", "hinge", 0), ("fake_sign_flipped", "wgan", 0),
                                              ("ls_half_missing", "ls", 0), ("ls_half_missing", "ls", 1),
                                              ("hinge_derivative_beyond_kink", "hinge", 0),
                                              ("g_rows_scored_as_generated", "ls", 1), ("g_rows_scored_as_generated", "hinge", 1),
                                              ("g_rows_scored_as_generated", "wgan", 1), ("wgan_threshold_half", "wgan", 0)])
def test_hook_criterion_rejects_seeded_mistakes(mistake, obj, mode):
    """Each planted mistake, applied to the float64 reference's own outputs, is rejected by the bounds or the exact counts for at least
    one case of either entry; the unmutated reference is accepted everywhere (test_input_conditions)."""
    for entry in ("head", "dstack"):
        hit = []
        for c in M.MATRIX:
            if c["entry"] != entry or c["objective"] != obj or c["mode"] != mode:
                continue
            if mistake == "hinge_derivative_beyond_kink" and not c["want_grad"]:
                continue
            if _rejects(c, M.reference(c["id"]), T.rounded(M.reference(c["id"], mistake))):
                hit.append(c["id"])
        assert hit, "no %s case rejects %r under %s" % (entry, mistake, obj)
