"""The f-GAN divergences (GT_OPT_GAN_OBJECTIVE: 4 kl, 5 rkl, 6 js) on the GPU.

(1) hook level: gt_op_d_head / gt_op_dstack with `objective` set, over the matrix of tests/test_gpu_gan_objective.py rebuilt for the three new
    objectives, through the guards of tests/test_gpu_d_tail.py (NaN pitch padding, NaN-prefilled results, sentinels, two runs bit-equal,
    launch census) and its float64 chain, with the head's float64 functions of tests/gan_fdiv_ref.py.  Every element lies inside a bound
    carried in float64; counts are compared exactly (the inputs keep every row 64 bounds away from its threshold, kl's at z = 1 included,
    and |z| <= 20: asserted by tests/test_gan_fdiv_host.py).  There is no rms ratchet here: the derived bound is the criterion, and each case
    prints its rms and its worst ratio to the bound (profiles/gan_fdiv_parity.md).  On a library without the feature the hooks refuse
    ids 4 .. 6 and every case of (1) fails.
(2) step level: two G+D steps against the CPU step reference at the suite's 1e-4, counts exactly, every objective on every case of
    gan_objective_ref.STEP_CASES (the "sru" case is PARITY UNPINNED, like every SRU path).
(3) the launches of "bce" on the same case.  (4) refusals, by message.
(5) composition under "js": the weight clip, spectral normalisation and R1, each against the existing step reference of that switch with
    this family's phi put in (gan_fdiv_ref.installed), at 1e-4.
(6) the used-engine contract of tests/engine_history.py: one row per objective, registered in its table for the duration of the test.

test_gpu_gan_objective's matrix builder, float64 reference and input conditioning name their objectives through two globals of that module
(OBJS and the reference module G); `borrowed` lends them this family for the duration of a call, the way that module lends `objective` to
test_gpu_d_tail.run_case."""
import contextlib
import functools
import math

import numpy as np
import pytest

import gan_fdiv_ref as F
import gan_objective_ref as G
import test_gpu_d_tail as T
import test_gpu_gan_objective as GO

MODE_D, MODE_G = T.MODE_D, T.MODE_G
OBJS = F.OBJECTIVES


@contextlib.contextmanager
def borrowed():
    before = GO.OBJS, GO.G
    GO.OBJS, GO.G = F.OBJECTIVES, F
    try:
        yield
    finally:
        GO.OBJS, GO.G = before


with borrowed():
    MATRIX = GO._matrix()
for _c in MATRIX:
    assert _c["id"] not in T._BY_ID and _c["objective"] in OBJS
    T._BY_ID[_c["id"]] = _c          # test_gpu_d_tail's operand cache is keyed by id
HEAD = [c for c in MATRIX if c["entry"] == "head"]
DSTACK = [c for c in MATRIX if c["entry"] == "dstack"]


def reference(key, mistake=None):
    """test_gpu_gan_objective.reference with gan_fdiv_ref's head (cached there by key: the ids of this matrix are its own)."""
    with borrowed():
        return GO.reference(key, mistake)


def conditioned_operands(key):
    with borrowed():
        return GO.conditioned_operands(key)


def condition_margin(key):
    with borrowed():
        return GO.condition_margin(key)


# ---------------------------------------------------------------------------------------------------------------------
# (1) the hooks against float64
# ---------------------------------------------------------------------------------------------------------------------
def _check_case(c):
    """test_gpu_gan_objective._check_case without the per-tensor rms limits (module docstring)."""
    from gantts_amd import _lib as Lb
    tag = c["id"]
    ops = conditioned_operands(tag)
    with GO.hook_objective(F.IDS[c["objective"]]):
        rc, counts, scal, out = T.run_case(c)
    assert rc == Lb.GT_OK, "%s: %s" % (tag, Lb.lib.gt_last_error())
    exp = T.expected_counts(c)           # the slot of the FORM, whatever the objective
    assert counts == exp, "%s: launches %s, expected %s" % (tag, {i: n for i, n in enumerate(counts) if n}, {i: n for i, n in enumerate(exp) if n})
    res = reference(tag)
    written = set(T.tensors(res)) - {"s_real", "s_fake", "s_adv"}
    got = {}
    for name, (flat, logical, buf) in out.items():
        buf.check_outside(flat, name, tag)
        if name in written:
            v = T._from_bf16_bits(logical) if buf.dtype == np.uint16 else logical
            assert not np.isnan(v).any(), "%s: %s has %d elements that are NaN or were never written" % (tag, name, int(np.isnan(v).sum()))
            got[name] = v.astype(np.float64)
        else:
            same = np.array_equal(logical.view(np.uint32), buf.view(buf.host).view(np.uint32)) if buf.dtype == np.float32 else \
                np.array_equal(logical, buf.view(buf.host))
            assert same, "%s: %s was written although the case does not ask for it" % (tag, name)
    assert written <= set(got), (tag, sorted(written - set(got)))
    names = ["s_real", "s_fake", "n_real_ok", "n_fake_ok", "s_adv"]
    mine = names[:4] if c["mode"] == MODE_D else names[4:]
    for i, name in enumerate(names):
        if name in mine:
            assert math.isfinite(scal[i]), "%s: %s = %r" % (tag, name, scal[i])
            got[name] = np.array([scal[i]]) if name.startswith("s_") else scal[i]
        else:
            assert math.isnan(scal[i]), "%s: %s = %r was written by a pass that does not own it" % (tag, name, scal[i])
    if c["norm"] == "unit":
        assert math.isnan(scal[5]) and math.isnan(scal[6]), "%s: unit_tv touched the normaliser" % tag
    else:
        assert scal[5] == float(ops["tv"]) and scal[6] == float(np.float32(1.0) / ops["tv"]), (tag, scal[5], scal[6])
    assert scal[7] == T.n_partials(c), (tag, scal[7])
    for name in T.tensors(res):
        bad, rms, worst = T.criterion(got[name], res[name])
        print("GANFDIVSTAT %s %s %s rms=%.3e worst_bound_ratio=%.3e" % (c["entry"], tag, name, rms, worst))
        assert bad == 0, "%s: %s has %d elements outside the float64 bound (worst ratio %.3g)" % (tag, name, bad, worst)
    for name in ("n_real_ok", "n_fake_ok"):
        if name in res:
            assert got[name] == res[name], "%s: %s = %r, the reference counts %r" % (tag, name, got[name], res[name])
    with GO.hook_objective(F.IDS[c["objective"]]):
        rc2, _, scal2, out2 = T.run_case(c)
    assert rc2 == Lb.GT_OK
    for name in out:
        assert np.array_equal(out[name][0].view(np.uint8), out2[name][0].view(np.uint8)), "%s: %s differs between two runs" % (tag, name)
    assert np.array_equal(np.array(scal).view(np.uint64), np.array(scal2).view(np.uint64)), "%s: the scalars differ between two runs" % tag


@pytest.mark.gpu
@pytest.mark.parametrize("c", HEAD, ids=[c["id"] for c in HEAD])
def test_d_head_fdiv_vs_float64(c):
    _check_case(c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", DSTACK, ids=[c["id"] for c in DSTACK])
def test_dstack_fdiv_vs_float64(c):
    _check_case(c)


# ---------------------------------------------------------------------------------------------------------------------
# (2), (3) whole steps
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def step_reference(name, obj, clip=0.0):
    return F.run_step_reference(G.STEP_CASES[name], obj, clip=clip)


@functools.lru_cache(maxsize=None)
def step_run(name, obj, clip=None):
    """(results, (head counts, gemm counts)) of test_gpu_gan_objective's driver: hp.gan_objective = obj, two G+D steps."""
    return GO.run_hip_objective(G.STEP_CASES[name], obj, clip=clip)


@pytest.mark.gpu
@pytest.mark.parametrize("obj", OBJS)
@pytest.mark.parametrize("name", sorted(G.STEP_CASES))
def test_two_steps_match_the_step_reference(name, obj):
    """(2).  The "sru" case is PARITY UNPINNED, like every SRU path."""
    got, (head, _) = step_run(name, obj)
    ref = step_reference(name, obj)
    for k in sorted(ref):
        if "scalars" in k:
            print("GANFDIVSTEP %s %s %s got %s ref %s" % (name, obj, k, got[k].tolist(), ref[k].tolist()))
    bad = G.step_close(got, ref)
    assert not bad, "%s / %s: outside 1e-4 of the step reference: %s" % (name, obj, bad)
    if name == "mlp128_fused":
        assert head[T.DSTACK128] == 2 * G.STEP_CASES[name]["steps"], head       # both passes of every step took the fused stack


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(G.STEP_CASES))
def test_every_divergence_issues_the_launches_of_bce(name):
    """(3): gt_head_path_counts and gt_gemm_path_counts of the two steps, objective by objective, against "bce" on the same case."""
    _, base = GO.run_hip_objective(G.bce_twin(G.STEP_CASES[name]), "bce")
    assert sum(base[0]) > 0 and sum(base[1]) > 0
    for obj in OBJS:
        counts = step_run(name, obj)[1]
        assert counts[0] == base[0], (name, obj, "head", {i: (a, b) for i, (a, b) in enumerate(zip(counts[0], base[0])) if a != b})
        assert counts[1] == base[1], (name, obj, "gemm", {i: (a, b) for i, (a, b) in enumerate(zip(counts[1], base[1])) if a != b})


# ---------------------------------------------------------------------------------------------------------------------
# (4) refusals, by message
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_and_read_back():
    from gantts_amd import _lib as Lb
    # option second: a bound sigmoid discriminator refuses 4 .. 6, and the option stays what it was
    eng, md_sig = GO._engine_and_models("bce", True)
    eng.bind_model(Lb.ROLE_D, md_sig)
    for obj in OBJS:
        with pytest.raises(ValueError, match="last_sigmoid=False"):
            eng.set_option("gan_objective", F.IDS[obj])
        assert eng.gan_objective == "bce"
    for obj in OBJS:
        # bind second: the divergence, then a sigmoid discriminator
        eng2, md_sig2 = GO._engine_and_models(obj, True)
        assert eng2.gan_objective == obj
        with pytest.raises(ValueError, match="last_sigmoid=False"):
            eng2.bind_model(Lb.ROLE_D, md_sig2)
        _, md_lin = GO._engine_and_models(obj, False)
        eng2.bind_model(Lb.ROLE_D, md_lin)
        # id 0 on an engine bound to a last_sigmoid=False discriminator
        with pytest.raises(ValueError, match="last_sigmoid=True"):
            eng2.set_option("gan_objective", 0)
        assert eng2.gan_objective == obj
        # the read-back follows the option through every id of the family
        for other in OBJS:
            eng2.set_option("gan_objective", F.IDS[other])
            assert eng2.gan_objective == other
    # the range ends behind 6
    with pytest.raises(ValueError, match="GT_OPT_GAN_OBJECTIVE takes 0"):
        eng.set_option("gan_objective", 7)


# ---------------------------------------------------------------------------------------------------------------------
# (5) composition under "js": the switches documented as independent of the objective
# ---------------------------------------------------------------------------------------------------------------------
CLIP = 0.01


@pytest.mark.gpu
def test_weight_clip_under_js():
    got, _ = step_run("mlp32", "js", CLIP)
    ref = step_reference("mlp32", "js", CLIP)
    bad = G.step_close(got, ref)
    assert not bad, "outside 1e-4 of the clamped step reference: %s" % bad
    assert G.step_close(got, step_reference("mlp32", "js"))           # ... and the unclamped reference is not met
    d = [v for k, v in got.items() if k.startswith("D.") and ".opt." not in k]
    assert max(float(np.abs(v).max()) for v in d) <= np.float32(CLIP) and any(np.any(np.abs(v) == np.float32(CLIP)) for v in d)


@pytest.mark.gpu
def test_spectral_norm_under_js():
    import spectral_norm_ref as S
    import test_gpu_spectral_norm as SN
    name = "mlp32"
    got, sn, _ = SN.sn_run(name, "js")
    with F.installed():
        ref = S.run_step_reference(G.STEP_CASES[name], "js")
    assert "D.sn_u" in ref and "D.sn_v" in ref
    bad = G.step_close(got, ref)
    assert not bad, "outside 1e-4 of the spectrally normalised step reference: %s" % bad
    steps = G.STEP_CASES[name]["steps"]
    assert sn == [2 * steps, 2 * steps, 2 * steps, steps, steps], sn
    assert G.step_close(got, step_reference(name, "js"))              # the plain "js" reference is not met: the switch was on


@pytest.mark.gpu
def test_r1_under_js():
    import grad_penalty_ref as R
    import test_gpu_grad_penalty as GP
    case = G.STEP_CASES["mlp32"]
    got, counts = GP.run_hip_gp(case, "js", "r1")
    with F.installed():
        ref = R.run_step_reference(case, "js", "r1", GP.WEIGHT)
    bad = G.step_close(got, ref)
    assert not bad, "outside 1e-4 of the penalised step reference: %s" % bad
    assert got["gp_steps"] == case["steps"] and sum(counts[0]) > 0
    assert G.step_close(got, step_reference("mlp32", "js"))           # the unpenalised reference is not met


# ---------------------------------------------------------------------------------------------------------------------
# (6) a used engine equals a fresh one, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
HISTORY_ROWS = {
    "kl_mlp": (dict(case=("STEP_CASES", "mlp32"), options={}, objective="kl"), "shrink"),
    "rkl_lstm_d": (dict(case=("STEP_CASES", "lstm"), options={}, objective="rkl"), "same_shape_refill"),
    "js_fused": (dict(case=("STEP_CASES", "mlp128_fused"), options={"fused_dstack": 2}, flip=("fused_dstack", 2, 0), objective="js"), "option_flip"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("backend", sorted(HISTORY_ROWS))
def test_used_engine_equals_fresh_engine(backend):
    """tests/engine_history.py's runner looks a row up by name in ALL_BACKENDS: the row is there for the duration of the run only (the
    host checks of that module pin the table)."""
    import engine_history as H
    row, history = HISTORY_ROWS[backend]
    assert backend not in H.ALL_BACKENDS
    H.ALL_BACKENDS[backend] = row
    try:
        worn, twin = H.run_feature_pair(backend, history)
    finally:
        del H.ALL_BACKENDS[backend]
    assert len(worn) > 20 and any(k.startswith("step2.") for k in worn) and "philox_d" in worn
    diffs = H.differences(worn, twin)
    for d in diffs:
        print(d)
    assert not diffs, "%s after %s: %d of %d records differ or are not finite; first: %s" % (backend, history, len(diffs), len(worn), diffs[0])
