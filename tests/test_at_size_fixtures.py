"""CPU checks of the at-size fixtures (tests/golden/at_size_*.npz) and of the RCCL test double's ABI.

The fixtures are digests of the REAL reference (or, for the un-vendored SRU, of the oracle) run once at the sizes
BASELINE.json names, in float32 and float64 (tests/golden/make_at_size.py); the -m gpu tests judge the HIP engine against them."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import at_size as A
import cases as C
import gantts_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


@pytest.mark.parametrize("name", sorted(n for n in A.AT_SIZE_CASES if os.path.isfile(os.path.join(GOLDEN, "at_size_%s.npz" % n))))
def test_fixture_is_complete_and_self_consistent(name):
    case = A.AT_SIZE_CASES[name]
    fx = np.load(os.path.join(GOLDEN, "at_size_%s.npz" % name))
    assert str(fx["meta.source"]) == case["source"]
    tensors = sorted(k[:-7] for k in fx.files if k.endswith(".sample"))
    assert "y_hat" in tensors and "y_hat_static" in tensors
    gnames = [n for n, _ in C.param_shapes(case["g"])]
    dnames = [n for n, _ in C.param_shapes(case["d"])]
    for pre, names in (("Ggrad.", gnames), ("Gupd.", gnames), ("Dgrad.", dnames), ("Dupd.", dnames)):
        assert [k for k in tensors if k.startswith(pre)] == sorted(pre + n for n in names)
    for k in tensors:
        assert np.isfinite(fx[k + ".sample"]).all() and float(fx[k + ".norm"]) > 0
        # the reference's own float32 run is close to its float64 run (1e-2 at the very worst: sign-like first Adam steps)
        # (a cold Adagrad accumulator makes the first update lr * sign(g): the reference's own two runs disagree on the sign of
        # gradient elements that are zero within rounding, each a 2 * lr difference -- those tensors are judged element-wise)
        assert 0 <= float(fx[k + ".err32"]) < (0.3 if case.get("cold") and k[1:5] == "upd." else 1e-2), (k, float(fx[k + ".err32"]))
        # the sample's norm cannot exceed the whole tensor's
        assert float(np.sqrt((fx[k + ".sample"].astype(np.float64) ** 2).sum())) <= float(fx[k + ".norm"]) * (1 + 1e-6)
    for st in range(case["steps"]):
        for k in ("d_scalars_%d" % st, "g_scalars_%d" % st):
            # the reference's own float32 and float64 runs agree to rounding for the first steps and then drift apart (ten steps of
            # cfg3: 1e-7 .. 2e-6 up to the 5th step, 1.6e-3 on loss_adv and 20 of 8457 counts at the 10th): the fixture must show that
            # drift, not hide it -- it is what the GPU tests' per-step limits are derived from
            rtol = 2e-5 if st < 4 else 5e-3
            np.testing.assert_allclose(fx[k + ".f32"], fx[k + ".f64"], rtol=rtol, atol=1e-7)      # (atol: a saturated loss_adv of 2e-6)
    # the sample positions are a function of the key alone
    a = np.arange(100000, dtype=np.float32)
    assert np.array_equal(A.sample_of("Ggrad.x", a), A.sample_of("Ggrad.x", a)) and A.sample_of("Ggrad.x", a).size == A.SAMPLE


def test_random_projections_estimate_the_full_tensor_distance():
    """at_size.proj_of: PROJ_K seeded Rademacher projections of the WHOLE tensor.  The rms of the projection differences of two tensors estimates
    their full distance |a - b| (every element takes part): a dense perturbation and one confined to a block that a 4096-element sample would
    hardly touch are both recovered to within the estimator's chi-square spread; the projections are a function of (key, tensor) alone."""
    rs = np.random.RandomState(7)
    a = rs.randn(300, 2048)
    for e in (1e-3 * rs.randn(300, 2048), np.pad(0.05 * rs.randn(3, 40), ((100, 197), (1000, 1008)))):
        est = A.rms(A.proj_of("Ggrad.w", a + e) - A.proj_of("Ggrad.w", a))
        true = float(np.sqrt((e * e).sum()))
        assert 0.6 * true < est < 1.5 * true, (est, true)
    assert np.array_equal(A.proj_of("k", a), A.proj_of("k", a.copy())) and not np.array_equal(A.proj_of("k", a), A.proj_of("k2", a))
    assert A.proj_of("k", a).shape == (A.PROJ_K,)
    # the committed fixtures that carry projections carry them for every tensor
    for name in sorted(A.AT_SIZE_CASES):
        path = os.path.join(GOLDEN, "at_size_%s.npz" % name)
        if os.path.isfile(path):
            fx = np.load(path)
            tensors = [k[:-7] for k in fx.files if k.endswith(".sample")]
            have = [k for k in tensors if (k + ".proj") in fx.files]
            assert not have or len(have) == len(tensors), name


def test_ratchet_covers_every_tensor_of_every_float32_at_size_case():
    """tests/golden/at_size_ratchet.json: per at-size case and tensor, the engine's distance to the float64 reference as MEASURED
    on the GPU with the committed build; tests/test_gpu_at_size.py holds every tensor to 4 x that (floor 4e-7) AND to the arbiter's limit.  It
    must name every tensor of every fixture (a tensor without an entry is judged by the arbiter alone), and nothing in it may exceed the
    reference-derived ceiling the arbiter would allow anyway (3 x the network's float32 level + kink allowance: a ratchet above it is dead)."""
    import json
    held = json.load(open(os.path.join(GOLDEN, "at_size_ratchet.json")))
    for name in sorted(A.AT_SIZE_CASES):
        path = os.path.join(GOLDEN, "at_size_%s.npz" % name)
        if not os.path.isfile(path):
            continue
        fx = np.load(path)
        tensors = sorted(k[:-7] for k in fx.files if k.endswith(".sample"))
        assert name in held, name
        if not A.AT_SIZE_CASES[name].get("cold"):
            assert sorted(held[name]) == tensors, name
        else:      # cold-accumulator updates are judged element-wise (judge_cold_update), not by an rms: no ratchet entry
            assert sorted(held[name]) == [k for k in tensors if k.split(".")[0] not in ("Dupd", "Gupd")], name
        for k, v in held[name].items():
            assert 0.0 <= v < 0.2, (name, k, v)
    # the tight rows the ratchet exists for: the D gradients of the cold cfg2 step sit at rounding level
    d = [v for k, v in held["cfg2_cold"].items() if k.startswith("Dgrad.")]
    assert d and max(d) < 5e-6


def test_drift_spread_of_the_real_reference_backs_the_long_run_limits():
    """tests/golden/drift_spread_cfg3_lstm_10.json (written by tests/golden/make_drift_spread.py in the build
    container): the REAL reference's ten float32 steps of cfg3_lstm_10 under other summation orders -- thread counts and relabelled
    discriminator hidden units -- each compared with the committed float64 digest exactly as the engine is.  At least five orders beside the
    fixture's own run; the limits tests/test_gpu_at_size.py derives from them (scalars: 2 x the largest late-step ratio to the reference's own
    float32 envelope, never below 15; update tensors of long runs: 1.5 x the largest ratio to the network's float32 level) must cover every
    measured order with room, and must not be looser than twice what was measured: the widening is a measurement, not a guess."""
    import json
    path = os.path.join(GOLDEN, "drift_spread_cfg3_lstm_10.json")
    d = json.load(open(path))
    v = d["variants"]
    assert d["case"] == "cfg3_lstm_10" and len([k for k in v if k != "threads8_fixture"]) >= 5, sorted(v)
    assert sum(1 for k in v if k.startswith("perm")) >= 2 and sum(1 for k in v if k.startswith("threads")) >= 2, sorted(v)
    ratios, upds = [], []
    for name, rec in v.items():
        assert len(rec["scalar_over_envelope"]) == 10 and len(rec["envelope"]) == 10, name
        late = [r for r in rec["scalar_over_envelope"] if r is not None]
        assert late, name
        ratios.append(max(late))
        upds.append(max(rec["worst_over_level_Dupd"], rec["worst_over_level_Gupd"]))
        for c in rec["count_diff"][:5]:     # the first steps' accuracy counts agree to the 3 frames the engine is allowed: the variants ARE the same computation
            assert max(abs(x) for x in c) <= 3.0, (name, c)
    # correct float32 evaluations of the reference itself leave the old limits (15 x envelope, 3 x level): that is the point of the file
    assert max(ratios) > 15.0 and max(upds) > 3.0, (ratios, upds)
    import importlib.util
    spec = importlib.util.spec_from_file_location("t_gpu_at_size", os.path.join(HERE, "test_gpu_at_size.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.SCALAR_DRIFT_FACTOR >= 2.0 * max(ratios) - 1e-9 and m.SCALAR_DRIFT_FACTOR <= max(15.0, 2.0 * max(ratios)) + 1e-9
    assert m.LONG_RUN_FACTOR * A.ARBITER_FACTOR >= 1.5 * max(upds) - 1e-9
    assert m.LONG_RUN_FACTOR * A.ARBITER_FACTOR <= max(A.ARBITER_FACTOR, 1.5 * max(upds)) + 1e-9


def test_oracle_reproduces_the_reference_fixture_at_full_size():
    """cfg5's duration pair at its real size (B = 64, generator noise 416 + 200 -> 5, conditioned D, Adam, two steps, injected
    dropout masks): the ORACLE in float32 against the digest of the REAL reference's float64 run -- the oracle is the reference's
    arithmetic, so it must sit within the reference's own float32 distance of it (the same arbiter rule the GPU tests apply)."""
    import sys
    sys.path.insert(0, GOLDEN)
    import make_at_size as M
    case = A.AT_SIZE_CASES["cfg5_duration"]
    fx = np.load(os.path.join(GOLDEN, "at_size_cfg5_duration.npz"))
    got = M.run_oracle(case, torch.float32)
    keys = sorted(k[:-7] for k in fx.files if k.endswith(".sample"))
    level = {}
    for k in keys:
        level[k.split(".")[0]] = max(level.get(k.split(".")[0], 0.0), float(fx[k + ".err32"]))
    for k in keys:
        ref = fx[k + ".sample"].astype(np.float64)
        g = A.sample_of(k, np.asarray(got[k])).astype(np.float64)
        err = A.rms(g - ref) / max(A.rms(ref), 1e-300)
        lim = A.ARBITER_FACTOR * max(float(fx[k + ".err32"]), level[k.split(".")[0]]) + A.ARBITER_FLOOR + A.kink_allowance(fx, k[0] if k[0] in "GD" else "G")
        assert err <= lim, (k, err, lim)
    for st in range(case["steps"]):
        d, r = got["d_scalars_%d" % st], fx["d_scalars_%d.f64" % st]
        np.testing.assert_allclose(d[:3], r[:3], rtol=1e-5)
        assert d[3] == r[3] and d[4] == r[4]
        np.testing.assert_allclose(got["g_scalars_%d" % st], fx["g_scalars_%d.f64" % st], rtol=1e-5)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.isfile("/opt/rocm/bin/hipcc"), reason="no HIP compiler")
def test_rccl_test_double_exports_what_the_engine_binds():
    """tests/fake_rccl.cpp must export the seven nccl* symbols of its interface, among them the five eng_comm.hip resolves (rccl_api())."""
    so = os.path.join(HERE, "libfake_rccl.so")
    src = os.path.join(HERE, "fake_rccl.cpp")
    if not os.path.isfile(so) or os.path.getmtime(so) < os.path.getmtime(src):
        hipcc = "/opt/rocm/bin/hipcc" if os.path.isfile("/opt/rocm/bin/hipcc") else "hipcc"
        subprocess.check_call([hipcc, "-O2", "-fPIC", "-shared", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", src, "-o", so, "-lrt"])
    lib = ctypes.CDLL(so)
    for sym in ("ncclGetUniqueId", "ncclCommInitRank", "ncclCommDestroy", "ncclAllReduce", "ncclGroupStart", "ncclGroupEnd", "ncclGetErrorString"):
        assert hasattr(lib, sym), sym
    eng = open(os.path.join(os.path.dirname(HERE), "gantts_amd", "csrc", "eng_comm.hip")).read()
    for sym in ("ncclGetUniqueId", "ncclCommInitRank", "ncclCommDestroy", "ncclAllReduce", "ncclGetErrorString"):
        assert '"%s"' % sym in eng
    buf = ctypes.create_string_buffer(128)
    assert lib.ncclGetUniqueId(buf) == 0 and buf.raw.startswith(b"/gt_fake_rccl_")
    assert "GT_RCCL_LIB" in eng
