"""tests/ledger_ref.py -- the pure-Python model the epoch ledger kernel is tested against -- checked against the arithmetic it claims to
follow: ``gantts_amd.train.compute_distortions`` on canned distortion sums (no device), and the running sums ``train_loop`` keeps.
Then the comparator is shown to reject the mistakes a ledger kernel is likely to make."""
import math
import types

import numpy as np
import pytest
import torch

import ledger_ref as LR
from gantts_amd import _lib as L
import gantts_amd.train as T

SMALL = dict(stream_sizes=[6, 3, 1, 3], has_dynamic_features=[True, True, False, True])      # Ds = 5
HP = {"acoustic": types.SimpleNamespace(name="acoustic", windows=[None] * 3, **SMALL),
      "duration": types.SimpleNamespace(name="duration", windows=[None], stream_sizes=[5], has_dynamic_features=[False]),
      "vc": types.SimpleNamespace(name="vc", windows=[None] * 3, stream_sizes=[9], has_dynamic_features=[True], order=3)}
DS = {"acoustic": 5, "duration": 5, "vc": 3}


def _sums(rs, n_voiced=None):
    """Seven distortion sums as a batch of 40 .. 4000 frames would leave them: random doubles, integer counts."""
    n = float(rs.randint(40, 4000))
    nv = float(rs.randint(1, int(n))) if n_voiced is None else float(n_voiced)
    return [rs.rand() * n * 3.0, rs.rand() * n * 1.7, rs.rand() * nv * 900.0, nv, float(rs.randint(0, int(n))), rs.rand() * n * 11.0, n]


def _canned(monkeypatch, dist):
    r = L.DistortionSums(*dist)
    monkeypatch.setattr(T, "_distortion_sums", lambda *a, **k: r)


CASES = [("acoustic", None), ("acoustic", 0), ("duration", None), ("vc", None)]


@pytest.mark.parametrize("name,n_voiced", CASES, ids=["acoustic", "acoustic-unvoiced", "duration", "vc"])
def test_reference_metrics_are_compute_distortions(monkeypatch, name, n_voiced):
    monkeypatch.setattr(T, "hp", HP[name])
    rs = np.random.RandomState(11)
    y = torch.zeros(2, 7, DS[name])
    for _ in range(6):
        dist = _sums(rs, n_voiced)
        _canned(monkeypatch, dist)
        want = T.compute_distortions(y, y, torch.zeros(13), torch.ones(13), [7, 3])
        got = LR.batch_metrics(dist, LR.KIND_OF[name], DS[name], T._LOGDB_CONST)
        assert list(got) == list(want)
        assert LR.same_bits([got[k] for k in want], [want[k] for k in want]), (got, want)
        if n_voiced == 0:
            assert math.isnan(got["f0_rmse"]) and math.isnan(want["f0_rmse"])


def _host_loop(steps, name):
    """The sums train_loop keeps on the host over ``steps`` = [(results float32[12], dist, flags)], as its body forms them."""
    running_loss = {"generator": 0.0, "mse": 0.0, "mge": 0.0, "loss_real_d": 0.0, "loss_fake_d": 0.0, "loss_adv": 0.0, "discriminator": 0.0}
    running_metrics, real, fake, nd, ng = {}, 0, 0, 0.0, 0.0
    kind, Ds = LR.KIND_OF[name], DS[name]
    for res, dist, flags in steps:
        r = [float(v) for v in res]           # ctypes hands c_float fields over as Python floats
        if flags & LR.HAS_D:
            running_loss["discriminator"] += r[0]
            running_loss["loss_fake_d"] += r[1]
            running_loss["loss_real_d"] += r[2]
            real += r[3]
            fake += r[4]
            nd += 1.0
        if flags & LR.HAS_G:
            running_loss["mse"] += r[5]
            running_loss["mge"] += r[6]
            running_loss["loss_adv"] += r[7]
            running_loss["generator"] += r[8]
            ng += 1.0
        if flags & LR.HAS_DIST:
            for k, v in LR.batch_metrics(dist, kind, Ds, T._LOGDB_CONST).items():
                running_metrics[k] = running_metrics.get(k, 0.0) + float(v)
    out = dict(running_loss, real_correct=float(real), fake_correct=float(fake), d_updates=nd, g_updates=ng)
    out.update(running_metrics)
    return [out.get(k, 0.0) for k in LR.KEYS] + [0.0] * (LR.SLOTS - len(LR.KEYS))


def _steps(name, seed=3, n=5, unvoiced_at=None):
    rs = np.random.RandomState(seed)
    steps = []
    for i in range(n):
        res = (rs.rand(12) * 3.0).astype(np.float32)
        res[1], res[3], res[4] = np.float32(0.1), np.float32(16384.0), np.float32(float(rs.randint(0, 16384)))
        steps.append((res, _sums(rs, 0 if i == unvoiced_at else None), LR.HAS_D | LR.HAS_G | LR.HAS_DIST))
    return steps


def _ledger(steps, name, add=None, trace=False):
    """The record after the last add; ``trace``: the records after every add, back to back (what the device test compares too)."""
    led, seen = LR.Ledger(), []
    for res, dist, flags in steps:
        (add or LR.Ledger.add)(led, res, dist, flags, LR.KIND_OF[name], DS[name], T._LOGDB_CONST)
        seen += led.slots
    return seen if trace else led.slots


@pytest.mark.parametrize("name", ["acoustic", "duration", "vc"])
def test_reference_ledger_is_the_host_loop(name):
    steps = _steps(name)
    assert LR.same_bits(_ledger(steps, name), _host_loop(steps, name))
    mixed = [(r, d, f) for (r, d, _), f in zip(steps, (LR.HAS_D, LR.HAS_G | LR.HAS_DIST, LR.HAS_D | LR.HAS_G | LR.HAS_DIST, LR.HAS_G, LR.HAS_D))]
    assert LR.same_bits(_ledger(mixed, name), _host_loop(mixed, name))


def test_a_nan_stays_in_its_slot_only():
    steps = _steps("acoustic", unvoiced_at=2)
    got = _ledger(steps, "acoustic")
    i = LR.KEYS.index("f0_rmse")
    assert math.isnan(got[i]) and not any(math.isnan(v) for k, v in enumerate(got) if k != i)
    assert LR.same_bits(got, _host_loop(steps, "acoustic"))


# ---- the comparator rejects seeded mistakes ---------------------------------------------------------------------------------
def _mistaken_add(mistake):
    def add(led, res, dist, flags, kind, Ds, C):
        s, before = led.slots, list(led.slots)
        LR.Ledger.add(led, res, dist, flags, kind, Ds, C)
        s_mcd, s_bap, s_f0, nv, _, _, n = dist
        i = LR.KEYS.index
        if mistake == "product_after_quotient":
            s[i("mcd")] = before[i("mcd")] + C * (s_mcd / n)
        elif mistake == "bap_without_tenth":
            s[i("bap_mcd")] = before[i("bap_mcd")] + (C * s_bap) / n
        elif mistake == "nan_as_zero":
            s[i("f0_rmse")] = before[i("f0_rmse")] + (math.sqrt(s_f0 / nv) if nv > 0 else 0.0)
        elif mistake == "slots_swapped":
            s[i("mse")], s[i("mge")] = before[i("mse")] + float(res[6]), before[i("mge")] + float(res[5])
        elif mistake == "float32_accumulation":
            for k in range(LR.SLOTS):
                s[k] = float(np.float32(before[k]) + np.float32(s[k] - before[k]))
        else:
            raise KeyError(mistake)
    return add


@pytest.mark.parametrize("mistake", ["product_after_quotient", "bap_without_tenth", "nan_as_zero", "slots_swapped", "float32_accumulation"])
def test_comparator_rejects_seeded_mistakes(mistake):
    steps = _steps("acoustic", seed=6, unvoiced_at=2)      # (a seed whose first batch already rounds apart under both orders)
    good = _ledger(steps, "acoustic", trace=True)
    assert LR.same_bits(good, _ledger(steps, "acoustic", trace=True))
    assert not LR.same_bits(good, _ledger(steps, "acoustic", _mistaken_add(mistake), trace=True)), mistake
