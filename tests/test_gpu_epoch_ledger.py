"""The epoch ledger on the device (gt_ledger_*, gt_op_epoch_ledger; hp.device_epoch_ledger in train_loop):
1. epoch_ledger_kernel against tests/ledger_ref.py, all 32 doubles exactly, after each of five successive adds, inside a guarded buffer;
2. the device-side distortion sums of gt_ledger_add against gt_compute_distortions, bit for bit;
3. train_loop with the switch on against the switch off: every logged value, every parameter and optimizer-state tensor, bit for bit;
4. the host waits once per phase with the switch on, at least twice per batch with it off (gt_host_wait_count);
5. the duration and the vc loop."""
import copy
import math
import types

import numpy as np
import pytest
import torch

import cases as CS
import ledger_ref as LR
import resident_ref as R
from gantts_amd import _lib as L
from gantts_amd import data as D

pytestmark = pytest.mark.gpu

SENT = -7.25e300
GUARD = 24


def _f64_view(addr, n):
    class _Arr(object):
        __cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (addr, False), "version": 2}
    return torch.as_tensor(_Arr(), device="cuda")


# ---- 1. the operator --------------------------------------------------------------------------------------------------------
def _results(rs, i):
    """12 float32 results with distinct values in every field: sums that round (0.1f), a large count (16384.0f)."""
    r = (rs.rand(12) * 4.0 + 0.01 * (i + 1)).astype(np.float32)
    r[1] = np.float32(0.1)
    r[3] = np.float32(16384.0)
    r[4] = np.float32(float(rs.randint(1, 16384)))
    r[6] = np.float32(0.1) * np.float32(i + 1)
    return r


def _dist(rs, n_voiced=None):
    n = float(rs.randint(40, 4000))
    nv = float(rs.randint(1, int(n)))       # drawn either way: a forced n_voiced leaves every later draw where it was
    nv = nv if n_voiced is None else float(n_voiced)
    return np.array([rs.rand() * n * 3.0, rs.rand() * n * 1.7, rs.rand() * nv * 900.0, nv, float(rs.randint(0, int(n))), rs.rand() * n * 11.0, n])


def _op_run(kind, Ds, flags_per_add, unvoiced_at=None, seed=0):
    """Five adds through gt_op_epoch_ledger into a record inside a sentinel-filled buffer; after each add the 32 doubles and the
    guards are compared with the reference."""
    import gantts_amd.train as T
    rs = np.random.RandomState(seed)
    buf = torch.full((LR.SLOTS + 2 * GUARD,), SENT, device="cuda", dtype=torch.float64)
    buf[GUARD:GUARD + len(LR.KEYS)] = 0.0
    rec = buf[GUARD:GUARD + LR.SLOTS]
    ref = LR.Ledger()
    traces = []
    for i, flags in enumerate(flags_per_add):
        res, dist = _results(rs, i), _dist(rs, 0 if i == unvoiced_at else None)
        res_d, dist_d = torch.from_numpy(res).cuda(), torch.from_numpy(dist).cuda()
        L.check(L.lib.gt_op_epoch_ledger(L.ptr(rec), L.ptr(res_d), L.ptr(dist_d) if flags & LR.HAS_DIST else None, flags, kind, Ds,
                                         T._LOGDB_CONST, L.current_stream()))
        torch.cuda.synchronize()
        ref.add(res, dist, flags, kind, Ds, T._LOGDB_CONST)
        want = ref.slots[:len(LR.KEYS)] + [SENT] * (LR.SLOTS - len(LR.KEYS))
        got = buf.cpu().tolist()
        assert got[:GUARD] == [SENT] * GUARD and got[GUARD + LR.SLOTS:] == [SENT] * GUARD, "words outside the record, add %d" % i
        rec_now = got[GUARD:GUARD + LR.SLOTS]
        assert LR.same_bits(rec_now, want), "add %d: %s" % (i, [(k, a, b) for k, a, b in zip(LR.KEYS, rec_now, want) if not LR.same_bits([a], [b])])
        traces.append(rec_now)
    return traces


FLAG_SETS = {"D": LR.HAS_D, "G": LR.HAS_G, "DG": LR.HAS_D | LR.HAS_G, "DG+DIST": LR.HAS_D | LR.HAS_G | LR.HAS_DIST}


@pytest.mark.parametrize("flags", sorted(FLAG_SETS))
@pytest.mark.parametrize("kind,Ds", [(LR.ACOUSTIC, 5), (LR.DURATION, 1), (LR.DURATION, 25), (LR.VC, 25), (LR.VC, 5)],
                         ids=["acoustic-5", "duration-1", "duration-25", "vc-25", "vc-5"])
def test_operator_equals_the_reference_ledger(kind, Ds, flags):
    tr = _op_run(kind, Ds, [FLAG_SETS[flags]] * 5, seed=Ds)
    i = LR.KEYS.index
    assert tr[-1][i("d_updates")] == (5.0 if FLAG_SETS[flags] & LR.HAS_D else 0.0)
    assert tr[-1][i("g_updates")] == (5.0 if FLAG_SETS[flags] & LR.HAS_G else 0.0)
    if flags == "DG+DIST":
        live = {LR.ACOUSTIC: ("mcd", "bap_mcd", "f0_rmse", "vuv_err"), LR.DURATION: ("dur_rmse",), LR.VC: ("mcd",)}[kind]
        for k in ("mcd", "bap_mcd", "f0_rmse", "vuv_err", "dur_rmse"):
            assert (tr[-1][i(k)] > 0.0) == (k in live), k


def test_operator_with_a_different_flag_set_per_add():
    _op_run(LR.ACOUSTIC, 5, [LR.HAS_D, LR.HAS_G | LR.HAS_DIST, LR.HAS_D | LR.HAS_G | LR.HAS_DIST, LR.HAS_G, LR.HAS_D], seed=9)


def test_operator_keeps_the_nan_of_a_batch_without_voiced_frames():
    tr = _op_run(LR.ACOUSTIC, 5, [LR.HAS_D | LR.HAS_G | LR.HAS_DIST] * 5, unvoiced_at=2, seed=4)
    clean = _op_run(LR.ACOUSTIC, 5, [LR.HAS_D | LR.HAS_G | LR.HAS_DIST] * 5, seed=4)
    f0 = LR.KEYS.index("f0_rmse")
    for k, (a, b) in enumerate(zip(tr, clean)):
        assert math.isnan(a[f0]) == (k >= 2)
        # the two runs differ only in n_voiced (and s_f0) of add 2: every other slot is unaffected, before and after
        assert LR.same_bits([v for j, v in enumerate(a) if j != f0], [v for j, v in enumerate(b) if j != f0])
        if k < 2:
            assert LR.same_bits(a, b)


def test_operator_refuses_bad_arguments():
    rec = torch.zeros(32, device="cuda", dtype=torch.float64)
    res = torch.zeros(12, device="cuda")
    st = L.current_stream()
    assert L.lib.gt_op_epoch_ledger(L.ptr(rec), L.ptr(res), None, LR.HAS_DIST, 0, 5, 1.0, st) == L.GT_ERR_INVALID
    assert L.lib.gt_op_epoch_ledger(L.ptr(rec), L.ptr(res), None, 8, 0, 5, 1.0, st) == L.GT_ERR_INVALID
    assert L.lib.gt_op_epoch_ledger(L.ptr(rec), L.ptr(res), None, LR.HAS_D, 3, 5, 1.0, st) == L.GT_ERR_INVALID
    assert L.lib.gt_op_epoch_ledger(None, L.ptr(res), None, LR.HAS_D, 0, 5, 1.0, st) == L.GT_ERR_INVALID
    torch.cuda.synchronize()
    assert not rec.any()


# ---- 2. device-side distortion sums -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("lengths", [[17, 9, 1], None], ids=["ragged", "full"])
def test_device_side_distortion_sums_equal_gt_compute_distortions(dtype, lengths):
    import gantts_amd.train as T
    from gantts_amd.engine import StepEngine
    hp = R.make_hp(R.SMALL)
    saved = T.hp
    T.hp = hp
    try:
        roles, stats, vuv_col, _ = T._acoustic_columns()
        g = torch.Generator().manual_seed(17)
        B, Tn, Ds = 3, 17, len(roles)
        y, yh = torch.randn(B, Tn, Ds, generator=g).cuda(), torch.randn(B, Tn, Ds, generator=g).cuda()
        mean, std = (torch.randn(13, generator=g) * 0.3).to(dtype), (0.5 + torch.rand(13, generator=g)).to(dtype)
        mean[stats[vuv_col]], std[stats[vuv_col]] = 0.5, 0.5      # half of the frames voiced on either side
        mean, std = mean.cuda(), std.cuda()
        want = T._distortion_sums(y, yh, mean, std, roles, stats, vuv_col, lengths)
        want = [want.s_mcd, want.s_bap, want.s_f0, want.n_voiced, want.n_vuv_err, want.s_mse, want.n_frames]
        eng = StepEngine(hp)
        eng.ledger_configure(L.LEDGER_ACOUSTIC, roles, stats, vuv_col, mean, std, T._LOGDB_CONST)
        eng.ledger_reset()
        lens = None if lengths is None else torch.tensor(lengths, dtype=torch.int64).cuda()
        waits = eng.host_waits()
        eng.ledger_add(L.LEDGER_HAS_DIST, y, yh, lens)
        assert eng.host_waits() == waits
        torch.cuda.synchronize()
        got = _f64_view(eng.ledger_buffers()[1], 7).cpu().tolist()
        assert want[6] == (27.0 if lengths else 51.0) and want[3] > 0 and want[0] > 0 and want[1] > 0 and want[2] > 0
        assert LR.same_bits(got, want), (got, want)
        # ... and the record holds that one batch's metrics
        led = eng.ledger_read()
        ref = LR.batch_metrics(want, LR.ACOUSTIC, Ds, T._LOGDB_CONST)
        assert LR.same_bits([led[k] for k in ref], [ref[k] for k in ref])
        assert eng.host_waits() == waits + 1
    finally:
        T.hp = saved


# ---- 3. the whole loop ------------------------------------------------------------------------------------------------------
TRAIN_BATCHES = {"train": [[0, 1, 2, 3], [4, 5, 6, 7], [8]], "test": [[2, 0, 3, 1]]}


class _Loop(object):
    """One (G, D, optimizers, loaders) set of the small acoustic layout; ``epoch(ledger)`` runs train_loop for one epoch (train and
    test phase) with hp.device_epoch_ledger = ledger and returns the logged (name, value) pairs."""

    def __init__(self, resident, dropout=0.0):
        from gantts_amd import hparams, optim
        from gantts_amd.engine import engine_for
        from hip_runner import build_model
        nz = 5
        hp = types.SimpleNamespace(**hparams.tts_acoustic.values())
        hp.stream_sizes, hp.has_dynamic_features, hp.windows = R.SMALL["stream_sizes"], R.SMALL["has_dynamic_features"], R.WINDOWS
        hp.adversarial_streams, hp.mask_nth_mgc_for_adv_loss, hp.discriminator_linguistic_condition = [True, False, False, False], 0, True
        hp.nepoch, hp.lr_decay_schedule, hp.lr_decay_epoch = 1, False, 10
        hp.generator_add_noise, hp.generator_noise_dim, hp.generator_noise_seed = True, nz, 99
        hp.optimizer_g_params, hp.optimizer_d_params = dict(lr=0.01, weight_decay=1e-7), dict(lr=0.01, weight_decay=1e-7)
        hp.resident_corpus = resident
        self.hp = hp
        datasets = {"train": R.make_dataset("tts", R.SMALL, np.float64, hp=hp, seed=5),
                    "test": R.make_dataset("tts", R.SMALL, np.float64, lengths=[30, 9, 30, 17], hp=hp, seed=6)}
        g = dict(kind="MLP", in_dim=7 + nz, out_dim=13, num_hidden=2, hidden_dim=16, dropout=dropout, last_sigmoid=False)
        d = dict(kind="MLP", in_dim=7 + 2, out_dim=1, num_hidden=2, hidden_dim=128, dropout=dropout, last_sigmoid=True)
        self.mg, self.md = build_model(g, 11), build_model(d, 22)
        self.og = optim.Adagrad(self.mg.parameters(), **hp.optimizer_g_params)
        self.od = optim.Adagrad(self.md.parameters(), **hp.optimizer_d_params)
        self.engine = engine_for(hp, self.mg)
        self.engine.set_seed(20240611)      # the dropout streams: a fixed seed, the same in every run
        self.loaders = {}
        for ph in datasets:
            if resident:
                self.loaders[ph] = D.ResidentLoader(datasets[ph], 4, ph == "train", hp, batch_sampler=TRAIN_BATCHES[ph],
                                                    first_draw={"train": 0, "test": 1 << 31}[ph])
            else:
                class Loader(list):
                    pass
                ld = Loader(D.collate_fn([datasets[ph][i] for i in idx]) for idx in TRAIN_BATCHES[ph])
                ld.dataset = datasets[ph]
                self.loaders[ph] = ld

    def epoch(self, ledger, monkeypatch=None, **kw):
        import gantts_amd.train as T
        self.hp.device_epoch_ledger = ledger
        logs = []
        saved = T.hp, T.global_epoch, T.log_value
        T.hp, T.global_epoch, T.log_value = self.hp, 0, lambda n, v, e: logs.append((n, float(v)))
        if ledger and monkeypatch is not None:
            def forbidden(name):
                def f(*a, **k):
                    raise AssertionError("the ledger path called train.%s" % name)
                return f
            for name in ("update_discriminator", "update_generator", "compute_distortions"):
                monkeypatch.setattr(T, name, forbidden(name))
        args = dict(w_d=1.0, mse_w=0.0, mge_w=1.0)
        args.update(kw)
        try:
            assert T.train_loop((self.mg, self.md), (self.og, self.od), self.loaders, **args) == 0
        finally:
            T.hp, T.global_epoch, T.log_value = saved
            if monkeypatch is not None:
                monkeypatch.undo()
        return logs

    def state(self):
        from hip_runner import state_arrays
        return state_arrays(self.mg, self.md, self.og, self.od)


def _same_logs(got, ref):
    assert [n for n, _ in got] == [n for n, _ in ref]
    for (n, g), (_, r) in zip(got, ref):
        assert LR.same_bits([g], [r]), "%s: %r != %r" % (n, g, r)


def _same_state(got, ref):
    assert sorted(got) == sorted(ref) and len(ref) > 10
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k


def _off_off_on(monkeypatch, resident, dropout, min_logs, **kw):
    runs = []
    for ledger in (False, False, True):
        loop = _Loop(resident, dropout)
        runs.append((loop.epoch(ledger, monkeypatch, **kw), loop.state()))
    (a_logs, a_state), (b_logs, b_state), (on_logs, on_state) = runs
    assert len(a_logs) >= min_logs and any("loss" in n and v != 0 for n, v in a_logs)
    _same_logs(b_logs, a_logs)       # the comparison is fair: the switch-off loop repeats itself bit for bit
    _same_state(b_state, a_state)
    _same_logs(on_logs, a_logs)
    _same_state(on_state, a_state)
    return a_logs


@pytest.mark.parametrize("dropout", [0.0, 0.5], ids=["nodrop", "dropout"])
@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host-loader"])
def test_train_loop_with_the_ledger_equals_the_loop_without(monkeypatch, resident, dropout):
    logs = _off_off_on(monkeypatch, resident, dropout, 16)
    names = [n for n, _ in logs]
    for n in ("E(mge)", "E(adv)", "train mcd metric", "test f0_rmse metric", "Real train acc", "Fake test acc", "test generator loss"):
        assert n in names, n


def test_train_loop_with_the_ledger_in_the_discriminator_warm_up(monkeypatch):
    logs = _off_off_on(monkeypatch, True, 0.0, 10, update_g=False)
    assert not any("metric" in n or "generator" in n for n, _ in logs)


def test_train_loop_with_the_ledger_generator_only(monkeypatch):
    logs = _off_off_on(monkeypatch, True, 0.0, 10, w_d=0.0, update_d=False)
    assert not any(" acc" in n or "discriminator" in n for n, _ in logs) and any("metric" in n for n, _ in logs)


# ---- 4. no host wait per batch ----------------------------------------------------------------------------------------------
def test_the_ledger_loop_waits_once_per_phase():
    loop = _Loop(True, 0.0)
    n_batches = sum(len(v) for v in TRAIN_BATCHES.values())
    loop.epoch(True)            # warm-up: every padded length's MLPG band, every workspace, the ledger's buffers
    w0 = loop.engine.host_waits()
    loop.epoch(True)
    w1 = loop.engine.host_waits()
    assert w1 - w0 == 2, "switch on: one wait per phase, got %d over two phases" % (w1 - w0)
    loop.epoch(False)
    w2 = loop.engine.host_waits()
    assert w2 - w1 >= 2 * n_batches, "switch off: %d waits over %d batches" % (w2 - w1, n_batches)


# ---- 5. duration and vc -----------------------------------------------------------------------------------------------------
DURATION_CASE = dict(
    hp="tts_duration", din=60, dout=5, stream_sizes=[5], has_dynamic_features=[False], adversarial_streams=[True], mask_nth_mgc=0,
    cond=True, windows=1, nepoch=1, lr_decay_schedule=False, lr_decay_epoch=10,
    g=dict(kind="MLP", in_dim=60, out_dim=5, num_hidden=2, hidden_dim=32, dropout=0.0, last_sigmoid=False),
    d=dict(kind="MLP", in_dim=65, out_dim=1, num_hidden=3, hidden_dim=16, dropout=0.0, last_sigmoid=True),
    opt_g=("Adam", dict(lr=1e-3, betas=(0.5, 0.9), weight_decay=0)), opt_d=("Adam", dict(lr=1e-3, betas=(0.5, 0.9), weight_decay=0)),
    batches=dict(train=[(5, 17), (3, 12)], test=[(2, 9)]), w_d=1.0, mse_w=0.0, mge_w=1.0, stats="float64")
VC_CASE = dict(copy.deepcopy(CS.TRAIN_LOOP_CASES["train_loop_vc"]), nepoch=1, batches=dict(train=[(2, 24), (2, 20)], test=[(2, 24)]))


def _case_run(case, ledger):
    import gantts_amd.train as T
    from gantts_amd import hparams, optim
    from hip_runner import build_model, state_arrays
    hp = types.SimpleNamespace(**getattr(hparams, case["hp"]).values())
    hp.stream_sizes, hp.has_dynamic_features = case["stream_sizes"], case["has_dynamic_features"]
    hp.windows = CS.WINDOWS[:case["windows"]]
    hp.adversarial_streams, hp.mask_nth_mgc_for_adv_loss = case["adversarial_streams"], case["mask_nth_mgc"]
    hp.discriminator_linguistic_condition = case["cond"]
    hp.nepoch, hp.lr_decay_schedule, hp.lr_decay_epoch = case["nepoch"], case["lr_decay_schedule"], case["lr_decay_epoch"]
    hp.generator_add_noise = False
    hp.optimizer_g_params, hp.optimizer_d_params = dict(case["opt_g"][1]), dict(case["opt_d"][1])
    hp.device_epoch_ledger = ledger
    if "order" in case:
        hp.order = case["order"]
    mg, md = build_model(case["g"], 11), build_model(case["d"], 22)
    og = getattr(optim, case["opt_g"][0])(mg.parameters(), **case["opt_g"][1])
    od = getattr(optim, case["opt_d"][0])(md.parameters(), **case["opt_d"][1])
    data, mean, std = CS.make_train_loop_data(case)

    class Loader(list):
        pass
    loaders = {}
    for phase in ("train", "test"):
        ld = Loader((torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(l)) for x, y, l in data[phase])
        ld.dataset = types.SimpleNamespace(data_mean=mean, data_std=std) if case["hp"] == "vc" \
            else types.SimpleNamespace(Y_data_mean=mean, Y_data_std=std)
        loaders[phase] = ld
    logs = []
    saved = T.hp, T.global_epoch, T.log_value
    T.hp, T.global_epoch, T.log_value = hp, 0, lambda n, v, e: logs.append((n, float(v)))
    try:
        assert T.train_loop((mg, md), (og, od), loaders, w_d=case["w_d"], mse_w=case["mse_w"], mge_w=case["mge_w"]) == 0
    finally:
        T.hp, T.global_epoch, T.log_value = saved
    return logs, state_arrays(mg, md, og, od)


@pytest.mark.parametrize("name", ["duration", "vc"])
def test_duration_and_vc_loops_with_the_ledger(name):
    case = {"duration": DURATION_CASE, "vc": VC_CASE}[name]
    off_logs, off_state = _case_run(case, False)
    on_logs, on_state = _case_run(case, True)
    assert any(n == "train %s metric" % {"duration": "dur_rmse", "vc": "mcd"}[name] for n, _ in off_logs)
    assert sum("metric" in n for n, _ in off_logs) == 2
    _same_logs(on_logs, off_logs)
    _same_state(on_state, off_state)
