"""gt_op_assemble_batch and gantts_amd.data.ResidentLoader on the device against the host pipeline (tests/resident_ref.py): every batch
bit for bit -- x, y, y_static, mask, lengths and the noise --, pad columns and padded frames exactly 0, sentinels around every output
buffer intact; recomputed deltas inside the float64 bound; one train_loop epoch against the host pipeline fed the same batches; the
prefix view generator_input[:, :, :Dx] as D's conditioning x against separately pitched tensors; the refusal of a corpus that does not fit."""
import copy
import types

import numpy as np
import pytest
import torch

import cases as C
import resident_ref as R
from gantts_amd import data as D

pytestmark = pytest.mark.gpu

SENT = 1.2345e30
GUARD = 64
BATCHES = {1: [[i] for i in range(9)], 4: [[0, 1, 2, 3], [4, 5, 6, 7], [8]], 9: [list(range(9))]}


def _guarded(shape, dtype=torch.float32):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENT if dtype == torch.float32 else -77, device="cuda", dtype=dtype)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _intact(buf, n):
    v = SENT if buf.dtype == torch.float32 else -77
    return bool((buf[:GUARD] == v).all()) and bool((buf[GUARD + n:] == v).all())


def _run(ds, hp, batches, key1=0):
    """Every batch of one epoch through ResidentLoader.assemble into guarded buffers: dicts as resident_ref.reference_batches gives."""
    loader = D.ResidentLoader(ds, 1, False, hp, batch_sampler=batches, first_draw=key1)
    case, plan = loader.begin_epoch()
    c, nz, Ds = loader.corpus, loader.nz, len(loader.scol_host)
    ld = (c.Dx + nz + 3) // 4 * 4
    out = []
    for first, B, T, cpu_lengths in plan:
        shapes = ((B, T, ld), (B, T, c.Dy), (B, T, Ds), (B, T, 1), (B,))
        pairs = [_guarded(s, torch.int64 if i == 4 else torch.float32) for i, s in enumerate(shapes)]
        loader.assemble(case, first, B, T, out=tuple(v for _, v in pairs))
        torch.cuda.synchronize()
        for (buf, v), name in zip(pairs, ("gi", "y", "y_static", "mask", "lengths")):
            assert _intact(buf, v.numel()), "sentinels around %s" % name
        gi, y, ys, mask, lengths = [v.cpu().numpy() for _, v in pairs]
        assert not gi[:, :, c.Dx + nz:].any(), "pad columns of gi"
        assert lengths.tolist() == cpu_lengths
        for b, n in enumerate(cpu_lengths):
            assert not gi[b, n:, :c.Dx].any() and not y[b, n:].any() and not ys[b, n:].any(), "padded frames"
        out.append(dict(x=np.ascontiguousarray(gi[:, :, :c.Dx]), y=y, y_static=ys, mask=mask, lengths=lengths,
                        z=np.ascontiguousarray(gi[:, :, c.Dx:c.Dx + nz]) if nz else None))
    return out


def _check(ds, hp, batches, key1=0):
    got, ref = _run(ds, hp, batches, key1), R.reference_batches(ds, hp, batches, key1)
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert R.mismatches(g, r) == [], "batch %d" % k
        for name in ("x", "y", "y_static", "mask", "lengths"):
            assert torch.equal(torch.from_numpy(g[name]), torch.from_numpy(r[name]))
        if r["z"] is not None:
            assert g["z"].min() >= 0.0 and g["z"].max() < 1.0


@pytest.mark.parametrize("bs", [1, 4, 9])
@pytest.mark.parametrize("nz", [0, 5])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["tts", "vc"])
def test_batches_equal_the_host_pipeline_bit_for_bit(kind, dtype, nz, bs):
    widths = R.SMALL if kind == "tts" else R.VC
    hp = R.make_hp(widths, nz=nz, name="acoustic" if kind == "tts" else "vc")
    _check(R.make_dataset(kind, widths, dtype, hp=hp), hp, BATCHES[bs], key1=3)


def test_batches_at_the_real_widths():
    """425 / 187 columns on pitches 428 / 188, Ds = 63; shorter utterances keep the case quick (ties, 1 frame, more than one workgroup)."""
    hp = R.make_hp(R.REAL, nz=5)
    ds = R.make_dataset("tts", R.REAL, np.float64, lengths=[37, 50, 5, 50, 1, 50], hp=hp)
    _check(ds, hp, [[0, 1, 2, 3], [4, 5]], key1=1)


def test_each_side_computes_in_its_own_statistics_dtype():
    """float32 min-max statistics beside float64 mean / variance: what minmax() of float32 utterances and meanvar() give."""
    hp = R.make_hp(R.SMALL, nz=5)
    ds = R.make_dataset("tts", R.SMALL, np.float64, hp=hp)
    ds.X_data_min, ds.X_data_scale = ds.X_data_min.astype(np.float32), ds.X_data_scale.astype(np.float32)
    _check(ds, hp, BATCHES[4])
    ds = R.make_dataset("tts", R.SMALL, np.float32, hp=hp)
    ds.X_data_min, ds.X_data_scale = ds.X_data_min.astype(np.float64), ds.X_data_scale.astype(np.float64)
    _check(ds, hp, BATCHES[4])


def test_noise_follows_the_utterance_and_the_draw_counter():
    hp = R.make_hp(R.SMALL, nz=5)
    ds = R.make_dataset("tts", R.SMALL, np.float64, hp=hp)
    a = _run(ds, hp, [[1, 3]], key1=0)[0]["z"]            # two utterances of 120 frames
    b = _run(ds, hp, [[3, 1, 8]], key1=0)[0]["z"]         # torch.sort decides their places
    order = R.reference_batches(ds, hp, [[3, 1, 8]])[0]["order"]
    assert np.array_equal(a[0], b[order.index(1)]) and np.array_equal(a[1], b[order.index(3)])
    assert not np.array_equal(a, _run(ds, hp, [[1, 3]], key1=1)[0]["z"])
    loader = D.ResidentLoader(ds, 9, False, hp)
    first, second = [next(iter(loader)).generator_input[:, :, 7:].cpu().numpy() for _ in range(2)]
    assert loader.draws == 2 and not np.array_equal(first, second)


def test_the_loader_yields_prefix_views_of_one_buffer():
    hp = R.make_hp(R.SMALL, nz=5)
    ds = R.make_dataset("tts", R.SMALL, np.float64, hp=hp)
    ref = R.reference_batches(ds, hp, BATCHES[4])
    got = list(D.ResidentLoader(ds, 4, False, hp))
    assert len(got) == 3
    for b, r in zip(got, ref):
        assert b.generator_input.shape == (len(r["order"]), r["T"], 12) and b.generator_input.stride(1) == 12
        assert b.x.shape[-1] == 7 and b.x.data_ptr() == b.generator_input.data_ptr() and b.x.stride() == b.generator_input.stride()
        assert torch.equal(b.generator_input[:, :, :7], b.x) and b.max_len == r["T"] and b.cpu_lengths == r["lengths"].tolist()
        assert np.array_equal(b.generator_input.cpu().numpy(), r["gi"]) and np.array_equal(b.y.cpu().numpy(), r["y"])
        assert np.array_equal(b.y_static.cpu().numpy(), r["y_static"]) and np.array_equal(b.mask.cpu().numpy(), r["mask"])
        assert np.array_equal(b.lengths.cpu().numpy(), r["lengths"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_recomputed_deltas_are_inside_the_float64_bound(dtype):
    """|got - v| <= 2^-24 |v| + 2^-45 sum_k |coef_k x_k| against the float64 host value v of the dataset's own scaled columns; window 0
    ([1.0]) and the stream without dynamic features bit for bit against the host pipeline (resident_ref.delta_mismatches)."""
    hp = R.make_hp(R.SMALL, nz=5, recompute=True)
    ds = R.make_dataset("tts", R.SMALL, dtype, lengths=R.LENGTHS_DELTA, hp=hp)
    for batches in (BATCHES[4], BATCHES[9]):
        got, ref = _run(ds, hp, batches), R.reference_batches(ds, hp, batches)
        for k, (g, r) in enumerate(zip(got, ref)):
            assert R.delta_mismatches(g, r, ds, hp) == [], "batch %d" % k


def test_a_corpus_that_does_not_fit_is_refused_before_anything_is_allocated(monkeypatch):
    hp = R.make_hp(R.SMALL, nz=5)
    ds = R.make_dataset("tts", R.SMALL, np.float64, hp=hp)
    corpus = D.ResidentCorpus(ds, device=None)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (D.RESIDENT_MARGIN_BYTES + corpus.nbytes - 1, 1 << 40))
    allocated = []
    for name in ("empty", "zeros"):
        real = getattr(torch, name)
        monkeypatch.setattr(torch, name, lambda *a, _real=real, **k: (allocated.append(a), _real(*a, **k))[1])
    with pytest.raises(RuntimeError, match=r"%d bytes do not fit.*%d bytes free" % (corpus.nbytes, D.RESIDENT_MARGIN_BYTES + corpus.nbytes - 1)):
        corpus.upload("cuda")
    assert allocated == [] and corpus.X_all is None
    with pytest.raises(RuntimeError, match="do not fit"):
        next(iter(D.ResidentLoader(ds, 4, False, hp)))


# ---- the prefix view as D's conditioning x ---------------------------------------------------------------------------------------
def _step_run(case, gi, x, y_np, lengths):
    """The steps of hip_runner.run_hip_case with the generator input and the conditioning x handed over separately."""
    import gantts_amd.train as T
    from gantts_amd import optim, paramgen
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model, make_hp, state_arrays
    hp = make_hp(case)
    saved = T.hp
    T.hp = hp
    try:
        mg, md = build_model(case["g"], 11), build_model(case["d"], 22)
        mg.train(), md.train()
        og = getattr(optim, case["opt_g"][0])(mg.parameters(), **case["opt_g"][1])
        od = getattr(optim, case["opt_d"][0])(md.parameters(), **case["opt_d"][1])
        y = torch.from_numpy(y_np).cuda()
        Tn = case["T"]
        Rm = paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, Tn)
        sl, cpu_lengths = torch.from_numpy(np.ascontiguousarray(lengths)).cuda(), list(lengths)
        out = {}
        for step in range(case["steps"]):
            gm, dm = C.make_dropout_masks(case, step)
            nh = len(C.hidden_sites(case["d"]))
            mg.set_dropout_masks(0, [torch.from_numpy(m) for m in gm])
            for p in range(3):
                md.set_dropout_masks(p, [torch.from_numpy(m) for m in dm[p * nh:(p + 1) * nh]])
            y_static = get_static_features(y, len(hp.windows), hp.stream_sizes, hp.has_dynamic_features)
            mask = sequence_mask(sl, max_len=Tn).unsqueeze(-1)
            og.zero_grad(), od.zero_grad()
            y_hat, y_hat_static = T.apply_generator(mg, gi, Rm, cpu_lengths)
            if step == 0:
                out["y_hat"], out["y_hat_static"] = y_hat.cpu().numpy(), y_hat_static.cpu().numpy()
            out["d_scalars_%d" % step] = np.array(T.update_discriminator(md, od, x, y_static, y_hat_static, cpu_lengths, mask, "train"), dtype=np.float64)
            out["g_scalars_%d" % step] = np.array(T.update_generator(mg, md, og, x, y, y_hat, y_static, y_hat_static, case["adv_w"], cpu_lengths, mask,
                                                                     "train", mse_w=case["mse_w"], mge_w=case["mge_w"]), dtype=np.float64)
        torch.cuda.synchronize()
        out.update(state_arrays(mg, md, og, od))
        return out
    finally:
        T.hp = saved


def test_the_step_reads_x_as_a_prefix_view_of_the_generator_input():
    """acoustic_chain_d with 5 noise columns: generator_input on pitch roundup(30 + 5, 4) = 36 and the conditioned D reading x from it at that
    pitch, against a cat-made generator input and an x on its own pitch of 32: the same values, so every result equal bit for bit."""
    from gantts_amd.engine import pitched_empty
    nz = 5
    case = copy.deepcopy(C.CASES["acoustic_chain_d"])
    case["g"]["in_dim"] = case["din"] + nz
    x_np, y_np, lengths = C.make_batch(case)
    B, Tn, Dx = x_np.shape
    z_np = np.stack([R.noise(7, 0, u, Tn, nz) for u in range(B)])
    x, z = torch.from_numpy(x_np).cuda(), torch.from_numpy(z_np).cuda()
    gi_a, x_a = pitched_empty(B, Tn, Dx + nz), pitched_empty(B, Tn, Dx)
    gi_a.copy_(torch.cat((x, z), -1))
    x_a.copy_(x)
    assert gi_a.stride(1) == 36 and x_a.stride(1) == 32
    ref = _step_run(case, gi_a, x_a, y_np, lengths)
    gi_b = pitched_empty(B, Tn, Dx + nz)
    gi_b.copy_(torch.cat((x, z), -1))
    x_b = gi_b[:, :, :Dx]
    assert x_b.stride(1) == 36 and x_b.data_ptr() == gi_b.data_ptr()
    got = _step_run(case, gi_b, x_b, y_np, lengths)
    assert sorted(got) == sorted(ref) and len(ref) > 10
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k


# ---- one train_loop epoch ------------------------------------------------------------------------------------------------------------
TRAIN_BATCHES = {"train": [[0, 1, 2, 3], [4, 5, 6, 7], [8]], "test": [[2, 0], [1]]}


def _train_loop_run(resident, monkeypatch):
    import gantts_amd.train as T
    from gantts_amd import hparams, multistream, optim, seqloss
    from hip_runner import build_model
    nz = 5
    hp = types.SimpleNamespace(**hparams.tts_acoustic.values())
    hp.stream_sizes, hp.has_dynamic_features, hp.windows = R.SMALL["stream_sizes"], R.SMALL["has_dynamic_features"], R.WINDOWS
    hp.adversarial_streams, hp.mask_nth_mgc_for_adv_loss, hp.discriminator_linguistic_condition = [True, False, False, False], 0, True
    hp.nepoch, hp.lr_decay_schedule, hp.lr_decay_epoch = 1, False, 10
    hp.generator_add_noise, hp.generator_noise_dim, hp.generator_noise_seed = True, nz, 99
    hp.optimizer_g_params, hp.optimizer_d_params = dict(lr=0.01, weight_decay=1e-7), dict(lr=0.01, weight_decay=1e-7)
    hp.resident_corpus = resident
    datasets = {"train": R.make_dataset("tts", R.SMALL, np.float64, hp=hp, seed=5),
                "test": R.make_dataset("tts", R.SMALL, np.float64, lengths=[30, 9, 30], hp=hp, seed=6)}
    draw0 = {"train": 0, "test": 1 << 31}
    g = dict(kind="MLP", in_dim=7 + nz, out_dim=13, num_hidden=2, hidden_dim=16, dropout=0.0, last_sigmoid=False)
    d = dict(kind="MLP", in_dim=7 + 2, out_dim=1, num_hidden=2, hidden_dim=128, dropout=0.0, last_sigmoid=True)
    mg, md = build_model(g, 11), build_model(d, 22)
    og, od = optim.Adagrad(mg.parameters(), **hp.optimizer_g_params), optim.Adagrad(md.parameters(), **hp.optimizer_d_params)
    loaders = {}
    if resident:
        for ph in datasets:
            loaders[ph] = D.ResidentLoader(datasets[ph], 4, ph == "train", hp, batch_sampler=TRAIN_BATCHES[ph], first_draw=draw0[ph])

        def forbidden(name):
            def f(*a, **k):
                raise AssertionError("the resident path called %s" % name)
            return f
        monkeypatch.setattr(torch, "rand", forbidden("torch.rand"))
        monkeypatch.setattr(torch, "cat", forbidden("torch.cat"))
        monkeypatch.setattr(multistream, "get_static_features", forbidden("get_static_features"))
        monkeypatch.setattr(seqloss, "sequence_mask", forbidden("sequence_mask"))
    else:
        class Loader(list):
            pass
        zs = []
        for ph in ("train", "test"):      # the host pipeline on the same index batches, in train_loop's order; z from the reference
            ld = Loader(D.collate_fn([datasets[ph][i] for i in idx]) for idx in TRAIN_BATCHES[ph])
            ld.dataset = datasets[ph]
            loaders[ph] = ld
            zs += [torch.from_numpy(r["z"]) for r in R.reference_batches(datasets[ph], hp, TRAIN_BATCHES[ph], key1=draw0[ph])]

        def rand(*shape, device=None, generator=None):
            z = zs.pop(0)
            assert tuple(z.shape) == tuple(shape)
            return z.to(device)
        monkeypatch.setattr(torch, "rand", rand)
    logs = []
    saved = T.hp, T.global_epoch, T.log_value
    T.hp, T.global_epoch, T.log_value = hp, 0, lambda n, v, e: logs.append((n, float(v)))
    try:
        assert T.train_loop((mg, md), (og, od), loaders, w_d=1.0, mse_w=0.0, mge_w=1.0) == 0
    finally:
        T.hp, T.global_epoch, T.log_value = saved
        monkeypatch.undo()
    return logs, {t + "." + k: v.cpu().numpy() for t, m in (("G", mg), ("D", md)) for k, v in m.state_dict().items()}


def test_train_loop_on_a_resident_corpus_equals_the_host_pipeline(monkeypatch):
    """An epoch's train and test phase, MLP generator with noise, conditioned MLP discriminator, no dropout: both runs execute the same
    step on bit-identical inputs, so every logged value and every parameter is equal; the resident run may not call torch.rand,
    torch.cat, get_static_features or sequence_mask (they raise)."""
    ref_logs, ref_params = _train_loop_run(False, monkeypatch)
    got_logs, got_params = _train_loop_run(True, monkeypatch)
    assert [n for n, _ in got_logs] == [n for n, _ in ref_logs] and len(ref_logs) > 15
    for (n, g), (_, r) in zip(got_logs, ref_logs):
        assert g == r or (g != g and r != r), "%s: %r != %r" % (n, g, r)
    assert any("loss" in n and v != 0 for n, v in ref_logs)
    for k in ref_params:
        assert np.array_equal(got_params[k], ref_params[k]), k
