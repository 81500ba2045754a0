"""gt_op_corpus_stats, ResidentCorpus.from_arrays / .minmax / .meanvar and data.resident_tts_loaders / resident_vc_loaders on the device.

min / max equal numpy's by value (NaN, +-inf included); mean / var / n inside the derived bound of tests/corpus_stats_ref.py against the
extended-precision two-pass reference, on the inputs tests/test_corpus_stats_host.py shows the host's meanvar to satisfy: widths with
3, 1, 0, 3, 1 and 1 pad columns (the pad columns of the device buffers hold NaN), row counts of one, around one slab, several slabs with
a ragged last one and more slabs than the merge has chains, utterances of 1 to 70 frames, with and without lengths; a constant column exact;
the continuation over a second side; two runs bit-identical with every sentinel intact; segments partly outside the corpus and of no
rows.  The loaders made from raw arrays: their statistics inside the bound, their batches those of the host pipeline fed the same
statistics, one train_loop epoch logging the same values, one upload per phase."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import corpus_stats_ref as S
import resident_ref as R
from gantts_amd import _lib as L
from gantts_amd import data as D

pytestmark = pytest.mark.gpu

SENT = 1.2345e30
GUARD = 64


def _poison_pads(corpus):
    corpus.X_all[:, corpus.Dx:] = float("nan")
    corpus.Y_all[:, corpus.Dy:] = float("nan")
    return corpus


def _corpus(X, Y=None):
    return _poison_pads(D.ResidentCorpus.from_arrays(X, X if Y is None else Y))


def test_the_reference_is_sized_for_the_kernel_as_built():
    assert (S.SLAB, S.FANIN) == (L.CORPUS_STATS_SLAB, L.CORPUS_STATS_FANIN)


@pytest.mark.parametrize("F", S.ROWS)
@pytest.mark.parametrize("Dn", S.WIDTHS)
def test_statistics_of_a_raw_corpus(Dn, F):
    worst = 0.0
    for family in S.FAMILIES:
        X, cut = S.make_corpus(family, F, Dn)
        corpus = _corpus(X)
        for lengths in (None, cut):
            ref = S.reference(X, lengths)
            mean, var, n = corpus.meanvar("x", lengths, return_last_sample_count=True)
            rm, rv = S.errors(mean, var, ref)
            worst = max(worst, float(rm.max()), float(rv.max()))
            print("D=%d F=%d %s lengths=%s: mean %.3g, var %.3g of the bound" % (Dn, F, family, lengths is not None, rm.max(), rv.max()))
            assert S.mismatches(mean, var, n, ref, Dn) == [], (family, lengths is not None)
            if family == "constant":
                assert S.constant_mismatches(mean, var, 0, np.float32(0.1)) == []
            lo, hi = corpus.minmax("x", lengths)
            hlo, hhi = D.minmax(X, lengths)
            assert lo.dtype == np.float32 and hi.dtype == np.float32 and lo.shape == (Dn,) and hi.shape == (Dn,)
            assert np.array_equal(lo, hlo) and np.array_equal(hi, hhi) and S.minmax_mismatches(lo, hi, X, lengths) == []
    assert worst <= 1.0


def test_min_and_max_follow_numpy_on_nan_and_infinities():
    X, cut = S.make_corpus("normal", S.SLAB + 1, 5)
    X[2][0, 1] = np.nan
    X[4][0, 3], X[len(X) - 1][0, 4] = np.inf, -np.inf
    X[0][0, 0], X[1][0, 0] = -0.0, 0.0
    corpus = _corpus(X)
    for lengths in (None, cut):
        lo, hi = corpus.minmax("x", lengths)
        assert S.minmax_mismatches(lo, hi, X, lengths) == []
        assert np.isnan(lo[1]) and np.isnan(hi[1]) and np.isfinite(lo[[0, 2, 3]]).all() and np.isfinite(hi[[0, 2]]).all()
        assert hi[3] == np.inf and lo[4] == -np.inf


@pytest.mark.parametrize("family", S.FAMILIES)
def test_the_second_side_continues_the_first(family):
    """VC's joint statistic (train.py:725-729): meanvar over x, continued over y, is the statistic of the concatenation."""
    X, cut = S.make_corpus(family, 3 * S.SLAB + 100, 63)
    Y = [np.ascontiguousarray(x[::-1] * np.float32(1.5) + np.float32(0.25)) for x in X]
    if family == "constant":
        for y in Y:
            y[:, 0] = np.float32(0.1)
    corpus = _corpus(X, Y)
    for lengths in (None, cut):
        m, v, n = corpus.meanvar("x", lengths, return_last_sample_count=True)
        mean, var, n2 = corpus.meanvar("y", lengths, mean_=m, var_=v, last_sample_count=n, return_last_sample_count=True)
        both = S.reference(X + Y, None if lengths is None else cut + cut)
        assert S.mismatches(mean, var, n2, both, 63) == []
        if family == "constant":
            assert S.constant_mismatches(mean, var, 0, np.float32(0.1)) == []
    # an empty selection returns the prior, as the host does
    none = [0] * len(X)
    got = corpus.meanvar("y", none, mean_=m, var_=v, last_sample_count=n, return_last_sample_count=True)
    want = D.meanvar(Y, none, mean_=m, var_=v, last_sample_count=n, return_last_sample_count=True)
    assert got[2] == want[2] == n and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[0], m)
    got, want = corpus.meanvar("y", none, return_last_sample_count=True), D.meanvar(Y, none, return_last_sample_count=True)
    assert got[2] == want[2] == 0 and np.array_equal(got[0], np.broadcast_to(want[0], (63,))) and np.array_equal(got[1], np.broadcast_to(want[1], (63,)))
    with pytest.raises(ValueError, match="no frame selected"):
        corpus.minmax("y", none)


# ---- the operator itself: guarded buffers ------------------------------------------------------------------------------------------------
def _guarded(n, dtype):
    buf = torch.full((n + 2 * GUARD,), SENT, device="cuda", dtype=dtype)
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, n):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + n:] == SENT).all())


def _op(A, Dn, seg, prior=None):
    """gt_op_corpus_stats on A [F][ld] (device) with sentinels around every output and around the workspace:
    (min, max, count, mean, M2) as numpy arrays."""
    F, ld = A.shape
    k = L.CorpusStatsCase()
    k.D, k.ld, k.F, k.n_seg = Dn, ld, F, len(seg)
    seg_dev = torch.from_numpy(np.ascontiguousarray(seg, dtype=np.int64).reshape(-1, 2)).cuda() if len(seg) else None
    k.A, k.seg = A.data_ptr(), seg_dev.data_ptr() if seg_dev is not None else None
    if prior is not None:
        pm, pv = torch.from_numpy(prior[0]).cuda(), torch.from_numpy(prior[1]).cuda()
        k.prior_mean, k.prior_var, k.prior_count = pm.data_ptr(), pv.data_ptr(), int(prior[2])
    nbytes = int(L.lib.gt_corpus_stats_workspace_bytes(F, Dn))
    assert nbytes % 8 == 0 and nbytes >= -(-F // S.SLAB) * ld * 32
    ws = _guarded(nbytes // 8, torch.float64)
    outs = [_guarded(Dn, torch.float32), _guarded(Dn, torch.float32)] + [_guarded(Dn, torch.float64) for _ in range(3)]
    k.workspace, k.workspace_bytes = ws[1].data_ptr(), nbytes
    k.out_min, k.out_max, k.out_count, k.out_mean, k.out_m2 = [v.data_ptr() for _, v in outs]
    L.check(L.lib.gt_op_corpus_stats(C.byref(k), L.current_stream()))
    torch.cuda.synchronize()
    assert _intact(ws[0], nbytes // 8), "sentinels around the workspace"
    for (buf, v), name in zip(outs, ("min", "max", "count", "mean", "M2")):
        assert _intact(buf, Dn), "sentinels around %s" % name
    return [v.cpu().numpy() for _, v in outs]


@pytest.mark.parametrize("Dn", [5, 187])
def test_two_runs_are_bit_identical_and_write_nothing_else(Dn):
    X, cut = S.make_corpus("large_offset", S.ROWS[-1], Dn)
    corpus = _corpus(X)
    seg = corpus.segments(cut)
    prior = (np.linspace(-1.0, 1.0, Dn), np.linspace(0.5, 2.0, Dn), 1234)
    for pr in (None, prior):
        a, b = _op(corpus.X_all, Dn, seg, pr), _op(corpus.X_all, Dn, seg, pr)
        for u, v in zip(a, b):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    assert a[2][0] == sum(cut) + 1234 and (a[2] == a[2][0]).all()
    # the same through the corpus' own workspace
    m1, m2 = corpus.meanvar("x", cut), corpus.meanvar("x", cut)
    assert np.array_equal(m1[0].view(np.uint8), m2[0].view(np.uint8)) and np.array_equal(m1[1].view(np.uint8), m2[1].view(np.uint8))


def test_segments_outside_the_corpus_and_of_no_rows_count_nothing():
    Dn, F = 5, S.SLAB + 44
    X, _ = S.make_corpus("five", F, Dn)
    corpus = _corpus(X)
    seg = [(-3, 5), (2, 0), (4, 6), (10, 0), (200, 90), (F - 2, 5), (F, 0), (F + 7, 1)]
    lo, hi, count, mean, m2 = _op(corpus.X_all, Dn, seg)
    rows = np.concatenate(X)
    want = [rows[4:10], rows[200:290]]
    ref = S.reference(want)
    assert (count == 96).all() and S.mismatches(mean, m2 / 96.0, 96, ref, Dn) == [] and S.minmax_mismatches(lo, hi, want) == []
    lo, hi, count, mean, m2 = _op(corpus.X_all, Dn, [])
    assert not count.any() and not mean.any() and not m2.any() and (lo == np.inf).all() and (hi == -np.inf).all()
    lo, hi, count, mean, m2 = _op(corpus.X_all, Dn, [(0, F + 1)])
    assert not count.any()


def test_a_malformed_case_is_refused_before_any_launch():
    A = torch.zeros(8, 8, device="cuda")
    k = L.CorpusStatsCase()
    k.D, k.ld, k.F = 7, 7, 8
    k.A = A.data_ptr()
    assert L.lib.gt_op_corpus_stats(C.byref(k), None) == L.GT_ERR_INVALID and b"pitch" in L.lib.gt_last_error()
    k.ld = 8
    assert L.lib.gt_op_corpus_stats(C.byref(k), None) == L.GT_ERR_INVALID and b"null result" in L.lib.gt_last_error()
    out = torch.zeros(5, 8, device="cuda", dtype=torch.float64)
    k.out_min, k.out_max, k.out_count, k.out_mean, k.out_m2 = [out[i].data_ptr() for i in range(5)]
    assert L.lib.gt_op_corpus_stats(C.byref(k), None) == L.GT_ERR_INVALID and b"workspace" in L.lib.gt_last_error()
    assert L.lib.gt_corpus_stats_workspace_bytes(8, 7) == 8 * 32 and L.lib.gt_corpus_stats_workspace_bytes(S.SLAB + 1, 187) == 2 * 188 * 32


# ---- loaders from raw arrays -------------------------------------------------------------------------------------------------------------
TRAIN_LENGTHS, TEST_LENGTHS = [37, 12, 5, 40, 64, 3, 29, 3, 40, 9, 17, 22], [30, 9, 30]
TRAIN_BATCHES = {"train": [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]], "test": [[2, 0], [1]]}
FIRST_DRAW = {"train": 0, "test": 1 << 31}


def _raw_arrays(kind, seed=5):
    widths = R.SMALL if kind == "tts" else R.VC
    rs = np.random.RandomState(seed)
    X = {ph: [(rs.randn(n, widths["Dx"]) * 3.0 + 1.0).astype(np.float32) for n in lens] for ph, lens in (("train", TRAIN_LENGTHS), ("test", TEST_LENGTHS))}
    Y = {ph: [(rs.randn(n, widths["Dy"]) * 2.0 - 0.5).astype(np.float32) for n in lens] for ph, lens in (("train", TRAIN_LENGTHS), ("test", TEST_LENGTHS))}
    return widths, X, Y


def _loader_hp(kind, recompute=False, nz=5):
    from gantts_amd import hparams
    widths = R.SMALL if kind == "tts" else R.VC
    hp = types.SimpleNamespace(**(hparams.tts_acoustic if kind == "tts" else hparams.vc).values())
    hp.stream_sizes, hp.has_dynamic_features, hp.windows = list(widths["stream_sizes"]), list(widths["has_dynamic_features"]), R.WINDOWS
    hp.nepoch, hp.lr_decay_schedule, hp.lr_decay_epoch = 1, False, 10
    hp.generator_add_noise, hp.generator_noise_dim, hp.generator_noise_seed = nz > 0, nz, 99
    hp.optimizer_g_params, hp.optimizer_d_params = dict(lr=0.01, weight_decay=1e-7), dict(lr=0.01, weight_decay=1e-7)
    hp.recompute_delta_features, hp.batch_size, hp.num_workers, hp.pin_memory, hp.resident_corpus = recompute, 4, 0, False, False
    if kind == "tts":
        hp.adversarial_streams, hp.mask_nth_mgc_for_adv_loss, hp.discriminator_linguistic_condition = [True, False, False, False], 0, True
    else:
        hp.adversarial_streams, hp.mask_nth_mgc_for_adv_loss, hp.discriminator_linguistic_condition, hp.order = [True], 0, False, 3
    return hp


def _make_loaders(kind, hp):
    """(resident loaders, stats, host loaders, X, Y): the host pipeline of get_*_data_loaders (resident_corpus off) fed the returned
    statistics; both on the index batches TRAIN_BATCHES."""
    _, X, Y = _raw_arrays(kind)
    if kind == "tts":
        loaders, stats = D.resident_tts_loaders(X, Y, hp)
        host = D.get_tts_data_loaders(X, Y, stats["X_data_min"], stats["X_data_max"], stats["Y_data_mean"], np.sqrt(stats["Y_data_var"]), hp)
    else:
        loaders, stats = D.resident_vc_loaders(X, Y, hp)
        host = D.get_vc_data_loaders(X, Y, stats["data_mean"], np.sqrt(stats["data_var"]), hp)
    for ph in loaders:
        loaders[ph].batch_sampler = TRAIN_BATCHES[ph]
    return loaders, stats, host, X, Y


def _device_batches(loader):
    key1, out = loader.draws, []
    Dx, nz = loader.corpus.Dx, loader.nz
    for b in loader:
        gi = b.generator_input.cpu().numpy()
        out.append(dict(x=np.ascontiguousarray(gi[:, :, :Dx]), y=b.y.cpu().numpy(), y_static=b.y_static.cpu().numpy(), mask=b.mask.cpu().numpy(),
                        lengths=b.lengths.cpu().numpy(), z=np.ascontiguousarray(gi[:, :, Dx:Dx + nz]) if nz else None))
    return key1, out


@pytest.mark.parametrize("kind,recompute", [("tts", False), ("tts", True), ("vc", False)])
def test_loaders_from_raw_arrays(kind, recompute, monkeypatch):
    hp = _loader_hp(kind, recompute)
    uploads, real = [], D.ResidentCorpus.upload

    def counting(self, device="cuda"):      # every call that finds the corpus not yet on the device
        if self.X_all is None:
            uploads.append(self)
        return real(self, device)
    monkeypatch.setattr(D.ResidentCorpus, "upload", counting)
    loaders, stats, host, X, Y = _make_loaders(kind, hp)
    assert len(uploads) == 2 and isinstance(host["train"], torch.utils.data.DataLoader)
    Dx, Dy = loaders["train"].corpus.Dx, loaders["train"].corpus.Dy
    # the statistics: those of the TRAIN phase, inside the bound; min / max equal the host's
    if kind == "tts":
        assert sorted(stats) == ["X_data_max", "X_data_min", "Y_data_mean", "Y_data_var"]
        lo, hi = D.minmax(X["train"])
        assert np.array_equal(stats["X_data_min"], lo) and np.array_equal(stats["X_data_max"], hi) and stats["X_data_min"].dtype == np.float32
        assert S.mismatches(stats["Y_data_mean"], stats["Y_data_var"], None, S.reference(Y["train"]), Dy) == []
        hm, hv = D.meanvar(Y["train"])
        ds = loaders["train"].dataset
        assert isinstance(ds, D.TTSDataset) and ds.Y_data_mean is stats["Y_data_mean"] and np.array_equal(ds.Y_data_std, np.sqrt(stats["Y_data_var"]))
    else:
        assert sorted(stats) == ["data_mean", "data_var"]
        assert S.mismatches(stats["data_mean"], stats["data_var"], None, S.reference(X["train"] + Y["train"]), Dy) == []
        n = np.array([len(x) for x in X["train"]])
        hm, hv, c = D.meanvar(X["train"], n, return_last_sample_count=True)
        hm, hv = D.meanvar(Y["train"], n, mean_=hm, var_=hv, last_sample_count=c)
        ds = loaders["train"].dataset
        assert isinstance(ds, D.VCDataset) and ds.data_mean is stats["data_mean"]
    mean, var = (stats["Y_data_mean"], stats["Y_data_var"]) if kind == "tts" else (stats["data_mean"], stats["data_var"])
    assert np.allclose(mean, hm, rtol=1e-12, atol=1e-13) and np.allclose(var, hv, rtol=1e-12, atol=1e-13)
    assert loaders["test"].draws == 1 << 31 and loaders["train"].draws == 0 and loaders["test"].dataset is not loaders["train"].dataset
    # the batches: the host pipeline's, fed the same statistics
    for ph in ("train", "test"):
        key1, got = _device_batches(loaders[ph])
        assert key1 == FIRST_DRAW[ph]
        ref = R.reference_batches(host[ph].dataset, hp, TRAIN_BATCHES[ph], key1=key1)
        assert len(got) == len(ref)
        for k, (g, r) in enumerate(zip(got, ref)):
            if recompute:
                assert R.delta_mismatches(g, r, host[ph].dataset, hp) == [], "%s batch %d" % (ph, k)
            else:
                assert R.mismatches(g, r) == [], "%s batch %d" % (ph, k)
        if not recompute:      # and DevicePrefetcher over the host loader's own dataset and collate
            staged = D.DevicePrefetcher([host[ph].collate_fn([host[ph].dataset[i] for i in idx]) for idx in TRAIN_BATCHES[ph]])
            for b, g in zip(staged, got):
                assert np.array_equal(b.x.cpu().numpy(), g["x"]) and np.array_equal(b.y.cpu().numpy(), g["y"]) and b.cpu_lengths == g["lengths"].tolist()
        _device_batches(loaders[ph])      # a second epoch
    assert len(uploads) == 2      # one upload per phase


def test_a_raw_corpus_needs_statistics_before_it_feeds_a_loader():
    _, X, Y = _raw_arrays("tts")
    hp = _loader_hp("tts")
    corpus = D.ResidentCorpus.from_arrays(X["train"], Y["train"])
    assert corpus.X_all is not None and corpus.dataset is None and corpus.stats is None
    with pytest.raises(ValueError, match="no statistics attached"):
        D.ResidentLoader(corpus, 4, False, hp)
    lo, hi = corpus.minmax("x")
    mean, var = corpus.meanvar("y")
    corpus.attach_statistics(D.TTSDataset(X["train"], Y["train"], lo, hi, mean, np.sqrt(var), hp=hp))
    assert len(list(D.ResidentLoader(corpus, 4, False, hp))) == 3


def _train_loop_run(kind, resident, monkeypatch):
    import gantts_amd.train as T
    from gantts_amd import multistream, optim, seqloss
    from hip_runner import build_model
    hp = _loader_hp(kind)
    nz = hp.generator_noise_dim if hp.generator_add_noise else 0
    loaders, stats, host, X, Y = _make_loaders(kind, hp)
    Dx, Dy = loaders["train"].corpus.Dx, loaders["train"].corpus.Dy
    Ds = len(loaders["train"].scol_host)
    g = dict(kind="MLP", in_dim=Dx + nz, out_dim=Dy, num_hidden=2, hidden_dim=16, dropout=0.0, last_sigmoid=False)
    d = dict(kind="MLP", in_dim=(Dx + 2) if kind == "tts" else Ds, out_dim=1, num_hidden=2, hidden_dim=128, dropout=0.0, last_sigmoid=True)
    mg, md = build_model(g, 11), build_model(d, 22)
    og, od = optim.Adagrad(mg.parameters(), **hp.optimizer_g_params), optim.Adagrad(md.parameters(), **hp.optimizer_d_params)
    if resident:
        hp.resident_corpus = True

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
        zs, run = [], {}
        for ph in ("train", "test"):      # the host pipeline on the same index batches, in train_loop's order; z from the reference
            ld = Loader(host[ph].collate_fn([host[ph].dataset[i] for i in idx]) for idx in TRAIN_BATCHES[ph])
            ld.dataset = host[ph].dataset
            run[ph] = ld
            if nz:
                zs += [torch.from_numpy(r["z"]) for r in R.reference_batches(host[ph].dataset, hp, TRAIN_BATCHES[ph], key1=FIRST_DRAW[ph])]
        loaders = run

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


@pytest.mark.parametrize("kind", ["tts", "vc"])
def test_train_loop_on_loaders_from_raw_arrays_equals_the_host_pipeline(kind, monkeypatch):
    """One epoch (train and test phase) through resident_*_loaders against the host pipeline of get_*_data_loaders fed the returned
    statistics: the same step on bit-identical inputs, so every logged value and every parameter is equal.  Without recomputed deltas:
    with them the device's batches are inside the float64 bound of the host's, not bit for bit, which
    test_loaders_from_raw_arrays[tts-True] checks batch by batch."""
    ref_logs, ref_params = _train_loop_run(kind, False, monkeypatch)
    got_logs, got_params = _train_loop_run(kind, True, monkeypatch)
    assert [n for n, _ in got_logs] == [n for n, _ in ref_logs] and len(ref_logs) > 10
    for (n, g), (_, r) in zip(got_logs, ref_logs):
        assert g == r or (g != g and r != r), "%s: %r != %r" % (n, g, r)
    assert any("loss" in n and v != 0 for n, v in ref_logs)
    for k in ref_params:
        assert np.array_equal(got_params[k], ref_params[k]), k
