"""gt_op_assemble_shard and a sharded gantts_amd.data.ResidentLoader on the device against the host pipeline on the WHOLE batch
(tests/resident_ref.py: reference_batches; tests/resident_shard_ref.py): every rank of world 1 .. 4 holds, bit for bit, the rows rank::world of
the whole batch padded to the global T -- noise columns included --, tv_global is the whole batch's valid-frame count exactly; world 1 through
the shard entry equals gt_op_assemble_batch byte for byte; table edge cases; refusals; two emulated ranks fed by sharded loaders against
one engine on the whole batch; DataParallelStep with and without the batch's tv_global.

Parity rule of the end-to-end comparison (the suite's float32 rule, restated): |got - ref| <= 1e-6 + 1e-4 * max|ref| per tensor; counts
exact; replicas bit-identical."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import resident_ref as R
import resident_shard_ref as S
from gantts_amd import _lib as L
from gantts_amd import data as D

pytestmark = pytest.mark.gpu

SENT = 1.2345e30
GUARD = 64
NAMES = ("gi", "y", "y_static", "mask", "lengths", "tv_global")
RTOL, ATOL = 1e-4, 1e-6


def _guarded(shape, dtype=torch.float32, fill=float("nan")):
    """A buffer of NaN (-77 for integers) between two guards of sentinels: (whole buffer, the view to write)."""
    n = int(np.prod(shape))
    integer = dtype == torch.int64
    buf = torch.full((n + 2 * GUARD,), -99 if integer else SENT, device="cuda", dtype=dtype)
    buf[GUARD:GUARD + n] = -77 if integer else fill
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _intact(buf, n):
    v = -99 if buf.dtype == torch.int64 else SENT
    return bool((buf[:GUARD] == v).all()) and bool((buf[GUARD + n:] == v).all())


def _buffers(loader, B, T, fill=float("nan")):
    c = loader.corpus
    ld = (c.Dx + loader.nz + 3) // 4 * 4
    shapes = ((B, T, ld), (B, T, c.Dy), (B, T, len(loader.scol_host)), (B, T, 1), (B,), (1,))
    dtypes = (torch.float32,) * 4 + (torch.int64, torch.float64)
    return [_guarded(s, d, fill) for s, d in zip(shapes, dtypes)]


def _read(loader, pairs, sharded=True):
    """The written buffers as the dict resident_ref compares, after the checks every launch has to pass: sentinels intact, every element
    written, pad columns 0."""
    torch.cuda.synchronize()
    c, nz = loader.corpus, loader.nz
    for (buf, v), name in zip(pairs, NAMES):
        assert _intact(buf, v.numel()), "sentinels around %s" % name
    gi, y, ys, mask, lengths, tv = [v.cpu().numpy() for _, v in pairs]
    for a, name in zip((gi, y, ys, mask), NAMES):
        assert not np.isnan(a).any(), "%s has unwritten elements" % name
    assert (lengths >= 0).all() and (not sharded or not np.isnan(tv).any())
    assert not gi[:, :, c.Dx + nz:].any(), "pad columns of gi"
    return dict(x=np.ascontiguousarray(gi[:, :, :c.Dx]), y=y, y_static=ys, mask=mask, lengths=lengths,
                z=np.ascontiguousarray(gi[:, :, c.Dx:c.Dx + nz]) if nz else None, tv=float(tv[0]))


def _run_rank(corpus, hp, batches, rank, world, key1=0, short_batch="drop"):
    loader = D.ResidentLoader(corpus, 1, False, hp, batch_sampler=batches, first_draw=key1, rank=rank, world=world, short_batch=short_batch)
    case, plan = loader.begin_epoch()
    out = []
    for entry in plan:
        if world == 1:
            first, B, T, cpu_lengths = entry
            pairs = _buffers(loader, B, T)
            loader.assemble(case, first, B, T, out=tuple(v for _, v in pairs[:5]))
        else:
            first, B_global, B, T, cpu_lengths = entry
            pairs = _buffers(loader, B, T)
            loader.assemble(case, first, B, T, out=tuple(v for _, v in pairs[:5]), B_global=B_global, tv_global=pairs[5][1])
        got = _read(loader, pairs, sharded=world > 1)
        assert got["lengths"].tolist() == cpu_lengths
        got["T"] = T
        out.append(got)
    return out


CASES = {"tts": S.tts_case, "vc": S.vc_case, "tts_delta": lambda: S.tts_case(recompute=True)}
_shared = {}


def _case(name):
    """(dataset, hp, uploaded corpus, host reference of the whole batches): made once per case and left unchanged."""
    if name not in _shared:
        ds, hp = CASES[name]()
        _shared[name] = (ds, hp, D.ResidentCorpus(ds), R.reference_batches(ds, hp, S.BATCHES, key1=3))
    return _shared[name]


@pytest.mark.parametrize("world", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["tts", "vc", "tts_delta"])
def test_every_rank_holds_its_rows_of_the_whole_batch_bit_for_bit(name, world):
    """tts: float32 min-max on x, float64 mean / variance on y, 5 noise columns; vc: one mean / variance for both sides (a VCDataset has
    equal widths: 10 / 10), no noise; tts_delta: recomputed deltas, whose y the suite judges by resident_ref.delta_mismatches (the
    float64 bound; window 0 and the plain stream bit for bit) -- the host's float64 sum is ordered differently."""
    ds, hp, corpus, ref = _case(name)
    kept = [r for r in ref if len(r["order"]) >= world]
    assert len(kept) == (3 if world == 1 else 2)                       # short_batch="drop": the one-sequence batch is left out
    tvs = []
    for rank in range(world):
        got = _run_rank(corpus, hp, S.BATCHES, rank, world, key1=3)
        assert len(got) == len(kept)
        for k, (g, r) in enumerate(zip(got, kept)):
            exp = S.expected_shard(r, rank, world)
            assert g["T"] == exp["T"] and g["x"].shape[:2] == (len(exp["order"]), r["T"])
            bad = R.delta_mismatches(g, exp, ds, hp) if name == "tts_delta" else R.mismatches(g, exp, S.KEYS)
            assert bad == [], "world %d rank %d batch %d" % (world, rank, k)
            if world > 1:
                assert g["tv"] == float(exp["tv"]) == float(r["lengths"].sum())
        tvs.append([g["tv"] for g in got])
    assert all(t == tvs[0] for t in tvs)                                # the same on every rank
    if world > 1:
        with pytest.raises(ValueError, match="batch 2 has 1 sequences for a world of %d ranks" % world):
            _run_rank(corpus, hp, S.BATCHES, 0, world, short_batch="error")


def _shard(rank, world, B_global, tv):
    s = L.AssembleShard()
    s.rank, s.world, s.B_global, s.tv_global = rank, world, B_global, tv
    return s


def test_world_one_through_the_shard_entry_equals_assemble_batch_byte_for_byte():
    ds, hp, corpus, ref = _case("tts")
    loader = D.ResidentLoader(corpus, 1, False, hp, batch_sampler=S.BATCHES, first_draw=3)
    case, plan = loader.begin_epoch()
    for (first, B, T, _), r in zip(plan, ref):
        a, b = _buffers(loader, B, T), _buffers(loader, B, T)
        loader.assemble(case, first, B, T, out=tuple(v for _, v in a[:5]))
        case.gi, case.y, case.y_static, case.mask, case.lengths = [v.data_ptr() for _, v in b[:5]]
        L.check(L.lib.gt_op_assemble_shard(C.byref(case), C.byref(_shard(0, 1, B, b[5][1].data_ptr())), L.current_stream()))
        _read(loader, a, sharded=False), _read(loader, b)
        for (buf_a, _), (buf_b, _), name in zip(a[:5], b[:5], NAMES):
            assert torch.equal(buf_a.view(torch.uint8), buf_b.view(torch.uint8)), name
        assert float(b[5][1]) == float(r["lengths"].sum())


def test_table_edge_cases():
    """A slot outside the corpus that belongs to ANOTHER rank changes nothing here and counts 0; a caller's T below the longest length
    cuts the count as it cuts the mask."""
    ds, hp, corpus, ref = _case("tts")
    loader = D.ResidentLoader(corpus, 1, False, hp, batch_sampler=S.BATCHES, first_draw=3, rank=0, world=2, short_batch="drop")
    case, plan = loader.begin_epoch()
    first, B_global, B, T, _ = plan[0]
    table_host, _ = D.plan_epoch(corpus.offsets, corpus.lengths, S.BATCHES)

    def run(T_call=T, rank=0):
        loader.rank = rank
        n = len(range(rank, B_global, 2))
        pairs = _buffers(loader, n, T_call)
        loader.assemble(case, first, n, T_call, out=tuple(v for _, v in pairs[:5]), B_global=B_global, tv_global=pairs[5][1])
        return _read(loader, pairs), pairs

    good, good_pairs = run()
    assert R.mismatches(good, S.expected_shard(ref[0], 0, 2), S.KEYS) == []
    broken = table_host.copy()
    broken[first + 1, 0] = corpus.F - 2                  # slot 1 is rank 1's: 37 frames from the corpus' last but one
    table = torch.from_numpy(broken).cuda()
    case.table = table.data_ptr()
    got, pairs = run()
    for (buf_a, _), (buf_b, _), name in zip(good_pairs[:5], pairs[:5], NAMES):
        assert torch.equal(buf_a.view(torch.uint8), buf_b.view(torch.uint8)), name
    assert got["tv"] == good["tv"] - float(table_host[first + 1, 1]) and good["tv"] == float(ref[0]["lengths"].sum())
    other, _ = run(rank=1)                               # the rank that holds it: an empty sequence, the same count
    assert other["lengths"].tolist() == [0] + ref[0]["lengths"][3::2].tolist() and other["tv"] == got["tv"]
    assert not other["mask"][0].any() and not other["x"][0].any() and not other["y"][0].any()
    case.table = case._table.data_ptr()
    for rank in range(2):                                # T = 20 below the longest length, 37
        cut, _ = run(T_call=20, rank=rank)
        exp = S.expected_shard(ref[0], rank, 2, T=20)
        assert R.mismatches(cut, exp, S.KEYS) == []
        assert cut["tv"] == float(exp["tv"]) == float(np.minimum(ref[0]["lengths"], 20).sum()) < good["tv"]


def test_every_refusal_leaves_the_outputs_untouched():
    ds, hp, corpus, ref = _case("tts")
    loader = D.ResidentLoader(corpus, 1, False, hp, batch_sampler=S.BATCHES, first_draw=3, rank=1, world=2, short_batch="drop")
    case, plan = loader.begin_epoch()
    first, B_global, B, T, _ = plan[1]                   # slots 5 .. 9 of 11; rank 1 holds 2 of the 5 sequences
    assert (first, B_global, B, int(case.n_slots)) == (5, 5, 2, 11)
    loader.assemble(case, first, B, T, B_global=B_global)             # fills the case
    pairs = _buffers(loader, B, T, fill=SENT)
    case.gi, case.y, case.y_static, case.mask, case.lengths = [v.data_ptr() for _, v in pairs[:5]]
    tv = pairs[5][1].data_ptr()
    stream = L.current_stream()

    def refused(shard, message, **fields):
        saved = {k: getattr(case, k) for k in fields}
        for k, v in fields.items():
            setattr(case, k, v)
        rc = L.lib.gt_op_assemble_shard(C.byref(case), None if shard is None else C.byref(shard), stream)
        for k, v in saved.items():
            setattr(case, k, v)
        assert rc == L.GT_ERR_INVALID and message in L.lib.gt_last_error().decode(), (message, L.lib.gt_last_error())

    refused(None, "null shard")
    refused(_shard(0, 0, 5, tv), "rank 0 of a world of 0")
    refused(_shard(-1, 2, 5, tv), "rank -1 of a world of 2")
    refused(_shard(2, 2, 5, tv), "rank 2 of a world of 2")
    refused(_shard(1, 2, 0, tv), "B_global = 0")
    refused(_shard(1, 2, 5, tv), "slots [7, 12) of a table of 11", first_slot=7)
    refused(_shard(1, 2, 5, tv), "holds 2 of 5 sequences, the case has B = 3", B=3)
    refused(_shard(1, 2, 5, tv), "holds 2 of 5 sequences, the case has B = 1", B=1)
    refused(_shard(3, 4, 3, tv), "holds 0 of 3 sequences", B=1)      # a share of 0
    refused(_shard(1, 2, 5, tv + 4), "8-byte aligned")
    refused(_shard(1, 2, 5, tv), "16-byte pitch", ldX=7)             # what gt_op_assemble_batch checks, by the same code
    refused(_shard(1, 2, 5, tv), "bad sizes", T=0)
    torch.cuda.synchronize()
    for (buf, _), name in zip(pairs, NAMES):
        untouched = ((buf == -99) | (buf == -77)) if name == "lengths" else (buf == SENT)
        assert bool(untouched.all()), name
    L.check(L.lib.gt_op_assemble_shard(C.byref(case), C.byref(_shard(1, 2, 5, tv)), stream))      # and the case itself was sound
    assert float(pairs[5][1]) == float(ref[1]["lengths"].sum())


# ---- end to end: two emulated ranks on sharded loaders against one engine on the whole batch ---------------------------------------
E2E_LENGTHS = [17, 30, 4, 22, 9, 11]          # sorted 30 22 17 11 9 4: rank 1 of 2 holds 22, 11, 4 -- its longest is shorter than T = 30
G_MLP = dict(kind="MLP", in_dim=6 + S.NZ, out_dim=10, num_hidden=2, hidden_dim=16, dropout=0.0, last_sigmoid=False)
G_LSTM = dict(kind="LSTMRNN", in_dim=6 + S.NZ, out_dim=10, num_hidden=1, hidden_dim=8, bidirectional=False, dropout=0.0, last_sigmoid=False)
D_MLP = dict(kind="MLP", in_dim=6 + 3, out_dim=1, num_hidden=2, hidden_dim=128, dropout=0.0, last_sigmoid=True)
WEIGHTS = dict(adv_w=1.0, mse_w=0.0, mge_w=1.0)


def _e2e_hp():
    from gantts_amd import hparams
    hp = types.SimpleNamespace(**hparams.tts_acoustic.values())
    hp.stream_sizes, hp.has_dynamic_features, hp.windows = S.WIDTHS["stream_sizes"], S.WIDTHS["has_dynamic_features"], R.WINDOWS
    hp.adversarial_streams, hp.mask_nth_mgc_for_adv_loss, hp.discriminator_linguistic_condition = [True, False], 0, True
    hp.generator_add_noise, hp.generator_noise_dim, hp.generator_noise_seed, hp.recompute_delta_features = True, S.NZ, 99, False
    return hp


def _backend(hp, g_spec):
    """An emulated rank: its own replicas, optimizers and engine.  SGD: the update is linear in the gradient, so the float32 parity rule
    carries over to the parameters (the first Adagrad step, lr * sign(g), is discontinuous at g = 0)."""
    import gantts_amd.train as T
    from gantts_amd import optim
    from gantts_amd.engine import HipStepBackend
    from hip_runner import build_model

    class Backend(HipStepBackend):
        def apply_generator(self, batch):      # through train.apply_generator: its refusal of a batch padded beyond its longest sequence
            self._out = T.apply_generator(self.mg, batch["g_in"], batch["R"], batch["lengths"])
            return self._out
    mg, md = build_model(g_spec, 11).eval(), build_model(D_MLP, 22).eval()
    return Backend(hp, mg, md, optim.SGD(mg.parameters(), lr=0.05), optim.SGD(md.parameters(), lr=0.05))


def _close(got, ref, msg):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, msg
    if ref.size:
        lim = ATOL + RTOL * float(np.abs(ref).max())
        assert float(np.abs(got - ref).max()) <= lim, "%s: %.3e > %.3e" % (msg, float(np.abs(got - ref).max()), lim)


@pytest.mark.parametrize("g_spec", [G_MLP, G_LSTM], ids=["mlp", "lstm"])
def test_two_sharded_ranks_equal_one_engine_on_the_whole_batch(g_spec):
    import gantts_amd.train as T
    from gantts_amd.parallel import DataParallelStep, step_batch
    hp = _e2e_hp()
    ds = R.make_dataset("tts", S.WIDTHS, np.float64, lengths=E2E_LENGTHS, hp=hp)
    corpus, batches, steps = D.ResidentCorpus(ds), [list(range(6))], 2
    saved = T.hp
    T.hp = hp
    try:
        # one engine on the whole ResidentLoader batch (the draw counter advances per epoch: step k sees epoch k's noise everywhere)
        be = _backend(hp, g_spec)
        dp, loader = DataParallelStep(be), D.ResidentLoader(corpus, 6, False, hp, batch_sampler=batches)
        whole = []
        for _ in range(steps):
            (batch,) = list(loader)
            assert batch.tv_global is None and batch.max_len == 30
            d, g = dp.step(step_batch(batch, hp), **WEIGHTS)
            whole.append((tuple(d), tuple(g)))
        torch.cuda.synchronize()
        # two emulated ranks, the exchange by hand
        ranks = [_backend(hp, g_spec) for _ in range(2)]
        loaders = [D.ResidentLoader(corpus, 6, False, hp, batch_sampler=batches, rank=r, world=2) for r in range(2)]
        for r, rb in enumerate(ranks):
            rb.set_shard(r, 2)
        hist = []
        for _ in range(steps):
            bs = []
            for r, (rb, ld) in enumerate(zip(ranks, loaders)):
                (batch,) = list(ld)
                assert batch.max_len == 30 and batch.cpu_lengths == sorted(E2E_LENGTHS, reverse=True)[r::2] and batch.x.size(1) == 30
                assert batch.tv_global.dtype == torch.float64 and batch.tv_global.is_cuda and float(batch.tv_global) == float(sum(E2E_LENGTHS))
                b = step_batch(batch, hp)
                assert b["R"].T == 30 and b["tv_global"] is batch.tv_global
                bs.append(b)
                rb.set_loss_normalizer(batch.tv_global)          # the device tensor the launch wrote
                rb.zero_grad()
                rb.apply_generator(b)
                rb.update_discriminator_begin(b, "train")
            for which in ("D", "G"):
                if which == "G":
                    for rb, b in zip(ranks, bs):
                        rb.update_generator_begin(b, WEIGHTS["adv_w"], WEIGHTS["mse_w"], WEIGHTS["mge_w"], "train")
                g = sum(rb.flat_grads(which) for rb in ranks)
                s = sum(rb.scalar_sums(which) for rb in ranks)
                for rb in ranks:
                    rb.flat_grads(which).copy_(g)
                    rb.scalar_sums(which).copy_(s)
                if which == "D":
                    d = [tuple(rb.update_discriminator_end(b, "train")) for rb, b in zip(ranks, bs)]
                else:
                    gr = [tuple(rb.update_generator_end(b, WEIGHTS["adv_w"], WEIGHTS["mse_w"], WEIGHTS["mge_w"], "train")) for rb, b in zip(ranks, bs)]
            assert d[0] == d[1] and gr[0] == gr[1]
            hist.append((d[0], gr[0]))
        for i, ((d, g), (wd, wg)) in enumerate(zip(hist, whole)):
            _close(d, wd, "D scalars of step %d" % i)
            _close(g, wg, "G scalars of step %d" % i)
            assert d[3] == wd[3] and d[4] == wd[4]                   # the correct-counts are exact
        fresh = _backend(hp, g_spec)
        for tag in ("mg", "md"):
            m0, m1, mw = getattr(ranks[0], tag), getattr(ranks[1], tag), getattr(be, tag)
            for (k, v0), v1, vw, vf in zip(m0.state_dict().items(), m1.state_dict().values(), mw.state_dict().values(),
                                           getattr(fresh, tag).state_dict().values()):
                assert torch.equal(v0, v1), k                         # replicas bit-identical
                _close(v0.cpu().numpy(), vw.cpu().numpy(), "%s.%s" % (tag, k))
                assert not torch.equal(vw, vf), k                     # (the steps did run)
    finally:
        T.hp = saved


def test_apply_generator_refuses_the_short_shard_without_set_shard():
    """The carve-out the LSTM end-to-end case goes through is the engine's _dp_world: 1 on a fresh engine, so the same call is refused."""
    import gantts_amd.train as T
    from gantts_amd.parallel import step_batch
    hp = _e2e_hp()
    ds = R.make_dataset("tts", S.WIDTHS, np.float64, lengths=E2E_LENGTHS, hp=hp)
    saved = T.hp
    T.hp = hp
    try:
        be = _backend(hp, G_LSTM)
        assert be.engine._dp_world == 1
        (batch,) = list(D.ResidentLoader(ds, 6, False, hp, batch_sampler=[list(range(6))], rank=1, world=2))
        with pytest.raises(ValueError, match="longest sequence has 22 frames in a batch padded to 30"):
            be.apply_generator(step_batch(batch, hp))
    finally:
        T.hp = saved


def test_a_step_with_the_batchs_tv_global_equals_the_step_without_it_bit_for_bit():
    """HipStepBackend at world 1, always_reduce=False: tv_global from the shard entry (rank 0 of world 1) against mask.sum() on the device."""
    import gantts_amd.train as T
    from gantts_amd.parallel import DataParallelStep, step_batch
    hp = _e2e_hp()
    ds = R.make_dataset("tts", S.WIDTHS, np.float64, lengths=E2E_LENGTHS, hp=hp)
    corpus = D.ResidentCorpus(ds)
    saved = T.hp
    T.hp = hp
    try:
        runs = []
        for with_tv in (False, True):
            be = _backend(hp, G_MLP)
            dp, loader = DataParallelStep(be, always_reduce=False), D.ResidentLoader(corpus, 6, False, hp, batch_sampler=[list(range(6))])
            res = []
            for _ in range(2):
                case, plan = loader.begin_epoch()
                (batch,) = list(loader.batches(case, plan))
                b = step_batch(batch, hp)
                assert b["tv_global"] is None
                if with_tv:
                    tv = torch.full((1,), float("nan"), device="cuda", dtype=torch.float64)
                    first, B, Tn, _ = plan[0]
                    L.check(L.lib.gt_op_assemble_shard(C.byref(case), C.byref(_shard(0, 1, B, tv.data_ptr())), L.current_stream()))
                    b["tv_global"] = tv
                d, g = dp.step(b, **WEIGHTS)
                res.append((tuple(d), tuple(g)))
            torch.cuda.synchronize()
            runs.append((res, [v.cpu().numpy() for m in (be.mg, be.md) for v in m.state_dict().values()]))
        assert runs[0][0] == runs[1][0]
        for a, b in zip(runs[0][1], runs[1][1]):
            assert np.array_equal(a, b)
        # and parallel.resident_epoch drives the same steps (lazy generator scalars, one epoch per call)
        from gantts_amd.parallel import resident_epoch
        be = _backend(hp, G_MLP)
        dp, loader = DataParallelStep(be), D.ResidentLoader(corpus, 6, False, hp, batch_sampler=[list(range(6))])
        res = [resident_epoch(dp, loader, **WEIGHTS) for _ in range(2)]
        assert [len(r) for r in res] == [1, 1]
        assert [(tuple(d), tuple(g)) for r in res for d, g in r] == runs[0][0]
        for a, v in zip(runs[0][1], [v for m in (be.mg, be.md) for v in m.state_dict().values()]):
            assert np.array_equal(a, v.cpu().numpy())
    finally:
        T.hp = saved
