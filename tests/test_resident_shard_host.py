"""Host side of the sharded resident batch path (no GPU): data.shard_plan, the same-epoch guarantee of a sharded ResidentLoader, the
comparator of the GPU test against seeded mistakes in a numpy model of the slot rule (tests/resident_shard_ref.py), the collectives
DataParallelStep.step makes with and without a batch's tv_global, and parallel.resident_epoch's refusal of ranks that planned different epochs."""
import zlib

import numpy as np
import pytest
import torch

import resident_ref as R
import resident_shard_ref as S
from gantts_amd import data as D
from gantts_amd import parallel as P


def _plan(batches=S.BATCHES):
    lens = np.array(S.LENGTHS, dtype=np.int64)
    return D.plan_epoch(np.cumsum(lens) - lens, lens, batches)


# ---- shard_plan -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2, 3, 4])
@pytest.mark.parametrize("batches", [[[0, 1, 2, 3, 4], [5, 6, 7, 8, 9, 10]], [[0, 1, 2, 3, 4, 5, 6], [7, 8, 9, 10]], [list(range(11))]])
def test_shard_plan_deals_whole_sequences_round_robin(world, batches):
    """Batches of 5, 6, 7, 4 and 11 sequences: no multiple of 3, and of 2 and 4 only some."""
    table, plan = _plan(batches)
    shards = [D.shard_plan(plan, r, world) for r in range(world)]
    assert all(len(s) == len(plan) for s in shards)
    for k, (first, B, T, lengths) in enumerate(plan):
        seen = []
        for r in range(world):
            f, B_global, B_local, T_r, local = shards[r][k]
            assert (f, B_global, T_r) == (first, B, T) and T_r == max(lengths)      # the GLOBAL T on every rank
            assert local == lengths[r::world] and B_local == len(local) == -(-(B - r) // world) >= 1
            seen.append(table[first + r:first + B:world, 2].tolist())
        flat = [u for s in seen for u in s]
        assert len(set(flat)) == len(flat) == B                                    # disjoint
        assert sorted(flat) == sorted(batches[k])                                  # their union is the batch


def test_shard_plan_refuses_or_drops_a_batch_shorter_than_the_world():
    _, plan = _plan()                                                              # 5, 5, 1 sequences
    assert [e[2] for e in D.shard_plan(plan, 0, 1)] == [5, 5, 1]
    for rank in range(2):
        with pytest.raises(ValueError, match=r"batch 2 has 1 sequences for a world of 2 ranks"):
            D.shard_plan(plan, rank, 2)
        with pytest.raises(ValueError, match=r"batch 2 has 1 sequences for a world of 2 ranks"):
            D.shard_plan(plan, rank, 2, short_batch="error")
        got = D.shard_plan(plan, rank, 2, short_batch="drop")
        assert [(e[0], e[1]) for e in got] == [(0, 5), (5, 5)] and [e[2] for e in got] == [3 - rank, 3 - rank]
    with pytest.raises(ValueError, match="rank 2 of a world of 2"):
        D.shard_plan(plan, 2, 2)
    with pytest.raises(ValueError, match="rank 0 of a world of 0"):
        D.shard_plan(plan, 0, 0)
    with pytest.raises(ValueError, match="short_batch"):
        D.shard_plan(plan, 0, 2, short_batch="pad")


# ---- every rank plans the same epoch --------------------------------------------------------------------------------------------------
def _loader(rank, world, seed=20240607, **kw):
    ds, hp = S.tts_case()
    hp.generator_noise_seed = seed
    for k, v in kw.items():
        setattr(hp, k, v)
    return D.ResidentLoader(ds, 5, True, hp, rank=rank, world=world, short_batch="drop")


def test_the_ranks_of_a_sharded_loader_plan_identical_epochs():
    torch.manual_seed(1)
    a = _loader(0, 2)
    torch.manual_seed(2)                       # the global generator plays no part
    b = _loader(1, 2)
    assert len(a) == len(b) == 2               # 5, 5 and the dropped batch of 1
    tables = []
    for epoch in range(3):
        torch.manual_seed(10 + epoch)
        ta, pa = a.plan()
        torch.manual_seed(20 + epoch)
        tb, pb = b.plan()
        assert np.array_equal(ta, tb) and pa == pb and sorted(ta[:, 2].tolist()) == list(range(11))
        assert a.last_table_crc == b.last_table_crc == zlib.crc32(ta.tobytes())
        tables.append(ta)
    assert not np.array_equal(tables[0], tables[1]) and not np.array_equal(tables[1], tables[2])
    # the seed: hp.shard_sampler_seed before hp.generator_noise_seed
    assert np.array_equal(_loader(0, 2).plan()[0], tables[0])
    assert np.array_equal(_loader(0, 2, seed=1, shard_sampler_seed=20240607).plan()[0], tables[0])
    assert not np.array_equal(_loader(0, 2, seed=1).plan()[0], tables[0])


def test_world_one_keeps_the_unseeded_sampler():
    one = _loader(0, 1)
    assert one.batch_sampler.sampler.generator is None and _loader(1, 2).batch_sampler.sampler.generator is not None
    assert len(one) == 3
    torch.manual_seed(3)
    t0 = one.plan()[0]
    torch.manual_seed(3)
    t1 = one.plan()[0]
    torch.manual_seed(4)
    t2 = one.plan()[0]
    assert np.array_equal(t0, t1) and not np.array_equal(t0, t2)         # torch's global generator, as before
    assert one.last_table_crc == zlib.crc32(t2.tobytes())


def test_device_batch_gains_tv_global_and_an_explicit_max_len():
    b = D.DeviceBatch("x", "y", "l", [5, 3], None)
    assert b.max_len == 5 and b.tv_global is None
    b = D.DeviceBatch("x", "y", "l", [5, 3], None, tv_global="tv", max_len=9)
    assert b.max_len == 9 and b.tv_global == "tv"


def test_assemble_shard_matches_the_header_layout():
    import ctypes as C
    from gantts_amd import _lib as L
    assert L.AssembleShard.B_global.offset == 8 and L.AssembleShard.tv_global.offset == 16 and C.sizeof(L.AssembleShard) == 24


# ---- the comparator rejects seeded mistakes ------------------------------------------------------------------------------------------
def _model_bad(mistake):
    """Mismatches of the slot model against the host pipeline over world 1 .. 4, every rank, every batch with a sequence for each rank;
    plus the two table edge cases: a caller's T below the longest length and a slot outside the corpus."""
    ds, hp = S.tts_case()
    ref = R.reference_batches(ds, hp, S.BATCHES)
    table, plan = _plan()
    F = int(sum(S.LENGTHS))
    bad = []
    for world in (1, 2, 3, 4):
        for rank in range(world):
            for (first, B, T, _), r in zip(plan, ref):
                if B < world:
                    continue
                bad.append(S.shard_mismatches(S.slot_model(table, first, B, T, F, rank, world, mistake), S.expected_shard(r, rank, world)))
                # T = 20 below the longest length of the batch: the count is cut as the mask is
                bad.append(S.shard_mismatches(S.slot_model(table, first, B, 20, F, rank, world, mistake), S.expected_shard(r, rank, world, T=20)))
    # slot 1 of batch 0 (rank 1's of a world of 2) points outside the corpus: that sequence is empty everywhere
    broken = table.copy()
    broken[1, 0] = F - 2
    exp = S.expected_shard(ref[0], 0, 2)
    exp["tv"] -= int(table[1, 1])
    bad.append(S.shard_mismatches(S.slot_model(broken, 0, 5, 37, F, 0, 2, mistake), exp))
    return bad


def test_the_slot_model_equals_the_host_pipeline():
    bad = _model_bad(None)
    assert len(bad) > 30 and not any(bad)


@pytest.mark.parametrize("mistake", S.MISTAKES)
def test_the_comparator_rejects_a_seeded_shard_mistake(mistake):
    bad = _model_bad(mistake)
    assert any(bad), "the comparator accepts '%s'" % mistake
    expect = {"contiguous_blocks": "order", "rank_and_world_exchanged": "order", "local_T": "T"}.get(mistake, "tv")
    assert any(expect in b for b in bad)


# ---- DataParallelStep.step: the collectives of one step -----------------------------------------------------------------------------
class _FakeBackend(object):
    """The backend protocol with trivial arithmetic: the results show the normaliser the step was given."""

    def __init__(self):
        self.tv, self.g, self.s = None, torch.zeros(3), torch.zeros(2, dtype=torch.float64)

    def mask_of(self, batch):
        return batch["mask"]

    def set_loss_normalizer(self, tv):
        self.tv = float(tv)

    def zero_grad(self):
        self.g.zero_()

    def apply_generator(self, batch):
        pass

    def flat_grads(self, which):
        return self.g

    def scalar_sums(self, which):
        return self.s

    def update_discriminator_begin(self, batch, phase):
        self.s[:] = torch.tensor([3.0, 5.0], dtype=torch.float64)

    def update_discriminator_end(self, batch, phase):
        return float(self.s[0]) / self.tv, float(self.s[1]) / self.tv

    def update_generator_begin(self, batch, adv_w, mse_w, mge_w, phase):
        self.s[:] = torch.tensor([7.0, 11.0], dtype=torch.float64)

    def update_generator_end(self, batch, adv_w, mse_w, mge_w, phase):
        return float(self.s[0]) / self.tv, float(self.s[1]) / self.tv


def _counted_step(batch):
    dp = P.DataParallelStep(_FakeBackend(), always_reduce=True)
    calls = []
    dp._allreduce = lambda *tensors: calls.append(len(tensors))
    return dp.step(batch), calls


def test_a_batch_that_carries_tv_global_saves_the_count_collective():
    mask = torch.zeros(2, 6, 1)
    mask[0, :5], mask[1, :2] = 1, 1
    without, calls = _counted_step(dict(mask=mask))
    assert calls == [1, 2, 2]                                  # Tv, then gradient + sums of D and of G
    with_tv, calls = _counted_step(dict(mask=mask, tv_global=torch.tensor([7.0], dtype=torch.float64)))
    assert calls == [2, 2]
    assert with_tv == without and without[0] == (3.0 / 7.0, 5.0 / 7.0)
    explicit, calls = _counted_step(dict(mask=mask, tv_global=None))
    assert calls == [1, 2, 2] and explicit == without


# ---- resident_epoch: the ranks must have planned the same epoch -----------------------------------------------------------------------
class _PlanOnlyLoader(D.ResidentLoader):
    def begin_epoch(self):          # no device: the plan and its crc only, no batch
        self.plan()
        return None, []


def test_resident_epoch_refuses_ranks_that_planned_different_epochs():
    ds, hp = S.tts_case()
    loader = _PlanOnlyLoader(ds, 5, True, hp, rank=0, world=2, short_batch="drop")
    other = _loader(1, 2)
    seen = []

    def peer(crc_of_peer):
        def all_reduce_max(t):
            seen.append(t.clone())
            return torch.maximum(t, torch.tensor([crc_of_peer(), -crc_of_peer()], dtype=torch.int64))
        return all_reduce_max

    def same():
        other.plan()
        return other.last_table_crc
    assert P.resident_epoch(None, loader, all_reduce_max=peer(same)) == []
    assert seen[0].tolist() == [loader.last_table_crc, -loader.last_table_crc] and seen[0].dtype == torch.int64
    for delta in (1, -1):           # a peer whose crc is larger, and one whose crc is smaller
        other.plan()
        with pytest.raises(RuntimeError, match="the ranks planned different epochs"):
            P.resident_epoch(None, loader, all_reduce_max=peer(lambda: loader.last_table_crc + delta))
