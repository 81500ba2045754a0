"""Host side of the device-resident batch path (no GPU): the epoch planner of gantts_amd.data.ResidentLoader against the host
pipeline (tests/resident_ref.py), and the comparator of the GPU test against seeded mistakes in a numpy model of the kernel."""
import numpy as np
import pytest
import torch

import resident_ref as R
from gantts_amd import data as D

BATCHES_4 = [[0, 1, 2, 3], [4, 5, 6, 7], [8]]           # batch size 4: a partial last batch


def _loader(batch_size=4, shuffle=False, batch_sampler=None, nz=5, kind="tts", widths=R.SMALL, dtype=np.float64):
    hp = R.make_hp(widths, nz=nz)
    ds = R.make_dataset(kind, widths, dtype, hp=hp)
    return D.ResidentLoader(ds, batch_size, shuffle, hp, batch_sampler=batch_sampler), ds, hp


def _check_plan(loader, ds, hp, batches):
    table, plan = loader.plan()
    ref = R.reference_batches(ds, hp, batches)
    assert len(plan) == len(ref) == len(loader)
    offsets = np.cumsum(R.LENGTHS) - np.array(R.LENGTHS)
    slot = 0
    for (first, B, T, cpu_lengths), r in zip(plan, ref):
        assert first == slot and B == len(r["order"]) and T == r["T"]
        assert cpu_lengths == [int(v) for v in r["lengths"]]
        rows = table[first:first + B]
        assert rows[:, 2].tolist() == r["order"]                          # the order torch.sort gives, ties included
        assert rows[:, 0].tolist() == [int(offsets[u]) for u in r["order"]]
        assert rows[:, 1].tolist() == cpu_lengths
        slot += B
    assert table.shape == (slot, 3) and table.dtype == np.int64


def test_sequential_plan_matches_the_host_pipeline_with_a_partial_last_batch():
    loader, ds, hp = _loader(4)
    assert len(loader) == 3 and loader.dataset is ds
    _check_plan(loader, ds, hp, BATCHES_4)


@pytest.mark.parametrize("bs", [1, 9])
def test_plan_at_batch_sizes_one_and_whole_corpus(bs):
    loader, ds, hp = _loader(bs)
    batches = [list(range(i, min(i + bs, 9))) for i in range(0, 9, bs)]
    assert len(loader) == len(batches)
    _check_plan(loader, ds, hp, batches)


def test_plan_takes_a_caller_supplied_batch_sampler():
    batches = [[8, 1, 3], [5], [2, 7, 0, 6, 4]]          # 8, 1, 3 tie at 120 frames
    loader, ds, hp = _loader(batch_sampler=batches)
    assert len(loader) == 3
    _check_plan(loader, ds, hp, batches)


def test_shuffled_plan_is_a_permutation_in_batches_of_the_batch_size():
    loader, ds, hp = _loader(4, shuffle=True)
    torch.manual_seed(3)
    table, plan = loader.plan()
    assert sorted(table[:, 2].tolist()) == list(range(9)) and [p[1] for p in plan] == [4, 4, 1]
    for first, B, T, cpu_lengths in plan:
        assert cpu_lengths == sorted(cpu_lengths, reverse=True) and T == cpu_lengths[0]


def test_device_batch_keeps_its_constructor_and_gains_three_optional_slots():
    b = D.DeviceBatch("x", "y", "l", [5, 3], None)
    assert b.max_len == 5 and b.generator_input is None and b.y_static is None and b.mask is None
    b = D.DeviceBatch("x", "y", "l", [5, 3], None, generator_input="g", y_static="s", mask="m")
    assert (b.generator_input, b.y_static, b.mask) == ("g", "s", "m")


def test_staging_chunks_pack_the_corpus_back_to_back_on_the_pitch():
    rs = np.random.RandomState(0)
    arrays = [rs.randn(n, 7).astype(np.float32) for n in R.LENGTHS]
    buf, got = torch.full((50, 8), 7.0), []
    buf[:, 7] = 0
    for filled in D._fill_chunks(arrays, buf, 7):
        assert 1 <= filled <= 50
        got.append(buf[:filled].clone().numpy())
    got = np.concatenate(got)
    assert np.array_equal(got[:, :7], np.concatenate(arrays)) and not got[:, 7].any()


def test_resident_corpus_refuses_what_the_kernel_cannot_reproduce():
    hp = R.make_hp(R.SMALL)
    ds = R.make_dataset("tts", R.SMALL, np.float64, hp=hp)
    ds.X = [a.astype(np.float64) for a in ds.X]
    with pytest.raises(TypeError, match="float32"):
        D.ResidentCorpus(ds, device=None)
    ds = R.make_dataset("tts", R.SMALL, np.float64, hp=hp)
    ds.Y_data_std = ds.Y_data_std.astype(np.float32)          # numpy would subtract in float64 and divide in float64 of a float32
    with pytest.raises(TypeError, match="share a dtype"):
        D.ResidentCorpus(ds, device=None)
    hp = R.make_hp(R.SMALL, recompute=True)
    with pytest.raises(ValueError, match="shorter than the longest window"):      # LENGTHS has an utterance of 1 frame
        D.ResidentCorpus(R.make_dataset("tts", R.SMALL, np.float64, hp=hp), device=None)


def test_resident_corpus_takes_each_side_in_its_own_statistics_dtype():
    hp = R.make_hp(R.SMALL)
    ds = R.make_dataset("tts", R.SMALL, np.float64, hp=hp)
    ds.X_data_min, ds.X_data_scale = ds.X_data_min.astype(np.float32), ds.X_data_scale.astype(np.float32)
    c = D.ResidentCorpus(ds, device=None)
    assert c.stats_f64 == 2 and (c.ldX, c.ldY, c.F) == (8, 16, sum(R.LENGTHS))
    assert D.ResidentCorpus(R.make_dataset("vc", R.VC, np.float32), device=None).stats_f64 == 0


def test_hp_resident_corpus_makes_the_loader_functions_return_resident_loaders():
    hp = R.make_hp(R.SMALL, nz=5)
    hp.batch_size, hp.num_workers, hp.pin_memory, hp.cache_size, hp.resident_corpus = 4, 0, False, 100, True
    ds = R.make_dataset("tts", R.SMALL, np.float64)
    X, Y = {"train": ds.X, "test": ds.X[:3]}, {"train": ds.Y, "test": ds.Y[:3]}
    lo, hi = D.minmax(ds.X)
    loaders = D.get_tts_data_loaders(X, Y, lo, hi, ds.Y_data_mean, ds.Y_data_std, hp)
    assert all(isinstance(loaders[p], D.ResidentLoader) for p in ("train", "test"))
    assert len(loaders["train"]) == 3 and len(loaders["test"]) == 1 and loaders["train"].draws != loaders["test"].draws
    hp.resident_corpus = False
    assert not isinstance(D.get_tts_data_loaders(X, Y, lo, hi, ds.Y_data_mean, ds.Y_data_std, hp)["train"], D.ResidentLoader)


# ---- the comparator rejects seeded mistakes ------------------------------------------------------------------------------------
def _case(mistake):
    """(dataset, hp, batches) on which the mistake is visible."""
    if mistake == "minmax_as_one_fma":       # float32 statistics: behind float64 arithmetic the float32 rounding hides the difference
        hp = R.make_hp(R.SMALL, nz=5)
        return R.make_dataset("tts", R.SMALL, np.float32, hp=hp), hp, BATCHES_4
    if mistake == "delta_taps_cross_the_utterance_end":
        hp = R.make_hp(R.SMALL, nz=5, recompute=True)
        return R.make_dataset("tts", R.SMALL, np.float64, lengths=R.LENGTHS_DELTA, hp=hp), hp, BATCHES_4
    hp = R.make_hp(R.SMALL, nz=5)
    return R.make_dataset("tts", R.SMALL, np.float64, hp=hp), hp, BATCHES_4


def _bad(ds, hp, batches, mistake):
    ref = R.reference_batches(ds, hp, batches)
    got = R.kernel_model(ds, hp, batches, mistake=mistake)
    if hp.recompute_delta_features:
        return [R.delta_mismatches(g, r, ds, hp) for g, r in zip(got, ref)]
    return [R.mismatches(g, r) for g, r in zip(got, ref)]


@pytest.mark.parametrize("kind,widths,dtype", [("tts", R.SMALL, np.float64), ("tts", R.SMALL, np.float32), ("vc", R.VC, np.float64),
                                               ("vc", R.VC, np.float32)])
def test_the_kernel_model_equals_the_host_pipeline_bit_for_bit(kind, widths, dtype):
    hp = R.make_hp(widths, nz=5, name="vc" if kind == "vc" else "acoustic")
    ds = R.make_dataset(kind, widths, dtype, hp=hp)
    assert _bad(ds, hp, BATCHES_4, None) == [[], [], []]


def test_the_kernel_model_with_recomputed_deltas_is_inside_the_bound():
    ds, hp, batches = _case("delta_taps_cross_the_utterance_end")
    assert _bad(ds, hp, batches, None) == [[], [], []]


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_the_comparator_rejects_a_seeded_mistake(mistake):
    ds, hp, batches = _case(mistake)
    bad = _bad(ds, hp, batches, mistake)
    assert any(bad), "the comparator accepts '%s'" % mistake
    expect = {"z_on_valid_frames_only": "z", "padded_frames_hold_scale_of_zero": "x", "minmax_as_one_fma": "x",
              "statistics_by_pitched_column": "x", "batch_left_unsorted": "lengths"}.get(mistake)
    if expect is not None:
        assert any(expect in b for b in bad)
    else:
        assert any(k.startswith("y of sequence") for b in bad for k in b)


# ---- the C ABI: layout and refusals (both before any device call) ------------------------------------------------------------------
def test_assemble_case_matches_the_header_layout():
    import ctypes as C
    from gantts_amd import _lib as L
    assert L.AssembleCase.ld_gi.offset == 32 and L.AssembleCase.key0.offset == 60 and L.AssembleCase.win_len.offset == 68
    assert L.AssembleCase.F.offset == 88 and L.AssembleCase.coef.offset == 112 and L.AssembleCase.X_all.offset == 400
    assert L.AssembleCase.lengths.offset == 512 and C.sizeof(L.AssembleCase) == 520


def _valid_case():
    from gantts_amd import _lib as L
    k = L.AssembleCase()
    k.B, k.T, k.Dx, k.Dy, k.nz, k.Ds = 2, 8, 7, 13, 5, 5
    k.ldX, k.ldY, k.ld_gi, k.ld_y, k.ld_ys = 8, 16, 12, 13, 5
    k.x_kind, k.y_kind, k.stats_f64 = L.SCALE_MINMAX, L.SCALE_MEANVAR, 3
    k.F, k.n_slots, k.first_slot = 100, 4, 0
    for name in ("X_all", "Y_all", "x_a", "x_b", "y_a", "y_b", "table", "scol", "gi", "y", "y_static", "mask", "lengths"):
        setattr(k, name, 0x1000)           # never dereferenced: every case below is refused before the launch
    return k


@pytest.mark.parametrize("field,value,message", [
    ("ldX", 7, "16-byte pitch"), ("ldY", 12, "16-byte pitch"), ("X_all", 0x1004, "16-byte pitch"), ("ld_gi", 11, "gi needs"),
    ("ld_gi", 8, "gi needs"), ("first_slot", 3, "slots"), ("first_slot", -1, "slots"), ("x_kind", 3, "scaling kind"), ("y_b", None, "null statistics"),
    ("table", None, "null corpus or table"), ("ld_y", 12, "ld_y"), ("scol", None, "y_static needs"), ("stats_f64", 4, "stats_f64"), ("T", 0, "bad sizes"),
    ("dsrc", 0x1000, "delta recomputation")])
def test_a_malformed_assemble_case_is_refused_before_the_launch(field, value, message):
    import ctypes as C
    from gantts_amd import _lib as L
    k = _valid_case()
    setattr(k, field, value)
    assert L.lib.gt_op_assemble_batch(C.byref(k), None) == L.GT_ERR_INVALID
    assert message in L.lib.gt_last_error().decode()
    assert L.lib.gt_op_assemble_batch(None, None) == L.GT_ERR_INVALID
