"""Host checks of variance-weighted MLPG (no GPU): the reference of tests/mlpg_var_ref.py against an independent dense construction, the
condition attached to the comparator's bound for every case the GPU tests use, the comparator against seeded mistakes in a float64 model
of the device's column solve, and the argument errors of gantts_amd.paramgen.mlpg."""
import numpy as np
import pytest

import mlpg_var_ref as V

SETS = V.window_sets()
DENSE_CASES = [(n, T, f) for n in V.SET_NAMES for T in (1, 2, 3, 5, 17, 65) for f in ("row", "frame")]


def test_half_bandwidths_reach_every_form():
    assert [V.half_bandwidth(SETS[n]) for n in V.SET_NAMES] == [2, 0, 2, 2, 4, 1]


@pytest.mark.parametrize("name,T,form", DENSE_CASES, ids=["%s_T%d_%s" % c for c in DENSE_CASES])
def test_reference_equals_the_dense_construction(name, T, form):
    windows = SETS[name]
    _, _, scol, sst, _, _ = V.layout(5, len(windows))
    y, var, lengths, ref = V.case(name, T, form)
    dense = V.reference(y, var, windows, scol, sst, lengths, solver=V.solve_column_dense)
    peak = np.abs(dense).max(axis=1, keepdims=True)
    # two float64 solves of a system with cond <= 2^11: each within a few hundred 2^-53 of the solution
    assert (np.abs(ref - dense) <= 2.0 ** -40 * peak).all()
    assert np.array_equal(ref[:, :, sst == 0], dense[:, :, sst == 0])


@pytest.mark.parametrize("name", V.SET_NAMES)
def test_condition_of_every_case_is_within_the_bounds_premise(name):
    windows = SETS[name]
    nW = len(windows)
    _, _, scol, sst, _, _ = V.layout(5, nW)
    worst = 0.0
    for T in V.T_VALUES:
        for form in V.VAR_FORMS:
            y, var, lengths, _ = V.case(name, T, form)
            seen = set()
            for b, n in enumerate(lengths):
                for c in np.nonzero(sst > 0)[0]:
                    key = (n,) if form == "ones" else (n, c) if form == "row" else (b, c)      # P depends on nothing else
                    if key in seen:
                        continue
                    seen.add(key)
                    worst = max(worst, V.condition(*V.columns_of(y, var, scol, sst, nW, b, c, n), windows))
    print("%s: worst cond(P) %.1f" % (name, worst))
    assert worst <= V.COND_LIMIT


MODEL_CASES = [("std", 17, "frame"), ("std", 65, "row"), ("four", 17, "frame"), ("hb1", 17, "row"), ("asym", 5, "frame"), ("static", 3, "row")]


@pytest.mark.parametrize("name,T,form", MODEL_CASES, ids=["%s_T%d_%s" % c for c in MODEL_CASES])
def test_model_of_the_column_solve_passes_the_comparator(name, T, form):
    windows = SETS[name]
    _, _, scol, sst, _, _ = V.layout(5, len(windows))
    y, var, lengths, ref = V.case(name, T, form)
    worst, over, bad = V.compare(V.model(y, var, windows, scol, sst, lengths), ref, y, scol, sst, lengths)
    assert over == 0 and bad == 0 and worst <= 1.0
    # the float64 part alone: the model before its rounding, against scipy
    b, c, n = 0, 0, lengths[0]
    x = V.model_column(y, var, windows, scol, sst, b, c, n)
    assert np.abs(x - ref[b, :n, c]).max() <= V.U40 * np.abs(ref[b, :n, c]).max() / 40


@pytest.mark.parametrize("mistake", V.MISTAKES)
def test_comparator_rejects_seeded_mistakes(mistake):
    form = "row" if mistake == "row_frame_stride" else "frame"
    # (hb1's windows reach forwards only, l_w = 0: frames beyond a length touch no column inside it, so "edge" is no mistake there)
    for name, T in (("std", 17), ("delta", 5) if mistake == "edge" else ("hb1", 5), ("four", 17)):
        windows = SETS[name]
        _, _, scol, sst, _, _ = V.layout(5, len(windows))
        y, var, lengths, ref = V.case(name, T, form)
        worst, over, bad = V.compare(V.model(y, var, windows, scol, sst, lengths, mistake), ref, y, scol, sst, lengths)
        assert over > 0 or bad > 0, "%s went unseen on %s T=%d (worst ratio %.3g)" % (mistake, name, T, worst)


def test_comparator_rejects_one_ulp_and_touched_exact_elements():
    windows = SETS["std"]
    _, _, scol, sst, _, _ = V.layout(5, 3)
    y, var, lengths, ref = V.case("std", 17, "frame")
    good = V.model(y, var, windows, scol, sst, lengths)
    off = good.copy()
    off[0, 3, 0] = np.nextafter(np.nextafter(off[0, 3, 0], np.float32(np.inf)), np.float32(np.inf))      # two float32 steps: beyond one rounding
    assert V.compare(off, ref, y, scol, sst, lengths)[1] == 1
    tail = good.copy()
    tail[1, lengths[1], 2] = np.float32(-0.0)
    assert V.compare(tail, ref, y, scol, sst, lengths)[2] == 1
    pt = good.copy()
    c = int(np.nonzero(sst == 0)[0][0])
    pt[0, 0, c] = np.nextafter(pt[0, 0, c], np.float32(np.inf))
    assert V.compare(pt, ref, y, scol, sst, lengths)[2] == 1
    nan = good.copy()
    nan[2, 0, 1] = np.nan
    assert V.compare(nan, ref, y, scol, sst, lengths)[1] == 1


# ---------------------------------------------------------------------------------------------------------------------
# paramgen.mlpg: argument errors come before anything touches the device
# ---------------------------------------------------------------------------------------------------------------------
def test_mlpg_refuses_a_dimension_that_is_no_multiple_of_the_windows():
    from gantts_amd import paramgen
    with pytest.raises(ValueError, match="multiple"):
        paramgen.mlpg(np.zeros((5, 10), np.float32), np.ones(10, np.float32), SETS["std"])
    with pytest.raises(ValueError, match="multiple"):
        paramgen.mlpg_batch(np.zeros((2, 5, 10), np.float32), np.ones(10, np.float32), SETS["std"])


def test_mlpg_refuses_shapes_that_do_not_fit():
    from gantts_amd import paramgen
    for var in (np.ones(6, np.float32), np.ones((4, 9), np.float32), np.ones((5, 9, 1), np.float32)):
        with pytest.raises(ValueError, match="variance_frames"):
            paramgen.mlpg(np.zeros((5, 9), np.float32), var, SETS["std"])
    with pytest.raises(ValueError, match="dimensions"):
        paramgen.mlpg(np.zeros(9, np.float32), np.ones(9, np.float32), SETS["std"])
    with pytest.raises(ValueError, match="dimensions"):
        paramgen.mlpg_batch(np.zeros((5, 9), np.float32), np.ones(9, np.float32), SETS["std"])
    with pytest.raises(ValueError, match="lengths"):
        paramgen.mlpg_batch(np.zeros((2, 5, 9), np.float32), np.ones(9, np.float32), SETS["std"], lengths=[5])
    with pytest.raises(ValueError, match="no windows"):
        paramgen.mlpg(np.zeros((5, 9), np.float32), np.ones(9, np.float32), [])


def test_ctypes_case_matches_the_header_layout():
    from gantts_amd import _lib
    import ctypes as C
    assert _lib.MlpgVarCase.B.offset == 8 and _lib.MlpgVarCase.ldys.offset == 28 and _lib.MlpgVarCase.scol.offset == 32
    assert _lib.MlpgVarCase.lengths.offset == 48 and _lib.MlpgVarCase.y.offset == 56 and _lib.MlpgVarCase.max_ws_bytes.offset == 80
    assert C.sizeof(_lib.MlpgVarCase) == 88


def test_gen_parameters_without_mge_is_its_own_entry():
    """gen_parameters(mge_training=False) keeps refusing, and names the entry that does the work; without a GPU that entry fails like
    every compute entry (RuntimeError), not with NotImplementedError"""
    import torch
    from gantts_amd import inference
    with pytest.raises(NotImplementedError, match="gen_parameters_without_mge"):
        inference.gen_parameters(np.zeros((4, 187), np.float32), np.zeros(187), np.ones(187), mge_training=False)
    if torch.cuda.is_available():
        return
    with pytest.raises(RuntimeError) as ei:
        inference.gen_parameters_without_mge(np.zeros((4, 187), np.float32), np.zeros(187), np.ones(187))
    assert not isinstance(ei.value, NotImplementedError)
