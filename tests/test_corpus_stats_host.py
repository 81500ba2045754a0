"""CPU checks of the corpus statistics' reference and bound (tests/corpus_stats_ref.py): the host's data.meanvar and sklearn's
_incremental_mean_and_var (the routine nnmnkwii's meanvar rests on; nnmnkwii itself is not vendored: parity unpinned) are inside the derived
bound on exactly the inputs tests/test_gpu_corpus_stats.py puts to the device; the numpy model of the kernel is inside it and each of its
seeded mistakes is rejected; the host-side halves of ResidentCorpus.from_arrays (validation, segment table, the refusal of a loader before
statistics are attached) need no device."""
import types

import numpy as np
import pytest

import corpus_stats_ref as S
from gantts_amd import _lib as L
from gantts_amd import data as D

WIDTHS, ROWS = S.WIDTHS, S.ROWS      # the GPU test's widths and row counts


def test_the_model_is_built_for_the_kernel_as_built():
    assert (S.SLAB, S.FANIN) == (L.CORPUS_STATS_SLAB, L.CORPUS_STATS_FANIN)


@pytest.mark.parametrize("Dn", WIDTHS)
def test_host_meanvar_is_inside_the_bound_on_the_gpu_tests_inputs(Dn):
    worst = 0.0
    for F in ROWS:
        for family in S.FAMILIES:
            X, cut = S.make_corpus(family, F, Dn)
            for lengths in (None, cut):
                ref = S.reference(X, lengths)
                mean, var, n = D.meanvar(X, lengths, return_last_sample_count=True)
                mean, var = np.broadcast_to(mean, (Dn,)).copy(), np.broadcast_to(var, (Dn,)).copy()
                assert S.mismatches(mean, var, n, ref, Dn) == [], (F, family, lengths is not None)
                if family == "constant":
                    assert S.constant_mismatches(mean, var, 0, np.float32(0.1)) == []
                worst = max(worst, *(float(e.max()) for e in S.errors(mean, var, ref)))
    print("D=%d: host meanvar at most %.3g of the bound" % (Dn, worst))


def _probe(family):
    """The probe's shape: 40 utterances of 1-59 frames, 7 columns."""
    rs = np.random.RandomState(7)
    F = int(rs.randint(1, 60, size=40).sum())
    return S.make_corpus(family, F, 7, seed=3)


@pytest.mark.parametrize("family", S.FAMILIES)
def test_sklearns_incremental_mean_and_var_is_inside_the_bound(family):
    """On a constant column the bound is 0 (dmax = 0): the host and the device have to be exact there and are.  sklearn is not: its
    mean is exact but its variance comes out as 2.3e-35 / 1.0e-35 (all rows / cut rows) where 0.0 is due, the second-order term
    (mean error)^2 <= (n u amax)^2 = 1.9e-28 / 4.2e-29 that the first-order bound leaves out.  That column of sklearn's is held to this
    second-order term instead; every other column, and everything of the host and the device, to the bound as it stands."""
    from sklearn.utils.extmath import _incremental_mean_and_var
    X, cut = _probe(family)
    for lengths in (None, cut):
        mean, var, n = np.zeros(7), np.zeros(7), np.zeros(7)
        for i, x in enumerate(X):      # nnmnkwii's meanvar: one utterance at a time
            x = x[:(None if lengths is None else lengths[i])].astype(np.float64)
            mean, var, n = _incremental_mean_and_var(x, mean, var, n)
        ref = S.reference(X, lengths)
        mean, var = np.asarray(mean, np.float64), np.asarray(var, np.float64)
        if family == "constant":
            print("sklearn on the constant column: mean error %.3g, var %.3g" % (mean[0] - np.float64(np.float32(0.1)), var[0]))
            assert mean[0] == np.float64(np.float32(0.1)) and 0.0 <= var[0] <= (ref["n"] * S.U * float(ref["amax"][0])) ** 2
            var[0] = 0.0
        assert S.mismatches(mean, var, int(np.asarray(n).reshape(-1)[0]), ref, 7) == []


@pytest.mark.parametrize("family", S.FAMILIES)
def test_the_kernel_model_is_inside_the_bound(family):
    X, cut = _probe(family)
    for lengths in (None, cut):
        for kw in (dict(), dict(slab=32, fanin=2)):      # the kernel's own sizes; sizes at which this corpus needs every level
            lo, hi, mean, var, n = S.kernel_model(X, lengths, **kw)
            ref = S.reference(X, lengths)
            assert S.mismatches(mean, var, n, ref, 7) == [] and S.minmax_mismatches(lo, hi, X, lengths) == []
            if family == "constant":
                assert S.constant_mismatches(mean, var, 0, np.float32(0.1)) == []
    # continued over a second corpus: the statistic of the concatenation
    X2, cut2 = S.make_corpus(family, 700, 7, seed=9)
    _, _, m1, v1, n1 = S.kernel_model(X, cut, slab=32, fanin=2)
    _, _, mean, var, n = S.kernel_model(X2, cut2, prior=(m1, v1, n1), slab=32, fanin=2)
    both = S.reference(X + X2, cut + cut2)
    assert S.mismatches(mean, var, n, both, 7) == []
    hm, hv, hn = D.meanvar(X, cut, return_last_sample_count=True)
    hm, hv, hn = D.meanvar(X2, cut2, mean_=hm, var_=hv, last_sample_count=hn, return_last_sample_count=True)
    assert S.mismatches(hm, hv, hn, both, 7) == []


@pytest.mark.parametrize("mistake", S.MISTAKES)
def test_the_comparators_reject_the_seeded_mistakes(mistake):
    X, cut = _probe("normal")
    if mistake == "prior_ignored":
        X2, cut2 = S.make_corpus("normal", 700, 7, seed=9)
        _, _, m1, v1, n1 = S.kernel_model(X, cut, slab=32, fanin=2)
        _, _, mean, var, n = S.kernel_model(X2, cut2, prior=(m1, v1, n1), mistake=mistake, slab=32, fanin=2)
        ref = S.reference(X + X2, cut + cut2)
    else:
        _, _, mean, var, n = S.kernel_model(X, cut, mistake=mistake, slab=32, fanin=2)
        ref = S.reference(X, cut)
    bad = S.mismatches(mean, var, n, ref, 7)
    assert bad != [], mistake
    print(mistake, "->", bad)


@pytest.mark.parametrize("family", S.FAMILIES)
def test_a_float32_accumulator_is_far_outside_the_bound(family):
    X, _ = _probe(family)
    _, _, mean, var, _ = S.kernel_model(X, mistake="float32_accumulation", slab=32, fanin=2)
    rm, rv = S.errors(mean, var, S.reference(X))
    cols = slice(1, None) if family == "constant" else slice(None)      # the constant column is exact in any precision
    assert rm[cols].max() > 1e3, rm


def test_the_minmax_comparator_follows_numpy():
    X, cut = _probe("normal")
    X[3][0, 2] = np.nan
    X[5][1, 4], X[6][0, 5] = np.inf, -np.inf
    lo, hi = D.minmax(X)
    assert S.minmax_mismatches(lo, hi, X) == [] and np.isnan(lo[2]) and np.isnan(hi[2]) and hi[4] == np.inf and lo[5] == -np.inf
    assert np.isfinite(np.delete(lo, [2, 5])).all() and np.isfinite(np.delete(hi, [2, 4])).all()
    mlo, mhi = S.kernel_model(X)[:2]
    assert S.minmax_mismatches(mlo, mhi, X) == []
    assert S.minmax_mismatches(np.nan_to_num(lo, nan=0.0), hi, X) == ["min"]                    # a NaN swallowed (fminf)
    assert S.minmax_mismatches(lo.astype(np.float64), hi, X) == ["min"]                         # the dtype
    assert S.minmax_mismatches(*D.minmax(X), X, cut) != []                                      # lengths ignored


# ---- the host half of ResidentCorpus.from_arrays ---------------------------------------------------------------------------------------
def test_a_raw_corpus_lays_out_its_segments_and_refuses_a_loader():
    X, cut = _probe("normal")
    Y = [x[:, :3] for x in X]
    corpus = D.ResidentCorpus.from_arrays(X, Y, device=None)
    lens = np.array([len(x) for x in X])
    assert corpus.F == lens.sum() and (corpus.Dx, corpus.Dy, corpus.ldX, corpus.ldY) == (7, 3, 8, 4) and corpus.dataset is None
    seg = corpus.segments()
    assert seg.dtype == np.int64 and seg.shape == (len(X), 2)
    assert np.array_equal(seg[:, 0], np.cumsum(lens) - lens) and np.array_equal(seg[:, 1], lens)
    assert np.array_equal(corpus.segments(cut)[:, 1], cut) and np.array_equal(corpus.segments(lens + 5)[:, 1], lens)
    hp = types.SimpleNamespace(generator_add_noise=False, windows=[(0, 0, np.array([1.0]))], stream_sizes=[3], has_dynamic_features=[False])
    with pytest.raises(ValueError, match="no statistics attached"):
        D.ResidentLoader(corpus, 4, False, hp)
    with pytest.raises(RuntimeError, match="not on the device"):
        corpus.meanvar("y")
    with pytest.raises(ValueError, match="side"):
        corpus.minmax("z")
    ds = D.TTSDataset(X, Y, *D.minmax(X), *D.meanvar(Y), hp=None)
    corpus.attach_statistics(ds)
    loader = D.ResidentLoader(corpus, 4, False, hp)
    assert loader.dataset is ds and corpus.stats_f64 == 2
    with pytest.raises(ValueError, match="attached already"):
        corpus.attach_statistics(ds)


def test_from_arrays_validates_like_the_dataset_constructor():
    x = np.zeros((3, 5), np.float32)
    with pytest.raises(ValueError, match="empty dataset"):
        D.ResidentCorpus.from_arrays([], [], device=None)
    with pytest.raises(TypeError, match="float32 arrays only"):
        D.ResidentCorpus.from_arrays([x.astype(np.float64)], [x], device=None)
    with pytest.raises(ValueError, match="3 input and 2 output frames"):
        D.ResidentCorpus.from_arrays([x], [x[:2]], device=None)
    with pytest.raises(ValueError, match="differ in width"):
        D.ResidentCorpus.from_arrays([x, x[:, :4]], [x, x], device=None)
    with pytest.raises(ValueError, match="2 input and 1 output utterances"):
        D.ResidentCorpus.from_arrays([x, x], [x], device=None)
