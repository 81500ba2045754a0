"""paramgen.MLPGBand: the weightless stand-in of the MLPG matrix R (CPU only).  What the device makes of it is checked in
tests/test_gpu_mlpg_band.py."""
import numpy as np
import pytest

import cases as C
from gantts_amd import paramgen

ASYM = [(0, 0, np.array([1.0])), (0, 1, np.array([-1.0, 1.0])), C.WINDOWS[2]]


@pytest.mark.parametrize("T", [1, 2, 17, 40])
def test_shape_size_and_dim_are_those_of_the_matrix(T):
    b = paramgen.MLPGBand(C.WINDOWS, T)
    R = paramgen.unit_variance_mlpg_matrix(C.WINDOWS, T)
    assert b.T == T and b.num_windows == len(C.WINDOWS) == 3
    assert b.shape == R.shape == (T, 3 * T)
    assert b.size() == R.shape and b.size(0) == T and b.size(1) == 3 * T and b.size(-1) == 3 * T and b.dim() == R.ndim == 2
    assert b.size(1) // b.size(0) == 3                      # multi_stream_mlpg's num_windows (reference multistream.py:88)
    assert [(l, u) for l, u, _ in b.windows] == [(l, u) for l, u, _ in C.WINDOWS]
    for (_, _, got), (_, _, want) in zip(b.windows, C.WINDOWS):
        assert got.dtype == np.float64 and np.array_equal(got, want)
    assert isinstance(paramgen.unit_variance_mlpg_band(C.WINDOWS, T), paramgen.MLPGBand)


def test_dense_is_the_host_matrix():
    for windows, T in ((C.WINDOWS, 23), (ASYM, 9), (C.WINDOWS[:1], 5)):
        b = paramgen.MLPGBand(windows, T)
        R = paramgen.unit_variance_mlpg_matrix(windows, T)
        assert b.dense() is R                                   # the cached host matrix itself
        assert R.dtype == np.float32 and not R.flags.writeable


def test_signature_equality():
    a = paramgen.MLPGBand(C.WINDOWS, 20)
    same = paramgen.MLPGBand([(int(l), int(u), [float(c) for c in w]) for l, u, w in C.WINDOWS], 20.0)      # lists, a float T
    assert a == same and hash(a) == hash(same) and not (a != same)
    assert a.signature == paramgen._signature(C.WINDOWS, 20)
    other_T, other_w = paramgen.MLPGBand(C.WINDOWS, 21), paramgen.MLPGBand(ASYM, 20)
    assert a != other_T and a != other_w and a != "R"
    assert a.window_signature == other_T.window_signature != other_w.window_signature      # what an engine registers: T is not part of it
    assert len({a, same, other_T, other_w}) == 3
    # the object keeps its own copy of the coefficients
    w = [(1, 1, np.array([1.0, -2.0, 1.0]))]
    b = paramgen.MLPGBand(w, 4)
    w[0][2][1] = 5.0
    assert b.windows[0][2][1] == -2.0 and b == paramgen.MLPGBand([(1, 1, [1.0, -2.0, 1.0])], 4)


def test_malformed_arguments_are_refused():
    with pytest.raises(ValueError):
        paramgen.MLPGBand(C.WINDOWS, 0)
    with pytest.raises(ValueError):
        paramgen.MLPGBand([], 5)
    with pytest.raises(ValueError):
        paramgen.MLPGBand([(1, 1, np.array([1.0, -1.0]))], 5)       # two coefficients for l + u + 1 = 3
    with pytest.raises(ValueError):
        paramgen.MLPGBand([(-1, 1, np.array([1.0]))], 5)


def test_library_declares_the_sentinel_and_the_span_as_the_header_does():
    import os
    import re
    from gantts_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gantts_hip.h")).read()
    assert int(re.search(r"#define GT_MLPG_R_FROM_WINDOWS \(\(const float\*\)\(uintptr_t\)(\d+)\)", src).group(1)) == _lib.MLPG_R_FROM_WINDOWS
    assert int(re.search(r"#define GT_MLPG_MAX_WINDOW_SPAN (\d+)", src).group(1)) == _lib.MLPG_MAX_WINDOW_SPAN
    # without a device the registration still validates its arguments before anything touches the GPU
    assert _lib.lib.gt_set_mlpg_windows(None, 1, None, None, None) == _lib.GT_ERR_INVALID
