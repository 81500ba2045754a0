"""Host-side construction of the MLPG matrix ``R = (W^T W)^-1 W^T`` -- the piece of
``nnmnkwii.paramgen`` the step path needs (reference train.py:49, 510-515 calls
``unit_variance_mlpg_matrix(hp.windows, max_len)`` for every batch).

Differences from the reference call pattern (results identical): W^T W is banded, so it is
solved with a banded Cholesky in float64 (O(T^2) instead of a dense inverse), and the result is
cached per (windows, T) together with its device copy -- the reference rebuilds it on the host
and uploads T x 3T floats every batch.

``MLPGBand`` / ``unit_variance_mlpg_band`` stand for the same matrix without forming it: the engine builds the taps its
kernels read on the device from the windows (gt_set_mlpg_windows, GT_MLPG_R_FROM_WINDOWS) -- no O(T^2) host work, upload or
cache entry per padded length.

``mlpg`` / ``mlpg_batch`` are ``nnmnkwii.paramgen.mlpg`` itself -- the general maximum-likelihood parameter generation with per-dimension
or per-frame variances, which no R expresses -- as a batch of banded solves on the device (gt_op_mlpg_var).
"""
import numpy as np
import scipy.linalg

_cache = {}
_dev_cache = {}


def _signature(windows, T):
    return (int(T),) + tuple((int(l), int(u), tuple(float(c) for c in np.asarray(w).ravel())) for (l, u, w) in windows)


def unit_variance_mlpg_matrix(windows, T):
    """(T, len(windows)*T) float32; column block w holds window w (window-major)."""
    T = int(T)
    key = _signature(windows, T)
    hit = _cache.get(key)
    if hit is not None:
        return hit
    nW = len(windows)
    Wt = np.zeros((T, nW * T), dtype=np.float64)            # W^T, block w = W_w^T
    bw = max(max(int(l), int(u)) for (l, u, _) in windows)
    for w, (l, u, coef) in enumerate(windows):
        coef = np.asarray(coef, dtype=np.float64)
        for k in range(-int(l), int(u) + 1):
            c = coef[k + int(l)]
            if c == 0.0:
                continue
            t = np.arange(max(0, -k), min(T, T - k))          # (W_w x)[t] += c * x[t + k]
            Wt[t + k, w * T + t] = c
    P = Wt @ Wt.T                                             # W^T W, bandwidth 2*bw
    ub = min(2 * bw, T - 1)
    ab = np.zeros((ub + 1, T), dtype=np.float64)              # upper banded storage for solveh_banded
    for d in range(ub + 1):
        ab[ub - d, d:] = np.diagonal(P, d)
    R = scipy.linalg.solveh_banded(ab, Wt, lower=False, check_finite=False)
    R = np.ascontiguousarray(R.astype(np.float32))
    R.setflags(write=False)
    _cache[key] = R
    return R


def unit_variance_mlpg_matrix_cuda(windows, T, device="cuda"):
    """Device-resident copy, cached: one upload per distinct T instead of one per batch."""
    import torch
    key = (_signature(windows, T), str(device))
    hit = _dev_cache.get(key)
    if hit is None:
        hit = _dev_cache[key] = torch.from_numpy(np.array(unit_variance_mlpg_matrix(windows, T))).to(device)
    return hit


class MLPGBand(object):
    """``R = (W^T W)^-1 W^T`` of ``unit_variance_mlpg_matrix(windows, T)`` as a weightless stand-in: it holds the windows and ``T``,
    and quacks like the (T, num_windows * T) matrix where the reference asks for its shape (``R.size(1) // R.size(0)``,
    multistream.py:88).  Accepted wherever the step functions take R; the engine builds the band on the device."""

    def __init__(self, windows, T):
        T = int(T)
        if T < 1:
            raise ValueError("MLPGBand: T must be positive, got %d" % T)
        if len(windows) < 1:
            raise ValueError("MLPGBand: no windows")
        self.windows = [(int(l), int(u), np.array(np.asarray(c, dtype=np.float64).ravel())) for (l, u, c) in windows]
        for l, u, c in self.windows:
            if l < 0 or u < 0 or c.size != l + u + 1:
                raise ValueError("MLPGBand: a window is (l, u, l + u + 1 coefficients), got (%d, %d, %d coefficients)" % (l, u, c.size))
        self.T = T
        self.num_windows = len(self.windows)
        self.shape = (T, self.num_windows * T)
        self.signature = _signature(self.windows, T)

    @property
    def window_signature(self):
        """the windows alone (what an engine registers once): equal for every T"""
        return self.signature[1:]

    def size(self, i=None):
        return self.shape if i is None else self.shape[i]

    def dim(self):
        return 2

    def dense(self):
        """today's host matrix (float32, read-only, cached)"""
        return unit_variance_mlpg_matrix(self.windows, self.T)

    def __eq__(self, other):
        return isinstance(other, MLPGBand) and self.signature == other.signature

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self.signature)

    def __repr__(self):
        return "MLPGBand(num_windows=%d, T=%d)" % (self.num_windows, self.T)


def unit_variance_mlpg_band(windows, T):
    """Drop-in for ``unit_variance_mlpg_matrix_cuda`` that never forms R."""
    return MLPGBand(windows, T)


_var_engines = {}


def _check_mlpg_args(means, variances, windows, batch):
    """shapes of ``mlpg`` / ``mlpg_batch``: ValueError before anything touches the device"""
    nd = 3 if batch else 2
    if len(windows) < 1:
        raise ValueError("mlpg: no windows")
    if len(means.shape) != nd:
        raise ValueError("mlpg: mean_frames must have %d dimensions, got shape %s" % (nd, tuple(means.shape)))
    D = int(means.shape[-1])
    if D % len(windows) != 0:
        raise ValueError("mlpg: the feature dimension %d is no multiple of the %d windows" % (D, len(windows)))
    if tuple(variances.shape) != (D,) and tuple(variances.shape) != tuple(means.shape):
        raise ValueError("mlpg: variance_frames must be (%d,) or %s, got %s" % (D, tuple(means.shape), tuple(variances.shape)))
    return D


def _var_engine(D, windows):
    """a cached engine of one stream with dynamic features, keyed by (D, windows): the idea of ``inference._engine``"""
    from .engine import StepEngine, _SingleStreamHP
    key = (int(D),) + _signature(windows, 0)[1:]
    eng = _var_engines.get(key)
    if eng is None:
        hp = _SingleStreamHP(int(D), len(windows), True)
        hp.windows = list(windows)
        eng = _var_engines[key] = StepEngine(hp)
    return eng


def mlpg_batch(means, variances, windows, lengths=None):
    """``mlpg`` for a padded batch: ``means`` (B, T, D), ``variances`` (D,) or (B, T, D), ``lengths`` B entries in [1, T] (all T when
    None).  Every sequence is solved over its own length, as if evaluated alone; its rows beyond are 0.  One call to the operator.
    Returns (B, T, D // len(windows)) in the input's dtype: numpy in, numpy out; a CUDA tensor in, a tensor out."""
    import torch
    as_tensor = isinstance(means, torch.Tensor)
    if not as_tensor:
        means, variances = np.asarray(means), np.asarray(variances)
    D = _check_mlpg_args(means, variances, windows, True)
    if lengths is not None and len(lengths) != means.shape[0]:
        raise ValueError("mlpg: lengths has %d entries for a batch of %d sequences" % (len(lengths), means.shape[0]))
    eng = _var_engine(D, windows)
    if as_tensor:
        y = means.detach().to(device="cuda", dtype=torch.float32)
        v = torch.as_tensor(variances).detach().to(device="cuda", dtype=torch.float32)
    else:
        y = torch.from_numpy(np.ascontiguousarray(means, dtype=np.float32)).cuda()
        v = torch.from_numpy(np.ascontiguousarray(variances, dtype=np.float32)).cuda()
    out = eng.mlpg_var(y, v, lengths=lengths, windows=windows)
    return out.to(means.dtype) if as_tensor else out.cpu().numpy().astype(means.dtype, copy=False)


def mlpg(mean_frames, variance_frames, windows):
    """``nnmnkwii.paramgen.mlpg``: for every static dimension the c that solves
    ``(sum_w W_w^T diag(1 / var_w) W_w) c = sum_w W_w^T (mean_w / var_w)``, on the device in float64 (rounded to float32 once).
    ``mean_frames`` (T, D) with the static and dynamic features window-major; ``variance_frames`` (D,) or (T, D); returns
    (T, D // len(windows)) in the input's dtype: numpy in, numpy out; a CUDA tensor in, a tensor out.  ValueError for shapes that do
    not fit and for variances that are not finite and positive; RuntimeError without a GPU."""
    import torch
    as_tensor = isinstance(mean_frames, torch.Tensor)
    if not as_tensor:
        mean_frames, variance_frames = np.asarray(mean_frames), np.asarray(variance_frames)
    _check_mlpg_args(mean_frames, variance_frames, windows, False)
    var = variance_frames if len(variance_frames.shape) == 1 else variance_frames[None]
    return mlpg_batch(mean_frames[None], var, windows)[0]
