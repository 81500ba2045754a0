"""Reference of the device-resident batch path (gantts_amd.data.ResidentLoader, gt_op_assemble_batch): the existing HOST pipeline
itself, run on synthetic in-memory corpora, plus a numpy model of the kernel whose seeded mistakes the comparator must reject.

Reference (``reference_batches``), per list of utterance indices:
    [dataset[i] for i in idx] -> collate_fn -> the sort and trim of DevicePrefetcher._stage -> the static columns
    (get_static_features' own column list, multistream.static_columns, applied with numpy: the gather is a bit-exact copy) ->
    the mask of sequence_mask ((t < length) as float32) -> the noise restated below.

Noise keying (gantts_amd/csrc/data_kernels.hip.h): column j of z at frame t of corpus utterance u is word j & 3 of
    philox4x32_10(c0 = u, c1 = t * G + (j >> 2), c2 = 0x243F6A88, c3 = 0x85A308D3, key0, key1),   G = ceil(nz / 4)
    z = (word >> 8) * 2^-24
on every frame of the padded batch (t >= length included); key0 = low word of hp.generator_noise_seed, key1 = the loader's draw counter.
"""
import types

import numpy as np
import torch

from gantts_amd import data as D
from gantts_amd.multistream import static_columns
from test_gpu_gemm_f32 import philox4x32_10

LENGTHS = [37, 120, 5, 120, 64, 1, 99, 3, 120]      # ties, a length of 1, lengths equal to the longest window of a batch
LENGTHS_DELTA = [37, 120, 5, 120, 64, 3, 99, 3, 120]      # >= 3 frames: np.correlate(..., "same") needs len >= the window's
WINDOWS = [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5])), (1, 1, np.array([1.0, -2.0, 1.0]))]
SMALL = dict(Dx=7, Dy=13, stream_sizes=[6, 3, 1, 3], has_dynamic_features=[True, True, False, True])      # Ds = 5
REAL = dict(Dx=425, Dy=187, stream_sizes=[180, 3, 1, 3], has_dynamic_features=[True, True, False, True])  # pitch 428 / 188, Ds = 63
VC = dict(Dx=9, Dy=9, stream_sizes=[9], has_dynamic_features=[True])                                      # Ds = 3


def make_hp(widths, nz=0, seed=20240607, recompute=False, name="acoustic"):
    return types.SimpleNamespace(name=name, windows=WINDOWS, stream_sizes=list(widths["stream_sizes"]),
                                 has_dynamic_features=list(widths["has_dynamic_features"]), generator_add_noise=nz > 0,
                                 generator_noise_dim=nz, generator_noise_seed=seed, recompute_delta_features=recompute)


def make_dataset(kind, widths, stats_dtype, lengths=LENGTHS, hp=None, seed=5):
    """A synthetic in-memory corpus behind the project's own dataset classes.  kind: "tts" (min-max x, mean-variance y) or "vc"
    (one mean-variance for both sides)."""
    rs = np.random.RandomState(seed)
    Dx, Dy = widths["Dx"], widths["Dy"]
    X = [(rs.randn(n, Dx) * 3.0 + 1.0).astype(np.float32) for n in lengths]
    Y = [(rs.randn(n, Dy) * 2.0 - 0.5).astype(np.float32) for n in lengths]
    dt = np.dtype(stats_dtype)
    if kind == "vc":
        mean, std = (rs.randn(Dy) * 0.3).astype(dt), (0.5 + rs.rand(Dy)).astype(dt)
        return D.VCDataset(X, Y, mean, std)
    lo, hi = D.minmax(X)
    lo, hi = lo.astype(dt), hi.astype(dt)
    hi[0] = lo[0]                                    # a constant column: scale 1 (minmax_scale_params)
    mean, std = (rs.randn(Dy) * 0.3).astype(dt), (0.5 + rs.rand(Dy)).astype(dt)
    ds = D.TTSDataset(X, Y, lo, hi, mean, std, hp=hp)
    assert ds.X_data_scale.dtype == dt and ds.X_data_min.dtype == dt
    return ds


def noise(key0, key1, utt, T, nz):
    """z (T, nz) float32 of corpus utterance ``utt``: the keying of the module docstring."""
    G = (nz + 3) // 4
    t = np.arange(T, dtype=np.uint64)[:, None]
    g = np.arange(G, dtype=np.uint64)[None, :]
    w = philox4x32_10(np.full((T, G), utt, dtype=np.uint64), t * np.uint64(G) + g, 0x243F6A88, 0x85A308D3, key0, key1)
    words = np.stack(w, axis=-1).reshape(T, 4 * G)[:, :nz]
    return ((words >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def reference_batches(dataset, hp, batches, key1=0):
    """The host pipeline's batches for the index lists ``batches``: dicts of numpy arrays x, y, y_static, mask (B, T, 1), lengths,
    z (or None), gi = [x | z], and the corpus order ``order`` of the batch's sequences."""
    nz = int(hp.generator_noise_dim) if hp.generator_add_noise else 0
    key0 = int(hp.generator_noise_seed) & 0xFFFFFFFF
    out = []
    for idx in batches:
        x, y, lengths = D.collate_fn([dataset[i] for i in idx])
        sorted_lengths, indices = torch.sort(lengths.view(-1).long(), dim=0, descending=True)      # DevicePrefetcher._stage
        T = int(sorted_lengths[0])
        x, y = x[indices][:, :T].contiguous().numpy(), y[indices][:, :T].contiguous().numpy()
        order = [int(idx[k]) for k in indices.tolist()]
        lens = sorted_lengths.numpy().astype(np.int64)
        cols = static_columns(len(hp.windows), hp.stream_sizes, hp.has_dynamic_features, None, y.shape[-1])
        mask = (np.arange(T)[None, :] < lens[:, None]).astype(np.float32)[:, :, None]
        z = np.stack([noise(key0, key1, u, T, nz) for u in order]) if nz else None
        out.append(dict(x=x, y=y, y_static=np.ascontiguousarray(y[:, :, cols]), mask=mask, lengths=lens, z=z,
                        gi=np.concatenate((x, z), -1) if nz else x, order=order, T=T))
    return out


KEYS = ("x", "y", "y_static", "mask", "lengths", "z")


def mismatches(got, ref, keys=KEYS):
    """Names of the entries of one batch that are not equal bit for bit (shape, dtype and every element)."""
    bad = []
    for k in keys:
        g, r = got.get(k), ref.get(k)
        if r is None and g is None:
            continue
        if g is None or r is None or g.shape != r.shape or g.dtype != r.dtype or not np.array_equal(g.view(np.uint8), r.view(np.uint8)):
            bad.append(k)
    return bad


def delta_bound(dataset, hp, idx):
    """Float64 host value ``v`` of every recomputed column of one utterance and the bound of the device's float32 result:
    |got - v| <= 2^-24 |v| + 2^-45 sum_k |coef_k x_k|  (the float32 rounding; the order of the float64 sum).  The scaled columns are
    the dataset's own (its statistics' dtype), the sums float64."""
    y = D.scale(dataset.Y[idx], dataset.Y_data_mean, dataset.Y_data_std).astype(np.float64)
    v = D.recompute_delta_features(y.copy(), None, None, hp.windows, hp.stream_sizes, hp.has_dynamic_features)
    absw = [(l, u, np.abs(c)) for l, u, c in hp.windows]
    s = D.recompute_delta_features(np.abs(y), None, None, absw, hp.stream_sizes, hp.has_dynamic_features)
    return v, 2.0 ** -24 * np.abs(v) + 2.0 ** -45 * s


def delta_mismatches(got, ref, dataset, hp):
    """One batch of a corpus with recomputed deltas: everything but y / y_static bit for bit against the host pipeline; the columns of
    window 0 (coefficient [1.0]) and of the streams without dynamic features likewise; every column of y inside ``delta_bound`` of
    its float64 host value; y_static the device's own static columns of y, copied bit for bit."""
    bad = mismatches(got, ref, ("x", "mask", "lengths", "z"))
    cols = static_columns(len(hp.windows), hp.stream_sizes, hp.has_dynamic_features, None, ref["y"].shape[-1])
    if got["y"].shape != ref["y"].shape or got["y"].dtype != np.float32:
        return bad + ["y"]
    if not np.array_equal(got["y"][:, :, cols].view(np.uint32), ref["y"][:, :, cols].view(np.uint32)):
        bad.append("y window 0")
    if not np.array_equal(got["y_static"].view(np.uint32), np.ascontiguousarray(got["y"][:, :, cols]).view(np.uint32)):
        bad.append("y_static")
    for b, (u, n) in enumerate(zip(ref["order"], ref["lengths"])):
        v, bound = delta_bound(dataset, hp, u)
        if not (np.abs(got["y"][b, :n].astype(np.float64) - v) <= bound).all() or np.any(got["y"][b, n:] != 0):
            bad.append("y of sequence %d" % b)
    return bad


# ---- numpy model of the kernel, with the mistakes the comparator has to reject ---------------------------------------------------
MISTAKES = ("z_on_valid_frames_only", "padded_frames_hold_scale_of_zero", "minmax_as_one_fma", "statistics_by_pitched_column",
            "batch_left_unsorted", "delta_taps_cross_the_utterance_end")


def _scale_side(raw, kind, a, b, mistake, ld, rounded=True):
    """raw (n, D) float32 -> float32 (rounded) or the statistics' dtype, each operation rounded on its own (the kernel's arithmetic)."""
    Dn = raw.shape[1]
    cols = np.arange(Dn)
    if mistake == "statistics_by_pitched_column":      # the column taken from a dense index into the pitched rows
        cols = (np.arange(raw.shape[0])[:, None] * Dn + np.arange(Dn)[None, :]) % ld % Dn
    a, b = a[cols], b[cols]
    v = raw.astype(a.dtype)
    if kind == "minmax":
        if mistake == "minmax_as_one_fma":             # one rounding: the product kept exact (float32 x float32 fits float64)
            assert a.dtype == np.float32
            return (v.astype(np.float64) * a.astype(np.float64) + b.astype(np.float64)).astype(np.float32)
        r = v * a + b
    else:
        r = (v - a) / b
    return r.astype(np.float32) if rounded else r


def kernel_model(dataset, hp, batches, key1=0, mistake=None):
    """What gt_op_assemble_batch computes, restated from its header comment on the raw corpus (no dataset.__getitem__, no collate)."""
    tts = hasattr(dataset, "X_data_scale")
    n = len(dataset)
    Xr, Yr = [np.asarray(dataset.X[i]) for i in range(n)], [np.asarray(dataset.Y[i]) for i in range(n)]
    lens_all = np.array([len(a) for a in Xr], dtype=np.int64)
    offsets = np.cumsum(lens_all) - lens_all
    X_all, Y_all = np.concatenate(Xr), np.concatenate(Yr)
    Dx, Dy = X_all.shape[1], Y_all.shape[1]
    if tts:
        xs = ("minmax", np.asarray(dataset.X_data_scale), np.asarray(dataset.X_data_min))
        ys = ("meanvar", np.asarray(dataset.Y_data_mean), np.asarray(dataset.Y_data_std))
    else:
        xs = ys = ("meanvar", np.asarray(dataset.data_mean), np.asarray(dataset.data_std))
    nz = int(hp.generator_noise_dim) if hp.generator_add_noise else 0
    key0 = int(hp.generator_noise_seed) & 0xFFFFFFFF
    cols = static_columns(len(hp.windows), hp.stream_sizes, hp.has_dynamic_features, None, Dy)
    recompute = tts and getattr(dataset, "hp", None) is not None and getattr(dataset.hp, "recompute_delta_features", False)
    table, plan = D.plan_epoch(offsets, lens_all, batches)
    if mistake == "batch_left_unsorted":
        table = np.array([(offsets[u], lens_all[u], u) for idx in batches for u in idx], dtype=np.int64).reshape(-1, 3)
    out = []
    for first, B, T, _ in plan:
        rows = table[first:first + B]
        x, y = np.zeros((B, T, Dx), np.float32), np.zeros((B, T, Dy), np.float32)
        z = np.zeros((B, T, nz), np.float32) if nz else None
        for b, (start, length, u) in enumerate(rows):
            length = min(int(length), T)
            sx = _scale_side(X_all[start:start + length], *xs, mistake, (Dx + 3) // 4 * 4)
            x[b, :length] = sx
            if recompute:
                ext = 1 if mistake == "delta_taps_cross_the_utterance_end" else 0      # one more frame of the CORPUS at the end
                ext = min(ext, len(Y_all) - (start + length))
                sy = _scale_side(Y_all[start:start + length + ext], *ys, mistake, (Dy + 3) // 4 * 4, rounded=False).astype(np.float64)
                y[b, :length] = D.recompute_delta_features(sy.copy(), None, None, hp.windows, hp.stream_sizes,
                                                           hp.has_dynamic_features)[:length].astype(np.float32)
            else:
                y[b, :length] = _scale_side(Y_all[start:start + length], *ys, mistake, (Dy + 3) // 4 * 4)
            if mistake == "padded_frames_hold_scale_of_zero" and length < T:
                x[b, length:] = _scale_side(np.zeros((1, Dx), np.float32), *xs, None, 0)
                y[b, length:] = _scale_side(np.zeros((1, Dy), np.float32), *ys, None, 0)
            if nz:
                z[b] = noise(key0, key1, int(u), T, nz)
                if mistake == "z_on_valid_frames_only":
                    z[b, length:] = 0
        lens = np.minimum(rows[:, 1], T).astype(np.int64)
        mask = (np.arange(T)[None, :] < lens[:, None]).astype(np.float32)[:, :, None]
        out.append(dict(x=x, y=y, y_static=np.ascontiguousarray(y[:, :, cols]), mask=mask, lengths=lens, z=z))
    return out
