"""Batch pipeline of the training loop (reference train.py:64-229, 494-524).

Host side (same names and on-disk format as the reference):

* ``NPYDataSource`` -- one float32 ``(T_i, D)`` ``.npy`` per utterance, sorted by file name; the last 5
  files are the real test set, the rest is split with ``train_test_split(test_size=0.112,
  random_state=1234)`` (train.py:64-93).
* ``FileSourceDataset`` / ``MemoryCacheDataset`` -- stand-ins for the two nnmnkwii dataset wrappers
  the reference imports (train.py:50-51; nnmnkwii is third-party and un-vendored).
* ``VCDataset`` / ``TTSDataset`` -- normalisation per utterance (train.py:96-135): mean/variance
  scaling of the acoustic side, min-max scaling to [0.01, 0.99] of the linguistic side, optional
  delta recomputation (gantts/multistream.py:15-30).
* ``collate_fn`` -- zero padding to the longest utterance of the batch (train.py:139-159; the
  reference's ``np.int`` no longer exists in numpy 2 -> int64 here).
* ``scale / inv_scale / minmax_scale_params / minmax_scale / meanvar / minmax / delta_features`` --
  the few nnmnkwii.preprocessing functions on this path, restated from their published definitions.

Device side (the part that matters at >10^6 frames/s): ``DevicePrefetcher`` wraps any iterable of
``(x, y, lengths)`` host batches and hands out batches that are already resident in HBM, sorted by
length (train.py:494-501) -- batch k+1 is staged into pinned memory and copied on a side stream
while step k runs on the compute stream, so the step never waits for PCIe.

Device-resident corpus (``hp.resident_corpus``): ``ResidentCorpus`` uploads the raw utterances once, ``ResidentLoader`` plans each epoch
on the host (``plan_epoch``), uploads one small table and produces every batch -- scaled, padded, sorted, with the generator's noise, the
static features and the mask -- by ONE launch (gt_op_assemble_batch), bit for bit what the host pipeline above computes.
``ResidentCorpus.from_arrays`` takes the raw utterances without statistics, ``corpus.minmax`` / ``corpus.meanvar`` compute them on the
device in one pass per side (gt_op_corpus_stats), and ``resident_tts_loaders`` / ``resident_vc_loaders`` go from the raw arrays to the
loaders (train.py:718-770) without host arithmetic on frames.
"""
import os
from os.path import join, splitext

import numpy as np
import torch

test_size = 0.112      # train.py:64 (1000 training utterances for cmu arctic)
random_state = 1234    # train.py:65


# ---- nnmnkwii.preprocessing (un-vendored third party), the functions train.py touches ------------
def scale(x, data_mean, data_std):
    return (x - data_mean) / data_std


def inv_scale(x, data_mean, data_std):
    return data_std * x + data_mean


def minmax_scale_params(data_min, data_max, feature_range=(0, 1)):
    data_range = data_max - data_min
    data_range = np.where(data_range == 0.0, 1.0, data_range)      # constant columns: scale 1
    scale_ = (feature_range[1] - feature_range[0]) / data_range
    min_ = feature_range[0] - data_min * scale_
    return min_, scale_


def minmax_scale(x, data_min=None, data_max=None, feature_range=(0, 1), scale_=None, min_=None):
    if scale_ is None or min_ is None:
        min_, scale_ = minmax_scale_params(data_min, data_max, feature_range)
    return x * scale_ + min_


def meanvar(dataset, lengths=None, mean_=0.0, var_=0.0, last_sample_count=0, return_last_sample_count=False):
    """Streaming mean / variance over all frames of a dataset of (T_i, D) arrays (Chan et al.
    pairwise update, the scheme sklearn's incremental mean/variance uses)."""
    n = float(last_sample_count)
    mean, m2 = np.asarray(mean_, dtype=np.float64), np.asarray(var_, dtype=np.float64) * n
    for idx in range(len(dataset)):
        x = np.asarray(dataset[idx], dtype=np.float64)
        if lengths is not None:
            x = x[:lengths[idx]]
        k = float(len(x))
        if k == 0:
            continue
        xm = x.mean(0)
        xv = ((x - xm) ** 2).sum(0)
        delta = xm - mean
        tot = n + k
        mean = mean + delta * (k / tot)
        m2 = m2 + xv + delta ** 2 * (n * k / tot)
        n = tot
    var = m2 / max(n, 1.0)
    if return_last_sample_count:
        return mean, var, int(n)
    return mean, var


def minmax(dataset, lengths=None):
    lo, hi = None, None
    for idx in range(len(dataset)):
        x = np.asarray(dataset[idx])
        if lengths is not None:
            x = x[:lengths[idx]]
        a, b = x.min(0), x.max(0)
        lo = a if lo is None else np.minimum(lo, a)
        hi = b if hi is None else np.maximum(hi, b)
    return lo, hi


def delta_features(x, windows):
    """[static | delta | delta-delta]: each window correlated along time with zeros beyond the edges."""
    T, D = x.shape
    out = np.empty((T, D * len(windows)), dtype=x.dtype)
    for i, (_, _, coef) in enumerate(windows):
        coef = np.asarray(coef, dtype=x.dtype)
        for d in range(D):
            out[:, i * D + d] = np.correlate(x[:, d], coef, mode="same")
    return out


def recompute_delta_features(Y, Y_data_mean, Y_data_std, windows, stream_sizes=[180, 3, 1, 3],
                             has_dynamic_features=[True, True, False, True]):
    """gantts/multistream.py:15-30: rebuilds the dynamic columns of every dynamic stream from its
    (already normalised) static columns, in place.  The statistics arguments are unused there too."""
    from .multistream import get_static_stream_sizes
    starts = np.hstack(([0], np.cumsum(stream_sizes)[:-1]))
    ends = np.cumsum(stream_sizes)
    statics = get_static_stream_sizes(stream_sizes, has_dynamic_features, len(windows))
    for s, e, n, dyn in zip(starts, ends, statics, has_dynamic_features):
        if dyn:
            Y[:, s:e] = delta_features(Y[:, s:s + int(n)], windows)
    return Y


# ---- datasets ---------------------------------------------------------------------------------
class NPYDataSource(object):
    """train.py:71-93"""

    def __init__(self, dirname, train=True, max_files=None, test=False):
        self.dirname, self.train, self.test, self.max_files = dirname, train, test, max_files

    def collect_files(self):
        from sklearn.model_selection import train_test_split
        npy_files = sorted(join(self.dirname, f) for f in os.listdir(self.dirname) if splitext(f)[-1] == ".npy")
        if self.test:                                  # last 5 is for real testset
            return npy_files[len(npy_files) - 5:]
        npy_files = npy_files[:len(npy_files) - 5]
        if self.max_files is not None and self.max_files > 0:
            npy_files = npy_files[:self.max_files]
        train_files, test_files = train_test_split(npy_files, test_size=test_size, random_state=random_state)
        return train_files if self.train else test_files

    def collect_features(self, path):
        return np.load(path)


class FileSourceDataset(object):
    """Lazy list of per-utterance arrays behind a data source (nnmnkwii.datasets.FileSourceDataset)."""

    def __init__(self, file_data_source):
        self.file_data_source = file_data_source
        self.collected_files = list(file_data_source.collect_files())

    def __getitem__(self, idx):
        if isinstance(idx, slice):
            return [self[i] for i in range(*idx.indices(len(self)))]
        return self.file_data_source.collect_features(self.collected_files[idx])

    def __len__(self):
        return len(self.collected_files)


class MemoryCacheDataset(object):
    """Keeps up to ``cache_size`` loaded utterances (nnmnkwii.datasets.MemoryCacheDataset)."""

    def __init__(self, dataset, cache_size=777):
        self.dataset, self.cache_size = dataset, cache_size
        self.cached = {}

    def __getitem__(self, idx):
        if idx not in self.cached:
            if len(self.cached) >= self.cache_size:
                self.cached.pop(next(iter(self.cached)))       # oldest first
            self.cached[idx] = self.dataset[idx]
        return self.cached[idx]

    def __len__(self):
        return len(self.dataset)


class VCDataset(object):
    """train.py:96-108"""

    def __init__(self, X, Y, data_mean, data_std):
        self.X, self.Y, self.data_mean, self.data_std = X, Y, data_mean, data_std

    def __getitem__(self, idx):
        return scale(self.X[idx], self.data_mean, self.data_std), scale(self.Y[idx], self.data_mean, self.data_std)

    def __len__(self):
        return len(self.X)


class TTSDataset(object):
    """train.py:111-135.  ``hp`` (module-global in the reference) is passed in."""

    def __init__(self, X, Y, X_data_min, X_data_max, Y_data_mean, Y_data_std, hp=None):
        self.X, self.Y = X, Y
        self.X_data_min, self.X_data_scale = minmax_scale_params(X_data_min, X_data_max, feature_range=(0.01, 0.99))
        self.Y_data_mean, self.Y_data_std = Y_data_mean, Y_data_std
        self.hp = hp

    def __getitem__(self, idx):
        x = minmax_scale(self.X[idx], min_=self.X_data_min, scale_=self.X_data_scale, feature_range=(0.01, 0.99))
        y = scale(self.Y[idx], self.Y_data_mean, self.Y_data_std)
        hp = self.hp
        if hp is not None and getattr(hp, "recompute_delta_features", False):
            y = recompute_delta_features(y, self.Y_data_mean, self.Y_data_std, hp.windows, hp.stream_sizes,
                                         hp.has_dynamic_features)
        return x, y

    def __len__(self):
        return len(self.X)


def _pad_2d(x, max_len):
    return np.pad(x, [(0, max_len - len(x)), (0, 0)], mode="constant", constant_values=0)


def collate_fn(batch):
    """train.py:145-159: ``(x_batch (B,T,Din) f32, y_batch (B,T,Dout) f32, lengths (B,) int64)``."""
    input_lengths = np.array([len(x[0]) for x in batch], dtype=np.int64)
    max_len = int(np.max(input_lengths))
    x_batch = np.array([_pad_2d(x[0], max_len) for x in batch], dtype=np.float32)
    y_batch = np.array([_pad_2d(x[1], max_len) for x in batch], dtype=np.float32)
    return torch.from_numpy(x_batch), torch.from_numpy(y_batch), torch.from_numpy(input_lengths)


def collate_ragged(batch):
    """Device-side collate (``DevicePrefetcher`` pads and sorts on the GPU, gt_op_pad_sequences): the utterances of the batch
    un-padded, back to back -- ``(x_cat (sum T_i, Din) f32, y_cat (sum T_i, Dout) f32, lengths (B,) int64)`` -- so that neither
    the padded copy is made on the host nor its padding crosses PCIe (a batch of real utterances is 30-50 % padding)."""
    input_lengths = np.array([len(x[0]) for x in batch], dtype=np.int64)
    x_cat = np.concatenate([np.asarray(x[0], dtype=np.float32) for x in batch], axis=0)
    y_cat = np.concatenate([np.asarray(x[1], dtype=np.float32) for x in batch], axis=0)
    return torch.from_numpy(x_cat), torch.from_numpy(y_cat), torch.from_numpy(input_lengths)


def _loaders(train_dataset, test_dataset, hp):
    from torch.utils import data as data_utils
    if bool(getattr(hp, "resident_corpus", False)):              # gantts_amd extension: the corpus lives on the device (ResidentLoader)
        return {"train": ResidentLoader(train_dataset, hp.batch_size, True, hp),
                "test": ResidentLoader(test_dataset, hp.batch_size, False, hp, first_draw=1 << 31)}
    ragged = bool(getattr(hp, "device_collate", False))          # gantts_amd extension: pad + sort on the device
    kw = dict(batch_size=hp.batch_size, num_workers=hp.num_workers, pin_memory=hp.pin_memory,
              collate_fn=collate_ragged if ragged else collate_fn)
    return {"train": data_utils.DataLoader(train_dataset, shuffle=True, **kw),
            "test": data_utils.DataLoader(test_dataset, shuffle=False, **kw)}


def get_vc_data_loaders(X, Y, data_mean, data_std, hp):
    """train.py:174-200 (the reference has a ``data_var``/``data_std`` name slip at :174/:182; std is meant)."""
    mk = lambda ph: VCDataset(MemoryCacheDataset(X[ph], cache_size=hp.cache_size),
                              MemoryCacheDataset(Y[ph], cache_size=hp.cache_size), data_mean, data_std)
    return _loaders(mk("train"), mk("test"), hp)


def get_tts_data_loaders(X, Y, X_data_min, X_data_max, Y_data_mean, Y_data_std, hp):
    """train.py:203-229"""
    mk = lambda ph: TTSDataset(MemoryCacheDataset(X[ph], cache_size=hp.cache_size),
                               MemoryCacheDataset(Y[ph], cache_size=hp.cache_size),
                               X_data_min, X_data_max, Y_data_mean, Y_data_std, hp=hp)
    return _loaders(mk("train"), mk("test"), hp)


# ---- device side --------------------------------------------------------------------------------
class DeviceBatch(object):
    """One length-sorted batch resident on the device (what train_loop consumes per step)."""
    __slots__ = ("x", "y", "lengths", "cpu_lengths", "max_len", "ready", "generator_input", "y_static", "mask", "tv_global")

    def __init__(self, x, y, lengths, cpu_lengths, ready, generator_input=None, y_static=None, mask=None, tv_global=None, max_len=None):
        self.x, self.y, self.lengths, self.cpu_lengths = x, y, lengths, cpu_lengths
        # max_len: the T the batch is padded to where that is not its own longest sequence -- a data-parallel rank's share of a batch is
        # padded to the WHOLE batch's longest sequence, which may live on another rank
        self.max_len = int(max_len) if max_len is not None else (int(cpu_lengths[0]) if len(cpu_lengths) else 0)
        # tv_global: the valid frames of the WHOLE batch as a 1-element float64 device tensor (a sharded ResidentLoader; the loss
        # normaliser of the data-parallel step), None where the batch is the whole batch
        self.tv_global = tv_global
        self.ready = ready
        # what train_loop derives from (x, y, lengths) per batch, when the loader has made it already (ResidentLoader): [x | z] with
        # x its prefix view, get_static_features(y), sequence_mask(lengths).unsqueeze(-1); None: train_loop derives it
        self.generator_input, self.y_static, self.mask = generator_input, y_static, mask


class DevicePrefetcher(object):
    """Iterates ``loader`` one batch ahead: sorts by length (descending -- what torch.sort gives the reference at
    train.py:495-501), trims the padding to the longest sequence, stages the batch in pinned host buffers and copies it on a
    dedicated stream; ``__next__`` makes the compute stream wait on that copy's event (no host sync).  With a
    ``collate_ragged`` loader (``hp.device_collate``) only the valid frames are staged and copied, and the padding and the
    sort happen on the device (gt_op_pad_sequences): device-side collate."""

    def __init__(self, loader, device="cuda", depth=2, pitch_x=False):
        """pitch_x: stage x with a row pitch that is a multiple of 4 floats (a (B, T, D) view over a (B, T, P) device buffer,
        ``gantts_amd.engine.pitched_empty``): the engine then reads the batch's rows with 16-byte loads in every product
        (gt_set_x_pitch) instead of making that copy itself once per step.  Free here -- the batch is being copied anyway."""
        self.loader, self.device, self.depth = loader, torch.device(device), max(1, int(depth))
        self.pitch_x = bool(pitch_x)
        self.copy_stream = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" else None
        self._pinned, self._slot_copied = {}, {}

    def __len__(self):
        return len(self.loader)

    def _pin(self, key, t):
        buf = self._pinned.get(key)
        if buf is None or buf.numel() < t.numel() or buf.dtype != t.dtype:
            buf = torch.empty(t.numel(), dtype=t.dtype).pin_memory() if self.copy_stream is not None else torch.empty(t.numel(), dtype=t.dtype)
            self._pinned[key] = buf
        v = buf[:t.numel()].view(t.shape)
        v.copy_(t)
        return v

    def _stage_ragged(self, slot, batch):
        """A ``collate_ragged`` batch: H2D of the valid frames only, then padding + the length sort on the device
        (gt_op_pad_sequences).  The ORDER is the reference's own: torch.sort(lengths, descending=True) (train.py:495)."""
        from . import _lib as L
        x, y, lengths = batch
        lengths = torch.as_tensor(lengths).view(-1).long()
        sorted_lengths, indices = torch.sort(lengths, dim=0, descending=True)
        B, max_len = int(lengths.numel()), int(sorted_lengths[0])
        starts = (torch.cumsum(lengths, 0) - lengths)[indices].contiguous()
        cpu_lengths = [int(v) for v in sorted_lengths.tolist()]
        prev = self._slot_copied.get(slot)
        if prev is not None:
            prev.synchronize()
        hx, hy = self._pin((slot, "x"), x.contiguous()), self._pin((slot, "y"), y.contiguous())
        hm = self._pin((slot, "meta"), torch.stack((starts, sorted_lengths)))
        Dx, Dy = x.size(-1), y.size(-1)
        with torch.cuda.stream(self.copy_stream):
            rx, ry = hx.to(self.device, non_blocking=True), hy.to(self.device, non_blocking=True)
            meta = hm.to(self.device, non_blocking=True)
            ldx = (Dx + 3) // 4 * 4 if self.pitch_x else Dx
            bx = torch.empty(B, max_len, ldx, device=self.device, dtype=torch.float32)
            dy = torch.empty(B, max_len, Dy, device=self.device, dtype=torch.float32)
            st = L.current_stream()
            L.check(L.lib.gt_op_pad_sequences(L.ptr(rx), Dx, L.ptr(meta[0]), L.ptr(meta[1]), B, max_len, L.ptr(bx), ldx, st))
            L.check(L.lib.gt_op_pad_sequences(L.ptr(ry), Dy, L.ptr(meta[0]), L.ptr(meta[1]), B, max_len, L.ptr(dy), Dy, st))
            dx = bx[:, :, :Dx] if ldx != Dx else bx
            dl = meta[1]
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        for t in (rx, ry, meta):
            t.record_stream(self.copy_stream)
        self._slot_copied[slot] = ev
        return DeviceBatch(dx, dy, dl, cpu_lengths, ev)

    def _stage(self, slot, batch):
        x, y, lengths = batch
        if x.dim() == 2 and self.copy_stream is not None:
            return self._stage_ragged(slot, batch)
        if x.dim() == 2:         # no device: pad on the host (CPU tests of the loop logic)
            lens = [int(v) for v in torch.as_tensor(lengths).view(-1).tolist()]
            offs = np.concatenate(([0], np.cumsum(lens)))
            T_ = max(lens)
            x = torch.stack([torch.from_numpy(_pad_2d(x[offs[i]:offs[i + 1]].numpy(), T_)) for i in range(len(lens))])
            y = torch.stack([torch.from_numpy(_pad_2d(y[offs[i]:offs[i + 1]].numpy(), T_)) for i in range(len(lens))])
        lengths = torch.as_tensor(lengths).view(-1).long()
        sorted_lengths, indices = torch.sort(lengths, dim=0, descending=True)
        max_len = int(sorted_lengths[0])
        x, y = x[indices][:, :max_len], y[indices][:, :max_len]
        cpu_lengths = [int(v) for v in sorted_lengths.tolist()]
        if self.copy_stream is None:
            return DeviceBatch(x.contiguous(), y.contiguous(), sorted_lengths, cpu_lengths, None)
        prev = self._slot_copied.get(slot)
        if prev is not None:
            prev.synchronize()          # the slot's previous H2D must have drained before the host overwrites it
        if self.pitch_x and x.size(-1) % 4:
            xp = x.new_zeros(x.size(0), x.size(1), (x.size(-1) + 3) // 4 * 4)
            xp[:, :, :x.size(-1)] = x
            x_host, width = xp, x.size(-1)
        else:
            x_host, width = x.contiguous(), None
        hx, hy = self._pin((slot, "x"), x_host), self._pin((slot, "y"), y.contiguous())
        with torch.cuda.stream(self.copy_stream):
            dx = hx.to(self.device, non_blocking=True)
            if width is not None:
                dx = dx[:, :, :width]             # the pitched view the engine takes as it is
            dy = hy.to(self.device, non_blocking=True)
            dl = sorted_lengths.to(self.device)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        self._slot_copied[slot] = ev
        return DeviceBatch(dx, dy, dl, cpu_lengths, ev)

    def __iter__(self):
        it = iter(self.loader)
        queue, slot = [], 0
        for batch in it:
            if self.copy_stream is not None and len(queue) >= self.depth:
                out = queue.pop(0)
                yield self._release(out)
            queue.append(self._stage(slot % (self.depth + 1), batch))
            slot += 1
            if self.copy_stream is None:
                yield self._release(queue.pop(0))
        while queue:
            yield self._release(queue.pop(0))

    def _release(self, b):
        if b.ready is not None:
            torch.cuda.current_stream(self.device).wait_event(b.ready)
            for t in (b.x, b.y, b.lengths):
                t.record_stream(torch.cuda.current_stream(self.device))
        return b


# ---- device-resident corpus ---------------------------------------------------------------------
RESIDENT_MARGIN_BYTES = 2 << 30      # device memory a resident corpus leaves free: the step's workspaces, the batches, the allocator's slack


def plan_epoch(offsets, lengths, batches):
    """Host plan of one epoch of a resident corpus (no device): ``(table, plan)``.  ``batches`` is an iterable of lists of corpus
    utterance indices.  ``table`` is the int64 ``[n_slots][3]`` array gt_op_assemble_batch reads -- first frame, length and utterance
    index of every batch slot, batches back to back, each batch in the order ``torch.sort(lengths, descending=True)`` gives it (the
    call DevicePrefetcher makes, train.py:495, so ties fall the same way); ``plan`` has one ``(first_slot, B, T, sorted lengths)``
    per batch."""
    rows, plan = [], []
    for idx in batches:
        idx = [int(i) for i in idx]
        if not idx:
            continue
        lens = torch.from_numpy(np.array([lengths[i] for i in idx], dtype=np.int64))
        sorted_lengths, indices = torch.sort(lens, dim=0, descending=True)
        cpu_lengths = [int(v) for v in sorted_lengths.tolist()]
        plan.append((len(rows), len(idx), cpu_lengths[0], cpu_lengths))
        for k in indices.tolist():
            u = idx[k]
            rows.append((int(offsets[u]), int(lengths[u]), u))
    return np.array(rows, dtype=np.int64).reshape(-1, 3), plan


def shard_plan(plan, rank, world, short_batch="error"):
    """One data-parallel rank's share of an epoch planned by ``plan_epoch`` (no device): per batch ``(first_slot, B_global, B_local, T,
    local lengths)``.  Whole sequences are dealt round-robin -- local sequence b of rank r is sequence r + world * b of the length-sorted
    batch, so the local lengths are ``lengths[rank::world]`` -- and ``T`` stays the WHOLE batch's longest sequence on every rank.

    A batch with fewer sequences than ranks cannot give every rank one; the last batch of an epoch (the loader's ``drop_last=False``) is
    the usual case.  ``short_batch="error"`` raises ValueError for it -- at plan time, on every rank alike --, ``short_batch="drop"``
    leaves it out on every rank."""
    rank, world = int(rank), int(world)
    if world < 1 or not 0 <= rank < world:
        raise ValueError("shard_plan: rank %d of a world of %d" % (rank, world))
    if short_batch not in ("error", "drop"):
        raise ValueError("shard_plan: short_batch is \"error\" or \"drop\", not %r" % (short_batch,))
    out = []
    for k, (first, B, T, cpu_lengths) in enumerate(plan):
        if B < world:
            if short_batch == "error":
                raise ValueError("shard_plan: batch %d has %d sequences for a world of %d ranks; every rank needs one "
                                 "(short_batch=\"drop\" leaves such a batch out)" % (k, B, world))
            continue
        local = list(cpu_lengths[rank::world])
        out.append((first, B, len(local), T, local))
    return out


def _stat_vector(v, D, name):
    v = np.asarray(v)
    if v.dtype not in (np.float32, np.float64):
        raise TypeError("ResidentCorpus: %s is %s; float32 or float64 statistics only" % (name, v.dtype))
    return np.ascontiguousarray(np.broadcast_to(v, (D,)))


def _fill_chunks(arrays, buf, D):
    """Packs the rows of ``arrays`` back to back into columns ``[0, D)`` of the staging buffer ``buf (chunk, ld)`` and yields the
    number of rows filled each time the buffer is full, and once more for the rest."""
    chunk, filled = buf.size(0), 0
    for a in arrays:
        pos = 0
        while pos < len(a):
            k = min(len(a) - pos, chunk - filled)
            buf[filled:filled + k, :D] = torch.from_numpy(np.ascontiguousarray(a[pos:pos + k]))
            filled, pos = filled + k, pos + k
            if filled == chunk:
                yield filled
                filled = 0
    if filled:
        yield filled


class ResidentCorpus(object):
    """The raw utterances of a ``TTSDataset`` / ``VCDataset`` on the device: ``X_all [F][ldX]``, ``Y_all [F][ldY]`` float32, back to
    back on a 16-byte row pitch, with the dataset's statistics beside them in their own dtype.  Every utterance is read once
    (``dataset.X[i]``, ``dataset.Y[i]``) and held on the host until ``upload`` has sent it in chunks through one pinned staging
    buffer.  A corpus that does not fit ``torch.cuda.mem_get_info()`` minus ``RESIDENT_MARGIN_BYTES`` is refused (RuntimeError)
    before anything is allocated: there is no fallback to the host pipeline."""

    def __init__(self, dataset, device="cuda", chunk_frames=1 << 16):
        n = len(dataset)
        if n < 1:
            raise ValueError("ResidentCorpus: empty dataset")
        self.chunk_frames = int(chunk_frames)
        self._take((dataset.X[i], dataset.Y[i]) for i in range(n))
        self._attach(dataset)
        if device is not None:
            self.upload(device)

    @classmethod
    def from_arrays(cls, X, Y, device="cuda", chunk_frames=1 << 16):
        """A corpus of the raw utterances ``X[i]``, ``Y[i]`` (``(T_i, D)`` float32) that carries no statistics yet: the same validation,
        refusal and upload as ``ResidentCorpus(dataset)``.  ``minmax`` / ``meanvar`` compute the statistics on the device; a
        ``ResidentLoader`` takes the corpus once ``attach_statistics(dataset)`` has named the dataset that carries them."""
        n = len(X)
        if n < 1:
            raise ValueError("ResidentCorpus: empty dataset")
        if len(Y) != n:
            raise ValueError("ResidentCorpus: %d input and %d output utterances" % (n, len(Y)))
        self = cls.__new__(cls)
        self.chunk_frames = int(chunk_frames)
        self._take((X[i], Y[i]) for i in range(n))
        self.dataset = self._stats_host = None
        self.x_kind = self.y_kind = self.stats_f64 = None
        self.windows, self.dsrc_host, self.dwin_host = None, None, None
        if device is not None:
            self.upload(device)
        return self

    def _take(self, pairs):
        """Validates the utterances and lays the corpus out (host side): lengths, offsets, widths, pitches."""
        self._host = []
        for i, (x, y) in enumerate(pairs):
            x, y = np.asarray(x), np.asarray(y)
            if x.dtype != np.float32 or y.dtype != np.float32 or x.ndim != 2 or y.ndim != 2:
                raise TypeError("ResidentCorpus: utterance %d is %s %s / %s %s; (T, D) float32 arrays only" % (i, x.dtype, x.shape, y.dtype, y.shape))
            if len(x) != len(y):
                raise ValueError("ResidentCorpus: utterance %d has %d input and %d output frames" % (i, len(x), len(y)))
            self._host.append((x, y))
        self.Dx, self.Dy = int(self._host[0][0].shape[1]), int(self._host[0][1].shape[1])
        if any(x.shape[1] != self.Dx or y.shape[1] != self.Dy for x, y in self._host):
            raise ValueError("ResidentCorpus: the utterances differ in width")
        self.lengths = np.array([len(x) for x, _ in self._host], dtype=np.int64)
        self.offsets = np.cumsum(self.lengths) - self.lengths
        self.F = int(self.lengths.sum())
        self.ldX, self.ldY = (self.Dx + 3) // 4 * 4, (self.Dy + 3) // 4 * 4
        self.nbytes = self.F * (self.ldX + self.ldY) * 4
        self.X_all = self.Y_all = self.stats = self.dsrc = self.dwin = None
        self._stats_ws = None

    def _attach(self, dataset):
        """The normalisation each ``dataset.__getitem__`` applies (train.py:96-135), as (kind, a, b) per side, and its delta plan."""
        from . import _lib as L
        self.dataset = dataset
        if hasattr(dataset, "X_data_scale"):         # TTSDataset: min-max x, mean-variance y
            self.x_kind, xa, xb = L.SCALE_MINMAX, dataset.X_data_scale, dataset.X_data_min
            self.y_kind, ya, yb = L.SCALE_MEANVAR, dataset.Y_data_mean, dataset.Y_data_std
        elif hasattr(dataset, "data_mean"):          # VCDataset: the same mean-variance on both sides
            if self.Dx != self.Dy:
                raise ValueError("ResidentCorpus: a VCDataset scales both sides with one set of statistics; widths %d / %d" % (self.Dx, self.Dy))
            self.x_kind, xa, xb = L.SCALE_MEANVAR, dataset.data_mean, dataset.data_std
            self.y_kind, ya, yb = L.SCALE_MEANVAR, dataset.data_mean, dataset.data_std
        else:
            raise TypeError("ResidentCorpus: a TTSDataset or a VCDataset, not %s" % type(dataset).__name__)
        self._stats_host = [_stat_vector(xa, self.Dx, "x statistics"), _stat_vector(xb, self.Dx, "x statistics"),
                            _stat_vector(ya, self.Dy, "y statistics"), _stat_vector(yb, self.Dy, "y statistics")]
        for a, b in (self._stats_host[:2], self._stats_host[2:]):
            if a.dtype != b.dtype:       # numpy would compute the first operation in one dtype and the second in the other
                raise TypeError("ResidentCorpus: the two statistics of one side must share a dtype (%s / %s)" % (a.dtype, b.dtype))
        self.stats_f64 = int(self._stats_host[0].dtype == np.float64) | (int(self._stats_host[2].dtype == np.float64) << 1)
        # delta recomputation of a TTSDataset (gantts/multistream.py:15-30): per column of y its source column and window
        self.windows, self.dsrc_host, self.dwin_host = None, None, None
        dhp = getattr(dataset, "hp", None)
        if hasattr(dataset, "X_data_scale") and dhp is not None and getattr(dhp, "recompute_delta_features", False):
            self._plan_deltas(dhp)

    def attach_statistics(self, dataset):
        """Names the ``TTSDataset`` / ``VCDataset`` over this corpus' utterances whose statistics the batches are scaled with (a corpus
        made by ``from_arrays``); the raw frames stay where they are -- nothing is uploaded again but the statistics themselves."""
        if self.dataset is not None:
            raise ValueError("ResidentCorpus: statistics are attached already")
        if len(dataset) != len(self.lengths):
            raise ValueError("ResidentCorpus: a dataset of %d utterances for a corpus of %d" % (len(dataset), len(self.lengths)))
        self._attach(dataset)
        if self.X_all is not None:
            self._upload_stats(self.device)
        return self

    def _plan_deltas(self, hp):
        from . import _lib as L
        from .multistream import get_static_stream_sizes
        windows = [np.asarray(c, dtype=np.float64) for _, _, c in hp.windows]
        if len(windows) > L.ASSEMBLE_MAX_WINDOWS or any(len(c) % 2 == 0 or len(c) > L.ASSEMBLE_MAX_TAPS for c in windows):
            raise ValueError("ResidentCorpus: delta recomputation takes at most %d windows of an odd number of at most %d taps"
                             % (L.ASSEMBLE_MAX_WINDOWS, L.ASSEMBLE_MAX_TAPS))
        if int(self.lengths.min()) < max(len(c) for c in windows):
            raise ValueError("ResidentCorpus: an utterance is shorter than the longest window; the host pipeline "
                             "(np.correlate(..., 'same')) cannot recompute its deltas either")
        if sum(hp.stream_sizes) != self.Dy:
            raise ValueError("ResidentCorpus: stream sizes %s for %d output columns" % (list(hp.stream_sizes), self.Dy))
        dsrc, dwin = np.arange(self.Dy, dtype=np.int32), np.full(self.Dy, -1, dtype=np.int32)
        statics = get_static_stream_sizes(hp.stream_sizes, hp.has_dynamic_features, len(windows))
        start = 0
        for size, n, dyn in zip(hp.stream_sizes, statics, hp.has_dynamic_features):
            n = int(n)
            if dyn:
                if n * len(windows) != size:
                    raise ValueError("ResidentCorpus: a dynamic stream of %d columns does not hold %d windows" % (size, len(windows)))
                for w in range(len(windows)):
                    dsrc[start + w * n:start + (w + 1) * n] = np.arange(start, start + n)
                    dwin[start + w * n:start + (w + 1) * n] = w
            start += size
        self.windows, self.dsrc_host, self.dwin_host = windows, dsrc, dwin

    def upload(self, device="cuda"):
        if self.X_all is not None:
            return self
        device = torch.device(device)
        free, total = torch.cuda.mem_get_info(device)
        if self.nbytes > free - RESIDENT_MARGIN_BYTES:
            raise RuntimeError("ResidentCorpus: %d frames x (%d + %d) floats = %d bytes do not fit the device: %d bytes free of %d, "
                               "of which %d stay free as margin" % (self.F, self.ldX, self.ldY, self.nbytes, free, total, RESIDENT_MARGIN_BYTES))
        X_all = torch.empty(self.F, self.ldX, device=device, dtype=torch.float32)
        Y_all = torch.empty(self.F, self.ldY, device=device, dtype=torch.float32)
        chunk = max(1, min(self.chunk_frames, self.F))
        stage = torch.zeros(chunk * max(self.ldX, self.ldY), dtype=torch.float32).pin_memory()
        for side, (dst, D, ld) in enumerate(((X_all, self.Dx, self.ldX), (Y_all, self.Dy, self.ldY))):
            buf = stage[:chunk * ld].view(chunk, ld)
            buf.zero_()                                              # the pad columns
            sent = 0
            for filled in _fill_chunks([h[side] for h in self._host], buf, D):
                dst[sent:sent + filled].copy_(buf[:filled], non_blocking=True)
                torch.cuda.current_stream(device).synchronize()      # one staging buffer: drained before it is refilled
                sent += filled
        if self._stats_host is not None:
            self._upload_stats(device)
        self.X_all, self.Y_all, self.device = X_all, Y_all, device
        self._host = None
        return self

    def _upload_stats(self, device):
        self.stats = [torch.from_numpy(v.copy()).to(device) for v in self._stats_host]
        if self.dsrc_host is not None:
            self.dsrc, self.dwin = torch.from_numpy(self.dsrc_host).to(device), torch.from_numpy(self.dwin_host).to(device)

    # ---- statistics on the device (gt_op_corpus_stats) ------------------------------------------------------------------------------
    def segments(self, lengths=None):
        """The valid rows as gt_op_corpus_stats reads them: int64 ``[n][2]`` = (first frame, valid frame count) per utterance, utterance
        ``idx`` cut to ``lengths[idx]`` as ``x[:lengths[idx]]`` cuts it on the host (a negative length counts from the end)."""
        n = len(self.lengths)
        valid = self.lengths.copy()
        if lengths is not None:
            valid = np.array([len(range(*slice(None, int(lengths[i])).indices(int(self.lengths[i])))) for i in range(n)], dtype=np.int64)
        return np.ascontiguousarray(np.stack((self.offsets, valid), axis=1).astype(np.int64))

    def stats_case(self, side, lengths=None, prior_mean=0.0, prior_var=0.0, prior_count=0):
        """The ``gt_corpus_stats_case`` of one pass over side "x" or "y" and its result buffers ``(out_f (2, D) float32: min, max;
        out_d (3, D) float64: count, mean, M2)``; the case keeps the device buffers it points to alive."""
        from . import _lib as L
        if side not in ("x", "y"):
            raise ValueError("ResidentCorpus: side is \"x\" or \"y\", not %r" % (side,))
        if self.X_all is None:
            raise RuntimeError("ResidentCorpus: the corpus is not on the device; upload() it first (the statistics have no host path here)")
        A, D, ld = (self.X_all, self.Dx, self.ldX) if side == "x" else (self.Y_all, self.Dy, self.ldY)
        dev = self.device
        seg = torch.from_numpy(self.segments(lengths)).to(dev)
        nbytes = int(L.lib.gt_corpus_stats_workspace_bytes(self.F, D))
        if self._stats_ws is None or self._stats_ws.numel() * 8 < nbytes:
            self._stats_ws = torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.float64)
        out_f, out_d = torch.empty(2, D, device=dev, dtype=torch.float32), torch.empty(3, D, device=dev, dtype=torch.float64)
        k = L.CorpusStatsCase()
        k.D, k.ld, k.F, k.n_seg, k.prior_count = D, ld, self.F, len(seg), int(prior_count)
        k.A, k.seg = A.data_ptr(), seg.data_ptr()
        prior = None
        if int(prior_count) > 0 or np.any(np.asarray(prior_mean) != 0.0):
            prior = torch.from_numpy(np.stack([np.broadcast_to(np.asarray(v, dtype=np.float64), (D,)) for v in (prior_mean, prior_var)])).to(dev)
            k.prior_mean, k.prior_var = prior[0].data_ptr(), prior[1].data_ptr()
        k.workspace, k.workspace_bytes = self._stats_ws.data_ptr(), self._stats_ws.numel() * 8
        k.out_min, k.out_max = out_f[0].data_ptr(), out_f[1].data_ptr()
        k.out_count, k.out_mean, k.out_m2 = out_d[0].data_ptr(), out_d[1].data_ptr(), out_d[2].data_ptr()
        k._alive = (seg, prior, self._stats_ws, out_f, out_d)
        return k, out_f, out_d

    def _device_stats(self, side, lengths, prior_mean, prior_var, prior_count):
        """One gt_op_corpus_stats pass over side "x" or "y": ``(min, max, count, mean, M2)`` as numpy arrays of shape ``(D,)``."""
        import ctypes as C
        from . import _lib as L
        k, out_f, out_d = self.stats_case(side, lengths, prior_mean, prior_var, prior_count)
        with torch.cuda.device(self.device):
            L.check(L.lib.gt_op_corpus_stats(C.byref(k), L.current_stream()))
            f, d = out_f.cpu().numpy(), out_d.cpu().numpy()      # the read-back waits for the two launches
        return f[0], f[1], d[0], d[1], d[2]

    def minmax(self, side, lengths=None):
        """``data.minmax`` of side "x" or "y" on the device: ``(lo, hi)`` float32 ``(D,)``; a NaN makes its column NaN, as numpy's."""
        lo, hi, count, _, _ = self._device_stats(side, lengths, 0.0, 0.0, 0)
        if count[0] == 0:
            raise ValueError("ResidentCorpus.minmax: no frame selected (numpy's min of an empty array has no identity either)")
        return lo, hi

    def meanvar(self, side, lengths=None, mean_=0.0, var_=0.0, last_sample_count=0, return_last_sample_count=False):
        """``data.meanvar`` of side "x" or "y" on the device, the host's signature: float64 ``(mean, var[, n])`` with
        ``var = M2 / max(n, 1)``, continued from ``(mean_, var_, last_sample_count)``; an empty selection returns that prior."""
        _, _, count, mean, m2 = self._device_stats(side, lengths, mean_, var_, last_sample_count)
        n = float(count[0])
        var = m2 / max(n, 1.0)
        if return_last_sample_count:
            return mean, var, int(n)
        return mean, var


class ResidentLoader(object):
    """Batches of a device-resident corpus (``hp.resident_corpus``): the raw corpus is uploaded once (``ResidentCorpus``), each epoch
    uploads one small table (``plan_epoch``), and every batch is ONE gt_op_assemble_batch launch on the current stream -- scaling,
    padding, the length sort, the generator's noise and its concatenation, the static features and the mask, bit for bit what
    ``DevicePrefetcher(DataLoader(dataset))`` + train_loop compute on the host and in launches of their own.  No host copy, host
    arithmetic on frames or synchronisation per batch.  Yields ``DeviceBatch``es with ``generator_input``, ``y_static`` and ``mask``
    set; ``x`` is the prefix view ``generator_input[:, :, :Dx]``.

    Noise: Philox4x32-10 keyed by (``hp.generator_noise_seed`` low word, draw counter); the draw counter starts at ``first_draw`` and
    advances once per epoch (per ``__iter__``); the counters are (corpus utterance index, t * ceil(nz / 4) + column group of 4), so a
    frame's noise depends on its utterance, not on the utterance's place in the batch (data_kernels.hip.h).

    Data parallelism (``world > 1``): every rank holds the whole corpus and plans the whole epoch; rank ``rank`` assembles sequences
    ``rank::world`` of each length-sorted batch (``shard_plan``), padded to the WHOLE batch's T, through gt_op_assemble_shard, whose
    launch also writes the whole batch's valid-frame count (``DeviceBatch.tv_global``, the step's loss normaliser -- no collective for
    it).  The ranks' rows are the rows of the one-process batch, noise included.  EVERY RANK MUST PLAN THE SAME EPOCH: the loader's own
    shuffling then draws from a private ``torch.Generator`` seeded with ``hp.shard_sampler_seed`` (default ``hp.generator_noise_seed``),
    whose state advances from epoch to epoch identically on all ranks; a caller's ``batch_sampler`` must be rank-identical itself.
    ``last_table_crc`` (zlib.crc32 of the epoch table's bytes) lets a driver enforce it (``parallel.resident_epoch`` does).
    ``short_batch``: see ``shard_plan``.  With ``world == 1`` nothing changes."""

    def __init__(self, dataset, batch_size, shuffle, hp, batch_sampler=None, device="cuda", first_draw=0, rank=0, world=1, short_batch="error"):
        from torch.utils import data as data_utils
        from .multistream import static_columns
        self.dataset, self.hp, self.device = dataset, hp, device
        self.corpus = dataset if isinstance(dataset, ResidentCorpus) else ResidentCorpus(dataset, device=None)
        if isinstance(dataset, ResidentCorpus):
            if dataset.dataset is None:
                raise ValueError("ResidentLoader: this corpus was made from raw arrays and has no statistics attached yet; compute them "
                                 "(corpus.minmax / corpus.meanvar) and call corpus.attach_statistics(dataset) first")
            self.dataset = dataset.dataset
        self.rank, self.world, self.short_batch = int(rank), int(world), short_batch
        shard_plan([], self.rank, self.world, short_batch)       # the argument checks
        self.last_table_crc = None
        n = len(self.corpus.lengths)
        self._short_last = False       # the loader's own last batch is shorter than the world and is dropped
        if batch_sampler is None:
            if shuffle and self.world > 1:
                g = torch.Generator()
                g.manual_seed(int(getattr(hp, "shard_sampler_seed", getattr(hp, "generator_noise_seed", 0))))
                sampler = data_utils.RandomSampler(range(n), generator=g)
            else:
                sampler = data_utils.RandomSampler(range(n)) if shuffle else data_utils.SequentialSampler(range(n))
            batch_sampler = data_utils.BatchSampler(sampler, int(batch_size), drop_last=False)
            self._short_last = short_batch == "drop" and 0 < n % int(batch_size) < self.world
        self.batch_sampler = batch_sampler
        self.nz = int(hp.generator_noise_dim) if getattr(hp, "generator_add_noise", False) else 0
        self.seed = int(getattr(hp, "generator_noise_seed", 0))
        self.draws = int(first_draw)
        self.scol_host = np.array(static_columns(len(hp.windows), hp.stream_sizes, hp.has_dynamic_features, None, self.corpus.Dy), dtype=np.int32)
        if len(self.scol_host) and int(self.scol_host.max()) >= self.corpus.Dy:
            raise RuntimeError("You probably have specified wrong dimention params.")
        self._scol = None

    def __len__(self):
        return len(self.batch_sampler) - int(self._short_last)

    def plan(self):
        """The host plan of the next epoch (draws the sampler): see ``plan_epoch``.  The WHOLE epoch on every rank (``shard_plan``
        takes this rank's share of it); sets ``last_table_crc``."""
        import zlib
        table, plan = plan_epoch(self.corpus.offsets, self.corpus.lengths, self.batch_sampler)
        self.last_table_crc = zlib.crc32(table.tobytes())
        return table, plan

    def _case(self, table, n_slots):
        from . import _lib as L
        c, k = self.corpus, L.AssembleCase()
        k.Dx, k.Dy, k.nz, k.Ds = c.Dx, c.Dy, self.nz, len(self.scol_host)
        k.ldX, k.ldY = c.ldX, c.ldY
        k.x_kind, k.y_kind, k.stats_f64 = c.x_kind, c.y_kind, c.stats_f64
        k.key0, k.key1 = self.seed & 0xFFFFFFFF, self.draws & 0xFFFFFFFF
        k.F, k.n_slots = c.F, n_slots
        k.X_all, k.Y_all = c.X_all.data_ptr(), c.Y_all.data_ptr()
        k.x_a, k.x_b, k.y_a, k.y_b = [t.data_ptr() for t in c.stats]
        k.table, k.scol = table.data_ptr(), self._scol.data_ptr()
        if c.windows is not None:
            k.n_windows = len(c.windows)
            for w, coef in enumerate(c.windows):
                k.win_len[w] = len(coef)
                for j, v in enumerate(coef):
                    k.coef[w][j] = float(v)
            k.dsrc, k.dwin = c.dsrc.data_ptr(), c.dwin.data_ptr()
        return k

    def begin_epoch(self):
        """Uploads the corpus if it is not resident yet, plans the next epoch on the host and uploads its table: ``(case, plan)`` for
        ``assemble``.  Advances the draw counter.  With ``world > 1`` the plan is this rank's ``shard_plan``; the table is the whole
        epoch's on every rank."""
        c = self.corpus.upload(self.device)
        if self._scol is None:
            self._scol = torch.from_numpy(self.scol_host).to(c.device) if len(self.scol_host) else torch.zeros(1, dtype=torch.int32, device=c.device)
        table_host, plan = self.plan()
        if self.world > 1:
            plan = shard_plan(plan, self.rank, self.world, self.short_batch)
        if not plan:
            return None, plan
        table = torch.from_numpy(table_host).pin_memory().to(c.device, non_blocking=True)      # the epoch's one upload
        case = self._case(table, len(table_host))
        case._table = table                   # the launches read it: it lives as long as the case
        self.draws += 1
        return case, plan

    def assemble(self, case, first, B, T, out=None, B_global=None, tv_global=None):
        """One batch of the epoch in one launch on the current stream: ``(gi (B, T, ld_gi), y, y_static, mask (B, T, 1), lengths)``.
        ``out``: the five buffers to write instead of fresh ones (dense, gi on its pitch ``roundup(Dx + nz, 4)``).
        With ``world > 1``: ``B`` is this rank's share of the ``B_global`` sequences in the slots from ``first``, ``T`` the whole
        batch's, the launch is gt_op_assemble_shard and a sixth element follows: ``tv_global``, the 1-element float64 tensor (the given
        one or a fresh one) that receives the whole batch's valid-frame count."""
        import ctypes as C
        from . import _lib as L
        c = self.corpus
        Dx, nz, Dy, Ds = c.Dx, self.nz, c.Dy, len(self.scol_host)
        ld_gi = (Dx + nz + 3) // 4 * 4
        if out is None:
            kw = dict(device=c.device, dtype=torch.float32)
            out = (torch.empty(B, T, ld_gi, **kw), torch.empty(B, T, Dy, **kw), torch.empty(B, T, Ds, **kw), torch.empty(B, T, 1, **kw),
                   torch.empty(B, device=c.device, dtype=torch.int64))
        gi, y, ys, mask, lengths = out
        for t, shape in ((gi, (B, T, ld_gi)), (y, (B, T, Dy)), (ys, (B, T, Ds)), (mask, (B, T, 1)), (lengths, (B,))):
            if tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
                raise ValueError("ResidentLoader.assemble: an output buffer of shape %s where %s is needed" % (tuple(t.shape), shape))
        case.B, case.T, case.first_slot = B, T, first
        case.ld_gi, case.ld_y, case.ld_ys = ld_gi, Dy, Ds
        case.gi, case.y, case.y_static = gi.data_ptr(), y.data_ptr(), ys.data_ptr() if Ds else None
        case.mask, case.lengths = mask.data_ptr(), lengths.data_ptr()
        if self.world == 1:
            L.check(L.lib.gt_op_assemble_batch(C.byref(case), L.current_stream()))
            return out
        if B_global is None:
            raise ValueError("ResidentLoader.assemble: a sharded loader needs B_global, the sequence count of the whole batch")
        if tv_global is None:
            tv_global = torch.empty(1, device=c.device, dtype=torch.float64)
        if tuple(tv_global.shape) != (1,) or tv_global.dtype != torch.float64 or not tv_global.is_cuda:
            raise ValueError("ResidentLoader.assemble: tv_global is a 1-element float64 device tensor")
        shard = L.AssembleShard()
        shard.rank, shard.world, shard.B_global, shard.tv_global = self.rank, self.world, int(B_global), tv_global.data_ptr()
        L.check(L.lib.gt_op_assemble_shard(C.byref(case), C.byref(shard), L.current_stream()))
        return tuple(out) + (tv_global,)

    def __iter__(self):
        case, plan = self.begin_epoch()
        yield from self.batches(case, plan)

    def batches(self, case, plan):
        """The ``DeviceBatch``es of an epoch begun with ``begin_epoch``."""
        Dx, nz = self.corpus.Dx, self.nz
        for entry in plan:
            if self.world == 1:
                first, B, T, cpu_lengths = entry
                gi, y, ys, mask, lengths = self.assemble(case, first, B, T)
                tv = None
            else:
                first, B_global, B, T, cpu_lengths = entry
                gi, y, ys, mask, lengths, tv = self.assemble(case, first, B, T, B_global=B_global)
            g = gi if gi.size(-1) == Dx + nz else gi[:, :, :Dx + nz]
            yield DeviceBatch(gi[:, :, :Dx] if gi.size(-1) != Dx else gi, y, lengths, cpu_lengths, None, generator_input=g, y_static=ys, mask=mask,
                              tv_global=tv, max_len=T)


def _resident_loaders(corpora, datasets, hp, rank=0, world=1, short_batch="error"):
    loaders = {}
    for ph, shuffle, first_draw in (("train", True, 0), ("test", False, 1 << 31)):      # the draw counters of _loaders
        corpora[ph].attach_statistics(datasets[ph])
        loaders[ph] = ResidentLoader(corpora[ph], hp.batch_size, shuffle, hp, device=corpora[ph].device, first_draw=first_draw,
                                     rank=rank, world=world, short_batch=short_batch)
    return loaders


def resident_tts_loaders(X, Y, hp, device="cuda", rank=0, world=1, short_batch="error"):
    """train.py:744-770 on a device-resident corpus, raw arrays in: ``X``, ``Y`` are the reference's ``{"train": ..., "test": ...}`` of
    utterance sequences.  Each phase is uploaded once; the TRAIN statistics -- ``minmax`` of X, ``meanvar`` of Y -- are one device
    pass per side (gt_op_corpus_stats), no host arithmetic on frames; the ordinary ``TTSDataset``s carry them (``loader.dataset``), and
    the uploaded corpora go to the ``ResidentLoader``s as they are.  Returns ``(loaders, stats)``, ``stats`` under the names of the
    ``.npy`` files the reference saves: X_data_min, X_data_max, Y_data_mean, Y_data_var.  ``rank``, ``world``, ``short_batch``: a
    data-parallel rank's loaders (``ResidentLoader``); every rank uploads the whole corpus and computes the statistics itself -- the
    statistics pass is bit-identical from run to run, so the ranks agree without an exchange."""
    corpora = {ph: ResidentCorpus.from_arrays(X[ph], Y[ph], device=device) for ph in ("train", "test")}
    X_data_min, X_data_max = corpora["train"].minmax("x")
    Y_data_mean, Y_data_var = corpora["train"].meanvar("y")
    Y_data_std = np.sqrt(Y_data_var)
    datasets = {ph: TTSDataset(MemoryCacheDataset(X[ph], cache_size=hp.cache_size), MemoryCacheDataset(Y[ph], cache_size=hp.cache_size),
                               X_data_min, X_data_max, Y_data_mean, Y_data_std, hp=hp) for ph in corpora}
    stats = dict(X_data_min=X_data_min, X_data_max=X_data_max, Y_data_mean=Y_data_mean, Y_data_var=Y_data_var)
    return _resident_loaders(corpora, datasets, hp, rank, world, short_batch), stats


def resident_vc_loaders(X, Y, hp, device="cuda", rank=0, world=1, short_batch="error"):
    """train.py:725-741 on a device-resident corpus: the joint ``meanvar`` over the TRAIN X continued over the TRAIN Y, each cut to the
    utterance lengths, on the device; ``VCDataset``s carry the result.  Returns ``(loaders, stats)`` with data_mean, data_var.
    ``rank``, ``world``, ``short_batch`` as in ``resident_tts_loaders``."""
    corpora = {ph: ResidentCorpus.from_arrays(X[ph], Y[ph], device=device) for ph in ("train", "test")}
    train = corpora["train"]
    data_mean, data_var, last_sample_count = train.meanvar("x", train.lengths, return_last_sample_count=True)
    data_mean, data_var = train.meanvar("y", train.lengths, mean_=data_mean, var_=data_var, last_sample_count=last_sample_count)
    data_std = np.sqrt(data_var)
    datasets = {ph: VCDataset(MemoryCacheDataset(X[ph], cache_size=hp.cache_size), MemoryCacheDataset(Y[ph], cache_size=hp.cache_size),
                              data_mean, data_std) for ph in corpora}
    return _resident_loaders(corpora, datasets, hp, rank, world, short_batch), dict(data_mean=data_mean, data_var=data_var)
