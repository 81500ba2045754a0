"""Inference path of the reference's evaluation scripts, on the HIP forward kernels.

Only the model-side arithmetic is here; text front end (HTS labels, Merlin question sets) and the
vocoder (pyworld / pysptk) stay what they are in the reference -- CPU third-party code either side
of these calls:

    _generator_input(hp, x, seed)                     evaluation_tts.py:133-140
    predict_duration(model, feats, X_min, X_max, Y_mean, Y_std)
                                                      evaluation_tts.py:153-178 (gen_duration minus the label I/O)
    predict_acoustic(model, feats, X_min, X_max)      evaluation_tts.py:205-219
    gen_parameters(y_predicted, Y_mean, Y_std)        evaluation_tts.py:47-100 (MGE branch)
    gen_parameters_without_mge(y_predicted, Y_mean, Y_std)
                                                      evaluation_tts.py:84-99 (the other branch, as it evidently means)
    vc_convert(model, mc, data_mean, data_std)        evaluation_vc.py:56-92 (between analysis and synthesis)

``hp_acoustic`` / ``hp_duration`` / ``hp_vc`` are module globals like in the reference scripts.
Checkpoints written by the reference load unchanged (``gantts_amd.train.load_checkpoint``): the
model classes keep torch's state_dict keys.

A generator trained with a weight average (``hp.generator_ema_decay`` / ``model.enable_weight_average``) synthesises from the averaged
weights inside ``with model.averaged_weights():`` (``model.eval()`` first) -- every call above made there runs on them --, or from a
plain model that loaded the checkpoint's ``"ema_state_dict"`` with ``load_state_dict``.
"""
import numpy as np
import torch

from . import hparams
from .data import minmax_scale
from .engine import StepEngine
from .multistream import get_static_stream_sizes
from .paramgen import unit_variance_mlpg_band, unit_variance_mlpg_matrix_cuda

hp_acoustic = hparams.tts_acoustic
hp_duration = hparams.tts_duration
hp_vc = hparams.vc

_engines = {}


def _engine(hp):
    key = (tuple(hp.stream_sizes), tuple(hp.has_dynamic_features), len(hp.windows))
    eng = _engines.get(key)
    if eng is None:
        eng = _engines[key] = StepEngine(hp)
    return eng


def _generator_input(hp, x, seed=None):
    """Appends z ~ U[0,1) of width hp.generator_noise_dim when the generator was trained with noise."""
    if seed is not None:
        torch.manual_seed(seed)
    if hp.generator_add_noise:
        z = torch.rand(x.size(0), x.size(1), hp.generator_noise_dim).to(x.device)
        return torch.cat((x, z), -1)
    return x


def _forward(model, hp, feats):
    model.eval()
    x = torch.from_numpy(np.ascontiguousarray(feats)).float()
    xl = len(x)
    x = x.view(1, -1, x.size(-1))
    x = _generator_input(hp, x).cuda()
    out = model(x, [xl])
    return out.detach().cpu().numpy().reshape(-1, out.shape[-1])


def predict_duration(duration_model, linguistic_features, X_min, X_max, Y_mean, Y_std):
    """Rounded state durations (>= 1 frame) for one utterance; the statistics are the per-type dicts
    of the reference (``X_min["duration"]`` ...)."""
    ty = "duration"
    feats = minmax_scale(np.asarray(linguistic_features, dtype=np.float32), X_min[ty], X_max[ty], feature_range=(0.01, 0.99))
    pred = _forward(duration_model.cuda(), hp_duration, feats)
    pred = np.round(Y_std[ty] * pred + Y_mean[ty])
    pred[pred <= 0] = 1            # minimum state duration
    return pred


def predict_acoustic(acoustic_model, linguistic_features, X_min, X_max):
    """Normalised acoustic features (T, sum(stream_sizes)) for one utterance.  The reference passes
    ``hp_duration`` to _generator_input here as well (evaluation_tts.py:216); so does this."""
    ty = "acoustic"
    feats = minmax_scale(np.asarray(linguistic_features), X_min[ty], X_max[ty], feature_range=(0.01, 0.99))
    return _forward(acoustic_model.cuda(), hp_duration, feats)


def _mlpg_matrix(windows, T, device_band):
    """R of an utterance: the cached dense device matrix, or (``device_band``) its weightless stand-in -- the engine then builds
    the band on the device, with no O(T^2) host work or copy for an utterance length it has not seen."""
    return unit_variance_mlpg_band(windows, T) if device_band else unit_variance_mlpg_matrix_cuda(windows, T)


def gen_parameters(y_predicted, Y_mean, Y_std, mge_training=True, device_band=False):
    """(mgc, lf0, vuv, bap) of one utterance.  ``Y_mean`` / ``Y_std`` are the reference's dicts (``["acoustic"]``) or plain arrays.

    ``mge_training=True``: multi-stream MLPG on the normalised features (the banded device kernel, unit variance) followed by inverse
    scaling with statistics indexed in the static+dynamic domain.  ``device_band``: build the MLPG band on the device from
    ``hp.windows`` instead of from a dense host R.

    ``mge_training=False`` raises ``NotImplementedError``, as before: the reference's own branch cannot run (it multiplies a dict,
    evaluation_tts.py:86).  What that branch evidently means is ``gen_parameters_without_mge``."""
    if not mge_training:
        raise NotImplementedError("the reference's non-MGE branch multiplies a dict (evaluation_tts.py:86) and cannot run; "
                                  "what it evidently means is gen_parameters_without_mge(y_predicted, Y_mean, Y_std)")
    hp = hp_acoustic
    mean = Y_mean["acoustic"] if isinstance(Y_mean, dict) else Y_mean
    std = Y_std["acoustic"] if isinstance(Y_std, dict) else Y_std
    mgc_dim, lf0_dim, vuv_dim, bap_dim = hp.stream_sizes
    nw = len(hp.windows)
    lf0_0, vuv_0, bap_0 = mgc_dim, mgc_dim + lf0_dim, mgc_dim + lf0_dim + vuv_dim
    y = y_predicted if isinstance(y_predicted, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(y_predicted))
    y = y.float().cuda().view(1, -1, y.shape[-1])
    T = y.size(1)
    static = _engine(hp).mlpg_forward(y, _mlpg_matrix(hp.windows, T, device_band))[0].double().cpu().numpy()
    smgc, slf0, svuv, sbap = [int(v) for v in get_static_stream_sizes(hp.stream_sizes, hp.has_dynamic_features, nw)]
    mean, std = np.asarray(mean), np.asarray(std)
    mgc = static[:, :smgc] * std[:mgc_dim // nw] + mean[:mgc_dim // nw]
    lf0 = static[:, smgc:smgc + slf0] * std[lf0_0:lf0_0 + lf0_dim // nw] + mean[lf0_0:lf0_0 + lf0_dim // nw]
    bap = static[:, smgc + slf0 + svuv:] * std[bap_0:bap_0 + bap_dim // nw] + mean[bap_0:bap_0 + bap_dim // nw]
    vuv = y[0, :, vuv_0].cpu().numpy() * std[vuv_0] + mean[vuv_0]
    return mgc, lf0, vuv, bap


def gen_parameters_without_mge(y_predicted, Y_mean, Y_std):
    """(mgc, lf0, vuv, bap) of one utterance for a generator trained WITHOUT the MGE criterion (the baseline stage of train_gan.sh, any
    plain-MSE model): evaluation_tts.py:84-99 as it evidently means -- the reference itself hands the dicts to inv_scale (line 86) and
    indexes a plain array with a string (line 95), so the branch cannot run there, and ``gen_parameters(mge_training=False)`` keeps
    refusing it.  The features are denormalised first; mgc, lf0 and bap come from the variance-weighted MLPG (``paramgen.mlpg``, one
    ``StepEngine.mlpg_var`` launch for the three) with the data variance ``Y_std ** 2``; vuv is the denormalised column.  ``Y_mean`` /
    ``Y_std`` and the return types are those of ``gen_parameters``.  The device takes the denormalised features and the variances
    rounded to float32."""
    hp = hp_acoustic
    mean = np.asarray(Y_mean["acoustic"] if isinstance(Y_mean, dict) else Y_mean, dtype=np.float64)
    std = np.asarray(Y_std["acoustic"] if isinstance(Y_std, dict) else Y_std, dtype=np.float64)
    y = y_predicted.detach().cpu().numpy() if isinstance(y_predicted, torch.Tensor) else np.asarray(y_predicted)
    y = y.reshape(-1, y.shape[-1]).astype(np.float64)
    den = y * std + mean
    mgc_dim, lf0_dim, vuv_dim, bap_dim = hp.stream_sizes
    nw = len(hp.windows)
    smgc, slf0, svuv, sbap = [int(v) for v in get_static_stream_sizes(hp.stream_sizes, hp.has_dynamic_features, nw)]
    dev_y = torch.from_numpy(den.astype(np.float32)).cuda().view(1, -1, den.shape[-1])
    dev_var = torch.from_numpy((std * std).astype(np.float32)).cuda()
    static = _engine(hp).mlpg_var(dev_y, dev_var)[0].double().cpu().numpy()
    mgc, lf0, bap = static[:, :smgc], static[:, smgc:smgc + slf0], static[:, smgc + slf0 + svuv:]
    vuv = den[:, mgc_dim + lf0_dim]
    return mgc, lf0, vuv, bap


def vc_convert(model, mc, data_mean, data_std, diffvc=True, device_band=False):
    """Static mel-cepstrum conversion of one utterance.  ``mc`` (T, 3*order) = delta_features of the
    smoothed source mel-cepstrum (without c0).  Returns ``(inputs, outputs, mc_static_for_synthesis)``:
    the source statics, the converted statics, and what the reference hands to the synthesis filter
    (the difference to the source when ``diffvc``).  ``device_band``: as in ``gen_parameters``."""
    hp = hp_vc
    model = model.cuda()
    model.eval()
    mc = np.asarray(mc, dtype=np.float32)
    T = mc.shape[0]
    static_dim = mc.shape[-1] // len(hp.windows)
    inputs = mc[:, :static_dim].copy()
    mc_scaled = torch.from_numpy(((mc - data_mean) / data_std).astype(np.float32)).cuda().view(1, T, -1)
    R = _mlpg_matrix(hp.windows, T, device_band)
    if model.include_parameter_generation():
        _, y_hat_static = model(mc_scaled, R, lengths=[T])
    else:
        assert hp.has_dynamic_features is not None
        y_hat = model(mc_scaled, lengths=[T])
        y_hat_static = _engine(hp).mlpg_forward(y_hat, R)
    pred = y_hat_static.detach().cpu().numpy().reshape(-1, static_dim)
    pred = data_std[:static_dim] * pred + data_mean[:static_dim]
    outputs = pred.copy()
    if diffvc:
        pred = pred - mc[:, :static_dim]
    return inputs, outputs, pred
