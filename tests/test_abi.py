"""CPU-runnable checks of the drop-in boundary: the C-ABI shared library loads, exports every
symbol include/gantts_hip.h declares, and fails loudly (no fallback) when there is no GPU."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "gantts_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gt_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from gantts_amd import _lib
    names = declared_symbols()
    assert len(names) >= 30
    raw = C.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), "libgantts_hip.so does not export %s" % n
    # and the ctypes binding table covers the whole header (nothing bound by accident only)
    assert sorted(_lib.SIGNATURES) == names


def test_version_and_error_channel():
    from gantts_amd import _lib
    assert b"gfx950" in _lib.lib.gt_version()
    assert isinstance(_lib.lib.gt_last_error(), bytes)


def test_ctypes_structs_match_header_layout():
    from gantts_amd import _lib
    assert C.sizeof(_lib.StreamConfig) == 4 * (1 + 8 + 8 + 1 + 8 + 3)
    assert C.sizeof(_lib.DResult) == 24 and C.sizeof(_lib.GResult) == 20
    assert _lib.ModelDesc.params.offset == 48 and C.sizeof(_lib.ModelDesc) == 72
    assert _lib.OptimDesc.step.offset == 32 and C.sizeof(_lib.OptimDesc) == 56
    assert _lib.GemmCase.x.offset == 104 and _lib.GemmCase.db.offset == 192 and C.sizeof(_lib.GemmCase) == 200
    assert _lib.GemmB16Case.ldcbt.offset == 68 and _lib.GemmB16Case.x.offset == 72 and _lib.GemmB16Case.db.offset == 152
    assert C.sizeof(_lib.GemmB16Case) == 160
    assert C.sizeof(_lib.CastJob) == 56 and _lib.CastJob.rows.offset == 24 and _lib.CastJob.ldi.offset == 40
    assert _lib.CastCase.rows.offset == 40 and _lib.CastCase.in_.offset == 72 and _lib.CastCase.idx.offset == 136
    assert _lib.CastCase.jobs.offset == 144 and C.sizeof(_lib.CastCase) == 144 + 8 * 56
    assert _lib.SruScanCase.keep_scale.offset == 32 and _lib.SruScanCase.ldu.offset == 56 and _lib.SruScanCase.ld_nxbt.offset == 80
    assert _lib.SruScanCase.U.offset == 96 and _lib.SruScanCase.dU_bt.offset == 224 and C.sizeof(_lib.SruScanCase) == 232
    assert C.sizeof(_lib.DropSite) == 56 and _lib.DropSite.dp_inv_t16.offset == 36 and _lib.DropSite.mask.offset == 48
    assert _lib.DHeadCase.eps.offset == 56 and _lib.DHeadCase.rows.offset == 64 and _lib.DHeadCase.drop.offset == 96
    assert _lib.DHeadCase.H.offset == 152 and _lib.DHeadCase.scalars.offset == 240 and C.sizeof(_lib.DHeadCase) == 248
    assert _lib.DStackCase.eps.offset == 48 and _lib.DStackCase.rows.offset == 56 and _lib.DStackCase.drop.offset == 80
    assert _lib.DStackCase.H0.offset == 304 and _lib.DStackCase.W.offset == 312 and _lib.DStackCase.Hout.offset == 408
    assert _lib.DStackCase.gadv.offset == 480 and _lib.DStackCase.scalars.offset == 488 and C.sizeof(_lib.DStackCase) == 496
    assert _lib.FrameCase.tv.offset == 88 and _lib.FrameCase.rows.offset == 112 and _lib.FrameCase.drop.offset == 144 and _lib.FrameCase.a.offset == 200
    assert _lib.FrameCase.out.offset == 280 and _lib.FrameCase.scalars.offset == 312 and C.sizeof(_lib.FrameCase) == 320
    assert _lib.MlpgCase.ldy.offset == 16 and _lib.MlpgCase.ldt.offset == 32 and _lib.MlpgCase.mse_w.offset == 36 and _lib.MlpgCase.e.offset == 40
    assert _lib.MlpgCase.R.offset == 48 and _lib.MlpgCase.scol.offset == 56 and _lib.MlpgCase.y.offset == 72 and _lib.MlpgCase.gs.offset == 88
    assert _lib.MlpgCase.yhat.offset == 104 and _lib.MlpgCase.mask.offset == 120 and _lib.MlpgCase.kb.offset == 128 and C.sizeof(_lib.MlpgCase) == 136


def test_invalid_arguments_are_reported_not_crashing():
    from gantts_amd import _lib
    cfg = _lib.StreamConfig()
    cfg.n_streams = 0
    h = C.c_void_p()
    rc = _lib.lib.gt_engine_create(C.byref(cfg), C.byref(h))
    assert rc == _lib.GT_ERR_INVALID and b"n_streams" in _lib.lib.gt_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc)
    assert _lib.lib.gt_zero_grad(None, 0) == _lib.GT_ERR_INVALID


@pytest.mark.skipif(torch.cuda.is_available(), reason="this is the no-GPU behaviour")
def test_no_gpu_means_loud_failure_not_fallback():
    import gantts_amd.train as T
    from gantts_amd import hparams, models
    from gantts_amd.engine import StepEngine
    m = models.MLP(in_dim=8, out_dim=3, num_hidden=1, hidden_dim=4, last_sigmoid=False)
    with pytest.raises(RuntimeError, match="GPU only|no CPU|no ROCm-capable device"):
        m(torch.rand(1, 5, 8))
    T.hp = hparams.tts_acoustic
    with pytest.raises(RuntimeError):
        T.apply_generator(m, torch.rand(1, 5, 8), None, [5])
    with pytest.raises(Exception) as ei:      # engine creation needs device memory
        StepEngine(hparams.tts_acoustic)
    assert "HIP" in str(ei.value) or "hip" in str(ei.value)
