"""How a step's scalars reach the host (csrc/eng_step.hip): early by ticket polling or by event (the fused calls), deferred with a
pinned page and an event per role (split-phase ``*_end(defer=True)`` + ``*_result()``), or a blocking fetch (split-phase ``*_end``).
The route decides only where the host waits: every pair of routes below must agree to the bit.  Two small golden cases at their
committed shapes with injected masks: ``acoustic_mlp_dropout`` (MLPG, split first layer, a kept leak gradient) and ``duration_mlp``
(no parameter generation, Adam).

Run as a script (``python tests/test_gpu_result_routes.py OUT.npz``) it dumps the fused run of ``duration_mlp``: the child process
of the GT_RES_HOSTMAP test."""
import ctypes as Ct
import functools
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np
import pytest

import cases as C

pytestmark = pytest.mark.gpu
NAMES = ["acoustic_mlp_dropout", "duration_mlp"]
FUSED, BLOCKING, DEFERRED = "fused", "blocking", "deferred"
DEFERRED_LATE_D = "deferred_late_d"      # the discriminator's result collected only behind update_generator_begin


@functools.lru_cache(maxsize=None)
def _fused(name):
    """The case through the fused calls under the default options: computed once, shared, never modified."""
    from hip_runner import run_hip_case
    return run_hip_case(C.CASES[name])


def _same_bits(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), "%s: %s" % (what, k)


class _Drive(object):
    """One engine with the case's networks, optimizers and batch, stepped by a chosen route per step (the setup of run_hip_case, the
    split-phase calls in the pattern of HipStepBackend / DataParallelStep).  Split-phase scalars are read from the C structs, so that
    grad_norm is among them."""

    def __init__(self, case):
        import torch
        from gantts_amd import optim, paramgen
        from gantts_amd.engine import engine_for
        from gantts_amd.multistream import get_static_features
        from gantts_amd.seqloss import sequence_mask
        from hip_runner import build_model, make_hp
        self.case, self.hp = case, make_hp(case)
        self.mg, self.md = build_model(case["g"], 11), build_model(case["d"], 22)
        for m in (self.mg, self.md):
            m.train() if case["dropout_on"] else m.eval()
        self.og = getattr(optim, case["opt_g"][0])(self.mg.parameters(), **case["opt_g"][1])
        self.od = getattr(optim, case["opt_d"][0])(self.md.parameters(), **case["opt_d"][1])
        self.eng = engine_for(self.hp, self.mg)
        x, y, lengths = C.make_batch(case)
        self.x, self.y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        self.lengths = list(lengths)
        self.R = paramgen.unit_variance_mlpg_matrix_cuda(self.hp.windows, case["T"]) if any(case["has_dynamic_features"]) else None
        self.y_static = get_static_features(self.y, len(self.hp.windows), self.hp.stream_sizes, self.hp.has_dynamic_features)
        self.mask = sequence_mask(torch.from_numpy(np.ascontiguousarray(lengths)).cuda(), max_len=case["T"]).unsqueeze(-1)
        self.w = (case["adv_w"], case["mse_w"], case["mge_w"])
        self.out = {}

    # the raw entry points: (status, scalars or None, message)
    def d_end(self, defer=False):
        from gantts_amd import _lib as L
        res = L.DResult()
        rc = L.lib.gt_update_discriminator_end(self.eng._h, 1, None if defer else Ct.byref(res), L.current_stream())
        return self._ret(rc, res, defer)

    def g_end(self, defer=False):
        from gantts_amd import _lib as L
        res = L.GResult()
        rc = L.lib.gt_update_generator_end(self.eng._h, 1, self.w[0], self.w[1], self.w[2], None if defer else Ct.byref(res), L.current_stream())
        return self._ret(rc, res, defer)

    def d_result(self):
        from gantts_amd import _lib as L
        res = L.DResult()
        return self._ret(L.lib.gt_update_discriminator_result(self.eng._h, Ct.byref(res)), res, False)

    def g_result(self):
        from gantts_amd import _lib as L
        res = L.GResult()
        return self._ret(L.lib.gt_update_generator_result(self.eng._h, Ct.byref(res)), res, False)

    @staticmethod
    def _ret(rc, res, defer):
        from gantts_amd import _lib as L
        if rc != L.GT_OK:
            return rc, None, L.lib.gt_last_error().decode()
        return rc, None if defer else np.array([getattr(res, f) for f, _ in res._fields_], dtype=np.float32), ""

    @staticmethod
    def _ok(r):
        assert r[0] == 0, r
        return r[1]

    def step(self, step, route):
        import torch
        from gantts_amd import _lib as L
        case, eng = self.case, self.eng
        if case["dropout_on"]:
            gm, dm = C.make_dropout_masks(case, step)
            nh = len(C.hidden_sites(case["d"]))
            self.mg.set_dropout_masks(0, [torch.from_numpy(m) for m in gm])
            for p in range(3):
                self.md.set_dropout_masks(p, [torch.from_numpy(m) for m in dm[p * nh:(p + 1) * nh]])
        self.og.zero_grad()
        self.od.zero_grad()
        y_hat, yhs = eng.apply_generator(self.mg, self.x, self.R, self.lengths)
        d_args = (self.md, self.od, self.x, self.y_static, yhs, self.mask, "train")
        g_args = (self.mg, self.md, self.og, self.x, self.y, y_hat, self.y_static, yhs, self.w[0], self.mask, "train", self.w[1], self.w[2])
        if route == FUSED:
            d = np.array(eng.update_discriminator(*d_args), dtype=np.float32)
            g = np.array(eng.update_generator(*g_args), dtype=np.float32)
        else:
            defer = route != BLOCKING
            eng.update_discriminator_begin(*d_args)
            d = self._ok(self.d_end(defer))
            self.od._note_step(eng, L.ROLE_D)
            if route == DEFERRED:
                d = self._ok(self.d_result())
            eng.update_generator_begin(*g_args)
            if route == DEFERRED_LATE_D:      # the generator step is already queued behind it
                d = self._ok(self.d_result())
            g = self._ok(self.g_end(defer))
            self.og._note_step(eng, L.ROLE_G)
            if defer:
                g = self._ok(self.g_result())
        self.out["d_scalars_%d" % step], self.out["g_scalars_%d" % step] = d, g

    def finish(self):
        import torch
        from hip_runner import state_arrays
        torch.cuda.synchronize()
        self.out.update(state_arrays(self.mg, self.md, self.og, self.od))
        return self.out


def _run(name, routes, hook=None):
    d = _Drive(C.CASES[name])
    for step, route in enumerate(routes):
        if hook:
            hook(d, "before", step)
        d.step(step, route)
        if hook:
            hook(d, "after", step)
    return d.finish()


@functools.lru_cache(maxsize=None)
def _split(name, route):
    """Two steps of the case through the split-phase calls by one route: computed once, shared, never modified."""
    return _run(name, [route, route])


@pytest.mark.parametrize("name", NAMES)
def test_fused_calls_polling_equals_event(name):
    """GT_OPT_POLL_RESULTS: the fused calls wait for a ticket behind the scalars in the host page, or for an event behind the
    finalising launch.  Only the host's wait differs: scalars, parameters and optimizer state are bit-identical."""
    from hip_runner import run_hip_case
    poll = run_hip_case(C.CASES[name], engine_options={"poll_results": 1})
    event = run_hip_case(C.CASES[name], engine_options={"poll_results": 0})
    _same_bits(poll, event, "poll_results 1 against 0")
    _same_bits(poll, _fused(name), "poll_results 1 against the default")


@pytest.mark.parametrize("route", [DEFERRED, DEFERRED_LATE_D])
@pytest.mark.parametrize("name", NAMES)
def test_split_phase_deferred_equals_blocking(name, route):
    """``*_end`` that fetches the scalars and blocks, against ``*_end(defer=True)`` + ``*_result()`` -- the discriminator's collected
    right away, or only once update_generator_begin is enqueued (the order of DataParallelStep): the same launches on the same
    stream, so every scalar (grad_norm included), every parameter and the optimizer state are bit-identical."""
    blocking, deferred = _split(name, BLOCKING), _split(name, route)
    assert blocking["d_scalars_0"].shape == (6,) and blocking["g_scalars_0"].shape == (5,)
    assert blocking["d_scalars_1"][5] > 0 and blocking["g_scalars_1"][4] > 0      # the gradient norms are reported on these routes
    _same_bits(blocking, deferred, route)


@pytest.mark.parametrize("name", NAMES)
def test_fused_equals_split_phase_in_the_first_d_step(name):
    """The D step of step 0 starts from the same parameters on both routes and runs the same head kernel: the counts are equal
    exactly, the three losses to the order of one float64 reduction (rtol 1e-6 / atol 1e-9, as for the launch riders: same sums,
    another place of reduction).  Nothing later is compared: the optimizer's squared norm is summed in another order there."""
    fused, split = _fused(name)["d_scalars_0"], _split(name, BLOCKING)["d_scalars_0"]
    print(name, "fused", [repr(float(v)) for v in fused[:5]], "split-phase", [repr(float(v)) for v in split[:5]])
    assert fused[3] == split[3] and fused[4] == split[4]
    np.testing.assert_allclose(np.asarray(split[:3], dtype=np.float64), np.asarray(fused[:3], dtype=np.float64), rtol=1e-6, atol=1e-9)


def test_refused_calls_leave_the_engine_as_it_was():
    """``_end`` without ``_begin`` and ``_result`` with nothing pending (a second ``_result`` after a collected one included) are
    refused with GT_ERR_STATE for both roles; the fused step that follows reproduces the bits of an engine that never saw them."""
    from gantts_amd import _lib as L
    name = "duration_mlp"
    seen = []

    def refuse(d, when, step):
        if (when, step) == ("before", 0):      # a fresh engine: nothing begun, nothing pending
            calls = [(d.d_end, "gt_update_discriminator_end without _begin"), (d.g_end, "gt_update_generator_end without _begin"),
                     (d.d_result, "no deferred discriminator result pending"), (d.g_result, "no deferred generator result pending")]
        elif (when, step) == ("after", 0):     # a finished step: its deferred results, if it had any, have been collected
            calls = [(d.d_result, "no deferred discriminator result pending"), (d.g_result, "no deferred generator result pending"),
                     (d.d_end, "gt_update_discriminator_end without _begin"), (d.g_end, "gt_update_generator_end without _begin")]
        else:
            return
        for call, text in calls:
            rc, res, msg = call()
            assert rc == L.GT_ERR_STATE and res is None and msg == text, (call.__name__, rc, msg)
            seen.append(text)
        with pytest.raises(RuntimeError, match="no deferred discriminator result pending"):      # the same refusal as the Python API raises it
            d.eng.update_discriminator_result()

    for routes in ([FUSED, FUSED], [DEFERRED, FUSED]):
        _same_bits(_run(name, routes, hook=refuse), _run(name, routes), "refused calls around %s" % (routes,))
    assert len(seen) == 16


def test_results_through_a_device_to_host_copy(tmp_path):
    """GT_RES_HOSTMAP=0 (read at engine creation, hence a process of its own): the early results leave through a device-to-host
    copy and an event instead of being written into the mapped host page.  Same bits as the default."""
    out = str(tmp_path / "hostmap0.npz")
    env = dict(os.environ, GT_RES_HOSTMAP="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, timeout=240, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode("utf-8", "replace")[-2000:]
    with np.load(out) as z:
        _same_bits({k: z[k] for k in z.files}, _fused("duration_mlp"), "GT_RES_HOSTMAP=0 against the default")


if __name__ == "__main__":
    from hip_runner import run_hip_case
    np.savez(sys.argv[1], **{k: np.asarray(v) for k, v in run_hip_case(C.CASES["duration_mlp"]).items()})
