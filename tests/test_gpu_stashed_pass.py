"""The refusals the stashed generator pass promises (GenPass and the event functions under gt_engine, gantts_amd/csrc/engine_internal.hip.h;
DESIGN.md 3.3.1): an event that drops the pass between apply_generator and the training update_generator makes that step ask for a
new apply_generator, gt_flush_generator_grads has nothing to back-propagate, and the next full step gives the undisturbed bits.

  dropping   model_forward of the generator (on_generator_plain_forward); matmul_bf16 on and off again (on_storage_form_changed, twice);
             a re-bind of the generator (on_generator_rebound)
  controls   model_forward of the DISCRIMINATOR and a flip of launch_riders and back drop nothing: the step goes on, same bits
  launches   gt_head_path_counts / gt_gemm_path_counts over one undisturbed step: the numbers of the step before the state moved into
             its owners (this file pins behaviour: every test here passes on the commit before it as well)

The freed-band event is pinned by tests/test_gpu_mlpg_stash.py, whose Step (the STEP networks of test_gpu_mlpg_band.py, no dropout: the
step count a plain forward advances changes no bit) and same_bits are used here.  The set of gt_clear_faults cannot be exercised:
nothing may provoke a fault."""
import functools

import pytest
import torch

from gantts_amd import _lib as L
from test_gpu_gan_objective import head_and_gemm_counts
from test_gpu_mlpg_stash import DENSE, Step, same_bits

B, TN, LENGTHS = 2, 24, [24, 17]
# one undisturbed step, launches by slot of gt_head_path_counts / gt_gemm_path_counts: read on the commit before the owners, where this file gives the same
HEAD_COUNTS = {0: 2, 13: 2}
GEMM_COUNTS = {36: 2, 132: 5, 216: 1, 312: 3, 324: 2, 420: 3, 480: 1, 492: 1, 582: 3, 583: 1, 584: 1}


def fresh():
    return Step(DENSE, B, TN, LENGTHS)


@functools.lru_cache(maxsize=None)
def undisturbed():
    """(the step's results, its head and product launches by slot): computed once, read by every test"""
    st = fresh()
    torch.cuda.synchronize()
    head_and_gemm_counts(reset=True)
    res = st.run()
    h, g = head_and_gemm_counts(reset=True)
    return res, {i: n for i, n in enumerate(h) if n}, {i: n for i, n in enumerate(g) if n}


def _forward_generator(st):
    out = st.eng.model_forward(st.mg, st.x)
    assert out.shape == (B, TN, 16) and bool(torch.isfinite(out).all())


def _storage_form_there_and_back(st):
    st.eng.set_option("matmul_bf16", 1)
    st.eng.set_option("matmul_bf16", 0)


def _rebind_generator(st):
    st.mg._version += 1      # what re-homed buffers do: bind_model sends gt_bind_model again
    st.eng.bind_model(L.ROLE_G, st.mg)


def _forward_discriminator(st):
    """gt_model_forward(role D) itself: Engine.model_forward would bind a network without spectral norm in the generator's slot"""
    st.eng.bind_model(L.ROLE_D, st.md)      # (as update_discriminator binds it)
    z = torch.rand(B, TN, 6, device="cuda")
    out = torch.empty(B, TN, 1, device="cuda")
    L.check(L.lib.gt_model_forward(st.eng._h, L.ROLE_D, L.ptr(z), None, B, TN, L.ptr(out), None, L.current_stream()))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


def _flip_launch_riders(st):
    st.eng.set_option("launch_riders", 0)
    st.eng.set_option("launch_riders", 1)      # (the default)


@pytest.mark.gpu
@pytest.mark.parametrize("event", [pytest.param(_forward_generator, id="model_forward_g"), pytest.param(_storage_form_there_and_back, id="matmul_bf16"),
                                   pytest.param(_rebind_generator, id="rebind_g")])
def test_a_dropped_pass_is_refused_and_the_next_step_is_undisturbed(event):
    want = undisturbed()[0]
    st = fresh()
    st.apply()
    event(st)
    with pytest.raises(RuntimeError, match="needs the y_hat / y_hat_static returned by the last apply_generator"):
        st.eng.update_generator(*st.g_args())
    with pytest.raises(RuntimeError, match="no generator pass to back-propagate"):
        st.eng.flush_generator_grads()
    same_bits(st.run(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("event", [pytest.param(_forward_discriminator, id="model_forward_d"), pytest.param(_flip_launch_riders, id="launch_riders")])
def test_what_does_not_drop_the_pass_does_not_move_the_step(event):
    same_bits(fresh().run(event), undisturbed()[0])      # (a dropped pass would have refused the step's update_generator)


@pytest.mark.gpu
def test_launches_of_one_step():
    _, head, gemm = undisturbed()
    print("head_path_counts", head)
    print("gemm_path_counts", gemm)
    assert (head, gemm) == (HEAD_COUNTS, GEMM_COUNTS)
