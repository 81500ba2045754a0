"""SRURNN.set_dropout_masks for the three passes of an SRURNN in the discriminator slot (0: D(real), 1: D(fake) of the D step,
2: D(fake) of the G step): host-side bookkeeping only, no device."""
import pytest
import torch

from gantts_amd import models


def _d():
    # 2 layers, 6 columns: sites per pass = layer 0 input (B, 10), layer 0 output (B, 6), layer 1 input (B, 6)
    return models.SRURNN(in_dim=10, out_dim=1, num_hidden=2, hidden_dim=3, bidirectional=True, dropout=0.3, last_sigmoid=True,
                         use_relu=1, rnn_dropout=0.25)


def _masks(B, fill):
    return [torch.full((B, 10), fill), torch.full((B, 6), fill), torch.full((B, 6), fill)]


def test_passes_1_and_2_are_accepted_and_kept_apart():
    m = _d()
    for p in range(3):
        m.set_dropout_masks(p, _masks(4, float(p)))
    for p in range(3):
        for site, width in ((0, 10), (1, 6), (2, 6)):
            t = m._masks[(p, site)]
            assert tuple(t.shape) == (4, width) and bool((t == float(p)).all()), (p, site)
        assert m._masks[(p, 3)] is None      # the last layer has no output dropout
    m._check_masks(4, 7)
    with pytest.raises(RuntimeError):
        m._check_masks(5, 7)                 # (B, width): one row per sequence


def test_pass_3_is_rejected():
    m = _d()
    with pytest.raises(ValueError):
        m.set_dropout_masks(3, _masks(4, 1.0))
    with pytest.raises(ValueError):
        m.set_dropout_masks(-1, _masks(4, 1.0))
    assert not m._masks


def test_wrong_widths_and_surplus_masks_are_rejected_on_every_pass():
    m = _d()
    for p in (1, 2):
        bad = _masks(4, 1.0)
        bad[1] = torch.ones(4, 10)
        with pytest.raises(ValueError, match="must be"):
            m.set_dropout_masks(p, bad)
        with pytest.raises(ValueError, match="too many"):
            m.set_dropout_masks(p, _masks(4, 1.0) + [torch.ones(4, 6)])
        with pytest.raises(ValueError, match="too few"):
            m.set_dropout_masks(p, _masks(4, 1.0)[:2])


def test_none_clears_one_pass_only():
    m = _d()
    for p in range(3):
        m.set_dropout_masks(p, _masks(4, 1.0))
    v = m._version
    m.set_dropout_masks(1, None)
    assert m._version > v                    # the engine re-binds and forgets the pointers of that pass
    for site in range(4):
        assert m._masks[(1, site)] is None
    for p in (0, 2):
        for site in range(3):
            assert m._masks[(p, site)] is not None
