"""WanModel(window_size=(left, right)): the sliding-window self-attention in inference and training, against the
reference's own WanModel run with the same band (tests/golden/dit_window_t2v_L2.npz, made by
tests/make_golden_window.py: tiny t2v, 2 layers, two clips of 288 and 120 tokens padded to seq_len 320, so the band's
shift k_lens - seq_len is negative as in the reference)."""
import importlib
import os

import numpy as np
import pytest
import torch

import make_golden_window as MW
from conftest import PKG, rel_rms

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dit_window_t2v_L2.npz")
TOL_TINY = 8.0e-3       # the tiny goldens' forward bound (test_gpu_dit.py)
TOL_GRAD = 2e-2         # the training step's gradient bound (test_gpu_train.py)


@pytest.fixture(scope="module")
def model_mod():
    return importlib.import_module(PKG + ".wan.modules.model")


def _model(model_mod, window, train=False):
    from oracle import wan_dit_oracle as O
    cfg, xs, ctx, t, targets = MW.case()
    m = model_mod.WanModel(num_layers=2, window_size=window, **MW.make_golden.TINY)
    m.load_state_dict(O.synth_state_dict(cfg, MW.TAG))
    m = m.cuda()
    m = m.train() if train else m.eval().requires_grad_(False)
    return m, [u.cuda() for u in xs], [c.cuda() for c in ctx], t.cuda(), [v.cuda() for v in targets]


def test_window_forward_matches_reference(model_mod):
    g = np.load(GOLD)
    window = tuple(int(w) for w in g["window"])
    m, xs, ctx, t, _ = _model(model_mod, window)
    out = m(xs, t, ctx, int(g["seq_len"]))
    for o, key in zip(out, ("out0", "out1")):
        assert rel_rms(o, torch.from_numpy(g[key])) < TOL_TINY
    # the CFG pair shares block 0's self-attention: the same band, the same bits as two forwards
    cond, uncond = m.forward_cfg_pair(xs, t, ctx, [c[:5] for c in ctx], int(g["seq_len"]))
    for a, b in zip(cond, out):
        assert torch.equal(a, b)
    alone = m(xs, t, [c[:5] for c in ctx], int(g["seq_len"]))
    for a, b in zip(uncond, alone):
        assert torch.equal(a, b)
    # a band wider than the sequence is full attention, bit for bit
    wide, *_ = _model(model_mod, (10_000, 10_000))
    full, *_ = _model(model_mod, (-1, -1))
    for a, b in zip(wide(xs, t, ctx, int(g["seq_len"])), full(xs, t, ctx, int(g["seq_len"]))):
        assert torch.equal(a, b)


def test_window_training_gradients_match_reference(model_mod):
    g = np.load(GOLD)
    window = tuple(int(w) for w in g["window"])
    m, xs, ctx, t, targets = _model(model_mod, window, train=True)
    out = m(xs, t, ctx, int(g["seq_len"]))
    for o, key in zip(out, ("out0", "out1")):
        assert rel_rms(o.detach(), torch.from_numpy(g[key])) < TOL_TINY
    loss = sum(torch.nn.functional.mse_loss(o, v) for o, v in zip(out, targets))
    assert abs(loss.item() - float(g["loss"])) < 2e-2 * float(g["loss"])
    loss.backward()
    params = dict(m.named_parameters())
    for name in MW.GRAD_NAMES:
        ref = torch.from_numpy(g[name])
        got = params[name].grad
        got = got if got.dim() == 1 else got[:ref.shape[0]]
        assert rel_rms(got, ref) < TOL_GRAD, name


def test_window_training_refuses_v1_backward(model_mod, monkeypatch):
    """The round-2 backward has no band: a windowed block under it is an error, not full-attention gradients."""
    mt = importlib.import_module(PKG + ".wan.modules.model_train")
    monkeypatch.setattr(mt, "_ATTN_BWD2", False)
    m, xs, ctx, t, _ = _model(model_mod, (70, 30), train=True)
    with pytest.raises(NotImplementedError):
        m(xs, t, ctx, 320)
