"""A resolved ``ops.AttnMask`` handed in as ``mask=`` runs the launches of the four keywords it stands for: the same bits,
forward and backward, for every kind.  B = 2, H = 2, Lq = Lk = 320 (three 128-blocks with a ragged last one, five interval
groups of 64), k_lens = q_lens = [320, 200]."""
import importlib

import pytest
import torch

import make_golden_chunk_causal as MC
import self_forcing_ref as SF
from conftest import PKG
from oracle import wan_dit_oracle as O

pytestmark = pytest.mark.gpu
B, H, L = 2, 2, 320


@pytest.fixture(scope="module")
def causal():
    return importlib.import_module(PKG + ".causal")


@pytest.fixture(scope="module")
def operands():
    g = torch.Generator().manual_seed(20)
    q, k, v, do = (torch.randn(B, L, H, 128, generator=g).to(torch.bfloat16).cuda() for _ in range(4))
    lens = torch.tensor([320, 200], dtype=torch.int32, device="cuda")
    return q, k, v, do, lens


def _keywords(causal, kind):
    three = [[1, 0, 0, 0, 0], [1, 1, 0, 0, 0], [1, 0, 1, 0, 0], [1, 0, 1, 1, 0], [1, 0, 1, 0, 1]]        # row 4: three runs
    return {"full": {}, "band": dict(window=(70, 30)),
            "block": dict(block_mask=torch.tensor([[1, 0, 1], [1, 1, 0], [0, 1, 1]], dtype=torch.bool)),
            "chunk": dict(chunk_causal=(64, 1, 0)),
            "interval2": dict(interval_mask=causal.IntervalMask(causal.sink_window_groups(5, 1, 1), 64, "cuda")),
            "interval3": dict(interval_mask=causal.IntervalMask(torch.tensor(three, dtype=torch.bool), 64, "cuda", runs=3))}[kind]


def _run(ops, operands, **kw):
    q, k, v, do, lens = operands
    q, k, v = (u.clone().requires_grad_(True) for u in (q, k, v))
    o = ops.flash_attn_func(q, k, v, lens, lens, **kw)
    o.backward(do)
    return o.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("kind", ["full", "band", "block", "chunk", "interval2", "interval3"])
def test_mask_value_has_the_keywords_bits(ops, causal, operands, kind):
    kw = _keywords(causal, kind)
    mask = ops.attn_mask(**kw, H=H, Lq=L, Lk=L, device=operands[0].device)
    assert mask.kind == kind.rstrip("23") and (kind[-1] not in "23" or mask.rule.runs == int(kind[-1]))
    for name, a, b in zip(("o", "dq", "dk", "dv"), _run(ops, operands, **kw), _run(ops, operands, mask=mask)):
        assert bool(a.float().abs().sum() > 0) and torch.equal(a, b), name


def test_mask_excludes_the_keywords_on_every_entry(ops, causal, operands):
    q, k, v, do, lens = operands
    vt = v.reshape(B, L, H * 128).transpose(1, 2).contiguous()
    q2 = q.view(B * L, H * 128)
    lse = torch.zeros(B, H, L, device="cuda")
    for kind in ("full", "chunk"):
        mask = ops.attn_mask(**_keywords(causal, kind), H=H, Lq=L, Lk=L, device=q.device)
        for extra in ("band", "block", "chunk", "interval2"):
            kw = _keywords(causal, extra)
            with pytest.raises(ValueError):
                ops.flash_attn(q, k, vt, mask=mask, **kw)
            with pytest.raises(ValueError):
                ops.flash_attn_func(q, k, v, mask=mask, **kw)
            with pytest.raises(ValueError):
                ops.flash_attn_bwd(q2, q2, q2, q2, q2, lse, None, B, H, L, L, mask=mask, **kw)
            with pytest.raises(ValueError):
                ops.flash_attn_raw(None, None, None, None, None, B, H, L, L, 0, 0, 0, 0, 0, 0, 0, L, 1.0, mask=mask, **kw)


def test_short_last_chunk_has_the_inference_bits(causal):
    """forward_chunk(grad=True) on a chunk shorter than the model's (one frame of two, behind a left_chunks = 1 window that
    has moved off the cache's start): the bits of the no_grad call on the same KVCache state.  (Whole chunks:
    test_gpu_self_forcing_model.py::test_forward_bits_are_the_inference_call.)"""
    model_mod = importlib.import_module(PKG + ".wan.modules.model")
    fpc, F = 2, 6
    cfg, clean, noisy, _, ctx, t = SF.inputs(F, fpc)
    m = model_mod.WanModel(num_layers=2, **MC.make_golden.TINY)
    m.load_state_dict(O.synth_state_dict(cfg, MC.TAG))
    m = m.cuda().train()
    m.set_causal_chunks(fpc, 1)
    cache = causal.KVCache(m, 2, F * SF.TPF, "cuda")
    ctx_d, zero = [u.cuda() for u in ctx], torch.zeros(2, device="cuda")
    with torch.no_grad():
        for I in range(2):
            m.forward_chunk([u[:, I * fpc:(I + 1) * fpc].contiguous().cuda() for u in clean], zero, ctx_d, cache, commit=True)
    x, tt = [u[:, 4:5].contiguous().cuda() for u in noisy], t[:, 2].cuda().contiguous()
    with torch.no_grad():
        want = m.forward_chunk(x, tt, ctx_d, cache, commit=False)
    got = m.forward_chunk(x, tt, ctx_d, cache, commit=False, grad=True)
    for a, b in zip(got, want):
        assert a.grad_fn is not None and a.shape == b.shape == (16, 1, 14, 16) and torch.equal(a.detach(), b)
