"""WanModel.set_attention_block_mask: block-sparse self-attention in inference, forward_cfg_pair and training, on the
tiny two-layer t2v case of tests/make_golden_window.py (two clips of 288 and 120 tokens padded to seq_len 320: nb = 3).

The reference is the CPU oracle run here, with ``oracle.wan_dit_oracle.masked_attention`` rebound by the test to a
dense-masked fp32 softmax: the block mask is applied where ``q.shape[1] == k.shape[1] == 320`` (the self-attention
call); cross-attention (text length != 320) passes through unchanged."""
import importlib

import pytest
import torch

import make_golden_window as MW
from conftest import PKG, rel_rms

pytestmark = pytest.mark.gpu
TOL_TINY = 8.0e-3       # the tiny goldens' forward bound (test_gpu_dit.py)
TOL_GRAD = 2e-2         # the training step's gradient bound (test_gpu_train.py)
SEQ_LEN = 320
NB = 3


@pytest.fixture(scope="module")
def model_mod():
    return importlib.import_module(PKG + ".wan.modules.model")


def _mask(heads=2):
    """Per head: diagonal forced, block (2, 0) dropped, block (0, 1) dropped for odd heads."""
    m = torch.ones(heads, NB, NB, dtype=torch.bool)
    m[:, 2, 0] = False
    m[1::2, 0, 1] = False
    return m


def _model(model_mod, train=False):
    from oracle import wan_dit_oracle as O
    cfg, xs, ctx, t, targets = MW.case()
    assert all(c.shape[0] != SEQ_LEN for c in ctx) and cfg.text_len != SEQ_LEN      # only self-attention has 320 keys
    m = model_mod.WanModel(num_layers=2, **MW.make_golden.TINY)
    m.load_state_dict(O.synth_state_dict(cfg, MW.TAG))
    m = m.cuda()
    m = m.train() if train else m.eval().requires_grad_(False)
    return m, [u.cuda() for u in xs], [c.cuda() for c in ctx], t.cuda(), [v.cuda() for v in targets]


class _Patched:
    """``masked_attention`` with a block mask on the self-attention calls: ``masks[i]`` for the i-th of them in a forward
    (None: unmasked), every other call passed through."""

    def __init__(self, monkeypatch, masks):
        from oracle import wan_dit_oracle as O
        self.orig, self.masks, self.calls = O.masked_attention, masks, 0
        monkeypatch.setattr(O, "masked_attention", self)

    def __call__(self, q, k, v, k_lens=None, **kw):
        if not (q.shape[1] == k.shape[1] == SEQ_LEN):
            return self.orig(q, k, v, k_lens, **kw)
        mask = self.masks[self.calls % len(self.masks)]
        self.calls += 1
        if mask is None:
            return self.orig(q, k, v, k_lens, **kw)
        B, S, N, D = q.shape
        dense = mask.repeat_interleave(128, 1).repeat_interleave(128, 2)[:, :S, :S]       # [N, S, S]
        out = []
        for b in range(B):
            vis = dense.clone()
            vis[:, :, int(k_lens[b]):] = False
            s = torch.einsum("qhd,khd->hqk", q[b].float(), k[b].float()) * D ** -0.5
            p = torch.nan_to_num(torch.softmax(s.masked_fill(~vis, float("-inf")), dim=-1), nan=0.0)
            out.append(torch.einsum("hqk,khd->qhd", p, v[b].float()))
        return torch.stack(out)


def _oracle_forward(monkeypatch, masks):
    from oracle import wan_dit_oracle as O
    cfg, xs, ctx, t, _ = MW.case()
    patch = _Patched(monkeypatch, masks)
    out = O.dit_forward(O.synth_state_dict(cfg, MW.TAG), cfg, xs, t, ctx, SEQ_LEN)
    assert patch.calls == 2                                                      # one self-attention per layer
    return out


def test_masked_inference_matches_oracle_and_cfg_pair(model_mod, monkeypatch):
    mask = _mask()
    ref = _oracle_forward(monkeypatch, [mask, mask])
    m, xs, ctx, t, _ = _model(model_mod)
    plain = m(xs, t, ctx, SEQ_LEN)
    m.set_attention_block_mask(mask)
    out = m(xs, t, ctx, SEQ_LEN)
    for o, r in zip(out, ref):
        err = rel_rms(o, r)
        print(f"masked inference rel-RMS {err:.2e}")
        assert err < TOL_TINY
    # (clip 1 has 120 tokens: its live rows and keys lie in block (0, 0), which every head keeps — only clip 0 can differ)
    assert not torch.equal(out[0], plain[0])
    # the CFG pair shares block 0's self-attention: the same mask, the same bits as two forwards
    cond, uncond = m.forward_cfg_pair(xs, t, ctx, [c[:5] for c in ctx], SEQ_LEN)
    for a, b in zip(cond, out):
        assert torch.equal(a, b)
    for a, b in zip(uncond, m(xs, t, [c[:5] for c in ctx], SEQ_LEN)):
        assert torch.equal(a, b)
    # a mask for another length is refused at the call
    m.set_attention_block_mask(torch.ones(4, 4, dtype=torch.bool))
    with pytest.raises(ValueError):
        m(xs, t, ctx, SEQ_LEN)
    # clearing restores the unmasked bits
    m.set_attention_block_mask(None)
    for a, b in zip(m(xs, t, ctx, SEQ_LEN), plain):
        assert torch.equal(a, b)
    # an all-true mask: both on the short-sequence kernel at this size, so the same bits too
    m.set_attention_block_mask(torch.ones(NB, NB, dtype=torch.bool))
    for a, b in zip(m(xs, t, ctx, SEQ_LEN), plain):
        assert torch.equal(a, b)


def test_mask_on_one_layer(model_mod, monkeypatch):
    mask = _mask()
    ref = _oracle_forward(monkeypatch, [None, mask])                             # only the second self-attention call
    m, xs, ctx, t, _ = _model(model_mod)
    plain = m(xs, t, ctx, SEQ_LEN)
    m.set_attention_block_mask(mask)
    full = m(xs, t, ctx, SEQ_LEN)
    m.set_attention_block_mask(None)
    m.set_attention_block_mask(mask, layers=[1])
    out = m(xs, t, ctx, SEQ_LEN)
    for o, r in zip(out, ref):
        assert rel_rms(o, r) < TOL_TINY
    # (clip 0: the 288-token clip, the one whose rows reach the dropped blocks)
    assert not torch.equal(out[0], plain[0]) and not torch.equal(out[0], full[0])


def test_masked_training_matches_oracle(model_mod, monkeypatch):
    from oracle import wan_dit_oracle as O
    mask = _mask()
    cfg, xs_c, ctx_c, t_c, targets_c = MW.case()
    sd = {k: v.clone().requires_grad_(True) for k, v in O.synth_state_dict(cfg, MW.TAG).items()}
    _Patched(monkeypatch, [mask, mask])
    ref_out = O.dit_forward_autograd(sd, cfg, xs_c, t_c, ctx_c, SEQ_LEN)
    ref_loss = sum(torch.nn.functional.mse_loss(o, v) for o, v in zip(ref_out, targets_c))
    ref_loss.backward()

    def grads(policy, keep):
        m, xs, ctx, t, targets = _model(model_mod, train=True)
        m.set_attention_block_mask(mask)
        if policy is not None:
            m.checkpoint_policy = policy
        m.use_checkpoint = not keep
        out = m(xs, t, ctx, SEQ_LEN)
        loss = sum(torch.nn.functional.mse_loss(o, v) for o, v in zip(out, targets))
        loss.backward()
        params = dict(m.named_parameters())
        return loss.item(), {n: params[n].grad.clone() for n in MW.GRAD_NAMES}

    loss, got = grads(None, False)
    print(f"masked training loss {loss:.6f} vs {ref_loss.item():.6f}")
    assert abs(loss - ref_loss.item()) < 2e-2 * ref_loss.item()
    for name in MW.GRAD_NAMES:
        err = rel_rms(got[name], sd[name].grad)
        print(f"{name}: rel-RMS {err:.2e}")
        assert err < TOL_GRAD, name
    # the same gradients, bit for bit, when every block is re-run in the backward and when the activations are kept
    for policy, keep in (("always", False), (None, True)):
        _, other = grads(policy, keep)
        for name in MW.GRAD_NAMES:
            assert torch.equal(other[name], got[name]), (policy, keep, name)


def test_masked_training_refuses_v1_backward(model_mod, monkeypatch):
    mt = importlib.import_module(PKG + ".wan.modules.model_train")
    monkeypatch.setattr(mt, "_ATTN_BWD2", False)
    m, xs, ctx, t, _ = _model(model_mod, train=True)
    m.set_attention_block_mask(_mask())
    with pytest.raises(NotImplementedError):
        m(xs, t, ctx, SEQ_LEN)
