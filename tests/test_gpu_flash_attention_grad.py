"""flash_attention (the reference-signature wrapper) and ops.flash_attn_func are differentiable: gradients against fp32
autograd through a masked softmax on the same bf16-rounded inputs (no torch.autograd.gradcheck: the operands are bf16)."""
import importlib

import pytest
import torch

from conftest import PKG, rel_rms

pytestmark = pytest.mark.gpu
GRAD_TOL, FWD_RMS, FWD_MAX = 1.2e-2, 8e-3, 3e-2


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


@pytest.fixture(scope="module")
def attn_mod():
    return importlib.import_module(PKG + ".wan.modules.attention")


def _ref_attention(q, k, v, qlens, klens, window=(-1, -1), scale=128 ** -0.5):
    """fp32 softmax attention under q_lens / k_lens and flash-attn's bottom-right aligned band (shift = klen - qlen);
    q [B, Lq, H, D], k / v [B, Lk, H, D] fp32 (autograd flows through)."""
    B, Lq = q.shape[:2]
    Lk = k.shape[1]
    i = torch.arange(Lq, device=q.device)[:, None]
    j = torch.arange(Lk, device=q.device)[None, :]
    masks = []
    for b in range(B):
        ql = Lq if qlens is None else qlens[b]
        kl = Lk if klens is None else klens[b]
        ok = (i < ql) & (j < kl)
        if window[0] >= 0:
            ok = ok & (j >= i + (kl - ql) - window[0])
        if window[1] >= 0:
            ok = ok & (j <= i + (kl - ql) + window[1])
        masks.append(ok)
    m = torch.stack(masks)[:, None]                                   # [B, 1, Lq, Lk]
    s = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    p = torch.nan_to_num(torch.softmax(s.masked_fill(~m, float("-inf")), dim=-1), nan=0.0)
    return torch.einsum("bhij,bjhd->bihd", p, v)


def _lens(x):
    return None if x is None else torch.tensor(x, dtype=torch.int32, device="cuda")


def _leaves(B, Lq, Lk, H, seed, dtype):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randn(B, Lq, H, 128, device="cuda", generator=g).to(dtype)
    k = torch.randn(B, Lk, H, 128, device="cuda", generator=g).to(dtype)
    v = torch.randn(B, Lk, H, 128, device="cuda", generator=g).to(dtype)
    go = torch.randn(B, Lq, H, 128, device="cuda", generator=g).bfloat16().to(dtype)
    return q, k, v, go


def _ref_grads(q, k, v, go, qlens, klens, window=(-1, -1), q_scale=None):
    """Reference output and gradients with respect to q, k, v as given (the bf16 rounding is the identity for autograd)."""
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    qs = qr if q_scale is None else qr * q_scale
    out = _ref_attention(qs.bfloat16().float(), kr.bfloat16().float(), vr.bfloat16().float(), qlens, klens, window)
    g = go.float().clone()
    if qlens is not None:
        for b, n in enumerate(qlens):
            g[b, n:] = 0
    out.backward(g)
    return out.detach(), (qr.grad, kr.grad, vr.grad)


def test_wrapper_fp32_leaves_with_lens(attn_mod):
    B, Lq, Lk, H = 2, 150, 200, 2
    qlens, klens = [150, 77], [200, 60]
    q, k, v, go = _leaves(B, Lq, Lk, H, 1, torch.float32)
    q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True)
    out = attn_mod.flash_attention(q, k, v, q_lens=_lens(qlens), k_lens=_lens(klens))
    assert out.grad_fn is not None and out.dtype == torch.float32 and out.shape == q.shape
    out.backward(go)
    ref_out, ref = _ref_grads(q, k, v, go, qlens, klens)
    assert rel_rms(out.detach(), ref_out) < FWD_RMS and float((out.detach() - ref_out).abs().max()) < FWD_MAX
    for name, t, r in (("q", q, ref[0]), ("k", k, ref[1]), ("v", v, ref[2])):
        assert t.grad is not None and t.grad.dtype == torch.float32 and t.grad.shape == t.shape, name
        assert torch.isfinite(t.grad).all(), name
        err = rel_rms(t.grad, r)
        print(f"wrapper d{name}: rel_rms {err:.3e}")
        assert err < GRAD_TOL, name
    assert float(q.grad[1, 77:].abs().sum()) == 0.0 and float(k.grad[1, 60:].abs().sum()) == 0.0
    with torch.no_grad():
        plain = attn_mod.flash_attention(q, k, v, q_lens=_lens(qlens), k_lens=_lens(klens))
    assert plain.grad_fn is None and torch.equal(plain, out.detach())
    # attention() forwards to the same code
    out2 = attn_mod.attention(q, k, v, q_lens=_lens(qlens), k_lens=_lens(klens), deterministic=True)
    assert out2.grad_fn is not None and torch.equal(out2.detach(), out.detach())


def test_wrapper_bf16_only_k_v_need_grad(attn_mod):
    B, Lq, Lk, H = 2, 150, 200, 2
    klens = [200, 60]
    q, k, v, go = _leaves(B, Lq, Lk, H, 2, torch.bfloat16)
    k.requires_grad_(True), v.requires_grad_(True)
    out = attn_mod.flash_attention(q, k, v, k_lens=_lens(klens))
    assert out.dtype == torch.bfloat16
    out.backward(go)
    _, ref = _ref_grads(q, k, v, go, None, klens)
    assert q.grad is None
    for name, t, r in (("k", k, ref[1]), ("v", v, ref[2])):
        assert t.grad.dtype == torch.bfloat16 and t.grad.shape == t.shape
        assert rel_rms(t.grad.float(), r) < GRAD_TOL, name
    with torch.no_grad():
        assert torch.equal(attn_mod.flash_attention(q, k, v, k_lens=_lens(klens)), out.detach())


def test_wrapper_q_scale_reaches_q_grad(attn_mod):
    B, Lq, Lk, H = 1, 130, 70, 2
    q, k, v, go = _leaves(B, Lq, Lk, H, 3, torch.float32)
    q.requires_grad_(True)
    out = attn_mod.flash_attention(q, k, v, q_scale=0.5)
    out.backward(go)
    _, ref = _ref_grads(q, k, v, go, None, None, q_scale=0.5)
    assert k.grad is None and v.grad is None
    assert rel_rms(q.grad, ref[0]) < GRAD_TOL


@pytest.mark.parametrize("window", [(-1, 0), (40, 25)])
@pytest.mark.parametrize("qlens", [None, [200, 77]])
def test_flash_attn_func_band(ops, window, qlens):
    B, L, H = 2, 200, 2
    q, k, v, go = _leaves(B, L, L, H, 4 + window[0], torch.bfloat16)
    for t in (q, k, v):
        t.requires_grad_(True)
    out = ops.flash_attn_func(q, k, v, q_lens=_lens(qlens), window=window)
    assert out.grad_fn is not None
    out.backward(go)
    ref_out, ref = _ref_grads(q, k, v, go, qlens, None, window)
    assert rel_rms(out.detach().float(), ref_out) < FWD_RMS and float((out.detach().float() - ref_out).abs().max()) < FWD_MAX
    for name, t, r in (("q", q, ref[0]), ("k", k, ref[1]), ("v", v, ref[2])):
        assert torch.isfinite(t.grad.float()).all(), name
        err = rel_rms(t.grad.float(), r)
        print(f"flash_attn_func window {window} q_lens {qlens} d{name}: rel_rms {err:.3e}")
        assert err < GRAD_TOL, name
    # the forward's bits are ops.flash_attn's (the short-sequence kernel at this size)
    Lp = (L + 63) // 64 * 64
    vt = torch.zeros(B, H * 128, Lp, dtype=torch.bfloat16, device="cuda")
    vt[:, :, :L] = v.detach().reshape(B, L, H * 128).transpose(1, 2)
    plain = ops.flash_attn(q.detach(), k.detach(), vt, q_lens=_lens(qlens), window=window)
    assert torch.equal(plain, out.detach())


def test_flash_attn_func_full_attention_and_selective_grads(ops):
    """No lens, no window (the full-attention backward entry); only q needs a gradient."""
    B, Lq, Lk, H = 2, 140, 90, 2
    q, k, v, go = _leaves(B, Lq, Lk, H, 9, torch.bfloat16)
    q.requires_grad_(True)
    out = ops.flash_attn_func(q, k, v, k_lens=_lens([90, 33]))
    out.backward(go)
    _, ref = _ref_grads(q, k, v, go, None, [90, 33])
    assert k.grad is None and v.grad is None
    assert rel_rms(q.grad.float(), ref[0]) < GRAD_TOL


def test_pinned_refusals(attn_mod):
    """Kept on purpose (tests/test_gpu_kernels.py pins both): a later change to either must be deliberate."""
    q, k, v, _ = _leaves(1, 64, 64, 1, 5, torch.bfloat16)
    with pytest.raises(NotImplementedError):
        attn_mod.flash_attention(q, k, v, dropout_p=0.1)
    qg = q.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="flash_attn_func"):
        attn_mod.flash_attention(qg, k, v, causal=True)
    with torch.no_grad():                                             # forward-only causal stays available
        assert attn_mod.flash_attention(qg, k, v, causal=True).shape == q.shape


def test_module_trains_through_flash_attention(attn_mod):
    """nn.Linear -> flash_attention -> nn.Linear at dim 256, five AdamW steps on a fixed batch: the loss goes down and the
    first Linear — reached only through the attention's gradients — moves."""
    torch.manual_seed(0)
    B, L, dim, H = 2, 96, 256, 2

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.inp, self.out = torch.nn.Linear(dim, dim), torch.nn.Linear(dim, dim)

        def forward(self, x):
            h = self.inp(x).view(B, L, H, dim // H)
            return self.out(attn_mod.flash_attention(h, h, h).reshape(B, L, dim))

    m = Toy().cuda()
    x = torch.randn(B, L, dim, device="cuda")
    y = torch.randn(B, L, dim, device="cuda")
    w0 = m.inp.weight.detach().clone()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(m(x), y)
        loss.backward()
        assert m.inp.weight.grad is not None and torch.isfinite(m.inp.weight.grad).all()
        assert float(m.inp.weight.grad.abs().sum()) > 0
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0], losses
    assert not torch.equal(m.inp.weight.detach(), w0)
