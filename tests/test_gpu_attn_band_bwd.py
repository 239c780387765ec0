"""Band (sliding-window) attention backward: omh_flash_attn_bwd_band_d128 through ops.flash_attn_bwd(window=) against
autograd through a banded fp32 softmax attention on the same bf16 inputs (flash-attn's bottom-right aligned band, as
the forward's test_flash_attention_causal_and_window)."""
import importlib

import pytest
import torch

from conftest import PKG, rel_rms

pytestmark = pytest.mark.gpu
LOG2E = 1.4426950408889634


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


def _band_mask(Lq, Lk, klen, left, right):
    """[Lq, Lk] bool: query i sees key j iff j < klen and i + klen - Lq - left <= j <= i + klen - Lq + right."""
    i = torch.arange(Lq, device="cuda")[:, None] + (klen - Lq)
    j = torch.arange(Lk, device="cuda")[None, :]
    ok = j < klen
    if left >= 0:
        ok = ok & (j >= i - left)
    if right >= 0:
        ok = ok & (j <= i + right)
    return ok


def _inputs(B, H, Lq, Lk, klens, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    d = H * 128
    q = torch.randn(B * Lq, d, device="cuda", generator=g).bfloat16()
    k = torch.randn(B * Lk, d, device="cuda", generator=g).bfloat16()
    v = torch.randn(B * Lk, d, device="cuda", generator=g).bfloat16()
    do = torch.randn(B * Lq, d, device="cuda", generator=g).bfloat16()
    kl = None if klens is None else torch.tensor(klens, dtype=torch.int32, device="cuda")
    return q, k, v, do, kl


def _forward(ops, q, k, v, kl, B, H, Lq, Lk, window, q_prescaled=0):
    """The product forward (short-sequence kernel, band): o, lse and the fp32 output o32 the backward needs."""
    d = H * 128
    Lp = (Lk + 63) // 64 * 64
    vt = torch.zeros(B, d, Lp, device="cuda", dtype=torch.bfloat16)
    vt[:, :, :Lk] = v.view(B, Lk, d).transpose(1, 2)
    o = torch.empty(B * Lq, d, device="cuda", dtype=torch.bfloat16)
    o32 = torch.empty(B * Lq, d, device="cuda", dtype=torch.float32)
    lse = torch.empty(B, H, Lq, device="cuda", dtype=torch.float32)
    ops.flash_attn_raw(ops.ptr(q), ops.ptr(k), ops.ptr(vt), ops.ptr(o), ops.ptr(kl) if kl is not None else None, B, H,
                       Lq, Lk, Lq * d, d, Lk * d, d, d * Lp, Lq * d, d, Lp, 128 ** -0.5, lse=ops.ptr(lse),
                       q_prescaled=q_prescaled, o32=ops.ptr(o32), window=window)
    return o, o32, lse


def _reference(q, k, v, do, klens, B, H, Lq, Lk, window):
    """Autograd through the banded fp32 attention; also the [B, Lq, Lk] band masks."""
    qr, kr, vr = (t.float().view(B, -1, H, 128).transpose(1, 2).detach().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bhid,bhjd->bhij", qr, kr) * 128 ** -0.5
    masks = torch.stack([_band_mask(Lq, Lk, Lk if klens is None else klens[b], *window) for b in range(B)])
    s = s.masked_fill(~masks[:, None], float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)          # rows whose band is empty
    out = torch.einsum("bhij,bhjd->bhid", p, vr)
    out.backward(do.float().view(B, Lq, H, 128).transpose(1, 2))
    d = H * 128
    grads = [g.transpose(1, 2).reshape(B * L, d) for g, L in ((qr.grad, Lq), (kr.grad, Lk), (vr.grad, Lk))]
    return grads, masks


CASES = [
    # B, H, Lq, Lk, klens, window
    (2, 2, 200, 200, None, (-1, 0)),                    # square causal-like
    (2, 2, 300, 300, None, (40, 25)),                   # a band across tile edges on both sides
    (1, 2, 700, 700, None, (128, 128)),                 # whole 64-position tiles skipped on both sides
    (2, 2, 260, 260, None, (0, -1)),                    # left-only
    (2, 2, 130, 333, [333, 150], (20, 10)),             # Lk > Lq: the band ends bottom-right
    (1, 2, 333, 130, None, (10, 5)),                    # Lk < Lq: the first rows see nothing
    (2, 2, 320, 320, [288, 120], (70, 30)),             # k_lens < Lq: negative shift (the padded model)
    (4, 12, 1560, 1560, [1560] * 4, (256, 256)),        # multi-clip: 4 clips x 1 560 rows, 12 heads
]


@pytest.mark.parametrize("B,H,Lq,Lk,klens,window", CASES)
def test_band_backward_matches_autograd(ops, B, H, Lq, Lk, klens, window):
    q, k, v, do, kl = _inputs(B, H, Lq, Lk, klens, Lq * 7 + Lk + window[0])
    o, o32, lse = _forward(ops, q, k, v, kl, B, H, Lq, Lk, window)
    dq, dk, dv = ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, o32=o32, window=window)
    (rq, rk, rv), masks = _reference(q, k, v, do, klens, B, H, Lq, Lk, window)
    for got, ref in ((dq, rq), (dk, rk), (dv, rv)):
        assert torch.isfinite(got).all()
        assert rel_rms(got, ref) < 1.2e-2
    # rows whose band is empty and keys no query reaches (past k_lens included): exactly zero, written
    dead_q = ~masks.any(2).reshape(B * Lq)
    dead_k = ~masks.any(1).reshape(B * Lk)
    assert float(dq[dead_q].abs().sum()) == 0.0
    assert float(dk[dead_k].abs().sum()) == 0.0 and float(dv[dead_k].abs().sum()) == 0.0
    # no atomics: repeatable bit for bit
    dq2, dk2, dv2 = ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, o32=o32, window=window)
    assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2)


@pytest.mark.parametrize("B,H,Lq,Lk,klens,window", [CASES[1], CASES[6]])
def test_band_backward_modes(ops, B, H, Lq, Lk, klens, window):
    """q_prescaled and bf16 outputs agree with the plain call; phases 1 + 2 + 3 give phase 0's bits."""
    q, k, v, do, kl = _inputs(B, H, Lq, Lk, klens, 11 + Lq)
    o, o32, lse = _forward(ops, q, k, v, kl, B, H, Lq, Lk, window)
    dq, dk, dv = ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, o32=o32, window=window)
    # bf16 gradients
    d = H * 128
    out = tuple(torch.empty(B * L, d, device="cuda", dtype=torch.bfloat16) for L in (Lq, Lk, Lk))
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, o32=o32, window=window, out=out)
    for got, ref in zip(out, (dq, dk, dv)):
        assert rel_rms(got.float(), ref) < 8e-3
    # q carrying scale * log2(e) (the model's q), forward and backward alike
    qp = (q.float() * (128 ** -0.5 * LOG2E)).bfloat16()
    op, o32p, lsep = _forward(ops, qp, k, v, kl, B, H, Lq, Lk, window, q_prescaled=1)
    dqp, dkp, dvp = ops.flash_attn_bwd(qp, k, v, op, do, lsep, kl, B, H, Lq, Lk, q_prescaled=True, o32=o32p, window=window)
    for got, ref in ((dqp, dq), (dkp, dk), (dvp, dv)):
        assert rel_rms(got, ref) < 1.2e-2
    # phases: delta, then dQ and dK / dV separately (the training step's two-stream split)
    delta = torch.empty(B, H, Lq, device="cuda", dtype=torch.float32)
    kw = dict(o32=o32, window=window, delta=delta)
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, phase=1, out=None, **kw)
    ph = [torch.full((B * L, d), float("nan"), device="cuda", dtype=torch.bfloat16) for L in (Lq, Lk, Lk)]
    ref0 = tuple(torch.empty(B * L, d, device="cuda", dtype=torch.bfloat16) for L in (Lq, Lk, Lk))
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, o32=o32, window=window, out=ref0)
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, phase=3, out=tuple(ph), **kw)
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, phase=2, out=tuple(ph), **kw)
    for a, b in zip(ph, ref0):
        assert torch.equal(a, b)


def test_unbounded_window_is_the_plain_call(ops):
    """window=(-1, -1) through ops.flash_attn_bwd is the call without the argument, bit for bit."""
    B, H, Lq, Lk, klens = 2, 2, 300, 300, [300, 170]
    q, k, v, do, kl = _inputs(B, H, Lq, Lk, klens, 5)
    o, o32, lse = _forward(ops, q, k, v, kl, B, H, Lq, Lk, (-1, -1))
    a = ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, o32=o32)
    b = ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, o32=o32, window=(-1, -1))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # the band kernels with a band wider than the problem: full attention (other kernels: close, not bit-equal)
    c = ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, o32=o32, window=(Lq + Lk, Lq + Lk))
    for x, y in zip(a, c):
        assert rel_rms(y, x) < 2e-3
    with pytest.raises(AssertionError):
        ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, window=(8, 8))     # a band needs o32
