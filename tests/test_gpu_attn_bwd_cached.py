"""The attention backward of a chunk of queries against cached keys, omh_flash_attn_bwd_cached_d128 through
``ops.flash_attn_bwd(own_lo=)``: dq over all Lk keys, dk / dv for the rows [own_lo, Lk) only — against autograd through a
dense fp32 softmax attention on the same bf16 operands (built as in test_gpu_attn_interval.py).  And the few-step
sampler update ``ops.flow_x0_step`` against the fp32 expression.

Bounds: the project's own for this arithmetic (test_gpu_attn_interval.py): attention gradients rel-RMS < 1.2e-2, bf16
outputs against fp32 ones < 8e-3.  ``flow_x0_step``: 1 ulp of the fp32 expression, elementwise."""
import importlib

import pytest
import torch

from conftest import PKG, rel_rms

pytestmark = pytest.mark.gpu
GRAD_RMS, BF16_RMS = 1.2e-2, 8e-3
LOG2E = 1.4426950408889634

CASES = [
    # B, H, Lq, Lk, own_lo, rows of the key buffer in front of the keys (look-back offset), rows of the buffer
    (1, 2, 168, 336, 168, 0, 336),                 # neither a multiple of 64
    (1, 2, 56, 280, 224, 0, 280),                  # Lq under one block
    (1, 2, 112, 112, 0, 0, 112),                   # own_lo = 0: the plain entry's bits
    (2, 2, 112, 224, 112, 56, 400),                # keys at row 56 of a larger buffer: batch stride != Lk d, B = 2
    (1, 12, 1560, 4680, 3120, 0, 4680),            # a real chunk against two cached ones, 12 heads: both passes split
]
PLAIN, OFFSET, REAL = 2, 3, 4
_CACHE = {}


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


def _case(idx, ops):
    """Operands, the forward's (o, o32, lse) and the fp32 reference gradients — computed once per case, left unchanged."""
    if idx in _CACHE:
        return _CACHE[idx]
    B, H, Lq, Lk, own_lo, front, cap = CASES[idx]
    d = H * 128
    g = torch.Generator(device="cuda").manual_seed(900 + idx)
    q = torch.randn(B, Lq, d, device="cuda", generator=g).bfloat16()
    kbuf = torch.randn(B, cap, d, device="cuda", generator=g).bfloat16()
    vbuf = torch.randn(B, cap, d, device="cuda", generator=g).bfloat16()
    do = torch.randn(B, Lq, d, device="cuda", generator=g).bfloat16()
    k, v = kbuf[:, front:front + Lk], vbuf[:, front:front + Lk]                    # views: the batch stride stays cap * d
    qr, kr, vr = (t.float().view(B, -1, H, 128).transpose(1, 2).detach().requires_grad_(True)
                  for t in (q, k.contiguous(), v.contiguous()))
    s = torch.einsum("bhid,bhjd->bhij", qr, kr) * 128 ** -0.5
    out = torch.einsum("bhij,bhjd->bhid", torch.softmax(s, dim=-1), vr)
    out.backward(do.float().view(B, Lq, H, 128).transpose(1, 2))
    flat = lambda t, L: t.grad.transpose(1, 2).reshape(B, L, d)
    ref = (flat(qr, Lq).reshape(B * Lq, d), flat(kr, Lk)[:, own_lo:].reshape(-1, d), flat(vr, Lk)[:, own_lo:].reshape(-1, d))
    del s, out
    # the forward the cached rollout runs: V^T with its pitch, the short kernel, lse and o32
    Lp = (Lk + 63) // 64 * 64
    vt = torch.zeros(B, d, Lp, device="cuda", dtype=torch.bfloat16)
    vt[:, :, :Lk] = v.transpose(1, 2)
    fwd = {}
    for pre in (0, 1):
        qq = q if not pre else (q.float() * (128 ** -0.5 * LOG2E)).bfloat16()
        o = torch.empty(B * Lq, d, device="cuda", dtype=torch.bfloat16)
        o32 = torch.empty(B * Lq, d, device="cuda", dtype=torch.float32)
        lse = torch.empty(B, H, Lq, device="cuda", dtype=torch.float32)
        ops.flash_attn_raw(ops.ptr(qq), ops.ptr(k), ops.ptr(vt), ops.ptr(o), None, B, H, Lq, Lk, Lq * d, d, cap * d, d,
                           d * Lp, Lq * d, d, Lp, 128 ** -0.5, lse=ops.ptr(lse), q_prescaled=pre, o32=ops.ptr(o32),
                           flags=ops.ATTN_SHORT_KERNEL)
        fwd[pre] = (qq.view(B * Lq, d), o, o32, lse)
    _CACHE[idx] = (k, v, do.view(B * Lq, d), fwd, ref)
    return _CACHE[idx]


def _bwd(ops, idx, pre=0, **kw):
    B, H, Lq, Lk, own_lo, front, cap = CASES[idx]
    k, v, do, fwd, _ = _case(idx, ops)
    q, o, o32, lse = fwd[pre]
    return ops.flash_attn_bwd(q, k, v, o, do, lse, None, B, H, Lq, Lk, o32=o32, q_prescaled=bool(pre), own_lo=own_lo,
                              k_bs=cap * H * 128, **kw)


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_cached_backward_against_autograd(ops, idx):
    B, H, Lq, Lk, own_lo, front, cap = CASES[idx]
    d = H * 128
    ref = _case(idx, ops)[4]
    got = _bwd(ops, idx)
    assert got[0].shape == (B * Lq, d) and got[1].shape == got[2].shape == (B * (Lk - own_lo), d)
    for name, gt, rf in zip(("dq", "dk", "dv"), got, ref):
        err = rel_rms(gt, rf)
        print(f"case {idx}: {name} rel-RMS {err:.2e}")
        assert torch.isfinite(gt).all()
        assert err < GRAD_RMS, name
    for a, b in zip(_bwd(ops, idx), got):                                    # no atomics: repeatable bit for bit
        assert torch.equal(a, b)
    # the pre-scaled q of the model's call and bf16 outputs: the same gradients within the formats' bounds
    out = tuple(torch.empty(B * L, d, device="cuda", dtype=torch.bfloat16) for L in (Lq, Lk - own_lo, Lk - own_lo))
    _bwd(ops, idx, pre=1, out=out)
    for name, gt, rf in zip(("dq", "dk", "dv"), out, ref):
        print(f"case {idx}: pre-scaled bf16 {name} rel-RMS {rel_rms(gt.float(), rf):.2e}")
        assert rel_rms(gt.float(), rf) < GRAD_RMS, name
    plain = _bwd(ops, idx, pre=1)
    for gt, rf in zip(out, plain):
        assert rel_rms(gt.float(), rf) < BF16_RMS


def test_own_lo_zero_is_the_plain_entry(ops):
    B, H, Lq, Lk, own_lo, front, cap = CASES[PLAIN]
    k, v, do, fwd, _ = _case(PLAIN, ops)
    q, o, o32, lse = fwd[0]
    plain = ops.flash_attn_bwd(q, k.reshape(B * Lk, -1), v.reshape(B * Lk, -1), o, do, lse, None, B, H, Lq, Lk, o32=o32)
    for a, b in zip(_bwd(ops, PLAIN), plain):
        assert torch.equal(a, b)


@pytest.mark.parametrize("idx", [0, OFFSET, REAL])
def test_phases_and_untouched_rows(ops, idx):
    """Phases 1 + 2 + 3 give phase 0's bits (with and without the split workspace), and the dK / dV pass writes rows
    [0, Lk - own_lo) of its buffers and nothing around them."""
    B, H, Lq, Lk, own_lo, front, cap = CASES[idx]
    d, Lown = H * 128, Lk - own_lo
    bf = lambda rows: torch.full((rows, d), float("nan"), device="cuda", dtype=torch.bfloat16)
    for split in (True, False):                                              # (a split pass adds its slabs: other bits)
        whole = (bf(B * Lq), bf(B * Lown), bf(B * Lown))
        _bwd(ops, idx, out=whole, split=split)
        delta = torch.empty(B, H, Lq, device="cuda", dtype=torch.float32)
        ph = (bf(B * Lq), bf(B * Lown), bf(B * Lown))
        _bwd(ops, idx, phase=1, delta=delta, out=ph, split=split)
        assert all(bool(torch.isnan(t.float()).all()) for t in ph)           # phase 1 writes delta only
        _bwd(ops, idx, phase=3, delta=delta, out=ph, split=split)
        assert bool(torch.isnan(ph[0].float()).all())                        # phase 3: dk, dv, not dq
        _bwd(ops, idx, phase=2, delta=delta, out=ph, split=split)
        for a, b in zip(ph, whole):
            assert torch.equal(a, b), split
    if B == 1:                                                               # (whole: the unsplit pass, like this one)
        pad = 8
        dkb, dvb = bf(Lown + 2 * pad), bf(Lown + 2 * pad)
        _bwd(ops, idx, out=(bf(Lq), dkb[pad:pad + Lown], dvb[pad:pad + Lown]), split=False)
        for buf, ref in ((dkb, whole[1]), (dvb, whole[2])):
            assert torch.equal(buf[pad:pad + Lown], ref)
            assert bool(torch.isnan(buf[:pad].float()).all()) and bool(torch.isnan(buf[pad + Lown:].float()).all())


def test_own_lo_argument_rules(ops):
    B, H, Lq, Lk, own_lo, front, cap = CASES[0]
    k, v, do, fwd, _ = _case(0, ops)
    q, o, o32, lse = fwd[0]
    call = lambda **kw: ops.flash_attn_bwd(q, k, v, o, do, lse, kw.pop("k_lens", None), B, H, Lq, Lk,
                                           **{"o32": o32, "own_lo": own_lo, **kw})
    with pytest.raises(ValueError):
        call(own_lo=4)
    with pytest.raises(ValueError):
        call(own_lo=Lk)
    with pytest.raises(ValueError):
        call(o32=None)
    with pytest.raises(ValueError):
        call(k_lens=torch.full((B,), Lk, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        call(window=(16, -1))
    with pytest.raises(ValueError):
        call(chunk_causal=(56, -1, 0))


# ----------------------------------------------------------------------------- ops.flow_x0_step
def _ulp_equal(a, b):
    """|a - b| <= 1 ulp of b, elementwise."""
    b = b.float()
    ulp = (torch.nextafter(b.abs(), torch.full_like(b, float("inf"))) - b.abs())
    return bool(((a.float() - b).abs() <= ulp).all())


@pytest.mark.parametrize("B,shape", [(2, (16, 1, 14, 16)), (3, (1001,)), (1, (5,))])
def test_flow_x0_step(ops, B, shape):
    """n = 3 584 (whole vectors), n = 1 001 with B = 3 and three different sigma (vectors straddle the samples, a live
    scalar tail), and a launch smaller than one vector per thread."""
    g = torch.Generator(device="cuda").manual_seed(5)
    v, x, eps = (torch.randn(B, *shape, device="cuda", generator=g) for _ in range(3))
    sig = torch.tensor([0.9, 0.35, 0.05][:B], device="cuda")
    nxt = torch.tensor([0.6, 0.2, 0.0][:B], device="cuda")
    col = lambda s: s.view(B, *([1] * len(shape)))
    want0 = x - col(sig) * v
    want1 = (1 - col(nxt)) * want0 + col(nxt) * eps
    x0 = ops.flow_x0_step(v, x, sig)                                         # eps absent
    assert x0.shape == v.shape and _ulp_equal(x0, want0)
    a, b = ops.flow_x0_step(v, x, sig, eps, nxt)
    assert torch.equal(a, x0) and _ulp_equal(b, want1)
    if B == 3:
        assert not _ulp_equal(ops.flow_x0_step(v, x, sig.flip(0)), want0)    # the sigma of each sample is its own
    # unaligned views of a larger buffer: everything through the scalar path, the same bits
    big = torch.randn(3, v.numel() + 1, device="cuda", generator=g)
    vv, xx = big[0, 1:].view_as(v), big[1, 1:].view_as(v)
    assert vv.data_ptr() % 16 != 0
    assert torch.equal(ops.flow_x0_step(vv.contiguous(), xx.contiguous(), sig),
                       ops._flow_x0_raw(vv, xx, sig)[0])
    # backward: dv = -sigma_b g, nothing for x
    vg, xg = v.clone().requires_grad_(True), x.clone().requires_grad_(True)
    gout = torch.randn(B, *shape, device="cuda", generator=g)
    out = ops.flow_x0_step(vg, xg, sig)
    out.backward(gout)
    assert xg.grad is None and _ulp_equal(vg.grad, -col(sig) * gout)
    assert torch.equal(out.detach(), x0)
