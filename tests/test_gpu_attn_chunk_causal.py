"""Chunk-causal attention (the staircase over frame groups), forward and backward: omh_flash_attn_fwd_chunk_d128 /
omh_flash_attn_bwd_chunk_d128 through ``ops.flash_attn(chunk_causal=)``, ``flash_attention(chunk_causal=)`` and
``ops.flash_attn_func(chunk_causal=)`` against autograd through a dense-masked fp32 softmax attention on the same bf16
operands (built as in test_gpu_attn_block_sparse.py).  The mask is ``causal.chunk_causal_visible``: query i sees key j iff
``i < qlen``, ``j < klen``, ``j // C <= (P + i) // C`` and (``W < 0`` or ``j // C >= (P + i) // C - W``).

Bounds: the project's own for this arithmetic (P and the output in bf16): forward rel-RMS < 8e-3 and max abs error
< 3e-2 (test_gpu_kernels.py), attention gradients rel-RMS < 1.2e-2 (test_gpu_attn_band_bwd.py)."""
import importlib

import pytest
import torch

from conftest import PKG, rel_rms, set_option

pytestmark = pytest.mark.gpu
FWD_RMS, FWD_MAX, GRAD_RMS = 8e-3, 3e-2, 1.2e-2


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


@pytest.fixture(scope="module")
def causal():
    return importlib.import_module(PKG + ".causal")


@pytest.fixture(scope="module")
def attn_mod():
    return importlib.import_module(PKG + ".wan.modules.attention")


CASES = [
    # B, H, Lq, Lk, k_lens, q_lens, C, W, P
    (1, 2, 256, 256, None, None, 64, -1, 0),                  # edges on tile edges
    (2, 2, 320, 320, [280, 168], None, 56, -1, 0),            # edges inside tiles, ragged batch
    (2, 2, 320, 320, [280, 168], None, 112, 1, 0),            # bounded look-back
    (1, 2, 130, 333, [250], [100], 24, 2, 200),               # Lq != Lk, an offset, NaN dout past row 100; every live row sees a key
    (1, 12, 4680, 4680, None, None, 1560, -1, 0),             # a real chunk (3 x 1560), 12 heads through xcd_remap
    (1, 2, 300, 300, None, None, 300, -1, 0),                 # full attention
    (1, 2, 130, 333, [200], [100], 24, 0, 200),               # live rows past position 215 see no key (their chunk starts at 216)
]
FULL, BLIND = 5, 6
_CACHE = {}


def _case(idx, causal):
    """Inputs, the fp32 reference (output, liveness, gradients) — computed once per case and left unchanged."""
    if idx in _CACHE:
        return _CACHE[idx]
    B, H, Lq, Lk, klens, qlens, C, W, P = CASES[idx]
    g = torch.Generator(device="cuda").manual_seed(300 + idx)
    q, k, v = (torch.randn(B, L, H, 128, device="cuda", generator=g).bfloat16() for L in (Lq, Lk, Lk))
    do = torch.randn(B, Lq, H, 128, device="cuda", generator=g).bfloat16()
    vis = torch.stack([causal.chunk_causal_visible(Lq, Lk, C, W, P, None if qlens is None else qlens[b],
                                                   None if klens is None else klens[b]) for b in range(B)])
    vis = vis.cuda()[:, None]                                                      # [B, 1, Lq, Lk]
    if qlens is not None:
        for b in range(B):
            do[b, qlens[b]:] = float("nan")                                        # nothing may depend on those rows
    qr, kr, vr = (t.float().transpose(1, 2).detach().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bhid,bhjd->bhij", qr, kr) * 128 ** -0.5
    s = s.masked_fill(~vis, float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)                         # rows that see no key
    out = torch.einsum("bhij,bhjd->bhid", p, vr)
    out.backward(torch.nan_to_num(do.float(), nan=0.0).transpose(1, 2))
    ref = dict(out=out.detach().transpose(1, 2).contiguous(),
               grads=tuple(t.grad.transpose(1, 2).contiguous() for t in (qr, kr, vr)),
               row_live=vis.any(3).expand(B, H, Lq).contiguous(),                  # [B, H, Lq]: the row sees a key
               key_live=vis.any(2).expand(B, H, Lk).contiguous())                  # [B, H, Lk]: a live query sees the key
    del s, p, out, vis
    kl = None if klens is None else torch.tensor(klens, dtype=torch.int32, device="cuda")
    ql = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device="cuda")
    _CACHE[idx] = (q, k, v, do, kl, ql, (C, W, P), ref)
    return _CACHE[idx]


def _vt(v):
    B, Lk, H, D = v.shape
    Lp = (Lk + 63) // 64 * 64
    vt = torch.zeros(B, H * D, Lp, device="cuda", dtype=torch.bfloat16)
    vt[:, :, :Lk] = v.reshape(B, Lk, H * D).transpose(1, 2)
    return vt


def test_blind_case_has_live_rows_that_see_nothing(causal):
    """On the CPU, before relying on them: the last case has rows below q_lens whose chunk holds no key below k_lens,
    and the fourth has none."""
    for idx, expect in ((3, False), (BLIND, True)):
        B, H, Lq, Lk, klens, qlens, C, W, P = CASES[idx]
        vis = causal.chunk_causal_visible(Lq, Lk, C, W, P, qlens[0], klens[0])
        blind = ~vis[:qlens[0]].any(1)
        assert bool(blind.any()) == expect


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_chunk_causal_forward(ops, causal, attn_mod, idx):
    B, H, Lq, Lk = CASES[idx][:4]
    q, k, v, do, kl, ql, rule, ref = _case(idx, causal)
    lse = torch.full((B, H, Lq), float("nan"), device="cuda")
    o = ops.flash_attn(q, k, _vt(v), kl, q_lens=ql, chunk_causal=rule, lse=lse)
    err_rms, err_max = rel_rms(o, ref["out"]), float((o.float() - ref["out"]).abs().max())
    print(f"case {idx}: forward rel-RMS {err_rms:.2e} max abs {err_max:.2e}")
    assert torch.isfinite(o.float()).all()
    assert err_rms < FWD_RMS and err_max < FWD_MAX
    # rows that see no key: exact zeros and lse = -inf; every other row a finite lse
    live = ref["row_live"]                                                   # [B, H, Lq]
    assert float(o.float().transpose(1, 2)[~live].abs().sum()) == 0.0
    assert bool((lse[~live] == float("-inf")).all()) and bool(torch.isfinite(lse[live]).all())
    # the wrapper with the reference's signature, and a second run: the same bits
    with torch.no_grad():
        ow = attn_mod.flash_attention(q, k, v, q_lens=ql, k_lens=kl, chunk_causal=rule)
    assert torch.equal(ow, o)
    assert torch.equal(ops.flash_attn(q, k, _vt(v), kl, q_lens=ql, chunk_causal=rule), o)
    if idx == FULL:                                                          # C >= max(Lk, P + Lq), W < 0: the plain kernel's bits
        set_option("OMH_ATTN_KERNEL", "base")
        assert torch.equal(o, ops.flash_attn(q, k, _vt(v), kl))
        assert torch.equal(o, ops.flash_attn(q, k, _vt(v), kl, chunk_causal=(2 ** 31 - 1, -1, 0)))


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_chunk_causal_backward(ops, causal, attn_mod, idx):
    B, H, Lq, Lk = CASES[idx][:4]
    q, k, v, do, kl, ql, rule, ref = _case(idx, causal)

    def run(through_wrapper=False):
        qg, kg, vg = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        if through_wrapper:
            attn_mod.flash_attention(qg, kg, vg, q_lens=ql, k_lens=kl, chunk_causal=rule).backward(do)
        else:
            ops.flash_attn_func(qg, kg, vg, kl, ql, chunk_causal=rule).backward(do)
        return qg.grad, kg.grad, vg.grad

    got = run()
    for name, gt, rf in zip(("dq", "dk", "dv"), got, ref["grads"]):
        err = rel_rms(gt, rf)
        print(f"case {idx}: {name} rel-RMS {err:.2e}")
        assert torch.isfinite(gt.float()).all()
        assert err < GRAD_RMS, name
    # rows that see no key (dead queries included) and keys no live query sees: exact zeros, written
    assert float(got[0].float().transpose(1, 2)[~ref["row_live"]].abs().sum()) == 0.0
    dead_k = ~ref["key_live"]
    assert float(got[1].float().transpose(1, 2)[dead_k].abs().sum()) == 0.0
    assert float(got[2].float().transpose(1, 2)[dead_k].abs().sum()) == 0.0
    for a, b in zip(run(), got):                                             # no atomics: repeatable bit for bit
        assert torch.equal(a, b)
    for a, b in zip(run(through_wrapper=True), got):                         # flash_attention(chunk_causal=) is differentiable
        assert torch.equal(a, b)


@pytest.mark.parametrize("idx", [2, 3])
def test_chunk_causal_backward_modes(ops, causal, idx):
    """bf16 outputs and q_prescaled agree with the plain call; phases 1 + 2 + 3 give phase 0's bits."""
    B, H, Lq, Lk = CASES[idx][:4]
    q4, k4, v4, do4, kl, ql, rule, _ = _case(idx, causal)
    d = H * 128
    q, k, v, do = q4.view(B * Lq, d), k4.view(B * Lk, d), v4.view(B * Lk, d), do4.view(B * Lq, d)
    vt = _vt(v4)
    LOG2E = 1.4426950408889634

    def forward(qq, pre):
        o = torch.empty(B * Lq, d, device="cuda", dtype=torch.bfloat16)
        o32 = torch.empty(B * Lq, d, device="cuda", dtype=torch.float32)
        lse = torch.empty(B, H, Lq, device="cuda", dtype=torch.float32)
        ops.flash_attn_raw(ops.ptr(qq), ops.ptr(k), ops.ptr(vt), ops.ptr(o), ops.ptr(kl), B, H, Lq, Lk, Lq * d, d, Lk * d, d,
                           d * vt.shape[2], Lq * d, d, vt.shape[2], 128 ** -0.5, lse=ops.ptr(lse), q_prescaled=pre,
                           o32=ops.ptr(o32), q_lens=None if ql is None else ops.ptr(ql), chunk_causal=rule)
        return o, o32, lse

    o, o32, lse = forward(q, 0)
    kw = dict(o32=o32, chunk_causal=rule, q_lens=ql)
    dq, dk, dv = ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, **kw)
    out = tuple(torch.empty(B * L, d, device="cuda", dtype=torch.bfloat16) for L in (Lq, Lk, Lk))
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, out=out, **kw)
    for got, ref in zip(out, (dq, dk, dv)):
        assert rel_rms(got.float(), ref) < 8e-3
    qp = (q.float() * (128 ** -0.5 * LOG2E)).bfloat16()
    op, o32p, lsep = forward(qp, 1)
    gp = ops.flash_attn_bwd(qp, k, v, op, do, lsep, kl, B, H, Lq, Lk, q_prescaled=True, o32=o32p, chunk_causal=rule, q_lens=ql)
    for got, ref in zip(gp, (dq, dk, dv)):
        assert rel_rms(got, ref) < GRAD_RMS
    delta = torch.empty(B, H, Lq, device="cuda", dtype=torch.float32)
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, phase=1, out=None, delta=delta, **kw)
    ph = [torch.full((B * L, d), float("nan"), device="cuda", dtype=torch.bfloat16) for L in (Lq, Lk, Lk)]
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, phase=3, out=tuple(ph), delta=delta, **kw)
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, phase=2, out=tuple(ph), delta=delta, **kw)
    for a, b in zip(ph, out):
        assert torch.equal(a, b)


def test_rollout_slice_is_the_staircase_row_block(ops, causal):
    """What WanModel.forward_chunk relies on: plain attention of one chunk's rows over the keys from the look-back's first
    token to the chunk's end — K and V^T addressed by a pointer offset into longer buffers — gives the rows the staircase
    kernel gives on the whole sequence, up to the key tiling (the tiles start at the look-back here, at 0 there)."""
    B, H, C, n = 1, 2, 56, 5
    L = C * n
    g = torch.Generator(device="cuda").manual_seed(11)
    q, k, v = (torch.randn(B, L, H, 128, device="cuda", generator=g).bfloat16() for _ in range(3))
    vt = _vt(v)
    full = ops.flash_attn(q, k, vt, chunk_causal=(C, 1, 0))
    d, pitch = H * 128, vt.shape[2]
    for c in range(n):
        lo, hi = max(0, c - 1) * C, (c + 1) * C
        o = torch.empty(B, C, H, 128, device="cuda", dtype=torch.bfloat16)
        ops.flash_attn_raw(ops.ptr(q, c * C * d), ops.ptr(k, lo * d), ops.ptr(vt, lo), ops.ptr(o), None, B, H, C, hi - lo,
                           L * d, d, L * d, d, d * pitch, C * d, d, pitch, 128 ** -0.5, flags=ops.ATTN_SHORT_KERNEL)
        assert rel_rms(o, full[:, c * C:(c + 1) * C]) < 4e-3, c


def test_chunk_causal_refuses_other_masks(ops, attn_mod):
    q = torch.randn(1, 256, 2, 128, device="cuda").bfloat16()
    mask = torch.ones(2, 2, dtype=torch.bool)
    with pytest.raises(ValueError):
        attn_mod.flash_attention(q, q, q, causal=True, chunk_causal=(64, -1, 0))
    with pytest.raises(ValueError):
        attn_mod.flash_attention(q, q, q, window_size=(16, 16), chunk_causal=(64, -1, 0))
    with pytest.raises(ValueError):
        attn_mod.flash_attention(q, q, q, block_mask=mask, chunk_causal=(64, -1, 0))
    with pytest.raises(ValueError):
        ops.flash_attn_func(q, q, q, window=(16, -1), chunk_causal=(64, -1, 0))
    with pytest.raises(ValueError):
        ops.flash_attn(q, q, _vt(q), block_mask=mask, chunk_causal=(64, -1, 0))
    with pytest.raises(ValueError):
        ops.flash_attn(q, q, _vt(q), chunk_causal=(0, -1, 0))
    with pytest.raises(ValueError):
        ops.flash_attn(q, q, _vt(q), chunk_causal=(64, -1, -8))
