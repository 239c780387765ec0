"""Interval-mask attention with one group size per axis (``causal.IntervalMask(k_group=)``), forward and backward:
omh_flash_attn_fwd_interval_rect_d128 / omh_flash_attn_bwd_interval_rect_d128 through ``ops.flash_attn(interval_mask=)``,
``flash_attention(interval_mask=)`` and ``ops.flash_attn_func(interval_mask=)`` against autograd through a dense-masked
fp32 softmax attention on the same bf16 operands (built as in test_gpu_attn_interval.py).  The mask is
``causal.interval_visible``: query i sees key j iff ``i < qlen``, ``j < klen`` and ``vis[i // q_group, j // k_group]`` — the
cross-attention of a video onto frame-aligned condition tokens (``causal.condition_window_visible``): a query group is a
latent frame, a key group one token (or a few).

Bounds: those of test_gpu_attn_interval.py (P and the output in bf16): forward rel-RMS < 8e-3 and max abs error < 3e-2,
attention gradients rel-RMS < 1.2e-2."""
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


def _window(frames, per_frame, n_global, n_text, back, ahead, k_group=1, segments=1):
    """The matrix of `frames` latent frames on `per_frame` tokens each (ascending), `n_global` tokens of frame -1 and
    `n_text` text tokens, one column per key group of `k_group` tokens (every group lies inside one kind of token)."""
    def make(c):
        tf = [f for f in range(frames) for _ in range(per_frame)] + [-1] * n_global
        vis = c.condition_window_visible(frames, torch.tensor(tf), n_text, back, ahead, segments=segments)
        assert per_frame % k_group == 0 and n_global % k_group == 0 and n_text % k_group == 0
        return vis[:, ::k_group]
    return make


def _hand(c):
    """3 query groups of 40 rows (the last one partial: 100 rows; q_lens = 80 leaves it dead) on 40 key groups of 5: row 0
    sees the key groups [0, 10) and [12, 40), row 1 nothing, row 2 all — so key groups 10 and 11 are seen by no live row."""
    vis = torch.zeros(3, 40, dtype=torch.bool)
    vis[0, :10] = True
    vis[0, 12:] = True
    vis[2] = True
    return vis


CASES = [
    # B, H, Lq, Lk, k_lens, q_lens, q_group, k_group, matrix
    (1, 2, 256, 64, None, None, 64, 1, _window(4, 3, 2, 50, 0, 0)),               # one key tile, masked per element throughout
    (2, 2, 560, 272, [272, 230], None, 56, 1, _window(10, 7, 2, 200, 1, 1)),      # ends inside tiles, several query groups per workgroup, ragged text
    (1, 2, 960, 384, None, None, 24, 8, _window(40, 8, 0, 64, 0, 0, k_group=8)),  # key tiles 1-4 skipped by the first query workgroup
    (1, 2, 448, 32, None, None, 56, 1, _window(4, 3, 0, 20, 1, 0, segments=2)),   # teacher forcing: k_iv rows with two separate runs
    (1, 2, 100, 200, [190], [80], 40, 5, _hand),                                  # partial last group, a blind live group, dead keys, NaN dout
    (1, 2, 240, 240, None, None, 40, 40, lambda c: c.sink_window_groups(6, 1, 1)),   # equal groups: the interval entry's bits
    (1, 12, 4680, 536, [500], None, 1560, 1, _window(3, 8, 0, 512, 1, 0)),        # the real chunk, 12 heads
    (1, 2, 300, 200, None, None, 300, 200, lambda c: torch.tensor([[1]])),        # full attention: the plain kernel's bits
]
TF, HAND, EQUAL, FULL = 3, 4, 5, 7
_CACHE = {}


def _case(idx, causal):
    """Inputs, the mask, the fp32 reference (output, liveness, gradients) — computed once per case and left unchanged."""
    if idx in _CACHE:
        return _CACHE[idx]
    B, H, Lq, Lk, klens, qlens, qg, kg, make = CASES[idx]
    mask = causal.IntervalMask(make(causal), qg, "cuda", k_group=kg)
    g = torch.Generator(device="cuda").manual_seed(900 + idx)
    q, k, v = (torch.randn(B, L, H, 128, device="cuda", generator=g).bfloat16() for L in (Lq, Lk, Lk))
    do = torch.randn(B, Lq, H, 128, device="cuda", generator=g).bfloat16()
    vis = torch.stack([causal.interval_visible(mask, Lq, Lk, None if qlens is None else qlens[b],
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
    _CACHE[idx] = (q, k, v, do, kl, ql, mask, ref)
    return _CACHE[idx]


def _vt(v):
    B, Lk, H, D = v.shape
    Lp = (Lk + 63) // 64 * 64
    vt = torch.zeros(B, H * D, Lp, device="cuda", dtype=torch.bfloat16)
    vt[:, :, :Lk] = v.reshape(B, Lk, H * D).transpose(1, 2)
    return vt


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_rect_forward(ops, causal, attn_mod, idx):
    B, H, Lq, Lk = CASES[idx][:4]
    q, k, v, do, kl, ql, mask, ref = _case(idx, causal)
    lse = torch.full((B, H, Lq), float("nan"), device="cuda")
    o = ops.flash_attn(q, k, _vt(v), kl, q_lens=ql, interval_mask=mask, lse=lse)
    err_rms, err_max = rel_rms(o, ref["out"]), float((o.float() - ref["out"]).abs().max())
    print(f"case {idx}: forward rel-RMS {err_rms:.2e} max abs {err_max:.2e}")
    assert torch.isfinite(o.float()).all()
    assert err_rms < FWD_RMS and err_max < FWD_MAX
    # rows that see no key: exact zeros and lse = -inf; every other row a finite lse
    live = ref["row_live"]                                                   # [B, H, Lq]
    assert float(o.float().transpose(1, 2)[~live].abs().sum()) == 0.0
    assert bool((lse[~live] == float("-inf")).all()) and bool(torch.isfinite(lse[live]).all())
    if idx == HAND:
        assert bool((~live).any())
    # the wrapper with the reference's signature, and a second run: the same bits
    with torch.no_grad():
        ow = attn_mod.flash_attention(q, k, v, q_lens=ql, k_lens=kl, interval_mask=mask)
    assert torch.equal(ow, o)
    assert torch.equal(ops.flash_attn(q, k, _vt(v), kl, q_lens=ql, interval_mask=mask), o)
    if idx == EQUAL:                                                         # q_group == k_group: the interval entry's bits
        square = causal.IntervalMask(mask.vis, mask.group, "cuda")
        assert torch.equal(o, ops.flash_attn(q, k, _vt(v), kl, q_lens=ql, interval_mask=square))
    if idx == FULL:                                                          # vis = [[1]]: the plain kernel's bits
        set_option("OMH_ATTN_KERNEL", "base")
        assert torch.equal(o, ops.flash_attn(q, k, _vt(v), kl))


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_rect_backward(ops, causal, attn_mod, idx):
    B, H, Lq, Lk = CASES[idx][:4]
    q, k, v, do, kl, ql, mask, ref = _case(idx, causal)

    def run(through_wrapper=False, m=mask):
        qg, kg, vg = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        if through_wrapper:
            attn_mod.flash_attention(qg, kg, vg, q_lens=ql, k_lens=kl, interval_mask=m).backward(do)
        else:
            ops.flash_attn_func(qg, kg, vg, kl, ql, interval_mask=m).backward(do)
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
    if idx == HAND:
        assert bool(dead_k[..., :190].any())
    assert float(got[1].float().transpose(1, 2)[dead_k].abs().sum()) == 0.0
    assert float(got[2].float().transpose(1, 2)[dead_k].abs().sum()) == 0.0
    for a, b in zip(run(), got):                                             # no atomics: repeatable bit for bit
        assert torch.equal(a, b)
    for a, b in zip(run(through_wrapper=True), got):                         # flash_attention(interval_mask=) is differentiable
        assert torch.equal(a, b)
    if idx == EQUAL:                                                         # q_group == k_group: the interval entry's bits
        for a, b in zip(run(m=causal.IntervalMask(mask.vis, mask.group, "cuda")), got):
            assert torch.equal(a, b)


@pytest.mark.parametrize("idx", [1, HAND])
def test_rect_backward_modes(ops, causal, idx):
    """bf16 outputs and q_prescaled agree with the plain call; phases 1 + 2 + 3 give phase 0's bits; the forward without
    lse writes the same output."""
    B, H, Lq, Lk = CASES[idx][:4]
    q4, k4, v4, do4, kl, ql, mask, _ = _case(idx, causal)
    d = H * 128
    q, k, v, do = q4.view(B * Lq, d), k4.view(B * Lk, d), v4.view(B * Lk, d), do4.view(B * Lq, d)
    vt = _vt(v4)
    LOG2E = 1.4426950408889634

    def forward(qq, pre, with_lse=True):
        o = torch.empty(B * Lq, d, device="cuda", dtype=torch.bfloat16)
        o32 = torch.empty(B * Lq, d, device="cuda", dtype=torch.float32)
        lse = torch.empty(B, H, Lq, device="cuda", dtype=torch.float32)
        ops.flash_attn_raw(ops.ptr(qq), ops.ptr(k), ops.ptr(vt), ops.ptr(o), ops.ptr(kl), B, H, Lq, Lk, Lq * d, d, Lk * d, d,
                           d * vt.shape[2], Lq * d, d, vt.shape[2], 128 ** -0.5, lse=ops.ptr(lse) if with_lse else None,
                           q_prescaled=pre, o32=ops.ptr(o32), q_lens=None if ql is None else ops.ptr(ql), interval_mask=mask)
        return o, o32, lse

    o, o32, lse = forward(q, 0)
    assert torch.equal(forward(q, 0, with_lse=False)[0], o)
    kw = dict(o32=o32, interval_mask=mask, q_lens=ql)
    dq, dk, dv = ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, **kw)
    out = tuple(torch.empty(B * L, d, device="cuda", dtype=torch.bfloat16) for L in (Lq, Lk, Lk))
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, out=out, **kw)
    for got, ref in zip(out, (dq, dk, dv)):
        assert rel_rms(got.float(), ref) < 8e-3
    qp = (q.float() * (128 ** -0.5 * LOG2E)).bfloat16()
    op, o32p, lsep = forward(qp, 1)
    gp = ops.flash_attn_bwd(qp, k, v, op, do, lsep, kl, B, H, Lq, Lk, q_prescaled=True, o32=o32p, interval_mask=mask, q_lens=ql)
    for got, ref in zip(gp, (dq, dk, dv)):
        assert rel_rms(got, ref) < GRAD_RMS
    delta = torch.empty(B, H, Lq, device="cuda", dtype=torch.float32)
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, phase=1, out=None, delta=delta, **kw)
    ph = [torch.full((B * L, d), float("nan"), device="cuda", dtype=torch.bfloat16) for L in (Lq, Lk, Lk)]
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, phase=3, out=tuple(ph), delta=delta, **kw)
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, phase=2, out=tuple(ph), delta=delta, **kw)
    for a, b in zip(ph, out):
        assert torch.equal(a, b)


def test_rect_refusals(ops, causal, attn_mod):
    """k_group 0, q_group 7, wrong group counts, a band beside the mask, runs=3 with k_group: the Python layers raise
    ValueError, the C entries return OMH_E_BADARG before any launch."""
    import ctypes as C
    _lib = importlib.import_module(PKG + "._lib")
    vis = causal.condition_window_visible(4, torch.tensor([0, 1, 2, 3]), 60, 0, 0)
    with pytest.raises(ValueError):
        causal.IntervalMask(vis, 64, k_group=0)
    with pytest.raises(ValueError):
        causal.IntervalMask(vis, 7, k_group=1)
    with pytest.raises(ValueError):
        causal.IntervalMask(vis, 64, runs=3, k_group=1)
    m = causal.IntervalMask(vis, 64, "cuda", k_group=1)
    q = torch.randn(1, 256, 2, 128, device="cuda").bfloat16()
    k = torch.randn(1, 64, 2, 128, device="cuda").bfloat16()
    with pytest.raises(ValueError):
        attn_mod.flash_attention(q, k, k, window_size=(16, 16), interval_mask=m)
    with pytest.raises(ValueError):
        ops.flash_attn_func(q, k, k, window=(16, -1), interval_mask=m)
    with pytest.raises(ValueError):                                              # 4 x 64 groups do not cover 256 x 128
        ops.flash_attn(q, torch.cat([k, k], 1), _vt(torch.cat([k, k], 1)), interval_mask=m)
    with pytest.raises(ValueError):                                              # nor 320 x 64
        ops.flash_attn(torch.cat([q, q[:, :64]], 1), k, _vt(k), interval_mask=m)
    # the C entries themselves
    vt, o = _vt(k), torch.empty_like(q)
    d = 256

    def args(**kw):
        a = _lib.AttnArgs(ops.ptr(q), ops.ptr(k), ops.ptr(vt), ops.ptr(o), None, 1, 2, 256, 64, 256 * d, d, 64 * d, d,
                          d * vt.shape[2], 256 * d, d, vt.shape[2], 128 ** -0.5, None, 0, None, 0, None, 0, None)
        for key, val in kw.items():
            setattr(a, key, val)
        return a

    def rect(qg=64, kg=1, nq=4, nk=64):
        return _lib.IntervalRectMaskArgs(qg, kg, nq, nk, m.q_iv.data_ptr(), m.k_iv.data_ptr())

    fwd = _lib.lib.omh_flash_attn_fwd_interval_rect_d128
    for bad in (rect(kg=0), rect(qg=7), rect(nq=5), rect(nk=63), rect(kg=2)):
        assert fwd(C.byref(args()), C.byref(bad), None) == -1
    assert fwd(C.byref(args(window_left=4, window_right=0)), C.byref(rect()), None) == -1
    assert fwd(C.byref(args()), None, None) == -1
    torch.cuda.synchronize()
    assert fwd(C.byref(args()), C.byref(rect()), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(o, ops.flash_attn(q, k, vt, interval_mask=m))
