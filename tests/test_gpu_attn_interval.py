"""Interval-mask attention (up to two key intervals per group of query rows), forward and backward:
omh_flash_attn_fwd_interval_d128 / omh_flash_attn_bwd_interval_d128 through ``ops.flash_attn(interval_mask=)``,
``flash_attention(interval_mask=)`` and ``ops.flash_attn_func(interval_mask=)`` against autograd through a dense-masked
fp32 softmax attention on the same bf16 operands (built as in test_gpu_attn_chunk_causal.py).  The mask is
``causal.interval_visible``: query i sees key j iff ``i < qlen``, ``j < klen`` and ``vis[i // group, j // group]``.

Bounds: the project's own for this arithmetic (P and the output in bf16): forward rel-RMS < 8e-3 and max abs error
< 3e-2, attention gradients rel-RMS < 1.2e-2 (test_gpu_attn_chunk_causal.py)."""
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


def _tf(n, W=-1):
    return lambda c: c.teacher_forcing_groups(n, W)


# Tables written by hand (not built from a matrix), (number of groups, row) pairs: rows with an EMPTY first slot and a live
# later one, bounds below 0 and above the other axis's group count (the kernels clamp them), and — group 8, Lq = 200,
# Lk = 328 — inside the first 128-row workgroup key tiles 1 and 2 (keys 64..191) between its two ranges, inside the first
# 128-key workgroup query tile 1 between its two.  HAND_K says of the key groups what HAND_Q says of the query groups.
HAND_Q = [(4, [-3, 6, 24, 30]), (4, [4, 6, 30, 30]), (4, [3, 3, 26, 46]), (4, [2, 2, 24, 26]), (4, [7, 7, 8, 17]),
          (5, [0, 4, 8, 17])]
HAND_K = [(4, [0, 4, 20, 99]), (2, [-2, 8, 8, 8]), (2, [0, 0, 0, 0]), (9, [9, 9, 16, 25]), (7, [0, 0, 0, 0]),
          (2, [0, 4, 12, 16]), (4, [0, 4, 8, 12]), (11, [8, 12, 12, 12])]


def hand_rows(pairs):
    return torch.tensor([row for n, row in pairs for _ in range(n)], dtype=torch.int32)


def table_matrix(rows, other):
    """The bool matrix [len(rows), other] a table says, read as the kernels read it: bounds clamped to [0, other]."""
    m = torch.zeros(rows.shape[0], other, dtype=torch.bool)
    for g, row in enumerate(rows.tolist()):
        for lo, hi in zip(row[0::2], row[1::2]):
            m[g, min(max(lo, 0), other):min(max(hi, 0), other)] = True
    return m


def hand_mask(causal, device="cpu"):
    """The IntervalMask of the matrix HAND_Q says, with the hand-written tables in place of the ones built from it."""
    q_rows, k_rows = hand_rows(HAND_Q), hand_rows(HAND_K)
    mask = causal.IntervalMask(table_matrix(q_rows, k_rows.shape[0]), 8)
    mask._host = (q_rows, k_rows)
    mask._move(torch.device(device))
    return mask


CASES = [
    # B, H, Lq, Lk, k_lens, q_lens, group, matrix
    (1, 2, 256, 256, None, None, 64, _tf(2)),                                    # interval ends on tile edges
    (2, 2, 560, 560, [560, 400], None, 56, _tf(5)),                              # ends inside tiles, ragged keys cutting the noisy half
    (1, 2, 192, 192, None, None, 24, _tf(4, 1)),                                 # several groups per tile and per workgroup, look-back
    (1, 2, 240, 240, None, None, 40, lambda c: c.sink_window_groups(6, 1, 1)),   # two intervals that merge for early rows
    (1, 2, 48, 240, [230], [40], 48, lambda c: torch.tensor([[1, 0, 0, 1, 1]])),  # Lq != Lk, NaN dout past row 40, two key groups nobody sees
    (1, 2, 120, 120, None, None, 40, lambda c: torch.tensor([[1, 0, 0], [0, 0, 0], [1, 1, 1]])),   # a live row group that sees nothing
    (2, 2, 320, 320, [280, 168], None, 56, lambda c: torch.ones(6, 6).tril()),   # the staircase, W = -1
    (1, 2, 300, 300, None, None, 300, lambda c: torch.tensor([[1]])),            # full attention
    (1, 12, 6240, 6240, None, None, 1560, _tf(2)),                               # a real chunk, 12 heads through xcd_remap
    (1, 2, 200, 328, None, None, 8, None),                                       # hand_mask: tables no matrix builds
]
DEAD_KEYS, BLIND, STAIRS, FULL, HAND = 4, 5, 6, 7, 9
_CACHE = {}


def _case(idx, causal):
    """Inputs, the mask, the fp32 reference (output, liveness, gradients) — computed once per case and left unchanged."""
    if idx in _CACHE:
        return _CACHE[idx]
    B, H, Lq, Lk, klens, qlens, group, make = CASES[idx]
    mask = hand_mask(causal, "cuda") if idx == HAND else causal.IntervalMask(make(causal), group, "cuda")
    g = torch.Generator(device="cuda").manual_seed(400 + idx)
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


def test_cases_hold_what_they_are_for(causal):
    """On the CPU, before relying on them: the blind case has live rows that see no key, the dead-key case whole key
    groups no live row sees, and the first teacher-forcing cases rows with two separate key intervals."""
    B, H, Lq, Lk, klens, qlens, group, make = CASES[BLIND]
    vis = causal.interval_visible(causal.IntervalMask(make(causal), group), Lq, Lk)
    assert bool((~vis.any(1)).any())
    B, H, Lq, Lk, klens, qlens, group, make = CASES[DEAD_KEYS]
    vis = causal.interval_visible(causal.IntervalMask(make(causal), group), Lq, Lk, qlens[0], klens[0])
    assert int((~vis.any(0))[:klens[0]].sum()) == 2 * group
    for idx in (0, 1, 2, 8):
        B, H, Lq, Lk, klens, qlens, group, make = CASES[idx]
        m = causal.IntervalMask(make(causal), group)
        assert bool(((m.q_iv[:, 3] > m.q_iv[:, 2]) & (m.q_iv[:, 2] > m.q_iv[:, 1])).any())
    # the hand-written tables: both say one matrix, no matrix builds them, and they hold what their comment promises
    B, H, Lq, Lk, klens, qlens, group, make = CASES[HAND]
    m = hand_mask(causal)
    built = causal.IntervalMask(m.vis, group)
    assert (m.q_groups, m.k_groups) == ((Lq + group - 1) // group, (Lk + group - 1) // group) == (25, 41)
    assert torch.equal(table_matrix(m.k_iv, m.q_groups), m.vis.t())
    assert not torch.equal(m.q_iv, built.q_iv) and not torch.equal(m.k_iv, built.k_iv)
    for t, other in ((m.q_iv, m.k_groups), (m.k_iv, m.q_groups)):
        assert bool(((t[:, 1] <= t[:, 0]) & (t[:, 3] > t[:, 2])).any())            # an empty first slot, a live second one
        assert bool((t < 0).any()) and bool((t > other).any())                     # bounds the kernels clamp
        assert bool((t[:, 0] <= t[:, 2]).all())                                    # rows ascend
    vis = causal.interval_visible(m, Lq, Lk)
    assert bool(vis.any(1).all())                                                  # no live row is blind
    assert bool(vis[:128, :64].any()) and not bool(vis[:128, 64:192].any()) and bool(vis[:128, 192:].any())
    assert bool(vis[:64, :128].any()) and not bool(vis[64:128, :128].any()) and bool(vis[128:, :128].any())
    assert Lq % 128 != 0 and (Lk + 63) // 64 == 6 and Lk % 64 != 0


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_interval_forward(ops, causal, attn_mod, idx):
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
    # the wrapper with the reference's signature, and a second run: the same bits
    with torch.no_grad():
        ow = attn_mod.flash_attention(q, k, v, q_lens=ql, k_lens=kl, interval_mask=mask)
    assert torch.equal(ow, o)
    assert torch.equal(ops.flash_attn(q, k, _vt(v), kl, q_lens=ql, interval_mask=mask), o)
    if idx == STAIRS:                                                        # the same mask through the staircase kernels
        oc = ops.flash_attn(q, k, _vt(v), kl, q_lens=ql, chunk_causal=(56, -1, 0))
        assert rel_rms(oc, ref["out"]) < FWD_RMS and rel_rms(o, oc) < FWD_RMS
    if idx == FULL:                                                          # vis = [[1]]: the plain kernel's bits
        set_option("OMH_ATTN_KERNEL", "base")
        assert torch.equal(o, ops.flash_attn(q, k, _vt(v), kl))


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_interval_backward(ops, causal, attn_mod, idx):
    B, H, Lq, Lk = CASES[idx][:4]
    q, k, v, do, kl, ql, mask, ref = _case(idx, causal)

    def run(through_wrapper=False, **other):
        qg, kg, vg = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        if through_wrapper:
            attn_mod.flash_attention(qg, kg, vg, q_lens=ql, k_lens=kl, interval_mask=mask).backward(do)
        elif other:
            ops.flash_attn_func(qg, kg, vg, kl, ql, **other).backward(do)
        else:
            ops.flash_attn_func(qg, kg, vg, kl, ql, interval_mask=mask).backward(do)
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
    for a, b in zip(run(through_wrapper=True), got):                         # flash_attention(interval_mask=) is differentiable
        assert torch.equal(a, b)
    if idx == STAIRS:
        for name, gt, rf in zip(("dq", "dk", "dv"), run(chunk_causal=(56, -1, 0)), ref["grads"]):
            assert rel_rms(gt, rf) < GRAD_RMS, name


@pytest.mark.parametrize("idx", [1, 4])
def test_interval_backward_modes(ops, causal, idx):
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


def test_interval_mask_refuses_other_masks(ops, causal, attn_mod):
    q = torch.randn(1, 256, 2, 128, device="cuda").bfloat16()
    blocks = torch.ones(2, 2, dtype=torch.bool)
    m = causal.IntervalMask(causal.teacher_forcing_groups(2), 64, "cuda")
    with pytest.raises(ValueError):
        attn_mod.flash_attention(q, q, q, causal=True, interval_mask=m)
    with pytest.raises(ValueError):
        attn_mod.flash_attention(q, q, q, window_size=(16, 16), interval_mask=m)
    with pytest.raises(ValueError):
        attn_mod.flash_attention(q, q, q, block_mask=blocks, interval_mask=m)
    with pytest.raises(ValueError):
        attn_mod.flash_attention(q, q, q, chunk_causal=(64, -1, 0), interval_mask=m)
    with pytest.raises(ValueError):
        ops.flash_attn_func(q, q, q, window=(16, -1), interval_mask=m)
    with pytest.raises(ValueError):
        ops.flash_attn(q, q, _vt(q), block_mask=blocks, interval_mask=m)
    with pytest.raises(ValueError):
        ops.flash_attn(q, q, _vt(q), chunk_causal=(64, -1, 0), interval_mask=m)
    with pytest.raises(ValueError):                                              # the bare matrix carries no group size
        attn_mod.flash_attention(q, q, q, interval_mask=m.vis)
    host = causal.IntervalMask(causal.teacher_forcing_groups(2), 64)             # tables on the CPU: moved beside q
    assert torch.equal(ops.flash_attn(q, q, _vt(q), interval_mask=host), ops.flash_attn(q, q, _vt(q), interval_mask=m))
    assert ops.attn_mask(interval_mask=host, H=q.shape[2], Lq=256, Lk=256, device=q.device).rule.q_iv.device == q.device
    with pytest.raises(ValueError):                                              # 4 x 4 groups of 64 do not cover 256 x 320
        ops.flash_attn(q, torch.cat([q, q[:, :64]], 1), _vt(torch.cat([q, q[:, :64]], 1)), interval_mask=m)
