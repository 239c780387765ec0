"""The long-sequence attention stream without a running max (csrc/gen_attn_w64.py V4, attention_w64.hip): the norm kernel
emits max |q|^2 and max |k|^2 per (sample, head), the attention kernel turns them into a bound m on that pair's scores
(Cauchy-Schwarz) and, where m <= 48 log2 units, computes p = 2^(s - m) against the fixed m.  Above the limit, with a
NaN / infinity in the buffer, or with option ATTN_BOUNDED = "0", the call is the plain one bit for bit."""
import importlib
import math

import pytest
import torch

from conftest import rel_rms, set_option

pytestmark = pytest.mark.gpu

D, LOG2E = 128, 1.4426950408889634
QS = D ** -0.5 * LOG2E                    # what the norm kernel folds into q (omh_attn_args.q_prescaled)
LIMIT = 48.0                              # attention_w64.hip: W64_BOUND_LIMIT
TOL_TINY = 8.0e-3                         # tests/test_gpu_dit.py: the miniature models against the oracle


def _bf(x):
    return x.to(torch.bfloat16)


def _vt(v):
    B, Lk, H, _ = v.shape
    Lp = (Lk + 63) // 64 * 64
    vt = torch.zeros(B, H * D, Lp, dtype=torch.bfloat16, device=v.device)
    vt[:, :, :Lk] = v.reshape(B, Lk, H * D).transpose(1, 2)
    return vt


def _norm2_max(q, k):
    """float [B, H, 2]: max over rows of |q row|^2 and |k row|^2 per (sample, head), from the bf16 operands."""
    return torch.stack([q.float().pow(2).sum(-1).amax(1), k.float().pow(2).sum(-1).amax(1)], -1).contiguous()


def _m_of(nm):
    """The kernel's bound: ceil(|q|max |k|max (1 + 2^-6))."""
    return torch.ceil(torch.sqrt(nm[..., 0] * nm[..., 1]) * (1.0 + 2.0 ** -6))


PAD = 8                                   # rows behind Lq in the output buffer: the kernel must leave them alone


def _run(ops, q, k, vt, klens, nm=None):
    """One launch on a NaN-filled output that is PAD rows longer than Lq; returns (out [B,Lq,H,D], lse, pad rows)."""
    B, Lq, H, _ = q.shape
    Lk = k.shape[1]
    kl = None if klens is None else torch.tensor(klens, dtype=torch.int32, device="cuda")
    buf = torch.full((B, Lq + PAD, H, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    lse = torch.full((B, H, Lq), float("nan"), dtype=torch.float32, device="cuda")
    ops.flash_attn_raw(ops.ptr(q), ops.ptr(k), ops.ptr(vt), ops.ptr(buf), ops.ptr(kl) if kl is not None else None,
                       B, H, Lq, Lk, q.stride(0), q.stride(1), k.stride(0), k.stride(1), vt.stride(0),
                       buf.stride(0), buf.stride(1), vt.stride(1), D ** -0.5, lse=ops.ptr(lse), q_prescaled=1,
                       qk_norm2_max=ops.ptr(nm) if nm is not None else None)
    return buf[:, :Lq], lse, buf[:, Lq:]


def _scores(q, k, klens):
    """log2-unit scores of the pre-scaled q, masked keys at -inf: [B, H, Lq, Lk] fp32."""
    s = torch.einsum("bqhd,bkhd->bhqk", q.float(), k.float())
    if klens is not None:
        for b, n in enumerate(klens):
            s[b, :, :, n:] = float("-inf")
    return s


def _ref(q, k, v, klens):
    s = _scores(q, k, klens) / LOG2E                                       # natural-log scores
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v.float()), torch.logsumexp(s, -1)


def _check(out, lse, ref, ref_lse):
    """The tolerances of test_flash_attention_w64_prescaled_q_lse_and_late_rescale."""
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    err, mx, el = rel_rms(out.float(), ref), float((out.float() - ref).abs().max()), float((lse - ref_lse).abs().max())
    print(f"rel-RMS {err:.3e}  max abs {mx:.3e}  lse {el:.3e}")
    assert err < 8e-3 and mx < 3e-2
    assert el < 5e-3


def _case(g, B, H, Lq, Lk, amp=1.0):
    q = _bf(torch.randn(B, Lq, H, D, device="cuda", generator=g) * amp * QS)
    k = _bf(torch.randn(B, Lk, H, D, device="cuda", generator=g) * amp)
    v = _bf(torch.randn(B, Lk, H, D, device="cuda", generator=g))
    return q, k, v


# ------------------------------------------------------------------ 1. the norm kernel's maxima
@pytest.mark.parametrize("B,S,grids", [(1, 130, [(2, 5, 13)]), (2, 70, [(1, 5, 13), (1, 7, 10)])])
def test_norm_maxima(ops, B, S, grids):
    """omh_rmsnorm_rope_bf16_pair_bound: q and k bit-equal to omh_rmsnorm_rope_bf16_pair (as it dispatches by itself, and in
    its one-wave-per-row form, which is the form the bounded entry copies); every emitted max |.|^2 within (1 +- 2^-7) of the
    maximum recomputed from the STORED bf16 rows of that (sample, head) (twice the 2^-8 envelope of squaring a 2^-9
    rounding).  Pad rows (sample 0 of the second shape has 65 tokens in 70 rows) and two samples."""
    from oracle import wan_dit_oracle as O
    torch.manual_seed(S)
    d, rows = 1536, B * S
    N = d // D
    qk = (torch.randn(rows, 2 * d, device="cuda") * 1.3).bfloat16()
    wq, wk = torch.rand(d, device="cuda") + 0.5, torch.rand(d, device="cuda") + 0.5
    ang = O.rope_table(D)
    cos, sin = torch.cos(ang).float().cuda(), torch.sin(ang).float().cuda()
    grid = torch.tensor(grids, dtype=torch.int32, device="cuda")
    args = (ops.ptr(qk), 2 * d, d)
    tail = (rows, d, ops.ptr(wq), ops.ptr(wk), 1e-6, 1, ops.ptr(cos), ops.ptr(sin), 1024, D, ops.ptr(grid), S)
    q0, k0 = torch.empty(rows, d, dtype=torch.bfloat16, device="cuda"), torch.empty(rows, d, dtype=torch.bfloat16, device="cuda")
    ops.rmsnorm_rope_bf16_pair_raw(*args, ops.ptr(q0), ops.ptr(k0), *tail, out_scale0=QS, out_scale1=1.0)
    set_option("RMS_PAIR_ROW", "1")
    qr, kr = torch.empty_like(q0), torch.empty_like(k0)
    ops.rmsnorm_rope_bf16_pair_raw(*args, ops.ptr(qr), ops.ptr(kr), *tail, out_scale0=QS, out_scale1=1.0)
    set_option("RMS_PAIR_ROW", None)
    assert torch.equal(qr, q0) and torch.equal(kr, k0)
    bufs = []
    for _ in range(2):
        q1, k1 = torch.full_like(q0, 3.0), torch.full_like(k0, 3.0)
        nm = torch.zeros(B, N, 2, dtype=torch.float32, device="cuda")
        ops.rmsnorm_rope_bf16_pair_bound_raw(*args, ops.ptr(q1), ops.ptr(k1), *tail, ops.ptr(nm), out_scale0=QS, out_scale1=1.0)
        assert torch.equal(q1, q0) and torch.equal(k1, k0)
        bufs.append(nm)
    assert torch.equal(bufs[0], bufs[1])                                  # an order-independent maximum: repeatable bits
    want = _norm2_max(q0.view(B, S, N, D), k0.view(B, S, N, D))
    ratio = bufs[0] / want
    print("emitted / recomputed:", float(ratio.min()), float(ratio.max()))
    assert float(want.min()) > 0
    assert float(ratio.min()) >= 1 - 2.0 ** -7 and float(ratio.max()) <= 1 + 2.0 ** -7


# ------------------------------------------------------------------ 2. bounded attention against fp32 softmax
@pytest.mark.parametrize("B,H,Lq,Lk,klens", [(1, 2, 300, 200, None), (2, 2, 777, 1000, [1000, 333]), (1, 1, 64, 100, [37]),
                                             (1, 2, 130, 320, [257])])
def test_bounded_attention_matches_fp32_softmax(ops, B, H, Lq, Lk, klens):
    set_option("OMH_ATTN_KERNEL", "w64")
    g = torch.Generator(device="cuda").manual_seed(11)
    q, k, v = _case(g, B, H, Lq, Lk)
    vt, nm = _vt(v), _norm2_max(q, k)
    assert float(_m_of(nm).max()) <= LIMIT                                 # every workgroup takes the bounded stream
    out, lse, pad = _run(ops, q, k, vt, klens, nm)
    ref, ref_lse = _ref(q, k, v, klens)
    _check(out, lse, ref, ref_lse)
    assert torch.isnan(pad.float()).all()                                  # rows past Lq: untouched
    out2, lse2, _ = _run(ops, q, k, vt, klens, nm)
    assert torch.equal(out, out2) and torch.equal(lse, lse2)
    plain, _, _ = _run(ops, q, k, vt, klens)
    assert not torch.equal(out, plain)                                     # another stream ran: P carries another factor per row


# ------------------------------------------------------------------ 3. slack
def _emulate_bounded(q, k, v, klens, m):
    """The bounded stream's arithmetic in fp32 on the CPU: P = 2^(S - m) rounded to bf16 for the P V product, the row sums
    taken on the unrounded fp32 P; m [B, H]."""
    s = _scores(q.cpu(), k.cpu(), klens)
    p = torch.exp2(s - m.cpu()[:, :, None, None])
    l = p.sum(-1)
    o = torch.einsum("bhqk,bkhd->bqhd", p.bfloat16().float(), v.cpu().float()) / l.permute(0, 2, 1)[..., None]
    return o, (m.cpu()[:, :, None] + torch.log2(l)) * math.log(2.0)


def test_bounded_attention_with_slack(ops):
    """One q row per head 30 x larger than the rest sets |q|max alone: every other row runs with slack ~ m between its own
    largest score and the fixed m, and the scale puts m at the limit (47.5 before the ceil: m = 48, p down to 2^-96)."""
    set_option("OMH_ATTN_KERNEL", "w64")
    g = torch.Generator(device="cuda").manual_seed(23)
    B, H, Lq, Lk, klens = 2, 2, 300, 400, [400, 171]
    q, k, v = _case(g, B, H, Lq, Lk)
    q[:, 17] = _bf(q[:, 17].float() * 30.0)
    for _ in range(2):                                                     # (the rounding to bf16 moves the norm by < 2^-9)
        f = 47.5 / (torch.sqrt(_norm2_max(q, k).prod(-1)) * (1.0 + 2.0 ** -6))           # [B, H]
        q = _bf(q.float() * f[:, None, :, None])
    nm = _norm2_max(q, k)
    m = _m_of(nm)
    print("m per (sample, head):", m.flatten().tolist())
    assert float(m.min()) >= 47.0 and float(m.max()) <= LIMIT
    smax = _scores(q, k, klens).amax(-1)                                   # [B, H, Lq]
    others = torch.ones(Lq, dtype=torch.bool, device="cuda")
    others[17] = False
    assert float((m[:, :, None] - smax)[:, :, others].min()) > 0.8 * LIMIT          # the slack the other rows run with
    ref, ref_lse = _ref(q, k, v, klens)
    emu, emu_lse = _emulate_bounded(q, k, v, klens, m)                     # the construction itself holds the tolerances
    _check(emu.bfloat16().cuda(), emu_lse.cuda(), ref, ref_lse)
    out, lse, _ = _run(ops, q, k, _vt(v), klens, nm)
    _check(out, lse, ref, ref_lse)
    assert float(out.float().abs().amax(-1).min()) > 0                     # no all-zero output row


# ------------------------------------------------------------------ 4. fallback
def test_fallback_is_the_plain_call(ops):
    """Scores about 180 (the amp = 4 spike case of the plain stream's test): the bound is far over the limit, the bounded
    entry's output and lse are the plain entry's bits; so with NaN or infinity in the buffer, and with ATTN_BOUNDED = 0
    whatever the buffer says."""
    set_option("OMH_ATTN_KERNEL", "w64")
    g = torch.Generator(device="cuda").manual_seed(11)
    B, H, Lq, Lk = 1, 2, 512, 4096
    q, k, v = _case(g, B, H, Lq, Lk, amp=4.0)
    k[:, Lk - 70] = _bf(q[:, 5].float() / QS)
    vt, nm = _vt(v), _norm2_max(q, k)
    assert float(_m_of(nm).min()) > LIMIT
    plain, plain_lse, _ = _run(ops, q, k, vt, None)
    ref, ref_lse = _ref(q, k, v, None)
    _check(plain, plain_lse, ref, ref_lse)

    def same(buf):
        out, lse, _ = _run(ops, q, k, vt, None, buf)
        return torch.equal(out, plain) and torch.equal(lse, plain_lse)
    assert same(nm)
    assert same(torch.full_like(nm, float("nan")))
    assert same(torch.full_like(nm, float("inf")))
    set_option("ATTN_BOUNDED", "0")
    assert same(nm) and same(torch.ones_like(nm))                          # a buffer that would select the bounded stream
    # ... and on a launch whose bound is under the limit
    q, k, v = _case(g, 1, 2, 300, 200)
    vt, nm = _vt(v), _norm2_max(q, k)
    assert float(_m_of(nm).max()) <= LIMIT
    plain, plain_lse, _ = _run(ops, q, k, vt, None)
    out, lse, _ = _run(ops, q, k, vt, None, nm)
    assert torch.equal(out, plain) and torch.equal(lse, plain_lse)


# ------------------------------------------------------------------ 5. the choice is per (sample, head)
def test_choice_is_per_sample_and_head(ops):
    set_option("OMH_ATTN_KERNEL", "w64")
    g = torch.Generator(device="cuda").manual_seed(31)
    B, H, Lq, Lk, klens = 2, 2, 300, 330, [330, 200]
    q, k, v = _case(g, B, H, Lq, Lk)
    k[1, :, 0] = _bf(k[1, :, 0].float() * 4.0)                             # (sample 1, head 0): over the limit
    vt, nm = _vt(v), _norm2_max(q, k)
    over = _m_of(nm) > LIMIT
    assert over.tolist() == [[False, False], [True, False]]
    out, lse, _ = _run(ops, q, k, vt, klens, nm)
    plain, plain_lse, _ = _run(ops, q, k, vt, klens)
    assert torch.equal(out[1, :, 0], plain[1, :, 0]) and torch.equal(lse[1, 0], plain_lse[1, 0])
    ref, ref_lse = _ref(q, k, v, klens)
    for b, h in ((0, 0), (0, 1), (1, 1)):
        assert not torch.equal(out[b, :, h], plain[b, :, h])
        _check(out[b:b + 1, :, h:h + 1], lse[b:b + 1, h:h + 1], ref[b:b + 1, :, h:h + 1], ref_lse[b:b + 1, h:h + 1])


# ------------------------------------------------------------------ 6. model level
def test_model_with_and_without_the_bounded_stream(ops, wan_model_mod):
    """The miniature WanModel of the DiT tests with the long-sequence kernel forced: ATTN_BOUNDED unset and "0" both hold
    those tests' tolerance against the oracle, the self-attention calls carry the norm buffer only when the option allows,
    and forward_cfg_pair equals two forward() calls bit for bit with the option unset."""
    from oracle import wan_dit_oracle as O, detgen
    kw = dict(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64, text_len=32, freq_dim=64)
    cfg = O.DiTConfig(**kw)
    sd = O.synth_state_dict(cfg, "tiny2")
    grids, seq_len = [(2, 3, 4), (1, 2, 3)], 30
    xs = [torch.from_numpy(detgen.normalish(f"tiny2/x{i}", (cfg.in_dim, g[0], g[1] * 2, g[2] * 2))) for i, g in enumerate(grids)]
    ctx = [torch.from_numpy(detgen.normalish(f"tiny2/c{i}", (n, cfg.text_dim))) for i, n in enumerate([32, 11])]
    t = torch.tensor([999., 500.])
    ref = O.dit_forward(sd, cfg, xs, t, ctx, seq_len)
    m = wan_model_mod.WanModel(**kw)
    m.load_state_dict(sd)
    m = m.cuda().eval().requires_grad_(False)
    xs, ctx, t = [u.cuda() for u in xs], [c.cuda() for c in ctx], t.cuda()
    set_option("OMH_ATTN_KERNEL", "w64")
    raw, seen = ops.flash_attn_raw, []

    def spy(*a, **kv):
        if a[7] == a[8] == seq_len:                                        # Lq == Lk == seq_len: a self-attention launch
            seen.append(kv.get("qk_norm2_max") is not None)
        return raw(*a, **kv)
    outs = {}
    try:
        ops.flash_attn_raw = spy
        for opt in (None, "0"):
            set_option("ATTN_BOUNDED", opt)
            del seen[:]
            outs[opt] = m(xs, t, ctx, seq_len)
            assert seen == [opt is None] * 2, (opt, seen)
            for o, r in zip(outs[opt], ref):
                print("ATTN_BOUNDED", opt, rel_rms(o, r))
                assert rel_rms(o, r) < TOL_TINY
    finally:
        ops.flash_attn_raw = raw
    set_option("ATTN_BOUNDED", None)
    null = [c[:5].clone() * 0.5 for c in ctx]
    want_c, want_u = m(xs, t, ctx, seq_len), m(xs, t, null, seq_len)
    got_c, got_u = m.forward_cfg_pair(xs, t, ctx, null, seq_len)
    for a, b in zip(got_c + got_u, want_c + want_u):
        assert torch.equal(a, b)
    assert all(torch.equal(a, b) for a, b in zip(want_c, outs[None]))
