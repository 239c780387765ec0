"""CPU statements for the pinned attention sink (causal.RollingKVCache(pin_sink=True)); a helper, not a test module.

``forward``: the fp32 restatement of a rollout under a pinned sink.  It is teacher_forcing_ref.forward over
[clean | noisy] under the dense ``teacher_forcing_groups(n, W, S)`` mask with ONE change: for the query rows of chunk I
(clean and noisy segment alike) whose shift Delta_I = (max(S, I - W) - S) fpc is positive, the scores against the clean
SINK columns are taken with k rotated at its frame + Delta_I.  With every Delta_I = 0 (or ``pinned=False``) the operations
are those of teacher_forcing_ref.forward, so the result is equal, not close.

``shift_exact`` / ``shift_emulated``: ops.rope_shift_frames by its rule in fp64, and by its stated arithmetic (fp64 angle
-> fp32 cos / sin -> fp32 multiply-adds -> one rounding to bf16)."""
import math

import torch

import teacher_forcing_ref as R
from oracle import wan_dit_oracle as O


def sink_deltas(n_chunks, W, S, fpc):
    """Delta_I in frames for I < n_chunks."""
    return [(max(S, I - W) - S) * fpc for I in range(n_chunks)]


def _shifted_angles(angles, head_dim, delta):
    """The rotary angle table with its frame columns moved up by ``delta`` rows."""
    cf = head_dim // 2 - 2 * (head_dim // 2 // 3)
    out = angles.clone()
    n = angles.shape[0] - delta
    out[:n, :cf] = angles[delta:, :cf]
    return out


def forward(sd, cfg, clean, noisy, t_chunks, ctx, causal, fpc, W, S, pinned=True, context_t=0.0):
    """``clean`` / ``noisy``: lists of [C, F, H, W]; ``t_chunks`` [B, F / fpc].  Returns the noisy half's outputs, a list of
    fp32 [C_out, F, H, W] — chunk I of it is what forward_chunk gives for noisy chunk I against a cache committed from the
    clean chunks before it."""
    B, F = len(clean), clean[0].shape[1]
    n = F // fpc
    tpf = (clean[0].shape[2] // cfg.patch_size[1]) * (clean[0].shape[3] // cfg.patch_size[2])
    Ct, part = fpc * tpf, F * tpf
    deltas = sink_deltas(n, W, S, fpc) if pinned else [0] * n
    vis = causal.teacher_forcing_groups(n, W, S)
    mask = vis.repeat_interleave(Ct, 0).repeat_interleave(Ct, 1)[None].expand(B, -1, -1)
    t_all = torch.cat([torch.full((B, F), float(context_t)), t_chunks.repeat_interleave(fpc, dim=1)], dim=1)

    def attention(sd_, p, cfg_, x, grids, angles, segments, m):
        Bx, Sx, _ = x.shape
        N, D = cfg_.num_heads, cfg_.dim // cfg_.num_heads
        q, k, v = O._lin(sd_, p + "q", x), O._lin(sd_, p + "k", x), O._lin(sd_, p + "v", x)
        if cfg_.qk_norm:
            q, k = O.rms_norm(q, sd_[p + "norm_q.weight"], cfg_.eps), O.rms_norm(k, sd_[p + "norm_k.weight"], cfg_.eps)
        prt = Sx // segments
        rot = lambda u, a: torch.cat([O.rope_apply(u.view(Bx, Sx, N, D)[:, i * prt:(i + 1) * prt], grids, a)
                                      for i in range(segments)], dim=1)
        k_raw = k
        q, k, v = rot(q, angles), rot(k, angles), v.view(Bx, Sx, N, D)
        s = torch.einsum("bihd,bjhd->bhij", q, k) / math.sqrt(D)
        for delta in sorted(set(d for d in deltas if d > 0)):
            # the clean sink keys as the pinned cache holds them for the chunks with this shift
            k_sink = rot(k_raw, _shifted_angles(angles, D, delta))[:, :S * Ct]
            for I in (i for i, d in enumerate(deltas) if d == delta):
                for r0 in (I * Ct, part + I * Ct):
                    s[:, :, r0:r0 + Ct, :S * Ct] = torch.einsum("bihd,bjhd->bhij", q[:, r0:r0 + Ct], k_sink) / math.sqrt(D)
        if m is not None:
            s = s.masked_fill(~m[:, None], float("-inf"))
        pr = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
        return O._lin(sd_, p + "o", torch.einsum("bhij,bjhd->bihd", pr, v).flatten(2))

    saved = R._self_attention
    R._self_attention = attention
    try:
        with torch.no_grad():
            return R.forward(sd, cfg, [torch.cat([c, x], 1) for c, x in zip(clean, noisy)], t_all, ctx, 2 * part, mask=mask,
                             segments=2, out_from=F)
    finally:
        R._self_attention = saved


def periodic_clip(F, B=2, seed=23):
    """A clip that repeats in time: the sink chunk, then identical clean frames; identical noisy frames; one t per
    sample.  (clean, noisy, t_chunks for fpc = 1) — under a pinned sink every chunk past the wrap computes the same."""
    g = torch.Generator().manual_seed(seed)
    clean, noisy = [], []
    for _ in range(B):
        sink, rest, x = (torch.randn(16, 1, 14, 16, generator=g) for _ in range(3))
        clean.append(torch.cat([sink] + [rest] * (F - 1), dim=1))
        noisy.append(x.repeat(1, F, 1, 1))
    t = torch.tensor([700., 300.])[:B, None].repeat(1, F)
    return clean, noisy, t


def periodic_restatement(causal, pinned, F=12):
    """``forward`` on the periodic clip at (fpc, W, S) = (1, 1, 1) with the tiny model of make_golden_chunk_causal."""
    import make_golden_chunk_causal as MC
    cfg, _, ctx, _, _ = MC.case()
    clean, noisy, t = periodic_clip(F)
    return forward(O.synth_state_dict(cfg, MC.TAG), cfg, clean, noisy, t, ctx, causal, 1, 1, 1, pinned=pinned)


def _frame_angles(delta, head_dim, theta):
    n = head_dim - 4 * (head_dim // 6)
    inv = 1.0 / torch.pow(torch.tensor(float(theta), dtype=torch.float64), torch.arange(0, n, 2, dtype=torch.float64) / n)
    return float(delta) * inv                                                    # fp64 [nf]


def shift_exact(src, delta, head_dim=128, theta=10000.0):
    """The rule in fp64: returns (y fp64 of src's shape — the frame pairs rotated, the other columns src's values —,
    the bool mask of the rotated elements, hypot(x0, x1) per element)."""
    B, rows, dim = src.shape
    a = _frame_angles(delta, head_dim, theta)
    nf = a.numel()
    x = src.double().view(B, rows, dim // head_dim, head_dim // 2, 2)
    y = x.clone()
    c, s = torch.cos(a), torch.sin(a)
    y[..., :nf, 0] = x[..., :nf, 0] * c - x[..., :nf, 1] * s
    y[..., :nf, 1] = x[..., :nf, 0] * s + x[..., :nf, 1] * c
    rotated = torch.zeros_like(x, dtype=torch.bool)
    rotated[..., :nf, :] = True
    hyp = torch.hypot(x[..., 0], x[..., 1]).unsqueeze(-1).expand_as(x)
    return y.reshape(B, rows, dim), rotated.reshape(B, rows, dim), hyp.reshape(B, rows, dim)


def shift_emulated(src, dst, delta, head_dim=128, theta=10000.0, fp32_angle=False):
    """ops.rope_shift_frames by its stated arithmetic, on the CPU: writes and returns ``dst`` (None: a fresh tensor).
    ``fp32_angle``: the shortcut the entry forbids (the angle as an fp32 product, fp32 cos / sin)."""
    B, rows, dim = src.shape
    if fp32_angle:
        n = head_dim - 4 * (head_dim // 6)
        inv = (1.0 / torch.pow(torch.tensor(float(theta), dtype=torch.float64),
                               torch.arange(0, n, 2, dtype=torch.float64) / n)).float()
        a = torch.tensor(float(delta), dtype=torch.float32) * inv
        c, s = torch.cos(a), torch.sin(a)
    else:
        a = _frame_angles(delta, head_dim, theta)
        c, s = torch.cos(a).float(), torch.sin(a).float()
    nf = a.numel()
    x = src.float().view(B, rows, dim // head_dim, head_dim // 2, 2)
    x0, x1 = x[..., :nf, 0], x[..., :nf, 1]
    out = src.clone().view(B, rows, dim // head_dim, head_dim // 2, 2)
    if delta != 0:
        # (fp64 holds every fp32 product exactly: one rounding of the sum to fp32, as a fused multiply-add makes it)
        out[..., :nf, 0] = (x0.double() * c.double() - (x1 * s).double()).float().to(torch.bfloat16)
        out[..., :nf, 1] = (x0.double() * s.double() + (x1 * c).double()).float().to(torch.bfloat16)
    out = out.view(B, rows, dim)
    if dst is None:
        return out
    dst.copy_(out)
    return dst
