"""The CPU statement of teacher forcing under a pinned sink as WanModel.forward_teacher_forcing(pin_sink=True) builds it: an
EXTENDED KEY AXIS; a helper, not a test module.

``forward`` is teacher_forcing_ref.forward over [clean | noisy] with the keys of every self-attention extended by one
rotated image of the S clean sink chunks per chunk I whose shift Delta_I is positive (causal.sink_copy_deltas):

    keys of a sample:  [ clean 0..n-1 | noisy 0..n-1 | sink @ Delta_{S+W+1} | sink @ Delta_{S+W+2} | ... ]

under the dense ``causal.teacher_forcing_groups(n, W, S, pin_sink=True)`` mask; V of an image is the sink's V.  It computes
what pinned_sink_ref.forward(pinned=True) computes by overwriting scores (pinned to it in tests/test_pinned_tf_host.py), and
autograd flows through it: the images are functions of the sink keys, so their gradients fold back into the sink rows by
the chain rule — the reference of the model's fold.  Without an image (the clip does not outlast the ring) the operations are
those of teacher_forcing_ref.forward under the square mask, so the result is equal, not close."""
import math

import torch

import teacher_forcing_ref as R
from oracle import wan_dit_oracle as O
from pinned_sink_ref import _shifted_angles


def forward(sd, cfg, clean, noisy, t_chunks, ctx, causal, fpc, W, S, context_t=0.0):
    """``clean`` / ``noisy``: lists of [C, F, H, W]; ``t_chunks`` [B, F / fpc].  Returns the noisy half's outputs, a list of
    fp32 [C_out, F, H, W].  Gradients reach ``sd``, the latents and ``t_chunks`` when they require them."""
    B, F = len(clean), clean[0].shape[1]
    n = F // fpc
    tpf = (clean[0].shape[2] // cfg.patch_size[1]) * (clean[0].shape[3] // cfg.patch_size[2])
    Ct, part = fpc * tpf, F * tpf
    copies = causal.sink_copy_deltas(n, W, S, fpc)
    vis = causal.teacher_forcing_groups(n, W, S, pin_sink=True) if copies else causal.teacher_forcing_groups(n, W, S)
    mask = vis.repeat_interleave(Ct, 0).repeat_interleave(Ct, 1)[None].expand(B, -1, -1)      # [B, 2 part, 2 part + C S Ct]
    t_all = torch.cat([torch.full((B, F), float(context_t)), t_chunks.repeat_interleave(fpc, dim=1)], dim=1)

    def attention(sd_, p, cfg_, x, grids, angles, segments, _square):
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
        if copies:
            # one image of the clean sink keys per shifted chunk, as the pinned cache holds them when that chunk runs
            k = torch.cat([k] + [rot(k_raw, _shifted_angles(angles, D, delta))[:, :S * Ct] for _, delta in copies], dim=1)
            v = torch.cat([v] + [v[:, :S * Ct]] * len(copies), dim=1)
        s = torch.einsum("bihd,bjhd->bhij", q, k) / math.sqrt(D)
        s = s.masked_fill(~mask[:, None], float("-inf"))
        pr = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
        return O._lin(sd_, p + "o", torch.einsum("bhij,bjhd->bihd", pr, v).flatten(2))

    saved = R._self_attention
    R._self_attention = attention
    try:
        return R.forward(sd, cfg, [torch.cat([c, x], 1) for c, x in zip(clean, noisy)], t_all, ctx, 2 * part, mask=None,
                         segments=2, out_from=F)
    finally:
        R._self_attention = saved
