"""An fp32 restatement of the DiT forward with a per-token time embedding and a dense self-attention mask, built from
oracle.wan_dit_oracle pieces: the reference of the per-frame-timestep forward and of WanModel.forward_teacher_forcing.
With a uniform t, one segment and no mask it is O.dit_forward (pinned in tests/test_interval_mask_host.py).  Autograd
flows through it (``sd`` tensors, latents and ``t_frames`` may require grad)."""
import math

import torch
import torch.nn.functional as F

from oracle import wan_dit_oracle as O


def _self_attention(sd, p, cfg, x, grids, angles, segments, mask):
    """x [B, S, d].  ``segments``: the sequence is that many equal parts, each rotated with the frame positions of a
    clip of grid ``grids[b]`` (teacher forcing: 2); ``mask``: bool [B, S, S] (True: visible) or None."""
    B, S, _ = x.shape
    N, D = cfg.num_heads, cfg.dim // cfg.num_heads
    q, k, v = O._lin(sd, p + "q", x), O._lin(sd, p + "k", x), O._lin(sd, p + "v", x)
    if cfg.qk_norm:
        q, k = O.rms_norm(q, sd[p + "norm_q.weight"], cfg.eps), O.rms_norm(k, sd[p + "norm_k.weight"], cfg.eps)
    part = S // segments
    rot = lambda u: torch.cat([O.rope_apply(u.view(B, S, N, D)[:, i * part:(i + 1) * part], grids, angles)
                               for i in range(segments)], dim=1)
    q, k, v = rot(q), rot(k), v.view(B, S, N, D)
    s = torch.einsum("bihd,bjhd->bhij", q, k) / math.sqrt(D)
    if mask is not None:
        s = s.masked_fill(~mask[:, None], float("-inf"))
    pr = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
    return O._lin(sd, p + "o", torch.einsum("bhij,bjhd->bihd", pr, v).flatten(2))


def forward(sd, cfg, x_list, t_frames, context, seq_len, mask=None, segments=1, out_from=0):
    """``x_list``: latents [C, G, H, W] (for teacher forcing the clean and noisy frames concatenated along the frame
    axis, G = 2 F); ``t_frames`` [B, seq_len / (h w)]: one timestep per frame of the padded sequence; ``mask``: bool
    [B, seq_len, seq_len] or None (keys past a clip's tokens are always hidden); ``segments``: see _self_attention;
    ``out_from``: the first FRAME the head runs on.  Returns the list of fp32 [C_out, frames, H, W]."""
    x, e, e0, ctx, context_lens, seq_lens, grids = O.embed_inputs(sd, cfg, x_list, t_frames, context, seq_len)
    B, S, d = x.shape
    G = t_frames.shape[1]
    tpf = S // G
    e_tok = e.view(B, G, d).repeat_interleave(tpf, dim=1)                       # [B, S, d]
    e0_tok = e0.view(B, G, 6, d).repeat_interleave(tpf, dim=1)                  # [B, S, 6, d]
    seg_grids = [(g[0] // segments, g[1], g[2]) for g in grids]
    live = torch.arange(S)[None, None, :] < seq_lens[:, None, None]              # [B, 1, S]
    full = live.expand(B, S, S) if mask is None else (mask & live)
    angles = O.rope_table(cfg.dim // cfg.num_heads)
    for i in range(cfg.num_layers):
        p = f"blocks.{i}."
        m = (sd[p + "modulation"].unsqueeze(0) + e0_tok).unbind(2)              # 6 x [B, S, d]
        h = O.layer_norm(x, cfg.eps) * (1 + m[1]) + m[0]
        x = x + _self_attention(sd, p + "self_attn.", cfg, h, seg_grids, angles, segments, full) * m[2]
        h = O.layer_norm(x, cfg.eps, sd[p + "norm3.weight"], sd[p + "norm3.bias"]) if cfg.cross_attn_norm else x
        x = x + O.cross_attention(sd, p + "cross_attn.", cfg, h, ctx, context_lens)
        h = O.layer_norm(x, cfg.eps) * (1 + m[4]) + m[3]
        x = x + O._lin(sd, p + "ffn.2", F.gelu(O._lin(sd, p + "ffn.0", h), approximate="tanh")) * m[5]
    x, e_tok = x[:, out_from * tpf:], e_tok[:, out_from * tpf:]
    em = (sd["head.modulation"].unsqueeze(0) + e_tok.unsqueeze(2)).unbind(2)    # 2 x [B, S', d]
    h = O._lin(sd, "head.head", O.layer_norm(x, cfg.eps) * (1 + em[1]) + em[0])
    outs = []
    for u, g in zip(h, grids):
        g = (g[0] - out_from, g[1], g[2])
        u = u[:math.prod(g)].view(*g, *cfg.patch_size, cfg.out_dim)
        u = torch.einsum("fhwpqrc->cfphqwr", u)
        outs.append(u.reshape(cfg.out_dim, *[a * b for a, b in zip(g, cfg.patch_size)]).float())
    return outs
