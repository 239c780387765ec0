"""An fp32 restatement of the DiT forward with condition tokens in front of the text and a dense CROSS-attention mask,
built from oracle.wan_dit_oracle pieces on top of tests/teacher_forcing_ref.py (whose self-attention, per-frame time
embedding and head it shares): the reference of frame-aligned condition tokens in WanModel.forward,
forward_teacher_forcing and forward_chunk.  The tokens stay in the CALLER's order — the mask's columns follow them
(``causal.condition_window_visible`` keeps the order of ``token_frames``) — so the model's own re-ordering is checked too.
With every token visible it is O.dit_forward(extra_tokens=) (pinned in tests/test_interval_rect_host.py).  Autograd flows
through it (``sd`` tensors, latents, ``t_frames`` and the tokens may require grad)."""
import math

import torch
import torch.nn.functional as F

import teacher_forcing_ref as R
from oracle import wan_dit_oracle as O


def cross_attention(sd, p, cfg, x, ctx, context_lens, cross_mask):
    """x [B, S, d] on ctx [B, Lc, d]; ``cross_mask``: bool [S, Lc] or [B, S, Lc] (True: visible) or None; keys at or past
    ``context_lens[b]`` are always hidden; a row that sees nothing is zero."""
    B, S, _ = x.shape
    Lc = ctx.shape[1]
    N, D = cfg.num_heads, cfg.dim // cfg.num_heads
    q, k, v = O._lin(sd, p + "q", x), O._lin(sd, p + "k", ctx), O._lin(sd, p + "v", ctx)
    if cfg.qk_norm:
        q, k = O.rms_norm(q, sd[p + "norm_q.weight"], cfg.eps), O.rms_norm(k, sd[p + "norm_k.weight"], cfg.eps)
    q, k, v = q.view(B, S, N, D), k.view(B, Lc, N, D), v.view(B, Lc, N, D)
    live = (torch.arange(Lc)[None, None, :] < context_lens[:, None, None]).expand(B, S, Lc)
    if cross_mask is not None:
        live = live & (cross_mask if cross_mask.dim() == 3 else cross_mask[None])
    s = torch.einsum("bihd,bjhd->bhij", q, k) / math.sqrt(D)
    pr = torch.nan_to_num(torch.softmax(s.masked_fill(~live[:, None], float("-inf")), dim=-1), nan=0.0)
    return O._lin(sd, p + "o", torch.einsum("bhij,bjhd->bihd", pr, v).flatten(2))


def forward(sd, cfg, x_list, t_frames, context, seq_len, extra_tokens=None, cross_mask=None, mask=None, segments=1,
            out_from=0, frame_offset=0):
    """teacher_forcing_ref.forward with ``extra_tokens`` [B, Ne, dim] in front of the embedded text and ``cross_mask``
    (bool [seq_len, Ne + text_len]) on every cross-attention.  ``frame_offset``: the rotary frame position of the first
    frame (a chunk of a rollout restated alone)."""
    x, e, e0, ctx, context_lens, seq_lens, grids = O.embed_inputs(sd, cfg, x_list, t_frames, context, seq_len,
                                                                  extra_tokens=extra_tokens)
    B, S, d = x.shape
    G = t_frames.shape[1]
    tpf = S // G
    e_tok = e.view(B, G, d).repeat_interleave(tpf, dim=1)
    e0_tok = e0.view(B, G, 6, d).repeat_interleave(tpf, dim=1)
    seg_grids = [(g[0] // segments, g[1], g[2]) for g in grids]
    live = torch.arange(S)[None, None, :] < seq_lens[:, None, None]
    full = live.expand(B, S, S) if mask is None else (mask & live)
    angles = O.rope_table(cfg.dim // cfg.num_heads)
    if frame_offset:                                       # the frame axis of the table starts at the chunk's first frame
        angles = _shift_frames(angles, cfg.dim // cfg.num_heads, frame_offset)
    for i in range(cfg.num_layers):
        p = f"blocks.{i}."
        m = (sd[p + "modulation"].unsqueeze(0) + e0_tok).unbind(2)
        h = O.layer_norm(x, cfg.eps) * (1 + m[1]) + m[0]
        x = x + R._self_attention(sd, p + "self_attn.", cfg, h, seg_grids, angles, segments, full) * m[2]
        h = O.layer_norm(x, cfg.eps, sd[p + "norm3.weight"], sd[p + "norm3.bias"]) if cfg.cross_attn_norm else x
        x = x + cross_attention(sd, p + "cross_attn.", cfg, h, ctx, context_lens, cross_mask)
        h = O.layer_norm(x, cfg.eps) * (1 + m[4]) + m[3]
        x = x + O._lin(sd, p + "ffn.2", F.gelu(O._lin(sd, p + "ffn.0", h), approximate="tanh")) * m[5]
    x, e_tok = x[:, out_from * tpf:], e_tok[:, out_from * tpf:]
    em = (sd["head.modulation"].unsqueeze(0) + e_tok.unsqueeze(2)).unbind(2)
    h = O._lin(sd, "head.head", O.layer_norm(x, cfg.eps) * (1 + em[1]) + em[0])
    outs = []
    for u, g in zip(h, grids):
        g = (g[0] - out_from, g[1], g[2])
        u = u[:math.prod(g)].view(*g, *cfg.patch_size, cfg.out_dim)
        u = torch.einsum("fhwpqrc->cfphqwr", u)
        outs.append(u.reshape(cfg.out_dim, *[a * b for a, b in zip(g, cfg.patch_size)]).float())
    return outs


def _shift_frames(angles, head_dim, frame_offset):
    """The oracle's rotary table with its FRAME part (the first head_dim / 2 - 2 (head_dim / 6) columns, model.py:68-76)
    moved up by ``frame_offset`` rows: position f of the result is frame ``frame_offset`` + f."""
    c = head_dim // 2
    nf = c - 2 * (c // 3)
    out = angles.clone()
    out[:angles.shape[0] - frame_offset, :nf] = angles[frame_offset:, :nf]
    return out


# ---- the inputs of tests/test_gpu_condition_window_model.py (and of the CPU pin in tests/test_interval_rect_host.py) ----
FRAMES = [0, 1, 1, 2, 2, 2, 3, 3, -1, 0, 3]          # the latent frame of each condition token, deliberately unsorted
# The tokens' amplitude.  At 1 (tokens of the text embedding's own scale) the windowed and the unwindowed outputs of this
# case differ by 0.2 - 0.5 rel-RMS for the windows (0, 0), (1, 1) and (-1, 0) — far above the forward's bound of 8e-3, so
# a mask that is ignored cannot pass; tests/test_interval_rect_host.py asserts >= 5e-2 on the CPU.
TOKEN_AMPLITUDE = 1.0
F_LATENT, TOKENS_PER_FRAME = 4, 56


def case():
    """(cfg, clips, noisy clips, targets, text, per-frame t, tokens [2, 11, dim], frames): the tiny t2v model of
    tests/make_golden_chunk_causal.py, B = 2 clips of 4 latent frames, 56 tokens per frame."""
    import make_golden_chunk_causal as MC
    cfg, _, ctx, _, _ = MC.case()
    g = torch.Generator().manual_seed(11)
    clean = [torch.randn(16, F_LATENT, 14, 16, generator=g) for _ in range(2)]
    noisy = [torch.randn(16, F_LATENT, 14, 16, generator=g) for _ in range(2)]
    target = [torch.randn(16, F_LATENT, 14, 16, generator=g) for _ in range(2)]
    t_frames = torch.tensor([[900., 700., 400., 100.], [50., 250., 650., 950.]])
    tokens = TOKEN_AMPLITUDE * torch.randn(2, len(FRAMES), cfg.dim, generator=g)
    return cfg, clean, noisy, target, ctx, t_frames, tokens, torch.tensor(FRAMES)
