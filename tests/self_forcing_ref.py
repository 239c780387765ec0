"""An fp32 restatement of the gradients of ``WanModel.forward_chunk(grad=True)`` (self forcing), on top of
tests/teacher_forcing_ref.py: the teacher-forcing forward over [clean | noisy] under the dense teacher-forcing mask with
K and V of the CLEAN half detached in every self-attention.  Its noisy outputs equal teacher forcing; its gradients are
those of a rollout whose cache was committed from the clean chunks — the clean rows reach the loss through the keys and
values only (the head runs on the noisy rows), and those are constants.  ``detach=False`` is
``teacher_forcing_ref.forward`` with ``segments=2``, bit for bit (tests/test_self_forcing_host.py).

Also the inputs the self-forcing tests share: the tiny 2-layer t2v model of tests/make_golden_chunk_causal.py, B = 2
clips [16, F, 14, 16], settings (frames per chunk, left_chunks, F) = (1, -1, 6) and (2, 1, 8)."""
import math

import torch
import torch.nn.functional as Fn

import make_golden_chunk_causal as MC
from oracle import wan_dit_oracle as O

SETTINGS = ((1, -1, 6), (2, 1, 8))                  # (frames_per_chunk, left_chunks, latent frames)
TPF = MC.TOKENS_PER_FRAME
GRAD_NAMES = ("blocks.0.self_attn.q.weight", "blocks.0.self_attn.v.weight", "blocks.1.self_attn.o.weight",
              "blocks.1.modulation", "blocks.0.ffn.0.weight", "time_embedding.0.weight", "time_projection.1.bias",
              "head.head.weight", "head.modulation", "patch_embedding.weight")      # test_gpu_teacher_forcing_model.py's ten
# + block 1's key and value weights: with blocks.0.self_attn.v.weight the three that carry DIRECT clean-row terms (the
# clean rows' k and v), which is where a detached clean half differs most from an attached one
COMPARED = GRAD_NAMES + ("blocks.1.self_attn.k.weight", "blocks.1.self_attn.v.weight")
_REF = {}


def _self_attention(sd, p, cfg, x, grids, angles, mask, detach):
    """teacher_forcing_ref._self_attention with segments = 2; ``detach``: K and V of the first half are constants."""
    B, S, _ = x.shape
    N, D = cfg.num_heads, cfg.dim // cfg.num_heads
    q, k, v = O._lin(sd, p + "q", x), O._lin(sd, p + "k", x), O._lin(sd, p + "v", x)
    if cfg.qk_norm:
        q, k = O.rms_norm(q, sd[p + "norm_q.weight"], cfg.eps), O.rms_norm(k, sd[p + "norm_k.weight"], cfg.eps)
    part = S // 2
    rot = lambda u: torch.cat([O.rope_apply(u.view(B, S, N, D)[:, i * part:(i + 1) * part], grids, angles)
                               for i in range(2)], dim=1)
    q, k, v = rot(q), rot(k), v.view(B, S, N, D)
    if detach:
        k = torch.cat([k[:, :part].detach(), k[:, part:]], dim=1)
        v = torch.cat([v[:, :part].detach(), v[:, part:]], dim=1)
    s = torch.einsum("bihd,bjhd->bhij", q, k) / math.sqrt(D)
    s = s.masked_fill(~mask[:, None], float("-inf"))
    pr = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
    return O._lin(sd, p + "o", torch.einsum("bhij,bjhd->bihd", pr, v).flatten(2))


def forward(sd, cfg, x_list, t_frames, context, seq_len, mask, out_from, detach=True):
    """``teacher_forcing_ref.forward(..., segments=2)`` with the clean half's K and V detached (``detach``)."""
    x, e, e0, ctx, context_lens, seq_lens, grids = O.embed_inputs(sd, cfg, x_list, t_frames, context, seq_len)
    B, S, d = x.shape
    G = t_frames.shape[1]
    tpf = S // G
    e_tok = e.view(B, G, d).repeat_interleave(tpf, dim=1)
    e0_tok = e0.view(B, G, 6, d).repeat_interleave(tpf, dim=1)
    seg_grids = [(g[0] // 2, g[1], g[2]) for g in grids]
    live = torch.arange(S)[None, None, :] < seq_lens[:, None, None]
    full = mask & live
    angles = O.rope_table(cfg.dim // cfg.num_heads)
    for i in range(cfg.num_layers):
        p = f"blocks.{i}."
        m = (sd[p + "modulation"].unsqueeze(0) + e0_tok).unbind(2)
        h = O.layer_norm(x, cfg.eps) * (1 + m[1]) + m[0]
        x = x + _self_attention(sd, p + "self_attn.", cfg, h, seg_grids, angles, full, detach) * m[2]
        h = O.layer_norm(x, cfg.eps, sd[p + "norm3.weight"], sd[p + "norm3.bias"]) if cfg.cross_attn_norm else x
        x = x + O.cross_attention(sd, p + "cross_attn.", cfg, h, ctx, context_lens)
        h = O.layer_norm(x, cfg.eps) * (1 + m[4]) + m[3]
        x = x + O._lin(sd, p + "ffn.2", Fn.gelu(O._lin(sd, p + "ffn.0", h), approximate="tanh")) * m[5]
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


def inputs(F, fpc):
    """(cfg, clean, noisy, target, context, t [2, F / fpc]) for clips of F latent frames."""
    cfg, _, ctx, _, _ = MC.case()
    g = torch.Generator().manual_seed(11 + F)
    clean = [torch.randn(16, F, 14, 16, generator=g) for _ in range(2)]
    noisy = [torch.randn(16, F, 14, 16, generator=g) for _ in range(2)]
    target = [torch.randn(16, F, 14, 16, generator=g) for _ in range(2)]
    n = F // fpc
    t = torch.stack([torch.linspace(950., 150., n), torch.linspace(80., 880., n)])
    return cfg, clean, noisy, target, ctx, t


def tf_mask(causal, F, fpc, W):
    m = causal.IntervalMask(causal.teacher_forcing_groups(F // fpc, W), fpc * TPF)
    S = F * TPF
    return causal.interval_visible(m, 2 * S, 2 * S)[None].expand(2, -1, -1)


def reference(causal, fpc, W, F, detach=True, sd=None):
    """Loss and gradients of the restatement for a setting — computed once per (setting, detach) and left unchanged.
    loss = sum over the clips of the MSE against the target.  ``sd``: another state dict (effective LoRA weights)."""
    key = (fpc, W, F, detach)
    if sd is None and key in _REF:
        return _REF[key]
    cfg, clean, noisy, target, ctx, t = inputs(F, fpc)
    own = sd is None
    sd = O.synth_state_dict(cfg, MC.TAG) if own else {k: v.clone() for k, v in sd.items()}
    xc, xn, tc = [u.clone() for u in clean], [u.clone() for u in noisy], t.clone()
    for v in list(sd.values()) + xc + xn + [tc]:
        v.requires_grad_(True)
    t_all = torch.cat([torch.zeros(2, F), tc.repeat_interleave(fpc, dim=1)], dim=1)
    out = forward(sd, cfg, [torch.cat([c, n], 1) for c, n in zip(xc, xn)], t_all, ctx, 2 * F * TPF,
                  tf_mask(causal, F, fpc, W), F, detach=detach)
    loss = sum(Fn.mse_loss(o, v) for o, v in zip(out, target))
    loss.backward()
    res = dict(out=[o.detach() for o in out], loss=float(loss.detach()), grads={n: g.grad for n, g in sd.items()},
               d_noisy=[u.grad for u in xn], d_clean=[u.grad for u in xc], d_t=tc.grad)
    if own:
        _REF[key] = res
    return res
