"""Generates tests/golden/dit_window_t2v_L2.npz: the REAL reference WanModel (tiny t2v, 2 layers) built with a
sliding-window self-attention, run on two clips of different length padded to a longer ``seq_len``.  TEST
INFRASTRUCTURE (not a test module; build container only, where the reference tree exists).

    python tests/make_golden_window.py          # from the repo root

The reference's ``flash_attention`` is rebound to a masked fp32 softmax that applies flash-attn's bottom-right aligned
band (``window_size=(left, right)``: query i of a sample with Lq queries and k_lens[b] keys sees key j iff
i + k_lens[b] - Lq - left <= j <= i + k_lens[b] - Lq + right, a side < 0 unbounded; a row whose band is empty is zero).
The shim of oracle/ref_import.py ignores the window, so it is not used here.  Stored: the forward output of both clips
and the gradients of a fixed scalar loss under the reference's autograd.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import detgen, make_golden, ref_import, wan_dit_oracle as O  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "dit_window_t2v_L2.npz")
WINDOW = (70, 30)
SEQ_LEN = 320
TAG = "golden/window_t2v2"
# the gradients stored (matrices: their first 32 rows, which keeps the file small)
GRAD_NAMES = ("blocks.0.self_attn.q.weight", "blocks.0.self_attn.k.weight", "blocks.1.self_attn.v.weight",
              "blocks.1.self_attn.o.weight", "blocks.0.self_attn.norm_q.weight", "blocks.1.ffn.0.weight",
              "patch_embedding.weight", "head.head.weight")


def band_attention(q, k, v, q_lens=None, k_lens=None, dropout_p=0., softmax_scale=None, q_scale=None, causal=False,
                   window_size=(-1, -1), deterministic=False, dtype=torch.bfloat16, version=None):
    """What flash_attn_varlen_func computes for the reference's self- and cross-attention calls, in fp32."""
    assert q_lens is None and q_scale is None and dropout_p == 0.
    left, right = window_size
    if causal:
        right = 0
    B, Lq, N, D = q.shape
    Lk = k.shape[1]
    scale = D ** -0.5 if softmax_scale is None else softmax_scale
    out = torch.zeros(B, Lq, N, D, dtype=torch.float32)
    for b in range(B):
        kl = Lk if k_lens is None else int(k_lens[b])
        i = torch.arange(Lq)[:, None] + (kl - Lq)
        j = torch.arange(kl)[None, :]
        ok = torch.ones(Lq, kl, dtype=torch.bool)
        if left >= 0:
            ok &= j >= i - left
        if right >= 0:
            ok &= j <= i + right
        s = torch.einsum("qhd,khd->hqk", q[b].float(), k[b, :kl].float()) * scale
        p = torch.softmax(s.masked_fill(~ok[None], float("-inf")), dim=-1)
        p = torch.nan_to_num(p, nan=0.0)                          # rows with an empty band
        out[b] = torch.einsum("hqk,khd->qhd", p, v[b, :kl].float())
    return out.type(q.dtype)


def case():
    """Inputs shared with tests/test_gpu_attn_window_model.py: two clips (288 and 120 tokens), seq_len 320, text 32 / 11."""
    cfg = O.DiTConfig(model_type="t2v", in_dim=16, num_layers=2, **make_golden.TINY)
    xs = [torch.from_numpy(detgen.normalish(f"{TAG}/x0", (16, 6, 12, 16))),
          torch.from_numpy(detgen.normalish(f"{TAG}/x1", (16, 4, 10, 12)))]
    ctx = [torch.from_numpy(detgen.normalish(f"{TAG}/c0", (32, 64))),
           torch.from_numpy(detgen.normalish(f"{TAG}/c1", (11, 64)))]
    targets = [torch.from_numpy(detgen.normalish(f"{TAG}/vt{i}", tuple(u.shape))) for i, u in enumerate(xs)]
    return cfg, xs, ctx, torch.tensor([900., 300.]), targets


def main():
    model_mod, _ = ref_import.load_reference()
    saved = model_mod.flash_attention
    model_mod.flash_attention = band_attention
    try:
        cfg, xs, ctx, t, targets = case()
        sd = O.synth_state_dict(cfg, TAG)
        m = model_mod.WanModel(model_type="t2v", patch_size=cfg.patch_size, text_len=cfg.text_len, in_dim=cfg.in_dim,
                               dim=cfg.dim, ffn_dim=cfg.ffn_dim, freq_dim=cfg.freq_dim, text_dim=cfg.text_dim,
                               out_dim=cfg.out_dim, num_heads=cfg.num_heads, num_layers=cfg.num_layers,
                               window_size=WINDOW, qk_norm=cfg.qk_norm, cross_attn_norm=cfg.cross_attn_norm, eps=cfg.eps,
                               use_checkpoint=False)
        m.load_state_dict(sd, strict=True)
        torch.cuda.empty_cache = lambda: None  # the reference calls it on every forward
        m.eval()
        with torch.enable_grad():
            out = m(xs, t, ctx, SEQ_LEN)
            loss = sum(torch.nn.functional.mse_loss(o, v) for o, v in zip(out, targets))
            loss.backward()
        res = {"out0": out[0].detach().numpy(), "out1": out[1].detach().numpy(), "loss": np.float32(loss.item()),
               "window": np.array(WINDOW, dtype=np.int32), "seq_len": np.int32(SEQ_LEN)}
        params = dict(m.named_parameters())
        for name in GRAD_NAMES:
            g = params[name].grad.numpy()
            res[name] = g if g.ndim == 1 else g[:32]
        np.savez_compressed(OUT, **res)
        print("window golden: loss", loss.item(), "bytes", os.path.getsize(OUT))
    finally:
        model_mod.flash_attention = saved


if __name__ == "__main__":
    main()
