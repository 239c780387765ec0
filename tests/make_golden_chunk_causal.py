"""Generates tests/golden/dit_chunk_causal_t2v_L2.npz: the REAL reference WanModel (tiny t2v, 2 layers) with its
self-attention run under the chunk-causal staircase, on two clips of different length padded to a longer ``seq_len``.
TEST INFRASTRUCTURE (not a test module; build container only, where the reference tree exists).

    python tests/make_golden_chunk_causal.py          # from the repo root

The reference's ``flash_attention`` is rebound to a masked fp32 softmax.  The reference has no such mask, so the rule
(``causal.chunk_causal_visible``: token i sees token j < k_lens[b] iff j // C <= i // C and, for left >= 0,
j // C >= i // C - left, C = frames_per_chunk x tokens per frame) is applied by the rebinding, to the self-attention
calls only: the model is built with a sentinel ``window_size`` that those calls pass on and the cross-attention calls
do not.  Stored: the forward output of both clips under two settings and, for the first, the gradients of a fixed
scalar loss under the reference's autograd.
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import detgen, make_golden, ref_import, wan_dit_oracle as O  # noqa: E402
from make_golden_window import GRAD_NAMES  # noqa: E402,F401  (matrices: their first 32 rows, as in the sibling file)

OUT = os.path.join(ROOT, "tests", "golden", "dit_chunk_causal_t2v_L2.npz")
SENTINEL = (-2, -2)                 # window_size of the reference model: marks its self-attention calls
SEQ_LEN = 320
TOKENS_PER_FRAME = 56               # (14 / 2) x (16 / 2)
SETTINGS = ((1, -1), (2, 1))        # (frames_per_chunk, left_chunks): gradients are stored for the first
TAG = "golden/chunk_causal_t2v2"
_RULE = {"chunk": None, "left": -1}


def staircase_attention(q, k, v, q_lens=None, k_lens=None, dropout_p=0., softmax_scale=None, q_scale=None, causal=False,
                        window_size=(-1, -1), deterministic=False, dtype=torch.bfloat16, version=None):
    """What flash_attn_varlen_func computes for the reference's cross-attention calls, and the same softmax under the
    staircase for its self-attention calls (those that pass the sentinel window), in fp32."""
    assert q_lens is None and q_scale is None and dropout_p == 0. and not causal
    visible = importlib.import_module("omnihuman-1-hack_amd.causal").chunk_causal_visible
    masked = tuple(window_size) == SENTINEL
    assert masked or tuple(window_size) == (-1, -1)
    B, Lq, N, D = q.shape
    Lk = k.shape[1]
    scale = D ** -0.5 if softmax_scale is None else softmax_scale
    out = torch.zeros(B, Lq, N, D, dtype=torch.float32)
    for b in range(B):
        kl = Lk if k_lens is None else int(k_lens[b])
        if masked:
            ok = visible(Lq, Lk, _RULE["chunk"], _RULE["left"], 0, None, kl)[:, :kl]
        else:
            ok = torch.ones(Lq, kl, dtype=torch.bool)
        s = torch.einsum("qhd,khd->hqk", q[b].float(), k[b, :kl].float()) * scale
        p = torch.softmax(s.masked_fill(~ok[None], float("-inf")), dim=-1)
        p = torch.nan_to_num(p, nan=0.0)                          # pad rows whose chunk starts past k_lens
        out[b] = torch.einsum("hqk,khd->qhd", p, v[b, :kl].float())
    return out.type(q.dtype)


def case():
    """Inputs shared with tests/test_gpu_chunk_causal_model.py: two clips of 5 and 3 latent frames (280 and 168 tokens, 56
    per frame), seq_len 320, text 32 / 11."""
    cfg = O.DiTConfig(model_type="t2v", in_dim=16, num_layers=2, **make_golden.TINY)
    xs = [torch.from_numpy(detgen.normalish(f"{TAG}/x0", (16, 5, 14, 16))),
          torch.from_numpy(detgen.normalish(f"{TAG}/x1", (16, 3, 14, 16)))]
    ctx = [torch.from_numpy(detgen.normalish(f"{TAG}/c0", (32, 64))),
           torch.from_numpy(detgen.normalish(f"{TAG}/c1", (11, 64)))]
    targets = [torch.from_numpy(detgen.normalish(f"{TAG}/vt{i}", tuple(u.shape))) for i, u in enumerate(xs)]
    return cfg, xs, ctx, torch.tensor([900., 300.]), targets


def main():
    model_mod, _ = ref_import.load_reference()
    saved = model_mod.flash_attention
    model_mod.flash_attention = staircase_attention
    try:
        cfg, xs, ctx, t, targets = case()
        sd = O.synth_state_dict(cfg, TAG)
        m = model_mod.WanModel(model_type="t2v", patch_size=cfg.patch_size, text_len=cfg.text_len, in_dim=cfg.in_dim,
                               dim=cfg.dim, ffn_dim=cfg.ffn_dim, freq_dim=cfg.freq_dim, text_dim=cfg.text_dim,
                               out_dim=cfg.out_dim, num_heads=cfg.num_heads, num_layers=cfg.num_layers,
                               window_size=SENTINEL, qk_norm=cfg.qk_norm, cross_attn_norm=cfg.cross_attn_norm, eps=cfg.eps,
                               use_checkpoint=False)
        m.load_state_dict(sd, strict=True)
        torch.cuda.empty_cache = lambda: None  # the reference calls it on every forward
        m.eval()
        res = {"seq_len": np.int32(SEQ_LEN), "settings": np.array(SETTINGS, dtype=np.int32)}
        for n, (fpc, left) in enumerate(SETTINGS):
            _RULE["chunk"], _RULE["left"] = fpc * TOKENS_PER_FRAME, left
            with torch.enable_grad():
                out = m(xs, t, ctx, SEQ_LEN)
                if n == 0:
                    loss = sum(torch.nn.functional.mse_loss(o, v) for o, v in zip(out, targets))
                    loss.backward()
            res[f"s{n}_out0"], res[f"s{n}_out1"] = out[0].detach().numpy(), out[1].detach().numpy()
            if n == 0:
                res["loss"] = np.float32(loss.item())
                params = dict(m.named_parameters())
                for name in GRAD_NAMES:
                    g = params[name].grad.numpy()
                    res[name] = g if g.ndim == 1 else g[:32]
        np.savez_compressed(OUT, **res)
        print("chunk-causal golden: loss", float(res["loss"]), "bytes", os.path.getsize(OUT))
    finally:
        model_mod.flash_attention = saved


if __name__ == "__main__":
    main()
