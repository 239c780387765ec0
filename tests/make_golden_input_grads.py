"""Generates tests/golden/dit_input_grads.npz: gradients of the REAL reference WanModel w.r.t. its INPUTS — the
latents x, the conditioning channels y, the text context, the CLIP tokens and the timestep t — on the tiny cases of
oracle/make_golden.tiny_case.  TEST INFRASTRUCTURE (not a test module; build container only, where the reference tree
exists).

    python tests/make_golden_input_grads.py          # from the repo root

Cases (``compute(forward)`` runs them on any forward with the reference's call signature, so tests can run the same
graphs on the CPU oracle):
  a  tiny t2v L2, two clips of different size padded to seq_len: gradients of sum_i mse(out_i, target_i) w.r.t.
     every x_i, context_i and t;
  b  tiny i2v L2: the same plus y_i and clip_fea (stored: its first 8 token rows per sample + its Frobenius norm);
  c  chain G -> D: a trainable tiny t2v G and a frozen tiny t2v D with other weights, x_hat = z - G(z, t, c),
     loss = sum_i mean(D(x_hat, t', c)_i ^ 2): six parameter gradients of G and dz;
  d  two-step rollout of one model: x1 = x0 - 0.5 m(x0), loss = sum_i mean(m(x1)_i ^ 2): the same six and dx0.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import detgen, make_golden, ref_import, wan_dit_oracle as O  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "dit_input_grads.npz")
TAG = "golden/input_grads"
TAG_G, TAG_D = TAG + "/G", TAG + "/D"
T_D = (250., 750.)                     # the timesteps D is evaluated at in case c
CLIP_ROWS = 8
# parameter gradients stored for cases c and d (matrices: their first 32 rows)
GRAD_NAMES = ("blocks.0.self_attn.q.weight", "patch_embedding.weight", "head.head.weight", "text_embedding.0.weight",
              "time_embedding.0.weight", "blocks.0.self_attn.norm_q.weight")


def case(model_type):
    """(cfg, tag, xs, ctx, t, seq_len, ys, clip, targets) of cases a (t2v) and b (i2v): make_golden.tiny_case plus the
    regression targets of the loss."""
    cfg, tag, xs, ctx, t, seq_len, ys, clip = make_golden.tiny_case(model_type, 2)
    targets = [torch.from_numpy(detgen.normalish(f"{TAG}/{model_type}/vt{i}", tuple(u.shape))) for i, u in enumerate(xs)]
    return cfg, tag, xs, ctx, t, seq_len, ys, clip, targets


def chain_case():
    """Cases c and d: the t2v inputs of case a, weights tags of G (also the rollout's model) and D, D's timesteps."""
    cfg, _, xs, ctx, t, seq_len, _, _ = make_golden.tiny_case("t2v", 2)
    return cfg, xs, ctx, t, torch.tensor(T_D), seq_len


def _leaf(v, device="cpu"):
    return v.detach().clone().to(device).requires_grad_(True)


def _np(v):
    return v.detach().cpu().numpy()


def loss_ab(fwd, xs, t, ctx, seq_len, targets, ys=None, clip=None):
    out = fwd(xs, t, ctx, seq_len, clip_fea=clip, y=ys)
    return sum(torch.nn.functional.mse_loss(o, v.to(o.device)) for o, v in zip(out, targets))


def loss_chain(fwd_g, fwd_d, z, t, t_d, ctx, seq_len):
    v = fwd_g(z, t, ctx, seq_len)
    x_hat = [a - b for a, b in zip(z, v)]
    return sum((o ** 2).mean() for o in fwd_d(x_hat, t_d, ctx, seq_len))


def loss_rollout(fwd, x0, t, ctx, seq_len):
    x1 = [a - 0.5 * b for a, b in zip(x0, fwd(x0, t, ctx, seq_len))]
    return sum((o ** 2).mean() for o in fwd(x1, t, ctx, seq_len))


def expected_keys():
    """{key: shape} of the fixture, from the cases alone."""
    keys = {}
    for mt, k in (("t2v", "a"), ("i2v", "b")):
        cfg, _, xs, ctx, t, _, ys, clip, _ = case(mt)
        keys[f"{k}/loss"] = ()
        keys[f"{k}/dt"] = tuple(t.shape)
        for i in range(len(xs)):
            keys[f"{k}/dx{i}"] = tuple(xs[i].shape)
            keys[f"{k}/dcontext{i}"] = tuple(ctx[i].shape)
            if ys is not None:
                keys[f"{k}/dy{i}"] = tuple(ys[i].shape)
        if clip is not None:
            keys[f"{k}/dclip_head"] = (clip.shape[0], CLIP_ROWS, clip.shape[2])
            keys[f"{k}/dclip_norm"] = ()
    cfg, xs, *_ = chain_case()
    shapes = O.param_shapes(cfg)
    for k, dn in (("c", "dz"), ("d", "dx0")):
        keys[f"{k}/loss"] = ()
        for i in range(len(xs)):
            keys[f"{k}/{dn}{i}"] = tuple(xs[i].shape)
        for name in GRAD_NAMES:
            shp = tuple(shapes[name])
            keys[f"{k}/{name}"] = shp if len(shp) == 1 else (min(32, shp[0]),) + shp[1:]
    return keys


def _store_params(res, k, named):
    for name in GRAD_NAMES:
        g = named[name].grad.detach().cpu().numpy()
        res[f"{k}/{name}"] = g if g.ndim == 1 else g[:32]


def compute(make_forward, device="cpu"):
    """All four cases on ``make_forward(cfg, tag, trainable) -> (forward, {name: parameter})`` with the inputs on
    ``device``; returns {key: array}."""
    res = {}
    _leaf = lambda v: globals()["_leaf"](v, device)
    for mt, k in (("t2v", "a"), ("i2v", "b")):
        cfg, tag, xs, ctx, t, seq_len, ys, clip, targets = case(mt)
        fwd, _ = make_forward(cfg, tag, False)
        xs, ctx, t = [_leaf(u) for u in xs], [_leaf(u) for u in ctx], _leaf(t)
        ys = None if ys is None else [_leaf(u) for u in ys]
        clip = None if clip is None else _leaf(clip)
        with torch.enable_grad():
            loss = loss_ab(fwd, xs, t, ctx, seq_len, targets, ys, clip)
            loss.backward()
        res[f"{k}/loss"] = np.float32(loss.item())
        res[f"{k}/dt"] = _np(t.grad)
        for i in range(len(xs)):
            res[f"{k}/dx{i}"] = _np(xs[i].grad)
            res[f"{k}/dcontext{i}"] = _np(ctx[i].grad)
            if ys is not None:
                res[f"{k}/dy{i}"] = _np(ys[i].grad)
        if clip is not None:
            res[f"{k}/dclip_head"] = _np(clip.grad[:, :CLIP_ROWS]).copy()
            res[f"{k}/dclip_norm"] = np.float32(clip.grad.double().norm().item())
    cfg, xs, ctx, t, t_d, seq_len = chain_case()
    ctx, t, t_d = [u.to(device) for u in ctx], t.to(device), t_d.to(device)
    # ---- c: G -> D
    fwd_g, named = make_forward(cfg, TAG_G, True)
    fwd_d, _ = make_forward(cfg, TAG_D, False)
    z = [_leaf(u) for u in xs]
    with torch.enable_grad():
        loss = loss_chain(fwd_g, fwd_d, z, t, t_d, ctx, seq_len)
        loss.backward()
    res["c/loss"] = np.float32(loss.item())
    for i, u in enumerate(z):
        res[f"c/dz{i}"] = _np(u.grad)
    _store_params(res, "c", named)
    # ---- d: two-step rollout
    fwd, named = make_forward(cfg, TAG_G, True)
    x0 = [_leaf(u) for u in xs]
    with torch.enable_grad():
        loss = loss_rollout(fwd, x0, t, ctx, seq_len)
        loss.backward()
    res["d/loss"] = np.float32(loss.item())
    for i, u in enumerate(x0):
        res[f"d/dx0{i}"] = _np(u.grad)
    _store_params(res, "d", named)
    return res


def reference_forward(cfg, tag, trainable):
    """The real reference WanModel with detgen weights."""
    m = ref_import.build_reference_dit(cfg, O.synth_state_dict(cfg, tag))
    m.requires_grad_(trainable)
    return m, dict(m.named_parameters())


def oracle_forward(cfg, tag, trainable):
    """The CPU oracle's formulas under autograd (oracle/wan_dit_oracle.py)."""
    sd = {k: v.clone().requires_grad_(trainable) for k, v in O.synth_state_dict(cfg, tag).items()}

    def fwd(xs, t, ctx, seq_len, clip_fea=None, y=None):
        return O.dit_forward_autograd(sd, cfg, xs, t, ctx, seq_len, clip_fea=clip_fea, y=y)
    return fwd, sd


def main():
    res = compute(reference_forward)
    want = expected_keys()
    assert {k: tuple(np.shape(v)) for k, v in res.items()} == want
    np.savez_compressed(OUT, **res)
    print("input-gradient golden:", {k: float(np.abs(v).mean()) for k, v in res.items()}, "bytes", os.path.getsize(OUT))


if __name__ == "__main__":
    main()
