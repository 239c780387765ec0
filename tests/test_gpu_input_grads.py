"""Gradients w.r.t. the INPUTS of WanModel.forward — latents x, conditioning channels y, text context, CLIP tokens,
timestep t — against the reference's own autograd (tests/golden/dit_input_grads.npz, made by
tests/make_golden_input_grads.py), the routing rules (a frozen model whose input requires grad takes the training
forward and forms no weight gradient), the forms an input may take, and the two kernels behind the last mile:
omh_patchify_bwd and omh_sinusoidal_embedding_bwd.

Bounds (tests/test_gpu_train.py): 2e-2 for dx, dy, dcontext, dclip_fea and parameter matrices — dx
and dy are one GEMM past the dxs that patch_embedding.weight is held to 2e-2 with, dcontext one GEMM past the dpre of
text_embedding.0.weight, dclip_fea sits where img_emb.proj.0 is held — and 4e-2 for dt and 1-D parameters.
Every figure is printed before it is asserted; with OMH_INPUT_GRAD_PARITY_OUT=<file> the module also writes them there
(the record kept as profiles/input_grad_parity.json)."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import make_golden_input_grads as MG
from conftest import PKG, rel_rms

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "dit_input_grads.npz")
TOL_TINY = 8.0e-3       # the tiny goldens' forward bound (test_gpu_dit.py)
TOL_GRAD = 2e-2         # matrices and input tensors
TOL_GRAD_1D = 4e-2      # 1-D parameters and dt
_FIGURES = {}


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    path = os.environ.get("OMH_INPUT_GRAD_PARITY_OUT")
    if path and _FIGURES:
        with open(path, "w") as fh:
            json.dump(_FIGURES, fh, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def model_mod():
    return importlib.import_module(PKG + ".wan.modules.model")


@pytest.fixture(scope="module")
def mt():
    return importlib.import_module(PKG + ".wan.modules.model_train")


def _check(key, got, ref):
    """rel-RMS of one tensor against the fixture: printed, recorded, then asserted."""
    ref = torch.from_numpy(np.asarray(ref))
    got = torch.as_tensor(np.asarray(got))
    err = rel_rms(got, ref)
    bound = TOL_GRAD_1D if (key.endswith("/dt") or (ref.dim() == 1 and key.endswith(".weight"))) else TOL_GRAD
    _FIGURES[key] = {"rel_rms": err, "bound": bound}
    print(f"input-grad parity {key}: {err:.3e} (bound {bound:.0e})")
    return err, bound


def _model(model_mod, cfg, tag, trainable):
    from oracle import make_golden, wan_dit_oracle as O
    m = model_mod.WanModel(model_type=cfg.model_type, in_dim=cfg.in_dim, num_layers=cfg.num_layers, **make_golden.TINY)
    m.load_state_dict(O.synth_state_dict(cfg, tag))
    m = m.cuda()
    m = m.train() if trainable else m.eval()
    return m.requires_grad_(trainable)


def _maker(model_mod, made):
    def make(cfg, tag, trainable):
        m = _model(model_mod, cfg, tag, trainable)
        made.append(m)

        def fwd(xs, t, ctx, seq_len, clip_fea=None, y=None):
            return m(xs, t, ctx, seq_len, clip_fea=clip_fea, y=y)
        return fwd, dict(m.named_parameters())
    return make


def _leaf(v):
    return v.detach().clone().cuda().requires_grad_(True)


# ------------------------------------------------------------------------------------------- model-level parity
@pytest.mark.parametrize("model_type,k", [("t2v", "a"), ("i2v", "b")])
def test_input_gradients_match_reference(model_mod, model_type, k):
    """Cases a and b: a frozen model, every input a leaf; outputs at the tiny goldens' bound, every input gradient
    against the reference's autograd."""
    g = np.load(GOLD)
    fwd_gold = np.load(os.path.join(HERE, "golden", f"dit_{model_type}_L2.npz"))
    cfg, tag, xs, ctx, t, seq_len, ys, clip, targets = MG.case(model_type)
    m = _model(model_mod, cfg, tag, False)
    xs, ctx, t = [_leaf(u) for u in xs], [_leaf(u) for u in ctx], _leaf(t)
    ys = None if ys is None else [_leaf(u) for u in ys]
    clip = None if clip is None else _leaf(clip)
    out = m(xs, t, ctx, seq_len, clip_fea=clip, y=ys)
    for o, key in zip(out, ("out0", "out1")):
        assert o.requires_grad and rel_rms(o.detach(), torch.from_numpy(fwd_gold[key])) < TOL_TINY
    loss = sum(torch.nn.functional.mse_loss(o, v.cuda()) for o, v in zip(out, targets))
    assert abs(loss.item() - float(g[f"{k}/loss"])) < 2e-2 * float(g[f"{k}/loss"])
    loss.backward()
    assert all(p.grad is None for p in m.parameters())
    got = {f"{k}/dt": t.grad}
    for i in range(len(xs)):
        got[f"{k}/dx{i}"], got[f"{k}/dcontext{i}"] = xs[i].grad, ctx[i].grad
        if ys is not None:
            got[f"{k}/dy{i}"] = ys[i].grad
    results = []
    for key, val in got.items():
        assert val is not None, key
        assert val.shape == tuple(g[key].shape) and val.dtype == torch.float32 and val.is_cuda
        results.append((key,) + _check(key, val.cpu().numpy(), g[key]))
    if clip is not None:
        assert clip.grad is not None and clip.grad.shape == clip.shape
        results.append((f"{k}/dclip_head",) + _check(f"{k}/dclip_head", clip.grad[:, :MG.CLIP_ROWS].cpu().numpy(),
                                                      g[f"{k}/dclip_head"]))
        norm = float(clip.grad.double().norm())
        _FIGURES[f"{k}/dclip_norm"] = {"got": norm, "ref": float(g[f"{k}/dclip_norm"])}
        assert abs(norm - float(g[f"{k}/dclip_norm"])) < TOL_GRAD * float(g[f"{k}/dclip_norm"])
    for key, err, bound in results:
        assert err < bound, (key, err)


def test_chain_and_rollout_match_reference(model_mod):
    """Cases c and d: the gradient through a frozen D into a trainable G (D's parameters get none), and through two
    calls of one model."""
    g = np.load(GOLD)
    made = []
    cfg, xs, ctx, t, t_d, seq_len = MG.chain_case()
    ctx, t, t_d = [u.cuda() for u in ctx], t.cuda(), t_d.cuda()
    make = _maker(model_mod, made)
    res = {}
    fwd_g, named = make(cfg, MG.TAG_G, True)
    fwd_d, _ = make(cfg, MG.TAG_D, False)
    z = [_leaf(u) for u in xs]
    loss = MG.loss_chain(fwd_g, fwd_d, z, t, t_d, ctx, seq_len)
    loss.backward()
    assert abs(loss.item() - float(g["c/loss"])) < 2e-2 * float(g["c/loss"])
    assert all(p.grad is None for p in made[1].parameters())               # D is frozen
    for i, u in enumerate(z):
        res[f"c/dz{i}"] = u.grad.cpu().numpy()
    for name in MG.GRAD_NAMES:
        gg = named[name].grad.cpu().numpy()
        res[f"c/{name}"] = gg if gg.ndim == 1 else gg[:32]
    fwd, named = make(cfg, MG.TAG_G, True)
    x0 = [_leaf(u) for u in xs]
    loss = MG.loss_rollout(fwd, x0, t, ctx, seq_len)
    loss.backward()
    assert abs(loss.item() - float(g["d/loss"])) < 2e-2 * float(g["d/loss"])
    for i, u in enumerate(x0):
        res[f"d/dx0{i}"] = u.grad.cpu().numpy()
    for name in MG.GRAD_NAMES:
        gg = named[name].grad.cpu().numpy()
        res[f"d/{name}"] = gg if gg.ndim == 1 else gg[:32]
    results = [(key,) + _check(key, val, g[key]) for key, val in res.items()]
    for key, err, bound in results:
        assert err < bound, (key, err)


# ------------------------------------------------------------------------------------------- routing and cost
def _t2v(model_mod, trainable):
    cfg, tag, xs, ctx, t, seq_len, _, _, targets = MG.case("t2v")
    m = _model(model_mod, cfg, tag, trainable)
    return m, xs, [c.cuda() for c in ctx], t.cuda(), seq_len, [v.cuda() for v in targets]


def _step(m, xs, ctx, t, seq_len, targets):
    out = m(xs, t, ctx, seq_len)
    sum(torch.nn.functional.mse_loss(o, v) for o, v in zip(out, targets)).backward()


def test_frozen_and_trainable_give_the_same_dx(model_mod, ops):
    ops.set_deterministic(True)
    m, xs, ctx, t, seq_len, targets = _t2v(model_mod, False)
    x_f = [_leaf(u) for u in xs]
    out = m(x_f, t, ctx, seq_len)
    assert all(o.requires_grad for o in out)                               # not the inference branch's detached outputs
    sum(torch.nn.functional.mse_loss(o, v) for o, v in zip(out, targets)).backward()
    m.requires_grad_(True)
    x_t = [_leaf(u) for u in xs]
    _step(m, x_t, ctx, t, seq_len, targets)
    for a, b in zip(x_f, x_t):
        assert a.grad is not None and torch.equal(a.grad, b.grad)
    # ... and asking for the input's gradient does not change a parameter's
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    _step(m, [u.cuda() for u in xs], ctx, t, seq_len, targets)
    assert grads and all(torch.equal(grads[n], p.grad) for n, p in m.named_parameters() if p.grad is not None)
    assert {n for n, p in m.named_parameters() if p.grad is not None} == set(grads)


def test_frozen_model_forms_no_weight_gradient(model_mod, mt, monkeypatch):
    calls = {"grouped": 0, "tn": 0}
    grouped, tn = mt.ops.gemm_tn_grouped, mt.ops.gemm_tn

    def count_grouped(problems):
        calls["grouped"] += 1
        return grouped(problems)

    def count_tn(*a, **k):
        calls["tn"] += 1
        return tn(*a, **k)
    monkeypatch.setattr(mt.ops, "gemm_tn_grouped", count_grouped)
    monkeypatch.setattr(mt.ops, "gemm_tn", count_tn)
    m, xs, ctx, t, seq_len, targets = _t2v(model_mod, False)
    x, c, tt = [_leaf(u) for u in xs], [_leaf(u) for u in ctx], _leaf(t)
    _step(m, x, c, tt, seq_len, targets)
    assert all(u.grad is not None and torch.isfinite(u.grad).all() and u.grad.abs().max() > 0 for u in x + c + [tt])
    assert calls == {"grouped": 0, "tn": 0}
    m.requires_grad_(True)                                                  # the counter does see a trainable step
    _step(m, [u.cuda() for u in xs], ctx, t, seq_len, targets)
    assert calls["grouped"] > 0 and calls["tn"] > 0


def test_inference_paths_stay_inference(model_mod):
    """No grad-requiring input, or no_grad: the frozen model's inference branch, same bits, detached outputs; a
    ContextState next to a grad-requiring input is refused like in training."""
    m, xs, ctx, t, seq_len, _ = _t2v(model_mod, False)
    x = [u.cuda() for u in xs]
    base = m(x, t, ctx, seq_len)
    assert not any(o.requires_grad for o in base)
    with torch.no_grad():
        again = m([_leaf(u) for u in xs], t, ctx, seq_len)
    assert all(torch.equal(a, b) and not b.requires_grad for a, b in zip(base, again))
    cond, _ = m.forward_cfg_pair([_leaf(u) for u in xs], t, ctx, [c[:5] for c in ctx], seq_len)
    assert all(torch.equal(a, b) and not b.requires_grad for a, b in zip(base, cond))
    st = m.encode_context(ctx)
    with pytest.raises(ValueError):
        m([_leaf(u) for u in xs], t, st, seq_len)


# ------------------------------------------------------------------------------------------- forms of input
def test_batched_tensor_x_and_autograd_grad(model_mod, ops):
    ops.set_deterministic(True)
    m, xs, ctx, t, seq_len, _ = _t2v(model_mod, True)
    xb = torch.stack([xs[0], xs[0].flip(1)]).cuda().requires_grad_(True)       # [B, C, F, H, W]
    out = m(xb, t, ctx, seq_len)
    (gb,) = torch.autograd.grad(sum((o ** 2).mean() for o in out), xb)
    assert gb.shape == xb.shape and all(p.grad is None for p in m.parameters())
    xl = [_leaf(u) for u in xb.detach()]
    out = m(xl, t, ctx, seq_len)
    gl = torch.autograd.grad(sum((o ** 2).mean() for o in out), xl)
    assert torch.equal(gb, torch.stack(gl)) and gb.abs().max() > 0


def test_create_graph_raises(model_mod):
    m, xs, ctx, t, seq_len, _ = _t2v(model_mod, False)
    x = [_leaf(u) for u in xs]
    out = m(x, t, ctx, seq_len)
    with pytest.raises(RuntimeError, match="double backward|create_graph"):
        torch.autograd.grad(sum((o ** 2).mean() for o in out), x, create_graph=True)


def test_block_hooks_see_outputs_and_taps_carry_gradient(model_mod):
    m, xs, ctx, t, seq_len, _ = _t2v(model_mod, False)
    taps = []
    handles = [blk.register_forward_hook(lambda mod, inp, out: taps.append(out)) for blk in m.blocks]
    x = [_leaf(u) for u in xs]
    out = m(x, t, ctx, seq_len)
    for h in handles:
        h.remove()
    assert len(taps) == len(m.blocks) and all(tp.shape == (2, seq_len, m.dim) and tp.requires_grad for tp in taps)
    # The backward is linear in the incoming gradient only up to its bf16 roundings: every branch of a block rounds its
    # gradient to bf16 before the dgrad GEMMs (2^-9 relative per rounding, about ten roundings in sequence through the
    # two blocks, independent in the three passes below), which is the noise the gradients are held to TOL_GRAD against
    # the fp32 reference for.  So the sum rule is asked at TOL_GRAD — and the tap's share of the gradient has to exceed
    # that noise by far, or the check would say nothing: the tap's loss is weighted to the size of the output's.
    loss_out = lambda: sum((o ** 2).mean() for o in out)
    loss_tap = lambda: 10.0 * taps[0].square().mean()
    g_tap = torch.autograd.grad(loss_tap(), x, retain_graph=True)
    assert all(torch.isfinite(v).all() and v.abs().max() > 0 for v in g_tap)
    g_out = torch.autograd.grad(loss_out(), x, retain_graph=True)
    g_both = torch.autograd.grad(loss_out() + loss_tap(), x)
    for a, b, c in zip(g_tap, g_out, g_both):
        err, share = rel_rms(c, a + b), rel_rms(c, b)
        print(f"tap sum rule: {err:.3e} (bound {TOL_GRAD:.0e}); the tap's share of the gradient: {share:.3e}")
        assert share > 10 * TOL_GRAD                                          # the tap's gradient is in g_both ...
        assert err < TOL_GRAD                                                 # ... and adds to the output's


# ------------------------------------------------------------------------------------------- omh_patchify_bwd
def _patchify_bwd_ref(dtok, grid, patch, shape):
    C, F, H, W = shape
    f, h, w = grid
    pt, ph, pw = patch
    kin = C * pt * ph * pw
    core = dtok[:f * h * w, :kin].reshape(f, h, w, C, pt, ph, pw).permute(3, 0, 4, 1, 5, 2, 6).reshape(C, f * pt, h * ph, w * pw)
    out = torch.zeros(C, F, H, W, dtype=torch.float32, device=dtok.device)
    out[:, :f * pt, :h * ph, :w * pw] = core
    return out


@pytest.mark.parametrize("shape,patch,split", [
    ((16, 1, 60, 104), (1, 2, 2), None), ((16, 21, 60, 104), (1, 2, 2), None), ((36, 21, 60, 104), (1, 2, 2), 16),
    ((16, 3, 7, 11), (1, 2, 2), None),          # H and W not multiples of the patch: one lane per element
    ((20, 3, 9, 16), (2, 2, 2), 4),             # a frame and a row no patch covers, 16-byte stores
    ((36, 1, 4, 256), (1, 2, 2), 16)])          # more patch columns than one workgroup's tile holds
def test_patchify_bwd_is_the_index_permutation(ops, shape, patch, split):
    C, F, H, W = shape
    pt, ph, pw = patch
    grid = (F // pt, H // ph, W // pw)
    kin = C * pt * ph * pw
    Kp = (kin + 7) // 8 * 8
    gen = torch.Generator(device="cuda").manual_seed(C * F + W)
    dtok = torch.randn(grid[0] * grid[1] * grid[2], Kp, device="cuda", generator=gen)
    ref = _patchify_bwd_ref(dtok, grid, patch, shape)
    cs = C if split is None else split
    nan = lambda n: torch.full((n, F, H, W), float("nan"), device="cuda")      # proves that every element is written
    o0, o1 = nan(cs), (nan(C - cs) if cs < C else None)
    ops.patchify_bwd(dtok, grid, patch, shape, c_split=split, out=(o0, o1))
    assert torch.equal(o0, ref[:cs]) and (o1 is None or torch.equal(o1, ref[cs:]))
    a0, a1 = ops.patchify_bwd(dtok, grid, patch, shape, c_split=split)
    assert torch.equal(a0, ref[:cs]) and ((a1 is None) == (cs == C)) and (a1 is None or torch.equal(a1, ref[cs:]))
    if cs < C:                                                                  # one destination null
        only0, none1 = ops.patchify_bwd(dtok, grid, patch, shape, c_split=split, need=(True, False))
        none0, only1 = ops.patchify_bwd(dtok, grid, patch, shape, c_split=split, need=(False, True))
        assert none0 is None and none1 is None and torch.equal(only0, ref[:cs]) and torch.equal(only1, ref[cs:])
    if (F % pt, H % ph, W % pw) == (0, 0, 0):
        # adjointness <patchify(x), g> == <x, patchify_bwd(g)>: exact for an x that bf16 holds (patchify rounds to bf16)
        x = torch.randn(shape, device="cuda", generator=gen).bfloat16().float()
        lhs = (ops.patchify(x, patch, Kp).double() * dtok.double()).sum()
        rhs = (x.double() * ref.double()).sum()
        assert abs(float(lhs - rhs)) < 1e-9 * float((x.double().abs() * ref.double().abs()).sum())


def test_patchify_bwd_row_stride(ops):
    """The token gradients may sit in a wider buffer (row stride > Kp)."""
    shape, patch, grid = (16, 2, 6, 8), (1, 2, 2), (2, 3, 4)
    buf = torch.randn(24, 96, device="cuda")
    a0, _ = ops.patchify_bwd(buf[:, :64], grid, patch, shape)
    assert torch.equal(a0, _patchify_bwd_ref(buf[:, :64].contiguous(), grid, patch, shape))


# ------------------------------------------------------------------------------------------- omh_sinusoidal_embedding_bwd
def test_sinusoidal_embedding_bwd(ops):
    from oracle import wan_dit_oracle as O
    t = torch.tensor([0., 1., 500., 999., 1000.])
    gen = torch.Generator().manual_seed(3)
    dsin = torch.randn(5, 256, generator=gen)
    t64 = t.double().requires_grad_(True)
    (O.sinusoidal_embedding_1d(256, t64).double() * dsin.double()).sum().backward()
    got = ops.sinusoidal_embedding_bwd(dsin.cuda(), t.cuda())
    assert got.shape == (5,) and got.dtype == torch.float32
    assert float((got.cpu().double() - t64.grad).abs().max()) < 1e-6        # the forward's bound (test_gpu_kernels.py)
