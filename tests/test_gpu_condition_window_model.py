"""Frame-aligned condition tokens in ``WanModel``: ``extra_conditions = {"tokens", "frames", "window"}`` through ``forward``,
``encode_context`` / ``forward_cfg_pair``, ``forward_teacher_forcing``, ``forward_chunk`` and the rollouts, against the fp32
restatement tests/condition_window_ref.py (pinned to the oracle in tests/test_interval_rect_host.py): the tiny t2v model
of tests/make_golden_chunk_causal.py (2 layers, 56 tokens per frame), B = 2 clips of 4 latent frames, 11 condition tokens
of frames [0, 1, 1, 2, 2, 2, 3, 3, -1, 0, 3] — deliberately unsorted: the restatement keeps the caller's order, the model
sorts.  Bounds as in test_gpu_teacher_forcing_model.py: forward 8e-3, gradients 2e-2, loss 2e-2, rollout against the full
forward 2e-3."""
import importlib

import pytest
import torch

import condition_window_ref as CR
import make_golden_chunk_causal as MC
from conftest import PKG, rel_rms
from oracle import wan_dit_oracle as O

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_GRAD, TOL_LOSS, TOL_ROLLOUT = 8e-3, 2e-2, 2e-2, 2e-3
WINDOWS = ((0, 0), (1, 1), (-1, 0))
SETTINGS = (None, (1, -1), (2, 1))
F, TPF = CR.F_LATENT, CR.TOKENS_PER_FRAME
S = F * TPF
GRAD_NAMES = ("blocks.0.self_attn.q.weight", "blocks.0.self_attn.v.weight", "blocks.1.self_attn.o.weight",
              "blocks.1.modulation", "blocks.0.ffn.0.weight", "time_embedding.0.weight", "time_projection.1.bias",
              "head.head.weight", "head.modulation", "patch_embedding.weight",
              "blocks.0.cross_attn.k.weight", "blocks.1.cross_attn.norm_k.weight")
T = torch.tensor([900., 300.])
mse = torch.nn.functional.mse_loss


@pytest.fixture(scope="module")
def model_mod():
    return importlib.import_module(PKG + ".wan.modules.model")


@pytest.fixture(scope="module")
def causal():
    return importlib.import_module(PKG + ".causal")


def _model(model_mod, train=False):
    cfg = CR.case()[0]
    m = model_mod.WanModel(num_layers=2, **MC.make_golden.TINY)
    m.load_state_dict(O.synth_state_dict(cfg, MC.TAG))
    m = m.cuda()
    return m.train() if train else m.eval().requires_grad_(False)


def _cuda(v):
    return [u.cuda() for u in v]


def _ec(tok, frames, window):
    return {"tokens": tok, "frames": frames, "window": window}


def _cross(causal, cfg, window, setting, segments=1):
    """The dense cross-attention mask of the restatement, columns in the caller's token order."""
    vis = causal.condition_window_visible(F, CR.case()[7], cfg.text_len, window[0], window[1],
                                          None if setting is None else setting[0], segments)
    return vis.repeat_interleave(TPF, 0)


def _stairs(causal, setting):
    return None if setting is None else causal.chunk_causal_visible(S, S, setting[0] * TPF, setting[1])[None].expand(2, -1, -1)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("window", WINDOWS)
def test_forward_matches_the_restatement(model_mod, causal, window, setting):
    cfg, clean, _, _, ctx, _, tok, frames = CR.case()
    sd = O.synth_state_dict(cfg, MC.TAG)
    with torch.no_grad():
        ref = CR.forward(sd, cfg, clean, T[:, None].expand(2, F), ctx, S, extra_tokens=tok,
                         cross_mask=_cross(causal, cfg, window, setting), mask=_stairs(causal, setting))
    m = _model(model_mod)
    m.set_causal_chunks(*(setting or (None,)))
    out = m(_cuda(clean), T.cuda(), _cuda(ctx), S, extra_conditions=_ec(tok.cuda(), frames, window))
    for o, r in zip(out, ref):
        err = rel_rms(o, r)
        print(f"window {window} setting {setting}: forward rel-RMS {err:.2e}")
        assert err < TOL_FWD
    # a ContextState carries the frames and the window: the same bits
    st = m.encode_context(_cuda(ctx), extra_conditions=_ec(tok.cuda(), frames, window))
    for a, b in zip(m(_cuda(clean), T.cuda(), st, S), out):
        assert torch.equal(a, b)


@pytest.mark.parametrize("window,setting", [((0, 0), None), ((1, 1), (2, 1))])
def test_gradients_match_the_restatement(model_mod, causal, window, setting):
    cfg, clean, _, target, ctx, _, tok, frames = CR.case()
    sd = O.synth_state_dict(cfg, MC.TAG)
    xr, tokr = [u.clone().requires_grad_(True) for u in clean], tok.clone().requires_grad_(True)
    for v in sd.values():
        v.requires_grad_(True)
    out_r = CR.forward(sd, cfg, xr, T[:, None].expand(2, F), ctx, S, extra_tokens=tokr,
                       cross_mask=_cross(causal, cfg, window, setting), mask=_stairs(causal, setting))
    loss_r = sum(mse(o, v) for o, v in zip(out_r, target))
    loss_r.backward()
    m = _model(model_mod, train=True)
    m.set_causal_chunks(*(setting or (None,)))
    xg, tokg = [u.cuda().requires_grad_(True) for u in clean], tok.cuda().requires_grad_(True)
    out = m(xg, T.cuda(), _cuda(ctx), S, extra_conditions=_ec(tokg, frames, window))
    loss = sum(mse(o, v.cuda()) for o, v in zip(out, target))
    loss.backward()
    print(f"loss {loss.item():.6f} reference {loss_r.item():.6f}")
    assert abs(loss.item() - loss_r.item()) < TOL_LOSS * loss_r.item()
    params = dict(m.named_parameters())
    for name in GRAD_NAMES:
        err = rel_rms(params[name].grad, sd[name].grad)
        print(f"{name}: rel-RMS {err:.2e}")
        assert err < TOL_GRAD, name
    for a, b in zip(xg, xr):
        assert rel_rms(a.grad, b.grad) < TOL_GRAD
    assert tokg.grad.shape == tok.shape                                          # the caller's order
    print(f"tokens rel-RMS {rel_rms(tokg.grad, tokr.grad):.2e}")
    assert rel_rms(tokg.grad, tokr.grad) < TOL_GRAD


def test_unbounded_window_is_the_plain_call(model_mod):
    """Sorted frames with window (-1, -1): every query sees every token — the bits of the call without 'frames'."""
    cfg, clean, _, _, ctx, _, tok, frames = CR.case()
    order = sorted(range(len(CR.FRAMES)), key=lambda j: (CR.FRAMES[j] < 0, CR.FRAMES[j]))
    tok_s, frames_s = tok[:, order].contiguous().cuda(), frames[order]
    m = _model(model_mod)
    plain = m(_cuda(clean), T.cuda(), _cuda(ctx), S, extra_conditions=tok_s)
    for ec in (_ec(tok_s, frames_s, (-1, -1)), _ec(tok.cuda(), frames, (-1, -1))):   # (unsorted: the model's order is that one)
        for a, b in zip(m(_cuda(clean), T.cuda(), _cuda(ctx), S, extra_conditions=ec), plain):
            assert torch.equal(a, b)
    windowed = m(_cuda(clean), T.cuda(), _cuda(ctx), S, extra_conditions=_ec(tok_s, frames_s, (0, 0)))
    assert not torch.equal(windowed[0], plain[0])


def test_cfg_pair_with_a_windowed_state(model_mod):
    cfg, clean, _, _, ctx, _, tok, frames = CR.case()
    m = _model(model_mod)
    null = [torch.zeros_like(c) for c in ctx]
    st_c = m.encode_context(_cuda(ctx), extra_conditions=_ec(tok.cuda(), frames, (1, 1)))
    st_u = m.encode_context(_cuda(null))
    c, u = m.forward_cfg_pair(_cuda(clean), T.cuda(), st_c, st_u, S)
    for a, b in zip(c, m(_cuda(clean), T.cuda(), st_c, S)):
        assert torch.equal(a, b)
    for a, b in zip(u, m(_cuda(clean), T.cuda(), st_u, S)):
        assert torch.equal(a, b)
    assert not torch.equal(c[0], u[0])


def test_causal_isolation_is_exact(model_mod):
    """Under (fpc 1, W -1) with window (1, 1) nothing of frame 3 reaches frames 0 - 2: other tokens at frame 3 leave their
    outputs bit for bit, and change frame 3's."""
    cfg, clean, _, _, ctx, _, tok, frames = CR.case()
    m = _model(model_mod)
    m.set_causal_chunks(1, -1)
    base = m(_cuda(clean), T.cuda(), _cuda(ctx), S, extra_conditions=_ec(tok.cuda(), frames, (1, 1)))
    other = tok.clone()
    other[:, frames == 3] = torch.randn(2, int((frames == 3).sum()), tok.shape[2], generator=torch.Generator().manual_seed(5))
    out = m(_cuda(clean), T.cuda(), _cuda(ctx), S, extra_conditions=_ec(other.cuda(), frames, (1, 1)))
    for a, b in zip(out, base):
        assert torch.equal(a[:, :3], b[:, :3]) and not torch.equal(a[:, 3], b[:, 3])


def test_module_isolation_is_exact(model_mod, causal):
    """WanT2VCrossAttention.forward alone under window (0, 0): the rows of the frames != g keep their bits when the
    tokens of frame g change."""
    cfg = CR.case()[0]
    m = _model(model_mod)
    ca = m.blocks[0].cross_attn
    d, n_text = cfg.dim, 24
    frames = sorted(f for f in CR.FRAMES if f >= 0) + [-1]
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, S, d, generator=g).cuda()
    context = torch.randn(2, len(frames) + n_text, d, generator=g).cuda()
    lens = torch.tensor([len(frames) + n_text, len(frames) + 17])
    mask = causal.IntervalMask(causal.condition_window_visible(F, torch.tensor(frames), n_text, 0, 0), TPF, "cuda", k_group=1)
    with torch.no_grad():
        base = ca(x, context, lens, interval_mask=mask)
        plain = ca(x, context, lens)
        for fg in range(F):
            other = context.clone()
            cols = torch.tensor([f == fg for f in frames] + [False] * n_text)
            other[:, cols] += 1.0
            out = ca(x, other, lens, interval_mask=mask).view(2, F, TPF, d)
            for f in range(F):
                assert torch.equal(out[:, f], base.view(2, F, TPF, d)[:, f]) == (f != fg)
    assert not torch.equal(base, plain)


@pytest.mark.parametrize("fpc,W", [(1, -1), (2, 1)])
def test_rollout_from_a_stream(model_mod, causal, fpc, W):
    """forward_chunk chunk by chunk, each call given only the tokens that exist by then, against forward under the same
    causal setting; passing all tokens to every chunk gives the bits of passing the slice."""
    cfg, clean, _, _, ctx, _, tok, frames = CR.case()
    window = (1, 1)
    m = _model(model_mod)
    m.set_causal_chunks(fpc, W)
    full = m(_cuda(clean), T.cuda(), _cuda(ctx), S, extra_conditions=_ec(tok.cuda(), frames, window))
    results = []
    for stream in (True, False):
        cache = causal.KVCache(m, 2, S, "cuda")
        outs = []
        for I in range(F // fpc):
            sl = slice(I * fpc, (I + 1) * fpc)
            keep = frames <= (I + 1) * fpc - 1 if stream else torch.ones_like(frames, dtype=torch.bool)   # (-1 included)
            ec = _ec(tok[:, keep].cuda(), frames[keep], window)
            outs.append(m.forward_chunk([u[:, sl].cuda() for u in clean], T.cuda(), _cuda(ctx), cache, commit=True,
                                        extra_conditions=ec))
        results.append(outs)
    for I, outs in enumerate(results[0]):
        for b in range(2):
            err = rel_rms(outs[b], full[b][:, I * fpc:(I + 1) * fpc])
            print(f"({fpc}, {W}) chunk {I} clip {b}: rollout against forward rel-RMS {err:.2e}")
            assert err < TOL_ROLLOUT
    for a, b in zip(results[0], results[1]):
        for u, v in zip(a, b):
            assert torch.equal(u, v)


@pytest.mark.parametrize("fpc,W", [(1, -1), (2, 1)])
def test_teacher_forcing_matches_the_restatement(model_mod, causal, fpc, W):
    cfg, clean, noisy, _, ctx, t_frames, tok, frames = CR.case()
    window = (1, 0)
    t_chunks = t_frames[:, ::fpc].clone()
    sd = O.synth_state_dict(cfg, MC.TAG)
    tf = causal.interval_visible(causal.IntervalMask(causal.teacher_forcing_groups(F // fpc, W), fpc * TPF), 2 * S, 2 * S)
    t_all = torch.cat([torch.zeros(2, F), t_chunks.repeat_interleave(fpc, dim=1)], dim=1)
    with torch.no_grad():
        ref = CR.forward(sd, cfg, [torch.cat([c, n], 1) for c, n in zip(clean, noisy)], t_all, ctx, 2 * S, extra_tokens=tok,
                         cross_mask=_cross(causal, cfg, window, (fpc, W), segments=2), mask=tf[None].expand(2, -1, -1),
                         segments=2, out_from=F)
    m = _model(model_mod)
    m.set_causal_chunks(fpc, W)
    out = m.forward_teacher_forcing(_cuda(clean), _cuda(noisy), t_chunks.cuda(), _cuda(ctx),
                                    extra_conditions=_ec(tok.cuda(), frames, window))
    for o, r in zip(out, ref):
        err = rel_rms(o, r)
        print(f"({fpc}, {W}): teacher forcing forward rel-RMS {err:.2e}")
        assert o.shape == (16, F, 14, 16) and err < TOL_FWD


def test_chunk_token_gradients(model_mod, causal):
    """forward_chunk(grad=True) of the frames 2, 3 at frame_offset 2 on an empty cache (fpc 2), window (1, 1): the token
    gradients against the restatement of that chunk, in the caller's order; tokens of frame 0 get none."""
    cfg, clean, _, target, ctx, _, tok, frames = CR.case()
    window, fpc = (1, 1), 2
    sd = O.synth_state_dict(cfg, MC.TAG)
    tokr = tok.clone().requires_grad_(True)
    vis = causal.condition_window_visible(fpc, frames, cfg.text_len, window[0], window[1], fpc, 1, 2).repeat_interleave(TPF, 0)
    out_r = CR.forward(sd, cfg, [u[:, 2:4] for u in clean], T[:, None].expand(2, fpc), ctx, fpc * TPF, extra_tokens=tokr,
                       cross_mask=vis, frame_offset=2)
    loss_r = sum(mse(o, v[:, 2:4]) for o, v in zip(out_r, target))
    loss_r.backward()
    m = _model(model_mod)
    m.set_causal_chunks(fpc, 1)
    cache = causal.KVCache(m, 2, S, "cuda")
    tokg = tok.cuda().requires_grad_(True)
    out = m.forward_chunk([u[:, 2:4].cuda() for u in clean], T.cuda(), _cuda(ctx), cache, frame_offset=2, commit=False,
                          grad=True, extra_conditions=_ec(tokg, frames, window))
    for o, r in zip(out, out_r):
        assert rel_rms(o.detach(), r.detach()) < TOL_FWD
    loss = sum(mse(o, v[:, 2:4].cuda()) for o, v in zip(out, target))
    loss.backward()
    assert abs(loss.item() - loss_r.item()) < TOL_LOSS * loss_r.item()
    print(f"chunk tokens rel-RMS {rel_rms(tokg.grad, tokr.grad):.2e}")
    assert tokg.grad.shape == tok.shape and rel_rms(tokg.grad, tokr.grad) < TOL_GRAD
    unseen = frames == 0
    assert float(tokg.grad[:, unseen].abs().sum()) == 0.0 and float(tokr.grad[:, unseen].abs().sum()) == 0.0
    assert bool((tokg.grad[:, ~unseen].abs().sum((0, 2)) > 0).all())


def test_self_forcing_rollout_takes_the_tokens(model_mod, causal):
    """The rollout runs with frame-aligned tokens; their gradient is non-zero only where some chunk can see them."""
    cfg, clean, noisy, target, ctx, _, tok, frames = CR.case()
    frames = frames.clone()
    frames[10] = F + 2                                                           # a token of a frame behind the clip: nobody sees it
    m = _model(model_mod)
    tokg = tok.cuda().requires_grad_(True)
    clips = causal.self_forcing_rollout(m, _cuda(noisy), _cuda(ctx), frames_per_chunk=2, left_chunks=1, sigmas=[1.0, 0.6, 0.3],
                                        timesteps=[1000., 600., 300.], exit_step=[1, 2],
                                        generator=torch.Generator(device="cuda").manual_seed(3),
                                        extra_conditions=_ec(tokg, frames, (0, 0)))
    assert len(clips) == 2 and all(c.shape == (16, F, 14, 16) and c.requires_grad for c in clips)
    sum(mse(c, v.cuda()) for c, v in zip(clips, target)).backward()
    per_token = tokg.grad.abs().sum((0, 2))
    assert torch.isfinite(tokg.grad).all()
    assert float(per_token[10]) == 0.0
    assert bool((per_token[:10] > 0).all())
    with torch.no_grad():                                                        # and the sampler: the conditional branch only
        make = lambda: _Euler()
        lat = causal.sample(m, noisy[0].cuda(), [ctx[0].cuda()], [torch.zeros_like(ctx[0]).cuda()], frames_per_chunk=2,
                            left_chunks=1, make_scheduler=make, guide_scale=2.0,
                            extra_conditions=_ec(tok[:1].cuda(), frames, (0, 0)))
        plain = causal.sample(m, noisy[0].cuda(), [ctx[0].cuda()], [torch.zeros_like(ctx[0]).cuda()], frames_per_chunk=2,
                              left_chunks=1, make_scheduler=make, guide_scale=2.0)
    assert lat.shape == (16, F, 14, 16) and torch.isfinite(lat).all() and not torch.equal(lat, plain)


class _Euler:
    """Two Euler steps of the flow ODE with classifier-free guidance: what ``causal.sample`` needs of a scheduler."""
    timesteps = torch.tensor([1000., 500.])

    def step_cfg(self, cond, uncond, scale, lat):
        return lat - 0.5 * (uncond + scale * (cond - uncond))
