"""Teacher forcing under a pinned sink — ``WanModel.forward_teacher_forcing(pin_sink=True)`` / ``causal.forcing_loss(pin_sink=
True)`` — against the fp32 restatements tests/pinned_sink_ref.py (forward: the rule) and tests/pinned_tf_ref.py (training:
autograd through the extended key axis), and against the rollout it is the training form of: ``forward_chunk`` on a
``causal.RollingKVCache(pin_sink=True)``.  The tiny t2v model of tests/make_golden_chunk_causal.py (2 layers, 2 heads of 128,
56 tokens per frame), B = 2 clips with the inputs of tests/test_gpu_sink_model.py; settings (frames per chunk, W, S, F) =
(1, 1, 1, 6), (2, 1, 1, 8), (1, 0, 2, 6).  Bounds as there: forward 8e-3, gradients and loss 2e-2, rollout 2e-3."""
import importlib

import pytest
import torch

import make_golden_chunk_causal as MC
import pinned_sink_ref as PR
import pinned_tf_ref as PT
from conftest import PKG, rel_rms
from oracle import wan_dit_oracle as O

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_GRAD, TOL_LOSS, TOL_ROLLOUT = 8e-3, 2e-2, 2e-2, 2e-3
SETTINGS = ((1, 1, 1, 6), (2, 1, 1, 8), (1, 0, 2, 6))                            # fpc, W, S, F
TRAIN_SETTINGS = ((1, 0, 2, 6), (1, 1, 1, 6))
TPF = MC.TOKENS_PER_FRAME
GRAD_NAMES = ("blocks.0.self_attn.q.weight", "blocks.0.self_attn.v.weight", "blocks.1.self_attn.o.weight",
              "blocks.1.modulation", "blocks.0.ffn.0.weight", "time_embedding.0.weight", "time_projection.1.bias",
              "head.head.weight", "head.modulation", "patch_embedding.weight",
              "blocks.0.self_attn.k.weight", "blocks.0.self_attn.norm_k.weight")
_REF = {}


@pytest.fixture(scope="module")
def model_mod():
    return importlib.import_module(PKG + ".wan.modules.model")


@pytest.fixture(scope="module")
def causal():
    return importlib.import_module(PKG + ".causal")


def _inputs(F):
    """tests/test_gpu_sink_model.py::_inputs."""
    cfg, _, ctx, _, _ = MC.case()
    g = torch.Generator().manual_seed(17)
    clean = [torch.randn(16, F, 14, 16, generator=g) for _ in range(2)]
    noisy = [torch.randn(16, F, 14, 16, generator=g) for _ in range(2)]
    target = [torch.randn(16, F, 14, 16, generator=g) for _ in range(2)]
    t_frames = torch.stack([torch.linspace(900., 100., F), torch.linspace(50., 950., F)])
    return cfg, clean, noisy, target, ctx, t_frames


def _model(model_mod, train=False):
    cfg = MC.case()[0]
    m = model_mod.WanModel(num_layers=2, **MC.make_golden.TINY)
    m.load_state_dict(O.synth_state_dict(cfg, MC.TAG))
    m = m.cuda()
    return m.train() if train else m.eval().requires_grad_(False)


def _cuda(v):
    return [u.cuda() for u in v]


def _ref_fwd(causal, fpc, W, S, F):
    """The rule, pinned and not (pinned_sink_ref.forward) — once per setting."""
    key = ("fwd", fpc, W, S, F)
    if key not in _REF:
        cfg, clean, noisy, _, ctx, t_frames = _inputs(F)
        sd = O.synth_state_dict(cfg, MC.TAG)
        t = t_frames[:, ::fpc].clone()
        _REF[key] = dict(t=t, pinned=PR.forward(sd, cfg, clean, noisy, t, ctx, causal, fpc, W, S, pinned=True),
                         plain=PR.forward(sd, cfg, clean, noisy, t, ctx, causal, fpc, W, S, pinned=False))
    return _REF[key]


def _ref_train(causal, fpc, W, S, F):
    """Loss and gradients by autograd through the extended-key restatement (pinned_tf_ref.forward) — once per setting."""
    key = ("train", fpc, W, S, F)
    if key not in _REF:
        cfg, clean, noisy, target, ctx, t_frames = _inputs(F)
        sd = O.synth_state_dict(cfg, MC.TAG)
        xc, xn, tc = [u.clone() for u in clean], [u.clone() for u in noisy], t_frames[:, ::fpc].clone()
        for v in list(sd.values()) + xc + xn + [tc]:
            v.requires_grad_(True)
        out = PT.forward(sd, cfg, xc, xn, tc, ctx, causal, fpc, W, S)
        loss = sum(torch.nn.functional.mse_loss(o, v) for o, v in zip(out, target))
        loss.backward()
        _REF[key] = dict(t=tc.detach().clone(), loss=float(loss.detach()), grads={n: sd[n].grad for n in GRAD_NAMES},
                         d_clean=[u.grad for u in xc], d_noisy=[u.grad for u in xn], d_t=tc.grad)
    return _REF[key]


@pytest.mark.parametrize("train", (False, True))
@pytest.mark.parametrize("fpc,W,S,F", SETTINGS)
def test_forward_under_a_pinned_sink(model_mod, causal, fpc, W, S, F, train):
    cfg, clean, noisy, _, ctx, _ = _inputs(F)
    ref = _ref_fwd(causal, fpc, W, S, F)
    deltas = PR.sink_deltas(F // fpc, W, S, fpc)
    m = _model(model_mod, train)
    m.set_causal_chunks(fpc, W, S)
    run = lambda **kw: [o.detach() for o in m.forward_teacher_forcing(_cuda(clean), _cuda(noisy), ref["t"].cuda(), _cuda(ctx), **kw)]
    out, plain = run(pin_sink=True), run()
    assert any(k[0] == "pin" for k in m._tf_masks) and torch.equal(run(pin_sink=False)[0], plain[0])
    for b, (o, u) in enumerate(zip(out, plain)):
        assert o.shape == (16, F, 14, 16) and o.dtype == torch.float32
        err = rel_rms(o, ref["pinned"][b])
        print(f"({fpc}, {W}, {S}) train = {train} clip {b}: pinned teacher forcing rel-RMS {err:.2e}")
        assert err < TOL_FWD
        for I, delta in enumerate(deltas):
            sl = slice(I * fpc, (I + 1) * fpc)
            if delta == 0:                                                       # nothing these chunks see has moved
                assert torch.equal(o[:, sl], u[:, sl]), (b, I)
                continue
            near, far = rel_rms(o[:, sl], ref["pinned"][b][:, sl]), rel_rms(o[:, sl], ref["plain"][b][:, sl])
            apart = rel_rms(ref["pinned"][b][:, sl], ref["plain"][b][:, sl])
            print(f"  chunk {I} (delta {delta}): to the pinned restatement {near:.2e}, to the unpinned {far:.2e} "
                  f"(the two are {apart:.2e} apart)")
            assert near < far, (b, I)
            assert not torch.equal(o[:, sl], u[:, sl])


def test_pinned_teacher_forcing_is_translation_invariant(model_mod, causal):
    """The periodic clip (pinned_sink_ref.periodic_clip) at (1, 1, 1): under the pin every chunk past the wrap computes what
    the last one does; with absolute sink positions the output drifts with the chunk index."""
    cfg, _, ctx, _, _ = MC.case()
    clean, noisy, t = PR.periodic_clip(12)
    m = _model(model_mod)
    m.set_causal_chunks(1, 1, 1)
    pinned = m.forward_teacher_forcing(_cuda(clean), _cuda(noisy), t.cuda(), _cuda(ctx), pin_sink=True)
    plain = m.forward_teacher_forcing(_cuda(clean), _cuda(noisy), t.cuda(), _cuda(ctx))
    for b in range(2):
        for I in range(4, 9):
            ep, eu = rel_rms(pinned[b][:, I], pinned[b][:, 11]), rel_rms(plain[b][:, I], plain[b][:, 11])
            print(f"clip {b} chunk {I} against chunk 11: pinned {ep:.2e}, unpinned {eu:.2e}")
            assert ep < 2e-3 and eu > 2e-3


def _rollout(m, cache, clean, noisy, ctx, t, fpc, F):
    """forward_chunk of every noisy chunk (commit=False) at t[:, I], the cache committed from the clean chunks at 0."""
    zero = torch.zeros(2, device="cuda")
    out = []
    for I in range(F // fpc):
        sl = slice(I * fpc, (I + 1) * fpc)
        out.append(m.forward_chunk([u[:, sl].cuda() for u in noisy], t[:, I].contiguous(), _cuda(ctx), cache, commit=False))
        m.forward_chunk([u[:, sl].cuda() for u in clean], zero, _cuda(ctx), cache, commit=True)
    return out


@pytest.mark.parametrize("fpc,W,S,F", SETTINGS)
def test_pinned_teacher_forcing_is_the_pinned_rollout(model_mod, causal, fpc, W, S, F):
    cfg, clean, noisy, _, ctx, t_frames = _inputs(F)
    t = t_frames[:, ::fpc].cuda()
    m = _model(model_mod)
    m.set_causal_chunks(fpc, W, S)
    full = m.forward_teacher_forcing(_cuda(clean), _cuda(noisy), t, _cuda(ctx), context_t=0.0, pin_sink=True)
    cache = causal.RollingKVCache(m, 2, fpc * TPF, S, W, "cuda", pin_sink=True)
    assert F // fpc > cache.slots                                                # the ring wraps inside the clip
    got = _rollout(m, cache, clean, noisy, ctx, t, fpc, F)
    for I, chunk in enumerate(got):
        for b in range(2):
            err = rel_rms(chunk[b], full[b][:, I * fpc:(I + 1) * fpc])
            print(f"({fpc}, {W}, {S}) chunk {I} clip {b}: pinned rollout against pinned teacher forcing rel-RMS {err:.2e}")
            assert err < TOL_ROLLOUT


def _tf_step(model_mod, setting, t, policy=None, keep=False, pin_sink=True):
    fpc, W, S, F = setting
    cfg, clean, noisy, target, ctx, _ = _inputs(F)
    m = _model(model_mod, train=True)
    if policy is not None:
        m.checkpoint_policy = policy
    m.use_checkpoint = not keep
    m.set_causal_chunks(fpc, W, S)
    xc, xn = [u.cuda().requires_grad_(True) for u in clean], [u.cuda().requires_grad_(True) for u in noisy]
    tg = t.cuda().requires_grad_(True)
    out = m.forward_teacher_forcing(xc, xn, tg, _cuda(ctx), pin_sink=pin_sink)
    loss = sum(torch.nn.functional.mse_loss(o, v.cuda()) for o, v in zip(out, target))
    loss.backward()
    return m, loss, xc, xn, tg


@pytest.mark.parametrize("setting", TRAIN_SETTINGS)
def test_training_under_a_pinned_sink(model_mod, causal, setting):
    """Loss, parameter gradients and x_noisy / x_clean / t gradients against autograd through the extended-key restatement;
    the sink frames of the clean latents' gradient — where every image's dK and dV are folded back — on their own; the
    checkpoint re-run and kept activations give the same bits under ops.set_deterministic(True)."""
    ops = importlib.import_module(PKG + ".ops")
    fpc, W, S, F = setting
    was = ops.set_deterministic(None)
    ops.set_deterministic(True)
    try:
        ref = _ref_train(causal, *setting)
        m, loss, xc, xn, tg = _tf_step(model_mod, setting, ref["t"])
        print(f"{setting}: loss {loss.item():.6f} reference {ref['loss']:.6f}")
        assert abs(loss.item() - ref["loss"]) < TOL_LOSS * ref["loss"]
        params = dict(m.named_parameters())
        for name in GRAD_NAMES:
            err = rel_rms(params[name].grad, ref["grads"][name])
            print(f"{name}: rel-RMS {err:.2e}")
            assert err < TOL_GRAD, name
        print(f"t {rel_rms(tg.grad, ref['d_t']):.2e}")
        assert tg.grad.shape == ref["d_t"].shape and rel_rms(tg.grad, ref["d_t"]) < TOL_GRAD
        for b in range(2):
            en, ec = rel_rms(xn[b].grad, ref["d_noisy"][b]), rel_rms(xc[b].grad, ref["d_clean"][b])
            es = rel_rms(xc[b].grad[:, :S * fpc], ref["d_clean"][b][:, :S * fpc])
            print(f"clip {b}: noisy {en:.2e} clean {ec:.2e} clean sink frames {es:.2e}")
            assert en < TOL_GRAD and ec < TOL_GRAD and es < TOL_GRAD
        for policy, keep in (("always", False), (None, True)):
            other, loss2, xc2, xn2, tg2 = _tf_step(model_mod, setting, ref["t"], policy, keep)
            op = dict(other.named_parameters())
            assert torch.equal(loss2, loss) and torch.equal(tg2.grad, tg.grad) and torch.equal(xn2[0].grad, xn[0].grad)
            assert torch.equal(xc2[1].grad, xc[1].grad)
            for name in GRAD_NAMES:
                assert torch.equal(op[name].grad, params[name].grad), (policy, keep, name)
    finally:
        ops.set_deterministic(was)


@pytest.mark.parametrize("fpc", (1, 2))
def test_a_clip_inside_the_ring_is_todays_call(model_mod, causal, fpc):
    """F = 3 fpc at (fpc, 1, 1): no chunk is shifted, no key is added — equal outputs and gradients, pin or no pin."""
    ops = importlib.import_module(PKG + ".ops")
    setting = (fpc, 1, 1, 3 * fpc)
    assert causal.sink_copy_deltas(3, 1, 1, fpc) == []
    t = _inputs(3 * fpc)[5][:, ::fpc].clone()
    was = ops.set_deterministic(None)
    ops.set_deterministic(True)
    try:
        a, la, xca, xna, ta = _tf_step(model_mod, setting, t, pin_sink=True)
        b, lb, xcb, xnb, tb = _tf_step(model_mod, setting, t, pin_sink=False)
    finally:
        ops.set_deterministic(was)
    assert not any(k[0] == "pin" for k in a._tf_masks)
    assert torch.equal(la, lb) and torch.equal(ta.grad, tb.grad)
    for u, v in zip(xca + xna, xcb + xnb):
        assert torch.equal(u.grad, v.grad)
    pb = dict(b.named_parameters())
    for name, p in a.named_parameters():
        assert (p.grad is None) == (pb[name].grad is None) and (p.grad is None or torch.equal(p.grad, pb[name].grad)), name
    m = _model(model_mod)
    m.set_causal_chunks(*setting[:3])
    cfg, clean, noisy, _, ctx, _ = _inputs(3 * fpc)
    run = lambda **kw: m.forward_teacher_forcing(_cuda(clean), _cuda(noisy), t.cuda(), _cuda(ctx), **kw)
    for u, v in zip(run(pin_sink=True), run()):
        assert torch.equal(u, v)


def test_forcing_loss_and_refusals(model_mod, causal):
    fpc, W, S, F = SETTINGS[0]
    cfg, clean, noise, _, ctx, t_frames = _inputs(F)
    m = _model(model_mod)
    m.set_causal_chunks(fpc, W, S)
    sig = (t_frames / 1000.0).cuda()
    x0, eps, c = _cuda(clean), _cuda(noise), _cuda(ctx)
    loss = causal.forcing_loss(m, x0, eps, sig, t_frames.cuda(), c, pin_sink=True)
    x_t = [(1 - sig[b].view(1, -1, 1, 1)) * x0[b] + sig[b].view(1, -1, 1, 1) * eps[b] for b in range(2)]
    out = m.forward_teacher_forcing(x0, x_t, t_frames.cuda(), c, pin_sink=True)
    want = torch.stack([(o - (e - x)).square().mean() for o, e, x in zip(out, eps, x0)]).mean()
    assert torch.equal(loss, want)
    assert not torch.equal(loss, causal.forcing_loss(m, x0, eps, sig, t_frames.cuda(), c))
    with pytest.raises(ValueError, match="pin_sink"):
        causal.forcing_loss(m, x0, eps, sig, t_frames.cuda(), c, mode="diffusion", pin_sink=True)
    for setting in ((fpc, W), (fpc, -1, S)):                                     # no sink; a sink needs a window
        m.set_causal_chunks(*setting)
        with pytest.raises(ValueError, match="pin_sink"):
            m.forward_teacher_forcing(x0, x_t, t_frames.cuda(), c, pin_sink=True)
        with pytest.raises(ValueError, match="pin_sink"):
            causal.forcing_loss(m, x0, eps, sig, t_frames.cuda(), c, pin_sink=True)
    m.set_causal_chunks(fpc, W, S)
    cache = causal.RollingKVCache(m, 2, fpc * TPF, S, W, "cuda", pin_sink=True)
    with pytest.raises(ValueError, match="self forcing under a pinned sink"):
        m.forward_chunk([u[:, :1] for u in x0], torch.zeros(2, device="cuda"), c, cache, grad=True)
