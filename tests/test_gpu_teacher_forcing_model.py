"""Per-frame timesteps in ``WanModel.forward`` and ``WanModel.forward_teacher_forcing`` / ``causal.forcing_loss``, against
the fp32 restatement tests/teacher_forcing_ref.py (pinned to the oracle in tests/test_interval_mask_host.py): the tiny
t2v model of tests/make_golden_chunk_causal.py (2 layers, 56 tokens per frame), B = 2 clips of 4 latent frames, settings
(frames per chunk, left_chunks) = (1, -1) and (2, 1).  Bounds as in test_gpu_chunk_causal_model.py: forward 8e-3,
gradients 2e-2, loss 2e-2, rollout against the full forward 2e-3."""
import importlib

import pytest
import torch

import make_golden_chunk_causal as MC
import teacher_forcing_ref as R
from conftest import PKG, rel_rms
from oracle import wan_dit_oracle as O

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_GRAD, TOL_LOSS, TOL_ROLLOUT = 8e-3, 2e-2, 2e-2, 2e-3
SETTINGS = ((1, -1), (2, 1))
F, TPF = 4, MC.TOKENS_PER_FRAME
S = F * TPF
GRAD_NAMES = ("blocks.0.self_attn.q.weight", "blocks.0.self_attn.v.weight", "blocks.1.self_attn.o.weight",
              "blocks.1.modulation", "blocks.0.ffn.0.weight", "time_embedding.0.weight", "time_projection.1.bias",
              "head.head.weight", "head.modulation", "patch_embedding.weight")
_REF = {}


@pytest.fixture(scope="module")
def model_mod():
    return importlib.import_module(PKG + ".wan.modules.model")


@pytest.fixture(scope="module")
def causal():
    return importlib.import_module(PKG + ".causal")


def _inputs():
    cfg, _, ctx, _, _ = MC.case()
    g = torch.Generator().manual_seed(7)
    clean = [torch.randn(16, F, 14, 16, generator=g) for _ in range(2)]
    noisy = [torch.randn(16, F, 14, 16, generator=g) for _ in range(2)]
    target = [torch.randn(16, F, 14, 16, generator=g) for _ in range(2)]
    t_frames = torch.tensor([[900., 700., 400., 100.], [50., 250., 650., 950.]])
    return cfg, clean, noisy, target, ctx, t_frames


def _model(model_mod, train=False):
    cfg = _inputs()[0]
    m = model_mod.WanModel(num_layers=2, **MC.make_golden.TINY)
    m.load_state_dict(O.synth_state_dict(cfg, MC.TAG))
    m = m.cuda()
    return m.train() if train else m.eval().requires_grad_(False)


def _cuda(v):
    return [u.cuda() for u in v]


def _tf_mask(causal, fpc, W):
    m = causal.IntervalMask(causal.teacher_forcing_groups(F // fpc, W), fpc * TPF)
    return causal.interval_visible(m, 2 * S, 2 * S)[None].expand(2, -1, -1)


def _ref_tf(causal, fpc, W, grad=False):
    """The restatement of forward_teacher_forcing (and, with ``grad``, its loss and gradients) — computed once."""
    key = ("tf", fpc, W, grad)
    if key in _REF:
        return _REF[key]
    cfg, clean, noisy, target, ctx, t_frames = _inputs()
    t_chunks = t_frames[:, ::fpc].clone()
    sd = O.synth_state_dict(cfg, MC.TAG)
    xc, xn, tc = [u.clone() for u in clean], [u.clone() for u in noisy], t_chunks.clone()
    if grad:
        for v in list(sd.values()) + xc + xn + [tc]:
            v.requires_grad_(True)
    t_all = torch.cat([torch.zeros(2, F), tc.repeat_interleave(fpc, dim=1)], dim=1)
    with torch.set_grad_enabled(grad):
        out = R.forward(sd, cfg, [torch.cat([c, n], 1) for c, n in zip(xc, xn)], t_all, ctx, 2 * S,
                        mask=_tf_mask(causal, fpc, W), segments=2, out_from=F)
        res = dict(out=[o.detach() for o in out], t=t_chunks)
        if grad:
            loss = sum(torch.nn.functional.mse_loss(o, v) for o, v in zip(out, target))
            loss.backward()
            res.update(loss=float(loss), grads={n: sd[n].grad for n in GRAD_NAMES}, d_clean=[u.grad for u in xc],
                       d_noisy=[u.grad for u in xn], d_t=tc.grad)
    _REF[key] = res
    return res


def test_per_frame_t_with_equal_values_is_the_per_sample_forward(model_mod):
    """The same kernels serve both forms (only rows_per_batch and the number of e0 rows differ, and every row of e0 is
    computed alone), so the outputs are equal bit for bit — which also bounds them by 1e-3."""
    cfg, clean, _, _, ctx, _ = _inputs()
    m = _model(model_mod)
    t = torch.tensor([900., 300.]).cuda()
    for setting in (None,) + SETTINGS:
        m.set_causal_chunks(*(setting or (None,)))
        a = m(_cuda(clean), t, _cuda(ctx), S)
        b = m(_cuda(clean), t[:, None].expand(2, F).contiguous(), _cuda(ctx), S)
        for u, v in zip(a, b):
            print(f"{setting}: per-frame against per-sample t rel-RMS {rel_rms(v, u):.2e}")
            assert rel_rms(v, u) < 1e-3
            assert torch.equal(u, v)
    # a longer seq_len: the pad frame takes the last frame's t
    m.set_causal_chunks(None)
    for u, v in zip(m(_cuda(clean), t, _cuda(ctx), S + TPF), m(_cuda(clean), t[:, None].expand(2, F).contiguous(), _cuda(ctx), S + TPF)):
        assert torch.equal(u, v)


def test_per_frame_t_with_distinct_values_forward_and_gradients(model_mod):
    cfg, clean, _, target, ctx, t_frames = _inputs()
    sd = O.synth_state_dict(cfg, MC.TAG)
    xr, tr = [u.clone().requires_grad_(True) for u in clean], t_frames.clone().requires_grad_(True)
    for v in sd.values():
        v.requires_grad_(True)
    out_r = R.forward(sd, cfg, xr, tr, ctx, S)
    loss_r = sum(torch.nn.functional.mse_loss(o, v) for o, v in zip(out_r, target))
    loss_r.backward()
    m = _model(model_mod)
    with torch.no_grad():
        for o, r in zip(m(_cuda(clean), t_frames.cuda(), _cuda(ctx), S), out_r):
            print(f"per-frame t forward rel-RMS {rel_rms(o, r.detach()):.2e}")
            assert rel_rms(o, r.detach()) < TOL_FWD
    m = _model(model_mod, train=True)
    xg, tg = [u.cuda().requires_grad_(True) for u in clean], t_frames.cuda().requires_grad_(True)
    out = m(xg, tg, _cuda(ctx), S)
    loss = sum(torch.nn.functional.mse_loss(o, v.cuda()) for o, v in zip(out, target))
    loss.backward()
    print(f"loss {loss.item():.6f} reference {float(loss_r):.6f}")
    assert abs(loss.item() - float(loss_r)) < TOL_LOSS * float(loss_r)
    params = dict(m.named_parameters())
    for name in GRAD_NAMES:
        err = rel_rms(params[name].grad, sd[name].grad)
        print(f"{name}: rel-RMS {err:.2e}")
        assert err < TOL_GRAD, name
    assert tg.grad.shape == (2, F)
    print(f"t.grad rel-RMS {rel_rms(tg.grad, tr.grad):.2e}, latents {rel_rms(xg[0].grad, xr[0].grad):.2e}")
    assert rel_rms(tg.grad, tr.grad) < TOL_GRAD
    for a, b in zip(xg, xr):
        assert rel_rms(a.grad, b.grad) < TOL_GRAD


@pytest.mark.parametrize("fpc,W", SETTINGS)
def test_teacher_forcing_forward_matches_the_restatement(model_mod, causal, fpc, W):
    cfg, clean, noisy, _, ctx, _ = _inputs()
    ref = _ref_tf(causal, fpc, W)
    m = _model(model_mod)
    m.set_causal_chunks(fpc, W)
    out = m.forward_teacher_forcing(_cuda(clean), _cuda(noisy), ref["t"].cuda(), _cuda(ctx))
    for o, r in zip(out, ref["out"]):
        assert o.shape == (16, F, 14, 16) and o.dtype == torch.float32
        print(f"({fpc}, {W}): teacher forcing forward rel-RMS {rel_rms(o, r):.2e}")
        assert rel_rms(o, r) < TOL_FWD


@pytest.mark.parametrize("fpc,W", SETTINGS)
def test_teacher_forcing_is_the_rollout(model_mod, causal, fpc, W):
    """Noisy chunk I of the teacher-forcing output against forward_chunk of that chunk at t[:, I], the cache committed
    from the clean chunks at context_t."""
    cfg, clean, noisy, _, ctx, t_frames = _inputs()
    t = t_frames[:, ::fpc].cuda()
    m = _model(model_mod)
    m.set_causal_chunks(fpc, W)
    full = m.forward_teacher_forcing(_cuda(clean), _cuda(noisy), t, _cuda(ctx), context_t=0.0)
    cache = causal.KVCache(m, 2, S, "cuda")
    zero = torch.zeros(2, device="cuda")
    for I in range(F // fpc):
        sl = slice(I * fpc, (I + 1) * fpc)
        got = m.forward_chunk([u[:, sl].cuda() for u in noisy], t[:, I].contiguous(), _cuda(ctx), cache, commit=False)
        for b in range(2):
            err = rel_rms(got[b], full[b][:, sl])
            print(f"({fpc}, {W}) chunk {I} clip {b}: rollout against teacher forcing rel-RMS {err:.2e}")
            assert err < TOL_ROLLOUT
        m.forward_chunk([u[:, sl].cuda() for u in clean], zero, _cuda(ctx), cache, commit=True)


def test_teacher_forcing_isolation(model_mod):
    cfg, clean, noisy, _, ctx, t_frames = _inputs()
    m = _model(model_mod)
    m.set_causal_chunks(1, -1)
    t = t_frames.cuda()
    base = m.forward_teacher_forcing(_cuda(clean), _cuda(noisy), t, _cuda(ctx))
    other = [u.clone() for u in noisy]
    for u in other:
        u[:, 0] += 1.0                                       # noisy chunk 0 changes: chunks 1.. do not see it
    out = m.forward_teacher_forcing(_cuda(clean), _cuda(other), t, _cuda(ctx))
    for a, b in zip(out, base):
        assert torch.equal(a[:, 1:], b[:, 1:]) and not torch.equal(a[:, 0], b[:, 0])
    other = [u.clone() for u in clean]
    for u in other:
        u[:, 2] += 1.0                                       # clean chunk 2 changes: only noisy chunk 3 sees it
    out = m.forward_teacher_forcing(_cuda(other), _cuda(noisy), t, _cuda(ctx))
    for a, b in zip(out, base):
        assert torch.equal(a[:, :3], b[:, :3]) and not torch.equal(a[:, 3], b[:, 3])


def _tf_step(model_mod, fpc, W, t, policy=None, keep=False):
    cfg, clean, noisy, target, ctx, _ = _inputs()
    m = _model(model_mod, train=True)
    if policy is not None:
        m.checkpoint_policy = policy
    m.use_checkpoint = not keep
    m.set_causal_chunks(fpc, W)
    xc, xn = [u.cuda().requires_grad_(True) for u in clean], [u.cuda().requires_grad_(True) for u in noisy]
    tg = t.cuda().requires_grad_(True)
    out = m.forward_teacher_forcing(xc, xn, tg, _cuda(ctx))
    loss = sum(torch.nn.functional.mse_loss(o, v.cuda()) for o, v in zip(out, target))
    loss.backward()
    return m, loss, xc, xn, tg


def test_teacher_forcing_training(model_mod, causal):
    """Loss and gradients against autograd through the restatement; then the checkpoint re-run, kept activations and a
    second step for equal bits — under ops.set_deterministic(True), the mode in which the library promises a training
    step that repeats bit for bit (by default a few backward launches, the time MLP's input gradient among them, add
    partial sums with float atomics: test_gpu_input_grads.py, test_gpu_lora.py do the same)."""
    ops = importlib.import_module(PKG + ".ops")
    was = ops.set_deterministic(None)
    ops.set_deterministic(True)
    try:
        _training_checks(model_mod, causal)
    finally:
        ops.set_deterministic(was)


def _training_checks(model_mod, causal):
    fpc, W = SETTINGS[1]
    ref = _ref_tf(causal, fpc, W, grad=True)
    m, loss, xc, xn, tg = _tf_step(model_mod, fpc, W, ref["t"])
    print(f"loss {loss.item():.6f} reference {ref['loss']:.6f}")
    assert abs(loss.item() - ref["loss"]) < TOL_LOSS * ref["loss"]
    params = dict(m.named_parameters())
    for name in GRAD_NAMES:
        err = rel_rms(params[name].grad, ref["grads"][name])
        print(f"{name}: rel-RMS {err:.2e}")
        assert err < TOL_GRAD, name
    assert tg.grad.shape == ref["d_t"].shape
    print(f"t {rel_rms(tg.grad, ref['d_t']):.2e} noisy {rel_rms(xn[0].grad, ref['d_noisy'][0]):.2e} "
          f"clean {rel_rms(xc[0].grad, ref['d_clean'][0]):.2e}")
    assert rel_rms(tg.grad, ref["d_t"]) < TOL_GRAD
    for b in range(2):
        assert rel_rms(xn[b].grad, ref["d_noisy"][b]) < TOL_GRAD and rel_rms(xc[b].grad, ref["d_clean"][b]) < TOL_GRAD
    # the checkpoint re-run, kept activations and a second step: the same bits
    for policy, keep in (("always", False), (None, True), (None, False)):
        other, loss2, _, xn2, tg2 = _tf_step(model_mod, fpc, W, ref["t"], policy, keep)
        op = dict(other.named_parameters())
        assert torch.equal(loss2, loss) and torch.equal(tg2.grad, tg.grad) and torch.equal(xn2[0].grad, xn[0].grad)
        for name in GRAD_NAMES:
            assert torch.equal(op[name].grad, params[name].grad), (policy, keep, name)


def test_teacher_forcing_lora_runs(model_mod):
    cfg, clean, noisy, _, ctx, t_frames = _inputs()
    omh = importlib.import_module(PKG)
    m = _model(model_mod)
    m.set_causal_chunks(2, 1)
    t = t_frames[:, ::2].cuda()
    before = m.forward_teacher_forcing(_cuda(clean), _cuda(noisy), t, _cuda(ctx))
    adapters = omh.add_lora(m, rank=4)
    with torch.no_grad():
        after = m.forward_teacher_forcing(_cuda(clean), _cuda(noisy), t, _cuda(ctx))
    assert torch.equal(after[0], before[0])                  # lora_B = 0: the adapters change nothing yet
    m.forward_teacher_forcing(_cuda(clean), _cuda(noisy), t, _cuda(ctx))[0].square().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in adapters)
    assert any(float(p.grad.abs().sum()) > 0.0 for p in adapters)


@pytest.mark.parametrize("mode", ("teacher", "diffusion"))
def test_forcing_loss(model_mod, causal, mode):
    cfg, clean, noisy, _, ctx, t_frames = _inputs()
    fpc, W = SETTINGS[1]
    n = F // fpc
    sig = torch.tensor([[0.9, 0.3], [0.2, 0.7]])
    t = sig * 1000.0
    sf = sig.repeat_interleave(fpc, 1)
    x_t = [(1 - sf[b].view(1, F, 1, 1)) * clean[b] + sf[b].view(1, F, 1, 1) * noisy[b] for b in range(2)]
    sd = O.synth_state_dict(cfg, MC.TAG)
    with torch.no_grad():
        if mode == "teacher":
            t_all = torch.cat([torch.zeros(2, F), t.repeat_interleave(fpc, 1)], 1)
            out = R.forward(sd, cfg, [torch.cat([c, x], 1) for c, x in zip(clean, x_t)], t_all, ctx, 2 * S,
                            mask=_tf_mask(causal, fpc, W), segments=2, out_from=F)
        else:
            stairs = causal.chunk_causal_visible(S, S, fpc * TPF, W)[None].expand(2, -1, -1)
            out = R.forward(sd, cfg, x_t, t.repeat_interleave(fpc, 1), ctx, S, mask=stairs)
    ref = torch.stack([(o - (e - c)).square().mean() for o, e, c in zip(out, noisy, clean)]).mean()
    m = _model(model_mod)
    m.set_causal_chunks(fpc, W)
    with torch.no_grad():
        got = causal.forcing_loss(m, _cuda(clean), _cuda(noisy), sig.cuda(), t.cuda(), _cuda(ctx), mode=mode)
    print(f"forcing_loss({mode}) {float(got):.6f} reference {float(ref):.6f}")
    assert abs(float(got) - float(ref)) < TOL_LOSS * float(ref)
    assert n == 2
    m = _model(model_mod, train=True)
    m.set_causal_chunks(fpc, W)
    causal.forcing_loss(m, _cuda(clean), _cuda(noisy), sig.cuda(), t.cuda(), _cuda(ctx), mode=mode).backward()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
    with pytest.raises(ValueError):
        causal.forcing_loss(m, _cuda(clean), _cuda(noisy), sig.cuda(), t.cuda(), _cuda(ctx), mode="other")


def test_refusals(model_mod, causal):
    cfg, clean, noisy, _, ctx, t_frames = _inputs()
    m = _model(model_mod)
    x, c, t2 = _cuda(clean), _cuda(ctx), t_frames.cuda()
    with pytest.raises(ValueError):                                              # clips that do not share h, w
        m([x[0], x[1][:, :, :12].contiguous()], t2, c, S)
    with pytest.raises(ValueError):                                              # seq_len no multiple of h w
        m(x, t2, c, S + 8)
    with pytest.raises(ValueError):                                              # t of another frame count
        m(x, t2[:, :3].contiguous(), c, S)
    with pytest.raises(ValueError):                                              # h w no multiple of 8: 7 x 6 = 42 tokens
        m([u[:, :, :, :12].contiguous() for u in x], t2, c, F * 42)
    with pytest.raises(ValueError):                                              # never silently the first column
        m.forward_cfg_pair(x, t2, c, c, S)
    cache = causal.KVCache(m, 2, S, "cuda")
    with pytest.raises(ValueError):
        m.forward_chunk([u[:, :1] for u in x], t2[:, :1], c, cache)
    with pytest.raises(ValueError):                                              # no causal chunks set
        m.forward_teacher_forcing(x, _cuda(noisy), t2, c)
    with pytest.raises(ValueError):
        causal.forcing_loss(m, x, _cuda(noisy), t2, t2, c)
    m.set_causal_chunks(3)
    with pytest.raises(ValueError):                                              # 4 frames are no multiple of 3
        m.forward_teacher_forcing(x, _cuda(noisy), t2, c)
    m.set_causal_chunks(2)
    with pytest.raises(ValueError):                                              # one t per chunk: [2, 2]
        m.forward_teacher_forcing(x, _cuda(noisy), t2, c)
    with pytest.raises(ValueError):                                              # clips of different shapes
        m.forward_teacher_forcing(x, [noisy[0].cuda(), noisy[1][:, :2].cuda()], t2[:, ::2], c)
    m.set_attention_block_mask(torch.ones(4, 4, dtype=torch.bool))
    with pytest.raises(ValueError):                                              # a block mask beside it
        m.forward_teacher_forcing(x, _cuda(noisy), t2[:, ::2], c)
    m.set_attention_block_mask(None)
    w = model_mod.WanModel(num_layers=2, window_size=(70, 30), **MC.make_golden.TINY).cuda().eval().requires_grad_(False)
    w._causal_chunks = (2, -1)                                                   # (set_causal_chunks itself refuses a windowed model)
    with pytest.raises(ValueError):
        w.forward_teacher_forcing(x, _cuda(noisy), t2[:, ::2], c)
