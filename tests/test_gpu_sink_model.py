"""The frame-causal student with an attention sink plus a window: ``set_causal_chunks(fpc, W, S)`` in ``forward``,
``forward_teacher_forcing`` (the three-run interval kernels), training, and the rollout on a ``causal.RollingKVCache`` —
against the fp32 restatement tests/teacher_forcing_ref.py under the dense sink masks.  The tiny t2v model of
tests/make_golden_chunk_causal.py (2 layers, 56 tokens per frame), B = 2 clips; settings (frames per chunk, W, S) =
(1, 1, 1) with 6 latent frames and (2, 1, 1) with 8.  Bounds as in test_gpu_teacher_forcing_model.py: forward 8e-3,
gradients and loss 2e-2, rollout 2e-3."""
import importlib

import pytest
import torch

import make_golden_chunk_causal as MC
import teacher_forcing_ref as R
from conftest import PKG, rel_rms
from oracle import wan_dit_oracle as O

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_GRAD, TOL_LOSS, TOL_ROLLOUT = 8e-3, 2e-2, 2e-2, 2e-3
SETTINGS = ((1, 1, 1, 6), (2, 1, 1, 8))                                          # fpc, W, S, F
TPF = MC.TOKENS_PER_FRAME
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


def _inputs(F):
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


def _tf_mask(causal, fpc, W, S, F):
    m = causal.IntervalMask(causal.teacher_forcing_groups(F // fpc, W, S), fpc * TPF, runs=3)
    return causal.interval_visible(m, 2 * F * TPF, 2 * F * TPF)[None].expand(2, -1, -1)


def _sink_mask(causal, fpc, W, S, F):
    n = -(-F // fpc)
    m = causal.IntervalMask(causal.sink_window_groups(n, S, W), fpc * TPF)
    return causal.interval_visible(m, n * fpc * TPF, n * fpc * TPF)[:F * TPF, :F * TPF][None].expand(2, -1, -1)


def _ref_tf(causal, fpc, W, S, F, grad=False):
    """The restatement of forward_teacher_forcing under the dense sink mask (with ``grad``: loss and gradients) — once."""
    key = (fpc, W, S, F, grad)
    if key in _REF:
        return _REF[key]
    cfg, clean, noisy, target, ctx, t_frames = _inputs(F)
    t_chunks = t_frames[:, ::fpc].clone()
    sd = O.synth_state_dict(cfg, MC.TAG)
    xc, xn, tc = [u.clone() for u in clean], [u.clone() for u in noisy], t_chunks.clone()
    if grad:
        for v in list(sd.values()) + xc + xn + [tc]:
            v.requires_grad_(True)
    t_all = torch.cat([torch.zeros(2, F), tc.repeat_interleave(fpc, dim=1)], dim=1)
    with torch.set_grad_enabled(grad):
        out = R.forward(sd, cfg, [torch.cat([c, n], 1) for c, n in zip(xc, xn)], t_all, ctx, 2 * F * TPF,
                        mask=_tf_mask(causal, fpc, W, S, F), segments=2, out_from=F)
        res = dict(out=[o.detach() for o in out], t=t_chunks)
        if grad:
            loss = sum(torch.nn.functional.mse_loss(o, v) for o, v in zip(out, target))
            loss.backward()
            res.update(loss=float(loss.detach()), grads={n: sd[n].grad for n in GRAD_NAMES}, d_clean=[u.grad for u in xc],
                       d_noisy=[u.grad for u in xn], d_t=tc.grad)
    _REF[key] = res
    return res


@pytest.mark.parametrize("fpc,W,S,F", SETTINGS)
def test_teacher_forcing_forward_with_a_sink(model_mod, causal, fpc, W, S, F):
    cfg, clean, noisy, _, ctx, _ = _inputs(F)
    ref = _ref_tf(causal, fpc, W, S, F)
    m = _model(model_mod)
    m.set_causal_chunks(fpc, W, S)
    out = m.forward_teacher_forcing(_cuda(clean), _cuda(noisy), ref["t"].cuda(), _cuda(ctx))
    assert any(k[-1] == S and v.runs == 3 for k, v in m._tf_masks.items() if isinstance(k[0], int))
    for o, r in zip(out, ref["out"]):
        assert o.shape == (16, F, 14, 16) and o.dtype == torch.float32
        print(f"({fpc}, {W}, {S}): teacher forcing forward rel-RMS {rel_rms(o, r):.2e}")
        assert rel_rms(o, r) < TOL_FWD
    m.set_causal_chunks(fpc, W)                                                  # no sink: another matrix, another result
    plain = m.forward_teacher_forcing(_cuda(clean), _cuda(noisy), ref["t"].cuda(), _cuda(ctx))
    assert not torch.equal(plain[0], out[0])


@pytest.mark.parametrize("fpc,W,S,F", SETTINGS)
def test_forward_under_sink_and_window(model_mod, causal, fpc, W, S, F):
    """``forward`` with per-frame t under set_causal_chunks(.., sink) against the restatement under the dense
    sink_window_groups mask; S = 0 keeps the staircase kernels."""
    cfg, clean, _, _, ctx, t_frames = _inputs(F)
    sd = O.synth_state_dict(cfg, MC.TAG)
    with torch.no_grad():
        ref = R.forward(sd, cfg, clean, t_frames, ctx, F * TPF, mask=_sink_mask(causal, fpc, W, S, F))
    m = _model(model_mod)
    m.set_causal_chunks(fpc, W, S)
    out = m(_cuda(clean), t_frames.cuda(), _cuda(ctx), F * TPF)
    for o, r in zip(out, ref):
        print(f"({fpc}, {W}, {S}): forward under sink + window rel-RMS {rel_rms(o, r):.2e}")
        assert rel_rms(o, r) < TOL_FWD
    pair = m.forward_cfg_pair(_cuda(clean), t_frames[:, 0].contiguous().cuda(), _cuda(ctx), _cuda(ctx), F * TPF)
    one = m(_cuda(clean), t_frames[:, 0].contiguous().cuda(), _cuda(ctx), F * TPF)
    assert rel_rms(pair[0][0], one[0]) < 1e-3
    m.set_causal_chunks(fpc, W, 0)
    stairs = m(_cuda(clean), t_frames.cuda(), _cuda(ctx), F * TPF)
    m.set_causal_chunks(fpc, W)
    assert torch.equal(stairs[0], m(_cuda(clean), t_frames.cuda(), _cuda(ctx), F * TPF)[0])
    assert not torch.equal(stairs[0], out[0])


def _tf_step(model_mod, setting, t, policy=None, keep=False):
    fpc, W, S, F = setting
    cfg, clean, noisy, target, ctx, _ = _inputs(F)
    m = _model(model_mod, train=True)
    if policy is not None:
        m.checkpoint_policy = policy
    m.use_checkpoint = not keep
    m.set_causal_chunks(fpc, W, S)
    xc, xn = [u.cuda().requires_grad_(True) for u in clean], [u.cuda().requires_grad_(True) for u in noisy]
    tg = t.cuda().requires_grad_(True)
    out = m.forward_teacher_forcing(xc, xn, tg, _cuda(ctx))
    loss = sum(torch.nn.functional.mse_loss(o, v.cuda()) for o, v in zip(out, target))
    loss.backward()
    return m, loss, xc, xn, tg


def test_teacher_forcing_training_with_a_sink(model_mod, causal):
    """Loss, parameter gradients and x_noisy / x_clean / t gradients against autograd through the restatement; the
    checkpoint re-run and kept activations give the same bits under ops.set_deterministic(True)."""
    ops = importlib.import_module(PKG + ".ops")
    was = ops.set_deterministic(None)
    ops.set_deterministic(True)
    try:
        setting = SETTINGS[1]
        ref = _ref_tf(causal, *setting, grad=True)
        m, loss, xc, xn, tg = _tf_step(model_mod, setting, ref["t"])
        print(f"loss {loss.item():.6f} reference {ref['loss']:.6f}")
        assert abs(loss.item() - ref["loss"]) < TOL_LOSS * ref["loss"]
        params = dict(m.named_parameters())
        for name in GRAD_NAMES:
            err = rel_rms(params[name].grad, ref["grads"][name])
            print(f"{name}: rel-RMS {err:.2e}")
            assert err < TOL_GRAD, name
        print(f"t {rel_rms(tg.grad, ref['d_t']):.2e} noisy {rel_rms(xn[0].grad, ref['d_noisy'][0]):.2e} "
              f"clean {rel_rms(xc[0].grad, ref['d_clean'][0]):.2e}")
        assert tg.grad.shape == ref["d_t"].shape and rel_rms(tg.grad, ref["d_t"]) < TOL_GRAD
        for b in range(2):
            assert rel_rms(xn[b].grad, ref["d_noisy"][b]) < TOL_GRAD and rel_rms(xc[b].grad, ref["d_clean"][b]) < TOL_GRAD
        for policy, keep in (("always", False), (None, True)):
            other, loss2, xc2, xn2, tg2 = _tf_step(model_mod, setting, ref["t"], policy, keep)
            op = dict(other.named_parameters())
            assert torch.equal(loss2, loss) and torch.equal(tg2.grad, tg.grad) and torch.equal(xn2[0].grad, xn[0].grad)
            assert torch.equal(xc2[1].grad, xc[1].grad)
            for name in GRAD_NAMES:
                assert torch.equal(op[name].grad, params[name].grad), (policy, keep, name)
    finally:
        ops.set_deterministic(was)


def _rollout(m, causal, cache, clean, noisy, ctx, t, fpc, F):
    """forward_chunk of every noisy chunk (commit=False) at t[:, I], the cache committed from the clean chunks at 0."""
    zero = torch.zeros(2, device="cuda")
    out = []
    for I in range(F // fpc):
        sl = slice(I * fpc, (I + 1) * fpc)
        out.append(m.forward_chunk([u[:, sl].cuda() for u in noisy], t[:, I].contiguous(), _cuda(ctx), cache, commit=False))
        m.forward_chunk([u[:, sl].cuda() for u in clean], zero, _cuda(ctx), cache, commit=True)
    return out


@pytest.mark.parametrize("fpc,W,S,F", SETTINGS)
def test_teacher_forcing_is_the_rolling_rollout(model_mod, causal, fpc, W, S, F):
    cfg, clean, noisy, _, ctx, t_frames = _inputs(F)
    t = t_frames[:, ::fpc].cuda()
    m = _model(model_mod)
    m.set_causal_chunks(fpc, W, S)
    full = m.forward_teacher_forcing(_cuda(clean), _cuda(noisy), t, _cuda(ctx), context_t=0.0)
    cache = causal.RollingKVCache(m, 2, fpc * TPF, S, W, "cuda")
    assert F // fpc > cache.slots                                                # the ring wraps inside the clip
    got = _rollout(m, causal, cache, clean, noisy, ctx, t, fpc, F)
    assert cache.length == F * TPF and cache.k[0].shape[1] == (S + W + 1) * fpc * TPF
    for I, chunk in enumerate(got):
        for b in range(2):
            err = rel_rms(chunk[b], full[b][:, I * fpc:(I + 1) * fpc])
            print(f"({fpc}, {W}, {S}) chunk {I} clip {b}: rolling rollout against teacher forcing rel-RMS {err:.2e}")
            assert err < TOL_ROLLOUT


def test_eviction_is_real(model_mod, causal):
    """With 2 layers, chunk I depends on the clean chunks within two hops of sink + window; clean chunk 1 is outside
    that for I = 4, 5 under (1, 1, 1): changing it leaves their outputs unchanged bit for bit, in teacher forcing and in
    the rollout — and does change chunk 2, which sees it."""
    fpc, W, S, F = SETTINGS[0]
    cfg, clean, noisy, _, ctx, t_frames = _inputs(F)
    t = t_frames.cuda()
    m = _model(model_mod)
    m.set_causal_chunks(fpc, W, S)
    other = [u.clone() for u in clean]
    for u in other:
        u[:, 1] += 1.0
    a = m.forward_teacher_forcing(_cuda(clean), _cuda(noisy), t, _cuda(ctx))
    b = m.forward_teacher_forcing(_cuda(other), _cuda(noisy), t, _cuda(ctx))
    for u, v in zip(a, b):
        assert torch.equal(u[:, 4:], v[:, 4:]) and torch.equal(u[:, :2], v[:, :2]) and not torch.equal(u[:, 2], v[:, 2])
    ra = _rollout(m, causal, causal.RollingKVCache(m, 2, TPF, S, W, "cuda"), clean, noisy, ctx, t, fpc, F)
    rb = _rollout(m, causal, causal.RollingKVCache(m, 2, TPF, S, W, "cuda"), other, noisy, ctx, t, fpc, F)
    for I in (0, 1, 4, 5):
        assert torch.equal(ra[I][0], rb[I][0]) and torch.equal(ra[I][1], rb[I][1])
    assert not torch.equal(ra[2][0], rb[2][0])


def test_rolling_cache_without_a_sink_is_the_window(model_mod, causal):
    """S = 0: the rolling cache against KVCache with left_chunks = W — equal bits before the ring wraps, <= 2e-3 after
    it (the keys arrive in another order)."""
    fpc, W, F = 1, 1, 6
    cfg, clean, noisy, _, ctx, t_frames = _inputs(F)
    t = t_frames.cuda()
    m = _model(model_mod)
    m.set_causal_chunks(fpc, W)
    ring = _rollout(m, causal, causal.RollingKVCache(m, 2, TPF, 0, W, "cuda"), clean, noisy, ctx, t, fpc, F)
    flat = _rollout(m, causal, causal.KVCache(m, 2, F * TPF, "cuda"), clean, noisy, ctx, t, fpc, F)
    for I in range(F):
        for b in range(2):
            if I <= W:
                assert torch.equal(ring[I][b], flat[I][b])
            else:
                print(f"chunk {I} clip {b}: ring against flat cache rel-RMS {rel_rms(ring[I][b], flat[I][b]):.2e}")
                assert rel_rms(ring[I][b], flat[I][b]) < TOL_ROLLOUT


@pytest.mark.parametrize("F", (7, 9))
def test_short_final_chunk_after_the_wrap(model_mod, causal, F):
    """fpc = 2, (W, S) = (1, 1): the last chunk has one frame and lands in a slot that still holds a stale frame behind
    it (F = 7: a middle slot, the interval kernel skips the stale keys; F = 9: the last slot, the key range ends
    before them).  forward_chunk against the last frame of ``forward`` over the whole clip, per-frame t."""
    fpc, W, S = 2, 1, 1
    cfg, clean, _, _, ctx, _ = _inputs(F)
    t_last = torch.tensor([700., 300.])
    t_frames = torch.cat([torch.zeros(2, F - 1), t_last[:, None]], 1)
    m = _model(model_mod)
    m.set_causal_chunks(fpc, W, S)
    full = m(_cuda(clean), t_frames.cuda(), _cuda(ctx), F * TPF)
    cache = causal.RollingKVCache(m, 2, fpc * TPF, S, W, "cuda")
    zero = torch.zeros(2, device="cuda")
    for f0 in range(0, F - 1, fpc):
        m.forward_chunk([u[:, f0:f0 + fpc].cuda() for u in clean], zero, _cuda(ctx), cache)
    assert cache.length // (fpc * TPF) >= cache.slots
    got = m.forward_chunk([u[:, F - 1:].cuda() for u in clean], t_last.cuda(), _cuda(ctx), cache, commit=False)
    for b in range(2):
        err = rel_rms(got[b], full[b][:, F - 1:])
        print(f"F = {F} clip {b}: short last chunk against the full forward rel-RMS {err:.2e}")
        assert err < TOL_ROLLOUT
    again = m.forward_chunk([u[:, F - 1:].cuda() for u in clean], t_last.cuda(), _cuda(ctx), cache, commit=False)
    assert torch.equal(again[0], got[0])


def test_sample_on_rolling_caches(model_mod, causal):
    unipc = importlib.import_module(PKG + ".wan.utils.fm_solvers_unipc")
    cfg, _, ctx, _, _ = MC.case()
    m = _model(model_mod)
    ctx = _cuda(ctx)
    noise = torch.randn(16, 5, 14, 16, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    cond, null = ctx[:1], [ctx[0][:5]]

    def make_scheduler():
        s = unipc.FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
        s.set_timesteps(2, device="cuda", shift=3.0)
        return s

    kw = dict(frames_per_chunk=1, left_chunks=1, make_scheduler=make_scheduler, guide_scale=5.0)
    a = causal.sample(m, noise, cond, null, sink_chunks=1, rolling=True, **kw)
    assert a.shape == (16, 5, 14, 16) and torch.isfinite(a).all() and m._causal_chunks is None
    caches = tuple(causal.RollingKVCache(m, 1, TPF, 1, 1, "cuda") for _ in range(2))
    b = causal.sample(m, noise, cond, null, sink_chunks=1, caches=caches, **kw)       # a sink alone implies the rolling caches
    assert torch.equal(a, b)
    for c in caches:                                                             # (S + W + 1) C rows, whatever the clip's length
        assert c.k[0].shape[1] == 3 * TPF and c.length == 4 * TPF
    plain = causal.sample(m, noise, cond, null, **kw)
    assert torch.equal(plain[:, :2], a[:, :2]) and not torch.equal(plain[:, 3:], a[:, 3:])
    ring = causal.sample(m, noise, cond, null, rolling=True, **kw)                   # S = 0 on a ring: the window's result
    assert rel_rms(ring, plain) < 5e-2


def test_refusals(model_mod, causal):
    cfg, clean, noisy, _, ctx, t_frames = _inputs(6)
    m = _model(model_mod)
    x, c = [u[:, :1].cuda() for u in clean], _cuda(ctx)
    t = torch.zeros(2, device="cuda")
    m.set_causal_chunks(1, 1, 1)
    with pytest.raises(ValueError, match="RollingKVCache"):                      # a plain cache cannot keep a sink
        m.forward_chunk(x, t, c, causal.KVCache(m, 2, 6 * TPF, "cuda"))
    for geometry in ((2 * TPF, 1, 1), (TPF, 2, 1), (TPF, 1, 0)):                 # the cache's (C, S, W) against (56, 1, 1)
        with pytest.raises(ValueError):
            m.forward_chunk(x, t, c, causal.RollingKVCache(m, 2, *geometry, "cuda"))
    with pytest.raises(ValueError):                                              # another batch size
        m.forward_chunk(x, t, c, causal.RollingKVCache(m, 1, TPF, 1, 1, "cuda"))
    m.set_causal_chunks(None)
    with pytest.raises(ValueError):                                              # no causal chunks set
        m.forward_chunk(x, t, c, causal.RollingKVCache(m, 2, TPF, 1, 1, "cuda"))
    with pytest.raises(ValueError):
        causal.sample(m, torch.zeros(16, 4, 14, 16, device="cuda"), c[:1], c[:1], frames_per_chunk=1, left_chunks=-1,
                      make_scheduler=None, guide_scale=1.0, rolling=True)
