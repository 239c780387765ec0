"""WanModel under the chunk-causal staircase: ``set_causal_chunks`` in inference and training, the chunk-at-a-time
``forward_chunk`` against a ``causal.KVCache`` and the rollout loop ``causal.sample`` — against the reference's own
WanModel run with its self-attention under the same mask (tests/golden/dit_chunk_causal_t2v_L2.npz, made by
tests/make_golden_chunk_causal.py: tiny t2v, 2 layers, two clips of 5 and 3 latent frames, 56 tokens per frame, padded to
seq_len 320).  Bounds as in test_gpu_attn_window_model.py."""
import importlib
import os

import numpy as np
import pytest
import torch

import make_golden_chunk_causal as MC
from conftest import PKG, rel_rms

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dit_chunk_causal_t2v_L2.npz")
TOL_TINY = 8.0e-3       # the tiny goldens' forward bound (test_gpu_dit.py)
TOL_GRAD = 2e-2         # the training step's gradient bound (test_gpu_train.py)
SEQ_LEN, TPF = MC.SEQ_LEN, MC.TOKENS_PER_FRAME


@pytest.fixture(scope="module")
def model_mod():
    return importlib.import_module(PKG + ".wan.modules.model")


@pytest.fixture(scope="module")
def causal():
    return importlib.import_module(PKG + ".causal")


def _model(model_mod, train=False, **kw):
    from oracle import wan_dit_oracle as O
    cfg, xs, ctx, t, targets = MC.case()
    m = model_mod.WanModel(num_layers=2, **MC.make_golden.TINY, **kw)
    m.load_state_dict(O.synth_state_dict(cfg, MC.TAG))
    m = m.cuda()
    m = m.train() if train else m.eval().requires_grad_(False)
    return m, [u.cuda() for u in xs], [c.cuda() for c in ctx], t.cuda(), [v.cuda() for v in targets]


def test_forward_matches_reference_under_both_settings(model_mod):
    g = np.load(GOLD)
    m, xs, ctx, t, _ = _model(model_mod)
    for n, (fpc, left) in enumerate(MC.SETTINGS):
        m.set_causal_chunks(fpc, left)
        out = m(xs, t, ctx, SEQ_LEN)
        for b, o in enumerate(out):
            err = rel_rms(o, torch.from_numpy(g[f"s{n}_out{b}"]))
            print(f"setting {(fpc, left)} clip {b}: rel-RMS {err:.2e}")
            assert err < TOL_TINY
        # the CFG pair shares block 0's self-attention: the same mask, the same bits as two forwards
        cond, uncond = m.forward_cfg_pair(xs, t, ctx, [c[:5] for c in ctx], SEQ_LEN)
        for a, b in zip(cond, out):
            assert torch.equal(a, b)
        for a, b in zip(uncond, m(xs, t, [c[:5] for c in ctx], SEQ_LEN)):
            assert torch.equal(a, b)
    # None clears it.  (How far the mask moves this tiny model's output: the reference's own bidirectional forward is
    # 1.6e-2 from its masked one on either clip — two bounds apart.)
    m.set_causal_chunks(None)
    plain = m(xs, t, ctx, SEQ_LEN)
    print(f"bidirectional model against the masked golden: rel-RMS {rel_rms(plain[0], torch.from_numpy(g['s0_out0'])):.2e}")
    assert not torch.equal(plain[0], out[0])
    # one chunk that holds the whole clip is full attention
    m.set_causal_chunks(5)
    for a, b in zip(m(xs, t, ctx, SEQ_LEN), plain):
        assert rel_rms(a, b) < 1e-3


def _train_step(model_mod, policy=None, keep=False):
    m, xs, ctx, t, targets = _model(model_mod, train=True)
    if policy is not None:
        m.checkpoint_policy = policy
    m.use_checkpoint = not keep
    m.set_causal_chunks(*MC.SETTINGS[0])
    out = m(xs, t, ctx, SEQ_LEN)
    loss = sum(torch.nn.functional.mse_loss(o, v) for o, v in zip(out, targets))
    loss.backward()
    return m, out, loss


def test_training_gradients_match_reference_and_the_checkpoint_rerun(model_mod):
    g = np.load(GOLD)
    m, out, loss = _train_step(model_mod)
    for b, o in enumerate(out):
        assert rel_rms(o.detach(), torch.from_numpy(g[f"s0_out{b}"])) < TOL_TINY
    print(f"loss {loss.item():.6f} golden {float(g['loss']):.6f}")
    assert abs(loss.item() - float(g["loss"])) < 2e-2 * float(g["loss"])
    params = dict(m.named_parameters())
    for name in MC.GRAD_NAMES:
        ref = torch.from_numpy(g[name])
        got = params[name].grad
        got = got if got.dim() == 1 else got[:ref.shape[0]]
        err = rel_rms(got, ref)
        print(f"{name}: rel-RMS {err:.2e}")
        assert err < TOL_GRAD, name
    # the same gradients, bit for bit, when every block is re-run in the backward (under the same mask) and when the
    # activations are kept
    for policy, keep in (("always", False), (None, True)):
        other = dict(_train_step(model_mod, policy, keep)[0].named_parameters())
        for name in MC.GRAD_NAMES:
            assert torch.equal(other[name].grad, params[name].grad), (policy, keep, name)


def test_input_gradients_and_lora_run_under_the_mask(model_mod):
    """A frozen model whose latents require grad takes the training forward under the mask.  With chunks of one frame a
    loss on frame 0 of the output gives exactly zero gradient to the latents of every later frame (frame 0 sees none of
    them, and everything else in the model acts per token); the bidirectional model gives them one.  LoRA adapters run
    under the mask in inference and training."""
    m, xs, ctx, t, _ = _model(model_mod)
    m.set_causal_chunks(1)
    x0 = xs[0].clone().requires_grad_(True)
    out = m([x0], t[:1], ctx[:1], 5 * TPF)
    out[0][:, 0].square().sum().backward()
    assert torch.isfinite(x0.grad).all() and float(x0.grad[:, 0].abs().sum()) > 0.0
    assert float(x0.grad[:, 1:].abs().sum()) == 0.0                               # frame 0 sees no later frame
    m.set_causal_chunks(None)
    x1 = xs[0].clone().requires_grad_(True)
    m([x1], t[:1], ctx[:1], 5 * TPF)[0][:, 0].square().sum().backward()
    assert float(x1.grad[:, 1:].abs().sum()) > 0.0                                # ... which the bidirectional model does
    omh = importlib.import_module(PKG)
    m.set_causal_chunks(1)
    before = m(xs[:1], t[:1], ctx[:1], 5 * TPF)
    adapters = omh.add_lora(m, rank=4)
    with torch.no_grad():
        after = m(xs[:1], t[:1], ctx[:1], 5 * TPF)
    assert torch.equal(after[0], before[0])                                       # lora_B = 0: the adapters change nothing yet
    m(xs[:1], t[:1], ctx[:1], 5 * TPF)[0].square().mean().backward()              # ... and train under the mask
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in adapters)
    assert any(float(p.grad.abs().sum()) > 0.0 for p in adapters)


@pytest.mark.parametrize("setting", range(2))
def test_rollout_matches_reference(model_mod, causal, setting):
    """Clip 0 chunk by chunk with commit=True — five chunks of one frame; three chunks of two frames with left = 1, the
    last of one frame — against the golden of the full forward under the same mask: the check on the RoPE frame offset
    and on the look-back slice.  (Not bit for bit: the GEMMs run at other row counts.)"""
    g = np.load(GOLD)
    fpc, left = MC.SETTINGS[setting]
    m, xs, ctx, t, _ = _model(model_mod)
    m.set_causal_chunks(fpc, left)
    x = xs[0]
    cache = causal.KVCache(m, 1, 5 * TPF, "cuda")
    outs = []
    for f0 in range(0, 5, fpc):
        outs.append(m.forward_chunk([x[:, f0:f0 + fpc]], t[:1], ctx[:1], cache)[0])
        assert cache.length == min(f0 + fpc, 5) * TPF
    got = torch.cat(outs, dim=1)
    err = rel_rms(got, torch.from_numpy(g[f"s{setting}_out0"]))
    print(f"rollout {(fpc, left)}: rel-RMS {err:.2e}")
    assert err < TOL_TINY
    with pytest.raises(ValueError):                                              # the cache is full
        m.forward_chunk([x[:, :1]], t[:1], ctx[:1], cache)
    # The rollout against this model's own full forward under the mask: the same mathematics on other launches (GEMMs at
    # other row counts, key tiles that start at the look-back), so the project's figure for that applies — rel-RMS 2e-3
    # (test_gpu_attn_block_sparse.py, test_all_true_mask_is_full_attention).  Sharper than the golden on this tiny model;
    # printed beside it: what rotating chunk 1 as frame 0 would cost.
    full = m([x], t[:1], ctx[:1], 5 * TPF)[0]
    assert rel_rms(got, full) < 2e-3
    cache.reset()
    m.forward_chunk([x[:, :fpc]], t[:1], ctx[:1], cache)
    wrong = m.forward_chunk([x[:, fpc:2 * fpc]], t[:1], ctx[:1], cache, frame_offset=0, commit=False)[0]
    print(f"rollout against the full forward: rel-RMS {rel_rms(got, full):.2e}; chunk 1 rotated as frame 0: "
          f"{rel_rms(wrong, outs[1]):.2e}")


def test_chunk_zero_is_the_plain_model_and_commit_false_leaves_the_cache(model_mod, causal):
    m, xs, ctx, t, _ = _model(model_mod)
    x = xs[0][:, :2].contiguous()
    plain = m([x], t[:1], ctx[:1], 2 * TPF)[0]                                   # bidirectional, seq_len = its token count
    cache = causal.KVCache(m, 1, 5 * TPF, "cuda")
    a = m.forward_chunk([x], t[:1], ctx[:1], cache, commit=False)[0]
    assert torch.equal(a, plain) and cache.length == 0
    b = m.forward_chunk([x], t[:1], ctx[:1], cache, commit=False)[0]
    assert torch.equal(a, b) and cache.length == 0
    m.set_causal_chunks(2, 1)
    c = m.forward_chunk([x], t[:1], ctx[:1], cache)[0]
    assert torch.equal(c, plain) and cache.length == 2 * TPF
    # a denoising step of the next chunk: the same bits twice, the committed rows untouched
    k0 = [k.clone() for k in cache.k]
    y = xs[0][:, 2:4].contiguous()
    d1 = m.forward_chunk([y], t[:1], ctx[:1], cache, commit=False)[0]
    d2 = m.forward_chunk([y], t[:1], ctx[:1], cache, commit=False)[0]
    assert torch.equal(d1, d2) and cache.length == 2 * TPF
    for k, kk in zip(cache.k, k0):
        assert torch.equal(k[:, :2 * TPF], kk[:, :2 * TPF])
    cache.truncate(0)
    assert torch.equal(m.forward_chunk([x], t[:1], ctx[:1], cache, commit=False)[0], plain)


def test_sample_rollout(model_mod, causal):
    """causal.sample with a 4-step UniPC scheduler: what is produced for a chunk does not depend on how many chunks
    follow it, and chunk 0 is the plain CFG loop over a one-chunk clip, bit for bit."""
    unipc = importlib.import_module(PKG + ".wan.utils.fm_solvers_unipc")
    m, xs, ctx, t, _ = _model(model_mod)
    noise = torch.randn(16, 6, 14, 16, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    cond, null = ctx[:1], [ctx[0][:5]]

    def make_scheduler():
        s = unipc.FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
        s.set_timesteps(4, device="cuda", shift=3.0)
        return s

    kw = dict(frames_per_chunk=2, left_chunks=1, make_scheduler=make_scheduler, guide_scale=5.0)
    two = causal.sample(m, noise[:, :4], cond, null, **kw)
    three = causal.sample(m, noise, cond, null, **kw)
    assert two.shape == (16, 4, 14, 16) and three.shape == (16, 6, 14, 16) and torch.isfinite(three).all()
    assert torch.equal(three[:, :4], two)
    assert m._causal_chunks is None                                              # the model's own setting is restored
    sched = make_scheduler()
    lat = noise[:, :2].contiguous()
    for ts in sched.timesteps:
        tt = torch.stack([ts])
        c = m([lat], tt, cond, 2 * TPF)[0]
        u = m([lat], tt, null, 2 * TPF)[0]
        lat = sched.step_cfg(c, u, 5.0, lat)
    assert torch.equal(lat, two[:, :2])


def test_refusals(model_mod, causal, monkeypatch):
    sparse = importlib.import_module(PKG + ".sparse")
    m, xs, ctx, t, _ = _model(model_mod)
    m.set_causal_chunks(1)
    with pytest.raises(ValueError):                                              # clips that do not share h, w
        m([xs[0], xs[1][:, :, :12]], t, ctx, SEQ_LEN)
    m.set_attention_block_mask(torch.ones(3, 3, dtype=torch.bool))               # set behind the chunks: found at forward
    with pytest.raises(ValueError):
        m(xs, t, ctx, SEQ_LEN)
    m.set_attention_block_mask(None)
    m.set_attention_block_policy(sparse.DynamicBlockPolicy(0.9))
    with pytest.raises(ValueError):
        m(xs, t, ctx, SEQ_LEN)
    m.set_attention_block_policy(None)
    w, *_ = _model(model_mod, window_size=(70, 30))
    with pytest.raises(ValueError):
        w.set_causal_chunks(1)
    # forward_chunk: tokens per chunk a multiple of 8, one shape per batch, the cache of this model and batch, no grad
    cache = causal.KVCache(m, 1, 5 * TPF, "cuda")
    with pytest.raises(ValueError):
        m.forward_chunk([xs[0][:, :1, :10, :12]], t[:1], ctx[:1], cache)           # 5 x 6 = 30 tokens
    with pytest.raises(ValueError):
        m.forward_chunk([xs[0][:, :2]], t[:1], ctx[:1], cache)                   # 2 frames under chunks of 1
    with pytest.raises(ValueError):
        m.forward_chunk([xs[0][:, :1], xs[1][:, :1]], t, ctx, cache)             # a cache of batch 1
    with pytest.raises(ValueError):
        m.forward_chunk([xs[0][:, :1]], t[:1], ctx[:1], causal.KVCache(w, 1, 5 * TPF, "cuda"))
    with pytest.raises(RuntimeError):
        m.forward_chunk([xs[0][:, :1].clone().requires_grad_(True)], t[:1], ctx[:1], cache)
    assert cache.length == 0
    # the round-2 backward has no staircase: an error, not full-attention gradients
    mt = importlib.import_module(PKG + ".wan.modules.model_train")
    monkeypatch.setattr(mt, "_ATTN_BWD2", False)
    tr, *_ = _model(model_mod, train=True)
    tr.set_causal_chunks(1)
    with pytest.raises(NotImplementedError):
        tr(xs, t, ctx, SEQ_LEN)
