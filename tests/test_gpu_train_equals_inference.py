"""The training forward of ``WanModel`` is its inference forward, bit for bit — pinned where
test_gpu_train.py::test_training_forward_equals_inference_and_checkpoint_equals_kept_activations (t2v, seq_len 24) does
not reach: the i2v branch, ``cross_attn_norm`` on and off, the chunk-causal staircase, teacher forcing, frame-aligned
condition tokens, a static block mask and a block policy.  (``forward_chunk(grad=True)`` against ``forward_chunk`` is
asserted bit for bit by test_gpu_self_forcing_model.py.)

Each case is one tiny two-layer model, frozen, run once under ``no_grad`` (the inference block) and twice with one input
requiring grad (the training node: activations kept, then ``checkpoint_policy = "always"``), so both sides read the same
weights; the backward is run once per mode so that the re-run of the blocks happens too."""
import dataclasses
import importlib

import pytest
import torch

import condition_window_ref as CR
import make_golden_chunk_causal as MC
from conftest import PKG
from oracle import make_golden, wan_dit_oracle as O

pytestmark = pytest.mark.gpu
TPF = MC.TOKENS_PER_FRAME


@pytest.fixture(scope="module")
def model_mod():
    return importlib.import_module(PKG + ".wan.modules.model")


def _cuda(v):
    return [u.cuda() for u in v]


def _frozen(model_mod, cfg, tag, **kw):
    m = model_mod.WanModel(num_layers=2, **make_golden.TINY, **kw)
    m.load_state_dict(O.synth_state_dict(cfg, tag))
    return m.cuda().eval().requires_grad_(False)


def _tiny(model_mod, model_type, **kw):
    """The tiny golden case (clips of 24 and 6 tokens) -> (model, call(x))."""
    cfg, tag, xs, ctx, t, _, ys, clip = make_golden.tiny_case(model_type, 2)
    cfg = dataclasses.replace(cfg, cross_attn_norm=kw.get("cross_attn_norm", True))
    m = _frozen(model_mod, cfg, tag, model_type=model_type, in_dim=cfg.in_dim, **kw)
    ctx, t = _cuda(ctx), t.cuda()
    extra = dict(clip_fea=clip.cuda(), y=_cuda(ys)) if model_type == "i2v" else {}
    return m, _cuda(xs), lambda x: m(x, t, ctx, 24, **extra)


def _causal_case(model_mod, prepare):
    """The chunk-causal tests' case (clips of 5 and 3 frames of 56 tokens, seq_len 5 * TPF: three 128-blocks)."""
    cfg, xs, ctx, t, _ = MC.case()
    m = _frozen(model_mod, cfg, MC.TAG)
    prepare(m)
    ctx, t = _cuda(ctx), t.cuda()
    return m, _cuda(xs), lambda x: m(x, t, ctx, 5 * TPF)


def _block_mask(m):
    mask = torch.ones(2, 3, 3, dtype=torch.bool)
    mask[:, 2, 0] = False
    mask[1, 0, 1] = False
    m.set_attention_block_mask(mask)


def _block_policy(m):
    sparse = importlib.import_module(PKG + ".sparse")
    m.set_attention_block_policy(sparse.DynamicBlockPolicy(0.4))


def _teacher_forcing(model_mod):
    cfg, clean, noisy, _, ctx, t_frames, _, _ = CR.case()
    m = _frozen(model_mod, cfg, MC.TAG)
    m.set_causal_chunks(2, 1)
    clean, ctx, t = _cuda(clean), _cuda(ctx), t_frames[:, ::2].contiguous().cuda()
    return m, _cuda(noisy), lambda x: m.forward_teacher_forcing(clean, x, t, ctx)


def _condition_window(model_mod):
    cfg, clean, _, _, ctx, _, tok, frames = CR.case()
    m = _frozen(model_mod, cfg, MC.TAG)
    ctx, t, ec = _cuda(ctx), torch.tensor([900., 300.]).cuda(), {"tokens": tok.cuda(), "frames": frames, "window": (1, 1)}
    return m, _cuda(clean), lambda x: m(x, t, ctx, CR.F_LATENT * TPF, extra_conditions=ec)


CASES = {
    "i2v": lambda mm: _tiny(mm, "i2v"),
    "cross_attn_norm": lambda mm: _tiny(mm, "t2v", cross_attn_norm=True),
    "no_cross_attn_norm": lambda mm: _tiny(mm, "t2v", cross_attn_norm=False),
    "i2v_no_cross_attn_norm": lambda mm: _tiny(mm, "i2v", cross_attn_norm=False),
    "causal_chunks": lambda mm: _causal_case(mm, lambda m: m.set_causal_chunks(1)),
    "teacher_forcing": _teacher_forcing,
    "condition_window": _condition_window,
    "block_mask": lambda mm: _causal_case(mm, _block_mask),
    "block_policy": lambda mm: _causal_case(mm, _block_policy),
}


@pytest.mark.parametrize("case", list(CASES))
def test_training_forward_equals_inference_forward(model_mod, case):
    m, xs, call = CASES[case](model_mod)
    with torch.no_grad():
        want = call(xs)
    for ck in (False, True):
        m.use_checkpoint, m.checkpoint_policy = ck, "always"       # True = re-run the blocks, whatever HBM is free
        x = [u.clone().requires_grad_(True) for u in xs]
        out = call(x)
        assert m.__dict__["_kept_activations"] is (not ck)
        assert all(o.requires_grad for o in out)
        for b, (o, w) in enumerate(zip(out, want)):
            assert torch.equal(o.detach(), w), f"{case}: training forward != inference forward (clip {b}, checkpoint={ck})"
        sum(o.square().mean() for o in out).backward()
        assert all(u.grad is not None and bool(torch.isfinite(u.grad).all()) for u in x)
