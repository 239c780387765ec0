"""WanModel.set_attention_block_policy: self-attention layers that choose their own block mask from q and k on the device,
on the tiny two-layer t2v case of tests/make_golden_window.py (two clips of 288 and 120 tokens padded to seq_len 320: nb = 3).

Everything here is a bit-for-bit comparison: a forward (or training step) under the policy against the same forward under
the masks it built, handed back in as static masks through ``set_attention_block_mask``.  What the masked kernels compute
is held to the reference by tests/test_gpu_attn_block_sparse_model.py; which blocks the rule picks, by
tests/test_gpu_block_select.py."""
import importlib

import pytest
import torch

import make_golden_window as MW
from conftest import PKG

pytestmark = pytest.mark.gpu
SEQ_LEN = 320
NB = 3
MASS = 0.4        # (at 0.5 both layers of this case keep key blocks {0, 1} for every row: the masks must differ, so lower)


@pytest.fixture(scope="module")
def model_mod():
    return importlib.import_module(PKG + ".wan.modules.model")


@pytest.fixture(scope="module")
def sparse():
    return importlib.import_module(PKG + ".sparse")


def _model(model_mod, train=False):
    from oracle import wan_dit_oracle as O
    cfg, xs, ctx, t, targets = MW.case()
    m = model_mod.WanModel(num_layers=2, **MW.make_golden.TINY)
    m.load_state_dict(O.synth_state_dict(cfg, MW.TAG))
    m = m.cuda()
    m = m.train() if train else m.eval().requires_grad_(False)
    return m, [u.cuda() for u in xs], [c.cuda() for c in ctx], t.cuda(), [v.cuda() for v in targets]


def _built(m):
    return [blk.self_attn.last_block_mask for blk in m.blocks]


def _set_static(m, masks):
    m.set_attention_block_policy(None)
    for i, bm in enumerate(masks):
        m.set_attention_block_mask(bm.mask.clone(), layers=[i])


def test_policy_inference_equals_its_own_static_masks(model_mod, sparse):
    m, xs, ctx, t, _ = _model(model_mod)
    plain = m(xs, t, ctx, SEQ_LEN)
    assert all(bm is None for bm in _built(m))
    m.set_attention_block_policy(sparse.DynamicBlockPolicy(MASS))
    out = m(xs, t, ctx, SEQ_LEN)
    masks = _built(m)
    for bm in masks:
        assert isinstance(bm, sparse.BlockMask) and (bm.heads, bm.q_blocks, bm.k_blocks) == (2, NB, NB)
        assert bm.mask.is_cuda and bool(bm.mask[:, torch.arange(NB), torch.arange(NB)].all())      # keep_diagonal
        print(bm.mask.int().tolist(), f"density {bm.density:.3f}")
    # the layers choose for themselves, and something is dropped
    assert not torch.equal(masks[0].mask, masks[1].mask)
    assert not all(bool(bm.mask.all()) for bm in masks)
    assert not torch.equal(out[0], plain[0])
    # the CFG pair builds block 0's shared mask once: the bits of two forwards
    null = [c[:5] for c in ctx]
    cond, uncond = m.forward_cfg_pair(xs, t, ctx, null, SEQ_LEN)
    for a, b in zip(cond, out):
        assert torch.equal(a, b)
    for a, b in zip(uncond, m(xs, t, null, SEQ_LEN)):
        assert torch.equal(a, b)
    # the same masks handed in: the same bits
    _set_static(m, masks)
    assert all(blk.self_attn._block_policy is None for blk in m.blocks)
    for a, b in zip(m(xs, t, ctx, SEQ_LEN), out):
        assert torch.equal(a, b)
    # clearing both restores the unmasked bits
    m.set_attention_block_mask(None)
    for a, b in zip(m(xs, t, ctx, SEQ_LEN), plain):
        assert torch.equal(a, b)
    # mass = 1 keeps every live block: here every block, the bits of the all-true static mask
    m.set_attention_block_policy(sparse.DynamicBlockPolicy(1.0))
    full = m(xs, t, ctx, SEQ_LEN)
    assert all(bool(bm.mask.all()) for bm in _built(m))
    m.set_attention_block_policy(None)
    m.set_attention_block_mask(torch.ones(NB, NB, dtype=torch.bool))
    for a, b in zip(m(xs, t, ctx, SEQ_LEN), full):
        assert torch.equal(a, b)


def test_policy_on_one_layer_and_misuse(model_mod, sparse):
    m, xs, ctx, t, _ = _model(model_mod)
    pol = sparse.DynamicBlockPolicy(MASS)
    m.set_attention_block_policy(pol, layers=[1])
    m(xs, t, ctx, SEQ_LEN)
    assert m.blocks[0].self_attn.last_block_mask is None and m.blocks[1].self_attn.last_block_mask is not None
    with pytest.raises(ValueError):                                              # a mask on a layer that has a policy
        m.set_attention_block_mask(torch.ones(NB, NB, dtype=torch.bool), layers=[1])
    m.set_attention_block_mask(torch.ones(NB, NB, dtype=torch.bool), layers=[0])
    with pytest.raises(ValueError):                                              # a policy on a layer that has a mask
        m.set_attention_block_policy(pol)
    with pytest.raises(ValueError):
        model_mod.WanModel(num_layers=2, window_size=(70, 30), **MW.make_golden.TINY).set_attention_block_policy(pol)
    # an always for another sequence length is refused where seq_len is known
    m.set_attention_block_mask(None)
    m.set_attention_block_policy(sparse.DynamicBlockPolicy(MASS, always=torch.ones(4, 4, dtype=torch.bool)))
    with pytest.raises(ValueError):
        m(xs, t, ctx, SEQ_LEN)


def test_policy_forward_does_not_synchronise(model_mod, sparse):
    m, xs, ctx, t, _ = _model(model_mod)
    m.set_attention_block_policy(sparse.DynamicBlockPolicy(MASS, always=torch.eye(NB, dtype=torch.bool)))
    first = m(xs, t, ctx, SEQ_LEN)                      # (the first call of a geometry uploads its small tables)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = m(xs, t, ctx, SEQ_LEN)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    for a, b in zip(out, first):
        assert torch.equal(a, b)


@pytest.mark.parametrize("keep", [False, True], ids=["checkpoint", "kept"])
def test_policy_training_equals_its_own_static_masks(model_mod, sparse, keep):
    """The mask a block's forward built is the one its backward (and the checkpoint re-run) uses: the loss and every
    parameter gradient equal, bit for bit, the run with those masks set statically."""
    ops = importlib.import_module(PKG + ".ops")
    ops.set_deterministic(True)         # column sums in a fixed order (the default adds partial sums with float atomics)

    def step(setup):
        m, xs, ctx, t, targets = _model(model_mod, train=True)
        setup(m)
        if not keep:
            m.checkpoint_policy = "always"
        m.use_checkpoint = not keep
        out = m(xs, t, ctx, SEQ_LEN)
        masks = _built(m)
        loss = sum(torch.nn.functional.mse_loss(o, v) for o, v in zip(out, targets))
        loss.backward()
        assert m._kept_activations is keep
        return loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}, masks

    loss, grads, masks = step(lambda m: m.set_attention_block_policy(sparse.DynamicBlockPolicy(MASS)))
    assert all(bm is not None for bm in masks) and not all(bool(bm.mask.all()) for bm in masks)
    loss_s, grads_s, _ = step(lambda m: _set_static(m, masks))
    assert torch.equal(loss, loss_s) and sorted(grads) == sorted(grads_s) and len(grads) > 20
    for n in grads:
        assert torch.equal(grads[n], grads_s[n]), n


def test_policy_training_refuses_v1_backward(model_mod, sparse, monkeypatch):
    mt = importlib.import_module(PKG + ".wan.modules.model_train")
    monkeypatch.setattr(mt, "_ATTN_BWD2", False)
    m, xs, ctx, t, _ = _model(model_mod, train=True)
    m.set_attention_block_policy(sparse.DynamicBlockPolicy(MASS))
    with pytest.raises(NotImplementedError):
        m(xs, t, ctx, SEQ_LEN)
