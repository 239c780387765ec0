"""ops.attn_mask / ops.AttnMask: the one resolver of an attention call's key restriction (no GPU needed)."""
import importlib
import inspect
import itertools

import pytest
import torch

from conftest import PKG

H, L = 2, 256
CPU = torch.device("cpu")
NAMES = ("window", "block_mask", "chunk_causal", "interval_mask")
KINDS = {(0, 0, 0, 0): "full", (1, 0, 0, 0): "band", (0, 1, 0, 0): "block", (0, 0, 1, 0): "chunk", (0, 0, 0, 1): "interval"}


@pytest.fixture(scope="module")
def things(omh):
    sparse, causal = importlib.import_module(PKG + ".sparse"), importlib.import_module(PKG + ".causal")
    return dict(window=(16, 16), block_mask=sparse.BlockMask(torch.ones(2, 2, dtype=torch.bool), L, L), chunk_causal=(64, -1, 0),
                interval_mask=causal.IntervalMask(causal.teacher_forcing_groups(2), 64))


def _keywords(things, present):
    return {n: things[n] if p else ((-1, -1) if n == "window" else None) for n, p in zip(NAMES, present)}


@pytest.mark.parametrize("present", list(itertools.product((0, 1), repeat=4)), ids=lambda p: "".join(map(str, p)))
def test_sixteen_combinations(ops, things, present):
    """At most one of the four resolves, to its kind; any two together are a ValueError (the table of the three helpers
    this replaced, run in flash_attn_raw's order: interval mask, chunk rule, block mask)."""
    kw = _keywords(things, present)
    if sum(present) > 1:
        with pytest.raises(ValueError):
            ops.attn_mask(**kw, H=H, Lq=L, Lk=L, device=CPU)
        return
    m = ops.attn_mask(**kw, H=H, Lq=L, Lk=L, device=CPU)
    assert isinstance(m, ops.AttnMask) and m.kind == KINDS[present]
    assert m.window == ((16, 16) if m.kind == "band" else (-1, -1))
    if m.kind in ("full", "band"):
        assert m.rule is None
    elif m.kind == "chunk":
        r = m.rule
        assert (r.chunk, r.left_chunks, r.q_offset, r.reserved) == (64, -1, 0, 0) and m.c_struct() is r
    else:
        assert m.rule is things["block_mask" if m.kind == "block" else "interval_mask"]      # on that device already
        assert type(m.c_struct()).__name__ == ("BlockMaskArgs" if m.kind == "block" else "IntervalMaskArgs")


def test_entries(ops, omh):
    causal, binding = importlib.import_module(PKG + ".causal"), importlib.import_module(PKG + "._lib")
    vis = causal.teacher_forcing_groups(2)
    names = []
    for runs in (2, 3):
        m = ops.attn_mask(interval_mask=causal.IntervalMask(vis, 64, runs=runs), H=H, Lq=L, Lk=L, device=CPU)
        names += ops._MASK_ENTRIES[m.kind, m.rule.runs]
    assert names == ["omh_flash_attn_fwd_interval_d128", "omh_flash_attn_bwd_interval_d128",
                     "omh_flash_attn_fwd_interval3_d128", "omh_flash_attn_bwd_interval3_d128"]
    assert ops._MASK_ENTRIES["block", 0] == ("omh_flash_attn_fwd_sparse_d128", "omh_flash_attn_bwd_sparse_d128")
    assert ops._MASK_ENTRIES["chunk", 0] == ("omh_flash_attn_fwd_chunk_d128", "omh_flash_attn_bwd_chunk_d128")
    for pair in ops._MASK_ENTRIES.values():
        assert all(n in binding.EXPORTED and hasattr(binding.lib, n) for n in pair)


@pytest.mark.parametrize("extra", NAMES)
def test_mask_excludes_the_keywords(ops, things, extra):
    """A resolved mask beside any of the four keywords it stands for: ValueError, before an operand is looked at.
    (``flash_attn`` looks at its operands' device first: tests/test_gpu_attn_mask_value.py.)"""
    kw = {extra: things[extra]}
    for m in (ops.attn_mask(H=H, Lq=L, Lk=L, device=CPU), ops.attn_mask(things["window"], H=H, Lq=L, Lk=L, device=CPU)):
        with pytest.raises(ValueError):
            ops.flash_attn_raw(None, None, None, None, None, 1, H, L, L, 0, 0, 0, 0, 0, 0, 0, L, 1.0, mask=m, **kw)
        with pytest.raises(ValueError):
            ops.flash_attn_bwd(None, None, None, None, None, None, None, 1, H, L, L, mask=m, **kw)
        q = torch.zeros(1, L, H, 128, dtype=torch.bfloat16)
        with pytest.raises(ValueError):
            ops.flash_attn_func(q, q, q, mask=m, **kw)


def test_signatures(ops, omh):
    attn = importlib.import_module(PKG + ".wan.modules.attention")
    for fn in (ops.flash_attn_raw, ops.flash_attn, ops.flash_attn_bwd, ops.flash_attn_func):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "mask" and p["mask"].default is None
        assert all(n in p for n in NAMES)
    for fn in (attn.flash_attention, attn.attention):
        assert list(inspect.signature(fn).parameters)[-1] == "block_mask"
