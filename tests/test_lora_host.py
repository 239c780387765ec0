"""CPU: the host side of the low-rank adapters (lora.py) — parameters, freezing, the adapter file format, argument
checks — and the C ABI declarations behind them (include/omh.h)."""
import importlib
import math
import os
import re

import pytest
import torch

from conftest import PKG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64, text_len=32, freq_dim=64)


@pytest.fixture(scope="module")
def lora(omh):
    return importlib.import_module(PKG + ".lora")


def _model(wan_model_mod, **kw):
    return wan_model_mod.WanModel(**dict(TINY, **kw))


def test_add_lora_parameters(wan_model_mod, lora, omh):
    m = _model(wan_model_mod)
    keys = list(m.state_dict())                               # importing the module touched nothing
    assert not any("lora" in k for k in keys)
    assert omh.add_lora is lora.add_lora and omh.DEFAULT_TARGETS == lora.DEFAULT_TARGETS
    params = lora.add_lora(m, 8, alpha=16)
    named = dict(m.named_parameters())
    assert len(params) == 2 * 2 * len(lora.DEFAULT_TARGETS)
    for i in range(2):
        for t in lora.DEFAULT_TARGETS:
            lin = m.blocks[i].get_submodule(t)
            A, B = named[f"blocks.{i}.{t}.lora_A"], named[f"blocks.{i}.{t}.lora_B"]
            assert A is lin.lora_A and B is lin.lora_B and any(A is p for p in params) and any(B is p for p in params)
            assert A.shape == (8, lin.in_features) and B.shape == (lin.out_features, 8)
            assert A.dtype == B.dtype == torch.float32 and A.requires_grad and B.requires_grad
            assert not B.any()
            bound = 1.0 / math.sqrt(lin.in_features)           # kaiming-uniform, a = sqrt(5): U(-1/sqrt(in), 1/sqrt(in))
            assert float(A.detach().abs().max()) <= bound and float(A.detach().std()) > 0.4 * bound
            assert wan_model_mod.lora_of(lin)[2] == 2.0        # alpha / rank
    assert all(p.requires_grad == ("lora_" in n) for n, p in m.named_parameters())      # freeze_base
    lora.remove_lora(m)
    assert list(m.state_dict()) == keys
    m2 = _model(wan_model_mod)
    lora.add_lora(m2, 4, targets=("self_attn.q", "self_attn.v"), freeze_base=False)
    assert all(p.requires_grad for p in m2.parameters())
    assert sorted(n for n, _ in m2.blocks[0].named_parameters() if "lora_" in n) == \
        ["self_attn.q.lora_A", "self_attn.q.lora_B", "self_attn.v.lora_A", "self_attn.v.lora_B"]
    assert wan_model_mod.lora_of(m2.blocks[0].self_attn.q)[2] == 1.0      # alpha defaults to rank
    lora.set_lora_scale(m2, 0.25)
    assert wan_model_mod.lora_of(m2.blocks[1].self_attn.v)[2] == 0.25
    lora.set_lora_scale(m2, None)
    assert wan_model_mod.lora_of(m2.blocks[1].self_attn.v)[2] == 1.0
    # i2v: the image-token projections join the default targets
    m3 = _model(wan_model_mod, model_type="i2v", in_dim=36)
    lora.add_lora(m3, 2)
    assert hasattr(m3.blocks[0].cross_attn.k_img, "lora_A") and hasattr(m3.blocks[1].cross_attn.v_img, "lora_B")


def test_adapter_file_round_trip(wan_model_mod, lora):
    m = _model(wan_model_mod)
    lora.add_lora(m, 8, alpha=4, targets=("self_attn.q", "ffn.2"))
    with torch.no_grad():
        for _, lin in lora.lora_modules(m):
            lin.lora_B.normal_()
    sd = lora.lora_state_dict(m)
    assert sorted(sd) == sorted(f"blocks.{i}.{t}.{k}" for i in range(2) for t in ("self_attn.q", "ffn.2")
                                for k in ("lora_A.weight", "lora_B.weight", "alpha"))
    assert float(sd["blocks.1.ffn.2.alpha"]) == 4.0 and sd["blocks.1.ffn.2.lora_B.weight"].shape == (256, 8)
    bare = _model(wan_model_mod)                              # onto a bare model: rank and targets from the file
    assert lora.load_lora_state_dict(bare, {"diffusion_model." + k: v for k, v in sd.items()}) == ([], [])
    assert [n for n, _ in lora.lora_modules(bare)] == [n for n, _ in lora.lora_modules(m)]
    for (_, a), (_, b) in zip(lora.lora_modules(bare), lora.lora_modules(m)):
        assert torch.equal(a.lora_A, b.lora_A) and torch.equal(a.lora_B, b.lora_B) and a.lora_alpha == b.lora_alpha == 4.0
    other = _model(wan_model_mod)                             # onto a model that has them: values replaced
    lora.add_lora(other, 8, targets=("self_attn.q", "ffn.2"))
    lora.load_lora_state_dict(other, sd)
    assert torch.equal(other.blocks[1].ffn[2].lora_B, m.blocks[1].ffn[2].lora_B) and other.blocks[0].ffn[2].lora_alpha == 4.0
    with pytest.raises(RuntimeError, match="unexpected"):
        lora.load_lora_state_dict(other, dict(sd, **{"blocks.0.head.lora_A.weight": torch.zeros(1)}))
    partial = {k: v for k, v in sd.items() if k.startswith("blocks.0.")}
    with pytest.raises(RuntimeError, match="missing"):
        lora.load_lora_state_dict(other, partial)
    assert lora.load_lora_state_dict(other, partial, strict=False)[0] == ["blocks.1.self_attn.q", "blocks.1.ffn.2"]


@pytest.mark.parametrize("kwargs,exc,word", [
    (dict(rank=0), ValueError, "rank"), (dict(rank=129), ValueError, "rank"),
    (dict(rank=4, lora_dropout=0.1), NotImplementedError, "lora_dropout"),
    (dict(rank=4, targets=("self_attn.q", "head.head")), ValueError, "targets")])
def test_add_lora_rejects(wan_model_mod, lora, kwargs, exc, word):
    m = _model(wan_model_mod)
    with pytest.raises(exc, match=word):
        lora.add_lora(m, **kwargs)
    assert not lora.lora_modules(m) and not any("lora" in k for k in m.state_dict())


def test_header_declares_the_adapter_entry_points(omh):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "omh.h")).read(), flags=re.S)
    for name in ("omh_pack_weights_lora_multi", "omh_lora_merge", "omh_lora_grads", "omh_lora_grads_workspace_bytes"):
        assert re.search(rf"\b{name}\s*\(", src), name
        assert hasattr(omh._lib.lib, name)
    assert re.search(r"^#define\s+OMH_ABI_VERSION\s+12\s*$", src, flags=re.M)
    lib, binding = omh._lib.lib, omh._lib
    assert lib.omh_pack_weights_lora_multi(None, 1, 1, None) == -1 and lib.omh_lora_merge(None, 1, 1, None) == -1
    assert lib.omh_lora_grads(None, None) == -1
    a = binding.LoraGradArgs(M=64, in_features=128, out_features=128, rank=129, ldx=128, lddy=128)
    assert lib.omh_lora_grads_workspace_bytes(a) == 0         # rank > 128
    a.rank, a.in_features = 32, 100
    assert lib.omh_lora_grads_workspace_bytes(a) == 0         # in % 8 != 0
    a.in_features = 128
    assert lib.omh_lora_grads_workspace_bytes(a) > 2 * 64 * 32 * 2
