"""Low-rank adapters (LoRA, Hu et al. 2021) for WanModel: inference, training and merge on the gfx950 kernels.

An adapted Linear computes with the EFFECTIVE weight ``W + s * B @ A`` (``lora_A`` [rank, in], ``lora_B`` [out, rank],
``s = alpha / rank``).  The hot path never reads the fp32 master weights, only bf16 operand copies that are rebuilt
when a parameter changes; with an adapter the copy is ``bf16(W + s B A)`` (csrc/lora.hip), so every fused GEMM of the
forward and the backward runs unchanged and an adapter costs nothing per sampling step.  Training gets the adapter
gradients from two skinny products per Linear (``omh_lora_grads``) without forming dW; a frozen base then needs no
weight-gradient GEMM, no gradient and no optimizer state (12 bytes per parameter).

    from lora import add_lora, merge_lora, lora_state_dict, load_lora_state_dict
    params = add_lora(model, rank=32)                    # base frozen, adapters trainable
    opt = optim.AdamW(params, lr=1e-4)
    ...
    torch.save(lora_state_dict(model), "adapter.pt")     # or merge_lora(model) for a plain checkpoint

Precision: an update reaches the forward once it exceeds the bf16 ulp of W — the same class as the
fp32-master / bf16-copy full fine-tuning of this package, and not the ``bf16(W) x + s B (A x)`` form of PEFT.
"""
import math
import re

import torch
import torch.nn as nn

__all__ = ["DEFAULT_TARGETS", "I2V_TARGETS", "MAX_RANK", "add_lora", "set_lora_scale", "remove_lora", "merge_lora",
           "lora_state_dict", "load_lora_state_dict", "lora_modules"]

DEFAULT_TARGETS = ("self_attn.q", "self_attn.k", "self_attn.v", "self_attn.o",
                   "cross_attn.q", "cross_attn.k", "cross_attn.v", "cross_attn.o", "ffn.0", "ffn.2")
I2V_TARGETS = ("cross_attn.k_img", "cross_attn.v_img")           # added to the default on an i2v model
MAX_RANK = 128


def _known_targets(model):
    i2v = hasattr(model.blocks[0].cross_attn, "k_img")
    return DEFAULT_TARGETS + (I2V_TARGETS if i2v else ())


def _changed(model):
    """Adapters were added or removed: the cached parameter lists and operand copies are rebuilt on the next call."""
    model.__dict__["_lora_epoch"] = model.__dict__.get("_lora_epoch", 0) + 1
    model.__dict__.pop("_omh_block_params", None)


def lora_modules(model):
    """[(name, Linear)] of the adapted Linears, ``name`` as in the adapter file: ``blocks.{i}.{target}``."""
    out = []
    for i, blk in enumerate(model.blocks):
        for tname in _known_targets(model):
            lin = blk.get_submodule(tname)
            if "lora_A" in lin._parameters:
                out.append((f"blocks.{i}.{tname}", lin))
    return out


def _attach(lin, rank, alpha, A=None, B=None):
    w = lin.weight
    if w.dtype != torch.float32:
        raise TypeError(f"adapters need fp32 master weights, got {w.dtype}")
    a = torch.empty(rank, w.shape[1], dtype=torch.float32, device=w.device)
    if A is None:
        nn.init.kaiming_uniform_(a, a=math.sqrt(5))
    else:
        a.copy_(A)
    b = torch.zeros(w.shape[0], rank, dtype=torch.float32, device=w.device)
    if B is not None:
        b.copy_(B)
    lin.register_parameter("lora_A", nn.Parameter(a))
    lin.register_parameter("lora_B", nn.Parameter(b))
    lin.lora_alpha = float(alpha)
    lin.__dict__.pop("lora_scale_override", None)


def _detach(lin):
    for n in ("lora_A", "lora_B"):
        lin._parameters.pop(n, None)
    for n in ("lora_alpha", "lora_scale_override"):
        lin.__dict__.pop(n, None)


def add_lora(model, rank, alpha=None, targets=DEFAULT_TARGETS, freeze_base=True, lora_dropout=0.0):
    """Give every ``targets`` Linear of every block two fp32 parameters, ``lora_A`` [rank, in] (kaiming-uniform,
    a = sqrt(5)) and ``lora_B`` [out, rank] (zeros: the adapted model starts bit-identical to the bare one), scale
    ``alpha / rank`` (``alpha`` defaults to ``rank``).  ``freeze_base``: every other parameter of the model stops
    requiring grad.  Returns the adapter parameters (for the optimizer)."""
    if lora_dropout:
        raise NotImplementedError("lora_dropout is not built: the effective-weight form W + s B A cannot express a "
                                  "dropout between A and B")
    if isinstance(rank, bool) or not isinstance(rank, int) or not 1 <= rank <= MAX_RANK:
        raise ValueError(f"rank must be an integer in [1, {MAX_RANK}], got {rank!r}")
    alpha = float(rank) if alpha is None else float(alpha)
    known = _known_targets(model)
    if targets is DEFAULT_TARGETS:
        targets = known
    targets = tuple(targets)
    for t in targets:
        if t not in known:
            raise ValueError(f"targets: unknown target {t!r} (known: {', '.join(known)})")
    if not targets:
        raise ValueError("targets: nothing to adapt")
    if lora_modules(model):
        raise RuntimeError("the model already carries adapters (stacking is not built): remove_lora() or merge_lora() first")
    for blk in model.blocks:
        for t in targets:
            _attach(blk.get_submodule(t), rank, alpha)
    _changed(model)
    params = [p for _, lin in lora_modules(model) for p in (lin.lora_A, lin.lora_B)]
    if freeze_base:
        mine = {id(p) for p in params}
        for p in model.parameters():
            if id(p) not in mine:
                p.requires_grad_(False)
    return params


def set_lora_scale(model, scale):
    """Override every adapter's scale ``s`` (strength control at sampling time); None restores ``alpha / rank``.
    The operand copies are rebuilt on the next call; a ContextState built before is rejected."""
    for _, lin in lora_modules(model):
        if scale is None:
            lin.__dict__.pop("lora_scale_override", None)
        else:
            lin.lora_scale_override = float(scale)


def remove_lora(model):
    """Drop the adapters: parameters, state-dict keys and outputs are those of the model before add_lora."""
    mods = lora_modules(model)
    for _, lin in mods:
        _detach(lin)
    if mods:
        _changed(model)


def merge_lora(model):
    """``W += s B A`` in fp32, in place, on the device (omh_lora_merge: the arithmetic of the fused pack, so the merged
    model computes the adapted model's bits), then remove the adapters."""
    from . import ops
    from .wan.modules.model import lora_of, lora_pack_row
    mods = lora_modules(model)
    if not mods:
        return model
    rows, tile0 = [], 0
    with torch.no_grad():
        for _, lin in mods:
            w = lin.weight
            if not w.is_cuda:
                raise ops.OmhError("merge_lora runs on the MI355X only (no CPU fallback): move the model to a GPU device")
            A, B, s = lora_of(lin)
            row = lora_pack_row(w.detach(), None, None, 0, 0, (A.detach(), B.detach(), s))
            row[7] = tile0
            tile0 += ((w.shape[0] + 63) // 64) * ((w.shape[1] + 63) // 64)
            rows.append(row)
        table = torch.tensor(rows, dtype=torch.int64).to(mods[0][1].weight.device)
        ops.lora_merge(table, len(rows), tile0)
        for _, lin in mods:
            lin.weight.mul_(1.0)            # exact identity: bumps the version counter that every operand copy keys on
    remove_lora(model)
    return model


def lora_state_dict(model):
    """{``blocks.{i}.{target}.lora_A.weight``, ``….lora_B.weight``: cpu-or-device tensors, ``….alpha``: 0-d tensor}."""
    sd = {}
    for name, lin in lora_modules(model):
        sd[f"{name}.lora_A.weight"] = lin.lora_A.detach().clone()
        sd[f"{name}.lora_B.weight"] = lin.lora_B.detach().clone()
        sd[f"{name}.alpha"] = torch.tensor(float(lin.lora_alpha))
    return sd


_KEY = re.compile(r"^(?:diffusion_model\.)?(blocks\.(\d+)\.([a-z_0-9.]+?))\.(lora_A\.weight|lora_B\.weight|alpha)$")


def load_lora_state_dict(model, sd, strict=True):
    """Load an adapter file (keys as lora_state_dict writes them, an optional ``diffusion_model.`` prefix accepted).
    On a model without adapters they are added first, rank and targets taken from the file.  ``strict``: every adapter
    of the model must be in the file and every key of the file must be used."""
    entries, unexpected = {}, []
    for k, v in sd.items():
        m = _KEY.match(k)
        if m is None:
            unexpected.append(k)
            continue
        entries.setdefault(m.group(1), {})[m.group(4)] = (v, int(m.group(2)), m.group(3))
    known = _known_targets(model)
    have = dict(lora_modules(model))
    fresh = not have
    for name, ent in entries.items():
        tname = next(iter(ent.values()))[2]
        idx = next(iter(ent.values()))[1]
        if tname not in known or idx >= len(model.blocks):
            unexpected.extend(f"{name}.{k}" for k in ent)
            continue
        if "lora_A.weight" not in ent or "lora_B.weight" not in ent:
            raise KeyError(f"{name}: an adapter needs both lora_A.weight and lora_B.weight")
        A, B = ent["lora_A.weight"][0], ent["lora_B.weight"][0]
        rank = A.shape[0]
        lin = model.blocks[idx].get_submodule(tname)
        if tuple(A.shape) != (rank, lin.weight.shape[1]) or tuple(B.shape) != (lin.weight.shape[0], rank) \
                or not 1 <= rank <= MAX_RANK:
            raise ValueError(f"{name}: adapter shapes {tuple(A.shape)}, {tuple(B.shape)} do not fit the Linear "
                             f"{tuple(lin.weight.shape)} (rank <= {MAX_RANK})")
        alpha = float(ent["alpha"][0]) if "alpha" in ent else float(rank)
        if fresh:
            _attach(lin, rank, alpha, A, B)
        elif name in have:
            if lin.lora_A.shape != A.shape:
                raise ValueError(f"{name}: rank {rank} in the file, {lin.lora_A.shape[0]} on the model")
            with torch.no_grad():
                lin.lora_A.copy_(A)
                lin.lora_B.copy_(B)
            lin.lora_alpha = alpha
        else:
            unexpected.append(name)
    if fresh:
        _changed(model)
    missing = [n for n in have if n not in entries]
    if strict and (missing or unexpected):
        raise RuntimeError(f"load_lora_state_dict: missing adapters {missing}, unexpected keys {unexpected}")
    return missing, unexpected
