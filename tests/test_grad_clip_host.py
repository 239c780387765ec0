"""CPU: the surface of the fused global gradient-norm clip (omnihuman_trainer.py:349-356) — the four C entries in
include/omh.h and their ctypes bindings, torch's signature on ``optim.clip_grad_norm_``, the ``max_grad_norm`` keyword
of ``optim.AdamW`` — and what can be decided without a device: argument checks and the host-side errors."""
import importlib
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "omnihuman-1-hack_amd"
ENTRIES = ("omh_grad_norm_multi", "omh_scale_multi", "omh_adamw_multi_dev", "omh_adamw_pack_multi_dev")


def _header():
    return open(os.path.join(ROOT, "include", "omh.h")).read()


def test_header_declares_the_entries_and_keeps_the_version():
    src = _header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    m = re.search(r"^#define\s+OMH_NORM_CHUNK\s+(\d+)\s*$", code, flags=re.M)
    assert m and int(m.group(1)) > 0 and int(m.group(1)) % 1024 == 0
    assert re.search(r"^#define\s+OMH_ABI_VERSION\s+12\s*$", code, flags=re.M)
    # the chain of fp32 additions the GPU test's tolerance is derived from is stated, and is within the contract
    chain = re.search(r"at most (\d+) chained fp32 additions", src)
    assert chain and int(chain.group(1)) <= 64
    # every entry cites the trainer lines it replaces
    for name in ENTRIES:
        at = src.index("int " + name)
        assert "omnihuman_trainer.py:349" in src[src.rfind("/*", 0, at):at], name


def test_bindings_and_argument_checks(omh, ops):
    binding = importlib.import_module(PKG + "._lib")
    for name in ENTRIES:
        assert name in binding.EXPORTED and hasattr(binding.lib, name)
    assert binding.lib.omh_abi_version() == 12
    chunk = int(re.search(r"#define\s+OMH_NORM_CHUNK\s+(\d+)", _header()).group(1))
    assert ops.NORM_CHUNK == chunk
    lib = binding.lib
    # refused before anything is launched: null pointers, empty tables, a zero loss scale, step 0
    assert lib.omh_grad_norm_multi(None, 1, 1, None, None, 1.0, 1.0, None) == -1
    assert lib.omh_grad_norm_multi(16, 0, 1, 16, 16, 1.0, 1.0, None) == -1
    assert lib.omh_grad_norm_multi(16, 1, 0, 16, 16, 1.0, 1.0, None) == -1
    assert lib.omh_grad_norm_multi(16, 1, 1 << 31, 16, 16, 1.0, 1.0, None) == -1
    assert lib.omh_grad_norm_multi(16, 1, 1, 16, 16, 1.0, 0.0, None) == -1
    assert lib.omh_grad_norm_multi(16, 1, 1, 16, None, 1.0, 1.0, None) == -1
    assert lib.omh_scale_multi(None, 1, 1, 16, None) == -1
    assert lib.omh_scale_multi(16, 1, 1, None, None) == -1
    assert lib.omh_scale_multi(16, 1, 0, 16, None) == -1
    assert lib.omh_adamw_multi_dev(16, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, None, None) == -1
    assert lib.omh_adamw_multi_dev(16, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1.0, 16, None) == -1
    assert lib.omh_adamw_multi_dev(None, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, 16, None) == -1
    assert lib.omh_adamw_pack_multi_dev(16, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, None, None) == -1
    assert lib.omh_adamw_pack_multi_dev(16, 1, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, 16, None) == -1
    assert lib.omh_adamw_pack_multi_dev(16, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0.0, 16, None) == -1
    for name in ("grad_norm_multi", "scale_multi", "adamw_multi_dev", "adamw_pack_multi_dev"):
        assert callable(getattr(ops, name))


def test_clip_grad_norm_has_torchs_signature(omh):
    optim = importlib.import_module(PKG + ".optim")
    ours = inspect.signature(optim.clip_grad_norm_).parameters
    theirs = inspect.signature(torch.nn.utils.clip_grad_norm_).parameters
    assert list(ours) == ["parameters", "max_norm", "norm_type", "error_if_nonfinite", "foreach"]
    assert list(ours) == list(theirs)
    for k in ours:
        assert ours[k].default == theirs[k].default, k


def test_clip_grad_norm_host_side_behaviour(omh, ops):
    optim = importlib.import_module(PKG + ".optim")
    p = torch.nn.Parameter(torch.zeros(4))
    out = optim.clip_grad_norm_([p], 1.0)                            # nothing has a gradient
    assert out.dim() == 0 and out.dtype == torch.float32 and float(out) == 0.0
    assert float(optim.clip_grad_norm_(p, 1.0)) == 0.0                # a single tensor
    assert float(optim.clip_grad_norm_(iter([p]), 1.0, foreach=True)) == 0.0
    for bad in (1.0, 3, float("inf")):
        with pytest.raises(NotImplementedError, match=re.escape(repr(bad))):
            optim.clip_grad_norm_([p], 1.0, norm_type=bad)
    p.grad = torch.ones(4)
    with pytest.raises(ops.OmhError):                                 # no CPU fallback
        optim.clip_grad_norm_([p], 1.0)


def test_adamw_accepts_max_grad_norm(omh):
    optim = importlib.import_module(PKG + ".optim")
    par = inspect.signature(optim.AdamW.__init__).parameters
    assert par["max_grad_norm"].default is None
    assert list(par)[:6] == ["self", "params", "lr", "betas", "eps", "weight_decay"]
    w = torch.nn.Parameter(torch.zeros(3))
    plain = optim.AdamW([w], lr=1e-3)
    assert plain.max_grad_norm is None and plain.grad_norm is None
    opt = optim.AdamW([w], lr=1e-3, max_grad_norm=1)
    assert opt.max_grad_norm == 1.0 and isinstance(opt.max_grad_norm, float)
    # an attribute of the optimizer, not a hyper-parameter: the state dict is torch's
    assert "max_grad_norm" not in opt.defaults and "max_grad_norm" not in opt.param_groups[0]
    ref = torch.optim.AdamW([w], lr=1e-3)
    assert set(opt.state_dict()["param_groups"][0]) <= set(ref.state_dict()["param_groups"][0])
    opt.load_state_dict(ref.state_dict())
    assert opt.max_grad_norm == 1.0 and "max_grad_norm" not in opt.param_groups[0]
    opt.step()                                                        # no gradients: nothing to launch, no norm
    assert opt.grad_norm is None
