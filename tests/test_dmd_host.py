"""CPU: the surface of the DMD objective (self forcing's distribution-matching loss) — the C entries in include/omh.h and
their ctypes bindings, the argument checks that come before the device, the workspace query (pure host arithmetic),
``causal.dmd_sigmas`` against its closed form, and the argument rules of ``causal.dmd_loss`` / ``causal.critic_loss``.
Nothing here launches a kernel."""
import importlib
import os
import re
import types

import pytest
import torch

import make_golden_chunk_causal as MC
from conftest import PKG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("omh_dmd_grad", "omh_dmd_grad_workspace_bytes", "omh_dmd_grad_scale")


@pytest.fixture(scope="module")
def causal(omh):
    return importlib.import_module(PKG + ".causal")


def _header():
    return open(os.path.join(ROOT, "include", "omh.h")).read()


def test_header_declares_the_entries_and_keeps_the_version():
    src = _header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+omh_dmd_grad\s*\(", code)
    assert re.search(r"\bint64_t\s+omh_dmd_grad_workspace_bytes\s*\(\s*int32_t\s+B\s*,\s*int64_t\s+n\s*\)", code)
    assert re.search(r"\bint\s+omh_dmd_grad_scale\s*\(", code)
    assert re.search(r"^#define\s+OMH_ABI_VERSION\s+12\s*$", code, flags=re.M)
    m = re.search(r"^#define\s+OMH_DMD_CHUNK\s+(\d+)\s*$", code, flags=re.M)
    assert m and int(m.group(1)) > 0 and int(m.group(1)) % 1024 == 0
    for name in ("omh_dmd_grad", "omh_dmd_grad_scale"):              # each cites what it replaces
        at = src.index("int " + name + "(")
        assert "replaces" in src[src.rfind("/*", 0, at):at], name


def test_bindings_and_argument_checks(omh, ops):
    binding = importlib.import_module(PKG + "._lib")
    lib = binding.lib
    for name in ENTRIES:
        assert name in binding.EXPORTED and hasattr(lib, name)
    assert lib.omh_abi_version() == 12
    chunk = int(re.search(r"#define\s+OMH_DMD_CHUNK\s+(\d+)", _header()).group(1))
    assert ops.DMD_CHUNK == chunk
    for name in ("dmd_grad", "dmd_loss", "flow_noise"):
        assert callable(getattr(ops, name)) and name in ops.__all__
    p = 4096                                                         # never dereferenced: refused before the device

    def call(x=p, xt=p, vc=p, vu=p, vf=p, sigma=p, B=2, n=8, grad=p, norm=p, loss=p, ws=p):
        return lib.omh_dmd_grad(x, xt, vc, vu, vf, sigma, 3.0, B, n, grad, norm, loss, ws, None)
    assert lib.omh_dmd_grad(None, None, None, None, None, None, 3.0, 2, 8, None, None, None, None, None) == -1
    for field in ("x", "xt", "vc", "vf", "sigma", "grad", "norm", "loss", "ws"):
        assert call(**{field: None}) == -1, field                    # every pointer but v_uncond is required
    assert call(B=0) == -2 and call(B=-1) == -2 and call(n=0) == -2 and call(n=-5) == -2
    assert call(x=None, B=0) == -1                                   # the NULL check comes first
    assert call(x=p + 2) == -2 and call(loss=p + 4) == -2 and call(ws=p + 4) == -2          # 4-byte / 8-byte alignment
    assert call(B=2, n=(1 << 23) * chunk) == -3                      # more chunks than a grid may hold
    assert lib.omh_dmd_grad_scale(None, p, 1.0, 8, p, None) == -1
    assert lib.omh_dmd_grad_scale(p, None, 1.0, 8, p, None) == -1
    assert lib.omh_dmd_grad_scale(p, p, 1.0, 8, None, None) == -1
    assert lib.omh_dmd_grad_scale(p, p, 1.0, 0, p, None) == -2
    assert lib.omh_dmd_grad_scale(p, p + 4, 1.0, 8, p, None) == -2


def test_workspace_query_is_host_arithmetic(omh, ops):
    ws, C = ops.dmd_grad_workspace_bytes, ops.DMD_CHUNK
    per_chunk = ws(1, 1)                                             # one chunk's partials
    assert per_chunk > 0 and per_chunk % 8 == 0
    assert ws(0, 8) == 0 and ws(2, 0) == 0
    for B in (1, 2, 3, 7):
        assert ws(B, 1) == ws(B, 5) == ws(B, C) == B * per_chunk     # equal inside one chunk count
        assert ws(B, C + 1) - ws(B, C) == B * per_chunk              # one chunk more per sample across the boundary
        assert ws(B, C + 1) == ws(B, C + 3) == ws(B, 2 * C)
        assert ws(B + 1, 3 * C) > ws(B, 3 * C)                       # monotone in B ...
        sizes = [ws(B, k * C + 1) for k in range(6)]
        assert sizes == sorted(sizes) and len(set(sizes)) == 6      # ... and in the chunk count
    assert ws(3, (1 << 33) + 1) == 3 * ((1 << 33) // C + 1) * per_chunk     # 64-bit sizes


def test_dmd_sigmas_closed_form(causal):
    lo, hi, shift = 0.02, 0.98, 5.0
    sigma, t = causal.dmd_sigmas(257, generator=torch.Generator().manual_seed(5), device="cpu")
    u = lo + (hi - lo) * torch.rand(257, dtype=torch.float32, generator=torch.Generator().manual_seed(5))
    assert sigma.shape == t.shape == (257,) and sigma.dtype == t.dtype == torch.float32
    want = shift * u.double() / (1 + (shift - 1) * u.double())
    assert float((sigma.double() - want).abs().max()) < 4 * 2.0 ** -24
    assert torch.equal(t, 1000.0 * sigma)
    s_lo, s_hi = shift * lo / (1 + (shift - 1) * lo), shift * hi / (1 + (shift - 1) * hi)
    assert float(sigma.min()) >= s_lo - 1e-6 and float(sigma.max()) <= s_hi + 1e-6 and float(sigma.min()) < float(sigma.max())
    for end, s_end in ((lo, s_lo), (hi, s_hi)):                      # the endpoints: u = lo and u = hi
        s, tt = causal.dmd_sigmas(3, lo=end, hi=end, device="cpu")
        assert float((s.double() - s_end).abs().max()) < 4 * 2.0 ** -24 and 0.0 < float(s.min()) and float(s.max()) < 1.0
        assert float((tt.double() - 1000 * s_end).abs().max()) < 1e-3
    s, _ = causal.dmd_sigmas(4, lo=0.3, hi=0.3, shift=1.0, device="cpu")                    # shift 1: the identity
    assert float((s - 0.3).abs().max()) < 1e-7
    assert causal.dmd_sigmas(2, generator=torch.Generator().manual_seed(1))[0].device.type == "cpu"   # the generator's device
    for bad in (dict(B=0), dict(B=2, lo=0.0), dict(B=2, hi=1.0), dict(B=2, lo=0.6, hi=0.4), dict(B=2, shift=0.0)):
        with pytest.raises(ValueError):
            causal.dmd_sigmas(device="cpu", **bad)


def test_loss_argument_errors_come_before_the_device(omh, ops, wan_model_mod, causal):
    teacher = wan_model_mod.WanModel(num_layers=2, **MC.make_golden.TINY)
    critic = wan_model_mod.WanModel(num_layers=2, **MC.make_golden.TINY)
    clips = [torch.zeros(16, 6, 14, 16) for _ in range(2)]
    ctx = [torch.zeros(8, 64) for _ in range(2)]
    ok = dict(sigma=torch.full((2,), 0.5), timesteps=torch.full((2,), 500.0))
    untouched = object()                                             # the models are not looked at before the shapes
    for fn, args in ((causal.dmd_loss, (untouched, untouched, ctx)), ):
        with pytest.raises(ValueError, match="clips"):
            fn([clips[0], clips[1][:, :3]], *args, **ok)
        with pytest.raises(ValueError, match="clips"):
            fn([], *args, **ok)
        with pytest.raises(ValueError, match="sigma"):
            fn(clips, *args, sigma=torch.full((3,), 0.5), timesteps=ok["timesteps"])
        with pytest.raises(ValueError, match="sigma"):
            fn(clips, *args, sigma=torch.full((2, 1), 0.5), timesteps=ok["timesteps"])
        with pytest.raises(ValueError, match="timesteps"):
            fn(clips, *args, sigma=ok["sigma"], timesteps=torch.full((1,), 500.0))
        with pytest.raises(ValueError, match="eps"):
            fn(clips, *args, eps=torch.zeros(2, 16, 6, 14, 8), **ok)
    with pytest.raises(ValueError, match="clips"):
        causal.critic_loss(untouched, [clips[0], clips[1][:, :3]], ctx, **ok)
    with pytest.raises(ValueError, match="sigma"):
        causal.critic_loss(untouched, clips, ctx, sigma=torch.full((3,), 0.5), timesteps=ok["timesteps"])
    with pytest.raises(ValueError, match="timesteps"):
        causal.critic_loss(untouched, clips, ctx, sigma=ok["sigma"], timesteps=torch.full((2, 2), 500.0))
    # a model with a forward that awaits its backward (the student): refused, and named
    teacher.__dict__["_omh_live_states"] = [types.SimpleNamespace()]
    with pytest.raises(RuntimeError, match="teacher"):
        causal.dmd_loss(clips, teacher, critic, ctx, **ok)
    with pytest.raises(RuntimeError, match="critic"):
        causal.dmd_loss(clips, critic, teacher, ctx, **ok)
    teacher.__dict__["_omh_live_states"] = [types.SimpleNamespace(bwd_done=True)]            # its backward has run: fine
    with pytest.raises(ops.OmhError):                                # valid arguments reach the device check: no CPU fallback
        causal.dmd_loss(clips, teacher, critic, ctx, **ok)
    with pytest.raises(ops.OmhError):
        causal.critic_loss(critic, clips, ctx, **ok)
    with pytest.raises(ops.OmhError):
        ops.flow_noise(torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(2))
    with pytest.raises(ops.OmhError):
        ops.dmd_grad(*[torch.zeros(2, 8)] * 5, torch.zeros(2), 3.0)
