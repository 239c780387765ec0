"""CPU: the host side of the streaming VAE decode — the omh_cl_to_u8 declaration and binding, the frame arithmetic of
``DecodeStream.push``, and the argument rules of ``WanVAE.decode_stream`` and ``causal.stream`` (no compute without a
GPU)."""
import importlib
import os
import re

import pytest
import torch

from conftest import PKG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vae_mod(omh):
    return importlib.import_module(PKG + ".wan.modules.vae")


@pytest.fixture(scope="module")
def causal(omh):
    return importlib.import_module(PKG + ".causal")


def test_cl_to_u8_is_declared_and_bound_with_matching_arity(omh):
    binding = importlib.import_module(PKG + "._lib")
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "omh.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+omh_cl_to_u8\s*\(([^)]*)\)\s*;", src)
    assert m, "omh_cl_to_u8 is not declared in include/omh.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert "omh_cl_to_u8" in binding.EXPORTED and hasattr(binding.lib, "omh_cl_to_u8")
    fn = binding.lib.omh_cl_to_u8
    assert len(fn.argtypes) == len(params) == 12 and fn.restype is binding.i32
    # pointers / int32 / float in the header's order
    kinds = ["p" if "*" in p or "omh_stream_t" in p else ("f" if p.startswith("float") else "i") for p in params]
    want = {"p": binding.vp, "f": binding.f32, "i": binding.i32}
    assert [want[k] for k in kinds] == list(fn.argtypes)
    # the comment in front of it cites the reference's rule
    head = open(os.path.join(ROOT, "include", "omh.h")).read().split("int omh_cl_to_u8")[0][-1500:]
    assert "utils.py:40-47" in head
    assert binding.ABI_VERSION == 12 and binding.lib.omh_abi_version() == 12
    assert re.search(r"#define\s+OMH_ABI_VERSION\s+12\b", open(os.path.join(ROOT, "include", "omh.h")).read())


def test_cl_to_u8_rejects_bad_arguments_before_the_device(omh):
    lib = importlib.import_module(PKG + "._lib").lib
    ok = dict(x=4096, out=4096, C=3, T=1, H=2, W=2, Cp=3, lo=-1.0, hi=1.0, t_total=2, t0=0)

    def rc(**kw):
        a = dict(ok, **kw)
        return lib.omh_cl_to_u8(a["x"], a["out"], a["C"], a["T"], a["H"], a["W"], a["Cp"], a["lo"], a["hi"], a["t_total"],
                                a["t0"], None)
    assert rc(x=None) == -1 and rc(out=None) == -1
    assert rc(T=0) == -1 and rc(H=0) == -1 and rc(W=-1) == -1 and rc(C=0) == -1
    assert rc(Cp=2) == -1                                            # Cp < C
    assert rc(t0=-1) == -1 and rc(t0=2) == -1 and rc(T=3) == -1      # frames outside [0, t_total)
    assert rc(lo=1.0, hi=1.0) == -1 and rc(lo=2.0) == -1             # an empty range
    assert rc(lo=-3.0e38, hi=3.0e38) == -3                           # hi - lo is no finite fp32
    assert rc(x=4098) == -2                                          # x not 4-byte aligned


def test_push_frame_arithmetic(vae_mod):
    """The clip's first latent frame is one pixel frame, every other one four: pushes of (1, 2, 1) give 1, 8 and 4."""
    f = vae_mod.stream_frames
    got, seen = [], 0
    for n in (1, 2, 1):
        got.append(f(seen, n))
        seen += n
    assert got == [1, 8, 4] and sum(got) == 4 * (seen - 1) + 1
    assert f(0, 5) == 17 and f(5, 5) == 20 and f(0, 1) == 1 and f(40, 1) == 4
    for parts in ([5], [1, 1, 1, 1, 1], [2, 2, 1], [1, 4], [3, 1, 2]):
        seen = total = 0
        for n in parts:
            total += f(seen, n)
            seen += n
        assert total == 4 * (seen - 1) + 1
    for bad in ((0, 0), (-1, 1), (3, -2)):
        with pytest.raises(ValueError):
            f(*bad)


def test_decode_stream_argument_rules_on_a_cpu_model(vae_mod, ops):
    vae = vae_mod.WanVAE(vae_pth=None, dtype=torch.bfloat16, device="cpu", dim=32)
    with pytest.raises(ValueError):
        vae.decode_stream(output="png")
    for output in ("float", "uint8"):
        ds = vae.decode_stream(output=output)
        assert isinstance(ds, vae_mod.DecodeStream) and ds.output == output
        assert (ds.frames_in, ds.frames_out, ds.h, ds.w) == (0, 0, None, None) and ds.state_bytes() == 0
        with pytest.raises(ops.OmhError):                            # no CPU fallback, as decode
            ds.push(torch.zeros(16, 1, 8, 8))
        assert (ds.frames_in, ds.frames_out) == (0, 0)
        ds.reset()                                                   # nothing to reset yet: a no-op
    assert vae.decode_stream() is not vae.decode_stream()            # streams of one VAE are separate objects
    with pytest.raises(ops.OmhError):
        vae.decode([torch.zeros(16, 1, 8, 8)])
    assert "DecodeStream" in (vae.model.clear_cache.__doc__ or "")


def test_stream_rejects_what_sample_rejects(causal, wan_model_mod):
    m = wan_model_mod.WanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=64, text_len=8, freq_dim=64)
    ctx = [torch.zeros(3, 64)]
    noise = torch.zeros(16, 5, 8, 8)
    kw = dict(frames_per_chunk=2, make_scheduler=lambda: None, guide_scale=5.0)
    for fn in (causal.sample, causal.stream):
        with pytest.raises(ValueError):
            fn(m, noise[0], ctx, ctx, **kw)                          # not one clip [C, F, H, W]
        with pytest.raises(ValueError):
            fn(m, noise, ctx, ctx, rolling=True, **kw)               # rolling needs a bounded look-back
        with pytest.raises(ValueError):
            fn(m, noise, ctx, ctx, left_chunks=1, sink_chunks=-1, **kw)
    with pytest.raises(ValueError):
        causal.stream(m, noise, ctx, ctx, output="png", **kw)
    assert getattr(m, "_causal_chunks", None) is None                # a refusal leaves the model's setting alone
    gen = causal.stream(m, noise, ctx, ctx, **kw)                    # nothing runs before the first chunk is asked for
    assert getattr(m, "_causal_chunks", None) is None
    gen.close()
    c = causal.StreamChunk(0, (0, 2), torch.zeros(1))
    assert (c.index, c.frames, c.video, c.ready) == (0, (0, 2), None, None) and c.wait() is c
