"""The streaming VAE decode on the GPU: omh_cl_to_u8 against torch's statement of the reference's 8-bit rule
(wan/utils/utils.py:40-47), and ``WanVAE.decode_stream`` — the frames of ANY partition of a clip's latent frames into
pushes equal ``WanVAE.decode`` of the whole clip bit for bit, in both arithmetic classes, across window wraps, buffer
regrowth, two interleaved streams and a reset.  Miniatures as in test_gpu_vae.py (dim 32 / 96, latents [16, T', 8, 8])."""
import importlib
import math

import pytest
import torch

from conftest import PKG, rel_rms

pytestmark = pytest.mark.gpu
TOL_VAE = 2.0e-2            # the whole-VAE bound of the bf16 mode (test_gpu_vae.py)
_CACHE = {}


@pytest.fixture(scope="module")
def vae_mod():
    return importlib.import_module(PKG + ".wan.modules.vae")


def _vae(vae_mod, dim, dtype):
    """(vae, state dict, oracle config) of a miniature, built once per module."""
    key = ("vae", dim, dtype)
    if key not in _CACHE:
        from oracle import wan_vae_oracle as V
        cfg = V.VAEConfig(dim=dim)
        sd = V.synth_state_dict(cfg, f"vae{dim}")
        vae = vae_mod.WanVAE(vae_pth=None, dtype=dtype, device="cuda", dim=dim)
        vae.model.load_state_dict(sd)
        _CACHE[key] = (vae, sd, cfg)
    return _CACHE[key]


def _clip(vae_mod, dim, dtype, frames, tag="vae/zs"):
    """(latent [16, frames, 8, 8] on the device, vae.decode of it), computed once and left unchanged."""
    key = ("clip", dim, dtype, frames, tag)
    if key not in _CACHE:
        from oracle import detgen
        z = torch.from_numpy(detgen.normalish(f"{tag}{frames}", (16, frames, 8, 8))).cuda()
        _CACHE[key] = (z, _vae(vae_mod, dim, dtype)[0].decode([z])[0])
    return _CACHE[key]


def _pushes(stream, z, parts):
    out, f = [], 0
    for n in parts:
        out.append(stream.push(z[:, f:f + n]))
        f += n
    assert f == z.shape[1]
    return out


def _u8_rule(x):
    """The reference's rule on fp32 values (utils.py:40-47 with value_range (-1, 1))."""
    return ((x.clamp(-1, 1) + 1) / 2 * 255).to(torch.uint8)


def _planted(shape, C, seed):
    """normal x 1.5 with the edge values planted in the channels that are converted."""
    T, H, W, Cp = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, H, W, Cp, generator=g) * 1.5
    k = torch.arange(256, dtype=torch.float32)
    edges = k / 127.5 - 1                                              # where u * 255 reaches the integer k
    inf = float("inf")
    special = torch.cat([torch.tensor([-1.0, 1.0, 1.0000001, -1.0000001, 3.0, -3.0, inf, -inf, 0.0]), edges,
                         torch.nextafter(edges, torch.full_like(edges, 2.0)),
                         torch.nextafter(edges, torch.full_like(edges, -2.0))])
    live = x[..., :C].reshape(-1).clone()
    n = min(live.numel(), special.numel())
    live[:n] = special[:n]
    x[..., :C] = live.view(T, H, W, C)
    return x.cuda()


@pytest.mark.parametrize("shape,C,t0,t_total", [
    ((1, 1, 1, 3), 3, 0, 1),
    ((2, 3, 5, 3), 3, 1, 4),            # 90 bytes at byte 45 of the buffer: an unaligned frame base, odd counts, a tail
    ((3, 8, 8, 8), 3, 0, 3),            # Cp > C
    ((1, 64, 64, 3), 3, 0, 1),          # several workgroups
    ((2, 3, 5, 3), 3, 0, 2),            # the same bytes from an aligned base
    ((1, 7, 9, 5), 4, 2, 3),            # Cp > C with another C
])
def test_cl_to_u8_equals_the_torch_rule(ops, shape, C, t0, t_total):
    T, H, W, Cp = shape
    x = _planted(shape, C, seed=T * 1000 + H * W + Cp)
    out = torch.full((t_total, H, W, C), 0xAB, dtype=torch.uint8, device="cuda")
    ops.cl_to_u8(x, out, t0, C)
    ref = _u8_rule(x[..., :C])
    assert torch.equal(out[t0:t0 + T], ref)
    keep = torch.ones(t_total, dtype=torch.bool)
    keep[t0:t0 + T] = False
    assert bool((out[keep.cuda()] == 0xAB).all())                      # frames outside [t0, t0 + T) keep the sentinel
    again = torch.full_like(out, 0xAB)
    ops.cl_to_u8(x, again, t0, C)
    assert torch.equal(again, out)
    assert torch.equal(ref, _u8_rule(x[..., :C].cpu()).cuda())         # torch agrees with itself on the host
    # another range, whose width is no power of two (the kernel then divides): IEEE arithmetic on the host as reference
    lo, hi = -0.5, 2.5
    ops.cl_to_u8(x, out, t0, C, lo=lo, hi=hi)
    xc = x[..., :C].cpu()
    want = ((xc.clamp(lo, hi) - lo) / torch.tensor(hi - lo, dtype=torch.float32) * 255).to(torch.uint8)
    assert torch.equal(out[t0:t0 + T].cpu(), want)


def test_cl_to_u8_refusals(ops):
    x = torch.zeros(1, 2, 2, 3, device="cuda")
    out = torch.zeros(1, 2, 2, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ops.OmhError):
        ops.cl_to_u8(x, out, 1, 3)                                     # frame 1 of a one-frame buffer
    with pytest.raises(ops.OmhError):
        ops.cl_to_u8(x, out, 0, 3, lo=1.0, hi=1.0)
    with pytest.raises(ops.OmhError):
        ops.cl_to_u8(x.cpu(), out, 0, 3)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float], ids=["bf16", "fp32"])
@pytest.mark.parametrize("dim", [32, 96])
def test_stream_equals_the_whole_clip(vae_mod, dim, dtype):
    vae, sd, cfg = _vae(vae_mod, dim, dtype)
    z, whole = _clip(vae_mod, dim, dtype, 5)
    assert whole.shape == (3, 17, 64, 64)
    for parts in ([5], [1, 1, 1, 1, 1], [2, 2, 1], [1, 4]):
        s = vae.decode_stream()
        got = _pushes(s, z, parts)
        assert [g.shape[1] for g in got] == [4 * n - 3 if i == 0 else 4 * n for i, n in enumerate(parts)]
        assert all(g.dtype == torch.float32 and g.shape[0] == 3 and g.shape[2:] == (64, 64) for g in got)
        assert torch.equal(torch.cat(got, 1), whole), parts
        assert (s.frames_in, s.frames_out, s.h, s.w) == (5, 17, 8, 8)
        assert s.state_bytes() >= s.history_bytes() > 0
    if dim == 32 and dtype == torch.bfloat16:                          # ... and pinned to the oracle, not only to itself
        from oracle import wan_vae_oracle as V
        ref = V.vae_decode(sd, cfg, z.cpu())
        e = rel_rms(whole, ref)
        print(f"rel_rms(decode, oracle) = {e:.3e}")
        assert e < TOL_VAE


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float], ids=["bf16", "fp32"])
def test_uint8_output_is_the_torch_rule_on_the_float_frames(vae_mod, dtype):
    vae, _, _ = _vae(vae_mod, 32, dtype)
    z, whole = _clip(vae_mod, 32, dtype, 5)
    parts = [2, 2, 1]
    got = _pushes(vae.decode_stream(output="uint8"), z, parts)
    assert [tuple(g.shape) for g in got] == [(5, 64, 64, 3), (8, 64, 64, 3), (4, 64, 64, 3)]
    assert all(g.dtype == torch.uint8 for g in got)
    assert torch.equal(torch.cat(got, 0), _u8_rule(whole.permute(1, 2, 3, 0)))


@pytest.mark.parametrize("window", ["default", "one-chunk", "two-chunks"])
def test_long_stream_and_window_wrap(vae_mod, window, monkeypatch):
    """40 pushes of one latent frame: past the default window of hist + 8 max(T, 4) frames, and with the window forced to
    exactly [history | chunk] (the history is copied back before every push, the overlapping T = 1, hist = 2 case
    included) and to two chunks (every other push wraps)."""
    vae, _, _ = _vae(vae_mod, 32, torch.bfloat16)
    z, whole = _clip(vae_mod, 32, torch.bfloat16, 40)                  # the reference first, under the default window
    assert whole.shape == (3, 157, 64, 64)
    if window != "default":
        orig_slot = vae_mod._ConvState.slot
        chunks = 1 if window == "one-chunk" else 2

        def small_slot(self, T, H, W, device):
            # budget of exactly hist + chunks * T frames for this layer
            monkeypatch.setattr(vae_mod._ConvState, "_WINDOW_BYTES", (self.hist + chunks * max(T, 1)) * H * W * self.Cin * 2)
            return orig_slot(self, T, H, W, device)
        monkeypatch.setattr(vae_mod._ConvState, "slot", small_slot)
    s = vae.decode_stream()
    got = _pushes(s, z, [1] * 40)
    assert torch.equal(torch.cat(got, 1), whole)
    assert (s.frames_in, s.frames_out) == (40, 157)


def test_streams_are_independent_and_reset_starts_a_new_clip(vae_mod):
    vae, _, _ = _vae(vae_mod, 32, torch.bfloat16)
    za, wa = _clip(vae_mod, 32, torch.bfloat16, 5)
    zb, wb = _clip(vae_mod, 32, torch.bfloat16, 5, tag="vae/zother")
    assert not torch.equal(wa, wb)
    a, b = vae.decode_stream(), vae.decode_stream()
    ga, gb, fa, fb = [], [], 0, 0
    for na, nb in ((2, 1), (1, 3), (2, 1)):                            # interleaved, different partitions
        ga.append(a.push(za[:, fa:fa + na]))
        gb.append(b.push(zb[:, fb:fb + nb]))
        fa, fb = fa + na, fb + nb
    assert torch.equal(torch.cat(ga, 1), wa) and torch.equal(torch.cat(gb, 1), wb)
    held = a.state_bytes()
    a.reset()
    assert (a.frames_in, a.frames_out) == (0, 0) and a.state_bytes() == held       # the buffers are kept
    assert torch.equal(torch.cat(_pushes(a, za, [1, 4]), 1), wa)                    # a first chunk again
    b.reset()
    assert torch.equal(torch.cat(_pushes(b, za, [3, 2]), 1), wa)                    # ... on another clip as well
    with pytest.raises(ValueError):
        a.push(torch.zeros(16, 1, 8, 6, device="cuda"))                            # another h, w
    with pytest.raises(ValueError):
        a.push(torch.zeros(16, 1, 8, 8))                                           # another device
    with pytest.raises(ValueError):
        a.push(torch.zeros(16, 0, 8, 8, device="cuda"))
    assert (a.frames_in, a.frames_out) == (5, 17)                                  # a refused push changes nothing


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float], ids=["bf16", "fp32"])
def test_varying_push_sizes_regrow_the_windows_with_their_history(vae_mod, dtype, monkeypatch):
    """(3, 1, 2): with windows of exactly [history | chunk] the push of 2 behind the push of 1 has to grow every buffer
    and carry the history over (``_ConvState.slot``); under the default window the same pushes slide."""
    vae, _, _ = _vae(vae_mod, 32, dtype)
    z, _ = _clip(vae_mod, 32, dtype, 5)
    z6 = torch.cat([z, z[:, :1] * 0.5], 1)
    whole = vae.decode([z6])[0]
    assert torch.equal(torch.cat(_pushes(vae.decode_stream(), z6, [3, 1, 2]), 1), whole)
    orig_slot = vae_mod._ConvState.slot

    def small_slot(self, T, H, W, device):
        for name in ("_WINDOW_BYTES", "_WINDOW_BYTES_F32"):
            monkeypatch.setattr(vae_mod._ConvState, name, (self.hist + max(T, 1)) * H * W * self.Cin * 2)
        return orig_slot(self, T, H, W, device)
    monkeypatch.setattr(vae_mod._ConvState, "slot", small_slot)
    assert torch.equal(torch.cat(_pushes(vae.decode_stream(), z6, [1, 1, 2, 1, 1]), 1), whole)


@pytest.mark.parametrize("K,epi", [(384, "bf16"), (1152, "f32")])
def test_attention_gemms_do_not_depend_on_the_frame_count(ops, K, epi):
    """The per-frame attention block's GEMMs at the 480 x 832 geometry (h w = 6 240 rows per latent frame, C = 384; the
    fp32 mode's contraction is three times as long): the q | k projection carries M = n h w rows, and whichever kernel
    the dispatch picks for n = 21 computes frame 0's rows as the n = 1 call does — every family walks k in ascending
    order into one accumulator per element (split K needs a workspace that these calls never pass).  The same for the
    batched score product, batch = 1 against 4."""
    HW, Cc = 6240, 384
    g = torch.Generator(device="cuda").manual_seed(K)
    a = (torch.randn(21 * HW, K, device="cuda", generator=g)).to(torch.bfloat16)
    w = (torch.randn(2 * Cc, K, device="cuda", generator=g) / math.sqrt(K)).to(torch.bfloat16)
    bias = torch.randn(2 * Cc, device="cuda", generator=g)
    e = ops.EPI_BF16 if epi == "bf16" else ops.EPI_F32
    one = ops.gemm(a[:HW], w, bias=bias, epilogue=e)
    for n in (3, 21):
        assert torch.equal(ops.gemm(a[:n * HW], w, bias=bias, epilogue=e)[:HW], one), n
    del one
    q = a[:4 * HW].contiguous()

    def scores(batch):
        s = torch.empty(batch, HW, HW, dtype=torch.float32, device="cuda")
        ops.gemm_raw(ops.ptr(q), ops.ptr(q), ops.ptr(s), HW, HW, K, K, K, HW, ops.EPI_F32, batch=batch,
                     strideA=HW * K, strideB=HW * K, strideC=HW * HW)
        return s
    s1 = scores(1)[0]
    assert torch.equal(scores(4)[0], s1)
