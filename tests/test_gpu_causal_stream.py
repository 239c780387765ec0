"""``causal.stream``: the chunk-by-chunk rollout as a generator, with the pixel frames of every chunk from a
``WanVAE.decode_stream`` — the latents are those of ``causal.sample`` and the frames those of ``WanVAE.decode`` on the
sampled clip, bit for bit, with the decode on the main stream or overlapped on a side stream.  The miniature WanModel,
scheduler and contexts of test_gpu_chunk_causal_model.py (tiny t2v, 2 layers), latents [16, 5, 8, 8] in chunks of 2 frames,
a 2-step UniPC scheduler, the dim-32 VAE of test_gpu_vae.py."""
import importlib

import pytest
import torch

import make_golden_chunk_causal as MC
from conftest import PKG

pytestmark = pytest.mark.gpu
_CACHE = {}


@pytest.fixture(scope="module")
def causal():
    return importlib.import_module(PKG + ".causal")


def _setup():
    """(model, conditional context, null context, noise, scheduler factory, vae), built once per module."""
    if "setup" not in _CACHE:
        from oracle import wan_dit_oracle as O, wan_vae_oracle as V
        model_mod = importlib.import_module(PKG + ".wan.modules.model")
        vae_mod = importlib.import_module(PKG + ".wan.modules.vae")
        unipc = importlib.import_module(PKG + ".wan.utils.fm_solvers_unipc")
        cfg, _, ctx, _, _ = MC.case()
        m = model_mod.WanModel(num_layers=2, **MC.make_golden.TINY)
        m.load_state_dict(O.synth_state_dict(cfg, MC.TAG))
        m = m.cuda().eval().requires_grad_(False)
        ctx = [c.cuda() for c in ctx]
        cond, null = ctx[:1], [ctx[0][:5]]
        noise = torch.randn(16, 5, 8, 8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(11))

        def make_scheduler():
            s = unipc.FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
            s.set_timesteps(2, device="cuda", shift=3.0)
            return s
        vae = vae_mod.WanVAE(vae_pth=None, dtype=torch.bfloat16, device="cuda", dim=32)
        vae.model.load_state_dict(V.synth_state_dict(V.VAEConfig(dim=32), "vae32"))
        _CACHE["setup"] = (m, cond, null, noise, make_scheduler, vae)
    return _CACHE["setup"]


SETTINGS = {"unbounded": dict(left_chunks=-1), "rolling": dict(rolling=True, sink_chunks=1, left_chunks=1)}


def _reference(causal, setting):
    """(causal.sample of the clip, vae.decode of it), computed once per setting and left unchanged."""
    if setting not in _CACHE:
        m, cond, null, noise, make_scheduler, vae = _setup()
        lat = causal.sample(m, noise, cond, null, frames_per_chunk=2, make_scheduler=make_scheduler, guide_scale=5.0,
                            **SETTINGS[setting])
        _CACHE[setting] = (lat, vae.decode([lat])[0])
    return _CACHE[setting]


def _kw(setting):
    return dict(frames_per_chunk=2, make_scheduler=_setup()[4], guide_scale=5.0, **SETTINGS[setting])


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_latents_equal_sample(causal, setting):
    m, cond, null, noise, _, _ = _setup()
    ref, _ = _reference(causal, setting)
    assert ref.shape == (16, 5, 8, 8) and bool(torch.isfinite(ref).all())
    chunks = list(causal.stream(m, noise, cond, null, **_kw(setting)))
    assert [c.index for c in chunks] == [0, 1, 2] and [c.frames for c in chunks] == [(0, 2), (2, 4), (4, 5)]
    assert all(c.video is None and c.latents.dtype == torch.float32 and isinstance(c.ready, torch.cuda.Event) for c in chunks)
    assert torch.equal(torch.cat([c.wait().latents for c in chunks], 1), ref)
    assert m._causal_chunks is None


@pytest.mark.parametrize("overlap", [False, True], ids=["main-stream", "overlap"])
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_video_equals_decode_of_the_sampled_clip(causal, setting, overlap):
    m, cond, null, noise, _, vae = _setup()
    ref, video = _reference(causal, setting)
    assert video.shape == (3, 17, 64, 64)
    lat, vid = [], []
    for c in causal.stream(m, noise, cond, null, vae=vae, overlap=overlap, **_kw(setting)):
        c.wait()
        lat.append(c.latents)
        vid.append(c.video)
    assert [v.shape[1] for v in vid] == [5, 8, 4]
    assert torch.equal(torch.cat(lat, 1), ref)
    assert torch.equal(torch.cat(vid, 1), video)
    torch.cuda.synchronize()
    assert m._causal_chunks is None


@pytest.mark.parametrize("overlap", [False, True], ids=["main-stream", "overlap"])
def test_uint8_video_is_the_torch_rule_on_the_float_video(causal, overlap):
    m, cond, null, noise, _, vae = _setup()
    _, video = _reference(causal, "unbounded")
    vid = [c.wait().video for c in causal.stream(m, noise, cond, null, vae=vae, output="uint8", overlap=overlap,
                                                 **_kw("unbounded"))]
    assert [tuple(v.shape) for v in vid] == [(5, 64, 64, 3), (8, 64, 64, 3), (4, 64, 64, 3)]
    want = ((video.permute(1, 2, 3, 0).clamp(-1, 1) + 1) / 2 * 255).to(torch.uint8)
    assert torch.equal(torch.cat(vid, 0), want)


@pytest.mark.parametrize("overlap", [False, True], ids=["main-stream", "overlap"])
def test_closing_the_generator_restores_the_models_setting(causal, overlap):
    m, cond, null, noise, _, vae = _setup()
    ref, video = _reference(causal, "unbounded")
    m.set_causal_chunks(1)
    before = m._causal_chunks
    try:
        gen = causal.stream(m, noise, cond, null, vae=vae, overlap=overlap, **_kw("unbounded"))
        assert m._causal_chunks == before                              # nothing ran yet
        first = next(gen).wait()
        assert m._causal_chunks != before                              # suspended under the rollout's setting
        assert first.index == 0 and torch.equal(first.latents, ref[:, :2]) and torch.equal(first.video, video[:, :5])
        gen.close()
        assert m._causal_chunks == before
        torch.cuda.synchronize()
    finally:
        m._causal_chunks = None
