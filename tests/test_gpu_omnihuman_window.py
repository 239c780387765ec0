"""OmniHuman with frame-aligned condition tokens: ``config["condition_window"] = (back, ahead)`` makes
``OmniHumanWanT2V.training_step`` pass the tokens' latent frames (``condition_frames``) and the window to the backbone.
Loss and adapter gradients against autograd through the fp32 restatement tests/condition_window_ref.py with the adapters of
oracle/omnihuman_oracle.py, set up as test_gpu_omnihuman.py's training-step test (its bounds: loss 1e-2, adapter gradients
2e-2) on latents of 2 frames x 12 tokens (a frame group needs 8)."""
import importlib

import pytest
import torch

import condition_window_ref as CR
from conftest import PKG, rel_rms
from test_gpu_omnihuman import _GateSpy, _StubT2V, _StubVAE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def omni(omh):
    return importlib.import_module(PKG + ".omnihuman_wan_t2v")


def test_training_step_with_a_condition_window(omni, wan_model_mod, monkeypatch):
    from oracle import detgen, make_golden, omnihuman_oracle as OH, wan_dit_oracle as O
    causal = importlib.import_module(PKG + ".causal")
    ops = importlib.import_module(PKG + ".ops")
    cfg = O.DiTConfig(model_type="t2v", in_dim=16, num_layers=2, **make_golden.TINY)
    dsd = O.synth_state_dict(cfg, "omni/dit")
    dsd["head.head.weight"] = torch.from_numpy(detgen.uniform("omni/dit/headw", tuple(dsd["head.head.weight"].shape),
                                                              -0.08, 0.08))
    kw = dict(model_dim=256, num_frames=5, audio_dim=32, pose_keypoints=6)
    osd = make_golden.omni_state_dict("omni/sd", pose_prefix="pose_processor.", widths=(128, 256), **kw)
    audio, pose = make_golden.omni_inputs("omni/in", **kw)
    frames = torch.from_numpy(detgen.normalish("omni/win/frames", (2, 16, 2, 8, 6)))    # 2 latent frames of 4 x 3 tokens
    noise = torch.from_numpy(detgen.normalish("omni/win/noise", (2, 16, 2, 8, 6)))
    ctx = torch.from_numpy(detgen.normalish("omni/ctx", (20, 64)))
    t = torch.tensor([0.3, 0.7])
    S, TPF, window = 24, 12, (1, 0)

    def product(config_extra):
        dit = wan_model_mod.WanModel(num_layers=2, **make_golden.TINY)
        dit.load_state_dict(dsd)
        dit = dit.cuda().train()
        m = omni.OmniHumanWanT2V(dict(num_frames=5, num_keypoints=6, model_dim=256, audio_dim=32, **config_extra), device_id=0,
                                 wan_t2v=_StubT2V(dit, _StubVAE(None)))
        m.load_state_dict(osd, strict=False)
        return m, dit

    # ---- the product with a window (the pose stack's ReLU decisions are recorded for the oracle)
    spy = _GateSpy(omni, monkeypatch)
    m, dit = product({"condition_window": window})
    loss = m.training_step(frames, {"text": ctx, "audio_features": audio, "pose_heatmaps": pose}, t, noise=noise)
    loss.backward()
    # ---- the restatement: 4 audio pairs and 5 pose tokens of 5 video frames on 2 latent frames
    token_frames = m.condition_frames(4, 5)
    assert token_frames.tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1]
    d_o = {k: v.clone().requires_grad_(True) for k, v in dsd.items()}
    o_o = {k: v.clone().requires_grad_(True) for k, v in osd.items()}
    tok = OH.condition_tokens(o_o, OH.process_audio(o_o, audio), OH.process_pose(o_o, pose, gates=spy.gates(pose.shape[0])))
    assert tok.shape[1] == token_frames.shape[0]
    tt = t.view(-1, 1, 1, 1, 1)
    noisy = (1 - tt) * frames + tt * noise
    vis = causal.condition_window_visible(2, token_frames, cfg.text_len, *window).repeat_interleave(TPF, 0)
    pred = torch.stack(CR.forward(d_o, cfg, list(noisy), t[:, None].expand(2, 2), [ctx, ctx], S, extra_tokens=tok,
                                  cross_mask=vis))
    lo = torch.mean((pred - frames) ** 2 * (1 - tt))
    lo.backward()
    with torch.no_grad():                                   # the window matters here: the unwindowed loss is another one
        plain = torch.stack(CR.forward(d_o, cfg, list(noisy), t[:, None].expand(2, 2), [ctx, ctx], S, extra_tokens=tok))
        lp = torch.mean((plain - frames) ** 2 * (1 - tt))
    print(f"loss {loss.item():.6f} restatement {lo.item():.6f} (unwindowed {lp.item():.6f})")
    assert abs(loss.item() - lo.item()) < 1e-2 * lo.item()
    bad, worst = [], 0.0
    for name, prm in m.named_parameters():
        if not name.startswith(("audio_processor", "pose_fc")):
            continue
        assert prm.grad is not None, name
        err = rel_rms(prm.grad, o_o[name].grad)
        worst = max(worst, err)
        if err > 2e-2:
            bad.append((name, err))
    print(f"[measured] windowed OmniHuman training step, audio MLP and pose_fc gradients vs the restatement: worst {worst:.3e}")
    assert not bad, bad
    # ---- without the key: the bits of the call the method made before it knew of windows
    was = ops.set_deterministic(None)
    ops.set_deterministic(True)
    try:
        m0, dit0 = product({})
        got = m0.training_step(frames, {"text": ctx, "audio_features": audio, "pose_heatmaps": pose}, t, noise=noise)
        m1, dit1 = product({})
        tokens = m1.condition_tokens(m1.process_audio(audio.cuda()), m1.process_pose(pose.cuda()))
        pred = torch.stack(dit1(noisy.cuda(), t.cuda(), context=[ctx.cuda()] * 2, seq_len=S, extra_conditions=tokens))
        want = torch.mean((pred - frames.cuda()) ** 2 * (1 - tt.cuda()))
        assert torch.equal(got, want)
        assert not torch.equal(got, loss.detach())
    finally:
        ops.set_deterministic(was)
