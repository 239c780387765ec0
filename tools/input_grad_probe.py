"""What the input gradients of WanModel cost (profiles/input_grad_probe.txt): the 4-clip training step of the 1.3B model
with and without ``x.requires_grad``, a frozen model's forward + backward against a trainable one's, and
omh_patchify_bwd alone at the i2v latent [36, 21, 60, 104] against the bytes it moves.

    python tools/input_grad_probe.py [clips]
"""
import importlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

ops = importlib.import_module("omnihuman-1-hack_amd.ops")
dev = torch.device("cuda", 0)
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4


def timed(fn, warmup=3, reps=10):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    model = bench.build_model(dev)
    model.reference_ffn_freeze, model.use_checkpoint, model.checkpoint_policy = True, True, "auto"
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn(B, 16, 1, 60, 104, device=dev, generator=g)
    ctx = [torch.randn(512, 4096, device=dev, generator=g) for _ in range(B)]
    tgt = torch.randn(B, 16, 1, 60, 104, device=dev, generator=g)
    tt = torch.full((B,), 999.0, device=dev)

    def step(x_grad):
        xs = [u.detach().requires_grad_(x_grad) for u in x]
        out = model(xs, t=tt, context=ctx, seq_len=1560)
        sum(torch.nn.functional.mse_loss(a, b) for a, b in zip(out, tgt)).backward()
        model.zero_grad(set_to_none=True)

    model.train().requires_grad_(True)
    rows = []
    # interleaved A / B / A: the box drifts by a few per cent over a minute
    for name, fn in (("trainable, x plain", lambda: step(False)), ("trainable, x.requires_grad", lambda: step(True)),
                     ("trainable, x plain (again)", lambda: step(False))):
        rows.append((name,) + timed(fn))
    model.eval().requires_grad_(False)
    rows.append(("frozen, x.requires_grad", ) + timed(lambda: step(True)))
    print(f"forward + backward, {B} clips [16,1,60,104], 1.3B, ms (median, min, max of 10)")
    for name, med, lo, hi in rows:
        print(f"  {name:32s} {med:8.2f} {lo:8.2f} {hi:8.2f}")
    # ---- the adjoint of patchify alone
    C, F, H, W = 36, 21, 60, 104
    n, Kp = F * (H // 2) * (W // 2), C * 4
    dtok = torch.randn(n, Kp, device=dev, generator=g)
    o0, o1 = torch.empty(16, F, H, W, device=dev), torch.empty(20, F, H, W, device=dev)
    med, lo, hi = timed(lambda: ops.patchify_bwd(dtok, (F, H // 2, W // 2), (1, 2, 2), (C, F, H, W), c_split=16, out=(o0, o1)),
                        warmup=5, reps=20)
    gb = (dtok.numel() + o0.numel() + o1.numel()) * 4 / 1e9
    print(f"omh_patchify_bwd [36,21,60,104] split 16|20: {med * 1e3:.1f} us median ({lo * 1e3:.1f} min), "
          f"{gb * 1e3:.1f} MB moved, {gb / (lo * 1e-3):.0f} GB/s at the minimum")


if __name__ == "__main__":
    main()
