"""What clipping the global gradient norm costs an optimizer step of the 1.3B model (omnihuman_trainer.py:349-356:
clip_grad_norm_(model.parameters(), max_grad_norm = 1.0), then optimizer.step()), on three routes in one process:

  (a) torch.nn.utils.clip_grad_norm_ + optim.AdamW.step()      the only route there was before the fused clip
  (b) optim.clip_grad_norm_          + optim.AdamW.step()      two launches for the clip (norm, scale)
  (c) optim.AdamW(max_grad_norm=1.0).step()                    one launch more than an unclipped step

each with gradients that get clipped and with gradients that do not.  Random gradients on the model's parameter
shapes, no forward (about 40 GB: parameters, gradients and their pristine copy, the moments of two optimizers, the bf16
operand copies); HIP events around every repetition, 5 warm-ups, median of 20; the gradients are restored from the
pristine copy before every repetition, outside the timed region (routes (a) and (b) scale them in place).  GPU box:
    python tools/grad_clip_probe.py > profiles/grad_clip_probe.txt
"""
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

PKG = "omnihuman-1-hack_amd"
WARMUP, REPS, MAX_NORM = 5, 20, 1.0


def main():
    dev = torch.device("cuda", 0)
    optim = importlib.import_module(PKG + ".optim")
    mt = importlib.import_module(PKG + ".wan.modules.model_train")
    model = bench.build_model(dev).train().requires_grad_(True)
    params = [p for p in model.parameters()]
    mt.TrainPacks.of(model).refresh(model)          # the operand copies of a training step: AdamW takes its pack kernel
    gen = torch.Generator(device=dev).manual_seed(11)
    pristine = [torch.randn(p.shape, device=dev, generator=gen) for p in params]
    for p in params:
        p.grad = torch.empty_like(p)
    grads = [p.grad for p in params]
    numel = sum(p.numel() for p in params)
    plain = optim.AdamW(params, lr=5e-6, weight_decay=0.01)
    fused = optim.AdamW(params, lr=5e-6, weight_decay=0.01, max_grad_norm=MAX_NORM)

    def route_a():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        plain.step()

    def route_b():
        optim.clip_grad_norm_(params, MAX_NORM)
        plain.step()

    def route_c():
        fused.step()

    def route_0():
        plain.step()

    routes = (("(0) AdamW.step() alone, no clip", route_0),
              ("(a) torch clip_grad_norm_ + AdamW.step()", route_a),
              ("(b) optim.clip_grad_norm_ + AdamW.step()", route_b),
              ("(c) AdamW(max_grad_norm=1.0).step()", route_c))
    print(f"grad_clip_probe: {len(params)} tensors, {numel} elements ({4 * numel / 1e9:.2f} GB of fp32 gradients), "
          f"max_norm {MAX_NORM}, {WARMUP} warm-ups, median of {REPS} (ms; min and max beside it)")
    print(f"AdamW kernel: {'adamw_pack (operand copies written by the step)' if mt.pack_entry_of(max(params, key=lambda p: p.numel())) else 'adamw_multi'}")
    med = {}
    for case, scale in (("clipped", 1e-3), ("unclipped", 1e-6)):
        torch._foreach_mul_(pristine, 1e-3)                                      # 1e-3, then 1e-6 of the unit normal
        assert abs(pristine[0].std().item() / scale - 1) < 0.5
        torch._foreach_copy_(grads, pristine)
        norm = float(torch.nn.utils.get_total_norm(grads)) if hasattr(torch.nn.utils, "get_total_norm") else \
            float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))
        print(f"-- gradients {case}: norm {norm:.4g} against max_norm {MAX_NORM}")
        for name, fn in routes:
            times = []
            for it in range(WARMUP + REPS):
                torch._foreach_copy_(grads, pristine)
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn()
                e.record()
                e.synchronize()
                if it >= WARMUP:
                    times.append(s.elapsed_time(e))
            med[(case, name[:3])] = statistics.median(times)
            print(f"   {name:<44} {statistics.median(times):8.3f}   [{min(times):.3f} .. {max(times):.3f}]")
        if fused.grad_norm is not None:
            print(f"   norm on the device after (c): {float(fused.grad_norm):.6g}")
    # "one launch": omh_scale_multi with a coefficient of 1 (every workgroup returns at once), 20 back to back
    ops = importlib.import_module(PKG + ".ops")
    rows, table, chunks, _ = next(iter(optim._CLIP_TABLES.values()))
    one = torch.ones(1, device=dev)
    ops.scale_multi(table, len(rows), chunks, one)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(20):
        ops.scale_multi(table, len(rows), chunks, one)
    e.record()
    e.synchronize()
    launch = s.elapsed_time(e) / 20
    print(f"one omh_scale_multi launch at coefficient 1 ({chunks} workgroups that return at once): {launch:.4f} ms")
    for case in ("clipped", "unclipped"):
        a, b, c, z = (med[(case, k)] for k in ("(a)", "(b)", "(c)", "(0)"))
        print(f"{case}: clip costs (a) {a - z:.3f}  (b) {b - z:.3f}  (c) {c - z:.3f} ms over the step alone; "
              f"(c) faster than (a): {'yes' if c < a else 'NO'}")
    b, c = med[("unclipped", "(b)")], med[("unclipped", "(c)")]
    print(f"unclipped: (b) no slower than (c) + one launch ({launch:.4f} ms): {'yes' if b <= c + launch else 'NO'} "
          f"((b) - (c) = {b - c:+.3f} ms)")


if __name__ == "__main__":
    main()
