"""What a LoRA training step costs against full fine-tuning (profiles/lora_step_probe.json): the 1.3B model at the
bench's training shapes (``clips`` x [16,1,60,104], rank 32), forward + backward + optim.AdamW step, for
  * the full step (every parameter trainable),
  * the frozen-base step with adapters on the attention projections,
  * the same with adapters on all targets,
interleaved (the box drifts by a few per cent over a minute), with ``torch.cuda.max_memory_allocated`` of each; and the
skinny adapter-gradient kernels alone at M = 6 240, in = out = 1 536, rank 32 beside the ``_wgrad`` launch they replace.

    python tools/lora_probe.py [clips] [out.json]
"""
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

ops = importlib.import_module("omnihuman-1-hack_amd.ops")
lora = importlib.import_module("omnihuman-1-hack_amd.lora")
optim = importlib.import_module("omnihuman-1-hack_amd.optim")
dev = torch.device("cuda", 0)
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
OUT = sys.argv[2] if len(sys.argv) > 2 else None
RANK = 32
ATTN = tuple(t for t in lora.DEFAULT_TARGETS if "attn" in t)


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
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def main():
    g = torch.Generator(device=dev).manual_seed(7)
    x = [u for u in torch.randn(B, 16, 1, 60, 104, device=dev, generator=g)]
    ctx = [torch.randn(512, 4096, device=dev, generator=g) for _ in range(B)]
    tgt = torch.randn(B, 16, 1, 60, 104, device=dev, generator=g)
    tt = torch.full((B,), 999.0, device=dev)
    record = {"clips": B, "rank": RANK, "device": torch.cuda.get_device_name(0), "cases": {}}

    def case(name, targets):
        model = bench.build_model(dev).train()
        model.reference_ffn_freeze, model.use_checkpoint, model.checkpoint_policy = True, True, "auto"
        if targets is None:
            params = [p for p in model.requires_grad_(True).parameters()]
        else:
            params = lora.add_lora(model, RANK, targets=targets)
        opt = optim.AdamW(params, lr=1e-5)

        def step():
            out = model(x, t=tt, context=ctx, seq_len=1560)
            sum(torch.nn.functional.mse_loss(a, b) for a, b in zip(out, tgt)).backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        rows = []
        for _ in range(2):                                    # two passes per case, the cases interleaved by the caller
            rows.append(timed(step, warmup=3, reps=8))
        record["cases"].setdefault(name, []).append({
            "timing": rows, "trainable_elements": sum(p.numel() for p in params),
            "max_memory_allocated": torch.cuda.max_memory_allocated(dev), "allocated_before": base})
        print(name, rows[-1], f"peak {torch.cuda.max_memory_allocated(dev) / 2 ** 30:.2f} GiB", flush=True)
        del model, opt, params
        torch.cuda.empty_cache()

    for _ in range(2):                                        # A / B / C / A / B / C
        case("full", None)
        case("lora_attention", ATTN)
        case("lora_all", lora.DEFAULT_TARGETS)
    # ---- the skinny kernels alone, beside the weight-gradient GEMM of the same Linear
    M, d = 1560 * B, 1536
    xx = torch.randn(M, d, device=dev, generator=g).to(torch.bfloat16)
    dy = torch.randn(M, d, device=dev, generator=g).to(torch.bfloat16)
    A, Bm = torch.randn(RANK, d, device=dev, generator=g), torch.randn(d, RANK, device=dev, generator=g)
    dA, dB = torch.empty_like(A), torch.empty_like(Bm)
    dW = torch.empty(d, d, device=dev)
    record["kernels"] = {
        "shape": {"M": M, "in": d, "out": d, "rank": RANK},
        "omh_lora_grads": timed(lambda: ops.lora_grads(xx, dy, A, Bm, 1.0, dA, dB), warmup=5, reps=20),
        "omh_gemm_bf16_tn (dW)": timed(lambda: ops.gemm_tn(dy, xx, out=dW), warmup=5, reps=20)}
    print(json.dumps(record["kernels"], indent=1))
    if OUT:
        with open(OUT, "w") as fh:
            json.dump(record, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
