"""What FP8 block-scaled AdamW moments (optim.AdamW(moments="fp8")) cost and save on one MI355X:

  (A) the optimizer launch alone over the 1.3B model's trainable tensors, moments="fp32" and "fp8", with the bytes each
      moves computed from the shapes and the resulting TB/s;
  (B) the one-clip and four-clip 1.3B training step (bench.py's config-3 step) in both modes: time, and — each mode alone
      in memory — torch.cuda.max_memory_allocated;
  (C) one one-clip step of a random-init 14B model with moments="fp8" and activations recomputed: peak memory, or the text
      of the allocation error.  An out-of-memory error is a finding, not a failure.  Runs in a child process of its own.

Device events around every repetition; warm-up first; the fp32 and the fp8 launches alternate in one process; three
rounds, the median of each, and the median of the three with their spread.  GPU box:
    python tools/adamw8_probe.py            (writes profiles/adamw8_probe.txt)
"""
import argparse
import gc
import importlib
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

PKG = "omnihuman-1-hack_amd"
ROUNDS, WARMUP, REPS = 3, 3, 10
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def alternate(fns, reps=REPS, warmup=WARMUP, rounds=ROUNDS):
    """{name: (median of the rounds' medians, smallest, largest round median)} with the routes taking turns."""
    per_round = {k: [] for k in fns}
    for _ in range(rounds):
        times = {k: [] for k in fns}
        for it in range(warmup + reps):
            for k, fn in fns.items():
                t = timed(fn)
                if it >= warmup:
                    times[k].append(t)
        for k in fns:
            per_round[k].append(statistics.median(times[k]))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in per_round.items()}


def bytes_moved(optim, mt, opt, params):
    """Bytes one step of ``opt`` reads and writes, from the shapes: p and g read, p written, the moments read and written
    (fp32: 4 + 4 each way; fp8: 1 + 1 and the two block scales), and the bf16 / fp32 operand copies written."""
    total = 0
    for p in params:
        n = p.numel()
        st = opt.state[p]
        total += 12 * n                                              # p, g in; p out
        if "exp_avg_q" in st:
            total += 2 * (2 * n + 2 * 4 * st["exp_avg_scale"].numel())
        else:
            total += 16 * n
        ent = mt.pack_entry_of(p)
        if ent is not None:
            pr = ent[0].rows[ent[1]]
            total += 4 * n if pr[8] == 1 else 2 * n * (int(pr[1] != 0) + int(pr[2] != 0))
    return total


def part_optimizer_and_steps(dev):
    optim = importlib.import_module(PKG + ".optim")
    mt = importlib.import_module(PKG + ".wan.modules.model_train")
    trainer = importlib.import_module(PKG + ".trainer")
    model = bench.build_model(dev).train().requires_grad_(True)
    model.use_checkpoint, model.checkpoint_policy = True, "auto"
    params = list(model.parameters())
    numel = sum(p.numel() for p in params)
    kw = dict(lr=5e-6, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    gen = torch.Generator(device=dev).manual_seed(7)

    def batch(bsz):
        return (torch.randn(bsz, 16, 1, 60, 104, device=dev, generator=gen),
                torch.randn(bsz, 512, 4096, device=dev, generator=gen),
                torch.randn(bsz, 16, 1, 60, 104, device=dev, generator=gen))

    # ---- (B, memory) each mode alone: the optimizer and its state exist only while its peak is taken
    say("== (B) 1.3B training step (reference quirks on, use_checkpoint=True, policy auto): peak memory, each mode alone")
    peaks = {}
    for bsz in (1, 4):
        b = batch(bsz)
        for mode in ("fp32", "fp8"):
            opt = optim.AdamW(params, moments=mode, **kw)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            for _ in range(2):
                trainer.forward_backward(b, model)
                opt.step()
                opt.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            state = sum(t.numel() * t.element_size() for st in opt.state.values() for k, t in st.items() if k != "step")
            peaks[(bsz, mode)] = torch.cuda.max_memory_allocated(dev)
            say(f"   {bsz} clip(s), moments={mode:<5} max_memory_allocated {peaks[(bsz, mode)] / 2**30:8.2f} GiB   "
                f"optimizer state {state / 2**30:6.2f} GiB ({state / numel:.3f} B per weight of the model)")
            del opt
            for p in params:
                p.__dict__.pop("_omh_moments_allocated", None)
            gc.collect()
            torch.cuda.empty_cache()
        say(f"   {bsz} clip(s): fp8 peak is {(peaks[(bsz, 'fp32')] - peaks[(bsz, 'fp8')]) / 2**30:.2f} GiB below fp32")

    # ---- (B, time) both optimizers alive, the two routes taking turns
    opts = {m: optim.AdamW(params, moments=m, **kw) for m in ("fp32", "fp8")}
    say(f"== (B) the same step, time in ms: median of {ROUNDS} rounds (each the median of {REPS} after {WARMUP} warm-ups), "
        "[smallest .. largest round]; fp32 and fp8 steps alternate")
    for bsz in (1, 4):
        b = batch(bsz)

        def step(opt):
            trainer.forward_backward(b, model)
            opt.step()
            opt.zero_grad(set_to_none=True)
        res = alternate({m: (lambda o=o: step(o)) for m, o in opts.items()}, reps=6, warmup=2)
        for m, (med, lo, hi) in res.items():
            say(f"   {bsz} clip(s), moments={m:<5} {med:9.3f}   [{lo:.3f} .. {hi:.3f}]")
        say(f"   {bsz} clip(s): fp8 - fp32 = {res['fp8'][0] - res['fp32'][0]:+.3f} ms")

    # ---- (A) the optimizer launch alone, on the gradients of the last backward
    trainer.forward_backward(batch(1), model)
    stepped = [p for p in params if p.grad is not None]
    res = alternate({m: o.step for m, o in opts.items()})
    say(f"== (A) optimizer step alone over {len(stepped)} tensors with a gradient, {sum(p.numel() for p in stepped)} elements "
        f"(of {numel}): ms as above, bytes from the shapes")
    for m, (med, lo, hi) in res.items():
        nbytes = bytes_moved(optim, mt, opts[m], stepped)
        say(f"   moments={m:<5} {med:8.3f}   [{lo:.3f} .. {hi:.3f}]   {nbytes / 1e9:7.2f} GB "
            f"({nbytes / sum(p.numel() for p in stepped):.2f} B per weight)   {nbytes / med / 1e9:.2f} TB/s")
    n8 = sum(p.numel() for p in stepped if "exp_avg_q" in opts["fp8"].state[p])
    say(f"   8-bit state on {n8} elements ({100.0 * n8 / sum(p.numel() for p in stepped):.2f} % of those stepped); launches per "
        f"fp8 step: {sum(1 for k in opts['fp8']._tables if 'norm' not in k)}")


def part_14b(dev):
    optim = importlib.import_module(PKG + ".optim")
    trainer = importlib.import_module(PKG + ".trainer")
    model_mod = importlib.import_module(PKG + ".wan.modules.model")
    cfgs = importlib.import_module(PKG + ".wan.configs")
    say("== (C) random-init 14B (t2v_14B), one clip [16, 1, 60, 104], moments=\"fp8\", use_checkpoint=True, policy always")
    stage = "building the model"
    try:
        torch.manual_seed(1234)
        with torch.device(dev):
            model = model_mod.WanModel(**cfgs.dit_kwargs(cfgs.t2v_14B))
            torch.nn.init.xavier_uniform_(model.head.head.weight)
        model.train().requires_grad_(True)
        model.reference_ffn_freeze = False                           # every parameter trained: the memory question
        model.use_checkpoint, model.checkpoint_policy = True, "always"
        numel = sum(p.numel() for p in model.parameters())
        say(f"   {numel} parameters; after the build: {torch.cuda.memory_allocated(dev) / 2**30:.2f} GiB allocated")
        opt = optim.AdamW(model.parameters(), lr=5e-6, weight_decay=0.01, moments="fp8")
        gen = torch.Generator(device=dev).manual_seed(7)
        b = (torch.randn(1, 16, 1, 60, 104, device=dev, generator=gen), torch.randn(1, 512, 4096, device=dev, generator=gen),
             torch.randn(1, 16, 1, 60, 104, device=dev, generator=gen))
        for it in range(2):
            stage = f"step {it + 1}: forward + backward"
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            loss = trainer.forward_backward(b, model, reference_loss_quirk=False)
            stage = f"step {it + 1}: optimizer"
            opt.step()
            opt.zero_grad(set_to_none=True)
            e.record()
            e.synchronize()
            say(f"   step {it + 1}: {s.elapsed_time(e):.1f} ms, loss {float(loss):.6f}, max_memory_allocated "
                f"{torch.cuda.max_memory_allocated(dev) / 2**30:.2f} GiB")
        state = sum(t.numel() * t.element_size() for st in opt.state.values() for k, t in st.items() if k != "step")
        say(f"   optimizer state {state / 2**30:.2f} GiB ({state / numel:.3f} B per weight); it fits: peak "
            f"{torch.cuda.max_memory_allocated(dev) / 2**30:.2f} GiB of {torch.cuda.get_device_properties(dev).total_memory / 2**30:.0f}")
    except torch.OutOfMemoryError as exc:
        say(f"   DOES NOT FIT ({stage}); peak before the error {torch.cuda.max_memory_allocated(dev) / 2**30:.2f} GiB; "
            f"the allocator said: {str(exc).splitlines()[0]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adamw8_probe.txt"))
    ap.add_argument("--part", default="all", choices=("all", "14b"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.part == "14b":
        part_14b(dev)
        return
    say(f"adamw8_probe: {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    part_optimizer_and_steps(dev)
    gc.collect()
    torch.cuda.empty_cache()
    # a process of its own: nothing of the 1.3B run is in its memory
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", "14b"], capture_output=True, text=True)
    body = [ln for ln in child.stdout.splitlines() if ln.startswith(("==", "   "))]
    for ln in body:
        say(ln)
    if child.returncode != 0:
        say(f"   the 14B child process ended with status {child.returncode}: {child.stderr.strip().splitlines()[-1:]}")
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
