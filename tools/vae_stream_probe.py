"""Streaming VAE decode and the streamed rollout at 480 x 832 on one MI355X.

    python tools/vae_stream_probe.py [--out profiles/vae_stream_probe.txt]

Without ``--step`` the steps below run one after the other, each as a fresh child process under its own
``timeout -k 10`` and only while the one before it ended well (the chain stops at the first failure; what has been
measured until then is still written).  One JSON line per step, also written to --out.

  vae_bf16 / vae_fp32   random-init WanVAE in the bf16 / fp32-faithful mode, a [16, 21, 60, 104] latent:
      ``decode_ms`` / ``decode_frames_per_s``: whole-clip ``decode`` (81 frames), the yardstick, in the same process;
      ``first_push_ms``: the first push (3 latent frames -> 9 frames) of a stream whose buffers exist (after ``reset()``);
      ``steady_push_ms``: the median of the six later pushes (3 latent frames -> 12 frames); ``*_frames_per_s`` of both, of
      the whole stream (81 frames over the seven pushes) and that over ``decode``; ``steady_push_u8_ms``: the same push
      with ``output="uint8"``; ``state_bytes`` / ``history_bytes``; ``equal_bits``: the streamed frames equal ``decode``'s.
  u8   omh_cl_to_u8 on 12 frames [12, 480, 832, 3] (57.5 MB read, 14.4 MB written) against a device copy that moves the same
      71.9 MB (``torch.Tensor.copy_`` of 35.9 MB), both over 8 rotating buffer sets (> 256 MiB, past the Infinity Cache),
      alternating: ``*_us`` the median of --reps runs, GB/s from the byte counts, and the kernel's rate over the copy's.
  rollout   Wan2.1-T2V-1.3B random init, 21 latent frames, ``causal.stream(frames_per_chunk=3, left_chunks=1,
      sink_chunks=1, rolling=True)``, a 4-step UniPC scheduler, the bf16 VAE, uint8 frames; the consumer blocks on every
      chunk's ``ready``.  ``first_frame_ms``: from the call to the first chunk's frames being ready; ``chunk_period_ms``: the
      mean distance of the later chunks' ready times; ``total_ms``; with ``overlap`` off and on (the second of two runs each).
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "omnihuman-1-hack_amd"
STEPS = (("vae_bf16", 300), ("vae_fp32", 420), ("u8", 180), ("rollout", 480))       # (name, seconds of its time limit)


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def step_vae(dtype_name):
    import torch
    vae_mod = importlib.import_module(PKG + ".wan.modules.vae")
    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float
    vae = vae_mod.WanVAE(vae_pth=None, device="cuda", dtype=dtype)
    g = torch.Generator(device="cuda").manual_seed(0)
    z = torch.randn(16, 21, 60, 104, device="cuda", generator=g)
    parts = [(f, 3) for f in range(0, 21, 3)]
    vae.decode([z[:, :2]])
    whole = vae.decode([z])[0]
    torch.cuda.synchronize()
    decode_ms = statistics.median(_timed(lambda: vae.decode([z]))[0] for _ in range(3))
    s = vae.decode_stream()
    got = [s.push(z[:, f:f + n]) for f, n in parts]                   # the first clip makes the buffers
    equal = bool(torch.equal(torch.cat(got, 1), whole))
    del got, whole
    firsts, steadies = [], []
    for _ in range(2):
        s.reset()
        torch.cuda.synchronize()
        ms = [_timed(lambda: s.push(z[:, f:f + n]))[0] for f, n in parts]
        firsts.append(ms[0])
        steadies += ms[1:]
    first, steady, total = statistics.median(firsts), statistics.median(steadies), statistics.median(firsts) + sum(steadies) / 2
    row = {"step": "vae_" + dtype_name, "latent": [16, 21, 60, 104], "push": 3, "decode_ms": round(decode_ms, 1),
           "decode_frames_per_s": round(81e3 / decode_ms, 1), "first_push_ms": round(first, 1),
           "first_push_frames_per_s": round(9e3 / first, 1), "steady_push_ms": round(steady, 1),
           "steady_push_frames_per_s": round(12e3 / steady, 1), "stream_ms": round(total, 1),
           "stream_frames_per_s": round(81e3 / total, 1), "stream_over_decode": round(decode_ms / total, 3),
           "state_bytes": s.state_bytes(), "history_bytes": s.history_bytes(), "equal_bits": equal}
    u = vae.decode_stream(output="uint8")
    ms = [_timed(lambda: u.push(z[:, f:f + n]))[0] for f, n in parts + parts[1:]]
    row["steady_push_u8_ms"] = round(statistics.median(ms[len(parts):]), 1)
    row["peak_memory_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    return row


def step_u8(reps):
    import torch
    ops = importlib.import_module(PKG + ".ops")
    T, H, W, C, sets = 12, 480, 832, 3, 8
    n = T * H * W * C
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(T, H, W, C, device="cuda", generator=g) * 0.7 for _ in range(sets)]
    outs = [torch.empty(T, H, W, C, dtype=torch.uint8, device="cuda") for _ in range(sets)]
    moved = 5 * n                                                     # 4 bytes in, 1 byte out per element
    src = [torch.empty(moved // 2, dtype=torch.uint8, device="cuda").random_(0, 255) for _ in range(sets)]
    dst = [torch.empty_like(b) for b in src]
    want = ((xs[0].clamp(-1, 1) + 1) / 2 * 255).to(torch.uint8)
    ops.cl_to_u8(xs[0], outs[0], 0, C)
    equal = bool(torch.equal(outs[0], want))
    k_us, c_us = [], []
    for i in range(reps + 2):
        j = i % sets
        tk = _timed(lambda: ops.cl_to_u8(xs[j], outs[j], 0, C))[0]
        tc = _timed(lambda: dst[j].copy_(src[j]))[0]
        if i >= 2:                                                    # two warm-up rounds
            k_us.append(tk * 1e3)
            c_us.append(tc * 1e3)
    ku, cu = statistics.median(k_us), statistics.median(c_us)
    return {"step": "u8", "shape": [T, H, W, C], "bytes_moved": moved, "reps": reps, "cl_to_u8_us": round(ku, 1),
            "cl_to_u8_gb_per_s": round(moved / ku / 1e3, 1), "copy_us": round(cu, 1), "copy_gb_per_s": round(moved / cu / 1e3, 1),
            "cl_to_u8_over_copy_rate": round(cu / ku, 3), "spread_us": [round(max(k_us) - min(k_us), 1), round(max(c_us) - min(c_us), 1)],
            "equal_bits": equal}


def step_rollout():
    import torch
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    causal = importlib.import_module(PKG + ".causal")
    vae_mod = importlib.import_module(PKG + ".wan.modules.vae")
    unipc = importlib.import_module(PKG + ".wan.utils.fm_solvers_unipc")
    m = bench.build_model("cuda").eval().requires_grad_(False)
    vae = vae_mod.WanVAE(vae_pth=None, device="cuda", dtype=torch.bfloat16)
    g = torch.Generator(device="cuda").manual_seed(0)
    noise = torch.randn(16, 21, 60, 104, device="cuda", generator=g)
    ctx, null = [torch.randn(77, 4096, device="cuda", generator=g)], [torch.randn(5, 4096, device="cuda", generator=g)]

    def make_scheduler():
        s = unipc.FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
        s.set_timesteps(4, device="cuda", shift=3.0)
        return s
    row = {"step": "rollout", "model": "Wan2.1-T2V-1.3B random init", "latent": [16, 21, 60, 104], "frames_per_chunk": 3,
           "steps": 4, "left_chunks": 1, "sink_chunks": 1, "rolling": True, "vae": "bf16", "output": "uint8"}
    frames = {}
    for overlap in (False, True, False, True):                        # the first run of each is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ready, vids = [], []
        for c in causal.stream(m, noise, ctx, null, frames_per_chunk=3, left_chunks=1, sink_chunks=1, rolling=True,
                               make_scheduler=make_scheduler, guide_scale=5.0, vae=vae, output="uint8", overlap=overlap):
            c.ready.synchronize()
            ready.append((time.perf_counter() - t0) * 1e3)
            vids.append(c.wait().video)
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
        key = "overlap_on" if overlap else "overlap_off"
        frames[key] = torch.cat(vids, 0)
        row[key] = {"first_frame_ms": round(ready[0], 1), "chunk_period_ms": round((ready[-1] - ready[0]) / (len(ready) - 1), 1),
                    "total_ms": round(total, 1), "chunks": len(ready), "frames": int(frames[key].shape[0])}
    row["equal_bits_on_off"] = bool(torch.equal(frames["overlap_on"], frames["overlap_off"]))
    row["period_on_over_off"] = round(row["overlap_on"]["chunk_period_ms"] / row["overlap_off"]["chunk_period_ms"], 3)
    row["peak_memory_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--part", help="(with --step) the file the step's JSON line goes to")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_stream_probe.txt"))
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, ROOT)
        row = {"vae_bf16": lambda: step_vae("bf16"), "vae_fp32": lambda: step_vae("fp32"), "u8": lambda: step_u8(a.reps),
               "rollout": step_rollout}[a.step]()
        line = json.dumps(row)
        print(line, flush=True)
        if a.part:
            with open(a.part, "w") as fh:
                fh.write(line + "\n")
        return 0
    lines = [f"# python tools/vae_stream_probe.py --reps {a.reps}   (one MI355X; 480 x 832, pushes of 3 latent frames; every step a "
             f"process of its own under timeout -k 10)"]
    rc = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name, secs in STEPS:
            part = os.path.join(tmp, name + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(secs), sys.executable, os.path.abspath(__file__), "--step", name,
                                 "--reps", str(a.reps), "--part", part]).returncode
            if rc != 0:                                               # the chain ends here: nothing more is started
                lines.append(f"# step {name} ended with exit status {rc}: the steps behind it were not run")
                break
            lines.append(open(part).read().strip())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
