"""The pinned attention sink of an unbounded rollout: what re-rotating the sink keys costs per chunk at the 1.3B geometry,
and the errors the tests print.

    python tools/pinned_sink_probe.py [--reps 20] [--out profiles/pinned_sink_probe.txt]

Kernel level (one JSON line): one chunk advance of ``causal.sample(pin_sink=True)`` on Wan2.1-T2V-1.3B at 480 x 832 with
3 latent frames per chunk and one sink chunk — S Ct = 4 680 key rows of dim 1 536, 30 layers, two caches (conditional and
unconditional): 60 launches of ``ops.rope_shift_frames`` from the pristine copy into the live rows of a cache with
W = 6 (batch stride = 8 chunks).  ``shift_us`` is the time of all 60, ``copy_us`` that of 60 device-to-device copies of the
same rows between the same tensors (``Tensor.copy_``), both in this process: HIP events around --reps repetitions after 5
warm-ups, the median of three rounds.  ``gbps`` counts the bytes read plus the bytes written.  No time was fixed in advance;
the chunk period this hides under is about 300 ms.  ``shift_err`` is the worst |error| / bound of the kernel at these rows
for delta in (0, 1, 3, 1000, 10^6), bound = 2^-8 |y| + 2^-20 hypot(x0, x1) against fp64 (tests/test_gpu_rope_shift.py).

Model level (one JSON line): the tiny model and the periodic clip of tests/test_gpu_pinned_sink_model.py at (fpc, W, S, F) =
(1, 1, 1, 12) — rel-RMS of chunks 4..8 against chunk 11 with the sink pinned and with absolute positions, on the GPU and
in the fp32 restatement, the pinned rollout against the restatement, and one chunk at frame 5 000 against frame 0.
Reported, not gated."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "omnihuman-1-hack_amd"
ops = importlib.import_module(PKG + ".ops")
causal = importlib.import_module(PKG + ".causal")
ROWS, DIM, LAYERS, CACHES, SLOTS = 4680, 1536, 30, 2, 8


def _time_us(fn, reps):
    for _ in range(5):
        fn()
    rounds = []
    for _ in range(3):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        e.synchronize()
        rounds.append(1000.0 * s.elapsed_time(e) / reps)
    return round(statistics.median(rounds), 1), round(max(rounds) - min(rounds), 1)


def kernel_level(reps):
    import pinned_sink_ref as PR
    g = torch.Generator(device="cuda").manual_seed(0)
    n = LAYERS * CACHES
    pristine = [torch.randn(1, ROWS, DIM, device="cuda", generator=g).to(torch.bfloat16) for _ in range(n)]
    live = [torch.zeros(1, SLOTS * ROWS, DIM, dtype=torch.bfloat16, device="cuda") for _ in range(n)]

    def shift():
        for p, k in zip(pristine, live):
            ops.rope_shift_frames(p, k[:, :ROWS], 3)

    def copy():
        for p, k in zip(pristine, live):
            k[:, :ROWS].copy_(p)
    nbytes = 2 * n * ROWS * DIM * 2
    row = {"level": "kernels", "rows": ROWS, "dim": DIM, "launches": n, "bytes_moved": nbytes}
    row["shift_us"], row["shift_spread_us"] = _time_us(shift, reps)
    row["copy_us"], row["copy_spread_us"] = _time_us(copy, reps)
    row["shift_gbps"] = round(nbytes / row["shift_us"] / 1e3, 1)
    row["copy_gbps"] = round(nbytes / row["copy_us"] / 1e3, 1)
    src = pristine[0][:, :1000].contiguous()
    errs = {}
    for delta in (0, 1, 3, 1000, 10 ** 6):
        y, rotated, hyp = PR.shift_exact(src.cpu(), delta)
        got = ops.rope_shift_frames(src, None, delta).cpu()
        ratio = (got.double() - y).abs() / (2.0 ** -8 * y.abs() + 2.0 ** -20 * hyp)
        errs[str(delta)] = round(float(ratio[rotated].max()), 4)
    row["shift_err_over_bound"] = errs
    return row


def model_level():
    import pinned_sink_ref as PR
    import test_gpu_pinned_sink_model as T
    from conftest import rel_rms
    model_mod = importlib.import_module(PKG + ".wan.modules.model")
    fpc, W, S, F = T.PERIODIC
    pinned, plain = T._periodic(model_mod, causal, True), T._periodic(model_mod, causal, False)
    ref_p, ref_u = PR.periodic_restatement(causal, True, F), PR.periodic_restatement(causal, False, F)
    # one chunk alone in its cache at frame 5 000 (past the rotary table) against the same chunk at frame 0
    m = T._model(model_mod)
    x = [u.cuda() for u in T._random_clip(2)[0]]
    one = lambda fo: m.forward_chunk(x, torch.tensor([700., 300.], device="cuda"), T._cuda(T.MC.case()[2]),
                                     causal.KVCache(m, 2, 2 * T.TPF, "cuda"), frame_offset=fo, commit=False)
    base, far = one(0), one(5000)
    spread = lambda out: [float(f"{max(rel_rms(out(I, b), out(11, b)) for b in range(2)):.2e}") for I in range(4, 9)]
    return {"level": "model", "model": "tiny t2v, 2 layers, 56 tokens per frame, B = 2", "setting": [fpc, W, S, F],
            "chunks": [4, 5, 6, 7, 8], "against_chunk": 11,
            "gpu_pinned": spread(lambda I, b: pinned[I][b]), "gpu_absolute": spread(lambda I, b: plain[I][b]),
            "restatement_pinned": spread(lambda I, b: ref_p[b][:, I]), "restatement_absolute": spread(lambda I, b: ref_u[b][:, I]),
            "gpu_pinned_against_restatement_max": float(f"{max(rel_rms(pinned[I][b], ref_p[b][:, I:I + 1]) for I in range(F) for b in range(2)):.2e}"),
            "frame_offset_5000_against_0": float(f"{max(rel_rms(far[b], base[b]) for b in range(2)):.2e}")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pinned_sink_probe.txt"))
    a = ap.parse_args()
    lines = [f"# python tools/pinned_sink_probe.py --reps {a.reps}   (one MI355X; sink rows {ROWS} x {DIM}, {LAYERS} layers x "
             f"{CACHES} caches)"]
    for level in (kernel_level(a.reps), model_level()):
        lines.append(json.dumps(level))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
