"""Sliding-window self-attention timing (WanModel(window_size=)): forward + backward of one self-attention as the
training step issues it (short-sequence forward with lse / o32, bf16 gradients), full attention against bands; and the
inference forward of one long clip (full: the long-sequence stream; a band: the short-sequence kernel).

    python tools/attn_band_probe.py [--reps 20]

Prints one JSON line per shape: median microseconds over --reps timed repetitions after warm-up."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ops = importlib.import_module("omnihuman-1-hack_amd.ops")
H, D = 12, 128
LOG2E = 1.4426950408889634


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def tensors(B, S):
    d = H * D
    g = torch.Generator(device="cuda").manual_seed(S)
    q = (torch.randn(B * S, d, device="cuda", generator=g) * (D ** -0.5 * LOG2E)).bfloat16()
    k = torch.randn(B * S, d, device="cuda", generator=g).bfloat16()
    v = torch.randn(B * S, d, device="cuda", generator=g).bfloat16()
    Sp = (S + 63) // 64 * 64
    vt = torch.zeros(B, d, Sp, device="cuda", dtype=torch.bfloat16)
    vt[:, :, :S] = v.view(B, S, d).transpose(1, 2)
    do = torch.randn(B * S, d, device="cuda", generator=g).bfloat16()
    lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
    return q, k, v, vt, do, lens, Sp


def train_pair(B, S, window, reps):
    d = H * D
    q, k, v, vt, do, lens, Sp = tensors(B, S)
    o = torch.empty(B * S, d, device="cuda", dtype=torch.bfloat16)
    o32 = torch.empty(B * S, d, device="cuda", dtype=torch.float32)
    lse = torch.empty(B, H, S, device="cuda", dtype=torch.float32)
    out = tuple(torch.empty(B * S, d, device="cuda", dtype=torch.bfloat16) for _ in range(3))
    flags = ops.ATTN_SHORT_KERNEL | ops.ATTN_ALLOW_SPLIT

    def fwd():
        ops.flash_attn_raw(ops.ptr(q), ops.ptr(k), ops.ptr(vt), ops.ptr(o), ops.ptr(lens), B, H, S, S, S * d, d, S * d,
                           d, d * Sp, S * d, d, Sp, D ** -0.5, lse=ops.ptr(lse), q_prescaled=1, o32=ops.ptr(o32),
                           flags=flags, window=window)

    def bwd():
        ops.flash_attn_bwd(q, k, v, o, do, lse, lens, B, H, S, S, D ** -0.5, q_prescaled=True, out=out, o32=o32,
                           window=window)
    fwd()
    return timed(fwd, reps), timed(bwd, reps)


def infer_fwd(S, window, reps):
    d = H * D
    q, k, v, vt, do, lens, Sp = tensors(1, S)
    o = torch.empty(S, d, device="cuda", dtype=torch.bfloat16)

    def fwd():
        ops.flash_attn_raw(ops.ptr(q), ops.ptr(k), ops.ptr(vt), ops.ptr(o), ops.ptr(lens), 1, H, S, S, S * d, d, S * d,
                           d, d * Sp, S * d, d, Sp, D ** -0.5, q_prescaled=1, window=window)
    return timed(fwd, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    for w in ((-1, -1), (256, 256), (780, 780)):
        f, b = train_pair(4, 1560, w, a.reps)
        print(json.dumps({"shape": "train 4 x 1560, 12 heads", "window": list(w), "fwd_us": round(f, 1),
                          "bwd_us": round(b, 1), "fwd_bwd_us": round(f + b, 1)}), flush=True)
    for w in ((-1, -1), (1560, 1560), (3120, 3120)):
        f = infer_fwd(32760, w, a.reps)
        print(json.dumps({"shape": "infer 1 x 32760, 12 heads", "window": list(w), "fwd_us": round(f, 1)}), flush=True)


if __name__ == "__main__":
    main()
