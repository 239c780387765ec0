"""Chunk-causal self-attention timing at the sampling length: S = 32 760 (21 latent frames of 1 560 tokens), 12 heads,
chunks of 3 frames (4 680 tokens, 7 chunks: 28 of the 49 chunk pairs, 4/7 of the score matrix, are visible).

    python tools/attn_chunk_causal_probe.py [--reps 10] [--rounds 3] [--out profiles/chunk_causal_probe.txt]

Rows (one JSON line each, also written to --out):
  * forward + backward of one self-attention on random operands: full attention on the short-sequence kernels (the
    forward pinned with ATTN_SHORT_KERNEL; the backward through the varlen entry with the unbounded band, i.e. the HIP
    kernels the staircase instantiations are made from — launches this feature does not change), the default
    full-attention backward (the w64 streams) for scale, and the staircase with unbounded and one-chunk look-back;
  * one rollout attention call per chunk position, as WanModel.forward_chunk issues it: Lq = 4 680 queries against
    Lk = 4 680 ... 32 760 cached keys (plain attention, short-sequence kernel).
``*_us`` is the middle one of --rounds medians over --reps timed repetitions after warm-up and ``*_spread_us`` their
max - min.  ``key_tiles`` counts the 64-key tiles the forward runs per head, summed over the 128-row query blocks;
``fwd_ns_per_tile`` divides the forward by H * key_tiles — equal figures mean the time follows the visible tile count."""
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
TPF, FRAMES, FPC = 1560, 21, 3
LOG2E = 1.4426950408889634


def timed(fn, reps, rounds, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    meds = []
    for _ in range(rounds):
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        ts.sort()
        meds.append(ts[len(ts) // 2])
    meds.sort()
    return round(meds[len(meds) // 2], 1), round(meds[-1] - meds[0], 1)


def stair_tiles(Lq, Lk, C, W, P=0):
    """64-key tiles the staircase forward runs per head: per 128-row query block, first row's lower end to last row's upper."""
    n = 0
    for q0 in range(0, Lq, 128):
        q1 = min(q0 + 128, Lq) - 1
        lo = 0 if W < 0 else max(0, ((P + q0) // C - W) * C)
        hi = min(Lk, ((P + q1) // C + 1) * C) - 1
        if hi >= lo:
            n += hi // 64 - lo // 64 + 1
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunk_causal_probe.txt"))
    a = ap.parse_args()
    S, C, d = TPF * FRAMES, TPF * FPC, H * D
    g = torch.Generator(device="cuda").manual_seed(S)
    q = (torch.randn(S, d, device="cuda", generator=g) * (D ** -0.5 * LOG2E)).bfloat16()
    k = torch.randn(S, d, device="cuda", generator=g).bfloat16()
    v = torch.randn(S, d, device="cuda", generator=g).bfloat16()
    do = torch.randn(S, d, device="cuda", generator=g).bfloat16()
    Sp = (S + 63) // 64 * 64
    vt = torch.zeros(1, d, Sp, device="cuda", dtype=torch.bfloat16)
    vt[:, :, :S] = v.view(1, S, d).transpose(1, 2)
    lens = torch.full((1,), S, dtype=torch.int32, device="cuda")
    o = torch.empty(S, d, device="cuda", dtype=torch.bfloat16)
    o32 = torch.empty(S, d, device="cuda", dtype=torch.float32)
    lse = torch.empty(1, H, S, device="cuda", dtype=torch.float32)
    out = tuple(torch.empty(S, d, device="cuda", dtype=torch.bfloat16) for _ in range(3))
    lines = [f"# python tools/attn_chunk_causal_probe.py --reps {a.reps} --rounds {a.rounds}   (one MI355X; S = {S}, {H} heads, "
             f"chunks of {C} tokens)"]

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    all_tiles = ((S + 127) // 128) * ((S + 63) // 64)
    for label, cc, bwd_kw in (("full, short-sequence kernels (varlen backward, unbounded band)", None, dict(q_lens=lens)),
                              ("full, default backward (w64 streams)", None, {}),
                              (f"staircase C = {C}, all earlier chunks", (C, -1, 0), {}),
                              (f"staircase C = {C}, one chunk back", (C, 1, 0), {})):
        def fwd():
            ops.flash_attn_raw(ops.ptr(q), ops.ptr(k), ops.ptr(vt), ops.ptr(o), ops.ptr(lens), 1, H, S, S, S * d, d, S * d, d,
                               d * Sp, S * d, d, Sp, D ** -0.5, lse=ops.ptr(lse), q_prescaled=1, o32=ops.ptr(o32),
                               flags=ops.ATTN_SHORT_KERNEL, chunk_causal=cc)

        def bwd():
            ops.flash_attn_bwd(q, k, v, o, do, lse, lens, 1, H, S, S, D ** -0.5, q_prescaled=True, out=out, o32=o32,
                               chunk_causal=cc, **bwd_kw)
        fwd()
        tiles = all_tiles if cc is None else stair_tiles(S, S, cc[0], cc[1])
        (f, fs), (b, bs) = timed(fwd, a.reps, a.rounds), timed(bwd, a.reps, a.rounds)
        emit({"shape": f"1 x {S}, {H} heads", "attention": label, "visible": round(tiles / all_tiles, 4), "key_tiles": tiles,
              "fwd_us": f, "fwd_spread_us": fs, "bwd_us": b, "bwd_spread_us": bs,
              "fwd_ns_per_tile": round(f * 1e3 / (H * tiles), 2)})
    # the rollout: chunk n of 7 against the n + 1 chunks of keys in the cache (K rows / V^T columns of the same buffers)
    oc = torch.empty(C, d, device="cuda", dtype=torch.bfloat16)
    for n in range(S // C):
        Lk = (n + 1) * C

        def call():
            ops.flash_attn_raw(ops.ptr(q, n * C * d), ops.ptr(k), ops.ptr(vt), ops.ptr(oc), None, 1, H, C, Lk, C * d, d, S * d, d,
                               d * Sp, C * d, d, Sp, D ** -0.5, q_prescaled=1, flags=ops.ATTN_SHORT_KERNEL)
        f, fs = timed(call, a.reps, a.rounds)
        tiles = ((C + 127) // 128) * ((Lk + 63) // 64)
        emit({"shape": f"rollout chunk {n}: Lq = {C}, Lk = {Lk}", "key_tiles": tiles, "fwd_us": f, "fwd_spread_us": fs,
              "fwd_ns_per_tile": round(f * 1e3 / (H * tiles), 2)})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
