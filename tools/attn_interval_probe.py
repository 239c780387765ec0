"""Interval-mask self-attention timing: 12 heads, chunks of 3 latent frames at 480 x 832 (group = 4 680 tokens).

    python tools/attn_interval_probe.py [--reps 10] [--rounds 3] [--out profiles/interval_mask_probe.txt]

Rows (one JSON line each, also written to --out):
  1. the chunk-causal staircase at Lq = Lk = 32 760 (7 chunks) through the staircase kernels (``chunk_causal=``) and as an
     interval table (``interval_mask=`` of the lower-triangular matrix): the same mask on the same operands;
  2. teacher forcing over [7 clean chunks | 7 noisy chunks], Lq = Lk = 65 520, with every earlier chunk visible (W = -1)
     and with one chunk of look-back (W = 1).
All variants of a group run in ONE process and alternate: a round times every variant once (--reps repetitions after a
warm-up, their median), and ``*_us`` is the middle one of --rounds such medians, ``*_spread_us`` their max - min.
``key_tiles`` counts the 64-key tiles the forward runs per head, summed over the 128-row query blocks, computed from the
table (``IntervalMask.tiles``); ``hull_tiles`` is what one range per query block — first visible tile to last — would
run, i.e. what skipping the gap between the two ranges saves.  ``fwd_ns_per_tile`` divides the forward by H * key_tiles."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ops = importlib.import_module("omnihuman-1-hack_amd.ops")
causal = importlib.import_module("omnihuman-1-hack_amd.causal")
H, D = 12, 128
TPF, FPC, CHUNKS = 1560, 3, 7
LOG2E = 1.4426950408889634


def median_of(fn, reps):
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


def alternate(fns, reps, rounds, warm=2):
    """[(median of the rounds' medians, their spread)] for the callables, timed round-robin."""
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    meds = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            meds[i].append(median_of(fn, reps))
    out = []
    for m in meds:
        m.sort()
        out.append((round(m[len(m) // 2], 1), round(m[-1] - m[0], 1)))
    return out


def stair_tiles(L, C, W):
    n = 0
    for q0 in range(0, L, 128):
        q1 = min(q0 + 128, L) - 1
        lo = 0 if W < 0 else max(0, (q0 // C - W) * C)
        n += (min(L, (q1 // C + 1) * C) - 1) // 64 - lo // 64 + 1
    return n


def hull_tiles(mask, L):
    """Tiles of one range per 128-row query block: from its first visible key tile to its last."""
    ends = [[r[0], r[3] if r[3] > r[2] else r[1]] for r in mask.intervals()[0]]
    n = 0
    for q0 in range(0, L, 128):
        rows = ends[q0 // mask.group:(min(q0 + 128, L) - 1) // mask.group + 1]
        lo, hi = min(r[0] for r in rows) * mask.group, min(max(r[1] for r in rows) * mask.group, L)
        n += (hi - 1) // 64 - lo // 64 + 1
    return n


class Operands:
    def __init__(self, S, variants):
        d = H * D
        g = torch.Generator(device="cuda").manual_seed(S)
        self.S, self.d = S, d
        self.q = (torch.randn(S, d, device="cuda", generator=g) * (D ** -0.5 * LOG2E)).bfloat16()
        self.k, self.v, self.do = (torch.randn(S, d, device="cuda", generator=g).bfloat16() for _ in range(3))
        self.Sp = (S + 63) // 64 * 64
        self.vt = torch.zeros(1, d, self.Sp, device="cuda", dtype=torch.bfloat16)
        self.vt[:, :, :S] = self.v.view(1, S, d).transpose(1, 2)
        self.lens = torch.full((1,), S, dtype=torch.int32, device="cuda")
        # every variant keeps its own forward results, so that the backwards can alternate too
        self.o = [torch.empty(S, d, device="cuda", dtype=torch.bfloat16) for _ in range(variants)]
        self.o32 = [torch.empty(S, d, device="cuda", dtype=torch.float32) for _ in range(variants)]
        self.lse = [torch.empty(1, H, S, device="cuda", dtype=torch.float32) for _ in range(variants)]
        self.out = tuple(torch.empty(S, d, device="cuda", dtype=torch.bfloat16) for _ in range(3))

    def fwd(self, i, **mask):
        S, d, Sp = self.S, self.d, self.Sp
        return lambda: ops.flash_attn_raw(ops.ptr(self.q), ops.ptr(self.k), ops.ptr(self.vt), ops.ptr(self.o[i]), ops.ptr(self.lens),
                                          1, H, S, S, S * d, d, S * d, d, d * Sp, S * d, d, Sp, D ** -0.5, lse=ops.ptr(self.lse[i]),
                                          q_prescaled=1, o32=ops.ptr(self.o32[i]), flags=ops.ATTN_SHORT_KERNEL, **mask)

    def bwd(self, i, **mask):
        S = self.S
        return lambda: ops.flash_attn_bwd(self.q, self.k, self.v, self.o[i], self.do, self.lse[i], self.lens, 1, H, S, S, D ** -0.5,
                                          q_prescaled=True, out=self.out, o32=self.o32[i], **mask)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interval_mask_probe.txt"))
    a = ap.parse_args()
    C = TPF * FPC
    lines = [f"# python tools/attn_interval_probe.py --reps {a.reps} --rounds {a.rounds}   (one MI355X; {H} heads, groups of "
             f"{C} tokens)"]

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    def group(S, variants):
        """variants: [(label, mask keywords, key tiles, hull tiles or None)]"""
        x = Operands(S, len(variants))
        all_tiles = ((S + 127) // 128) * ((S + 63) // 64)
        f = alternate([x.fwd(i, **v[1]) for i, v in enumerate(variants)], a.reps, a.rounds)
        b = alternate([x.bwd(i, **v[1]) for i, v in enumerate(variants)], a.reps, a.rounds)   # each against its own forward's lse / o32
        for (label, _, tiles, hull), (fu, fs), (bu, bs) in zip(variants, f, b):
            row = {"shape": f"1 x {S}, {H} heads", "attention": label, "visible": round(tiles / all_tiles, 4), "key_tiles": tiles,
                   "fwd_us": fu, "fwd_spread_us": fs, "bwd_us": bu, "bwd_spread_us": bs,
                   "fwd_ns_per_tile": round(fu * 1e3 / (H * tiles), 2), "bwd_ns_per_tile": round(bu * 1e3 / (H * tiles), 2)}
            if hull is not None:
                row["hull_tiles"] = hull
            emit(row)

    S = C * CHUNKS
    stairs = causal.IntervalMask(torch.ones(CHUNKS, CHUNKS).tril(), C, "cuda")
    group(S, [("staircase, chunk_causal kernels", dict(chunk_causal=(C, -1, 0)), stair_tiles(S, C, -1), None),
              ("staircase as an interval table", dict(interval_mask=stairs), stairs.tiles(S, S), hull_tiles(stairs, S))])
    S = 2 * C * CHUNKS
    variants = []
    for W in (-1, 1):
        m = causal.IntervalMask(causal.teacher_forcing_groups(CHUNKS, W), C, "cuda")
        variants.append((f"teacher forcing, n = {CHUNKS}, W = {W}", dict(interval_mask=m), m.tiles(S, S), hull_tiles(m, S)))
    group(S, variants)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
