"""Windowed cross-attention timing: the video's queries on frame-aligned condition tokens, masked against plain.

    python tools/attn_condition_window_probe.py [--reps 20] [--rounds 3] [--out profiles/condition_window_probe.txt]

12 heads; queries: 4 latent frames of 1 560 tokens (a chunk of a rollout) and 21 frames (Lq = 32 760, a whole clip at
480 x 832); keys: 21 frames x 8 condition tokens + 512 text rows, of which k_lens = 168 + 300 are live.  For the windows
(1, 0) and (2, 2) the masked launch (``causal.IntervalMask(k_group=1)`` of ``causal.condition_window_visible``:
omh_flash_attn_*_interval_rect_d128) and the plain launch on the same operands (the training forward's short-sequence
kernel with its fp32 output, the round-3 backward) alternate in ONE process: a round times every variant once (--reps
repetitions after a warm-up, their median), ``*_us`` is the middle one of --rounds such medians and ``*_spread_us`` their
max - min.  ``key_tiles``: the 64-key tiles the forward runs per head, summed over its 128-row query blocks
(``IntervalMask.tiles``; the plain launch runs every live tile).  One JSON line per variant, also written to --out."""
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
TPF, FRAMES, PER_FRAME, N_TEXT, TEXT_LIVE = 1560, 21, 8, 512, 300
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


class Operands:
    def __init__(self, Lq, Lk, klen, variants):
        d = H * D
        g = torch.Generator(device="cuda").manual_seed(Lq)
        self.Lq, self.Lk, self.d = Lq, Lk, d
        self.q = (torch.randn(Lq, d, device="cuda", generator=g) * (D ** -0.5 * LOG2E)).bfloat16()
        self.k, self.v = (torch.randn(Lk, d, device="cuda", generator=g).bfloat16() for _ in range(2))
        self.do = torch.randn(Lq, d, device="cuda", generator=g).bfloat16()
        self.Lp = (Lk + 63) // 64 * 64
        self.vt = torch.zeros(1, d, self.Lp, device="cuda", dtype=torch.bfloat16)
        self.vt[:, :, :Lk] = self.v.view(1, Lk, d).transpose(1, 2)
        self.lens = torch.full((1,), klen, dtype=torch.int32, device="cuda")
        # every variant keeps its own forward results, so that the backwards can alternate too
        self.o = [torch.empty(Lq, d, device="cuda", dtype=torch.bfloat16) for _ in range(variants)]
        self.o32 = [torch.empty(Lq, d, device="cuda", dtype=torch.float32) for _ in range(variants)]
        self.lse = [torch.empty(1, H, Lq, device="cuda", dtype=torch.float32) for _ in range(variants)]
        self.out = (torch.empty(Lq, d, device="cuda", dtype=torch.bfloat16),
                    torch.empty(Lk, d, device="cuda", dtype=torch.bfloat16), torch.empty(Lk, d, device="cuda", dtype=torch.bfloat16))

    def fwd(self, i, **mask):
        Lq, Lk, d, Lp = self.Lq, self.Lk, self.d, self.Lp
        return lambda: ops.flash_attn_raw(ops.ptr(self.q), ops.ptr(self.k), ops.ptr(self.vt), ops.ptr(self.o[i]), ops.ptr(self.lens),
                                          1, H, Lq, Lk, Lq * d, d, Lk * d, d, d * Lp, Lq * d, d, Lp, D ** -0.5,
                                          lse=ops.ptr(self.lse[i]), q_prescaled=1, o32=ops.ptr(self.o32[i]),
                                          flags=ops.ATTN_SHORT_KERNEL | ops.ATTN_ALLOW_SPLIT, **mask)

    def bwd(self, i, **mask):
        return lambda: ops.flash_attn_bwd(self.q, self.k, self.v, self.o[i], self.do, self.lse[i], self.lens, 1, H, self.Lq, self.Lk,
                                          D ** -0.5, q_prescaled=True, out=self.out, o32=self.o32[i], **mask)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "condition_window_probe.txt"))
    a = ap.parse_args()
    Lk, klen = FRAMES * PER_FRAME + N_TEXT, FRAMES * PER_FRAME + TEXT_LIVE
    lines = [f"# python tools/attn_condition_window_probe.py --reps {a.reps} --rounds {a.rounds}   (one MI355X; {H} heads, "
             f"Lk = {FRAMES} x {PER_FRAME} + {N_TEXT}, k_lens = {klen})"]
    token_frames = torch.tensor([f for f in range(FRAMES) for _ in range(PER_FRAME)])
    for q_frames in (4, FRAMES):
        Lq = q_frames * TPF
        live_tiles = ((Lq + 127) // 128) * ((klen + 63) // 64)
        variants = [("plain", {}, live_tiles)]
        for window in ((1, 0), (2, 2)):
            vis = causal.condition_window_visible(q_frames, token_frames, N_TEXT, *window)
            m = causal.IntervalMask(vis, TPF, "cuda", k_group=1)
            variants.append((f"window {window}", dict(interval_mask=m), m.tiles(Lq, klen)))
        x = Operands(Lq, Lk, klen, len(variants))
        f = alternate([x.fwd(i, **v[1]) for i, v in enumerate(variants)], a.reps, a.rounds)
        b = alternate([x.bwd(i, **v[1]) for i, v in enumerate(variants)], a.reps, a.rounds)   # each against its own forward
        for (label, _, tiles), (fu, fs), (bu, bs) in zip(variants, f, b):
            lines.append(json.dumps({"shape": f"Lq = {q_frames} x {TPF}, Lk = {Lk} ({klen} live), {H} heads", "attention": label,
                                     "key_tiles": tiles, "fwd_us": fu, "fwd_spread_us": fs, "bwd_us": bu, "bwd_spread_us": bs}))
            print(lines[-1], flush=True)
        del x
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
