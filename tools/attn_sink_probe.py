"""Three-run interval-mask self-attention timing: teacher forcing with an attention sink, 12 heads, chunks of 3 latent
frames at 480 x 832 (group = 4 680 tokens), [7 clean chunks | 7 noisy chunks] = 2 x 32 760 tokens.

    python tools/attn_sink_probe.py [--reps 10] [--rounds 3] [--out profiles/sink_mask_probe.txt]

Rows (one JSON line each, also written to --out), all variants alternating in ONE process as in
tools/attn_interval_probe.py (``*_us``: the middle one of --rounds medians of --reps runs, ``*_spread_us``: their max - min):
  1. W = 1, S = 1 (three runs per noisy row) through the three-run entries;
  2. W = 1, S = 0 (two runs) through the unchanged two-run entries;
  3. the table of row 2 through the three-run entries: what the three-run form costs per tile on the same mask.
``key_tiles``: the 64-key tiles the forward runs per head, from ``IntervalMask.tiles``; ``one_hull_tiles`` /
``two_hull_tiles``: what a kernel with one range per query block, or with two (the sink merged with whichever neighbour
costs fewer tiles), would run."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from attn_interval_probe import CHUNKS, FPC, H, TPF, Operands, alternate, causal  # noqa: E402


def block_ranges(mask, L, block=128, tile=64):
    """Per query block the merged tile ranges [(first, end)] the forward runs — ``IntervalMask.tiles`` before the sum."""
    q_iv, out = mask.intervals()[0], []
    for q0 in range(0, L, block):
        rows = q_iv[q0 // mask.group:(min(q0 + block, L) - 1) // mask.group + 1]
        hull = []
        for s in range(mask.runs):
            iv = [(r[2 * s] * mask.group, min(r[2 * s + 1] * mask.group, L)) for r in rows if r[2 * s + 1] > r[2 * s]]
            iv = [(a, b) for a, b in iv if b > a]
            if not iv:
                continue
            a, b = min(a for a, _ in iv) // tile, (max(b for _, b in iv) - 1) // tile + 1
            if hull and a <= hull[-1][1]:
                hull[-1] = (hull[-1][0], max(hull[-1][1], b))
            else:
                hull.append((a, b))
        out.append(hull)
    return out


def hull_counts(mask, L):
    """(tiles as run, with at most two ranges per block, with one)."""
    run = two = one = 0
    for hull in block_ranges(mask, L):
        n = sum(b - a for a, b in hull)
        gaps = [hull[i + 1][0] - hull[i][1] for i in range(len(hull) - 1)]
        run += n
        two += n + (min(gaps) if len(gaps) == 2 else 0)
        one += n + sum(gaps)
    return run, two, one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sink_mask_probe.txt"))
    a = ap.parse_args()
    C, S = TPF * FPC, 2 * TPF * FPC * CHUNKS
    lines = [f"# python tools/attn_sink_probe.py --reps {a.reps} --rounds {a.rounds}   (one MI355X; {H} heads, groups of {C} "
             f"tokens, [{CHUNKS} clean | {CHUNKS} noisy] chunks)"]
    sink3 = causal.IntervalMask(causal.teacher_forcing_groups(CHUNKS, 1, 1), C, "cuda", runs=3)
    win2 = causal.IntervalMask(causal.teacher_forcing_groups(CHUNKS, 1), C, "cuda")
    win3 = causal.IntervalMask(causal.teacher_forcing_groups(CHUNKS, 1), C, "cuda", runs=3)
    variants = [("teacher forcing W = 1, S = 1, three-run entries", sink3),
                ("teacher forcing W = 1, S = 0, two-run entries", win2),
                ("teacher forcing W = 1, S = 0, three-run entries", win3)]
    x = Operands(S, len(variants))
    all_tiles = ((S + 127) // 128) * ((S + 63) // 64)
    f = alternate([x.fwd(i, interval_mask=m) for i, (_, m) in enumerate(variants)], a.reps, a.rounds)
    b = alternate([x.bwd(i, interval_mask=m) for i, (_, m) in enumerate(variants)], a.reps, a.rounds)
    for (label, m), (fu, fs), (bu, bs) in zip(variants, f, b):
        run, two, one = hull_counts(m, S)
        assert run == m.tiles(S, S)
        lines.append(json.dumps({
            "shape": f"1 x {S}, {H} heads", "attention": label, "visible": round(run / all_tiles, 4), "key_tiles": run,
            "two_hull_tiles": two, "one_hull_tiles": one, "fwd_us": fu, "fwd_spread_us": fs, "bwd_us": bu, "bwd_spread_us": bs,
            "fwd_ns_per_tile": round(fu * 1e3 / (H * run), 2), "bwd_ns_per_tile": round(bu * 1e3 / (H * run), 2)}))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
