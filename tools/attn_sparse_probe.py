"""Block-sparse self-attention timing (WanModel.set_attention_block_mask) beside the band and full attention: forward +
backward of one self-attention as the training step issues it, and the inference forward of one long clip (full: the
long-sequence stream; band and block mask: the short-sequence kernel).

    python tools/attn_sparse_probe.py [--reps 20] [--rounds 3]

Prints one JSON line per row: the median microseconds over --reps timed repetitions after warm-up, taken --rounds
times — ``*_us`` is the middle one of those medians and ``*_spread_us`` their max - min (what "the same" means
between two rows).  ``density`` is the share of 128 x 128 blocks kept (of 64-key tiles met, for a band) and
``key_tiles`` the 64-key tiles the forward runs per (sample, head), summed over the query blocks; ``fwd_ns_per_tile``
divides the forward by B * H * key_tiles.  Everything in one process on one device."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ops = importlib.import_module("omnihuman-1-hack_amd.ops")
sparse = importlib.import_module("omnihuman-1-hack_amd.sparse")
H, D = 12, 128
LOG2E = 1.4426950408889634


def timed(fn, reps, rounds, warm=3):
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
    return meds[len(meds) // 2], meds[-1] - meds[0]


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


def band_tiles(S, w):
    """64-key tiles the band kernel runs per (sample, head): per 128-row query block, the tiles its rows' bands meet."""
    n = 0
    for q0 in range(0, S, 128):
        q1 = min(q0 + 128, S) - 1
        n += min(S - 1, q1 + w) // 64 - max(0, q0 - w) // 64 + 1
    return n


def band_cover(S, w):
    """The block mask that covers exactly the blocks a (w, w) band touches."""
    nb = (S + 127) // 128
    lo = torch.arange(nb) * 128
    hi = torch.clamp(lo + 127, max=S - 1)
    return (lo[None, :] <= hi[:, None] + w) & (hi[None, :] >= lo[:, None] - w)


def mask_tiles(bm, S):
    """64-key tiles the block-list kernel runs per (sample, head), averaged over the mask's heads (klen = S)."""
    last = (S - 1) // 128
    drop = 1 if last * 128 + 64 >= S else 0                          # the last block's second tile holds no key
    return (2 * int(bm.row_cnt.sum()) - drop * int(bm.mask[:, :, last].sum())) / bm.heads


def variant(kind, arg, S):
    """-> (label, window, BlockMask or None, density, key tiles)."""
    all_tiles = ((S + 127) // 128) * ((S + 63) // 64)
    if kind == "full":
        return "full", (-1, -1), None, 1.0, all_tiles
    if kind == "band":
        t = band_tiles(S, arg)
        return f"band +-{arg}", (arg, arg), None, t / all_tiles, t
    mask = band_cover(S, arg) if kind == "cover" else sparse.block_mask_from_3d_window((21, 30, 52), arg)
    bm = sparse.BlockMask(mask, S, S).to("cuda")
    label = f"block cover of band +-{arg}" if kind == "cover" else f"3d window {tuple(arg)}"
    return label, (-1, -1), bm, bm.density, mask_tiles(bm, S)


def train_pair(B, S, window, bm, reps, rounds):
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
                           flags=flags, window=window, block_mask=bm)

    def bwd():
        ops.flash_attn_bwd(q, k, v, o, do, lse, lens, B, H, S, S, D ** -0.5, q_prescaled=True, out=out, o32=o32,
                           window=window, block_mask=bm)
    fwd()
    return timed(fwd, reps, rounds), timed(bwd, reps, rounds)


def infer_fwd(S, window, bm, reps, rounds):
    d = H * D
    q, k, v, vt, do, lens, Sp = tensors(1, S)
    o = torch.empty(S, d, device="cuda", dtype=torch.bfloat16)

    def fwd():
        ops.flash_attn_raw(ops.ptr(q), ops.ptr(k), ops.ptr(vt), ops.ptr(o), ops.ptr(lens), 1, H, S, S, S * d, d, S * d,
                           d, d * Sp, S * d, d, Sp, D ** -0.5, q_prescaled=1, window=window, block_mask=bm)
    return timed(fwd, reps, rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    B, S = 4, 1560
    for kind, arg in (("full", None), ("band", 256), ("cover", 256), ("band", 780), ("cover", 780)):
        label, window, bm, dens, tiles = variant(kind, arg, S)
        (f, fs), (b, bs) = train_pair(B, S, window, bm, a.reps, a.rounds)
        print(json.dumps({"shape": "train 4 x 1560, 12 heads", "attention": label, "density": round(dens, 4),
                          "key_tiles": tiles, "fwd_us": round(f, 1), "fwd_spread_us": round(fs, 1), "bwd_us": round(b, 1),
                          "bwd_spread_us": round(bs, 1), "fwd_ns_per_tile": round(f * 1e3 / (B * H * tiles), 2)}), flush=True)
    S = 32760
    for kind, arg in (("full", None), ("band", 1560), ("cover", 1560), ("band", 3120), ("cover", 3120),
                      ("3d", (2, 6, 52)), ("3d", (1, 30, 52)), ("3d", (21, 4, 8))):
        label, window, bm, dens, tiles = variant(kind, arg, S)
        f, fs = infer_fwd(S, window, bm, a.reps, a.rounds)
        print(json.dumps({"shape": "infer 1 x 32760, 12 heads", "attention": label, "density": round(dens, 4),
                          "key_tiles": tiles, "fwd_us": round(f, 1), "fwd_spread_us": round(fs, 1),
                          "fwd_ns_per_tile": round(f * 1e3 / (H * tiles), 2)}), flush=True)


if __name__ == "__main__":
    main()
