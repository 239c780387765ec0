"""Dynamic block masks (sparse.block_mask_from_qk, WanModel.set_attention_block_policy): what building a mask from q and k
on the device costs, what the masked forward under it costs beside the full forward of the same process, and what the mask
keeps.

    python tools/attn_dynamic_mask_probe.py [--reps 20] [--rounds 3] [--out profiles/dynamic_mask_probe.txt]

Shapes (B, H, S) = (1, 12, 32 760) and (4, 12, 1 560); operands: lattice-structured (tokens on an (F, 30, 52) lattice, 20
spatial groups, per head centre[group] + frame[f], q = 1.5 base + 0.7 noise, k likewise) and random; q carries
softmax_scale * log2(e) as the model's does, so score_scale = 1.  One JSON line per row, all device-event times: the median
microseconds over --reps repetitions after warm-up, taken --rounds times — ``*_us`` the middle median, ``*_spread_us`` their
max - min.  ``pool_us`` / ``select_us`` / ``tables_us`` time the three launches one by one (each with the allocation of its
outputs, as a layer issues them), ``build_us`` the three together.  Per mass tau: ``density``; ``mass_mean`` / ``mass_min``,
the true softmax mass the kept blocks hold per query row (fp32 scores in torch, chunk by chunk, over every head and row);
``rel_rms``, the masked output against the full one; ``masked_fwd_us``; ``build_share`` = build / full forward.
``break_even_density`` solves build + masked(d) = full on the straight line through the shape's measured (density, masked
forward) points.  Everything in one process on one device; quality on trained weights is not measured here or anywhere."""
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


def operands(kind, B, S, seed):
    """q (pre-scaled), k, V^T for the kernels: q, k bf16 [B * S, H * 128]."""
    d = H * D
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=g)
    if kind == "random":
        q, k = rnd(B, S, H, D), rnd(B, S, H, D)
    else:
        F = (S + 1559) // 1560
        tok = torch.arange(S, device="cuda")
        f, hh, ww = tok // 1560, (tok // 52) % 30, tok % 52
        group = (hh // 6) * 4 + ww // 13
        q, k = torch.empty(B, S, H, D, device="cuda"), torch.empty(B, S, H, D, device="cuda")
        for b in range(B):
            base = (rnd(H, 20, D)[:, group] + 0.5 * rnd(H, F, D)[:, f]).permute(1, 0, 2)
            q[b] = 1.5 * base + 0.7 * rnd(S, H, D)
            k[b] = 1.5 * base + 0.7 * rnd(S, H, D)
    q = (q * (D ** -0.5 * LOG2E)).bfloat16().view(B * S, d)
    k = k.bfloat16().view(B * S, d)
    v = rnd(B * S, d).bfloat16()
    Sp = (S + 63) // 64 * 64
    vt = torch.zeros(B, d, Sp, device="cuda", dtype=torch.bfloat16)
    vt[:, :, :S] = v.view(B, S, d).transpose(1, 2)
    return q, k, vt, Sp


def retained_mass(q, k, B, S, masks):
    """Per mask: (mean, min) over every (sample, head, query row) of the softmax mass its kept key blocks hold."""
    qs, ks = q.view(B, S, H, D), k.view(B, S, H, D)
    nb = (S + 127) // 128
    tot = [0.0 for _ in masks]
    low = [1.0 for _ in masks]
    step = 16                                                        # query blocks per chunk: 2 048 x S fp32 scores
    for b in range(B):
        for h in range(H):
            kf = ks[b, :, h].float()
            for i0 in range(0, nb, step):
                i1 = min(i0 + step, nb)
                r0, r1 = i0 * 128, min(i1 * 128, S)
                s = qs[b, r0:r1, h].float() @ kf.t()                 # base-2 logits (q carries the scale)
                p = torch.exp2(s - s.amax(-1, keepdim=True))
                p = p / p.sum(-1, keepdim=True)
                pb = torch.nn.functional.pad(p, (0, nb * 128 - S)).view(r1 - r0, nb, 128).sum(-1)      # per key block
                blk = torch.arange(r0, r1, device="cuda") // 128
                for n, m in enumerate(masks):
                    held = (pb * m[h % m.shape[0]][blk].float()).sum(-1)
                    tot[n] += float(held.sum())
                    low[n] = min(low[n], float(held.min()))
    return [(t / (B * H * S), l) for t, l in zip(tot, low)]


def rel_rms(a, b):
    a, b = a.float(), b.float()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt().clamp(min=1e-30))


def run_shape(B, S, kind, a, emit):
    d = H * D
    q, k, vt, Sp = operands(kind, B, S, seed=S + B)
    lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
    o = torch.empty(B * S, d, device="cuda", dtype=torch.bfloat16)
    shape = f"{B} x {H} x {S}, {kind}"

    def fwd(bm=None, out=o):
        ops.flash_attn_raw(ops.ptr(q), ops.ptr(k), ops.ptr(vt), ops.ptr(out), ops.ptr(lens), B, H, S, S, S * d, d, S * d, d,
                           d * Sp, S * d, d, Sp, D ** -0.5, q_prescaled=1, block_mask=bm)
    full_us, full_sp = timed(fwd, a.reps, a.rounds)
    o_full = torch.empty_like(o)
    fwd(out=o_full)
    pol = sparse.DynamicBlockPolicy(0.9)
    always = pol.always_on(q.device, (S + 127) // 128, (S + 127) // 128, H)
    pool_us, pool_sp = timed(lambda: sparse.pool_blocks(q, B, S, H, d, None, k, S, d, lens), a.reps, a.rounds)
    qp, kp = sparse.pool_blocks(q, B, S, H, d, None, k, S, d, lens)
    sel_us, sel_sp = timed(lambda: sparse.select_blocks(qp, kp, S, S, 1.0, 0.9, 0.0, always, None, lens), a.reps, a.rounds)
    m09 = sparse.select_blocks(qp, kp, S, S, 1.0, 0.9, 0.0, always, None, lens)
    tab_us, tab_sp = timed(lambda: sparse.tables_from_mask(m09, S, S), a.reps, a.rounds)
    build = lambda mass=0.9: sparse.block_mask_from_rows(q, k, B, H, S, S, d, d, sparse.DynamicBlockPolicy(mass) if mass != 0.9
                                                         else pol, 1.0, None, lens)
    build_us, build_sp = timed(build, a.reps, a.rounds)
    bytes_read = 2 * B * S * d * 2
    emit({"shape": shape, "full_fwd_us": round(full_us, 1), "full_fwd_spread_us": round(full_sp, 1),
          "pool_us": round(pool_us, 1), "pool_spread_us": round(pool_sp, 1), "pool_bytes_read": bytes_read,
          "pool_TB_per_s": round(bytes_read / pool_us * 1e-6, 2), "select_us": round(sel_us, 1),
          "select_spread_us": round(sel_sp, 1), "tables_us": round(tab_us, 1), "tables_spread_us": round(tab_sp, 1),
          "build_us": round(build_us, 1), "build_spread_us": round(build_sp, 1), "build_share": round(build_us / full_us, 4)})
    masses = (0.5, 0.9, 0.98)
    bms = [build(m) for m in masses]
    kept = retained_mass(q, k, B, S, [bm.mask for bm in bms])
    points = []
    for mass, bm, (mean, low) in zip(masses, bms, kept):
        us, sp = timed(lambda: fwd(bm), a.reps, a.rounds)
        fwd(bm)
        points.append((bm.density, us))
        emit({"shape": shape, "mass": mass, "density": round(bm.density, 4), "mass_mean": round(mean, 4),
              "mass_min": round(low, 4), "rel_rms": float(f"{rel_rms(o, o_full):.3e}"), "masked_fwd_us": round(us, 1),
              "masked_fwd_spread_us": round(sp, 1), "masked_over_full": round(us / full_us, 3),
              "build_plus_masked_over_full": round((us + build_us) / full_us, 3)})
    return shape, full_us, build_us, points


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dynamic_mask_probe.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_dynamic_mask_probe: no GPU (times are device times; there is nothing to measure without one)")
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    for B, S in ((1, 32760), (4, 1560)):
        pts, full, build = [], None, None
        for kind in ("structured", "random"):
            shape, full, build, p = run_shape(B, S, kind, a, emit)
            pts += p
        # masked(d) ~ c0 + c1 d through the measured points of this shape; build + masked(d*) = full
        n = len(pts)
        mx, my = sum(x for x, _ in pts) / n, sum(y for _, y in pts) / n
        c1 = sum((x - mx) * (y - my) for x, y in pts) / max(sum((x - mx) ** 2 for x, _ in pts), 1e-30)
        c0 = my - c1 * mx
        emit({"shape": f"{B} x {H} x {S}", "masked_fwd_fit_us": [round(c0, 1), round(c1, 1)],
              "break_even_density": round((full - build - c0) / c1, 3) if c1 > 0 else None})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
