"""Teacher forcing under a pinned sink: what the extended key axis costs at the 1.3B geometry — 12 heads of 128, chunks of
3 latent frames at 480 x 832 (4 680 tokens), [7 clean | 7 noisy] chunks, W = 1, S = 1: four rotated images of the sink
chunk behind the 65 520 tokens of the key axis, Lk = 84 240.

    python tools/pinned_tf_probe.py [--reps 10] [--rounds 3] [--step-layers 2] [--out profiles/pinned_tf_probe.txt]

Rows (one JSON line each, also written to --out), every pair alternating in ONE process as in tools/attn_interval_probe.py
(``*_us``: the middle one of --rounds medians of --reps runs, ``*_spread_us``: their max - min):
  1. self-attention forward / backward under ``teacher_forcing_groups(7, 1, 1)`` (Lk = Lq) and under its ``pin_sink=True``
     form (Lk = Lq + 4 x 4 680), the three-run entries both; ``key_tiles`` from ``IntervalMask.tiles``;
  2. one layer's fan-out (``ops.rope_shift_fan``: 4 images of 4 680 x 1 536 into the K buffer) and the device copy of the
     same rows into the same place; one layer's fold (``ops.rope_shift_fold`` for dK with the table and for dV without, out
     of the [Lk, 2 dim] scratch into the dk | dv thirds of dqkv) and a device copy that reads and writes as many bytes;
     the copy of the rows nothing is folded into (scratch -> dqkv), which a backward writing dqkv directly would not need;
  3. with --step-layers N > 0: one ``causal.forcing_loss`` step (forward + backward, B = 1) of an N-layer model of the 1.3B
     width on that clip, pinned against unpinned.
``gbps`` counts bytes read plus bytes written.  Reported, not gated: no time was fixed in advance."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from attn_interval_probe import CHUNKS, D, FPC, H, LOG2E, TPF, alternate, causal, ops  # noqa: E402

W, S = 1, 1
CT = TPF * FPC
DIM = H * D


class Attention:
    """q over Lq rows, k / v over Lk >= Lq rows (the first Lq of them shared by every variant), one result set per variant."""

    def __init__(self, Lq, Lk_max):
        g = torch.Generator(device="cuda").manual_seed(Lq)
        self.Lq = Lq
        self.q = (torch.randn(Lq, DIM, device="cuda", generator=g) * (D ** -0.5 * LOG2E)).bfloat16()
        self.k, self.v = (torch.randn(Lk_max, DIM, device="cuda", generator=g).bfloat16() for _ in range(2))
        self.do = torch.randn(Lq, DIM, device="cuda", generator=g).bfloat16()
        self.ldv = (Lk_max + 63) // 64 * 64
        self.vt = torch.zeros(1, DIM, self.ldv, device="cuda", dtype=torch.bfloat16)
        self.vt[:, :, :Lk_max] = self.v.view(1, Lk_max, DIM).transpose(1, 2)
        self.res = {}

    def _res(self, i, Lk):
        if i not in self.res:
            e = lambda *s, dt=torch.bfloat16: torch.empty(*s, device="cuda", dtype=dt)
            self.res[i] = (e(self.Lq, DIM), e(self.Lq, DIM, dt=torch.float32), e(1, H, self.Lq, dt=torch.float32),
                           (e(self.Lq, DIM), e(Lk, DIM), e(Lk, DIM)))
        return self.res[i]

    def fwd(self, i, Lk, mask):
        o, o32, lse, _ = self._res(i, Lk)
        Lq = self.Lq
        return lambda: ops.flash_attn_raw(ops.ptr(self.q), ops.ptr(self.k), ops.ptr(self.vt), ops.ptr(o), None, 1, H, Lq, Lk,
                                          Lq * DIM, DIM, Lk * DIM, DIM, DIM * self.ldv, Lq * DIM, DIM, self.ldv, D ** -0.5,
                                          lse=ops.ptr(lse), q_prescaled=1, o32=ops.ptr(o32), interval_mask=mask)

    def bwd(self, i, Lk, mask):
        o, o32, lse, out = self._res(i, Lk)
        return lambda: ops.flash_attn_bwd(self.q, self.k[:Lk], self.v[:Lk], o, self.do, lse, None, 1, H, self.Lq, Lk, D ** -0.5,
                                          q_prescaled=True, out=out, o32=o32, interval_mask=mask)


def attention_rows(a, emit):
    Lq = 2 * CT * CHUNKS
    copies = causal.sink_copy_deltas(CHUNKS, W, S, FPC)
    Lk = Lq + len(copies) * S * CT
    plain = causal.IntervalMask(causal.teacher_forcing_groups(CHUNKS, W, S), CT, "cuda", runs=3)
    pinned = causal.IntervalMask(causal.teacher_forcing_groups(CHUNKS, W, S, pin_sink=True), CT, "cuda", runs=3)
    variants = [("teacher forcing W = 1, S = 1", Lq, plain), ("teacher forcing W = 1, S = 1, pinned sink", Lk, pinned)]
    x = Attention(Lq, Lk)
    f = alternate([x.fwd(i, L, m) for i, (_, L, m) in enumerate(variants)], a.reps, a.rounds)
    b = alternate([x.bwd(i, L, m) for i, (_, L, m) in enumerate(variants)], a.reps, a.rounds)
    for (label, L, m), (fu, fs), (bu, bs) in zip(variants, f, b):
        tiles = m.tiles(Lq, L)
        emit({"shape": f"1 x {Lq} queries, {L} keys, {H} heads", "attention": label, "key_tiles": tiles, "fwd_us": fu,
              "fwd_spread_us": fs, "bwd_us": bu, "bwd_spread_us": bs, "fwd_ns_per_tile": round(fu * 1e3 / (H * tiles), 2),
              "bwd_ns_per_tile": round(bu * 1e3 / (H * tiles), 2)})


def kernel_rows(a, emit):
    Lq = 2 * CT * CHUNKS
    deltas = [d for _, d in causal.sink_copy_deltas(CHUNKS, W, S, FPC)]
    copies, sr = len(deltas), S * CT
    Lk = Lq + copies * sr
    g = torch.Generator(device="cuda").manual_seed(1)
    k = torch.randn(1, Lk, DIM, device="cuda", generator=g).bfloat16()
    tab = ops.rope_shift_table(deltas, D, device="cuda")
    images = torch.as_strided(k, (1, copies, sr, DIM), (Lk * DIM, sr * DIM, DIM, 1), Lq * DIM)
    fan = lambda: ops.rope_shift_fan(k[:, :sr], images, tab, D)
    fan_copy = lambda: images.copy_(k[:, None, :sr].expand(-1, copies, -1, -1))
    (fu, fs), (cu, cs) = alternate([fan, fan_copy], a.reps, a.rounds)
    nbytes = 2 * 2 * copies * sr * DIM                                            # every image: read its source, written once
    emit({"kernel": "rope_shift_fan, one layer", "copies": copies, "rows": sr, "dim": DIM, "bytes_moved": nbytes, "fan_us": fu,
          "fan_spread_us": fs, "copy_us": cu, "copy_spread_us": cs, "fan_gbps": round(nbytes / fu / 1e3, 1),
          "copy_gbps": round(nbytes / cu / 1e3, 1)})
    dkv = torch.randn(1, Lk, 2 * DIM, device="cuda", generator=g).bfloat16()
    dqkv = torch.empty(1, Lq, 3 * DIM, device="cuda", dtype=torch.bfloat16)
    image = lambda c0: torch.as_strided(dkv, (1, copies, sr, DIM), (Lk * 2 * DIM, sr * 2 * DIM, 2 * DIM, 1), Lq * 2 * DIM + c0)

    def fold():
        ops.rope_shift_fold((dkv[:, :sr, :DIM], image(0)), dqkv[:, :sr, DIM:2 * DIM], tab, D)
        ops.rope_shift_fold((dkv[:, :sr, DIM:], image(DIM)), dqkv[:, :sr, 2 * DIM:], None, D)
    flat_in = torch.empty((copies + 2) * sr, DIM, device="cuda", dtype=torch.bfloat16)      # reads + writes of one fold ...
    flat_out = torch.empty_like(flat_in)                                                 # ... as a plain copy, per operand

    def fold_copy():
        flat_out.copy_(flat_in)
        flat_out.copy_(flat_in)
    rest = lambda: dqkv[:, sr:, DIM:].copy_(dkv[:, sr:Lq])
    (fu, fs), (cu, cs), (ru, rs) = alternate([fold, fold_copy, rest], a.reps, a.rounds)
    nbytes = 2 * 2 * (copies + 2) * sr * DIM                                      # dK and dV: base + images read, sink rows written
    emit({"kernel": "rope_shift_fold, one layer (dK with the table + dV without)", "copies": copies, "rows": sr, "dim": DIM,
          "bytes_moved": nbytes, "fold_us": fu, "fold_spread_us": fs, "copy_us": cu, "copy_spread_us": cs,
          "fold_gbps": round(nbytes / fu / 1e3, 1), "copy_gbps": round(2 * 2 * 2 * flat_in.numel() / cu / 1e3, 1),
          "unfolded_rows_copy_us": ru, "unfolded_rows_copy_spread_us": rs,
          "unfolded_rows_copy_gbps": round(2 * 2 * (Lq - sr) * 2 * DIM / ru / 1e3, 1)})


def step_rows(a, emit):
    import importlib
    model_mod = importlib.import_module("omnihuman-1-hack_amd.wan.modules.model")
    torch.manual_seed(0)
    m = model_mod.WanModel(model_type="t2v", dim=DIM, ffn_dim=8960, num_heads=H, num_layers=a.step_layers).cuda().train()
    m.set_causal_chunks(FPC, W, S)
    F = FPC * CHUNKS
    g = torch.Generator(device="cuda").manual_seed(2)
    x0, eps = ([torch.randn(16, F, 60, 104, device="cuda", generator=g)] for _ in range(2))
    ctx = [torch.randn(64, 4096, device="cuda", generator=g)]
    sig = torch.linspace(0.9, 0.1, CHUNKS, device="cuda")[None]

    def step(pin):
        def go():
            m.zero_grad(set_to_none=True)
            causal.forcing_loss(m, x0, eps, sig, 1000.0 * sig, ctx, pin_sink=pin).backward()
        return go
    (pu, ps), (uu, us) = alternate([step(True), step(False)], max(2, a.reps // 3), a.rounds, warm=1)
    emit({"step": f"forcing_loss forward + backward, {a.step_layers} layers of the 1.3B width, B = 1, {2 * F * TPF} tokens",
          "pinned_us": pu, "pinned_spread_us": ps, "unpinned_us": uu, "unpinned_spread_us": us,
          "pinned_over_unpinned": round(pu / uu, 3)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-layers", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pinned_tf_probe.txt"))
    a = ap.parse_args()
    lines = [f"# python tools/pinned_tf_probe.py --reps {a.reps} --rounds {a.rounds} --step-layers {a.step_layers}   (one MI355X; {H} "
             f"heads, groups of {CT} tokens, [{CHUNKS} clean | {CHUNKS} noisy] chunks, W = {W}, S = {S})"]

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    for part in (attention_rows, kernel_rows) + ((step_rows,) if a.step_layers > 0 else ()):
        part(a, emit)
        flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
