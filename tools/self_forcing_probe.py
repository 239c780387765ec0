"""Self forcing: the cached attention backward and a few-step rollout with gradients.

    python tools/self_forcing_probe.py [--reps 10] [--rounds 3] [--skip-model] [--out profiles/self_forcing_probe.txt]

Attention level (one JSON line per chunk I = 0 .. 6, also written to --out): random operands, 12 heads, chunks of 3 latent
frames at 480 x 832 (4 680 tokens); the queries of chunk I against I cached chunks and itself.
  ``cached_us``  omh_flash_attn_bwd_cached_d128, own_lo = 4 680 I: dQ over all keys, dK / dV for the chunk's own rows;
  ``plain_us``   omh_flash_attn_bwd_d128 phase 0 over the same operands and ALL keys (dK / dV of the cached rows computed
                 and thrown away: what the block backward would cost without the new entry);
  ``assemble_us`` K (a strided copy) and V (a transpose of the cache's V^T) of the cached rows plus the chunk's own rows
                 into the contiguous [Lk, d] buffers the dQ pass reads — what ``_cached_kv`` (model_train.py) launches.
The variants alternate in ONE process as in tools/attn_interval_probe.py: ``*_us`` is the middle one of --rounds medians of
--reps runs, ``*_spread_us`` their max - min.

Model level (one line; skipped with --skip-model): Wan2.1-T2V-1.3B, random init, 21 latent frames 480 x 832,
``causal.self_forcing_rollout(frames_per_chunk=3, 4 steps, exit at the last step)`` and ``backward()`` of an MSE loss:
milliseconds per rollout forward and per backward (the second of two runs), peak memory."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from attn_interval_probe import CHUNKS, D, FPC, H, LOG2E, TPF, alternate, causal, ops  # noqa: E402


class Operands:
    """Chunk I's queries, a cache-like K [cap, d] / V^T [d, pitch] holding I + 1 chunks, and the forward's lse / o32."""

    def __init__(self, I):
        C, d = TPF * FPC, H * D
        self.C, self.d, self.I = C, d, I
        self.Lk = Lk = (I + 1) * C
        g = torch.Generator(device="cuda").manual_seed(I)
        self.q = (torch.randn(C, d, device="cuda", generator=g) * (D ** -0.5 * LOG2E)).bfloat16()
        self.k, self.v, self.do = (torch.randn(n, d, device="cuda", generator=g).bfloat16() for n in (Lk, Lk, C))
        self.pitch = (Lk + 63) // 64 * 64
        self.vt = torch.zeros(1, d, self.pitch, device="cuda", dtype=torch.bfloat16)
        self.vt[:, :, :Lk] = self.v.view(1, Lk, d).transpose(1, 2)
        self.o = torch.empty(C, d, device="cuda", dtype=torch.bfloat16)
        self.o32 = torch.empty(C, d, device="cuda", dtype=torch.float32)
        self.lse = torch.empty(1, H, C, device="cuda", dtype=torch.float32)
        ops.flash_attn_raw(ops.ptr(self.q), ops.ptr(self.k), ops.ptr(self.vt), ops.ptr(self.o), None, 1, H, C, Lk, C * d, d,
                           Lk * d, d, d * self.pitch, C * d, d, self.pitch, D ** -0.5, lse=ops.ptr(self.lse), q_prescaled=1,
                           o32=ops.ptr(self.o32), flags=ops.ATTN_SHORT_KERNEL)
        bf = lambda n: torch.empty(n, d, device="cuda", dtype=torch.bfloat16)
        self.out_own = (bf(C), bf(C), bf(C))
        self.out_all = (bf(C), bf(Lk), bf(Lk))
        self.k_own, self.v_own = self.k[I * C:].clone(), self.v[I * C:].clone()
        self.k_full, self.v_full = bf(Lk), bf(Lk)

    def cached(self):
        ops.flash_attn_bwd(self.q, self.k, self.v, self.o, self.do, self.lse, None, 1, H, self.C, self.Lk, D ** -0.5,
                           q_prescaled=True, out=self.out_own, o32=self.o32, own_lo=self.I * self.C)

    def plain(self):
        ops.flash_attn_bwd(self.q, self.k, self.v, self.o, self.do, self.lse, None, 1, H, self.C, self.Lk, D ** -0.5,
                           q_prescaled=True, out=self.out_all, o32=self.o32)

    def assemble(self):
        past, C, d = self.I * self.C, self.C, self.d
        if past == 0:
            return                                           # the own copies ARE the operands
        self.k_full[:past].copy_(self.k[:past])
        self.k_full[past:].copy_(self.k_own)
        ops.transpose_bf16_raw(ops.ptr(self.vt), ops.ptr(self.v_full), d, past, self.pitch, d)
        self.v_full[past:].copy_(self.v_own)


def model_level():
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    m = bench.build_model("cuda").train().requires_grad_(True)
    F, steps = FPC * CHUNKS, 4
    g = torch.Generator(device="cuda").manual_seed(0)
    noise = [torch.randn(16, F, 60, 104, device="cuda", generator=g)]
    target = torch.randn(16, F, 60, 104, device="cuda", generator=g)
    ctx = [torch.randn(77, 4096, device="cuda", generator=g)]
    sig = [1.0, 0.9375, 0.8333, 0.625]
    row = {}
    for run in range(2):
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        clip = causal.self_forcing_rollout(m, noise, ctx, frames_per_chunk=FPC, sigmas=sig, timesteps=[1000 * s for s in sig],
                                           exit_step=steps - 1, generator=g)
        ev[1].record()
        torch.nn.functional.mse_loss(clip[0], target).backward()
        ev[2].record()
        torch.cuda.synchronize()
        row = {"model": "Wan2.1-T2V-1.3B random init", "latent": [16, F, 60, 104], "frames_per_chunk": FPC, "steps": steps,
               "exit_step": steps - 1, "rollout_forward_ms": round(ev[0].elapsed_time(ev[1]), 1),
               "backward_ms": round(ev[1].elapsed_time(ev[2]), 1),
               "peak_memory_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
               "grads_finite": bool(all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None))}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "self_forcing_probe.txt"))
    a = ap.parse_args()
    C = TPF * FPC
    lines = [f"# python tools/self_forcing_probe.py --reps {a.reps} --rounds {a.rounds}   (one MI355X; {H} heads, chunks of {C} "
             f"tokens; chunk I against I cached chunks)"]
    for I in range(CHUNKS):
        x = Operands(I)
        (cu, cs), (pu, ps), (au, as_) = alternate([x.cached, x.plain, x.assemble], a.reps, a.rounds)
        lines.append(json.dumps({"chunk": I, "Lq": C, "Lk": x.Lk, "own_lo": I * C, "cached_us": cu, "cached_spread_us": cs,
                                 "plain_us": pu, "plain_spread_us": ps, "assemble_us": au, "assemble_spread_us": as_,
                                 "cached_plus_assemble_over_plain": round((cu + au) / pu, 3)}))
        print(lines[-1], flush=True)
        del x
    if not a.skip_model:
        lines.append(json.dumps(model_level()))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
