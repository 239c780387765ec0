"""The bound m = ceil(|q|max |k|max (1 + 2^-6)) that each self-attention launch of the benchmark's sampling steps hands to the
long-sequence stream (attention_w64.hip runs the stream without a running max where m <= 48): min and max over the step's
launches and (sample, head) pairs.  Same model, latent, prompts and scheduler as bench.py --gpus 1; reads the buffer each
self-attention layer keeps from its last launch (WanSelfAttention.last_qk_norm2_max).

    python tools/attn_bound_values.py [steps]
"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
PKG = bench.PKG
ops = importlib.import_module(PKG + ".ops")
sched_mod = importlib.import_module(PKG + ".wan.utils.fm_solvers_unipc")
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
device = torch.device("cuda", 0)
model = bench.build_model(device)
seq_len = 21 * 30 * 52
g = torch.Generator(device=device).manual_seed(100)
x = torch.randn((16, 21, 60, 104), device=device, generator=g)
ctx = torch.randn(120, 4096, device=device, generator=g)
ctx_null = torch.randn(40, 4096, device=device, generator=g)
st_c, st_u = model.encode_context([ctx]), model.encode_context([ctx_null])
sched = sched_mod.FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
sched.set_timesteps(50, device=device, shift=5.0)
sched.set_begin_index(0)
vals = []


def tap(sa):
    inner = sa._attend

    def attend(*args, **kw):
        o = inner(*args, **kw)
        vals.append(None if sa.last_qk_norm2_max is None else sa.last_qk_norm2_max.clone())
        return o
    sa._attend = attend


for blk in model.blocks:
    tap(blk.self_attn)
for i in range(steps):
    t = sched.timesteps[sched.step_index or 0].reshape(1).to(device)
    del vals[:]
    c, u = model.forward_cfg_pair([x], t, st_c, st_u, seq_len)
    have = [v for v in vals if v is not None]
    if not have:
        print(f"step {i}: {len(vals)} self-attention launches, none with a norm buffer", flush=True)
    else:
        m = torch.cat([torch.ceil(torch.sqrt(v[..., 0] * v[..., 1]) * (1.0 + 2.0 ** -6)).flatten() for v in have])
        print(f"step {i}: t = {float(t):.0f}  self-attention launches {len(vals)} (with a norm buffer: {len(have)})  "
              f"m over launches x heads: min {float(m.min()):.0f}  max {float(m.max()):.0f}  "
              f"over the limit of 48: {int((m > 48).sum())} of {m.numel()}", flush=True)
    x = sched.step_cfg(c[0], u[0], 5.0, x)
