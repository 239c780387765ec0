"""ms per launch of the long-sequence self-attention at the benchmark shape (12 heads x 32 760^2, D = 128, q pre-scaled as the
norm kernel leaves it): the plain entry (stream V2) against the bounded entry (stream V4 where the bound allows), interleaved
rounds on one box.  A library without the bounded entry (an older checkout) times the plain entry alone."""
import importlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
ops = importlib.import_module("omnihuman-1-hack_amd.ops")
D, S, H = 128, int(os.environ.get("S", 32760)), 12
amp = float(os.environ.get("AMP", 1.0))           # AMP=4: the bound exceeds the limit, the bounded entry runs V2 (the fallback's cost)
q = (torch.randn(1, S, H, D, device="cuda") * amp * (D ** -0.5 * 1.4426950408889634)).to(torch.bfloat16)
k = (torch.randn(1, S, H, D, device="cuda") * amp).to(torch.bfloat16)
Sp = (S + 63) // 64 * 64
vt = torch.zeros(1, H * D, Sp, dtype=torch.bfloat16, device="cuda")
vt[:, :, :S] = torch.randn(1, H * D, S, device="cuda").to(torch.bfloat16)
o = torch.empty_like(q)
nm = torch.stack([q.float().pow(2).sum(-1).amax(1), k.float().pow(2).sum(-1).amax(1)], -1).contiguous()
print("m per head:", torch.ceil(torch.sqrt(nm[..., 0] * nm[..., 1]) * (1 + 2.0 ** -6)).flatten().tolist())
ops.set_option("OMH_ATTN_KERNEL", "w64")
modes = ["plain"] + (["bounded"] if hasattr(ops, "rmsnorm_rope_bf16_pair_bound_raw") else [])


def run(mode):
    kw = {"qk_norm2_max": ops.ptr(nm)} if mode == "bounded" else {}
    ops.flash_attn_raw(ops.ptr(q), ops.ptr(k), ops.ptr(vt), ops.ptr(o), None, 1, H, S, S, q.stride(0), q.stride(1), k.stride(0),
                       k.stride(1), vt.stride(0), o.stride(0), o.stride(1), vt.stride(1), D ** -0.5, q_prescaled=1, **kw)


res = {m: [] for m in modes}
for rnd in range(3):
    for m in modes:
        for _ in range(2):
            run(m)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(8):
            run(m)
        e.record(); torch.cuda.synchronize()
        res[m].append(s.elapsed_time(e) / 8)
for m in modes:
    ms = sorted(res[m])[1]
    print(f"{m}: median {ms:.4f} ms  {4.0 * S * S * H * D / ms / 1e9:.1f} TF   all {['%.3f' % x for x in res[m]]}", flush=True)
