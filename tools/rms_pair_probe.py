"""us per launch of omh_rmsnorm_rope_bf16_pair at the headline's shape (32 760 rows x 2 x 1 536), the two forms interleaved, and
of omh_rmsnorm_rope_bf16_pair_bound (also emits max |q|^2, |k|^2 per head) in its forms, on the same buffers: "bound/row" the
one-wave-per-row form (option RMS_PAIR_BOUND = "0"), "bound" the persistent form (the default), "bound/nopf" the persistent
form without its next-row prefetch ("2").  "+zero": the buffer is zeroed by a fill kernel before every launch, as the model
did before it took its slices from one buffer per forward; the other bound legs time the norm kernel alone."""
import importlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
ops = importlib.import_module("omnihuman-1-hack_amd.ops")
rows, d, D = 32760, 1536, 128
qk = (torch.randn(rows, 2 * d, device="cuda") * 1.3).bfloat16()
wq, wk = torch.rand(d, device="cuda") + 0.5, torch.rand(d, device="cuda") + 0.5
ang = torch.rand(1024, D // 2) * 6.28                        # (any table: timing only)
cos, sin = torch.cos(ang).float().cuda(), torch.sin(ang).float().cuda()
grid = torch.tensor([(21, 30, 52)], dtype=torch.int32, device="cuda")
q, k = torch.empty(rows, d, dtype=torch.bfloat16, device="cuda"), torch.empty(rows, d, dtype=torch.bfloat16, device="cuda")
def plain(): ops.rmsnorm_rope_bf16_pair_raw(ops.ptr(qk), 2 * d, d, ops.ptr(q), ops.ptr(k), rows, d, ops.ptr(wq), ops.ptr(wk), 1e-6, 1,
                                            ops.ptr(cos), ops.ptr(sin), 1024, D, ops.ptr(grid), rows, out_scale0=0.1275, out_scale1=1.0)
nm = torch.zeros(1, d // D, 2, device="cuda")
def bound():
    ops.rmsnorm_rope_bf16_pair_bound_raw(ops.ptr(qk), 2 * d, d, ops.ptr(q), ops.ptr(k), rows, d, ops.ptr(wq), ops.ptr(wk), 1e-6, 1,
                                         ops.ptr(cos), ops.ptr(sin), 1024, D, ops.ptr(grid), rows, ops.ptr(nm), out_scale0=0.1275,
                                         out_scale1=1.0)
def bound_zero():
    nm.zero_()
    bound()
# leg -> (RMS_PAIR_ROW, RMS_PAIR_BOUND, what runs)
LEGS = {"pair/two_wg": ("0", None, plain), "pair/row": ("1", None, plain), "bound/row+zero": (None, "0", bound_zero),
        "bound/row": (None, "0", bound), "bound+zero": (None, None, bound_zero), "bound": (None, None, bound),
        "bound/nopf": (None, "2", bound)}
for rep in range(int(os.environ.get("REPS", "3"))):
    for leg, (pair_row, pair_bound, run) in LEGS.items():
        ops.set_option("RMS_PAIR_ROW", pair_row)
        ops.set_option("RMS_PAIR_BOUND", pair_bound)
        for _ in range(5): run()
        torch.cuda.synchronize(); s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True); s.record()
        for _ in range(50): run()
        e.record(); torch.cuda.synchronize(); us = s.elapsed_time(e) / 50 * 1e3
        print(f"{leg:15s} {us:.1f} us  {4.0 * rows * d * 2 / us / 1e6:.2f} TB/s", flush=True)
    # the bound forms on a buffer that holds zeros, as in the model, the fill outside the timed span: one event pair per launch
    for leg, pair_bound in (("bound/row", "0"), ("bound", None)):
        ops.set_option("RMS_PAIR_ROW", None)
        ops.set_option("RMS_PAIR_BOUND", pair_bound)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
        for s, e in ev:
            nm.zero_(); s.record(); bound(); e.record()
        torch.cuda.synchronize()
        us = sorted(s.elapsed_time(e) * 1e3 for s, e in ev)
        print(f"{leg:15s} {us[len(us) // 2]:.1f} us median of single launches on fresh zeros (min {us[0]:.1f})", flush=True)
