"""Block-sparse attention (128 x 128 block masks), forward and backward: omh_flash_attn_fwd_sparse_d128 /
omh_flash_attn_bwd_sparse_d128 through ``ops.flash_attn(block_mask=)``, ``flash_attention(block_mask=)`` and
``ops.flash_attn_func(block_mask=)`` against autograd through a dense-masked fp32 softmax attention on the same bf16
operands (built as ``_reference`` of test_gpu_attn_band_bwd.py is).  Query i of sample b, head h sees key j iff
``M[h][i // 128][j // 128]``, ``j < k_lens[b]`` and ``i < q_lens[b]``.

Bounds: the project's own for this arithmetic (P and the output in bf16): forward rel-RMS < 8e-3 and max abs error
< 3e-2 (test_gpu_kernels.py), attention gradients rel-RMS < 1.2e-2 (test_gpu_attn_band_bwd.py)."""
import importlib

import pytest
import torch

from conftest import PKG, rel_rms, set_option

pytestmark = pytest.mark.gpu
LOG2E = 1.4426950408889634
FWD_RMS, FWD_MAX, GRAD_RMS = 8e-3, 3e-2, 1.2e-2


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


@pytest.fixture(scope="module")
def sparse():
    return importlib.import_module(PKG + ".sparse")


@pytest.fixture(scope="module")
def attn_mod():
    return importlib.import_module(PKG + ".wan.modules.attention")


def _random_mask(shape, seed, diagonal=False):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(*shape, generator=g) < 0.5
    if diagonal:
        i = torch.arange(min(shape[-2:]))
        m[..., i, i] = True
    return m


def _mask_of(name, sparse):
    if name == "tri":                                    # the simplest: lists of length 1 and 2
        return torch.tensor([[1, 0], [1, 1]], dtype=torch.bool)
    if name == "head_random_diag":                       # per head, p = 0.5, diagonal forced
        return _random_mask((2, 3, 3), 1, diagonal=True)
    if name == "empty_row":                              # query block 1 keeps nothing; key block 0 kept only by query block 2
        return torch.tensor([[0, 1, 1], [0, 0, 0], [1, 0, 1]], dtype=torch.bool)
    if name == "rect_random":                            # shared, nQb 3 != nKb 5
        return _random_mask((3, 5), 2)
    if name == "head_random_rect":                       # per head, 2 x 3 blocks
        return _random_mask((2, 2, 3), 3)
    if name == "window3d":                               # 13 blocks, 12 heads: even heads a spatial window, odd heads a strip
        even = sparse.block_mask_from_3d_window((1, 30, 52), (0, 6, 52))
        odd = sparse.block_mask_from_3d_window((1, 30, 52), (0, 30, 8))
        return torch.stack([even if h % 2 == 0 else odd for h in range(12)])
    raise KeyError(name)


CASES = [
    # B, H, Lq, Lk, k_lens, q_lens, mask
    (1, 2, 256, 256, None, None, "tri"),
    (2, 2, 320, 320, [320, 150], None, "head_random_diag"),   # klen 150: block 1's second tile dead, block 2 kept but dead
    (2, 2, 320, 320, [288, 120], None, "empty_row"),          # empty rows; a key column reached by one partial query block
    (1, 2, 300, 520, None, None, "rect_random"),              # Lq != Lk: the transposed lists
    (1, 2, 130, 333, [200], [100], "head_random_rect"),       # q_lens: NaN dout past row 100, dead query block 1
    (4, 12, 1560, 1560, [1560, 1560, 1000, 1560], None, "window3d"),   # 12 heads through xcd_remap, ragged batch
]
_CACHE = {}


def _dense(mask, Lq, Lk):
    """[Hm, nQb, nKb] block mask -> [Hm, Lq, Lk] element mask."""
    m = mask if mask.dim() == 3 else mask[None]
    return m.repeat_interleave(128, 1).repeat_interleave(128, 2)[:, :Lq, :Lk]


def _case(idx, sparse):
    """Inputs, the fp32 reference (output, lse liveness, gradients) — computed once per case and left unchanged."""
    if idx in _CACHE:
        return _CACHE[idx]
    B, H, Lq, Lk, klens, qlens, mname = CASES[idx]
    g = torch.Generator(device="cuda").manual_seed(100 + idx)
    q, k, v = (torch.randn(B, L, H, 128, device="cuda", generator=g).bfloat16() for L in (Lq, Lk, Lk))
    do = torch.randn(B, Lq, H, 128, device="cuda", generator=g).bfloat16()
    mask = _mask_of(mname, sparse)
    vis = _dense(mask, Lq, Lk).cuda()[None].expand(B, -1, -1, -1).clone()          # [B, Hm, Lq, Lk]
    for b in range(B):
        if klens is not None:
            vis[b, :, :, klens[b]:] = False
        if qlens is not None:
            vis[b, :, qlens[b]:, :] = False
            do[b, qlens[b]:] = float("nan")                                        # nothing may depend on those rows
    qr, kr, vr = (t.float().transpose(1, 2).detach().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bhid,bhjd->bhij", qr, kr) * 128 ** -0.5
    s = s.masked_fill(~vis, float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)                         # rows that see no key
    out = torch.einsum("bhij,bhjd->bhid", p, vr)
    out.backward(torch.nan_to_num(do.float(), nan=0.0).transpose(1, 2))
    ref = dict(out=out.detach().transpose(1, 2).contiguous(),
               grads=tuple(t.grad.transpose(1, 2).contiguous() for t in (qr, kr, vr)),
               row_live=vis.any(3).expand(B, H, Lq).contiguous(),                  # [B, H, Lq]: the row sees a key
               key_live=vis.any(2).expand(B, H, Lk).contiguous())                  # [B, H, Lk]: a live query sees the key
    del s, p, out, vis
    kl = None if klens is None else torch.tensor(klens, dtype=torch.int32, device="cuda")
    ql = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device="cuda")
    _CACHE[idx] = (q, k, v, do, kl, ql, mask, ref)
    return _CACHE[idx]


def _vt(v):
    B, Lk, H, D = v.shape
    Lp = (Lk + 63) // 64 * 64
    vt = torch.zeros(B, H * D, Lp, device="cuda", dtype=torch.bfloat16)
    vt[:, :, :Lk] = v.reshape(B, Lk, H * D).transpose(1, 2)
    return vt


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_block_sparse_forward(ops, sparse, attn_mod, idx):
    B, H, Lq, Lk = CASES[idx][:4]
    q, k, v, do, kl, ql, mask, ref = _case(idx, sparse)
    bm = sparse.BlockMask(mask, Lq, Lk)
    lse = torch.full((B, H, Lq), float("nan"), device="cuda")
    o = ops.flash_attn(q, k, _vt(v), kl, q_lens=ql, block_mask=bm, lse=lse)
    err_rms, err_max = rel_rms(o, ref["out"]), float((o.float() - ref["out"]).abs().max())
    print(f"case {idx}: density {bm.density:.3f} forward rel-RMS {err_rms:.2e} max abs {err_max:.2e}")
    assert torch.isfinite(o.float()).all()
    assert err_rms < FWD_RMS and err_max < FWD_MAX
    # rows that see no key: exact zeros and lse = -inf; every other row a finite lse
    live = ref["row_live"]                                                   # [B, H, Lq]
    assert float(o.float().transpose(1, 2)[~live].abs().sum()) == 0.0
    assert bool((lse[~live] == float("-inf")).all()) and bool(torch.isfinite(lse[live]).all())
    # the wrapper with the reference's signature (a raw bool mask), and a second run: the same bits
    with torch.no_grad():
        ow = attn_mod.flash_attention(q, k, v, q_lens=ql, k_lens=kl, block_mask=mask)
    assert torch.equal(ow, o)
    assert torch.equal(ops.flash_attn(q, k, _vt(v), kl, q_lens=ql, block_mask=bm), o)


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_block_sparse_backward(ops, sparse, idx):
    B, H, Lq, Lk = CASES[idx][:4]
    q, k, v, do, kl, ql, mask, ref = _case(idx, sparse)

    def run():
        qg, kg, vg = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        ops.flash_attn_func(qg, kg, vg, kl, ql, block_mask=mask).backward(do)
        return qg.grad, kg.grad, vg.grad

    got = run()
    for name, gt, rf in zip(("dq", "dk", "dv"), got, ref["grads"]):
        err = rel_rms(gt, rf)
        print(f"case {idx}: {name} rel-RMS {err:.2e}")
        assert torch.isfinite(gt.float()).all()
        assert err < GRAD_RMS, name
    # rows that see no key (dead queries included) and keys no live query sees: exact zeros, written
    assert float(got[0].float().transpose(1, 2)[~ref["row_live"]].abs().sum()) == 0.0
    dead_k = ~ref["key_live"]
    assert float(got[1].float().transpose(1, 2)[dead_k].abs().sum()) == 0.0
    assert float(got[2].float().transpose(1, 2)[dead_k].abs().sum()) == 0.0
    for a, b in zip(run(), got):                                             # no atomics: repeatable bit for bit
        assert torch.equal(a, b)


def test_forward_is_the_plain_kernel_on_the_kept_blocks(ops, sparse):
    """Exactness without an oracle: the masked output rows of (head, query block) equal, bit for bit, the plain
    short-sequence kernel on those 128 rows against the ascending concatenation of the kept key blocks' K and V — the
    same sequence of key tiles."""
    B, H, Lq, Lk = 1, 2, 384, 512
    g = torch.Generator(device="cuda").manual_seed(7)
    q, k, v = (torch.randn(B, L, H, 128, device="cuda", generator=g).bfloat16() for L in (Lq, Lk, Lk))
    mask = _random_mask((H, 3, 4), 5)
    o = ops.flash_attn(q, k, _vt(v), block_mask=mask)
    set_option("OMH_ATTN_KERNEL", "base")
    for h in range(H):
        for i in range(3):
            kept = [j for j in range(4) if mask[h, i, j]]
            rows = o[:, 128 * i:128 * (i + 1), h]
            if not kept:
                assert float(rows.float().abs().sum()) == 0.0
                continue
            sel = torch.cat([torch.arange(128 * j, 128 * (j + 1)) for j in kept]).cuda()
            qs = q[:, 128 * i:128 * (i + 1), h:h + 1].contiguous()
            ks, vs = k[:, sel, h:h + 1].contiguous(), v[:, sel, h:h + 1].contiguous()
            assert torch.equal(ops.flash_attn(qs, ks, _vt(vs))[:, :, 0], rows), (h, i)


def test_all_true_mask_is_full_attention(ops, sparse):
    """Forward: the unmasked short-sequence kernel's bits.  Backward: the unmasked call runs other kernels (the w64
    streams) on the same mathematics — within rel-RMS 2e-3, the project's figure for that."""
    B, H, Lq, Lk, klens = 2, 2, 300, 300, [300, 170]
    g = torch.Generator(device="cuda").manual_seed(9)
    q, k, v = (torch.randn(B, L, H, 128, device="cuda", generator=g).bfloat16() for L in (Lq, Lk, Lk))
    do = torch.randn(B, Lq, H, 128, device="cuda", generator=g).bfloat16()
    kl = torch.tensor(klens, dtype=torch.int32, device="cuda")
    mask = torch.ones(3, 3, dtype=torch.bool)
    o = ops.flash_attn(q, k, _vt(v), kl, block_mask=mask)
    set_option("OMH_ATTN_KERNEL", "base")
    assert torch.equal(o, ops.flash_attn(q, k, _vt(v), kl))
    grads = []
    for m in (mask, None):
        qg, kg, vg = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        ops.flash_attn_func(qg, kg, vg, kl, block_mask=m).backward(do)
        grads.append((qg.grad, kg.grad, vg.grad))
    for a, b in zip(*grads):
        assert rel_rms(a, b) < 2e-3


@pytest.mark.parametrize("idx", [1, 2])
def test_block_sparse_backward_modes(ops, sparse, idx):
    """bf16 outputs and q_prescaled agree with the plain call; phases 1 + 2 + 3 give phase 0's bits."""
    B, H, Lq, Lk = CASES[idx][:4]
    q4, k4, v4, do4, kl, ql, mask, _ = _case(idx, sparse)
    d = H * 128
    q, k, v, do = q4.view(B * Lq, d), k4.view(B * Lk, d), v4.view(B * Lk, d), do4.view(B * Lq, d)
    bm = sparse.BlockMask(mask, Lq, Lk)
    vt = _vt(v4)

    def forward(qq, pre):
        o = torch.empty(B * Lq, d, device="cuda", dtype=torch.bfloat16)
        o32 = torch.empty(B * Lq, d, device="cuda", dtype=torch.float32)
        lse = torch.empty(B, H, Lq, device="cuda", dtype=torch.float32)
        ops.flash_attn_raw(ops.ptr(qq), ops.ptr(k), ops.ptr(vt), ops.ptr(o), ops.ptr(kl), B, H, Lq, Lk, Lq * d, d, Lk * d, d,
                           d * vt.shape[2], Lq * d, d, vt.shape[2], 128 ** -0.5, lse=ops.ptr(lse), q_prescaled=pre,
                           o32=ops.ptr(o32), block_mask=bm)
        return o, o32, lse

    o, o32, lse = forward(q, 0)
    dq, dk, dv = ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, o32=o32, block_mask=bm)
    out = tuple(torch.empty(B * L, d, device="cuda", dtype=torch.bfloat16) for L in (Lq, Lk, Lk))
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, o32=o32, block_mask=bm, out=out)
    for got, ref in zip(out, (dq, dk, dv)):
        assert rel_rms(got.float(), ref) < 8e-3
    qp = (q.float() * (128 ** -0.5 * LOG2E)).bfloat16()
    op, o32p, lsep = forward(qp, 1)
    gp = ops.flash_attn_bwd(qp, k, v, op, do, lsep, kl, B, H, Lq, Lk, q_prescaled=True, o32=o32p, block_mask=bm)
    for got, ref in zip(gp, (dq, dk, dv)):
        assert rel_rms(got, ref) < GRAD_RMS
    delta = torch.empty(B, H, Lq, device="cuda", dtype=torch.float32)
    kw = dict(o32=o32, block_mask=bm, delta=delta)
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, phase=1, out=None, **kw)
    ph = [torch.full((B * L, d), float("nan"), device="cuda", dtype=torch.bfloat16) for L in (Lq, Lk, Lk)]
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, phase=3, out=tuple(ph), **kw)
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, phase=2, out=tuple(ph), **kw)
    for a, b in zip(ph, out):
        assert torch.equal(a, b)


def test_mask_refuses_causal_and_window(ops, attn_mod):
    q = torch.randn(1, 256, 2, 128, device="cuda").bfloat16()
    mask = torch.ones(2, 2, dtype=torch.bool)
    with pytest.raises(ValueError):
        attn_mod.flash_attention(q, q, q, causal=True, block_mask=mask)
    with pytest.raises(ValueError):
        attn_mod.flash_attention(q, q, q, window_size=(16, 16), block_mask=mask)
    with pytest.raises(ValueError):
        ops.flash_attn_func(q, q, q, window=(16, -1), block_mask=mask)
    with pytest.raises(ValueError):
        ops.flash_attn(q, q, _vt(q), window=(-1, 0), block_mask=mask)
    with pytest.raises(ValueError):                                              # 3 heads on a 2-head call
        ops.flash_attn(q, q, _vt(q), block_mask=torch.ones(3, 2, 2, dtype=torch.bool))
    with pytest.raises(ValueError):                                              # block counts of another length
        ops.flash_attn(q, q, _vt(q), block_mask=torch.ones(3, 3, dtype=torch.bool))
