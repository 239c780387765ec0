"""The three block-selection kernels (omh_block_pool_d128, omh_block_select, omh_block_mask_tables) against the fp64
restatement of the rule in tests/dyn_mask_ref.py, and sparse.block_mask_from_qk end to end.

A row (b, h, I) is *decided* in the fp64 reference when the mass at theta exceeds tau by more than delta = 1e-4, the mass
just before falls short by more than delta and the next smaller p lies below theta by more than delta * theta (fp32 dot
products of 128 terms and a hardware exp2 move p by about 2e-5 relative on these operands).  On decided rows the device
mask must equal the reference exactly; on the others the kept set must hold fp64 mass >= tau - delta; undecided rows are at
most 2 % of the live rows of a case (tests/test_block_policy_host.py holds the operands to that on the CPU)."""
import importlib

import pytest
import torch

import dyn_mask_ref as R
from conftest import PKG, rel_rms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sparse():
    return importlib.import_module(PKG + ".sparse")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


_OPERANDS = {}


def _case(name):
    """The operands of a select case, generated once (CPU) and left unchanged."""
    if name not in _OPERANDS:
        _OPERANDS[name] = R.case_operands(name)
    return _OPERANDS[name]


def _lens(lens):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")


def _tables_match(sparse, bm):
    """The device tables hold what sparse._lists makes of the same mask, in the entries that mean anything."""
    mask = bm.mask.cpu()
    for cnt, idx, m in ((bm.row_cnt, bm.row_idx, mask), (bm.col_cnt, bm.col_idx, mask.transpose(1, 2))):
        rc, ri = sparse._lists(m)
        assert torch.equal(cnt.cpu(), rc)
        used = torch.arange(m.shape[-1])[None, None, :] < rc[..., None]
        assert torch.equal(idx.cpu()[used], ri[used])


# ------------------------------------------------------------------------------------------------------------- pool
@pytest.mark.parametrize("B,H,S,lens", [(2, 2, 700, [700, 400]), (1, 12, 1560, None)])
def test_pool(sparse, B, H, S, lens):
    g = torch.Generator().manual_seed(S)
    x = (torch.randn(B, S, H, 128, generator=g) + 0.5).to(torch.bfloat16)
    mean, coh = sparse.pool_blocks(x.cuda().view(B * S, H * 128), B, S, H, H * 128, _lens(lens))
    torch.cuda.synchronize()
    rm, rc, c = R.pool(x, lens, torch.float64)
    nb = (S + 127) // 128
    assert mean.shape == (B, H, nb, 128) and coh.shape == (B, H, nb)
    # per block: 2e-5 x mean |x| over its live rows (twice the worst case of 128 fp32 additions)
    row_live = (torch.arange(nb * 128)[None] < (torch.tensor(lens) if lens is not None else torch.full((B,), S))[:, None])
    xa = torch.zeros(B, nb * 128, H, 128, dtype=torch.float64)
    xa[:, :S] = x.double().abs()
    xa = xa * row_live[..., None, None]
    mabs = xa.view(B, nb, 128, H, 128).sum((2, 4)).permute(0, 2, 1) / (c.clamp(min=1) * 128)[:, None, :]
    err = (mean.cpu().double() - rm).abs().amax(-1)
    print(f"pool {B}x{H}x{S}: worst mean error / mean|x| {float((err / mabs.clamp(min=1e-30))[:, :, :].max()):.2e}, "
          f"coherence error {float((coh.cpu().double() - rc).abs().max()):.2e}")
    assert bool((err <= 2e-5 * mabs).all())
    assert float((coh.cpu().double() - rc).abs().max()) < 1e-4
    dead = (c == 0)[:, None, :].expand(B, H, nb)
    assert bool((mean.cpu()[dead] == 0).all()) and bool((coh.cpu()[dead] == 1).all())
    if lens is not None:
        assert dead.any()


# ----------------------------------------------------------------------------------------------------------- select
def _select_case(sparse, name, mass, keep_diagonal):
    q, k, lens, _ = _case(name)
    pol = sparse.DynamicBlockPolicy(mass, keep_diagonal=keep_diagonal)
    bm = sparse.block_mask_from_qk(q.cuda(), k.cuda(), pol, _lens(lens), _lens(lens))
    nb = (q.shape[1] + 127) // 128
    always = torch.eye(nb, dtype=torch.bool) if keep_diagonal else None
    undecided, live = R.check_against(bm.mask.cpu(), q, k, mass, lens, lens, always)
    print(f"{name} mass {mass}: density {bm.density:.4f}, {undecided} of {live} live rows undecided")
    assert undecided <= R.UNDECIDED_CAP * live
    _tables_match(sparse, bm)
    return bm


@pytest.mark.parametrize("mass", [0.5, 0.9])
def test_select_one_clip_74_blocks(sparse, mass):
    """(1, 12, 9 360): 74 key blocks, more than one value per lane."""
    bm = _select_case(sparse, "one_clip_74_blocks", mass, False)
    assert (bm.heads, bm.q_blocks, bm.k_blocks) == (12, 74, 74)


@pytest.mark.parametrize("mass", [0.5, 0.9])
def test_select_batch_union(sparse, mass):
    """(2, 12, 1 560) with lens [1 560, 1 000]: the mask is the union over the samples (and the diagonal)."""
    _select_case(sparse, "batch_union_lens", mass, True)


def test_select_300_blocks(sparse):
    """(1, 2, 38 400) with 38 333 live positions: 300 blocks, five values per lane, a ragged last block."""
    _select_case(sparse, "300_blocks", 0.5, False)


def test_select_rectangular_per_head_always(sparse):
    """Lq 300, Lk 520, lens on both sides: query block 2 is dead in every sample and keeps only its always entries."""
    qf, kf = R.structured_qk(2, 1, 2, 21, 520)
    q, k = qf[:, :300].contiguous(), kf
    ql, kl = [200, 130], [520, 300]
    always = torch.zeros(2, 3, 5, dtype=torch.bool)
    always[0, 2, 4] = always[1, 0, 0] = always[1, 2, 1] = always[0, 1, 3] = True
    pol = sparse.DynamicBlockPolicy(0.5, always=always)
    bm = sparse.block_mask_from_qk(q.cuda(), k.cuda(), pol, _lens(ql), _lens(kl))
    mask = bm.mask.cpu()
    undecided, live = R.check_against(mask, q, k, 0.5, ql, kl, always)
    assert undecided <= R.UNDECIDED_CAP * live and live == 2 * (2 + 2)
    assert torch.equal(mask[:, 2], always[:, 2])                                 # the dead query block
    assert (bm.q_blocks, bm.k_blocks, bm.Lq, bm.Lk) == (3, 5, 300, 520)
    _tables_match(sparse, bm)


def test_select_min_coherence(sparse):
    """Four query blocks and four key blocks of pure noise (coherence ~ 1 / 128 against >= 0.5 elsewhere): at
    min_coherence = 0.3 those query blocks keep every key block and those key blocks are kept by every query block."""
    q, k = R.structured_qk(1, 1, 2, 31)
    g = torch.Generator().manual_seed(32)
    # (one lattice block spans all four column groups, which holds its coherence near 0.35: a per-head offset shared by
    # every token lifts the structured blocks above 0.5, clear of the threshold)
    u = 2.0 * torch.randn(1, 1, 2, 128, generator=g)
    q, k = (q.float() + u).to(torch.bfloat16), (k.float() + u).to(torch.bfloat16)
    qb, kb = [1, 4, 7, 12], [0, 3, 8, 11]
    for I in qb:
        n = q[:, I * 128:(I + 1) * 128].shape[1]
        q[:, I * 128:(I + 1) * 128] = torch.randn(1, n, 2, 128, generator=g).to(torch.bfloat16)
    for J in kb:
        n = k[:, J * 128:(J + 1) * 128].shape[1]
        k[:, J * 128:(J + 1) * 128] = torch.randn(1, n, 2, 128, generator=g).to(torch.bfloat16)
    _, qc, _ = R.pool(q)
    _, kc, _ = R.pool(k)
    assert not ((qc - 0.3).abs() < 1e-3).any() and not ((kc - 0.3).abs() < 1e-3).any()      # nobody near the threshold
    assert bool((qc[..., qb] < 0.05).all()) and bool((kc[..., kb] < 0.05).all())
    assert int((qc < 0.5).sum()) == 8 and int((kc < 0.5).sum()) == 8                          # (4 blocks x 2 heads each)
    pol = sparse.DynamicBlockPolicy(0.5, min_coherence=0.3, keep_diagonal=False)
    mask = sparse.block_mask_from_qk(q.cuda(), k.cuda(), pol).mask.cpu()
    undecided, live = R.check_against(mask, q, k, 0.5, min_coherence=0.3)
    assert undecided <= R.UNDECIDED_CAP * live
    assert bool(mask[:, qb].all()) and bool(mask[:, :, kb].all()) and not bool(mask.all())
    # the same call without the coherence rule keeps less
    plain = sparse.block_mask_from_qk(q.cuda(), k.cuda(), sparse.DynamicBlockPolicy(0.5, keep_diagonal=False)).mask.cpu()
    assert bool((mask | plain == mask).all()) and int(plain.sum()) < int(mask.sum())


def test_select_mass_one_keeps_every_live_block(sparse):
    q, k, lens, _ = _case("batch_union_lens")
    bm = sparse.block_mask_from_qk(q.cuda(), k.cuda(), sparse.DynamicBlockPolicy(1.0, keep_diagonal=False), _lens(lens), _lens(lens))
    c = R.live_counts(q.shape[1], lens, q.shape[0]) > 0
    want = (c[:, :, None] & c[:, None, :]).any(0)
    assert torch.equal(bm.mask.cpu(), want[None].expand(12, -1, -1))
    assert abs(bm.density - float(want.float().mean())) < 1e-7


def test_select_repeats_bit_for_bit(sparse):
    q, k, lens, _ = _case("one_clip_74_blocks")
    qd, kd = q.cuda(), k.cuda()
    pol = sparse.DynamicBlockPolicy(0.9)
    a = sparse.block_mask_from_qk(qd, kd, pol)
    b = sparse.block_mask_from_qk(qd, kd, pol)
    assert torch.equal(a.mask, b.mask) and torch.equal(a.row_cnt, b.row_cnt) and torch.equal(a.col_cnt, b.col_cnt)
    used = torch.arange(74, device="cuda")[None, None, :] < a.row_cnt[..., None]
    assert torch.equal(a.row_idx[used], b.row_idx[used])
    pa, pb = sparse.pool_blocks(qd.view(-1, 1536), 1, 9360, 12, 1536), sparse.pool_blocks(qd.view(-1, 1536), 1, 9360, 12, 1536)
    assert torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1])


# ----------------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("shape", [(1, 3, 5), (2, 13, 13), (12, 74, 74), (2, 300, 300)])
def test_tables_against_lists(sparse, shape):
    g = torch.Generator().manual_seed(sum(shape))
    mask = torch.rand(*shape, generator=g) < 0.3
    mask[-1, 0] = True                                                           # a full row (but for the column below)
    mask[0, 1] = False                                                           # an empty row, an empty column
    mask[:, :, 2] = False
    bm = sparse.tables_from_mask(mask.cuda(), shape[1] * 128 - 5, shape[2] * 128)
    assert torch.equal(bm.mask.cpu(), mask) and (bm.heads, bm.q_blocks, bm.k_blocks) == shape
    _tables_match(sparse, bm)
    assert int(bm.row_cnt[0, 1]) == 0 and int(bm.col_cnt[0, 2]) == 0 and int(bm.row_cnt[-1, 0]) == shape[2] - 1


# ------------------------------------------------------------------------------------------------------- end to end
def test_block_mask_from_qk_end_to_end(sparse, ops):
    """(2, 2, 320) with k_lens [320, 150]: the device-built mask drives ops.flash_attn within the block-sparse bounds of
    a dense-masked fp32 softmax under that same mask, and flash_attention(block_mask=policy) is, bit for bit in the
    output and the gradients, flash_attention(block_mask=that mask)."""
    attn = importlib.import_module(PKG + ".wan.modules.attention")
    B, H, S = 2, 2, 320
    g = torch.Generator().manual_seed(77)
    q, k, v = (torch.randn(B, S, H, 128, generator=g).to(torch.bfloat16).cuda() for _ in range(3))
    kl = torch.tensor([320, 150], dtype=torch.int32, device="cuda")
    pol = sparse.DynamicBlockPolicy(0.6)
    bm = sparse.block_mask_from_qk(q, k, pol, k_lens=kl)
    mask = bm.mask.cpu()
    assert not bool(mask.all()) and bool(mask[:, torch.arange(3), torch.arange(3)].all())
    vt = torch.zeros(B, H * 128, 320, dtype=torch.bfloat16, device="cuda")
    vt[:, :, :S] = v.reshape(B, S, H * 128).transpose(1, 2)
    out = ops.flash_attn(q, k, vt, kl, block_mask=bm).float().cpu()
    dense = mask.repeat_interleave(128, 1).repeat_interleave(128, 2)[:, :S, :S]
    ref = torch.zeros(B, S, H, 128)
    for b in range(B):
        vis = dense.clone()
        vis[:, :, int(kl[b]):] = False
        s = torch.einsum("qhd,khd->hqk", q[b].float().cpu(), k[b].float().cpu()) * 128 ** -0.5
        p = torch.nan_to_num(torch.softmax(s.masked_fill(~vis, float("-inf")), dim=-1), nan=0.0)
        ref[b] = torch.einsum("hqk,khd->qhd", p, v[b].float().cpu())
    err, worst = rel_rms(out, ref), float((out - ref).abs().max())
    print(f"end to end: density {bm.density:.3f}, rel-RMS {err:.2e}, max abs {worst:.2e}")
    assert err < 8e-3 and worst < 3e-2

    def run(block_mask):
        qs, ks, vs = (t.clone().requires_grad_(True) for t in (q, k, v))
        o = attn.flash_attention(qs, ks, vs, k_lens=kl, block_mask=block_mask)
        o.float().square().sum().backward()
        return o.detach(), qs.grad, ks.grad, vs.grad
    for a, b in zip(run(pol), run(bm)):
        assert torch.equal(a, b)
    with torch.no_grad():
        assert torch.equal(attn.flash_attention(q, k, v, k_lens=kl, block_mask=pol),
                           attn.attention(q, k, v, k_lens=kl, block_mask=bm))
    with pytest.raises(ValueError):
        attn.flash_attention(q, k, v, k_lens=kl, block_mask=pol, causal=True)
