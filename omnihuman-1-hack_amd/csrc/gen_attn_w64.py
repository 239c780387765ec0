#!/usr/bin/env python3
"""Generator of the instruction streams of ``flash_attn_fwd_d128_w64_kernel<V>`` (attention_w64.hip).

The long-sequence attention kernel of round 2: 4 waves x 64 query rows per workgroup, ONE wave per SIMD owning
the whole 512-entry register file.  hipcc cannot be made to keep 128 accumulators + 64 operand registers in the
accumulator half without shuffling them through v_accvgpr_read/write (round 1, DESIGN.md 4.4 last row: 744 TF), so
the kernel body is written out instruction by instruction here, with a fixed register map, and pasted into the
kernel as one ``asm volatile`` block (``attention_w64_asm.inc``).  The surrounding HIP code computes addresses
and descriptors only.

    python gen_attn_w64.py > attention_w64_asm.inc        (build.py does this when the generator changed)

Math and layouts are those of attention.hip (S^T = K Q^T, O^T = V^T P^T, key bits 2<->3 swapped so P never moves
between lanes; K [64][128] / V^T [128][64] bf16 tiles, 16-byte-slot XOR swizzle, LDS-DMA staged).  What is new:

  * two 32-query blocks per wave share every K / V^T fragment read: 0.5 ds_read_b128 per MFMA instead of 1;
  * O (128 regs) and the pre-scaled Q fragments (64 regs) live in AGPRs, K / V^T fragment rings too — the arch
    VGPRs hold two score sets (128), the packed P (32) and the softmax state;
  * q carries scale*log2(e) (folded into the norm kernel, or applied in the prologue here), and the running max
    enters the scores through the MFMA's C operand (16 registers per query block holding -m): p = exp2(S) needs NO
    per-element subtract / fma;
  * the running max is only moved when a row's new maximum exceeds it by more than THR = 4 (factor 16 in P):
    the rescale of O (AGPR round trip) is a rare slow path, never on the hot path;
  * per tile: phase 1 = K(t+1).Q^T (32 MFMA) || exp2 + bf16 packing of tile t (96 VALU) || K fragment reads,
    phase 2 = V^T(t).P^T(t) (32 MFMA) || row sums of tile t + row max of tile t+1 (~100 VALU) || V^T fragment reads;
    <= 4.2 non-MFMA issues per MFMA (the budget is 5: MI355X_MICROARCH.md, one wave per SIMD).

Variants (the numbers are history: V0 / V1, the steps that led to V2, are no longer generated):
  V2  a V^T ring of two 16 KiB slots and a K ring of THREE, filled three tiles ahead; the eight DMA pieces of a tile are
      spread over phase 1, the first three V^T fragments of phase 2 are read under the last MFMAs of phase 1 and the
      first K fragments of the next tile under the last MFMAs of phase 2 (no phase starts by waiting for the LDS);
  V3  = V2 storing its normalised result in fp32: the split-KV workers of the tail (attention_w64.hip).
  V4  = V2 WITHOUT a running max: the caller supplies m >= every score of the workgroup's (sample, head) as an SGPR operand
      (%[sm], from the norms of q and k: attention_w64.hip); MI holds -m from the prologue on and is never touched, so
      p = exp2(s - m) <= 1 with no row maxima, no rescale check, no slow path and no first-tile special case; the log-sum-exp
      is (m + log2 l) ln 2.  Row sums, exp2 + packing, masks, DMA schedule, K ring and barriers are V2's.  Not a launch
      variant: the kernel of V2 picks it per workgroup.

Schedules of the loop body (V2 / V3 / V4; option W64_SCHED, chosen per launch — the kernels hold both text blocks):
  0  the order described above: all 64 exponentials and 32 packs of tile t under the K(t+1).Q^T MFMAs of phase 1 — next to the
     eight LDS-DMA pieces, their SALU and 15 fragment reads, two exponentials (8 issue cycles each) per MFMA gap — and only the
     row sums (V2 / V3: and the row maxima) under the V^T.P^T MFMAs of phase 2;
  1  the balanced order, the default: pv_mfmas() issues key block 0 before key block 1, so P(qb, kb = 1, a) is first read by MFMA
     16 + 8 a + qb of phase 2, and the exponentials and packs of key block 1 may run under MFMAs [0, 16) of phase 2.  DEFER[variant] of
     them do (V4, whose phase 2 carries nothing but the row sums: all 32; V2 / V3, whose phase 2 also finds the row maxima of
     tile t+1: 8), and the VALU work of both phases is spread by issue cost (spread_cost) instead of by count.  Order only: every
     pack keeps two MFMAs between itself and the first MFMA that reads its P register, every row-sum add of a deferred score
     register follows the group's exponentials and packs by at least one MFMA, the adds of each accumulator chain keep their
     order, the DMA pieces, fragment reads, waits and barriers stay where they are, and nothing is added behind the last MFMA
     of phase 2.  Same bits as schedule 0 (tests/test_attn_w64_sched_host.py, tests/test_gpu_attn_w64_sched.py).
  The two schedules differ in the four phases of the loop (two per body) and in one .p2align: the .inc holds each stream as
  ten pieces (PIECES below), schedule 1 adds its four phases and shares the other six.
  The V^T(t+1) DMA pieces stay in phase 1 (moving them into the second half of phase 2 was not tried).

Register map (asm-owned; the thirteen per-lane inputs stay in the compiler's operand registers v0..v11):
  a[0:127]    O^T accumulators   [qb][db] 16 each
  a[128:191]  Q fragments        [qb][kk] 4 each (bf16x8)
  a[192:215]  K fragment ring    3 stages x [kb] x 4
  a[216:231]  V^T fragment ring  4 stages x 4
  v[12:19]    K fragment LDS addresses (per kk)      v[20:23]  V^T fragment LDS addresses (per kb, a)
  v[32:95]    score set 0        [qb][kb] 16 each    v[96:159] score set 1
  v[160:191]  MI = -m_run        [qb] 16 copies (MFMA C operand)
  v[192:223]  P packed bf16      [qb][kb][a] 4 each
  v[224:255]  state / temporaries
  s92 s93 DMA source offsets, s94 tile counter, s95 K tile stride, s[96:97] exec save, s98 K read-slot offset,
  s99 K DMA-slot offset, s91 address step of the K ring
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_w64_common import Emit, ar, linearize, spread, vr        # noqa: E402

THR = "4.0"                      # inline constant: rescale when a row max exceeds the running max by > 4 (log2 units)
KSLOT = 16384


# ---------------------------------------------------------------- register map
def O(qb, db):      return (qb * 4 + db) * 16
def Q(qb, kk):      return 128 + (qb * 8 + kk) * 4
def KR(stage, kb):  return 192 + stage * 8 + kb * 4
def VR(stage):      return 216 + stage * 4
def S(st, qb, kb):  return 32 + st * 64 + (qb * 2 + kb) * 16
def MI(qb):         return 160 + qb * 16
def P(qb, kb, a):   return 192 + ((qb * 2 + kb) * 2 + a) * 4


KA = list(range(12, 20))
VA = list(range(20, 24))
M_RUN = [224, 225]
L_A = [226, 227]
L_B = [228, 229]
MXA = [230, 231]
MXB = [232, 233]
T0, T1, T2, T3 = 234, 235, 236, 237
NEGINF = 238
VLIM = 239
INV = [240, 241]
E0 = 242                          # 242..249 scratch (8)


# ---------------------------------------------------------------- op lists (gen_w64_common.py: their three kinds, linearize)
def weave(mfmas, plans, pre=()):
    """mfmas: list of ("m", ...) ops; plans: lists (one entry per gap) of lists of ops issued after that MFMA."""
    ops = list(pre)
    for g, m in enumerate(mfmas):
        ops.append(m)
        for pl in plans:
            ops.extend(pl[g])
    return ops


def X(lines):
    return [("x", ln) for ln in lines]


def issue_cost(op):
    """Issue cycles of one filler beside the MFMAs of a one-wave-per-SIMD stream (MI355X_MICROARCH.md, 'vector-instruction
    ISSUE cost'): transcendentals 8, the bf16 pack 5, any other VALU instruction 4.  What does not go through the vector
    issue port is priced by assumption, in the same units (not measured one by one; the sweep judged the resulting
    orders as wholes): an LDS read 4, an LDS-DMA piece 8, a scalar instruction 2."""
    txt = op[2] if op[0] == "r" else op[1]
    if txt.startswith("v_exp_f32"):
        return 8
    if txt.startswith("v_cvt_pk"):
        return 5
    if txt.startswith("buffer_load"):
        return 8
    if txt.startswith("s_"):
        return 2
    return 4


def spread_cost(items, gaps, start, end, base=(), floor=None):
    """spread() by issue cost instead of by count: `items` (ordered) go into gaps[start:end] in order, each gap filled up
    to one common level of issue cost ON TOP of what the plans in `base` already put there, so that a gap that carries a
    DMA piece or fragment reads gets fewer of the items.  floor[i]: the first gap item i may go to (it reads what another
    plan writes there).  With 8-cycle items no more numerous than the gaps the level keeps them one to a gap."""
    load = [float(sum(issue_cost(op) for pl in base for op in pl[g])) for g in range(gaps)]
    cost = [issue_cost(it) for it in items]
    lo, hi = min(load[start:end]), max(load[start:end]) + sum(cost)
    for _ in range(60):                                          # the level L: sum over the gaps of max(0, L - load) = total
        mid = 0.5 * (lo + hi)
        if sum(max(0.0, mid - load[g]) for g in range(start, end)) < sum(cost):
            lo = mid
        else:
            hi = mid
    out = [[] for _ in range(gaps)]
    g = start
    for i, it in enumerate(items):
        if floor is not None:
            g = max(g, floor[i])
        while g < end - 1 and load[g] + 0.5 * cost[i] > hi:
            g += 1
        out[g].append(it)
        load[g] += cost[i]
    return out


# Schedules of the loop body body(p) of V2 / V3 / V4 (option W64_SCHED, attention_w64.hip): ORDER ONLY, the instructions and
# their operands are those of schedule 0, and so is every bit of the result (tests/test_attn_w64_sched_host.py).
#   0      the order the streams always had, text included: exp2 + packing of the whole tile spread by COUNT over phase 1,
#          row sums (and V2's row maxima) by count over phase 2;
#   1      DEFER[variant] exponentials of key block 1 (whole (qb, kb = 1, a) groups of 8, with the 4 packs that trail
#          them) are issued under MFMAs [0, 16) of phase 2 instead of in phase 1, and the VALU work of both phases is
#          spread by issue cost (spread_cost) on top of the DMA pieces and fragment reads.  The loop head is aligned to
#          64 bytes.  What a launch runs with the option unset.
# The sweep that chose them (defer 0 / 8 / 16 / 24 / 32, by count and by cost, both 4-byte alignment phases:
# profiles/attn_phase_balance_ab.txt): spreading by count lost to spreading by cost at every defer; V4, whose
# phase 2 carries the row sums only, is fastest with all of key block 1 deferred (-4.0 % per launch), V2 / V3, whose phase 2
# also carries the row maxima of the next tile, with one group (-2.3 %).
DEFER = {2: 8, 3: 8, 4: 32}
# groups of key block 1 in the order they are deferred: the one whose P registers are read last goes first
DEFER_ORDER = [(1, 1, 1), (0, 1, 1), (1, 1, 0), (0, 1, 0)]


def first_reader(qb, kb, a):
    """Index of the first MFMA of pv_mfmas() that reads P(qb, kb, a)."""
    return 2 * (8 * kb + 4 * a) + qb


# ---------------------------------------------------------------- pieces
def kread_ops(kk, kbase):
    st = kk % 3
    return [("r", f"K{kk}.0", f"ds_read_b128 {ar(KR(st, 0), 4)}, {vr(KA[kk])} offset:{kbase}"),
            ("r", f"K{kk}.1", f"ds_read_b128 {ar(KR(st, 1), 4)}, {vr(KA[kk])} offset:{kbase + 8192}")]


def vread_op(i, vbase):
    kb, a, db = i >> 3, (i >> 2) & 1, i & 3
    return ("r", f"V{i}", f"ds_read_b128 {ar(VR(i % 4), 4)}, {vr(VA[2 * kb + a])} offset:{vbase + db * 4096}")


def qk_mfmas(nxt, c_zero=False):
    """32 MFMAs of K.Q^T into score set nxt (C = MI = -m_run on the first k step), + the fragment reads that ride
    behind them (steps kk+2, after the 2nd MFMA of step kk)."""
    mf = []
    for kk in range(8):
        for kb, qb in ((0, 0), (0, 1), (1, 0), (1, 1)):
            c = ("0" if c_zero else vr(MI(qb), 16)) if kk == 0 else vr(S(nxt, qb, kb), 16)
            mf.append(("m", f"v_mfma_f32_32x32x16_bf16 {vr(S(nxt, qb, kb), 16)}, {ar(KR(kk % 3, kb), 4)}, "
                            f"{ar(Q(qb, kk), 4)}, {c}", [f"K{kk}.{kb}"]))
    return mf


def qk_read_plan(kbase, first=2):
    plan = [[] for _ in range(32)]
    for kk in range(8):
        if first <= kk + 2 < 8:
            plan[kk * 4 + 1] = kread_ops(kk + 2, kbase)
    return plan


def softmax_lines(cur):
    """exp2 in place + bf16 packing of score set cur: 64 + 32 VALU; a block's packing trails its exponentials."""
    out = []
    for qb in range(2):
        for kb in range(2):
            base = S(cur, qb, kb)
            for r in range(16):
                out.append(f"v_exp_f32 {vr(base + r)}, {vr(base + r)}")
            for a in range(2):
                for eidx in range(4):
                    r0 = base + 8 * a + 2 * eidx
                    out.append(f"v_cvt_pk_bf16_f32 {vr(P(qb, kb, a) + eidx)}, {vr(r0)}, {vr(r0 + 1)}")
    return out


def softmax_split(cur, deferred):
    """softmax_lines(cur) as (lines of phase 1, {group: lines} of the deferred (qb, kb, a) groups): a group's eight
    exponentials, then its four packs.  Both keep the order softmax_lines() has."""
    now, later = [], {g: [] for g in deferred}
    for ln in softmax_lines(cur):
        m = re.findall(r"v(\d+)", ln)
        reg = int(m[1])                                          # first source: a score register of set cur
        i = reg - S(cur, 0, 0)
        key = (i // 32, (i // 16) % 2, (i % 16) // 8)
        (later[key] if key in later else now).append(ln)
    return now, later


def rowsum_lines(cur):
    # (round 5: the same sums as 32 v_pk_add_f32 on (L_A, L_B) register pairs — bit-identical, 32 VALU instructions fewer per
    #  tile — measured SLOWER, 4.88 -> 5.07 ms per launch on one box: packed fp32 adds do not issue faster here and the two
    #  accumulator chains end up two instructions apart instead of four).  Likewise 32 v_dot2_f32_bf16 on the PACKED bf16 pairs
    #  (P.lo * 1 + P.hi * 1 + acc): 4.82 -> 4.99 ms.  VOP3P instructions cost ~3x a plain VALU instruction in this stream.)
    a, b = [], []
    for qb, dst in ((0, a), (1, b)):
        regs = [S(cur, qb, kb) + r for kb in range(2) for r in range(16)]
        for i, r in enumerate(regs):
            acc = L_A[qb] if i % 2 == 0 else L_B[qb]
            dst.append(f"v_add_f32 {vr(acc)}, {vr(acc)}, {vr(r)}")
    mixed = []
    for i in range(0, 32, 2):                                   # dependent adds end up 4 apart
        mixed += [a[i], a[i + 1], b[i], b[i + 1]]
    return mixed


def rowmax_lines(nxt):
    """Row max of score set nxt per query block -> MXA[qb] (both half-waves hold the row's max)."""
    out = []
    for qb in range(2):
        s0, s1 = S(nxt, qb, 0), S(nxt, qb, 1)
        out.append(f"v_max_f32 {vr(MXA[qb])}, {vr(s0)}, {vr(s1)}")
        out.append(f"v_max_f32 {vr(MXB[qb])}, {vr(s0 + 1)}, {vr(s1 + 1)}")
    for r in range(2, 16, 2):
        for qb in range(2):
            s0, s1 = S(nxt, qb, 0), S(nxt, qb, 1)
            out.append(f"v_max3_f32 {vr(MXA[qb])}, {vr(MXA[qb])}, {vr(s0 + r)}, {vr(s1 + r)}")
            out.append(f"v_max3_f32 {vr(MXB[qb])}, {vr(MXB[qb])}, {vr(s0 + r + 1)}, {vr(s1 + r + 1)}")
    for qb in range(2):
        out.append(f"v_max_f32 {vr(MXA[qb])}, {vr(MXA[qb])}, {vr(MXB[qb])}")
    for qb in range(2):
        out.append(f"v_mov_b32 {vr(MXB[qb])}, {vr(MXA[qb])}")
    out.append("s_nop 1")
    for qb in range(2):
        out.append(f"v_permlane32_swap_b32 {vr(MXA[qb])}, {vr(MXB[qb])}")
    for qb in range(2):
        out.append(f"v_max_f32 {vr(MXA[qb])}, {vr(MXA[qb])}, {vr(MXB[qb])}")
    return out


def pv_mfmas(cur):
    mf = []
    for i in range(16):
        kb, a, db = i >> 3, (i >> 2) & 1, i & 3
        for qb in range(2):
            mf.append(("m", f"v_mfma_f32_32x32x16_bf16 {ar(O(qb, db), 16)}, {ar(VR(i % 4), 4)}, "
                            f"{vr(P(qb, kb, a), 4)}, {ar(O(qb, db), 16)}", [f"V{i}"]))
    return mf


def pv_read_plan(vbase, first=3):
    plan = [[] for _ in range(32)]
    for i in range(16):
        if first <= i + 3 < 16:
            plan[2 * i] = [vread_op(i + 3, vbase)]
    return plan


def mask_block(e, st):
    """Scores of set `st` whose key index >= klen -> -inf.  %[srem] = klen - 64 * tile (1..63 when the block runs)."""
    e(f"v_lshlrev_b32 {vr(VLIM)}, 3, %[lh]")
    e(f"v_sub_u32 {vr(VLIM)}, %[srem], {vr(VLIM)}")           # rem - 8 h : mask register r when c(r) >= vlim
    for kb in range(2):
        for r in range(16):
            c = 32 * kb + 16 * (r >> 3) + (r & 7)
            e(f"v_cmp_ge_i32 vcc, {c}, {vr(VLIM)}")
            for qb in range(2):
                reg = S(st, qb, kb) + r
                e(f"v_cndmask_b32 {vr(reg)}, {vr(reg)}, {vr(NEGINF)}, vcc")


def slow_path(e, st, qb, first):
    """Move the running max of query block qb: delta = first ? rowmax : max(rowmax, 0) (rowmax is relative to the
    running max already), then O, l, the pending scores of set `st` and -m (MI) follow."""
    d, al = T0, T1
    if first:
        e(f"v_mov_b32 {vr(d)}, {vr(MXA[qb])}")
    else:
        e(f"v_max_f32 {vr(d)}, 0, {vr(MXA[qb])}")
    e(f"v_add_f32 {vr(M_RUN[qb])}, {vr(M_RUN[qb])}, {vr(d)}")
    e(f"v_sub_f32 {vr(al)}, 0, {vr(d)}")
    e(f"v_exp_f32 {vr(al)}, {vr(al)}")
    for kb in range(2):
        for r in range(16):
            reg = S(st, qb, kb) + r
            e(f"v_sub_f32 {vr(reg)}, {vr(reg)}, {vr(d)}")
    for r in range(16):
        e(f"v_sub_f32 {vr(MI(qb) + r)}, {vr(MI(qb) + r)}, {vr(d)}")
    if not first:
        e(f"v_mul_f32 {vr(L_A[qb])}, {vr(L_A[qb])}, {vr(al)}")
        e(f"v_mul_f32 {vr(L_B[qb])}, {vr(L_B[qb])}, {vr(al)}")
        e("s_nop 7")
        e("s_nop 7")
        e("s_nop 7")                                           # MFMA write of O -> v_accvgpr_read
        for db in range(4):
            for r in range(0, 16, 4):
                regs = [O(qb, db) + r + i for i in range(4)]
                tmp = [E0 + i for i in range(4)]
                for a_, t_ in zip(regs, tmp):
                    e(f"v_accvgpr_read_b32 {vr(t_)}, {ar(a_)}")
                for t_ in tmp:
                    e(f"v_mul_f32 {vr(t_)}, {vr(t_)}, {vr(al)}")
                for a_, t_ in zip(regs, tmp):
                    e(f"v_accvgpr_write_b32 {ar(a_)}, {vr(t_)}")
    e("s_nop 7")                                               # VALU write -> MFMA read (MI as C, O as C)


def check_and_rescale(e, st, tag, first=False):
    """Per query block: move the running max when the new row max exceeds it by more than THR.  ONE branch skips both
    blocks' checks in the common case (round 5: a taken branch costs a one-wave-per-SIMD stream ~40 cycles of instruction
    fetch, and there were two per tile); vccz is stale after a scalar write of vcc, so the merged test goes through scc."""
    if first:
        for qb in range(2):
            slow_path(e, st, qb, True)
        return
    both = e.lab(f"nores_{tag}")
    e(f"v_cmp_lt_f32 vcc, {THR}, {vr(MXA[0])}")
    e("s_mov_b64 s[96:97], vcc")
    e(f"v_cmp_lt_f32 vcc, {THR}, {vr(MXA[1])}")
    e("s_or_b64 s[96:97], s[96:97], vcc")
    e("s_cmp_eq_u64 s[96:97], 0")
    e(f"s_cbranch_scc1 {both}")
    for qb in range(2):
        skip = e.lab(f"nores_{tag}_{qb}")
        e(f"v_cmp_lt_f32 vcc, {THR}, {vr(MXA[qb])}")
        e(f"s_cbranch_vccz {skip}")
        slow_path(e, st, qb, False)
        e.label(skip)
    e.label(both)


def rotate(sreg, nslots):
    return [f"s_add_u32 {sreg}, {sreg}, {KSLOT}", f"s_cmp_eq_u32 {sreg}, {nslots * KSLOT}", f"s_cselect_b32 {sreg}, 0, {sreg}"]


# ---------------------------------------------------------------- whole stream
def generate(variant, sched=0):
    defer = DEFER[variant] if sched else 0
    # V4 (round 5: V2 without the row maxima and the rescale check measured 4.707 -> 4.555 ms per launch).  A stream without
    # the running max needs a bound on the scores; the a-priori one is useless (the model's RMS norm runs over all 1 536
    # channels, not per head: 196 log2 units, p would underflow), but the stream does not need the worst case, it needs a
    # bound for THIS launch's q and k: s_ij <= |q_i| |k_j| per head (Cauchy-Schwarz), and the norm kernel that writes q and k
    # emits max |q|^2 and max |k|^2 per (sample, head) on the way (dit_elementwise.hip).  The kernel takes V4 only where
    # that bound is <= 48, so that p >= 2^-96 stays a normal number; above it the workgroup runs V2.
    bounded = variant == 4
    # (timing-only ablations of V2 measured in round 2, profiles/r02_attention_w64_ablations.json: no LDS-DMA in the
    # loop -5.9 %, v_exp -> v_mov -3.4 %, no barrier -0.2 %, no ds_reads -8.1 %: nothing dominates)
    # variant 3 = variant 2 with the "partial" epilogue of the split-KV tail workers: the normalised output is stored
    # in fp32 (one [256, 128] slab per worker) instead of bf16; with the log-sum-exp stored next to it a combine
    # pass weights the workers' results (attention_w64.hip)
    partial = variant == 3
    # LDS map: V^T ring of two slots [0, 32K) | K ring of three slots [32K, 80K) — the K addresses carry the ring base
    # and slot in the address registers, so every ds_read offset stays below 64 KiB
    VBASE = 0
    KBASE = 2 * KSLOT
    e = Emit("w64v", variant)                 # (both schedules: the labels end in %=, unique per asm statement)

    def k_dma(slot_expr, advance=True):
        """4 pieces of K(next) -> K ring slot; slot_expr: literal byte offset or an SGPR name."""
        out = [f"s_add_u32 m0, %[ldsw], {slot_expr}", f"s_add_u32 m0, m0, {KBASE}"]
        for j in range(4):
            if j:
                out.append("s_add_u32 m0, m0, 4096")
            out.append("s_mov_b32 s92, %[skn]" if j == 0 else "s_add_u32 s92, s92, %[skp]")
            out.append("buffer_load_dwordx4 %[vok], %[rk], s92 offen lds")
        if advance:
            out.append("s_add_u32 %[skn], %[skn], s95")
        return out

    def v_dma(slot):
        out = [f"s_add_u32 m0, %[ldsw], {VBASE + slot * KSLOT}"]
        for j in range(4):
            if j:
                out.append("s_add_u32 m0, m0, 4096")
            out.append("s_mov_b32 s93, %[svn]" if j == 0 else "s_add_u32 s93, s93, %[svp]")
            out.append("buffer_load_dwordx4 %[vov], %[rv], s93 offen lds")
        out.append("s_add_u32 %[svn], %[svn], 128")
        return out

    # ---------------- prologue: Q fragments -> (pre-scaled) bf16 -> AGPRs
    for qb in range(2):
        for kk in range(8):
            so = "0" if qb == 0 else "%[sq1]"
            e(f"buffer_load_dwordx4 {vr(32 + (qb * 8 + kk) * 4, 4)}, %[voq], %[rq], {so} offen offset:{kk * 32}")
    e("s_lshl_b32 s95, %[skp], 2")
    for kk in range(8):
        e(f"v_xor_b32 {vr(T0)}, {kk}, %[xh]")
        e(f"v_lshl_add_u32 {vr(KA[kk])}, {vr(T0)}, 5, %[kab]")
        e(f"v_add_u32 {vr(KA[kk])}, {KBASE}, {vr(KA[kk])}")
    for j in range(4):
        e(f"v_xor_b32 {vr(T0)}, {j}, %[yh]")
        e(f"v_lshl_add_u32 {vr(VA[j])}, {vr(T0)}, 5, %[vab]")
    e(f"v_mov_b32 {vr(NEGINF)}, 0xff800000")
    for qb in range(2):
        e(f"v_mov_b32 {vr(M_RUN[qb])}, " + ("%[sm]" if bounded else "0"))      # V4: the fixed bound m, for the log-sum-exp
        e(f"v_mov_b32 {vr(L_A[qb])}, 0")
        e(f"v_mov_b32 {vr(L_B[qb])}, 0")
        for r in range(16):
            if bounded:
                e(f"v_xor_b32 {vr(MI(qb) + r)}, 0x80000000, {vr(M_RUN[qb])}")  # -m: the C operand of every tile's first MFMAs
            else:
                e(f"v_mov_b32 {vr(MI(qb) + r)}, 0")
    for i in range(128):
        e(f"v_accvgpr_write_b32 {ar(i)}, 0")
    # first tiles: K(0), V(0), K(1), K(2)
    n_dma = 0
    for ln in k_dma(0) + v_dma(0) + k_dma(KSLOT) + k_dma(2 * KSLOT):
        e(ln)
        n_dma += ln.startswith("buffer_load")
    e(f"s_waitcnt vmcnt({n_dma})")                              # the 16 Q loads (issued first) have landed
    for i in range(64):
        src = 32 + i
        e(f"v_lshlrev_b32 {vr(T0)}, 16, {vr(src)}")
        e(f"v_and_b32 {vr(T1)}, 0xffff0000, {vr(src)}")
        e(f"v_mul_f32 {vr(T0)}, %[sc], {vr(T0)}")
        e(f"v_mul_f32 {vr(T1)}, %[sc], {vr(T1)}")
        e(f"v_cvt_pk_bf16_f32 {vr(T2)}, {vr(T0)}, {vr(T1)}")
        e(f"v_accvgpr_write_b32 {ar(128 + i)}, {vr(T2)}")
    e("s_waitcnt vmcnt(0)")
    e("s_barrier")
    e("s_nop 7")
    # ---------------- scores of tile 0 -> set 0 (C = 0; V4: C = -m like every other tile)
    ops = weave(qk_mfmas(0, c_zero=not bounded), [qk_read_plan(0)], pre=kread_ops(0, 0) + kread_ops(1, 0))
    pending = linearize(e, ops, [])
    assert not pending
    # K ring bookkeeping: tile t reads slot (t+1) % 3 and refills slot t % 3; the address registers now move to slot 1
    e(f"s_mov_b32 s98, {KSLOT}")                                # slot offset the K addresses point at
    e("s_mov_b32 s99, 0")                                       # slot offset the next K DMA fills
    for kk in range(8):
        e(f"v_add_u32 {vr(KA[kk])}, {KSLOT}, {vr(KA[kk])}")
    for op in kread_ops(0, 0) + kread_ops(1, 0):
        e(op[2])
    pending = ["K0.0", "K0.1", "K1.0", "K1.1"]
    e("s_nop 7")
    e("s_nop 7")                                               # MFMA write of the scores -> VALU
    nomask0 = e.lab("nomask_first")
    e("s_cmp_ge_i32 %[srem], 64")
    e(f"s_cbranch_scc1 {nomask0}")
    mask_block(e, 0)
    e.label(nomask0)
    if not bounded:
        for ln in rowmax_lines(0):
            e(ln)
        check_and_rescale(e, 0, "first", first=True)
    e("s_mov_b32 s94, 0")                                      # t
    LOOP_PENDING = list(pending)

    LOOP, LAST, EPI = e.lab("loop"), [e.lab("last0"), e.lab("last1")], e.lab("epi")

    def body(p):
        cur, nxt = p, p ^ 1
        e("s_waitcnt vmcnt(0)")
        e("s_barrier")
        dma = k_dma("s99") + v_dma(nxt)
        vbase = VBASE + p * KSLOT
        # ---- phase 1: the eight DMA pieces spread over it, the first three V^T fragments of phase 2 read under its last MFMAs
        mf1 = qk_mfmas(nxt)
        plans = [qk_read_plan(0)]                              # (offset 0: the address registers carry the K slot)
        plans.append(spread(X(dma), 32, 0, 30))
        vp = [[] for _ in range(32)]
        vp[29], vp[30], vp[31] = [vread_op(0, vbase)], [vread_op(1, vbase)], [vread_op(2, vbase)]
        groups = DEFER_ORDER[:defer // 8]
        sm_now, sm_later = softmax_split(cur, groups) if sched else (softmax_lines(cur), {})
        plans.append(spread_cost(X(sm_now), 32, 2, 32, base=plans + [vp]) if sched else spread(X(sm_now), 32, 2, 32))
        plans.append(vp)
        ops1 = weave(mf1, plans)
        e.cut()
        pend = linearize(e, ops1, LOOP_PENDING)
        e.cut()
        # ---- between the phases: mask the new scores if tile t+1 is the last one and partial
        e("s_sub_u32 %[srem], %[srem], 64")                    # keys left from tile t+1 on
        nomask = e.lab(f"nomask_{p}")
        e("s_cmp_ge_i32 %[srem], 64")
        e(f"s_cbranch_scc1 {nomask}")
        e("s_nop 7")
        e("s_nop 7")
        mask_block(e, nxt)
        e.label(nomask)
        # ---- phase 2
        mf2 = pv_mfmas(cur)
        plans = [pv_read_plan(vbase)]
        tail = rowsum_lines(cur) + ([] if bounded else rowmax_lines(nxt))
        # the K addresses step to the next slot once the reads of phase 1 are all issued; the first fragments of
        # the next tile's K are read under the last MFMAs
        step = ["s_mov_b32 s91, s98"] + rotate("s98", 3) + ["s_sub_u32 s91, s98, s91"] + rotate("s99", 3)
        step += [f"v_add_u32 {vr(KA[kk])}, s91, {vr(KA[kk])}" for kk in range(8)]
        plans.append(spread(X(step), 32, 0, 12))
        kp = [[] for _ in range(32)]
        kp[27], kp[29] = kread_ops(0, 0), kread_ops(1, 0)
        plans.append(kp)
        floor = None
        if groups:
            # the deferred groups, first reader first, under MFMAs [0, 16); every pack at least two MFMAs before the first
            # MFMA that reads its P register (VALU write -> MFMA operand read), every row-sum add of a deferred score
            # register at least one MFMA behind its group's last line (a transcendental's result is not forwarded to the next
            # VALU instruction, and the register keeps schedule 0's order of readers: pack, then add)
            late = [ln for g in sorted(groups, key=lambda g: first_reader(*g)) for ln in sm_later[g]]
            dp = spread_cost(X(late), 32, 0, 16, base=plans)
            plans.append(dp)
            where = {op[1]: g for g in range(32) for op in dp[g]}
            for g in groups:
                assert all(where[ln] <= first_reader(*g) - 2 for ln in sm_later[g]), (g, sched)
            done = {ln.split()[1].rstrip(","): max(where[x] for x in sm_later[g])
                    for g in groups for ln in sm_later[g] if ln.startswith("v_exp_f32")}
            floor = [done.get(ln.split()[-1], -1) + 1 if ln.startswith("v_add_f32") else 0 for ln in tail]
        by_count = spread(X(tail), 32, 1, 32)
        if sched:
            # behind the last MFMA (in front of the rescale check) exactly what schedule 0 has there, the rest by cost
            n = len(tail) - len(by_count[31])
            by_cost = spread_cost(X(tail[:n]), 32, 1, 31, base=plans, floor=floor)
            by_cost[31] = by_count[31]
            plans.append(by_cost)
        else:
            plans.append(by_count)
        e.cut()
        pend = linearize(e, weave(mf2, plans), pend)
        e.cut()
        assert pend == LOOP_PENDING, (pend, LOOP_PENDING)
        if not bounded:
            check_and_rescale(e, nxt, f"b{p}")
        e("s_add_u32 s94, s94, 1")

    def last(p):
        e("s_waitcnt vmcnt(0)")
        e("s_barrier")
        vbase = VBASE + p * KSLOT
        for ln in softmax_lines(p):
            e(ln)
        ops2 = weave(pv_mfmas(p), [pv_read_plan(vbase), spread(X(rowsum_lines(p)), 32, 1, 32)],
                     pre=[vread_op(0, vbase), vread_op(1, vbase), vread_op(2, vbase)])
        linearize(e, ops2, LOOP_PENDING)

    e.cut()
    if sched:
        # hand-written streams lose up to 13 % under a uniform shift of 4 mod 8 bytes (cdna_hip_programming.md): the loop head
        # does not move with what the compiler puts in front of the block
        e(".p2align 6")
    e.label(LOOP)
    for p in range(2):
        e("s_cmp_eq_u32 s94, %[slast]")
        e(f"s_cbranch_scc1 {LAST[p]}")
        body(p)
    e(f"s_branch {LOOP}")
    for p in range(2):
        e.label(LAST[p])
        last(p)
        if p == 0:
            e(f"s_branch {EPI}")
    e.label(EPI)

    # ---------------- epilogue: l = sum over both half-waves, O / l -> bf16 -> global
    e("s_waitcnt lgkmcnt(0)")
    e("s_nop 7")
    e("s_nop 7")
    e("s_nop 7")
    for qb in range(2):
        e(f"v_add_f32 {vr(L_A[qb])}, {vr(L_A[qb])}, {vr(L_B[qb])}")
    for qb in range(2):
        e(f"v_mov_b32 {vr(L_B[qb])}, {vr(L_A[qb])}")
    e("s_nop 1")
    for qb in range(2):
        e(f"v_permlane32_swap_b32 {vr(L_A[qb])}, {vr(L_B[qb])}")
    for qb in range(2):
        e(f"v_add_f32 {vr(L_A[qb])}, {vr(L_A[qb])}, {vr(L_B[qb])}")
        e(f"v_rcp_f32 {vr(INV[qb])}, {vr(L_A[qb])}")
    for qb in range(2):
        so = "0" if qb == 0 else "%[so1]"
        for db in range(4):
            for g in range(4):
                regs = [O(qb, db) + 4 * g + i for i in range(4)]
                tmp = [E0 + 4 * (g & 1) + i for i in range(4)]
                for a_, t_ in zip(regs, tmp):
                    e(f"v_accvgpr_read_b32 {vr(t_)}, {ar(a_)}")
                for t_ in tmp:
                    e(f"v_mul_f32 {vr(t_)}, {vr(t_)}, {vr(INV[qb])}")
                if partial:
                    e(f"buffer_store_dwordx4 {vr(tmp[0], 4)}, %[voo], %[ro], {so} offen offset:{db * 128 + g * 32}")
                    e("s_nop 1")
                    continue
                e(f"v_cvt_pk_bf16_f32 {vr(tmp[0])}, {vr(tmp[0])}, {vr(tmp[1])}")
                e(f"v_cvt_pk_bf16_f32 {vr(tmp[1])}, {vr(tmp[2])}, {vr(tmp[3])}")
                e(f"buffer_store_dwordx2 {vr(tmp[0], 2)}, %[voo], %[ro], {so} offen offset:{db * 64 + g * 16}")
    # log-sum-exp (natural log) for the backward, lower half-wave.  No lse requested: the descriptor %[rl] has zero
    # records and the two stores are dropped by the hardware
    for qb in range(2):
        e(f"v_log_f32 {vr(T0 + qb)}, {vr(L_A[qb])}")
    e("s_nop 0")
    for qb in range(2):
        e(f"v_add_f32 {vr(T0 + qb)}, {vr(T0 + qb)}, {vr(M_RUN[qb])}")
        e(f"v_mul_f32 {vr(T0 + qb)}, 0x3f317218, {vr(T0 + qb)}")
    e("s_mov_b64 s[96:97], exec")
    e("s_mov_b64 exec, 0xffffffff")
    e(f"buffer_store_dword {vr(T0)}, %[vol], %[rl], 0 offen")
    e(f"buffer_store_dword {vr(T1)}, %[vol], %[rl], 0 offen offset:128")
    e("s_mov_b64 exec, s[96:97]")
    e("s_waitcnt vmcnt(0)")
    return e


N_VARIANTS = 4
LDS_BYTES = 5 * KSLOT                                            # V^T ring of two slots, K ring of three
CLOBBER_V = range(12, 256)
CLOBBER_A = range(0, 256)
CLOBBER_S = range(91, 100)


# The text of a stream in the .inc: ten pieces (Emit.cut), so that the two schedules, which differ in the four phases of the
# loop only, share the other six: the prologue, the head of each loop body (loop label, end test, wait, barrier), what
# stands between the phases (mask of a partial last tile), and the end (rescale check of the second body, `last` blocks,
# epilogue, with the rescale check of the first body in HEAD1).
PIECES = ("PRO", "HEAD0", "P1_0", "MID0", "P2_0", "HEAD1", "P1_1", "MID1", "P2_1", "END")
PHASES = ("P1_0", "P2_0", "P1_1", "P2_1")


def put(name, lines):
    print(f"#define {name} \\")
    print(" \\\n".join('    "%s\\n\\t"' % ln for ln in lines))
    print("")


def put_whole(name, parts):
    print(f"#define {name} \\")
    print(" \\\n".join("    " + " ".join(parts[i:i + 4]) for i in range(0, len(parts), 4)))


def main():
    print("// GENERATED by gen_attn_w64.py — do not edit; edit the generator.")
    # V2 (the default stream), V3 (the split-KV workers') and V4 (the bounded stream: not a launch variant, V2's kernel
    # holds it).  The numbering is history: V0 / V1 were the steps that led to V2.
    for v in (2, 3, 4):
        e = generate(v)
        p0 = e.pieces()
        assert len(p0) == len(PIECES)
        for name, lines in zip(PIECES, p0):
            put(f"OMH_ATTN_W64_V{v}_{name}", lines)
        put_whole(f"OMH_ATTN_W64_ASM_V{v}", [f"OMH_ATTN_W64_V{v}_{name}" for name in PIECES])
        print(f"#define OMH_ATTN_W64_LDS_V{v} {LDS_BYTES}")
        n_mfma = sum("v_mfma" in ln for ln in e.lines)
        print(f"// variant {v}: {len(e.lines)} lines, {n_mfma} MFMA")
        # schedule 1 (option W64_SCHED picks per launch): its four phases, everything else is schedule 0's text
        parts, p1 = [], generate(v, 1).pieces()
        for i in (2, 6):                                         # a loop body: the same lines in both schedules
            assert sorted(p0[i] + p0[i + 2]) == sorted(p1[i] + p1[i + 2]), (v, i)
        for name, a, b in zip(PIECES, p0, p1):
            if name in PHASES:
                assert a != b, (v, name)
                put(f"OMH_ATTN_W64_V{v}_{name}_S1", b)
                parts.append(f"OMH_ATTN_W64_V{v}_{name}_S1")
            else:
                align = [ln for ln in b if ln.startswith(".p2align")]
                assert b == align + a and len(align) == (name == "HEAD0"), (v, name)
                parts += ['"%s\\n\\t"' % ln for ln in align] + [f"OMH_ATTN_W64_V{v}_{name}"]
        put_whole(f"OMH_ATTN_W64_ASM_V{v}_S1", parts)
    clob = ['"memory"', '"vcc"', '"scc"'] + [f'"s{i}"' for i in CLOBBER_S] + [f'"v{i}"' for i in CLOBBER_V] + \
           [f'"a{i}"' for i in CLOBBER_A]
    print("#define OMH_ATTN_W64_CLOBBERS \\")
    rows = [", ".join(clob[i:i + 12]) for i in range(0, len(clob), 12)]
    print("    " + ", \\\n    ".join(rows))
    print(f"#define OMH_ATTN_W64_VARIANTS {N_VARIANTS}")


if __name__ == "__main__":
    main()
