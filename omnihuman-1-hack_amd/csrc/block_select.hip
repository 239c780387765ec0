// Block masks chosen from q and k on the device (include/omh.h: omh_block_pool_d128, omh_block_select,
// omh_block_mask_tables).  Three small launches turn the bf16 q and k of an attention call into the int32 tables the
// block-list attention kernels walk: pooled block means + coherence, top-p selection over the pooled scores, lists.
// No atomics anywhere: every sum runs in a fixed order, so the mask repeats bit for bit.
#include "omh_common.h"

namespace {

constexpr int BLK = 128;       // rows of a block = head dim

__device__ __forceinline__ int live_rows(const int32_t* lens, int b, int L, int blk) {
    int len = lens ? lens[b] : L;
    len = len < 0 ? 0 : (len > L ? L : len);                 // never past the operand
    const int c = len - blk * BLK;
    return c < 0 ? 0 : (c > BLK ? BLK : c);
}

// ---------------------------------------------------------------------------------------------------------------------
// Pool.  One workgroup per (operand, sample, block, head): 128 rows x 128 columns of bf16 = 32 KiB, read once with
// 16-byte loads.  Thread (rg = tid / 16, cl = tid % 16) owns columns [8 cl, 8 cl + 8) of rows rg, rg + 16, ...: a wave
// load covers four 256-byte row segments.  Head is the fastest-varying part of the block id, so that neighbouring
// workgroups read neighbouring segments of the same rows.  3 072 workgroups at B x H x nb = 1 x 12 x 256.
struct PoolOp {
    const uint16_t* x; int64_t ld; const int32_t* lens; float* mean; float* coh; int L, nb;
};
struct PoolParams { PoolOp op[2]; int first1; int B, H; };

__global__ __launch_bounds__(256, 4) void block_pool_kernel(const PoolParams p) {
    __shared__ float part[16][BLK];                          // column sums of the 16 row groups
    __shared__ float red[8];
    const int which = (int)blockIdx.x >= p.first1;
    const PoolOp o = which ? p.op[1] : p.op[0];
    int id = (int)blockIdx.x - (which ? p.first1 : 0);
    const int h = id % p.H;
    id /= p.H;
    const int I = id % o.nb, b = id / o.nb;
    const int c = live_rows(o.lens, b, o.L, I);
    const int tid = threadIdx.x, cl = tid & 15, rg = tid >> 4, lane = tid & 63, w = tid >> 6;
    const uint16_t* base = o.x + ((int64_t)b * o.L + (int64_t)I * BLK) * o.ld + h * BLK + cl * 8;
    u32x4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {                            // all eight loads in flight before the first use
        const int r = rg + 16 * j;
        v[j] = u32x4{0u, 0u, 0u, 0u};
        if (r < c) v[j] = *reinterpret_cast<const u32x4*>(base + (int64_t)r * o.ld);
    }
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float lo = __uint_as_float(v[j][e] << 16), hi = __uint_as_float(v[j][e] & 0xffff0000u);
            s[2 * e] += lo;
            s[2 * e + 1] += hi;
            ss = fmaf(lo, lo, ss);
            ss = fmaf(hi, hi, ss);
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) part[rg][cl * 8 + e] = s[e];
    ss = wave_sum(ss);
    if (lane == 0) red[w] = ss;
    __syncthreads();
    float m = 0.f;
    if (tid < BLK) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) t += part[g][tid];
        m = c > 0 ? t / (float)c : 0.f;
        o.mean[(((int64_t)b * p.H + h) * o.nb + I) * BLK + tid] = m;
    }
    if (w < 2) {
        const float n2 = wave_sum(m * m);
        if (lane == 0) red[4 + w] = n2;
    }
    __syncthreads();
    if (tid == 0) {
        const float den = c > 0 ? ((red[0] + red[1]) + (red[2] + red[3])) / (float)c : 0.f;
        const float coh = den > 0.f ? fminf((red[4] + red[5]) / den, 1.f) : 1.f;
        o.coh[((int64_t)b * p.H + h) * o.nb + I] = coh;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Select.  One wave per (head, query block), four per workgroup (four neighbouring query blocks of one head); the
// samples are walked in order and their selections OR-ed in registers, so every byte of the mask is written exactly once.
// Lane l holds the scores of key blocks l, l + 64, ... (up to 16: nKb <= 1024).  The pooled keys go through LDS 64 blocks
// at a time, shared by the four waves; lane l reads row l starting at column 4 l (mod 128), which spreads a 16-byte
// read of 16 lanes over all 64 banks without padding; the pooled query row is read with the same rotation.
constexpr int SEL_T = 16;      // score slots per lane

struct SelParams {
    const float* qm; const float* qc; const float* km; const float* kc;
    const int32_t* ql; const int32_t* kl; const uint8_t* always; uint8_t* mask;
    int B, H, Lq, Lk, nqb, nkb, always_heads;
    float scale, mass, min_coh;
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(256) void block_select_kernel(const SelParams p) {
    __shared__ __attribute__((aligned(16))) float kt[64 * BLK];          // 32 KiB: 64 pooled key rows
    __shared__ __attribute__((aligned(16))) float qt[4 * BLK];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int h = blockIdx.y, I0 = blockIdx.x * 4, I = I0 + w;
    const bool row_ok = I < p.nqb;
    uint32_t keep_all = 0;                                               // bit t: key block lane + 64 t is kept
    for (int b = 0; b < p.B; ++b) {
        if (live_rows(p.ql, b, p.Lq, I0) == 0) continue;                 // no live row in this workgroup (uniform)
        int klen = p.kl ? p.kl[b] : p.Lk;
        klen = klen < 0 ? 0 : (klen > p.Lk ? p.Lk : klen);
        const int nlive = (klen + BLK - 1) / BLK;                        // live key blocks: 0 .. nlive - 1
        if (nlive == 0) continue;
        const bool row_live = row_ok && live_rows(p.ql, b, p.Lq, I) > 0;
        __syncthreads();                                                 // the previous sample's reads of qt / kt are done
        if (tid < 4 * 32) {
            const int r = tid >> 5, c4 = (tid & 31) * 4;
            f32x4 q4 = {0.f, 0.f, 0.f, 0.f};
            if (I0 + r < p.nqb)
                q4 = *reinterpret_cast<const f32x4*>(p.qm + (((int64_t)b * p.H + h) * p.nqb + I0 + r) * BLK + c4);
            *reinterpret_cast<f32x4*>(&qt[r * BLK + c4]) = q4;
        }
        const float* kbase = p.km + ((int64_t)b * p.H + h) * p.nkb * BLK;
        float e[SEL_T];
#pragma unroll
        for (int t = 0; t < SEL_T; ++t) {
            e[t] = 0.f;
            if (t * 64 < nlive) {                                        // uniform over the workgroup
                if (t > 0) __syncthreads();
                const int rows = min(64, nlive - t * 64);
#pragma unroll
                for (int i = 0; i < 8; ++i) {                            // 64 rows x 128 floats, 16 bytes per thread and pass
                    const int f = (i * 256 + tid) * 4, r = f >> 7;
                    f32x4 k4 = {0.f, 0.f, 0.f, 0.f};
                    if (r < rows) k4 = *reinterpret_cast<const f32x4*>(kbase + (int64_t)t * 64 * BLK + f);
                    *reinterpret_cast<f32x4*>(&kt[f]) = k4;
                }
                __syncthreads();
                float acc = 0.f;
#pragma unroll 8
                for (int d4 = 0; d4 < 32; ++d4) {
                    const int d = ((d4 + lane) * 4) & (BLK - 1);
                    const f32x4 k4 = *reinterpret_cast<const f32x4*>(&kt[lane * BLK + d]);
                    const f32x4 q4 = *reinterpret_cast<const f32x4*>(&qt[w * BLK + d]);
                    acc = fmaf(k4[0], q4[0], acc);
                    acc = fmaf(k4[1], q4[1], acc);
                    acc = fmaf(k4[2], q4[2], acc);
                    acc = fmaf(k4[3], q4[3], acc);
                }
                e[t] = acc;
            }
        }
        if (!row_live) continue;                                         // (wave-uniform; no barrier below)
        // s = scale q.k + log2(live keys); p ~ 2^(s - max s) over the live key blocks
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < SEL_T; ++t) {
            const int J = lane + 64 * t;
            if (J < nlive) {
                const int cj = min(BLK, klen - J * BLK);
                e[t] = fmaf(p.scale, e[t], __log2f((float)cj));
                mx = fmaxf(mx, e[t]);
            }
        }
        mx = wave_max(mx);
        uint32_t bits[SEL_T];
        float z = 0.f;
#pragma unroll
        for (int t = 0; t < SEL_T; ++t) {
            const int J = lane + 64 * t;
            e[t] = J < nlive ? exp2f(e[t] - mx) : 0.f;
            bits[t] = __float_as_uint(e[t]);
            z += e[t];
        }
        z = wave_sum(z);
        // the largest bit pattern u with  sum_{e >= u} e >= mass z  (the sum is monotone in u: fixed order, terms >= 0)
        uint32_t lo = 0u;
        if (p.mass < 1.f) {
            const float target = p.mass * z;
            uint32_t hi = 0x3f800001u;                                   // e <= 1: nothing reaches it
            while (hi - lo > 1u) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                float s = 0.f;
#pragma unroll
                for (int t = 0; t < SEL_T; ++t) s += bits[t] >= mid ? e[t] : 0.f;
                s = wave_sum(s);
                if (s >= target) lo = mid; else hi = mid;
            }
        }
        const bool q_low = p.min_coh > 0.f && p.qc[((int64_t)b * p.H + h) * p.nqb + I] < p.min_coh;
#pragma unroll
        for (int t = 0; t < SEL_T; ++t) {
            const int J = lane + 64 * t;
            if (J < nlive) {
                bool keep = bits[t] >= lo || q_low;
                if (p.min_coh > 0.f && !keep) keep = p.kc[((int64_t)b * p.H + h) * p.nkb + J] < p.min_coh;
                keep_all |= keep ? (1u << t) : 0u;
            }
        }
    }
    if (!row_ok) return;
    const int ah = p.always_heads == 1 ? 0 : h;
#pragma unroll
    for (int t = 0; t < SEL_T; ++t) {
        const int J = lane + 64 * t;
        if (J < p.nkb) {
            bool keep = (keep_all >> t) & 1u;
            if (p.always) keep = keep || p.always[((int64_t)ah * p.nqb + I) * p.nkb + J] != 0;
            p.mask[((int64_t)h * p.nqb + I) * p.nkb + J] = keep ? 1 : 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Tables.  One wave per list: heads x (q_blocks row lists + k_blocks column lists).  64 entries at a time: a ballot of
// the kept ones, each kept lane writes its index at (entries so far) + (kept lanes below it).
__global__ __launch_bounds__(256) void block_tables_kernel(const uint8_t* __restrict__ mask, int heads, int nq, int nk,
                                                           int32_t* __restrict__ row_cnt, int32_t* __restrict__ row_idx,
                                                           int32_t* __restrict__ col_cnt, int32_t* __restrict__ col_idx) {
    const int lane = threadIdx.x & 63;
    const int list = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int per_head = nq + nk;
    if (list >= heads * per_head) return;                                // (wave-uniform)
    const int h = list / per_head, l = list % per_head;
    const bool is_row = l < nq;
    const int i = is_row ? l : l - nq;                                   // the list's own row (column) of the mask
    const int n = is_row ? nk : nq;                                      // entries to look at
    const int64_t stride = is_row ? 1 : nk;
    const uint8_t* src = mask + (int64_t)h * nq * nk + (is_row ? (int64_t)i * nk : (int64_t)i);
    int32_t* idx = is_row ? row_idx + ((int64_t)h * nq + i) * nk : col_idx + ((int64_t)h * nk + i) * nq;
    int cnt = 0;
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        const bool kept = j < n && src[(int64_t)j * stride] != 0;
        const unsigned long long bal = __ballot(kept);
        const int below = __popcll(bal & ((1ull << lane) - 1ull));
        if (kept) idx[cnt + below] = j;
        cnt += __popcll(bal);
    }
    if (lane == 0) (is_row ? row_cnt + (int64_t)h * nq : col_cnt + (int64_t)h * nk)[i] = cnt;
}

}  // namespace

extern "C" int omh_block_pool_d128(const omh_block_pool_operand* operands, int32_t n_ops, int32_t B, int32_t H,
                                   omh_stream_t stream) {
    if (!operands || n_ops < 1 || n_ops > 2 || B <= 0 || H <= 0) return OMH_E_BADARG;
    PoolParams p = {};
    p.B = B;
    p.H = H;
    int64_t total = 0;
    for (int i = 0; i < n_ops; ++i) {
        const omh_block_pool_operand& o = operands[i];
        if (!o.x || !o.mean || !o.coh || o.L <= 0 || o.ld < (int64_t)H * BLK) return OMH_E_BADARG;
        if (((uintptr_t)o.x & 15) || (o.ld & 7) || (((uintptr_t)o.mean | (uintptr_t)o.coh | (uintptr_t)o.lens) & 3))
            return OMH_E_ALIGN;
        const int nb = (o.L + BLK - 1) / BLK;
        p.op[i] = PoolOp{(const uint16_t*)o.x, o.ld, o.lens, o.mean, o.coh, o.L, nb};
        if (i == 1) p.first1 = (int)total;
        total += (int64_t)B * H * nb;
        if (total > 0x7fffffffLL) return OMH_E_SHAPE;
    }
    if (n_ops == 1) p.first1 = (int)total;
    omh_clear_status();
    hipLaunchKernelGGL(block_pool_kernel, dim3((unsigned)total), dim3(256), 0, (hipStream_t)stream, p);
    return omh_launch_status();
}

extern "C" int omh_block_select(const omh_block_select_args* a, omh_stream_t stream) {
    if (!a || !a->q_mean || !a->q_coh || !a->k_mean || !a->k_coh || !a->mask) return OMH_E_BADARG;
    if (a->B <= 0 || a->H <= 0 || a->Lq <= 0 || a->Lk <= 0) return OMH_E_BADARG;
    if (!(a->mass > 0.f && a->mass <= 1.f) || !(a->min_coherence >= 0.f && a->min_coherence <= 1.f)) return OMH_E_BADARG;
    if (a->always && a->always_heads != 1 && a->always_heads != a->H) return OMH_E_BADARG;
    if (((uintptr_t)a->q_mean | (uintptr_t)a->k_mean) & 15) return OMH_E_ALIGN;
    if (((uintptr_t)a->q_coh | (uintptr_t)a->k_coh | (uintptr_t)a->q_lens | (uintptr_t)a->k_lens) & 3) return OMH_E_ALIGN;
    const int nqb = (a->Lq + BLK - 1) / BLK, nkb = (a->Lk + BLK - 1) / BLK;
    if (nkb > 64 * SEL_T || a->H > 65535) return OMH_E_SHAPE;
    SelParams p = {a->q_mean, a->q_coh, a->k_mean, a->k_coh, a->q_lens, a->k_lens, a->always, a->mask,
                   a->B, a->H, a->Lq, a->Lk, nqb, nkb, a->always ? a->always_heads : 1,
                   a->score_scale, a->mass, a->min_coherence};
    omh_clear_status();
    hipLaunchKernelGGL(block_select_kernel, dim3((unsigned)((nqb + 3) / 4), (unsigned)a->H), dim3(256), 0,
                       (hipStream_t)stream, p);
    return omh_launch_status();
}

extern "C" int omh_block_mask_tables(const uint8_t* mask, int32_t heads, int32_t q_blocks, int32_t k_blocks,
                                     int32_t* row_cnt, int32_t* row_idx, int32_t* col_cnt, int32_t* col_idx,
                                     omh_stream_t stream) {
    if (!mask || !row_cnt || !row_idx || !col_cnt || !col_idx || heads <= 0 || q_blocks <= 0 || k_blocks <= 0)
        return OMH_E_BADARG;
    if (((uintptr_t)row_cnt | (uintptr_t)row_idx | (uintptr_t)col_cnt | (uintptr_t)col_idx) & 3) return OMH_E_ALIGN;
    const int64_t lists = (int64_t)heads * ((int64_t)q_blocks + k_blocks);
    if (lists > 0x7fffffffLL) return OMH_E_SHAPE;
    omh_clear_status();
    hipLaunchKernelGGL(block_tables_kernel, dim3((unsigned)((lists + 3) / 4)), dim3(256), 0, (hipStream_t)stream, mask,
                       (int)heads, (int)q_blocks, (int)k_blocks, row_cnt, row_idx, col_cnt, col_idx);
    return omh_launch_status();
}
