// Low-rank adapters (LoRA) on the effective-weight form, for gfx950.
//
// The hot path never reads the fp32 master weights: it reads bf16 operand copies (omh_pack_weights_multi).  With an
// adapter W_eff = W + s B A  (A fp32 [rank, cols], B fp32 [rows, rank], s = alpha / rank) the pack step writes
// bf16(W_eff) instead of bf16(W), and every fused GEMM of the forward and the backward runs unchanged.  Three pieces:
//   * omh_pack_weights_lora_multi — omh_pack_weights_multi's tiles, layouts and ragged edges with the rank-r sum added
//     before the one rounding to bf16;
//   * omh_lora_merge — the same kernel writing fp32 W_eff back over W (same staging, same device function, hence the
//     same fp32 value: a plain pack after a merge gives the bits of the fused pack);
//   * omh_lora_grads — the adapter gradients without forming dW:  U = X A^T, T = dY B (bf16 [M, rank]) and then
//     dB = s dY^T U, dA = s T^T X, contracted over the M rows.  These products are tall and skinny (N = rank <= 128):
//     one wave per 32-wide strip, v_mfma_f32_32x32x16_bf16 with fp32 accumulation, a fixed split over M whose partial
//     sums a second pass adds in a fixed order — no atomics, the result repeats bit for bit.
#include "omh_common.h"

namespace {

constexpr int LP_COLS = 13;                                       // table columns of the pack / merge entries
constexpr int RC = 32;                                            // rank chunk staged in LDS

// THE rank-r sum of the effective weight: for the 4 x 4 elements a thread owns (rows rl0 + 16 j, columns tc .. tc + 3
// of the 64 x 64 tile), acc += sum over the staged ranks in ascending order, one fused multiply-add per rank.  Shared
// by the pack and the merge instantiation, so both see the same fp32 value.
__device__ __forceinline__ void lora_accumulate(float (&acc)[4][4], const float (*Bs)[RC + 1], const float (*As)[64],
                                                const int rl0, const int tc, const int n) {
    for (int r = 0; r < n; ++r) {
        const float a0 = As[r][tc], a1 = As[r][tc + 1], a2 = As[r][tc + 2], a3 = As[r][tc + 3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float b = Bs[rl0 + 16 * j][r];
            acc[j][0] = __builtin_fmaf(b, a0, acc[j][0]);
            acc[j][1] = __builtin_fmaf(b, a1, acc[j][1]);
            acc[j][2] = __builtin_fmaf(b, a2, acc[j][2]);
            acc[j][3] = __builtin_fmaf(b, a3, acc[j][3]);
        }
    }
}
__device__ __forceinline__ float lora_apply(const float w, const float s, const float acc) {
    return __builtin_fmaf(s, acc, w);
}

// entry e of the device table = omh_pack_weights_multi's nine columns + {A, B, rank, scale (fp32 bits)}; A == 0: no
// adapter, the entry is packed exactly as omh_pack_weights_multi packs it.  MERGE: src = fp32 W_eff, no copies.
template <bool MERGE>
__global__ __launch_bounds__(256)
void lora_pack_kernel(const int64_t* __restrict__ table, int n_entries) {
    __shared__ uint16_t tile[64][66];
    __shared__ float As[RC][64];
    __shared__ float Bs[64][RC + 1];
    const int64_t t = blockIdx.x;
    int lo = 0, hi = n_entries - 1;                               // last entry whose first tile is <= t
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(int64_t)mid * LP_COLS + 7] <= t) lo = mid; else hi = mid - 1;
    }
    const int64_t* e = table + (int64_t)lo * LP_COLS;
    float* src = (float*)e[0];
    const int64_t rows = e[3], cols = e[4], ld_dst = e[5], ld_t = e[6];
    const int64_t local = t - e[7];
    const int tid = threadIdx.x;
    if (e[8] == 1) {                                              // fp32 copy
        if (MERGE) return;
        float* dstf = (float*)e[1];
        const int64_t n = rows * cols, i0 = local * 4096;
        for (int64_t i = i0 + tid; i < min(n, i0 + 4096); i += 256) dstf[i] = src[i];
        return;
    }
    const float* A = (const float*)e[9];
    const float* B = (const float*)e[10];
    const int rank = (int)e[11];
    const float s = __uint_as_float((uint32_t)e[12]);
    uint16_t* dst = MERGE ? nullptr : (uint16_t*)e[1];
    uint16_t* dstT = MERGE ? nullptr : (uint16_t*)e[2];
    const int64_t tiles_c = (cols + 63) >> 6;
    const int64_t r0 = (local / tiles_c) << 6, c0 = (local % tiles_c) << 6;
    const bool vec = (cols & 3) == 0;
    const int tr = tid >> 4, tc = (tid & 15) << 2;
    float4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t r = r0 + tr + 16 * j, c = c0 + tc;
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < rows) {
            if (vec && c + 3 < cols) v[j] = *(const float4*)(src + r * cols + c);
            else {
                if (c < cols) v[j].x = src[r * cols + c];
                if (c + 1 < cols) v[j].y = src[r * cols + c + 1];
                if (c + 2 < cols) v[j].z = src[r * cols + c + 2];
                if (c + 3 < cols) v[j].w = src[r * cols + c + 3];
            }
        }
    }
    if (A && B && rank > 0) {                                     // workgroup-uniform
        float acc[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[j][i] = 0.f;
        for (int k0 = 0; k0 < rank; k0 += RC) {
            const int n = min(RC, rank - k0);
            __syncthreads();                                      // the previous chunk has been consumed
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int idx = tid + 256 * i;
                const int ra = idx >> 6, ca = idx & 63;           // A chunk [RC][64]: rank row, tile column
                As[ra][ca] = (ra < n && c0 + ca < cols) ? A[(int64_t)(k0 + ra) * cols + c0 + ca] : 0.f;
                const int rb = idx / RC, kb = idx % RC;           // B chunk [64][RC]: tile row, rank
                Bs[rb][kb] = (kb < n && r0 + rb < rows) ? B[(r0 + rb) * rank + k0 + kb] : 0.f;
            }
            __syncthreads();
            lora_accumulate(acc, Bs, As, tr, tc, n);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j].x = lora_apply(v[j].x, s, acc[j][0]);
            v[j].y = lora_apply(v[j].y, s, acc[j][1]);
            v[j].z = lora_apply(v[j].z, s, acc[j][2]);
            v[j].w = lora_apply(v[j].w, s, acc[j][3]);
        }
    }
    if (MERGE) {
        if (!(A && B && rank > 0)) return;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t r = r0 + tr + 16 * j, c = c0 + tc;
            if (r >= rows) continue;
            if (vec && c + 3 < cols) *(float4*)(src + r * cols + c) = v[j];
            else {
                if (c < cols) src[r * cols + c] = v[j].x;
                if (c + 1 < cols) src[r * cols + c + 1] = v[j].y;
                if (c + 2 < cols) src[r * cols + c + 2] = v[j].z;
                if (c + 3 < cols) src[r * cols + c + 3] = v[j].w;
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int rl = tr + 16 * j;
        const int64_t r = r0 + rl, c = c0 + tc;
        const uint32_t lo2 = pack_bf2(v[j].x, v[j].y), hi2 = pack_bf2(v[j].z, v[j].w);
        if (dst && r < rows) {
            if ((ld_dst & 3) == 0 && c + 3 < cols) *(uint2*)(dst + r * ld_dst + c) = make_uint2(lo2, hi2);
            else {
                if (c < cols) dst[r * ld_dst + c] = (uint16_t)(lo2 & 0xffff);
                if (c + 1 < cols) dst[r * ld_dst + c + 1] = (uint16_t)(lo2 >> 16);
                if (c + 2 < cols) dst[r * ld_dst + c + 2] = (uint16_t)(hi2 & 0xffff);
                if (c + 3 < cols) dst[r * ld_dst + c + 3] = (uint16_t)(hi2 >> 16);
            }
        }
        *(uint32_t*)&tile[rl][tc] = lo2;
        *(uint32_t*)&tile[rl][tc + 2] = hi2;
    }
    if (!dstT) return;                                            // workgroup-uniform
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int cl = tr + 16 * j;                               // source column = row of the transposed copy
        const int64_t c = c0 + cl, r = r0 + tc;
        if (c >= cols) continue;
        const uint16_t a0 = tile[tc][cl], a1 = tile[tc + 1][cl], a2 = tile[tc + 2][cl], a3 = tile[tc + 3][cl];
        if ((ld_t & 3) == 0 && r + 3 < rows) {
            *(uint2*)(dstT + c * ld_t + r) = make_uint2((uint32_t)a0 | ((uint32_t)a1 << 16), (uint32_t)a2 | ((uint32_t)a3 << 16));
        } else {
            if (r < rows) dstT[c * ld_t + r] = a0;
            if (r + 1 < rows) dstT[c * ld_t + r + 1] = a1;
            if (r + 2 < rows) dstT[c * ld_t + r + 2] = a2;
            if (r + 3 < rows) dstT[c * ld_t + r + 3] = a3;
        }
    }
}

// ---------------------------------------------------------------------------------------------- adapter gradients
typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));

struct LoraGeom {
    uint16_t* U;                                                  // bf16 [M, rp]: X A^T   (columns >= rank are zero)
    uint16_t* T;                                                  // bf16 [M, rp]: dY B
    float* partial;                                               // fp32 [splits][out * rank + rank * in]
    int rp, splits, rows_per_split;
};

// Fragment of v_mfma_f32_32x32x16_bf16: lane l (r = l & 31, h = l >> 5) holds A[row r][k = 8 h + j] and
// B[k = 8 h + j][col r], j = 0..7; the result has col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h.

// U = X A^T (blockIdx.y = 0) and T = dY B (1): one wave per 32 rows of M, the contraction index contiguous in the
// activation (16-byte loads), the fp32 adapter matrix rounded to bf16 as it is loaded.
template <int NT>
__global__ __launch_bounds__(64)
void lora_proj_kernel(const omh_lora_grad_args p, const LoraGeom g) {
    const int which = blockIdx.y;
    const uint16_t* L = (const uint16_t*)(which ? p.dy : p.x);
    const int64_t ld = which ? p.lddy : p.ldx;
    const int K = which ? p.out_features : p.in_features;
    const float* W = which ? p.B : p.A;                           // element (j, k): A[j][k] or B[k][j]
    const int64_t sj = which ? 1 : p.in_features, sk = which ? p.rank : 1;
    uint16_t* O = which ? g.T : g.U;
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int64_t m = (int64_t)blockIdx.x * 32 + r;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    for (int k0 = 0; k0 < K; k0 += 16) {
        const int k = k0 + 8 * h;                                 // K % 8 == 0: the eight elements are in or out together
        u16x8 a = {0, 0, 0, 0, 0, 0, 0, 0};
        if (m < p.M && k < K) a = *(const u16x8*)(L + m * ld + k);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int j = t * 32 + r;
            u16x8 b = {0, 0, 0, 0, 0, 0, 0, 0};
            if (j < p.rank && k < K) {
                const float* w = W + j * sj + (int64_t)k * sk;
#pragma unroll
                for (int i = 0; i < 8; ++i) b[i] = f2bf(w[i * sk]);
            }
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                             acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t mi = (int64_t)blockIdx.x * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (mi < p.M) O[mi * g.rp + t * 32 + r] = f2bf(acc[t][i]);      // (columns >= rank: zero, b was zero)
        }
}

// eight rows m0 .. m0 + 7 of one column of a row-major bf16 matrix: an MFMA fragment whose contraction index runs
// down the rows
__device__ __forceinline__ bf16x8 lora_col_frag(const uint16_t* __restrict__ base, const int64_t ld, const int64_t m0,
                                                const int64_t m_end, const int col, const int ncols) {
    u16x8 f = {0, 0, 0, 0, 0, 0, 0, 0};
    if (col < ncols) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (m0 + i < m_end) f[i] = base[(m0 + i) * ld + col];
    }
    return __builtin_bit_cast(bf16x8, f);
}

// partial dB = dY^T U (blockIdx.z = 0) and partial dA = T^T X (1) over the rows of split blockIdx.y: one wave per 32
// columns of the wide operand (dY: out, X: in) and all rank columns of the skinny one.
template <int NT>
__global__ __launch_bounds__(64)
void lora_grad_kernel(const omh_lora_grad_args p, const LoraGeom g) {
    const int which = blockIdx.z;
    const int wide_n = which ? p.in_features : p.out_features;
    const int w0 = blockIdx.x * 32;
    if (w0 >= wide_n) return;
    const uint16_t* Wd = (const uint16_t*)(which ? p.x : p.dy);
    const int64_t ldw = which ? p.ldx : p.lddy;
    const uint16_t* Sk = which ? g.T : g.U;
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int64_t m_begin = (int64_t)blockIdx.y * g.rows_per_split;
    const int64_t m_end = min((int64_t)p.M, m_begin + g.rows_per_split);
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    for (int64_t mb = m_begin; mb < m_end; mb += 16) {
        const bf16x8 fw = lora_col_frag(Wd, ldw, mb + 8 * h, m_end, w0 + r, wide_n);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const bf16x8 fs = lora_col_frag(Sk, g.rp, mb + 8 * h, m_end, t * 32 + r, g.rp);
            acc[t] = which ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(fs, fw, acc[t], 0, 0, 0)      // rows: rank, cols: in
                           : __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw, fs, acc[t], 0, 0, 0);     // rows: out, cols: rank
        }
    }
    const int64_t n_b = (int64_t)p.out_features * p.rank, n_a = (int64_t)p.rank * p.in_features;
    float* part = g.partial + (int64_t)blockIdx.y * (n_b + n_a) + (which ? n_b : 0);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
            if (which) {                                          // dA[j][q]
                const int j = t * 32 + row, q = w0 + r;
                if (j < p.rank && q < p.in_features) part[(int64_t)j * p.in_features + q] = acc[t][i];
            } else {                                              // dB[o][j]
                const int o = w0 + row, j = t * 32 + r;
                if (o < p.out_features && j < p.rank) part[(int64_t)o * p.rank + j] = acc[t][i];
            }
        }
}

// dB | dA (+)= s * (partial sums added in ascending split order)
__global__ __launch_bounds__(256)
void lora_reduce_kernel(const omh_lora_grad_args p, const LoraGeom g) {
    const int64_t n_b = (int64_t)p.out_features * p.rank, n = n_b + (int64_t)p.rank * p.in_features;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float sum = g.partial[i];
        for (int sp = 1; sp < g.splits; ++sp) sum += g.partial[(int64_t)sp * n + i];
        const float val = p.scale * sum;
        const bool is_a = i >= n_b;
        float* dst = is_a ? p.dA + (i - n_b) : p.dB + i;
        const bool add = is_a ? (p.accumulate & 1) : (p.accumulate & 2);
        *dst = add ? *dst + val : val;
    }
}

inline int lora_rp(int rank) { return (rank + 31) / 32 * 32; }

// the split over M depends on the shapes alone: about two waves per SIMD-pair slot of the chip, at least 64 rows each
inline void lora_plan(const omh_lora_grad_args& a, int& splits, int& rows_per_split) {
    const int wide = a.in_features > a.out_features ? a.in_features : a.out_features;
    const int tiles = (wide + 31) / 32;
    int s = 1024 / (2 * tiles);
    const int smax = (a.M + 63) / 64;
    s = s > 32 ? 32 : s;
    s = s > smax ? smax : s;
    s = s < 1 ? 1 : s;
    rows_per_split = ((a.M + s - 1) / s + 15) / 16 * 16;
    splits = (a.M + rows_per_split - 1) / rows_per_split;
}

inline int64_t lora_ut_bytes(const omh_lora_grad_args& a) {
    return (((int64_t)a.M * lora_rp(a.rank) * 2) + 255) / 256 * 256;
}

int lora_check(const omh_lora_grad_args& a) {
    if (a.M <= 0 || a.in_features <= 0 || a.out_features <= 0) return OMH_E_BADARG;
    if (a.rank < 1 || a.rank > 128) return OMH_E_SHAPE;
    if ((a.in_features & 7) || (a.out_features & 7) || (a.ldx & 7) || (a.lddy & 7) || a.ldx < a.in_features ||
        a.lddy < a.out_features) return OMH_E_ALIGN;
    return 0;
}

}  // namespace

extern "C" int omh_pack_weights_lora_multi(const int64_t* table, int32_t n_entries, int64_t total_tiles, omh_stream_t stream) {
    if (!table || n_entries <= 0 || total_tiles <= 0 || total_tiles > 0x7fffffffLL) return OMH_E_BADARG;
    omh_clear_status();
    hipLaunchKernelGGL(lora_pack_kernel<false>, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, table,
                       n_entries);
    return omh_launch_status();
}

extern "C" int omh_lora_merge(const int64_t* table, int32_t n_entries, int64_t total_tiles, omh_stream_t stream) {
    if (!table || n_entries <= 0 || total_tiles <= 0 || total_tiles > 0x7fffffffLL) return OMH_E_BADARG;
    omh_clear_status();
    hipLaunchKernelGGL(lora_pack_kernel<true>, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, table,
                       n_entries);
    return omh_launch_status();
}

extern "C" int64_t omh_lora_grads_workspace_bytes(const omh_lora_grad_args* args) {
    if (!args || lora_check(*args) != 0) return 0;
    int splits, rps;
    lora_plan(*args, splits, rps);
    const int64_t n = (int64_t)args->out_features * args->rank + (int64_t)args->rank * args->in_features;
    return 2 * lora_ut_bytes(*args) + (int64_t)splits * n * 4;
}

extern "C" int omh_lora_grads(const omh_lora_grad_args* args, omh_stream_t stream) {
    if (!args || !args->x || !args->dy || !args->A || !args->B || !args->dA || !args->dB || !args->workspace)
        return OMH_E_BADARG;
    const omh_lora_grad_args& a = *args;
    const int rc = lora_check(a);
    if (rc != 0) return rc;
    if (((uintptr_t)a.x & 15) || ((uintptr_t)a.dy & 15) || ((uintptr_t)a.workspace & 15) || ((uintptr_t)a.dA & 3) ||
        ((uintptr_t)a.dB & 3)) return OMH_E_ALIGN;
    if (a.workspace_bytes < omh_lora_grads_workspace_bytes(args)) return OMH_E_BADARG;
    LoraGeom g;
    g.rp = lora_rp(a.rank);
    lora_plan(a, g.splits, g.rows_per_split);
    const int64_t ut = lora_ut_bytes(a);
    g.U = (uint16_t*)a.workspace;
    g.T = (uint16_t*)((unsigned char*)a.workspace + ut);
    g.partial = (float*)((unsigned char*)a.workspace + 2 * ut);
    hipStream_t s = (hipStream_t)stream;
    const int nt = g.rp / 32;
    const int wide = a.in_features > a.out_features ? a.in_features : a.out_features;
    const dim3 gp((unsigned)((a.M + 31) / 32), 2), gg((unsigned)((wide + 31) / 32), (unsigned)g.splits, 2);
    omh_clear_status();
    switch (nt) {
        case 1:
            hipLaunchKernelGGL(lora_proj_kernel<1>, gp, dim3(64), 0, s, a, g);
            hipLaunchKernelGGL(lora_grad_kernel<1>, gg, dim3(64), 0, s, a, g);
            break;
        case 2:
            hipLaunchKernelGGL(lora_proj_kernel<2>, gp, dim3(64), 0, s, a, g);
            hipLaunchKernelGGL(lora_grad_kernel<2>, gg, dim3(64), 0, s, a, g);
            break;
        case 3:
            hipLaunchKernelGGL(lora_proj_kernel<3>, gp, dim3(64), 0, s, a, g);
            hipLaunchKernelGGL(lora_grad_kernel<3>, gg, dim3(64), 0, s, a, g);
            break;
        default:
            hipLaunchKernelGGL(lora_proj_kernel<4>, gp, dim3(64), 0, s, a, g);
            hipLaunchKernelGGL(lora_grad_kernel<4>, gg, dim3(64), 0, s, a, g);
            break;
    }
    const int64_t n = (int64_t)a.out_features * a.rank + (int64_t)a.rank * a.in_features;
    int64_t blocks = (n + 255) / 256;
    blocks = blocks > 2048 ? 2048 : blocks;
    hipLaunchKernelGGL(lora_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, g);
    return omh_launch_status();
}
