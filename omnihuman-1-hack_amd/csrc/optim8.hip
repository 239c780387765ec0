// AdamW with FP8 block-scaled moments for gfx950 (include/omh.h states the format): the first moment m and the ROOT of
// the second, r = sqrt(v), are kept as OCP e4m3fn codes with one fp32 scale per 64 columns of a row — 2.125 bytes per
// weight instead of 8.  One workgroup per 64 x 64 tile with adamw_pack_kernel's thread mapping (optim.hip): the 16
// lanes with equal tid >> 4 hold one 64-element row segment, which IS one block, so both block maxima are four
// cross-lane steps and the update, the re-quantisation and the bf16 operand copies are one pass.
// The hardware converts (v_cvt_pk_fp8_f32, v_cvt_f32_fp8) are OCP e4m3fn on gfx950, round to nearest even.
#include "omh_common.h"

namespace {

constexpr float E4M3_MAX = 448.0f;

__device__ __forceinline__ float clip_coef() { return 1.0f; }
__device__ __forceinline__ float clip_coef(const float* __restrict__ coef) { return *coef; }

// optim.hip's adamw_one, expression for expression (that file keeps its instruction streams: it is not edited)
template <bool DEV>
__device__ __forceinline__ float adamw_one(float p, float g, float& m, float& v, float lr, float beta1, float beta2, float eps,
                                           float wd, float bc1, float bc2, float inv_scale, float coef) {
    float gi = g * inv_scale;
    if (DEV) gi *= coef;
    const float mi = beta1 * m + (1.0f - beta1) * gi;
    const float vi = beta2 * v + (1.0f - beta2) * gi * gi;
    m = mi;
    v = vi;
    return p * (1.0f - lr * wd) - (lr / bc1) * (mi / (sqrtf(vi) / bc2 + eps));
}

// four codes of one 32-bit word -> fp32 (byte k = element k)
__device__ __forceinline__ void fp8_dec4(uint32_t w, float out[4]) {
    out[0] = __builtin_amdgcn_cvt_f32_fp8((int)w, 0);
    out[1] = __builtin_amdgcn_cvt_f32_fp8((int)w, 1);
    out[2] = __builtin_amdgcn_cvt_f32_fp8((int)w, 2);
    out[3] = __builtin_amdgcn_cvt_f32_fp8((int)w, 3);
}

// max that keeps a NaN once it has one (fmaxf would drop it): a block that met a non-finite value gets a non-finite scale
__device__ __forceinline__ float max_sticky(float acc, float a) { return (a > acc || a != a) ? a : acc; }

// One block's scale and this lane's four codes: x[0..3] are four of the block's 64 values (0 where the tensor ends), the
// 16 lanes of the block are consecutive and all of them are here.  scale = max|x| / 448; code = RNE_e4m3(x / scale),
// clamped to +-448 so that 0x7f / 0xff are never written; an all-zero block: scale 0, codes 0.  ROOT (r = sqrt(v)): a
// positive value never gets code 0 — a live first moment must not meet a zero denominator.
// A block with a non-finite value: NaN -> scale NaN, codes 0; +-inf -> scale inf, codes 0 where the value was finite and
// +-448 where it was not.  Either way the block decodes to non-finite values, as fp32 moments would hold them.
template <bool ROOT>
__device__ __forceinline__ uint32_t fp8_quant4(const float x[4], float& scale) {
    float a = max_sticky(max_sticky(fabsf(x[0]), fabsf(x[1])), max_sticky(fabsf(x[2]), fabsf(x[3])));
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) a = max_sticky(a, __shfl_xor(a, o, 64));
    scale = a / E4M3_MAX;
    float q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = scale > 0.f ? fminf(fmaxf(x[k] / scale, -E4M3_MAX), E4M3_MAX) : 0.f;
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], w, true);
    uint32_t u = (uint32_t)w;
    if (ROOT) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x[k] > 0.f && ((u >> (8 * k)) & 0xffu) == 0u) u |= 1u << (8 * k);
    }
    return u;
}

// last entry whose first tile (column `col` of `ncols`) is <= t
__device__ __forceinline__ int tile_entry(const int64_t* __restrict__ table, int n_entries, int ncols, int col, int64_t t) {
    int lo = 0, hi = n_entries - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(int64_t)mid * ncols + col] <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// four codes at `q + o`: one 32-bit access where the tensor's rows are multiples of four columns, bytes otherwise
// (n = live elements of the quad, 1..4)
__device__ __forceinline__ uint32_t load_codes(const uint8_t* __restrict__ q, int64_t o, bool vec, int n) {
    if (vec) return *(const uint32_t*)(q + o);
    uint32_t w = 0;
    for (int k = 0; k < n; ++k) w |= (uint32_t)q[o + k] << (8 * k);
    return w;
}
__device__ __forceinline__ void store_codes(uint8_t* __restrict__ q, int64_t o, bool vec, int n, uint32_t w) {
    if (vec) { *(uint32_t*)(q + o) = w; return; }
    for (int k = 0; k < n; ++k) q[o + k] = (uint8_t)(w >> (8 * k));
}

// entry e of the device table = {p, g fp32, m codes, m scales, r codes, r scales, dst, dstT, rows, cols, ld_dst, ld_dstT,
// first tile}: AdamW on the tile from the decoded moments, the fresh moments re-quantised per block, then dst = bf16(p)
// and / or dstT = bf16(p)^T through LDS as adamw_pack_kernel writes them (either may be 0).
constexpr int A8_COLS = 13;

template <bool DEV, typename... Coef>
__global__ __launch_bounds__(256)
void adamw8_pack_kernel(const int64_t* __restrict__ table, int n_entries, float lr, float beta1, float beta2, float eps,
                        float wd, float bc1, float bc2, float inv_scale, Coef... coef_p) {
    __shared__ uint16_t tile[64][66];
    const float coef = clip_coef(coef_p...);
    const int64_t t = blockIdx.x;
    const int64_t* e = table + (int64_t)tile_entry(table, n_entries, A8_COLS, 12, t) * A8_COLS;
    float* P = (float*)e[0];
    const float* G = (const float*)e[1];
    uint8_t* MQ = (uint8_t*)e[2];
    float* MS = (float*)e[3];
    uint8_t* RQ = (uint8_t*)e[4];
    float* RS = (float*)e[5];
    uint16_t* dst = (uint16_t*)e[6];
    uint16_t* dstT = (uint16_t*)e[7];
    const int64_t rows = e[8], cols = e[9], ld_dst = e[10], ld_t = e[11];
    const int64_t local = t - e[12];
    const int tid = threadIdx.x;
    const int64_t tiles_c = (cols + 63) >> 6;                     // = blocks per row: tile column b is block b
    const int64_t r0 = (local / tiles_c) << 6, c0 = (local % tiles_c) << 6;
    const bool vec = (cols & 3) == 0;
    const int tr = tid >> 4, tc = (tid & 15) << 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int rl = tr + 16 * j;
        const int64_t r = r0 + rl, c = c0 + tc;
        const bool live = r < rows && c < cols;
        const int n = live ? (int)min((int64_t)4, cols - c) : 0;  // vec: 4 or 0
        const int64_t o = r * cols + c, so = r * tiles_c + (c0 >> 6);
        float pv[4] = {0.f, 0.f, 0.f, 0.f}, mv[4] = {0.f, 0.f, 0.f, 0.f}, rv[4] = {0.f, 0.f, 0.f, 0.f};
        if (live) {
            float p_[4] = {0.f, 0.f, 0.f, 0.f}, g_[4] = {0.f, 0.f, 0.f, 0.f}, md[4], rd[4];
            if (vec) {
                const float4 p4 = *(const float4*)(P + o), g4 = *(const float4*)(G + o);
                p_[0] = p4.x; p_[1] = p4.y; p_[2] = p4.z; p_[3] = p4.w;
                g_[0] = g4.x; g_[1] = g4.y; g_[2] = g4.z; g_[3] = g4.w;
            } else {
                for (int k = 0; k < n; ++k) { p_[k] = P[o + k]; g_[k] = G[o + k]; }
            }
            const float sm = MS[so], sr = RS[so];
            fp8_dec4(load_codes(MQ, o, vec, n), md);
            fp8_dec4(load_codes(RQ, o, vec, n), rd);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) {
                    float m = md[k] * sm;
                    const float ro = rd[k] * sr;
                    float v = ro * ro;
                    pv[k] = adamw_one<DEV>(p_[k], g_[k], m, v, lr, beta1, beta2, eps, wd, bc1, bc2, inv_scale, coef);
                    mv[k] = m;
                    rv[k] = sqrtf(v);
                }
            if (vec) *(float4*)(P + o) = make_float4(pv[0], pv[1], pv[2], pv[3]);
            else for (int k = 0; k < n; ++k) P[o + k] = pv[k];
        }
        float s_m, s_r;                                           // every lane takes part in the block maxima
        const uint32_t mc = fp8_quant4<false>(mv, s_m), rc = fp8_quant4<true>(rv, s_r);
        if (live) {
            store_codes(MQ, o, vec, n, mc);
            store_codes(RQ, o, vec, n, rc);
            if (tc == 0) { MS[so] = s_m; RS[so] = s_r; }
        }
        const uint32_t lo2 = pack_bf2(pv[0], pv[1]), hi2 = pack_bf2(pv[2], pv[3]);
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

// entry e = {fp32 [rows, cols], codes, scales, rows, cols, first tile}; the same tiles and the same rule.
// ROOT: the fp32 tensor is v, the codes hold sqrt(v) (quantize) and the result is squared (dequantize).
constexpr int MQ_COLS = 6;

template <bool ROOT>
__global__ __launch_bounds__(256)
void moments_quantize_kernel(const int64_t* __restrict__ table, int n_entries) {
    const int64_t t = blockIdx.x;
    const int64_t* e = table + (int64_t)tile_entry(table, n_entries, MQ_COLS, 5, t) * MQ_COLS;
    const float* X = (const float*)e[0];
    uint8_t* Q = (uint8_t*)e[1];
    float* S = (float*)e[2];
    const int64_t rows = e[3], cols = e[4], local = t - e[5];
    const int64_t tiles_c = (cols + 63) >> 6;
    const int64_t r0 = (local / tiles_c) << 6, c0 = (local % tiles_c) << 6;
    const bool vec = (cols & 3) == 0;
    const int tr = (int)threadIdx.x >> 4, tc = ((int)threadIdx.x & 15) << 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t r = r0 + tr + 16 * j, c = c0 + tc;
        const bool live = r < rows && c < cols;
        const int n = live ? (int)min((int64_t)4, cols - c) : 0;
        const int64_t o = r * cols + c, so = r * tiles_c + (c0 >> 6);
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (live) {
            if (vec) { const float4 x4 = *(const float4*)(X + o); x[0] = x4.x; x[1] = x4.y; x[2] = x4.z; x[3] = x4.w; }
            else for (int k = 0; k < n; ++k) x[k] = X[o + k];
            if (ROOT) {
#pragma unroll
                for (int k = 0; k < 4; ++k) x[k] = sqrtf(x[k]);
            }
        }
        float s;
        const uint32_t w = fp8_quant4<ROOT>(x, s);
        if (live) {
            store_codes(Q, o, vec, n, w);
            if (tc == 0) S[so] = s;
        }
    }
}

template <bool ROOT>
__global__ __launch_bounds__(256)
void moments_dequantize_kernel(const int64_t* __restrict__ table, int n_entries) {
    const int64_t t = blockIdx.x;
    const int64_t* e = table + (int64_t)tile_entry(table, n_entries, MQ_COLS, 5, t) * MQ_COLS;
    float* X = (float*)e[0];
    const uint8_t* Q = (const uint8_t*)e[1];
    const float* S = (const float*)e[2];
    const int64_t rows = e[3], cols = e[4], local = t - e[5];
    const int64_t tiles_c = (cols + 63) >> 6;
    const int64_t r0 = (local / tiles_c) << 6, c0 = (local % tiles_c) << 6;
    const bool vec = (cols & 3) == 0;
    const int tr = (int)threadIdx.x >> 4, tc = ((int)threadIdx.x & 15) << 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t r = r0 + tr + 16 * j, c = c0 + tc;
        if (r >= rows || c >= cols) continue;
        const int n = (int)min((int64_t)4, cols - c);
        const int64_t o = r * cols + c;
        const float s = S[r * tiles_c + (c0 >> 6)];
        float x[4];
        fp8_dec4(load_codes(Q, o, vec, n), x);
#pragma unroll
        for (int k = 0; k < 4; ++k) { x[k] *= s; if (ROOT) x[k] *= x[k]; }
        if (vec) *(float4*)(X + o) = make_float4(x[0], x[1], x[2], x[3]);
        else for (int k = 0; k < n; ++k) X[o + k] = x[k];
    }
}

inline bool bad_launch(const int64_t* table, int32_t n_entries, int64_t total_tiles) {
    return !table || n_entries <= 0 || total_tiles <= 0 || total_tiles > 0x7fffffffLL;
}

}  // namespace

extern "C" int omh_adamw8_pack_multi(const int64_t* table, int32_t n_entries, int64_t total_tiles, float lr, float beta1,
                                     float beta2, float eps, float weight_decay, int32_t step, float grad_scale,
                                     omh_stream_t stream) {
    if (bad_launch(table, n_entries, total_tiles) || step <= 0 || grad_scale == 0.f) return OMH_E_BADARG;
    const float bc1 = 1.0f - powf(beta1, (float)step);
    const float bc2 = sqrtf(1.0f - powf(beta2, (float)step));
    omh_clear_status();
    hipLaunchKernelGGL((adamw8_pack_kernel<false>), dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, table,
                       n_entries, lr, beta1, beta2, eps, weight_decay, bc1, bc2, 1.0f / grad_scale);
    return omh_launch_status();
}

extern "C" int omh_adamw8_pack_multi_dev(const int64_t* table, int32_t n_entries, int64_t total_tiles, float lr, float beta1,
                                         float beta2, float eps, float weight_decay, int32_t step, float grad_scale,
                                         const float* coef, omh_stream_t stream) {
    if (bad_launch(table, n_entries, total_tiles) || !coef || step <= 0 || grad_scale == 0.f) return OMH_E_BADARG;
    const float bc1 = 1.0f - powf(beta1, (float)step);
    const float bc2 = sqrtf(1.0f - powf(beta2, (float)step));
    omh_clear_status();
    hipLaunchKernelGGL((adamw8_pack_kernel<true, const float*>), dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream,
                       table, n_entries, lr, beta1, beta2, eps, weight_decay, bc1, bc2, 1.0f / grad_scale, coef);
    return omh_launch_status();
}

extern "C" int omh_moments_quantize(const int64_t* table, int32_t n_entries, int64_t total_tiles, int32_t second_moment,
                                    omh_stream_t stream) {
    if (bad_launch(table, n_entries, total_tiles)) return OMH_E_BADARG;
    omh_clear_status();
    if (second_moment)
        hipLaunchKernelGGL(moments_quantize_kernel<true>, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream,
                           table, n_entries);
    else
        hipLaunchKernelGGL(moments_quantize_kernel<false>, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream,
                           table, n_entries);
    return omh_launch_status();
}

extern "C" int omh_moments_dequantize(const int64_t* table, int32_t n_entries, int64_t total_tiles, int32_t second_moment,
                                      omh_stream_t stream) {
    if (bad_launch(table, n_entries, total_tiles)) return OMH_E_BADARG;
    omh_clear_status();
    if (second_moment)
        hipLaunchKernelGGL(moments_dequantize_kernel<true>, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream,
                           table, n_entries);
    else
        hipLaunchKernelGGL(moments_dequantize_kernel<false>, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream,
                           table, n_entries);
    return omh_launch_status();
}
