// The distribution-matching (DMD) objective of self forcing for gfx950: the score-difference gradient between a frozen
// teacher's and a trainable critic's velocity on a noised clip, its per-sample normaliser and the loss value
// (include/omh.h, omh_dmd_grad; DMD2 / Self-Forcing form in the flow parameterisation).  As a chain of torch ops this is
// about 12 launches with two library-chosen reductions in the middle of a step that is otherwise bit-repeatable under
// omh_set_deterministic(1); here it is four launches with fixed-order fp64 reductions, after the pattern of
// omh_grad_norm_multi (optim.hip): one workgroup per DMD_CHUNK-element chunk of ONE sample writes one fp64 partial, a
// small launch adds the partials in a fixed order.  No atomics; nothing depends on the order in which workgroups run.
// The kernels move five tensors once or twice: beside three DiT forwards they are noise — they are here for exactness,
// repeatability and the absence of a host synchronisation, not for speed.
#include "omh_common.h"

namespace {

constexpr int DMD_CHUNK = OMH_DMD_CHUNK;
static_assert(DMD_CHUNK % 1024 == 0, "a chunk is whole rounds of 256 threads x 4 elements");

// Every product is rounded on its own: the build's -ffp-contract=fast would otherwise fuse per loop shape, and a sample
// must give the same bits through the float4 body and through the scalar path (flow_x0_one, dit_elementwise.hip).
__device__ __forceinline__ float rounded(float a) {
    asm volatile("" : "+v"(a));
    return a;
}
// v_real = v_u + g (v_c - v_u); without an unconditional branch v_real = v_c
template <bool CFG>
__device__ __forceinline__ float v_real_of(float vc, float vu, float g) {
    if (!CFG) return vc;
    return vu + rounded(g * (vc - vu));
}

// Element j of a chunk [i0, i1) belongs to thread ((j - i0) / 4) % 256, round (j - i0) / 1024, slot (j - i0) % 4 — whatever
// the pointers' alignment: 16-byte aligned samples load whole groups of four as float4, everything else element by element,
// and both add into the thread's fp64 accumulator in the same order.  So the bits of a sample do not depend on where it lies.
struct Chunk {
    int64_t base, i0, i1;      // flat offset of the sample; the chunk's range inside the sample
    int b;
};
__device__ __forceinline__ Chunk chunk_of(int64_t n, int64_t chunks_per_sample) {
    Chunk c;
    const int64_t t = blockIdx.x;
    c.b = (int)(t / chunks_per_sample);
    c.i0 = (t - (int64_t)c.b * chunks_per_sample) * DMD_CHUNK;
    c.i1 = c.i0 + DMD_CHUNK < n ? c.i0 + DMD_CHUNK : n;
    c.base = (int64_t)c.b * n;
    return c;
}
__device__ __forceinline__ bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
__device__ __forceinline__ void load4(const float* __restrict__ p, int m, bool vec, float (&o)[4]) {
    if (vec && m == 4) {
        const float4 v = *(const float4*)p;
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = k < m ? p[k] : 0.f;
    }
}
// the workgroup's sum, fixed order: across the wave by xor shuffles, the four waves as (0 + 1) + (2 + 3); valid in thread 0
__device__ __forceinline__ double block_sum(double s, double* wsum) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    return (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// launch 1: partial[chunk] = sum |p_real|, p_real = (x - x_t) + sigma_b v_real, in fp64
template <bool CFG>
__global__ __launch_bounds__(256)
void dmd_abs_kernel(const float* __restrict__ x, const float* __restrict__ xt, const float* __restrict__ vc,
                    const float* __restrict__ vu, const float* __restrict__ sigma, float guide, int64_t n,
                    int64_t chunks_per_sample, double* __restrict__ partial) {
    __shared__ double wsum[4];
    const Chunk c = chunk_of(n, chunks_per_sample);
    const float s = sigma[c.b];
    x += c.base; xt += c.base; vc += c.base;
    if (CFG) vu += c.base;
    const bool vec = aligned16(x) && aligned16(xt) && aligned16(vc) && (!CFG || aligned16(vu));
    double acc = 0.0;
    for (int64_t j = c.i0 + 4 * (int64_t)threadIdx.x; j < c.i1; j += 1024) {
        const int m = c.i1 - j < 4 ? (int)(c.i1 - j) : 4;
        float xa[4], ta[4], ca[4], ua[4] = {0.f, 0.f, 0.f, 0.f};
        load4(x + j, m, vec, xa);
        load4(xt + j, m, vec, ta);
        load4(vc + j, m, vec, ca);
        if (CFG) load4(vu + j, m, vec, ua);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float p = (xa[k] - ta[k]) + rounded(s * v_real_of<CFG>(ca[k], ua[k], guide));
            if (k < m) acc += (double)fabsf(p);
        }
    }
    const double tot = block_sum(acc, wsum);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// launch 2, one workgroup per sample: thread i adds the sample's partials i, i + 256, ... , then a fixed tree over the 256
// sums; n_b = mean |p_real| rounded ONCE to fp32
__global__ __launch_bounds__(256)
void dmd_norm_kernel(const double* __restrict__ partial, int64_t chunks_per_sample, int64_t n, float* __restrict__ norm) {
    __shared__ double acc[256];
    const double* p = partial + (int64_t)blockIdx.x * chunks_per_sample;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < chunks_per_sample; i += 256) s += p[i];
    acc[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) acc[threadIdx.x] += acc[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) norm[blockIdx.x] = (float)(acc[0] / (double)n);
}

// torch.nan_to_num's defaults: NaN -> 0, +-inf -> +-FLT_MAX
__device__ __forceinline__ float nan_to_num(float q) {
    if (q != q) return 0.f;
    if (q > 3.402823466e+38f) return 3.402823466e+38f;
    if (q < -3.402823466e+38f) return -3.402823466e+38f;
    return q;
}

// launch 3: grad = nan_to_num(sigma_b (v_real - v_fake) / n_b), stored; partial[chunk] = sum of the squares of the fp32
// values as stored, in fp64
template <bool CFG>
__global__ __launch_bounds__(256)
void dmd_grad_kernel(const float* __restrict__ vc, const float* __restrict__ vu, const float* __restrict__ vf,
                     const float* __restrict__ sigma, const float* __restrict__ norm, float guide, int64_t n,
                     int64_t chunks_per_sample, float* __restrict__ grad, double* __restrict__ partial) {
    __shared__ double wsum[4];
    const Chunk c = chunk_of(n, chunks_per_sample);
    const float s = sigma[c.b], nb = norm[c.b];
    vc += c.base; vf += c.base; grad += c.base;
    if (CFG) vu += c.base;
    const bool vec = aligned16(vc) && aligned16(vf) && aligned16(grad) && (!CFG || aligned16(vu));
    double acc = 0.0;
    for (int64_t j = c.i0 + 4 * (int64_t)threadIdx.x; j < c.i1; j += 1024) {
        const int m = c.i1 - j < 4 ? (int)(c.i1 - j) : 4;
        float ca[4], ua[4] = {0.f, 0.f, 0.f, 0.f}, fa[4], ga[4];
        load4(vc + j, m, vec, ca);
        load4(vf + j, m, vec, fa);
        if (CFG) load4(vu + j, m, vec, ua);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float num = rounded(s * (v_real_of<CFG>(ca[k], ua[k], guide) - fa[k]));
            ga[k] = nan_to_num(num / nb);
            if (k < m) acc += (double)ga[k] * (double)ga[k];
        }
        if (vec && m == 4) {
            *(float4*)(grad + j) = make_float4(ga[0], ga[1], ga[2], ga[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < m) grad[j + k] = ga[k];
        }
    }
    const double tot = block_sum(acc, wsum);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// launch 4, one workgroup: all partials in a fixed order (dmd_norm_kernel's), loss = 0.5 * sum / N in fp64
__global__ __launch_bounds__(256)
void dmd_loss_kernel(const double* __restrict__ partial, int64_t n_partials, double total, double* __restrict__ loss) {
    __shared__ double acc[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n_partials; i += 256) s += partial[i];
    acc[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) acc[threadIdx.x] += acc[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = 0.5 * (acc[0] / total);
}

// the backward of the loss: dx = grad * c, c = float(*upstream) * inv_total — one fp32 multiply per element
__global__ __launch_bounds__(256)
void dmd_scale_kernel(const float* __restrict__ grad, const double* __restrict__ upstream, float inv_total, int64_t total,
                      float* __restrict__ dx, int vec_ok) {
    const float c = rounded((float)upstream[0] * inv_total);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nvec = vec_ok ? total / 4 : 0;
    for (int64_t i = tid; i < nvec; i += stride) {
        float4 g = *(const float4*)(grad + 4 * i);
        g.x *= c; g.y *= c; g.z *= c; g.w *= c;
        *(float4*)(dx + 4 * i) = g;
    }
    for (int64_t i = 4 * nvec + tid; i < total; i += stride) dx[i] = grad[i] * c;
}

inline int64_t chunks_of(int64_t n) { return (n + DMD_CHUNK - 1) / DMD_CHUNK; }
// the launches are one workgroup of 256 threads per chunk: 2^23 chunks (2^37 elements) keep the grid inside every limit
constexpr int64_t MAX_CHUNKS = 1LL << 23;

}  // namespace

extern "C" int64_t omh_dmd_grad_workspace_bytes(int32_t B, int64_t n) {
    if (B < 1 || n < 1) return 0;
    return (int64_t)B * chunks_of(n) * OMH_DMD_PARTIAL_BYTES;
}

extern "C" int omh_dmd_grad(const float* x, const float* xt, const float* v_cond, const float* v_uncond, const float* v_fake,
                            const float* sigma, float guide, int32_t B, int64_t n, float* grad, float* norm, double* loss,
                            void* workspace, omh_stream_t stream) {
    if (!x || !xt || !v_cond || !v_fake || !sigma || !grad || !norm || !loss || !workspace) return OMH_E_BADARG;
    if (B < 1 || n < 1) return -2;
    if (((uintptr_t)x | (uintptr_t)xt | (uintptr_t)v_cond | (uintptr_t)v_uncond | (uintptr_t)v_fake | (uintptr_t)sigma |
         (uintptr_t)grad | (uintptr_t)norm) & 3)
        return OMH_E_ALIGN;
    if (((uintptr_t)loss | (uintptr_t)workspace) & 7) return OMH_E_ALIGN;
    const int64_t cps = chunks_of(n);
    if (cps > MAX_CHUNKS / B) return OMH_E_SHAPE;
    const int64_t chunks = (int64_t)B * cps;
    double* part_abs = (double*)workspace;                           // [B][cps] each; two arrays, so that no launch
    double* part_sq = part_abs + chunks;                             // writes what another one of the group reads
    hipStream_t s = (hipStream_t)stream;
    omh_clear_status();
    if (v_uncond)
        hipLaunchKernelGGL(dmd_abs_kernel<true>, dim3((unsigned)chunks), dim3(256), 0, s, x, xt, v_cond, v_uncond, sigma, guide,
                           n, cps, part_abs);
    else
        hipLaunchKernelGGL(dmd_abs_kernel<false>, dim3((unsigned)chunks), dim3(256), 0, s, x, xt, v_cond, v_uncond, sigma, guide,
                           n, cps, part_abs);
    hipLaunchKernelGGL(dmd_norm_kernel, dim3((unsigned)B), dim3(256), 0, s, part_abs, cps, n, norm);
    if (v_uncond)
        hipLaunchKernelGGL(dmd_grad_kernel<true>, dim3((unsigned)chunks), dim3(256), 0, s, v_cond, v_uncond, v_fake, sigma, norm,
                           guide, n, cps, grad, part_sq);
    else
        hipLaunchKernelGGL(dmd_grad_kernel<false>, dim3((unsigned)chunks), dim3(256), 0, s, v_cond, v_uncond, v_fake, sigma, norm,
                           guide, n, cps, grad, part_sq);
    hipLaunchKernelGGL(dmd_loss_kernel, dim3(1), dim3(256), 0, s, part_sq, chunks, (double)B * (double)n, loss);
    return omh_launch_status();
}

extern "C" int omh_dmd_grad_scale(const float* grad, const double* upstream, float inv_total, int64_t total, float* dx,
                                  omh_stream_t stream) {
    if (!grad || !upstream || !dx) return OMH_E_BADARG;
    if (total < 1) return -2;
    if ((((uintptr_t)grad | (uintptr_t)dx) & 3) || ((uintptr_t)upstream & 7)) return OMH_E_ALIGN;
    const int vec_ok = (((uintptr_t)grad | (uintptr_t)dx) & 15) == 0;
    int64_t g = (total / 4 + 255) / 256;
    g = g < 1 ? 1 : (g > 8192 ? 8192 : g);
    omh_clear_status();
    hipLaunchKernelGGL(dmd_scale_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, grad, upstream, inv_total, total, dx,
                       vec_ok);
    return omh_launch_status();
}
