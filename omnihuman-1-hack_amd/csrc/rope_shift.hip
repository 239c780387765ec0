// Rotate the FRAME part of cached, already rotated keys by a further delta frames (include/omh.h, omh_rope_shift_frames):
// what keeps an attention sink at a fixed rotary distance behind the window of an unbounded rollout
// (causal.RollingKVCache(pin_sink=True)).  RoPE rotations compose, so a key rotated at frame f and then by delta is the
// key rotated at frame f + delta — up to the one more rounding to bf16 this kernel adds.
//
// One 16-byte vector (8 bf16 = 4 rotary pairs) per lane, read once and written once; the kernel is a copy with a few
// multiply-adds on 6 of the 16 vectors of a 128-wide head, and runs at the rate of one.  The cos / sin of the at most
// OMH_ROPE_SHIFT_MAX_PAIRS frame pairs are formed on the HOST in fp64 (the angle delta * theta^(-2j/n) is never an fp32
// product: at delta = 10^6 that product alone is off by up to 0.03 rad) and travel in the kernel arguments: no
// allocation, no copy, nothing the stream has to wait for.  Pairs past the frame part hold the identity (1, 0), and a
// pair under the identity keeps its BITS — so the h / w columns, and every column at delta = 0, are the source's.
#include <math.h>

#include "omh_common.h"

namespace {

constexpr int MAX_PAIRS = OMH_ROPE_SHIFT_MAX_PAIRS;
static_assert(MAX_PAIRS % 4 == 0, "a vector holds four pairs");

struct ShiftTable {
    float4 cs[MAX_PAIRS / 2];                          // (cos, sin) of pairs 2i, 2i + 1
};

// one (even, odd) pair, packed as it lies in memory: fp32 multiply-adds, one RNE rounding to bf16 each
__device__ __forceinline__ uint32_t rotate_pair(uint32_t w, float c, float s) {
    const float x0 = bf2f((uint16_t)(w & 0xffffu)), x1 = bf2f((uint16_t)(w >> 16));
    const float y0 = x0 * c - x1 * s;
    const float y1 = x0 * s + x1 * c;
    const uint32_t r = (uint32_t)f2bf(y0) | ((uint32_t)f2bf(y1) << 16);
    return (c == 1.0f && s == 0.0f) ? w : r;
}

// grid: (ceil(n_vec / 256), B).  n_vec = rows * vpr vectors per batch entry (rows are contiguous), vpr = dim / 8,
// vph = head_dim / 8, rot_vecs = the vectors of a head that hold a frame pair.
__global__ __launch_bounds__(256)
void rope_shift_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, int64_t src_stride, int64_t dst_stride,
                       int64_t n_vec, int vpr, int vph, int rot_vecs, const ShiftTable tab) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_vec) return;                            // the tail: nothing past [rows, dim] is read or written
    const int64_t b = blockIdx.y;
    // (src and dst may be the same rows: every lane reads its own 16 bytes before it writes them, and no other lane's)
    uint4 v = *(const uint4*)(src + b * src_stride + i * 8);
    const int hv = (int)(i % vpr) % vph;               // this vector's place in its head
    if (hv < rot_vecs) {
        const float4 t0 = tab.cs[2 * hv], t1 = tab.cs[2 * hv + 1];
        v.x = rotate_pair(v.x, t0.x, t0.y);
        v.y = rotate_pair(v.y, t0.z, t0.w);
        v.z = rotate_pair(v.z, t1.x, t1.y);
        v.w = rotate_pair(v.w, t1.z, t1.w);
    }
    *(uint4*)(dst + b * dst_stride + i * 8) = v;
}

}  // namespace

extern "C" int omh_rope_shift_frames(const void* src, void* dst, int32_t B, int64_t rows, int32_t dim, int64_t src_batch_stride,
                                     int64_t dst_batch_stride, int64_t delta_frames, int32_t head_dim, double theta,
                                     omh_stream_t stream) {
    if (!src || !dst || B < 1 || rows < 1 || dim < 1 || head_dim < 1 || !(theta > 0.0)) return OMH_E_BADARG;
    if (dim % 128 || head_dim % 8 || dim % head_dim) return OMH_E_SHAPE;
    const int64_t extent = rows * (int64_t)dim;        // elements of one batch entry
    if (src_batch_stride < extent || dst_batch_stride < extent) return OMH_E_BADARG;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) || (src_batch_stride | dst_batch_stride) % 8) return OMH_E_ALIGN;
    const int n_frame = head_dim - 4 * (head_dim / 6); // channels of the frame axis (rope_params' first table)
    const int nf = n_frame / 2;
    if (nf > MAX_PAIRS || B > 65535 || extent / 8 > (int64_t)0x7fffffff * 256) return OMH_E_SHAPE;
    // in place (the same rows at the same stride) or apart; anything between would read rows another lane has written
    const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
    const uintptr_t s1 = s0 + 2 * (uintptr_t)((B - 1) * src_batch_stride + extent);
    const uintptr_t d1 = d0 + 2 * (uintptr_t)((B - 1) * dst_batch_stride + extent);
    if (s0 == d0 ? src_batch_stride != dst_batch_stride : (s0 < d1 && d0 < s1)) return OMH_E_BADARG;

    ShiftTable tab;
    float* cs = (float*)tab.cs;
    for (int j = 0; j < MAX_PAIRS; ++j) {
        double c = 1.0, s = 0.0;
        if (j < nf) {
            const double a = (double)delta_frames * (1.0 / pow(theta, (double)(2 * j) / (double)n_frame));
            c = cos(a);
            s = sin(a);
        }
        cs[2 * j] = (float)c;
        cs[2 * j + 1] = (float)s;
    }
    const int vpr = dim / 8;
    const int64_t n_vec = rows * vpr;
    omh_clear_status();
    hipLaunchKernelGGL(rope_shift_kernel, dim3((unsigned)((n_vec + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)src, (uint16_t*)dst, src_batch_stride, dst_batch_stride, n_vec, vpr, head_dim / 8,
                       (nf + 3) / 4, tab);
    return omh_launch_status();
}
