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
//
// Teacher forcing under a pinned sink (WanModel.forward_teacher_forcing(pin_sink=True)) needs the sink keys under several
// deltas at once, and their gradients summed back: omh_rope_shift_fan writes one rotated image per delta in one launch
// (the tables of omh_rope_shift_table in device memory, the same rotate_pair), omh_rope_shift_fold adds the images of the
// gradient rows, each rotated back, to the base rows in fp32 and rounds once.
#include <math.h>

#include "omh_common.h"

namespace {

constexpr int MAX_PAIRS = OMH_ROPE_SHIFT_MAX_PAIRS;
static_assert(MAX_PAIRS % 4 == 0, "a vector holds four pairs");

struct ShiftTable {
    float4 cs[MAX_PAIRS / 2];                          // (cos, sin) of pairs 2i, 2i + 1
};

// one (even, odd) pair, packed as it lies in memory: fp32 multiply-adds, one RNE rounding to bf16 each.
// The fp32 arithmetic is spelled out — the x1 product rounded, the x0 product fused into the sum — so that it is the one
// tests/pinned_sink_ref.py::shift_emulated states, whatever contraction the compiler would choose for `x0 * c - x1 * s`
// (it chose a packed multiply and a subtraction for y0, and fused the other product for y1: an ulp of bf16 apart from the
// emulation on about one element in 10^5).
__device__ __forceinline__ uint32_t rotate_pair(uint32_t w, float c, float s) {
    const float x0 = bf2f((uint16_t)(w & 0xffffu)), x1 = bf2f((uint16_t)(w >> 16));
    const float y0 = __builtin_fmaf(x0, c, -(x1 * s));
    const float y1 = __builtin_fmaf(x0, s, x1 * c);
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

// The fan-out of teacher forcing under a pinned sink (include/omh.h, omh_rope_shift_fan): `copies` rotated images of the
// same rows in ONE launch, copy c under the table row c.  The tables lie in device memory (one delta fits the kernel
// arguments, sixty do not); the arithmetic per vector is rotate_pair's, so copy c has the bits of
// omh_rope_shift_frames(src, ., delta_c).
// grid: (ceil(n_vec / 256), copies, B).
__global__ __launch_bounds__(256)
void rope_shift_fan_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, int64_t src_stride, int64_t dst_stride,
                           int64_t copy_stride, int64_t n_vec, int vpr, int vph, int rot_vecs,
                           const float4* __restrict__ tabs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_vec) return;                            // the tail: nothing past [rows, dim] is read or written
    const int64_t c = blockIdx.y, b = blockIdx.z;
    uint4 v = *(const uint4*)(src + b * src_stride + i * 8);
    const int hv = (int)(i % vpr) % vph;
    if (hv < rot_vecs) {
        const float4* tab = tabs + c * (MAX_PAIRS / 2);
        const float4 t0 = tab[2 * hv], t1 = tab[2 * hv + 1];
        v.x = rotate_pair(v.x, t0.x, t0.y);
        v.y = rotate_pair(v.y, t0.z, t0.w);
        v.z = rotate_pair(v.z, t1.x, t1.y);
        v.w = rotate_pair(v.w, t1.z, t1.w);
    }
    *(uint4*)(dst + b * dst_stride + c * copy_stride + i * 8) = v;
}

// acc += R(-delta) (x0, x1): the pair rotated BACK, in fp32, not rounded
__device__ __forceinline__ void fold_pair(float& a0, float& a1, uint32_t w, float c, float s) {
    const float x0 = bf2f((uint16_t)(w & 0xffffu)), x1 = bf2f((uint16_t)(w >> 16));
    a0 += x0 * c + x1 * s;
    a1 += x1 * c - x0 * s;
}

__device__ __forceinline__ uint32_t pack_pair(float a0, float a1) { return (uint32_t)f2bf(a0) | ((uint32_t)f2bf(a1) << 16); }

// The fold behind the attention backward (omh_rope_shift_fold): dst = bf16(base + sum_c R(-delta_c) image_c), the sum in
// fp32 in ascending c, one rounding at the end; every lane owns its 16 bytes of dst, so nothing is atomic and two runs
// give the same bits.  tabs == nullptr: the plain sum (rot_vecs = 0).
// grid: (ceil(n_vec / 256), B);  n_vec = rows * vpr, every operand with its own row pitch.
__global__ __launch_bounds__(256)
void rope_shift_fold_kernel(const uint16_t* __restrict__ base, const uint16_t* __restrict__ img, uint16_t* dst, int64_t base_ld,
                            int64_t base_stride, int64_t img_ld, int64_t img_stride, int64_t copy_stride, int64_t dst_ld,
                            int64_t dst_stride, int copies, int64_t n_vec, int vpr, int vph, int rot_vecs,
                            const float4* __restrict__ tabs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_vec) return;
    const int64_t b = blockIdx.y, r = i / vpr;
    const int cv = (int)(i % vpr), hv = cv % vph;
    // (dst may be base: this lane reads its 16 bytes of base before it writes them, and no other lane's)
    const uint4 v0 = *(const uint4*)(base + b * base_stride + r * base_ld + cv * 8);
    float a[8];
    a[0] = bf2f((uint16_t)(v0.x & 0xffffu)), a[1] = bf2f((uint16_t)(v0.x >> 16));
    a[2] = bf2f((uint16_t)(v0.y & 0xffffu)), a[3] = bf2f((uint16_t)(v0.y >> 16));
    a[4] = bf2f((uint16_t)(v0.z & 0xffffu)), a[5] = bf2f((uint16_t)(v0.z >> 16));
    a[6] = bf2f((uint16_t)(v0.w & 0xffffu)), a[7] = bf2f((uint16_t)(v0.w >> 16));
    const uint16_t* p = img + b * img_stride + r * img_ld + cv * 8;
    const bool rot = hv < rot_vecs;
    for (int c = 0; c < copies; ++c, p += copy_stride) {
        const uint4 v = *(const uint4*)p;
        if (rot) {
            const float4* tab = tabs + (int64_t)c * (MAX_PAIRS / 2);
            const float4 t0 = tab[2 * hv], t1 = tab[2 * hv + 1];
            fold_pair(a[0], a[1], v.x, t0.x, t0.y);
            fold_pair(a[2], a[3], v.y, t0.z, t0.w);
            fold_pair(a[4], a[5], v.z, t1.x, t1.y);
            fold_pair(a[6], a[7], v.w, t1.z, t1.w);
        } else {                                       // the h / w columns, and every column of a plain sum
            a[0] += bf2f((uint16_t)(v.x & 0xffffu)), a[1] += bf2f((uint16_t)(v.x >> 16));
            a[2] += bf2f((uint16_t)(v.y & 0xffffu)), a[3] += bf2f((uint16_t)(v.y >> 16));
            a[4] += bf2f((uint16_t)(v.z & 0xffffu)), a[5] += bf2f((uint16_t)(v.z >> 16));
            a[6] += bf2f((uint16_t)(v.w & 0xffffu)), a[7] += bf2f((uint16_t)(v.w >> 16));
        }
    }
    uint4 o;
    o.x = pack_pair(a[0], a[1]), o.y = pack_pair(a[2], a[3]), o.z = pack_pair(a[4], a[5]), o.w = pack_pair(a[6], a[7]);
    *(uint4*)(dst + b * dst_stride + r * dst_ld + cv * 8) = o;
}

// the (cos, sin) of the frame pairs of one delta: fp64 angle, fp64 cos / sin, one rounding to fp32; identity past the frame part
void shift_table(int64_t delta_frames, int n_frame, double theta, float* cs) {
    const int nf = n_frame / 2;
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
}

// byte ranges [a0 + b a_bs, + a_len) and [b0 + b' b_bs, + b_len), b, b' < B (lengths and strides in bytes): do any two meet?
// Apart as wholes, or — the row ranges of ONE buffer, the same batch stride — apart inside every period of it.
bool ranges_meet(uintptr_t a0, uint64_t a_len, uint64_t a_bs, uintptr_t b0, uint64_t b_len, uint64_t b_bs, int B) {
    const uintptr_t a1 = a0 + (uint64_t)(B - 1) * a_bs + a_len, b1 = b0 + (uint64_t)(B - 1) * b_bs + b_len;
    if (a1 <= b0 || b1 <= a0) return false;
    if (B == 1 || a_bs != b_bs || a_len > a_bs || b_len > a_bs) return true;
    const uint64_t off = b0 >= a0 ? (b0 - a0) % a_bs : (a_bs - (a0 - b0) % a_bs) % a_bs;
    return !(off >= a_len && off + b_len <= a_bs);
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
    shift_table(delta_frames, n_frame, theta, (float*)tab.cs);
    const int vpr = dim / 8;
    const int64_t n_vec = rows * vpr;
    omh_clear_status();
    hipLaunchKernelGGL(rope_shift_kernel, dim3((unsigned)((n_vec + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)src, (uint16_t*)dst, src_batch_stride, dst_batch_stride, n_vec, vpr, head_dim / 8,
                       (nf + 3) / 4, tab);
    return omh_launch_status();
}

extern "C" int omh_rope_shift_table(int64_t delta_frames, int32_t head_dim, double theta, float* cs) {
    if (!cs || head_dim < 1 || !(theta > 0.0)) return OMH_E_BADARG;
    if (head_dim % 8) return OMH_E_SHAPE;
    const int n_frame = head_dim - 4 * (head_dim / 6);
    if (n_frame / 2 > MAX_PAIRS) return OMH_E_SHAPE;
    shift_table(delta_frames, n_frame, theta, cs);
    return 0;
}

extern "C" int omh_rope_shift_fan(const void* src, void* dst, int32_t B, int64_t rows, int32_t dim, int32_t copies,
                                  int64_t src_batch_stride, int64_t dst_batch_stride, int64_t dst_copy_stride,
                                  const float* tables, int32_t head_dim, omh_stream_t stream) {
    if (!src || !dst || !tables || B < 1 || rows < 1 || dim < 1 || head_dim < 1 || copies < 1) return OMH_E_BADARG;
    if (dim % 128 || head_dim % 8 || dim % head_dim) return OMH_E_SHAPE;
    const int64_t extent = rows * (int64_t)dim;        // elements of one image
    if (dst_copy_stride < extent) return OMH_E_BADARG;
    const int64_t hull = (copies - 1) * dst_copy_stride + extent;       // elements of one batch entry's images
    if (src_batch_stride < extent || dst_batch_stride < hull) return OMH_E_BADARG;
    if ((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)tables) & 15) || (src_batch_stride | dst_batch_stride | dst_copy_stride) % 8)
        return OMH_E_ALIGN;
    const int nf = (head_dim - 4 * (head_dim / 6)) / 2;
    if (nf > MAX_PAIRS || B > 65535 || copies > 65535 || extent / 8 > (int64_t)0x7fffffff * 256) return OMH_E_SHAPE;
    if (ranges_meet((uintptr_t)src, 2 * (uint64_t)extent, 2 * (uint64_t)src_batch_stride, (uintptr_t)dst, 2 * (uint64_t)hull,
                    2 * (uint64_t)dst_batch_stride, B))
        return OMH_E_BADARG;
    const int vpr = dim / 8;
    const int64_t n_vec = rows * vpr;
    omh_clear_status();
    hipLaunchKernelGGL(rope_shift_fan_kernel, dim3((unsigned)((n_vec + 255) / 256), (unsigned)copies, (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, (const uint16_t*)src, (uint16_t*)dst, src_batch_stride, dst_batch_stride,
                       dst_copy_stride, n_vec, vpr, head_dim / 8, (nf + 3) / 4, (const float4*)tables);
    return omh_launch_status();
}

extern "C" int omh_rope_shift_fold(const void* base, const void* images, void* dst, int32_t B, int64_t rows, int32_t dim,
                                   int32_t copies, int64_t base_ld, int64_t base_batch_stride, int64_t img_ld,
                                   int64_t img_batch_stride, int64_t img_copy_stride, int64_t dst_ld, int64_t dst_batch_stride,
                                   const float* tables, int32_t head_dim, omh_stream_t stream) {
    if (!base || !images || !dst || B < 1 || rows < 1 || dim < 1 || head_dim < 1 || copies < 1) return OMH_E_BADARG;
    if (dim % 128 || head_dim % 8 || dim % head_dim) return OMH_E_SHAPE;
    if (base_ld < dim || img_ld < dim || dst_ld < dim) return OMH_E_BADARG;
    const int64_t base_ext = (rows - 1) * base_ld + dim, img_ext = (rows - 1) * img_ld + dim, dst_ext = (rows - 1) * dst_ld + dim;
    if (img_copy_stride < img_ext) return OMH_E_BADARG;
    const int64_t img_hull = (copies - 1) * img_copy_stride + img_ext;
    if (base_batch_stride < base_ext || img_batch_stride < img_hull || dst_batch_stride < dst_ext) return OMH_E_BADARG;
    if ((((uintptr_t)base | (uintptr_t)images | (uintptr_t)dst | (uintptr_t)tables) & 15) ||
        (base_ld | base_batch_stride | img_ld | img_batch_stride | img_copy_stride | dst_ld | dst_batch_stride) % 8)
        return OMH_E_ALIGN;
    const int nf = (head_dim - 4 * (head_dim / 6)) / 2;
    if (nf > MAX_PAIRS || B > 65535 || rows * (int64_t)(dim / 8) > (int64_t)0x7fffffff * 256) return OMH_E_SHAPE;
    // dst: the base rows themselves (same pointer and pitches) or apart from them; always apart from the images
    const bool in_place = base == dst && base_ld == dst_ld && base_batch_stride == dst_batch_stride;
    if (!in_place && ranges_meet((uintptr_t)base, 2 * (uint64_t)base_ext, 2 * (uint64_t)base_batch_stride, (uintptr_t)dst,
                                 2 * (uint64_t)dst_ext, 2 * (uint64_t)dst_batch_stride, B))
        return OMH_E_BADARG;
    if (ranges_meet((uintptr_t)images, 2 * (uint64_t)img_hull, 2 * (uint64_t)img_batch_stride, (uintptr_t)dst,
                    2 * (uint64_t)dst_ext, 2 * (uint64_t)dst_batch_stride, B))
        return OMH_E_BADARG;
    const int vpr = dim / 8;
    const int64_t n_vec = rows * vpr;
    omh_clear_status();
    hipLaunchKernelGGL(rope_shift_fold_kernel, dim3((unsigned)((n_vec + 255) / 256), (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, (const uint16_t*)base, (const uint16_t*)images, (uint16_t*)dst, base_ld,
                       base_batch_stride, img_ld, img_batch_stride, img_copy_stride, dst_ld, dst_batch_stride, (int)copies, n_vec,
                       vpr, head_dim / 8, tables ? (nf + 3) / 4 : 0, (const float4*)tables);
    return omh_launch_status();
}
