// Shared device helpers for the gfx950 kernels of libomh.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/omh.h"

// ---------------------------------------------------------------------------------------------------------------------
// Process options (ABI v10, include/omh.h: omh_set_option / omh_get_option).  Every dispatch switch of the library —
// kernel-family overrides for tests and A/B timing — lives in ONE table.  The environment is consulted exactly once per
// process (the first omh_opt() / omh_set_option() call: variable OMH_<NAME> seeds option <NAME>); after that the launch
// path never calls getenv and a switch changes only through omh_set_option().  omh_opt() returns NULL for an unset option.
#define OMH_OPTIONS(X)                                                                                                   \
    X(ATTN_KERNEL) X(ATTN_SPLIT) X(W64_SPLIT) X(CONV_PERSIST) X(CONV_W64_UP2) X(LN_RPW) X(GEMM_GROUP_M)                  \
    X(GEMM_TILE) X(GEMM_RULE) X(GEMM_KERNEL) X(GEMM_W64_GBWD) X(GEMM_W64_GAUX) X(GEMM_W64_R192) X(GEMM_W64_BF16M)        \
    X(GEMM_W64_N192) X(GEMM_TN_SPLIT) X(GEMM_TN_W64) X(GEMM_TN_TILE) X(GEMM_TN_GROUP_TILE) X(GEMM_SPLITK) X(CONV_TILE)   \
    X(CONV_WIDE_MIN) X(CONV_W64) X(CONV_FUSE_NORM) X(CONV_KW3) X(GEMM_QKV) X(ATTN_BWD_W64) X(RMS_PAIR_ROW)                  \
    X(ATTN_BOUNDED) X(W64_SCHED) X(RMS_PAIR_BOUND)
enum OmhOpt {
#define X(n) OMH_OPT_##n,
    OMH_OPTIONS(X)
#undef X
    OMH_OPT_COUNT
};
const char* omh_opt(int id);

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

#define OMH_WAVE 64

// round-to-nearest-even fp32 -> bf16 bit pattern (NaN kept quiet)
__device__ __forceinline__ uint16_t f2bf(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__device__ __forceinline__ float bf2f(uint16_t h) { return __uint_as_float(((uint32_t)h) << 16); }

// two fp32 -> packed bf16x2 with the gfx950 hardware convert v_cvt_pk_bf16_f32 (RNE, NaN-safe), through the vector
// conversion the compiler selects it for.  Rounds 1-4 had a one-line asm here; inline asm is opaque to the compiler's
// hazard recognizer, and on gfx950 a VALU instruction that reads the result of a transcendental one (v_exp_f32,
// v_rcp_f32, ...) in the very next issue slot gets the OLD register contents ("trans forwarding" hazard, 1 wait
// state).  Round 5's attention backward put exp2 -> pack back to back and produced garbage in dV; the conversion below
// lets the compiler insert the s_nop where needed (and schedule the convert like any other VALU instruction).
typedef float omh_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 omh_bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_bf2(float lo, float hi) {
    const omh_f32x2 v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, omh_bf16x2));
}
// raw v_exp_f32 (2^x): no denormal fix-up sequence; inputs here are <= 0 and
// results below 2^-126 may flush to zero, which is what a softmax wants.
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// 0.5 x (1 + tanh( sqrt(2/pi) (x + 0.044715 x^3) ))  ==  x * sigmoid(2u) = x / (1 + 2^(-2u log2 e)).
// Raw v_exp_f32 / v_rcp_f32 (1 ulp-class) instead of the IEEE division sequence: ~9 VALU per element,
// this runs 128 times per lane in a GEMM epilogue.
__device__ __forceinline__ float gelu_tanh(float x) {
    const float x2 = x * x;
    const float k = -2.0f * 0.7978845608028654f * 1.4426950408889634f;          // -2 c log2(e)
    const float t = k * x * fmaf(0.044715f, x2, 1.0f);
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(t));
}
// d/dx gelu_tanh(x) = 0.5 (1 + t) + 0.5 x (1 - t^2) c (1 + 3 a x^2),  t = tanh(c (x + a x^3))
// With s = sigmoid(2u) = 1 / (1 + 2^(-2u log2 e)):  0.5 (1 + t) = s  and  0.5 (1 - t^2) = 2 s (1 - s), so
//   gelu' = s + x * 2 s (1 - s) * c (1 + 3 a x^2)      (raw v_exp_f32 / v_rcp_f32: ~12 VALU, no IEEE division —
// this runs 128 times per lane in the epilogue of the FFN dgrad GEMM)
__device__ __forceinline__ float gelu_tanh_grad(float x) {
    const float c = 0.7978845608028654f, a = 0.044715f;
    const float x2 = x * x;
    const float k = -2.0f * c * 1.4426950408889634f;                  // -2 c log2(e)
    const float s = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(k * x * fmaf(a, x2, 1.0f)));
    return fmaf(x * (2.0f * c) * fmaf(3.0f * a, x2, 1.0f), s * (1.0f - s), s);
}
__device__ __forceinline__ float silu(float x) {
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// XCD-aware bijective remap of a 1-D block id: consecutive *work* ids land on
// the same XCD (block b runs on XCD b % 8 — observed, speed only).
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int nx = 8;
    const int q = nwg / nx, r = nwg % nx;
    const int xcd = bid % nx, idx = bid / nx;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

// Work id -> output tile.  Consecutive ids (which xcd_remap keeps on one XCD, ~64 resident at a
// time) walk 8 m-tiles x all n-tiles in m-fastest order, so the resident set is an 8 x 8 patch of
// tiles: 8 A panels + 8 B panels live in that XCD's 4 MiB L2 instead of 1 + 64.
__device__ __forceinline__ void tile_of(int wid, int tiles_m, int tiles_n, int& tm, int& tn, const int GM = 8) {
    const int per_group = GM * tiles_n;
    const int gid = wid / per_group, in_g = wid - gid * per_group;
    const int first_m = gid * GM;
    const int gsz = min(tiles_m - first_m, GM);
    tm = first_m + in_g % gsz;
    tn = in_g / gsz;
}

// Zero fill of rows x cols fp32 (row pitch ld) as a KERNEL.  Not hipMemsetAsync: under hipGraph stream capture a
// memset node recorded through this library was replayed out of stream order on ROCm 7 (round-2 finding: the
// input-gradient scratch of omh_dense_f32_bwd lives in recycled graph-pool memory, the memset ran early, a later
// kernel of the graph reused the block, and the atomics then added onto that kernel's data — every replay after
// the first returned wrong time-embedding gradients).  A kernel node keeps its place.
__global__ __launch_bounds__(256) static void omh_zero_f32_kernel(float* __restrict__ p, int64_t rows, int64_t cols,
                                                                  int64_t ld) {
    const int64_t n = rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        p[(i / cols) * ld + (i % cols)] = 0.f;
}
static inline void omh_zero_f32(float* p, int64_t rows, int64_t cols, int64_t ld, hipStream_t s) {
    const int64_t n = rows * cols;
    int64_t g = (n + 255) / 256;
    g = g < 1 ? 1 : (g > 4096 ? 4096 : g);
    hipLaunchKernelGGL(omh_zero_f32_kernel, dim3((unsigned)g), dim3(256), 0, s, p, rows, cols, ld);
}

// omh_set_deterministic()'s state (dit_elementwise.hip): launchers that combine partial sums with atomics ask it
bool omh_deterministic();

// hipGetLastError() reports the last error of ANY earlier runtime call on this
// thread (e.g. a probe made by the host framework): clear it before a launch
// so the status returned after the launch belongs to that launch only.
static inline void omh_clear_status() { (void)hipGetLastError(); }
static inline int omh_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}


// ---- block masks (include/omh.h omh_block_mask; attention.hip, attention_bwd2.hip) ----
// What a BLK kernel gets: one list per (mask head, 128-row block of the workgroup's side) — `cnt` entries of `idx`,
// ascending indices of the 128-position blocks of the other side (row lists: forward and dQ; column lists: dK / dV).
// The IVL kernels (interval masks, below) receive their table in this same argument, since no kernel has both a block
// mask and an interval mask: idx = the table, heads = group, lists = its rows, stride = groups of the other axis, cnt
// unused — but for the rectangular form (omh_interval_rect_mask: one group size per axis), whose kernels read the OTHER
// axis' group size from cnt's eight bytes as an integer.  omh_ivl_arg / omh_ivl_tab are the only two places that know the
// mapping; a change of this struct's fields must keep them (and the asserts behind IvlTab) in step.
struct BlkList {
    const int32_t* cnt;   // [heads][lists]
    const int32_t* idx;   // [heads][lists][stride]
    int heads, lists, stride;
};
static inline int omh_block_mask_check(const omh_block_mask* m, int H, int Lq, int Lk) {
    if (!m->row_cnt || !m->row_idx || !m->col_cnt || !m->col_idx) return OMH_E_BADARG;
    if (m->heads != 1 && m->heads != H) return OMH_E_BADARG;
    if (m->q_blocks != (Lq + 127) / 128 || m->k_blocks != (Lk + 127) / 128) return OMH_E_BADARG;
    if (((uintptr_t)m->row_cnt | (uintptr_t)m->row_idx | (uintptr_t)m->col_cnt | (uintptr_t)m->col_idx) & 3) return OMH_E_ALIGN;
    return 0;
}
// A mask excludes a band.  (0, 0) is what a zero-initialised omh_attn_args holds, so the sparse entries read it as "no
// band set", not as the one-key band it is elsewhere; both sides < 0 is the unbounded band; anything else is refused.
static inline bool omh_mask_window_unset(int wl, int wr) { return (wl < 0 && wr < 0) || (wl == 0 && wr == 0); }

// ---- the chunk-causal staircase (include/omh.h omh_chunk_causal; attention.hip, attention_bwd2.hip) ----
// What a CHK kernel gets: query i sits at position off + i; it sees key j iff  j / chunk <= (off + i) / chunk  and
// (left < 0 or j / chunk >= (off + i) / chunk - left).  Normalised by omh_chunk_rule so that every product of a chunk
// index with `chunk` the kernels form stays below 2^31.
struct ChunkRule {
    int chunk, left, off;
};
// 0 or the error code.  A chunk at least as long as both axes is clamped to that length (every position is then in chunk
// 0 either way) and a look-back past the first chunk to one that reaches it: the same mask, small numbers.
static inline int omh_chunk_rule(const omh_chunk_causal* c, int Lq, int Lk, ChunkRule* out) {
    if (!c || c->chunk <= 0 || c->q_offset < 0 || c->reserved != 0) return OMH_E_BADARG;
    const int64_t span = (int64_t)c->q_offset + Lq;                  // positions of the query axis end here
    if (span + Lk >= (1LL << 28)) return OMH_E_SHAPE;
    const int64_t cap = span > Lk ? span : Lk;
    out->chunk = c->chunk > cap ? (int)cap : c->chunk;
    const int64_t reach = span / out->chunk + 1;                     // chunks a look-back can span at most
    out->left = c->left_chunks < 0 ? -1 : (c->left_chunks > reach ? (int)reach : c->left_chunks);
    out->off = c->q_offset;
    return 0;
}

// ---- interval masks (include/omh.h omh_interval_mask / omh_interval3_mask; attention.hip, attention_bwd2.hip) ----
// What an IVL kernel gets: ONE of the two tables — row g of `iv` holds the (at most RUNS) intervals [lo0, hi0) U [lo1, hi1)
// ... of groups of the OTHER axis that group g of the workgroup's axis sees (q_iv: forward and dQ; k_iv: dK / dV), in
// groups of `group` positions; `n` rows, `other` groups on the other axis.  RUNS (2: omh_interval_mask, 3:
// omh_interval3_mask) is a template argument of the kernels and of every helper below: one implementation, two
// instantiations (a two-run mask through the three-run kernels costs 7 % forward, 15 % backward: DESIGN.md 4.2g).
// `group` cuts the workgroup's own axis (which row of the table a position reads), `ogroup` the other axis (what a table
// value is worth in positions).  The square masks have one size for both and their kernels one value: RECT (a template
// argument, like RUNS) tells the instantiations of omh_interval_rect_mask, which hold the two apart.
struct IvlTab {
    const int32_t* iv;    // [n][2 RUNS]
    int group, n, other, ogroup;
};
// The IVL kernels take their table in the BlkList argument (no kernel has both): a further kernel argument would change
// the kernarg segment, and with it the scalar loads of the instantiations that must keep their instruction streams.
// (ogroup: the rectangular form only — an integer in the place of the cnt pointer, never dereferenced)
static inline BlkList omh_ivl_arg(const int32_t* iv, int group, int n, int other, int ogroup = 0) {
    return BlkList{(const int32_t*)(uintptr_t)(uint32_t)ogroup, iv, group, n, other};
}
static_assert(sizeof(BlkList) == 2 * sizeof(void*) + 4 * sizeof(int) && sizeof(IvlTab) + sizeof(void*) == sizeof(BlkList),
              "IvlTab travels in a BlkList: one pointer and three ints, and the other axis' group in the place of cnt");
static_assert(std::is_same<decltype(BlkList::idx), decltype(IvlTab::iv)>::value && std::is_same<decltype(BlkList::heads), int>::value &&
              std::is_same<decltype(BlkList::lists), int>::value && std::is_same<decltype(BlkList::stride), int>::value,
              "omh_ivl_arg / omh_ivl_tab map idx, heads, lists, stride to iv, group, n, other");
// 0 or the error code, for either public struct (the same fields; the tables themselves live on the device: the kernels
// clamp what they read to [0, other] and know the row stride from their instantiation)
template <typename Mask>
static inline int omh_interval_mask_check(const Mask* m, int Lq, int Lk) {
    if (!m || !m->q_iv || !m->k_iv || m->group < 8 || m->reserved != 0) return OMH_E_BADARG;
    if ((int64_t)Lq + Lk >= (1LL << 28)) return OMH_E_SHAPE;
    if (m->q_groups != (Lq + m->group - 1) / m->group || m->k_groups != (Lk + m->group - 1) / m->group) return OMH_E_BADARG;
    if (((uintptr_t)m->q_iv | (uintptr_t)m->k_iv) & 3) return OMH_E_ALIGN;
    return 0;
}
// the same for omh_interval_rect_mask (one group size per axis, no reserved field), in the same order with the same codes
static inline int omh_interval_rect_mask_check(const omh_interval_rect_mask* m, int Lq, int Lk) {
    if (!m || !m->q_iv || !m->k_iv || m->q_group < 8 || m->k_group < 1) return OMH_E_BADARG;
    if ((int64_t)Lq + Lk >= (1LL << 28)) return OMH_E_SHAPE;
    if (m->q_groups != (Lq + m->q_group - 1) / m->q_group || m->k_groups != (Lk + m->k_group - 1) / m->k_group) return OMH_E_BADARG;
    if (((uintptr_t)m->q_iv | (uintptr_t)m->k_iv) & 3) return OMH_E_ALIGN;
    return 0;
}
#if defined(__HIPCC__)
template <bool RECT = false>
__device__ __forceinline__ IvlTab omh_ivl_tab(const BlkList& bl) {
    return IvlTab{bl.idx, bl.heads, bl.lists, bl.stride, RECT ? (int)(uint32_t)(uintptr_t)bl.cnt : bl.heads};
}
// One position's (or one workgroup's) view of the other axis: RUNS intervals of positions [lo, lo + len), len <= 0: empty.
// (Every loop over the runs is fully unrolled and indexes with constants: the arrays are registers, never scratch.)
template <int RUNS>
struct IvlSpan {
    int lo[RUNS], len[RUNS];
    // (bitwise: a compare per run and an OR between them, no short-circuit branches per element — what the compiler makes of
    // || over three runs in the forward)
    __device__ __forceinline__ bool sees(int x) const {
        bool in = (unsigned)(x - lo[0]) < (unsigned)len[0];
#pragma unroll
        for (int i = 1; i < RUNS; ++i) in = in | ((unsigned)(x - lo[i]) < (unsigned)len[i]);
        return in;
    }
};
// row g of the [n][2 RUNS] table in positions, cut at `end` (the live length of the other axis)
template <int RUNS>
__device__ __forceinline__ IvlSpan<RUNS> omh_ivl_row(const IvlTab& tb, int g, int end) {
    const int32_t* __restrict__ r = tb.iv + 2 * RUNS * (int64_t)min(max(g, 0), tb.n - 1);
    int a[RUNS], b[RUNS];                                            // [a, b) in groups, clamped
#pragma unroll
    for (int i = 0; i < RUNS; ++i) { a[i] = min(max(r[2 * i], 0), tb.other); b[i] = min(max(r[2 * i + 1], 0), tb.other); }
    IvlSpan<RUNS> s;
#pragma unroll
    for (int i = 0; i < RUNS; ++i) { s.lo[i] = a[i] * tb.ogroup; s.len[i] = max(min(b[i] * tb.ogroup, end) - s.lo[i], 0); }
    return s;
}
// The tiles of `tile` positions a workgroup runs: up to RUNS ranges of consecutive tiles.  tile(x), x in [0, n_tiles), is
// the x-th of them: n[j] counts the tiles of the first j + 1 ranges and gap[j] the tiles skipped behind them (a jump that
// does not exist has n[j] = n_tiles, gap[j] = 0).  The one place that knows the jump formula.
template <int RUNS>
struct IvlTiles {
    int t_first, n_tiles, n[RUNS - 1], gap[RUNS - 1];
    __device__ __forceinline__ int tile(int x) const {
        int t = t_first + x;
#pragma unroll
        for (int j = 0; j < RUNS - 1; ++j) t += x >= n[j] ? gap[j] : 0;
        return t;
    }
};
// The plan of a workgroup whose live positions are x0 .. x1 (x1 >= x0): the hulls of its groups' first, second, ...
// intervals (their lower ends ascend: every row's do), empty ones dropped, neighbours that touch or overlap in tile units
// merged.  whole (may be NULL; 2 RUNS ints): [lo, hi] of the positions EVERY one of those groups sees through its i-th
// interval (hi < lo: none).  Scalar reads, once per workgroup.
// WIDE (the rectangular dK / dV kernel, whose 128 keys span up to 128 rows of one-token groups): the rows are read across
// the lanes of the wave instead, row g0 + lane, + 64, ..., and the hulls and intersections reduced with six butterfly
// steps — min and max of the same integers, so the plan is the one the scalar walk gives.
template <int RUNS, bool WIDE = false>
__device__ __forceinline__ IvlTiles<RUNS> omh_ivl_tiles(const IvlTab& tb, int x0, int x1, int end, int tile, int* whole) {
    const int g0 = x0 / tb.group, g1 = x1 / tb.group;
    int hlo[RUNS], hhi[RUNS], wlo[RUNS], whi[RUNS];                  // hulls and intersections, [lo, hi)
#pragma unroll
    for (int i = 0; i < RUNS; ++i) hlo[i] = 1 << 30;
#pragma unroll
    for (int i = 0; i < RUNS; ++i) hhi[i] = 0;
#pragma unroll
    for (int i = 0; i < RUNS; ++i) wlo[i] = 0;
#pragma unroll
    for (int i = 0; i < RUNS; ++i) whi[i] = 1 << 30;
    if constexpr (WIDE) {
        for (int g = g0 + (int)(threadIdx.x & 63); g <= g1; g += 64) {
            const IvlSpan<RUNS> s = omh_ivl_row<RUNS>(tb, g, end);
#pragma unroll
            for (int i = 0; i < RUNS; ++i) {
                if (s.len[i] > 0) { hlo[i] = min(hlo[i], s.lo[i]); hhi[i] = max(hhi[i], s.lo[i] + s.len[i]); }
                wlo[i] = max(wlo[i], s.lo[i]); whi[i] = min(whi[i], s.lo[i] + s.len[i]);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int i = 0; i < RUNS; ++i) {
                hlo[i] = min(hlo[i], __shfl_xor(hlo[i], o, 64)); hhi[i] = max(hhi[i], __shfl_xor(hhi[i], o, 64));
                wlo[i] = max(wlo[i], __shfl_xor(wlo[i], o, 64)); whi[i] = min(whi[i], __shfl_xor(whi[i], o, 64));
            }
        }
#pragma unroll
        for (int i = 0; i < RUNS; ++i) {
            hlo[i] = __builtin_amdgcn_readfirstlane(hlo[i]); hhi[i] = __builtin_amdgcn_readfirstlane(hhi[i]);
            wlo[i] = __builtin_amdgcn_readfirstlane(wlo[i]); whi[i] = __builtin_amdgcn_readfirstlane(whi[i]);
        }
    } else {
    for (int g = g0; g <= g1; ++g) {
        const IvlSpan<RUNS> s = omh_ivl_row<RUNS>(tb, __builtin_amdgcn_readfirstlane(g), end);
#pragma unroll
        for (int i = 0; i < RUNS; ++i) {
            if (s.len[i] > 0) { hlo[i] = min(hlo[i], s.lo[i]); hhi[i] = max(hhi[i], s.lo[i] + s.len[i]); }
            wlo[i] = max(wlo[i], s.lo[i]); whi[i] = min(whi[i], s.lo[i] + s.len[i]);
        }
    }
    }
    if (whole) {
#pragma unroll
        for (int i = 0; i < RUNS; ++i) { whole[2 * i] = wlo[i]; whole[2 * i + 1] = whi[i] - 1; }
    }
    int rs[RUNS], re[RUNS], nr = 0;                                  // merged tile ranges [rs, re), ascending
#pragma unroll
    for (int i = 0; i < RUNS; ++i) { rs[i] = 0; re[i] = 0; }
#pragma unroll
    for (int i = 0; i < RUNS; ++i) {
        if (hhi[i] <= hlo[i]) continue;
        const int a = hlo[i] / tile, b = (hhi[i] - 1) / tile + 1;
#pragma unroll
        for (int j = 0; j < RUNS; ++j)                               // nr == j: range j - 1 grows, or range j opens
            if (j == RUNS - 1 || nr == j) {
                if (j > 0 && a <= re[j - 1]) re[j - 1] = max(re[j - 1], b); else { rs[j] = a; re[j] = b; nr = j + 1; }
                break;
            }
    }
    IvlTiles<RUNS> t = {};
    if (nr == 0) return t;
    t.t_first = rs[0];
    t.n_tiles = re[0] - rs[0];
#pragma unroll
    for (int j = 0; j < RUNS - 1; ++j) t.n[j] = t.n_tiles;
#pragma unroll
    for (int j = 1; j < RUNS; ++j)
        if (nr > j) {
            t.gap[j - 1] = rs[j] - re[j - 1];
            t.n_tiles = t.n[j - 1] + (re[j] - rs[j]);
#pragma unroll
            for (int jj = j; jj < RUNS - 1; ++jj) t.n[jj] = t.n_tiles;
        }
    return t;
}
#endif

// ---- which mask a kernel instantiation carries: the template arguments of the masked launchers, by name ----
// (attention.hip: flash_attn_fwd_d128_kernel<WIN, BLK, CHK, RUNS>; attention_bwd2.hip: the dQ and dK / dV kernels'
// <.., WIN, VLEN, BLK, CHK, RUNS, RECT>.  VLEN — q_lens — exists in the backward only: the forward's band kernel reads q_lens
// itself.  RECT: the interval mask has one group size per axis.)
template <bool WIN_, bool VLEN_, bool BLK_, bool CHK_, int RUNS_, bool RECT_ = false>
struct MaskKind {
    static constexpr bool WIN = WIN_, VLEN = VLEN_, BLK = BLK_, CHK = CHK_, RECT = RECT_;
    static constexpr int RUNS = RUNS_;
};
template <bool VLEN> using MaskBand = MaskKind<true, VLEN, false, false, 0>;     // the band, with or without q_lens
using MaskBlocks = MaskKind<false, false, true, false, 0>;                       // omh_block_mask
using MaskStairs = MaskKind<true, true, false, true, 0>;                         // omh_chunk_causal
template <int RUNS> using MaskIntervals = MaskKind<true, true, false, false, RUNS>;   // omh_interval_mask (2), omh_interval3_mask (3)
using MaskIntervalsRect = MaskKind<true, true, false, false, 2, true>;           // omh_interval_rect_mask

// ---- split of a launch's last, partly filled round of workgroups (host side; attention.hip, attention_bwd2.hip) ----
// A launch of `nwg` equal workgroups on `slots` resident slots takes ceil(nwg / slots) rounds; its last round holds
// r = nwg mod slots workgroups.  Those r are split into `splits` workers each over their inner loop (`loop_tiles` tiles,
// at least `min_tiles` per worker), dispatched as the LAST blocks of the same launch: they start when the last full
// round drains, and that round then costs ceil(r splits / slots) / splits of a full one — the smallest `splits` <= 8
// that minimises this is taken, if it saves at least a third of the round (the workers write partial results into a
// workspace that a small kernel combines in a fixed order: that is not free).  Examples (MI355X, 256 CUs): 624
// workgroups on 512 slots: r = 112, 4 workers each, 1.25 rounds instead of 2; 156 on 512 (one clip): 3 workers each,
// 1/3 of a round; 156 on 256: 3 workers, 2/3.
// `single_round_only`: split only launches that do not fill the chip once.  Measured on the training step (round 4,
// profiles/r04_attention_split_ab.txt): a workgroup alone on its CU runs almost twice as fast as one that shares it, so
// the partly filled LAST round of a long launch costs about half a round, not a whole one — splitting it saves 3-13 %
// of the kernel and the combine pass (10 us: the partial results are HBM traffic) takes that back; a launch of 156
// workgroups (one clip) on 256 CUs gains 25-37 % before the combine.
struct OmhSplitPlan { int n_regular, n_tail, splits; };
static inline OmhSplitPlan omh_tail_split_plan(int nwg, int slots, int loop_tiles, int min_tiles, bool single_round_only = false,
                                               double max_cost = 0.67) {
    OmhSplitPlan pl = {nwg, 0, 1};
    if (nwg <= 0 || slots <= 0) return pl;
    if (single_round_only && nwg >= slots) return pl;
    const int r = nwg % slots;
    if (r == 0) return pl;
    int smax = loop_tiles / min_tiles;
    if (smax > 8) smax = 8;
    int best_s = 1;
    double best = 1.0;
    for (int sp = 2; sp <= smax; ++sp) {
        const double c = (double)((r * sp + slots - 1) / slots) / sp;
        if (c < best - 1e-9) { best = c; best_s = sp; }
    }
    // at least a third of the round must go: 192 workgroups on 256 slots split 4 ways (0.75 of a round on paper)
    // measured 0.9 % SLOWER per training step at 4 clips — a lone workgroup already has its CU to itself
    if (best_s < 2 || best > max_cost) return pl;
    pl.n_tail = r;
    pl.n_regular = nwg - r;
    pl.splits = best_s;
    return pl;
}
static inline int omh_cu_count() {                       // whole XCDs; cached
    static int ncu = 0;
    if (!ncu) {
        int dev = 0;
        hipDeviceProp_t prop;
        ncu = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ? prop.multiProcessorCount : 256;
        ncu -= ncu % 8;
        if (ncu < 8) ncu = 256;
    }
    return ncu;
}
