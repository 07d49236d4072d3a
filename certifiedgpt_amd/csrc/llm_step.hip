// llm_step.hip -- the kernels of the LLaMA token step (sequences and C-ABI: llm.hip) and one launcher per kernel (llm.h, llm_select.h).
//
// One step = embedding lookup, layers x (RMSNorm, fused q/k/v GEMM, rotary + K/V append + one-query attention, o_proj GEMM +
// residual, RMSNorm, fused gate/up GEMM + SwiGLU, down GEMM + residual), final RMSNorm, lm_head GEMM.  The GEMMs are
// llm_gemm.hip; the rest is here.  Every kernel rounds where HF's fp16 eager model rounds: what is left between
// the two is summation order.  Feature work belongs in llm.hip: untouched, these 32 kernels are the code they were.
#include "llm.h"
#include "llm_select.h"

using namespace cgpt;

namespace {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
constexpr int HD = 128;                // head size the attention kernel is written for

__device__ __forceinline__ float rf16(float v) { return (float)(half_t)v; }
// fp16(a * b) as a value of its own: without the barrier the compiler contracts fp16(a * b) + c into one v_fma_f16, which skips
// the product's rounding -- closer to the exact result, but not where HF's eager model rounds (16 % of a rotated key row differed).
__device__ __forceinline__ float mul_f16(float a, float b) {
    float r = rf16(a * b);
    asm volatile("" : "+v"(r));
    return r;
}

// Early stop (cgpt_llm_set_early_stop): every kernel of a token step exists twice.  GUARD = true reads *live -- one
// int, uniform over the grid, written by llm_live_kernel earlier on the same stream -- before any load, LDS write or barrier and
// returns when it is 0.  GUARD = false never looks at `live` (null) and is the kernel as it was: cgpt_llm_step, the prefill's tail,
// the scoring pass and a greedy call with early stop off take it.

// h[b, :] = embed[token[b], :].  A token outside the table reads row 0 (never out of bounds).
template <bool GUARD>
__global__ __launch_bounds__(256) void llm_embed_kernel(const long long* __restrict__ tokens, const half_t* __restrict__ table,
                                                        int vocab, int hidden, half_t* __restrict__ h, const int* __restrict__ live) {
    if constexpr (GUARD)
        if (*live == 0) return;
    long long t = tokens[blockIdx.x];
    if (t < 0 || t >= vocab) t = 0;
    const h16x8* src = reinterpret_cast<const h16x8*>(table + (int64_t)t * hidden);
    h16x8* dst = reinterpret_cast<h16x8*>(h + (int64_t)blockIdx.x * hidden);
    for (int i = threadIdx.x; i < hidden / 8; i += 256) dst[i] = src[i];
}

// LlamaRMSNorm: y = weight * fp16(x * rsqrt(mean(x^2) + eps)), statistics in fp32, both products rounded to fp16.
// One workgroup per row; the sum runs in a fixed order (per-thread strided, wave butterfly, 4 wave sums in order).
template <bool GUARD>
__global__ __launch_bounds__(256) void llm_rmsnorm_kernel(const half_t* __restrict__ x, const half_t* __restrict__ w, int hidden,
                                                          float eps, half_t* __restrict__ y, const int* __restrict__ live) {
    __shared__ float wsum[4];
    if constexpr (GUARD)
        if (*live == 0) return;
    const half_t* xr = x + (int64_t)blockIdx.x * hidden;
    half_t* yr = y + (int64_t)blockIdx.x * hidden;
    float ss = 0.0f;
    for (int i = threadIdx.x; i < hidden / 8; i += 256) {
        const h16x8 v = reinterpret_cast<const h16x8*>(xr)[i];
#pragma unroll
        for (int e = 0; e < 8; ++e) ss += (float)v[e] * (float)v[e];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float total = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    const float inv = rsqrtf(total / (float)hidden + eps);
    for (int i = threadIdx.x; i < hidden / 8; i += 256) {
        const h16x8 v = reinterpret_cast<const h16x8*>(xr)[i];
        const h16x8 g = reinterpret_cast<const h16x8*>(w)[i];
        h16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)g[e] * rf16((float)v[e] * inv));
        reinterpret_cast<h16x8*>(yr)[i] = o;
    }
}

// cos / sin of the default rotary law: table[pos][0..63] = fp16(cos(pos * inv_freq[i])), [64..127] = fp16(sin(...)),
// the angle in fp32 as HF's LlamaRotaryEmbedding forms it.
__global__ __launch_bounds__(64) void llm_rope_table_kernel(const float* __restrict__ inv_freq, half_t* __restrict__ table) {
    const float a = (float)blockIdx.x * inv_freq[threadIdx.x];
    table[(int64_t)blockIdx.x * HD + threadIdx.x] = (half_t)cosf(a);
    table[(int64_t)blockIdx.x * HD + 64 + threadIdx.x] = (half_t)sinf(a);
}

// Rotary + K/V append + attention of one query, one wavefront per (row, head).
//   q, k, v  = the head's 128 columns of the fused projection row qkv[b, 0 | hidden | 2 hidden + h * 128 ...]
//   q', k'   = x * cos + rotate_half(x) * sin at position `pos`, each product and the sum rounded to fp16
//   K[b, h, pos, :] = k',  V[b, h, pos, :] = v        (the only cache rows written)
//   out[b, h * 128 ...] = fp16(softmax(q' . K[0..pos] / sqrt(128)) . V[0..pos]),  scores, probabilities and the sum in fp32
// HBM-bound: a head reads (pos + 1) x 2 x 256 B; a wave instruction covers 4 keys x 256 B in 16-byte lanes.
// RAGGED (left-padded rows, cgpt_llm_step_ragged): the token sits at buffer position `bufpos` of a row whose first real position is
// s = starts[b] (clamped into 0 .. smax; smax = the prompt's last buffer position, so that prefill and steps clamp alike).  The head's cache pointers move by s and `pos` stands for bufpos - s: rotary row
// bufpos - s, keys s .. bufpos walked in groups of four from s -- the unpadded row's operations in the unpadded row's order.
template <bool RAGGED, bool GUARD>
__global__ __launch_bounds__(64) void llm_attn_kernel(const half_t* __restrict__ qkv, int hidden, int heads, half_t* Kc, half_t* Vc,
                                                      int64_t len_stride, const half_t* __restrict__ rope, int bufpos,
                                                      half_t* __restrict__ out, const int* __restrict__ starts, int smax,
                                                      const int* __restrict__ live) {
    extern __shared__ float asmem[];                   // [128] rotated query, [128 + 128] halfs: the new key and value, [pos + 1] scores
    if constexpr (GUARD)
        if (*live == 0) return;
    float* qs = asmem;
    half_t* knew = reinterpret_cast<half_t*>(asmem + HD);
    half_t* vnew = knew + HD;
    float* sc = asmem + 2 * HD;
    const int b = blockIdx.x / heads, h = blockIdx.x % heads, lane = threadIdx.x;
    const half_t* q = qkv + (int64_t)b * 3 * hidden + h * HD;
    const half_t* k = q + hidden;
    const half_t* v = k + hidden;
    const int s = RAGGED ? min(max(starts[b], 0), min(smax, bufpos)) : 0;
    const int pos = bufpos - s;
    half_t* Kh = Kc + ((int64_t)(b * heads + h) * len_stride + s) * HD;
    half_t* Vh = Vc + ((int64_t)(b * heads + h) * len_stride + s) * HD;

    {   // lane i owns the rotary pair (i, i + 64)
        const float c = (float)rope[(int64_t)pos * HD + lane], s = (float)rope[(int64_t)pos * HD + 64 + lane];
        const float q0 = (float)q[lane], q1 = (float)q[lane + 64], k0 = (float)k[lane], k1 = (float)k[lane + 64];
        qs[lane] = rf16(mul_f16(q0, c) - mul_f16(q1, s));
        qs[lane + 64] = rf16(mul_f16(q1, c) + mul_f16(q0, s));
        const half_t r0 = (half_t)(mul_f16(k0, c) - mul_f16(k1, s)), r1 = (half_t)(mul_f16(k1, c) + mul_f16(k0, s));
        const half_t v0 = v[lane], v1 = v[lane + 64];
        Kh[(int64_t)pos * HD + lane] = knew[lane] = r0;
        Kh[(int64_t)pos * HD + lane + 64] = knew[lane + 64] = r1;
        Vh[(int64_t)pos * HD + lane] = vnew[lane] = v0;
        Vh[(int64_t)pos * HD + lane + 64] = vnew[lane + 64] = v1;
    }
    __syncthreads();                                   // key `pos` is attended from LDS: the cache row just stored is not read back

    const int n = pos + 1;
    const int kk = lane >> 4, dc = (lane & 15) * 8;    // key within a group of 4, first of the lane's 8 dims
    float qr[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) qr[e] = qs[dc + e];
    const float scale = 0.08838834764831845f;          // 1 / sqrt(128)
    float mx = -INFINITY;
    for (int t0 = 0; t0 < n; t0 += 4) {
        const int t = t0 + kk;
        float d = 0.0f;
        if (t < n) {
            const h16x8 kv = *reinterpret_cast<const h16x8*>(t == pos ? knew + dc : Kh + (int64_t)t * HD + dc);
#pragma unroll
            for (int e = 0; e < 8; ++e) d += qr[e] * (float)kv[e];
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) d += __shfl_xor(d, o);
        d *= scale;
        if (t < n) {
            mx = fmaxf(mx, d);
            if ((lane & 15) == 0) sc[t] = d;
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    __syncthreads();

    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float l = 0.0f;
    for (int t0 = 0; t0 < n; t0 += 4) {
        const int t = t0 + kk;
        if (t < n) {
            const float p = expf(sc[t] - mx);
            const h16x8 vv = *reinterpret_cast<const h16x8*>(t == pos ? vnew + dc : Vh + (int64_t)t * HD + dc);
            l += p;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += p * (float)vv[e];
        }
    }
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        acc[e] += __shfl_xor(acc[e], 16);
        acc[e] += __shfl_xor(acc[e], 32);
    }
    if (kk == 0) {
        h16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (half_t)(acc[e] / l);
        *reinterpret_cast<h16x8*>(out + (int64_t)b * hidden + h * HD + dc) = o;
    }
}

// Grouped-query attention (cgpt_llm_config_gqa.grouped_kv): the token step's attention with ONE read of a K/V head for
// the G = heads / kv_heads query heads that share it.  One workgroup per (row, K/V head), G wavefronts, wave w = query head
// kvh * G + w.  The caches are [B, kv_heads, len_stride, 128]; the fused projection row is [hidden | kv_heads * 128 | kv_heads * 128].
//   every wave rotates its own q; wave 0 rotates and appends the group's one new key / value row, to the cache and to LDS
//   score pass: the group's cache rows are staged into LDS in chunks of 64 keys (16-byte loads, all waves load), every wave takes
//       its dot products from the staged chunk; P.V pass: the same walk over V.  Two passes with the scores in LDS, as the plain kernel.
// A query's arithmetic and key order are exactly llm_attn_kernel's: keys in groups of four from the row's first real key (chunks
// begin at multiples of 64 keys from it, so the groups of four are the same groups), fp32 dot products with the 16-lane butterfly,
// the maximum, then expf(sc - mx) and acc += p * v in key order, the same final shuffles and the division.  Staging changes where
// a byte comes from, never the order of a sum: head h of a grouped handle gives the bits the plain kernel gives on a cache whose
// head h holds K/V head h / G.  RAGGED and GUARD as in llm_attn_kernel; every barrier sits in block-uniform control flow (n depends on
// the row alone).  Plain vector stores, no atomics.
// Dynamic LDS: [64][128] halfs staging, [128 + 128] halfs new key / value, G x [128] floats rotated queries, G x [bufpos + 1] floats
// scores (gqa_attn_lds_bytes; the limit is set at create, and a (G, max_len) that exceeds the CU's LDS is refused there).
constexpr int GQA_KC = 64;                          // keys staged per chunk

template <int G, bool RAGGED, bool GUARD>
__global__ __launch_bounds__(64 * G) void llm_attn_gqa_kernel(const half_t* __restrict__ qkv, int hidden, int kv_heads, half_t* Kc, half_t* Vc,
                                                              int64_t len_stride, const half_t* __restrict__ rope, int bufpos,
                                                              half_t* __restrict__ out, const int* __restrict__ starts, int smax,
                                                              const int* __restrict__ live) {
    extern __shared__ __attribute__((aligned(16))) float gsmem[];
    if constexpr (GUARD)
        if (*live == 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    half_t* stage = reinterpret_cast<half_t*>(gsmem);
    half_t* knew = stage + GQA_KC * HD;
    half_t* vnew = knew + HD;
    float* qs = reinterpret_cast<float*>(vnew + HD) + wave * HD;
    float* sc = reinterpret_cast<float*>(vnew + HD) + G * HD + (int64_t)wave * (bufpos + 1);
    const int b = blockIdx.x / kv_heads, kvh = blockIdx.x % kv_heads, h = kvh * G + wave;
    const int kvw = kv_heads * HD;
    const half_t* q = qkv + (int64_t)b * (hidden + 2 * kvw) + h * HD;
    const half_t* k = qkv + (int64_t)b * (hidden + 2 * kvw) + hidden + kvh * HD;
    const half_t* v = k + kvw;
    const int s = RAGGED ? min(max(starts[b], 0), min(smax, bufpos)) : 0;
    const int pos = bufpos - s;
    half_t* Kh = Kc + ((int64_t)(b * kv_heads + kvh) * len_stride + s) * HD;
    half_t* Vh = Vc + ((int64_t)(b * kv_heads + kvh) * len_stride + s) * HD;

    {   // lane i owns the rotary pair (i, i + 64)
        const float c = (float)rope[(int64_t)pos * HD + lane], s = (float)rope[(int64_t)pos * HD + 64 + lane];
        const float q0 = (float)q[lane], q1 = (float)q[lane + 64];
        qs[lane] = rf16(mul_f16(q0, c) - mul_f16(q1, s));
        qs[lane + 64] = rf16(mul_f16(q1, c) + mul_f16(q0, s));
        if (wave == 0) {
            const float k0 = (float)k[lane], k1 = (float)k[lane + 64];
            const half_t r0 = (half_t)(mul_f16(k0, c) - mul_f16(k1, s)), r1 = (half_t)(mul_f16(k1, c) + mul_f16(k0, s));
            const half_t v0 = v[lane], v1 = v[lane + 64];
            Kh[(int64_t)pos * HD + lane] = knew[lane] = r0;
            Kh[(int64_t)pos * HD + lane + 64] = knew[lane + 64] = r1;
            Vh[(int64_t)pos * HD + lane] = vnew[lane] = v0;
            Vh[(int64_t)pos * HD + lane + 64] = vnew[lane + 64] = v1;
        }
    }
    __syncthreads();                                   // key `pos` is attended from LDS: the cache row just stored is not read back

    const int n = pos + 1;
    const int kk = lane >> 4, dc = (lane & 15) * 8;    // key within a group of 4, first of the lane's 8 dims
    float qr[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) qr[e] = qs[dc + e];
    const float scale = 0.08838834764831845f;          // 1 / sqrt(128)
    float mx = -INFINITY;
    for (int c0 = 0; c0 < n; c0 += GQA_KC) {
        const int nk = min(GQA_KC, n - c0);
        if (c0 > 0) __syncthreads();                   // the previous chunk has been read by every wave
        for (int i = tid; i < nk * 16; i += 64 * G) {  // nk keys x 16 pieces of 16 bytes; key `pos` stays in knew
            const int key = i >> 4, d8 = (i & 15) * 8;
            if (c0 + key != pos)
                *reinterpret_cast<h16x8*>(stage + key * HD + d8) = *reinterpret_cast<const h16x8*>(Kh + (int64_t)(c0 + key) * HD + d8);
        }
        __syncthreads();
        for (int t0 = c0; t0 < c0 + nk; t0 += 4) {
            const int t = t0 + kk;
            float d = 0.0f;
            if (t < n) {
                const h16x8 kv = *reinterpret_cast<const h16x8*>(t == pos ? knew + dc : stage + (t - c0) * HD + dc);
#pragma unroll
                for (int e = 0; e < 8; ++e) d += qr[e] * (float)kv[e];
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) d += __shfl_xor(d, o);
            d *= scale;
            if (t < n) {
                mx = fmaxf(mx, d);
                if ((lane & 15) == 0) sc[t] = d;
            }
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));

    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float l = 0.0f;
    for (int c0 = 0; c0 < n; c0 += GQA_KC) {
        const int nk = min(GQA_KC, n - c0);
        __syncthreads();                               // the scores are written / the previous chunk has been read by every wave
        for (int i = tid; i < nk * 16; i += 64 * G) {
            const int key = i >> 4, d8 = (i & 15) * 8;
            if (c0 + key != pos)
                *reinterpret_cast<h16x8*>(stage + key * HD + d8) = *reinterpret_cast<const h16x8*>(Vh + (int64_t)(c0 + key) * HD + d8);
        }
        __syncthreads();
        for (int t0 = c0; t0 < c0 + nk; t0 += 4) {
            const int t = t0 + kk;
            if (t < n) {
                const float p = expf(sc[t] - mx);
                const h16x8 vv = *reinterpret_cast<const h16x8*>(t == pos ? vnew + dc : stage + (t - c0) * HD + dc);
                l += p;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += p * (float)vv[e];
            }
        }
    }
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        acc[e] += __shfl_xor(acc[e], 16);
        acc[e] += __shfl_xor(acc[e], 32);
    }
    if (kk == 0) {
        h16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (half_t)(acc[e] / l);
        *reinterpret_cast<h16x8*>(out + (int64_t)b * hidden + h * HD + dc) = o;
    }
}

typedef signed char i8x16 __attribute__((ext_vector_type(16)));

// The weight law of an int8 handle, one workgroup per source row of an HF nn.Linear.weight [rows, K] in fp16:
//   s = fp16(absmax / 127)           the maximum is exact in any order; the division is fp32, correctly rounded
//   q = clamp(rint(w / s), -127, 127)   fp32 division, round to nearest even; s == 0 (a zero row, or an underflow): q = 0
// Row r goes to row r of the destination (interleave < 0) or to row 32 (r / 16) + 16 interleave + r % 16 (gate / up fusion):
// a row keeps its scale.  16 values per thread and pass: 16-byte stores.
__global__ __launch_bounds__(256) void llm_quant_rows_kernel(const half_t* __restrict__ w, int K, int interleave,
                                                             signed char* __restrict__ q, half_t* __restrict__ scales) {
    __shared__ float wmax[4];
    const int r = blockIdx.x;
    const int dr = interleave < 0 ? r : 32 * (r / 16) + 16 * interleave + (r % 16);
    const h16x8* src = reinterpret_cast<const h16x8*>(w + (int64_t)r * K);
    float amax = 0.0f;
    for (int i = threadIdx.x; i < K / 8; i += 256) {
        const h16x8 v = src[i];
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf((float)v[e]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    const half_t sh = (half_t)__fdiv_rn(amax, 127.0f);
    const float sf = (float)sh;
    if (threadIdx.x == 0) scales[dr] = sh;
    i8x16* dst = reinterpret_cast<i8x16*>(q + (int64_t)dr * K);
    for (int i = threadIdx.x; i < K / 16; i += 256) {
        const h16x8 lo = src[2 * i], hi = src[2 * i + 1];
        i8x16 o;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float x = (float)(e < 8 ? lo[e] : hi[e - 8]);
            const float t = fminf(fmaxf(rintf(__fdiv_rn(x, sf)), -127.0f), 127.0f);
            o[e] = sf == 0.0f ? (signed char)0 : (signed char)(int)t;
        }
        dst[i] = o;
    }
}

// out[n, k] = fp16(q[n, k]) * s[n] (ONE fp16 multiply; the conversion is exact) for the rows_padded x K int8 matrix of an int8
// handle: the prefill's expansion into the handle's fp16 scratch.  Pad rows hold q = 0 and s = 0 and come out as zeros.
// One thread per 16 values: a 16-byte load, two 16-byte stores.
__global__ __launch_bounds__(256) void llm_dequant_kernel(const signed char* __restrict__ q, const half_t* __restrict__ scales, int K,
                                                          int64_t chunks, half_t* __restrict__ out) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= chunks) return;
    const int per_row = K / 16;
    const half_t s = scales[id / per_row];
    const i8x16 v = reinterpret_cast<const i8x16*>(q)[id];
    h16x8 lo, hi;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        lo[e] = (half_t)(short)v[e];
        hi[e] = (half_t)(short)v[e + 8];
    }
    lo = lo * s;
    hi = hi * s;
    asm volatile("" : "+v"(lo), "+v"(hi));                 // the products stay values of their own
    reinterpret_cast<h16x8*>(out)[2 * id] = lo;
    reinterpret_cast<h16x8*>(out)[2 * id + 1] = hi;
}

// EosIds, StopSeqs and the bookkeeping tail of a select (CGPT_SELECT_TAIL) are llm_select.h's: the sampled select (llm_sample.hip) shares them.

// Greedy bookkeeping of one step, one workgroup per row (greedy_tokens in minigpt4.py): EOS columns read as -inf while
// `mask_eos` (the first min_new_tokens steps), first-max arg-max, pad once the row has produced an EOS.
//   dst != null: the (masked) logits are also written there (row stride ldd); dst may be src.
//   first != 0:  every row starts unfinished (step 0)
// GUARD (early stop): a select other than the first that reads *live == 0 -- every row has produced an EOS -- is a dead select: no
// vocabulary scan, no logits copy, `unfinished` left as it is (all zeros); it writes the pad id, which is what the scan would have
// ended in.  The first select never reads `live` (it holds the previous call's value until llm_live_kernel has run).
// STOP (stop sequences): a still-unfinished row also finishes when its tokens up to and including this one end in one of the
// sequences.  The row's earlier tokens are read back from tokens_out (columns col - 1, col - 2, ..., written by the earlier selects
// of the call on the same stream); a sequence longer than col + 1 is skipped, so nothing left of column 0 -- the previous row's last
// tokens -- is ever read.  STOP = false is the kernel as it was.
template <bool GUARD, bool STOP = false>
__global__ __launch_bounds__(256) void llm_select_kernel(const float* src, int64_t lds, float* dst, int64_t ldd, int vocab,
                                                         int mask_eos, EosIds eos, long long pad, int first, int* __restrict__ unfinished,
                                                         long long* __restrict__ tokens_out, int64_t ld_tokens,
                                                         long long* __restrict__ next_tok, const int* __restrict__ live,
                                                         StopArg<STOP> stop) {
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int row = blockIdx.x;
    if constexpr (GUARD) {
        if (!first && *live == 0) {
            if (threadIdx.x == 0) {
                tokens_out[(int64_t)row * ld_tokens] = pad;
                next_tok[row] = pad;
            }
            return;
        }
    }
    const float* s = src + (int64_t)row * lds;
    float* d = dst ? dst + (int64_t)row * ldd : nullptr;
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int j = threadIdx.x; j < vocab; j += 256) {
        float v = s[j];
        if (mask_eos)
            for (int e = 0; e < eos.n; ++e)
                if (eos.id[e] == j) v = -INFINITY;
        if (d) d[j] = v;
        if (idx == 0x7fffffff || v > best) { best = v; idx = j; }          // ascending j: the first maximum stays
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(idx, o);
        if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
    }
    if ((threadIdx.x & 63) == 0) { bv[threadIdx.x >> 6] = best; bi[threadIdx.x >> 6] = idx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
        CGPT_SELECT_TAIL(STOP, row, idx, first, eos, pad, unfinished, tokens_out, ld_tokens, next_tok, stop);
    }
}

// The reduction behind early stop, ONE workgroup of 256 threads after a select (rows <= 256): live = any(unfinished[0 .. rows)), and
// live_steps counts the token steps of the call that run: reset by the first select's launch, + 1 when a step follows this select
// (`more`) and some row is unfinished.  The next launches of the stream read `live` (the kernel boundary orders the store).
__global__ __launch_bounds__(256) void llm_live_kernel(const int* __restrict__ unfinished, int rows, int first, int more,
                                                       int* __restrict__ live, int* __restrict__ live_steps) {
    const int u = (int)threadIdx.x < rows ? unfinished[threadIdx.x] : 0;
    const int any = __syncthreads_or(u) ? 1 : 0;
    if (threadIdx.x == 0) {
        const int steps = first ? 0 : *live_steps;
        *live = any;
        *live_steps = steps + (any & more);
    }
}

// The step attention of one (G, RAGGED, GUARD); G = 0 is llm_attn_kernel, whose third argument is `heads` where the grouped kernel has kv_heads.
using AttnFn = void (*)(const half_t*, int, int, half_t*, half_t*, int64_t, const half_t*, int, half_t*, const int*, int, const int*);
template <int G, bool RAGGED>
AttnFn attn_pick(bool guard) {
    if constexpr (G == 0) return guard ? llm_attn_kernel<RAGGED, true> : llm_attn_kernel<RAGGED, false>;
    else return guard ? llm_attn_gqa_kernel<G, RAGGED, true> : llm_attn_gqa_kernel<G, RAGGED, false>;
}
template <int G>
AttnFn attn_fn(bool ragged, bool guard) { return ragged ? attn_pick<G, true>(guard) : attn_pick<G, false>(guard); }
AttnFn attn_fn(int G, bool r, bool g) {                    // the one G dispatch
    return G == 0 ? attn_fn<0>(r, g) : G == 1 ? attn_fn<1>(r, g) : G == 2 ? attn_fn<2>(r, g) : G == 4 ? attn_fn<4>(r, g) : attn_fn<8>(r, g);
}

}  // namespace

namespace cgpt {

hipError_t launch_llm_embed(const long long* tokens, const half_t* table, int vocab, int hidden, half_t* h, int rows, hipStream_t st, const int* live) {
    hipLaunchKernelGGL(live ? llm_embed_kernel<true> : llm_embed_kernel<false>, dim3(rows), dim3(256), 0, st, tokens, table, vocab, hidden, h, live);
    return hipGetLastError();
}
hipError_t launch_llm_rmsnorm(const half_t* x, const half_t* w, int hidden, float eps, half_t* y, int rows, hipStream_t st, const int* live) {
    hipLaunchKernelGGL(live ? llm_rmsnorm_kernel<true> : llm_rmsnorm_kernel<false>, dim3(rows), dim3(256), 0, st, x, w, hidden, eps, y, live);
    return hipGetLastError();
}
hipError_t launch_llm_rope_table(const float* inv_freq, half_t* table, int positions, hipStream_t st) {
    hipLaunchKernelGGL(llm_rope_table_kernel, dim3(positions), dim3(64), 0, st, inv_freq, table);
    return hipGetLastError();
}

size_t llm_step_attn_lds_bytes(int G, int positions) {
    return G == 0 ? (size_t)(2 * HD + positions) * sizeof(float)
                  : (size_t)(GQA_KC + 2) * HD * sizeof(half_t) + (size_t)G * (HD + positions) * sizeof(float);
}
hipError_t llm_step_prepare(int G, int max_len) {
    hipError_t e = hipSuccess;                             // G = 0: the plain kernel stays below the default limit up to max_len = 8192
    for (int i = 0; i < 4 && G && e == hipSuccess; ++i)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(attn_fn(G, i & 2, i & 1)), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)llm_step_attn_lds_bytes(G, max_len));
    return e;
}
hipError_t launch_llm_step_attention(const StepAttnArgs& a, int rows, hipStream_t st) {
    const int kvh = a.G ? a.heads / a.G : a.heads;
    hipLaunchKernelGGL(attn_fn(a.G, a.starts != nullptr, a.live != nullptr), dim3(rows * kvh), dim3(a.G ? 64 * a.G : 64),
                       llm_step_attn_lds_bytes(a.G, a.pos + 1), st, a.qkv, a.hidden, kvh, a.Kc, a.Vc, a.len_stride, a.rope, a.pos, a.out,
                       a.starts, a.starts ? a.smax : 0, a.live);
    return hipGetLastError();
}

hipError_t launch_llm_quant_rows(const half_t* w, int rows, int K, int interleave, signed char* q, half_t* scales, hipStream_t st) {
    hipLaunchKernelGGL(llm_quant_rows_kernel, dim3((unsigned)rows), dim3(256), 0, st, w, K, interleave, q, scales);
    return hipGetLastError();
}
hipError_t launch_llm_dequant(const signed char* q, const half_t* scales, int N, int K, half_t* out, hipStream_t st) {
    const int64_t chunks = (int64_t)((N + 255) / 256 * 256) * (K / 16);
    hipLaunchKernelGGL(llm_dequant_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, st, q, scales, K, chunks, out);
    return hipGetLastError();
}

hipError_t launch_llm_select(bool guard, const StopSeqs* stop, const SelectArgs& a, int rows, hipStream_t st) {
    auto go = [&](auto kernel, auto s) {
        hipLaunchKernelGGL(kernel, dim3(rows), dim3(256), 0, st, a.src, a.lds, a.dst, a.ldd, a.vocab, a.mask_eos, a.eos, a.pad, a.first,
                           a.unfinished, a.tokens_out, a.ld_tokens, a.next_tok, a.live, s);
    };
    if (stop) go(guard ? llm_select_kernel<true, true> : llm_select_kernel<false, true>, *stop);
    else go(guard ? llm_select_kernel<true, false> : llm_select_kernel<false, false>, NoStop{});
    return hipGetLastError();
}
hipError_t launch_llm_live(const int* unfinished, int rows, int first, int more, int* live, int* live_steps, hipStream_t st) {
    hipLaunchKernelGGL(llm_live_kernel, dim3(1), dim3(256), 0, st, unfinished, rows, first, more, live, live_steps);
    return hipGetLastError();
}

}  // namespace cgpt
