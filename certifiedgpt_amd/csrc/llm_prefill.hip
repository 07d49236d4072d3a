// llm_prefill.hip -- the kernels of the native LLaMA prefill (cgpt_llm_prefill, include/cgpt.h) that are not GEMMs: residual add +
// RMSNorm, rotary + K/V cache write, causal self-attention for head size 128, SwiGLU.  The GEMMs between them are the large-shape
// path (launch_gemm); llm.hip strings the launches together.
//
// Reference call replaced: the first forward inside `self.llama_model.generate(...)` (minigpt_base.py:418-431), HF
// LlamaForCausalLM on B prompts of L positions each (no padding, positions 0 .. L-1).  Token row r = b * L + p everywhere.
// Left-padded prompts (cgpt_llm_prefill_ragged): a device array starts[B] gives each row's number of pad positions; the rotary and
// attention kernels have a RAGGED instantiation that works in row-relative coordinates -- the row's q / k / v, cache and output
// pointers moved by start[b], the same arithmetic on len[b] = L - start[b] positions -- so a padded row performs the operations of
// the unpadded run in the same order.  The plain instantiation reads no starts and compiles to the code it was before.
// Every kernel rounds where HF's fp16 eager model rounds; the one documented difference is the attention
// probabilities, which are rounded to fp16 as the MFMA operand of P.V.  Plain vector stores, no atomics, fixed summation orders:
// a row's result does not depend on the rows around it or on the launch.
#include <math.h>

#include "llm.h"

namespace cgpt {

namespace {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int HD = 128;

__device__ __forceinline__ float rf16(float v) { return (float)(half_t)v; }
// fp16(a * b) as a value of its own (llm_step.hip: kept from contracting into a fused multiply-add, which would skip the rounding)
__device__ __forceinline__ float mul_f16(float a, float b) {
    float r = rf16(a * b);
    asm volatile("" : "+v"(r));
    return r;
}

// x_out[r] = fp16(x[src(r)] + delta[src(r)])   (delta == null: x_out[r] = x[src(r)]),   y[r] = weight * fp16(x_out[r] * rsqrt(mean + eps))
// with src(r) = r * src_mul + src_add: the identity for the layers, row (b * L + L - 1) for the tail's gather of last positions.
// One workgroup per row; the statistics are llm_rmsnorm_kernel's: fp32, per-thread strided, wave butterfly, 4 wave sums in order.
// x_out may alias x (each thread reads back only what it wrote itself).
__global__ __launch_bounds__(256) void llm_prefill_addnorm_kernel(const half_t* x, const half_t* __restrict__ delta, int64_t src_mul,
                                                                  int64_t src_add, const half_t* __restrict__ w, int hidden, float eps,
                                                                  half_t* x_out, half_t* __restrict__ y) {
    __shared__ float wsum[4];
    const int64_t src = (int64_t)blockIdx.x * src_mul + src_add;
    const half_t* xr = x + src * hidden;
    const half_t* dr = delta ? delta + src * hidden : nullptr;
    half_t* xo = x_out + (int64_t)blockIdx.x * hidden;
    half_t* yr = y + (int64_t)blockIdx.x * hidden;
    float ss = 0.0f;
    for (int i = threadIdx.x; i < hidden / 8; i += 256) {
        h16x8 v = reinterpret_cast<const h16x8*>(xr)[i];
        if (dr) {
            const h16x8 d = reinterpret_cast<const h16x8*>(dr)[i];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (half_t)((float)v[e] + (float)d[e]);
        }
        reinterpret_cast<h16x8*>(xo)[i] = v;
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
        const h16x8 v = reinterpret_cast<const h16x8*>(xo)[i];
        const h16x8 g = reinterpret_cast<const h16x8*>(w)[i];
        h16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)g[e] * rf16((float)v[e] * inv));
        reinterpret_cast<h16x8*>(yr)[i] = o;
    }
}

// Rotary + cache write, one thread per (token row, head, 8 rotary pairs): q is rotated in place in the fused projection row, the
// rotated k and the v go to cache row p of (b, head).  The arithmetic is llm_attn_kernel's head: x' = x cos + rotate_half(x) sin,
// each product and the sum rounded to fp16.  RAGGED: the rotary angle of buffer position p is table row p - start[b] (start clamped
// into 0 .. L-1); pad positions p < start[b] are left alone -- q is not rotated, their cache rows are NOT written.
// GROUPED (grouped-query attention): the projection row is [hidden | kv_heads * 128 | kv_heads * 128] and the cache
// [B, kv_heads, len_stride, 128]: q is rotated for all heads; k is rotated, and k / v written, by the threads of heads 0 .. kv_heads-1.
// The plain instantiation never reads kv_heads.
// CONT (cgpt_llm_prefill_from): the L positions of a row follow pos0 positions whose cache rows exist.  Token row p takes rotary row
// pos0 + p (RAGGED: pos0 + p - start[b]) and cache row pos0 + p, which is the layout the whole prompt of pos0 + L positions has
// under the same starts: [start[b] pad rows][pos0 earlier rows][the row's real new rows].  CONT = false never reads pos0.
template <bool RAGGED, bool GROUPED, bool CONT = false>
__global__ __launch_bounds__(256) void llm_prefill_rope_kernel(half_t* __restrict__ qkv, int64_t rows, int L, int hidden, int heads,
                                                               half_t* __restrict__ Kc, half_t* __restrict__ Vc, int64_t len_stride,
                                                               const half_t* __restrict__ rope, const int* __restrict__ starts,
                                                               int kv_heads, int pos0) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= rows * heads * 8) return;
    const int c8 = (int)(id & 7) * 8;
    const int h = (int)((id >> 3) % heads);
    const int64_t r = (id >> 3) / heads;
    const int b = (int)(r / L), p = (int)(r % L);
    int rp = p;                                              // row of the rotary table
    if (RAGGED) {
        const int s = min(max(starts[b], 0), L - 1);
        if (p < s) return;
        rp = p - s;
    }
    if constexpr (CONT) rp += pos0;
    const h16x8 cs = *reinterpret_cast<const h16x8*>(rope + (int64_t)rp * HD + c8);
    const h16x8 sn = *reinterpret_cast<const h16x8*>(rope + (int64_t)rp * HD + 64 + c8);
    if constexpr (GROUPED) {
        if (h >= kv_heads) {                                 // a query head without a K/V head of its own: q only
            half_t* q = qkv + r * (hidden + 2 * kv_heads * HD) + h * HD + c8;
            const h16x8 q0 = *reinterpret_cast<const h16x8*>(q), q1 = *reinterpret_cast<const h16x8*>(q + 64);
            h16x8 qa, qb;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float c = (float)cs[e], s = (float)sn[e];
                qa[e] = (half_t)(mul_f16((float)q0[e], c) - mul_f16((float)q1[e], s));
                qb[e] = (half_t)(mul_f16((float)q1[e], c) + mul_f16((float)q0[e], s));
            }
            *reinterpret_cast<h16x8*>(q) = qa;
            *reinterpret_cast<h16x8*>(q + 64) = qb;
            return;
        }
    }
    half_t* q = qkv + r * (GROUPED ? hidden + 2 * kv_heads * HD : 3 * hidden) + h * HD + c8;
    half_t* k = q + hidden;                                  // head h of the k block: h < kv_heads
    const half_t* v = k + (GROUPED ? kv_heads * HD : hidden);
    const int64_t crow = ((int64_t)(b * (GROUPED ? kv_heads : heads) + h) * len_stride + (CONT ? pos0 + p : p)) * HD + c8;
    const h16x8 q0 = *reinterpret_cast<const h16x8*>(q), q1 = *reinterpret_cast<const h16x8*>(q + 64);
    const h16x8 k0 = *reinterpret_cast<const h16x8*>(k), k1 = *reinterpret_cast<const h16x8*>(k + 64);
    h16x8 qa, qb, ka, kb;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float c = (float)cs[e], s = (float)sn[e];
        qa[e] = (half_t)(mul_f16((float)q0[e], c) - mul_f16((float)q1[e], s));
        qb[e] = (half_t)(mul_f16((float)q1[e], c) + mul_f16((float)q0[e], s));
        ka[e] = (half_t)(mul_f16((float)k0[e], c) - mul_f16((float)k1[e], s));
        kb[e] = (half_t)(mul_f16((float)k1[e], c) + mul_f16((float)k0[e], s));
    }
    *reinterpret_cast<h16x8*>(q) = qa;
    *reinterpret_cast<h16x8*>(q + 64) = qb;
    *reinterpret_cast<h16x8*>(Kc + crow) = ka;
    *reinterpret_cast<h16x8*>(Kc + crow + 64) = kb;
    *reinterpret_cast<h16x8*>(Vc + crow) = *reinterpret_cast<const h16x8*>(v);
    *reinterpret_cast<h16x8*>(Vc + crow + 64) = *reinterpret_cast<const h16x8*>(v + 64);
}

// Causal self-attention, head size 128: out[b, p, head] = softmax(q_p . K[0..p] / sqrt(128)) . V[0..p].
// One workgroup per (b, head, block of 64 queries); wave w owns queries 16 w .. 16 w + 15 of the block.  The keys the block can see
// are walked in chunks of 64: all four waves stage the chunk's K rows ([key][128], rows padded to 136 halfs) and its V rows
// transposed ([dim][key], rows padded to 72 halfs) in LDS, then each wave runs an online softmax over the chunk's two 32-key blocks.
//   scores, transposed:  S^T[key, q] = K[key, :] . Q[q, :]   4 x v_mfma_f32_16x16x32_f16 per 16 keys (A = K rows from LDS, B = Q rows
//       from registers); the lane then holds q = lane & 15 and keys 4 g + r (g = lane >> 4) of both 16-key tiles, in fp32
//   softmax statistics in fp32 (running maximum and sum per query, reduced over the lane's 8 keys, then lanes +-16, +-32: fixed order)
//   P.V: the lane's 8 probabilities, rounded to fp16, ARE the A fragment of q = lane & 15 with the MFMA's k slot (g, j) standing
//       for key 4 g + j (j < 4) or 16 + 4 g + j - 4; the B fragment reads V^T[dim][the same keys] from LDS, 8 MFMAs per 32 keys.
// Queries at or past L (last block) are computed on clamped rows and not stored; keys at or past L or above the query are masked.
// RAGGED: query and key indices are relative to s = start[b] (clamped into 0 .. L-1) and L stands for len = L - s, so the 64-key
// chunks and 32-key blocks begin at the row's first real token: fully padded chunks cost nothing and the summation order of a row is
// the unpadded run's.  Pad queries are never computed (key 0 of the relative walk is visible to every query that is); the block
// whose grid index covers buffer positions below s writes those rows of the output as zeros, and a block past the row's last real
// query leaves before the first barrier (block-uniform).
constexpr int AQ = 64, AKC = 64, AKP = HD + 8, AVP = AKC + 8;

// GROUPED: query head h reads K/V head h / (heads / kv_heads) of a [B, kv_heads, len_stride, 128] cache, and a
// projection row is hidden + 2 kv_heads 128 wide.  Each query head still stages its K/V head for itself (the G heads of a group do
// not share a staged chunk here: this kernel is 3 % of a prefill).  The plain instantiation never reads kv_heads.
//
// CONT (cgpt_llm_prefill_from): the queries are positions pos0 .. pos0 + Lbuf - 1 (RAGGED: relative to s, pos0 .. pos0 + Lbuf - s - 1)
// and qkv / out hold their Lbuf rows only: query q is row b Lbuf + (q - pos0) (RAGGED: + s); keys are cache rows 0 .. q as ever, the
// earlier ones left by an earlier call.  The queries are tiled by their ABSOLUTE position -- grid index y stands for block
// pos0 / 64 + y, queries 64 (pos0 / 64 + y) .., wave w for 16 w .. of them -- so a query meets the 64-key chunks, the 32-key blocks,
// the wave-uniform break and the reduction order it meets in the plain kernel on the whole prompt: its output has the same bits.
// Queries of the first block below pos0 are treated like queries past L: read from a clamped row, never stored; a wave that has
// none at or above pos0 still stages and meets the barriers.  CONT = false never reads pos0.
template <bool RAGGED, bool GROUPED, bool CONT = false>
__global__ __launch_bounds__(256) void llm_prefill_attn_kernel(const half_t* __restrict__ qkv, int Lbuf, int hidden, int heads,
                                                               const half_t* __restrict__ Kc, const half_t* __restrict__ Vc,
                                                               int64_t len_stride, half_t* __restrict__ out,
                                                               const int* __restrict__ starts, int kv_heads, int pos0) {
    __shared__ __attribute__((aligned(16))) half_t ks[AKC * AKP];
    __shared__ __attribute__((aligned(16))) half_t vt[HD * AVP];
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    const int qbase = (CONT ? pos0 / AQ + (int)blockIdx.y : (int)blockIdx.y) * AQ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r15 = lane & 15, g = lane >> 4;
    const int q0 = qbase + wave * 16;                       // wave-uniform
    int s = 0;
    if (RAGGED) {
        s = min(max(starts[b], 0), Lbuf - 1);
        for (int i = tid; i < AQ * 16; i += 256) {           // pad query rows among buffer positions qbase .. qbase + 63: zeros
            const int row = (CONT ? qbase - pos0 : qbase) + (i >> 4);
            if (row < s && (!CONT || row >= 0))
                *reinterpret_cast<h16x8*>(out + ((int64_t)b * Lbuf + row) * hidden + h * HD + (i & 15) * 8) = h16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
        if (qbase >= (CONT ? pos0 + Lbuf - s : Lbuf - s)) return;
    }
    const int L = CONT ? pos0 + Lbuf - s : Lbuf - s;         // real positions; everything below is relative to the first of them
    const int64_t row0 = CONT ? (int64_t)b * Lbuf + s - pos0 : (int64_t)b * Lbuf + s;      // row0 + q: the row of (relative) query q
    const int64_t chead = GROUPED ? (int64_t)b * kv_heads + h / (heads / kv_heads) : (int64_t)(b * heads + h);
    const int64_t ldq = GROUPED ? hidden + 2 * kv_heads * HD : 3 * hidden;
    const half_t* Kh = Kc + (chead * len_stride + s) * HD;
    const half_t* Vh = Vc + (chead * len_stride + s) * HD;

    // B fragments of the wave's 16 queries: Q[q0 + r15][32 d + 8 g ..]
    h16x8 qf[4];
    {
        const int qrow = CONT ? max(min(q0 + r15, L - 1), pos0) : min(q0 + r15, L - 1);
        const half_t* qp = qkv + (row0 + qrow) * ldq + h * HD + 8 * g;
#pragma unroll
        for (int d = 0; d < 4; ++d) qf[d] = *reinterpret_cast<const h16x8*>(qp + 32 * d);
    }
    const int myq = q0 + r15;                                // the query of this lane's score columns
    const float scale = 0.08838834764831845f;                // 1 / sqrt(128)
    float mrun = -INFINITY, lrun = 0.0f;
    f32x4 o[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int last_key = min(L - 1, qbase + AQ - 1);
    for (int k0 = 0; k0 <= last_key; k0 += AKC) {
        __syncthreads();                                     // the previous chunk has been read by every wave
#pragma unroll
        for (int i = 0; i < 4; ++i) {                        // 64 keys x 16 chunks of 16 bytes, K and V
            const int c = tid + 256 * i, key = c >> 4, d8 = (c & 15) * 8;
            h16x8 kv = h16x8{0, 0, 0, 0, 0, 0, 0, 0}, vv = kv;
            if (k0 + key < L) {
                kv = *reinterpret_cast<const h16x8*>(Kh + (int64_t)(k0 + key) * HD + d8);
                vv = *reinterpret_cast<const h16x8*>(Vh + (int64_t)(k0 + key) * HD + d8);
            }
            *reinterpret_cast<h16x8*>(ks + key * AKP + d8) = kv;
#pragma unroll
            for (int e = 0; e < 8; ++e) vt[(d8 + e) * AVP + key] = vv[e];
        }
        __syncthreads();
        if (q0 >= L || (CONT && q0 + 15 < pos0)) continue;   // a wave with no query still stages and meets the barriers
#pragma unroll
        for (int kb = 0; kb < AKC; kb += 32) {
            const int kbase = k0 + kb;
            if (kbase > min(q0 + 15, L - 1)) break;          // wave-uniform: nothing of this block is visible
            f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = s0;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const h16x8 a0 = *reinterpret_cast<const h16x8*>(ks + (kb + r15) * AKP + 32 * d + 8 * g);
                const h16x8 a1 = *reinterpret_cast<const h16x8*>(ks + (kb + 16 + r15) * AKP + 32 * d + 8 * g);
                s0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, qf[d], s0, 0, 0, 0);
                s1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, qf[d], s1, 0, 0, 0);
            }
            float sc[8];
            float bmax = -INFINITY;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int key = kbase + (j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4));
                const float v = (j < 4 ? s0[j] : s1[j - 4]) * scale;
                sc[j] = (key <= myq && key < L) ? v : -INFINITY;
                bmax = fmaxf(bmax, sc[j]);
            }
            bmax = fmaxf(bmax, __shfl_xor(bmax, 16));
            bmax = fmaxf(bmax, __shfl_xor(bmax, 32));
            // (relative) key 0 is visible to every query, so from the first block on the running maximum is finite
            const float mnew = fmaxf(mrun, bmax);
            const float alpha = expf(mrun - mnew);
            float psum = 0.0f;
            h16x8 pf;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float p = expf(sc[j] - mnew);
                psum += p;
                pf[j] = (half_t)p;
            }
            psum += __shfl_xor(psum, 16);
            psum += __shfl_xor(psum, 32);
            lrun = lrun * alpha + psum;
            mrun = mnew;
            // the accumulator rows are queries 4 g + r: their alpha lives in the lanes whose r15 is that query
            float ar[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) ar[r] = __shfl(alpha, 4 * g + r);
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const half_t* vp = vt + (16 * t + r15) * AVP + kb + 4 * g;
                const h16x4 lo = *reinterpret_cast<const h16x4*>(vp), hi = *reinterpret_cast<const h16x4*>(vp + 16);
                const h16x8 bf = h16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                f32x4 acc = o[t];
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] *= ar[r];
                o[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pf, bf, acc, 0, 0, 0);
            }
        }
    }
    if (q0 >= L || (CONT && q0 + 15 < pos0)) return;
    float lr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) lr[r] = __shfl(lrun, 4 * g + r);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = q0 + 4 * g + r;
        if (q >= L || (CONT && q < pos0)) continue;
        half_t* orow = out + (row0 + q) * hidden + h * HD + r15;
#pragma unroll
        for (int t = 0; t < 8; ++t) orow[16 * t] = (half_t)(o[t][r] / lr[r]);
    }
}

// Prefix broadcast (cgpt_llm_kv_broadcast): rows 0 .. P-1 of every head of a one-row cache [1, kv_heads, src_stride, 128] go to rows
// s_b .. s_b + P - 1 of every row b of a [B, kv_heads, dst_stride, 128] cache, s_b = start[b] clamped into 0 .. dst_stride - P (0
// without starts).  One thread per 16 bytes; blockIdx.y = 0 copies K, 1 copies V.  Nothing else is written.
__global__ __launch_bounds__(256) void llm_kv_broadcast_kernel(const half_t* __restrict__ srcK, const half_t* __restrict__ srcV,
                                                               int64_t src_stride, int P, int B, int kv_heads,
                                                               const int* __restrict__ starts, half_t* __restrict__ dstK,
                                                               half_t* __restrict__ dstV, int64_t dst_stride) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (int64_t)B * kv_heads * P * 16) return;
    const int c8 = (int)(id & 15) * 8;
    const int p = (int)((id >> 4) % P);
    const int64_t bh = (id >> 4) / P;
    const int b = (int)(bh / kv_heads), h = (int)(bh % kv_heads);
    const int s = starts ? (int)min((int64_t)max(starts[b], 0), dst_stride - P) : 0;
    const half_t* src = (blockIdx.y ? srcV : srcK) + ((int64_t)h * src_stride + p) * HD + c8;
    half_t* dst = (blockIdx.y ? dstV : dstK) + (((int64_t)b * kv_heads + h) * dst_stride + s + p) * HD + c8;
    *reinterpret_cast<h16x8*>(dst) = *reinterpret_cast<const h16x8*>(src);
}

__device__ __forceinline__ float silu_f16(float gate) { return rf16(gate / (1.0f + expf(-gate))); }

// act[r, c] = fp16(fp16(silu(gate)) * up) on the fused gate / up product, whose columns are interleaved in blocks of 16 as the
// weights are stored for DEC_SWIGLU: gate of column c at (c >> 4) * 32 + (c & 15), up 16 further.  One thread per 8 columns.
__global__ __launch_bounds__(256) void llm_prefill_swiglu_kernel(const half_t* __restrict__ gu, int64_t rows, int mlp,
                                                                 half_t* __restrict__ act) {
    const int per_row = mlp / 8;
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= rows * per_row) return;
    const int64_t r = id / per_row;
    const int c = (int)(id % per_row) * 8;
    const half_t* src = gu + r * 2 * mlp + (c >> 4) * 32 + (c & 15);
    const h16x8 gv = *reinterpret_cast<const h16x8*>(src), uv = *reinterpret_cast<const h16x8*>(src + 16);
    h16x8 ov;
#pragma unroll
    for (int e = 0; e < 8; ++e) ov[e] = (half_t)(silu_f16((float)gv[e]) * (float)uv[e]);
    *reinterpret_cast<h16x8*>(act + r * mlp + c) = ov;
}

}  // namespace

hipError_t launch_prefill_addnorm(const half_t* x, const half_t* delta, int64_t src_mul, int64_t src_add, const half_t* w, int hidden,
                                  float eps, half_t* x_out, half_t* y, int64_t rows, hipStream_t stream) {
    if (rows < 1 || hidden < 8 || hidden % 8 || !x || !w || !x_out || !y) return hipErrorInvalidValue;
    hipLaunchKernelGGL(llm_prefill_addnorm_kernel, dim3((unsigned)rows), dim3(256), 0, stream, x, delta, src_mul, src_add, w, hidden, eps,
                       x_out, y);
    return hipGetLastError();
}

hipError_t launch_prefill_rope(half_t* qkv, int B, int L, int hidden, int heads, int kv_heads, half_t* Kc, half_t* Vc, int64_t len_stride,
                               const half_t* rope, const int32_t* starts, hipStream_t stream) {
    if (B < 1 || L < 1 || L > len_stride || hidden != heads * HD || kv_heads < 1 || kv_heads > heads || heads % kv_heads || !qkv || !Kc ||
        !Vc || !rope)
        return hipErrorInvalidValue;
    const int64_t rows = (int64_t)B * L, threads = rows * heads * 8;
    const dim3 grid((unsigned)((threads + 255) / 256));
    const bool grouped = kv_heads != heads;
    if (grouped && starts)
        hipLaunchKernelGGL((llm_prefill_rope_kernel<true, true>), grid, dim3(256), 0, stream, qkv, rows, L, hidden, heads, Kc, Vc, len_stride,
                           rope, starts, kv_heads, 0);
    else if (grouped)
        hipLaunchKernelGGL((llm_prefill_rope_kernel<false, true>), grid, dim3(256), 0, stream, qkv, rows, L, hidden, heads, Kc, Vc, len_stride,
                           rope, nullptr, kv_heads, 0);
    else if (starts)
        hipLaunchKernelGGL((llm_prefill_rope_kernel<true, false>), grid, dim3(256), 0, stream, qkv, rows, L, hidden, heads, Kc, Vc, len_stride,
                           rope, starts, heads, 0);
    else
        hipLaunchKernelGGL((llm_prefill_rope_kernel<false, false>), grid, dim3(256), 0, stream, qkv, rows, L, hidden, heads, Kc, Vc, len_stride,
                           rope, nullptr, heads, 0);
    return hipGetLastError();
}

hipError_t launch_prefill_attention(const half_t* qkv, int B, int L, int hidden, int heads, int kv_heads, const half_t* Kc, const half_t* Vc,
                                    int64_t len_stride, half_t* out, const int32_t* starts, hipStream_t stream) {
    if (B < 1 || L < 1 || L > len_stride || hidden != heads * HD || kv_heads < 1 || kv_heads > heads || heads % kv_heads || !qkv || !Kc ||
        !Vc || !out)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(B * heads), (unsigned)((L + AQ - 1) / AQ));
    const bool grouped = kv_heads != heads;
    if (grouped && starts)
        hipLaunchKernelGGL((llm_prefill_attn_kernel<true, true>), grid, dim3(256), 0, stream, qkv, L, hidden, heads, Kc, Vc, len_stride, out,
                           starts, kv_heads, 0);
    else if (grouped)
        hipLaunchKernelGGL((llm_prefill_attn_kernel<false, true>), grid, dim3(256), 0, stream, qkv, L, hidden, heads, Kc, Vc, len_stride, out,
                           nullptr, kv_heads, 0);
    else if (starts)
        hipLaunchKernelGGL((llm_prefill_attn_kernel<true, false>), grid, dim3(256), 0, stream, qkv, L, hidden, heads, Kc, Vc, len_stride, out,
                           starts, heads, 0);
    else
        hipLaunchKernelGGL((llm_prefill_attn_kernel<false, false>), grid, dim3(256), 0, stream, qkv, L, hidden, heads, Kc, Vc, len_stride, out,
                           nullptr, heads, 0);
    return hipGetLastError();
}

hipError_t launch_prefill_rope_from(half_t* qkv, int B, int pos0, int L, int hidden, int heads, int kv_heads, half_t* Kc, half_t* Vc,
                                    int64_t len_stride, const half_t* rope, const int32_t* starts, hipStream_t stream) {
    if (B < 1 || L < 1 || pos0 < 0 || (int64_t)pos0 + L > len_stride || hidden != heads * HD || kv_heads < 1 || kv_heads > heads ||
        heads % kv_heads || !qkv || !Kc || !Vc || !rope)
        return hipErrorInvalidValue;
    const int64_t rows = (int64_t)B * L, threads = rows * heads * 8;
    const dim3 grid((unsigned)((threads + 255) / 256));
    const bool grouped = kv_heads != heads;
    if (grouped && starts)
        hipLaunchKernelGGL((llm_prefill_rope_kernel<true, true, true>), grid, dim3(256), 0, stream, qkv, rows, L, hidden, heads, Kc, Vc,
                           len_stride, rope, starts, kv_heads, pos0);
    else if (grouped)
        hipLaunchKernelGGL((llm_prefill_rope_kernel<false, true, true>), grid, dim3(256), 0, stream, qkv, rows, L, hidden, heads, Kc, Vc,
                           len_stride, rope, nullptr, kv_heads, pos0);
    else if (starts)
        hipLaunchKernelGGL((llm_prefill_rope_kernel<true, false, true>), grid, dim3(256), 0, stream, qkv, rows, L, hidden, heads, Kc, Vc,
                           len_stride, rope, starts, heads, pos0);
    else
        hipLaunchKernelGGL((llm_prefill_rope_kernel<false, false, true>), grid, dim3(256), 0, stream, qkv, rows, L, hidden, heads, Kc, Vc,
                           len_stride, rope, nullptr, heads, pos0);
    return hipGetLastError();
}

hipError_t launch_prefill_attention_from(const half_t* qkv, int B, int pos0, int L, int hidden, int heads, int kv_heads, const half_t* Kc,
                                         const half_t* Vc, int64_t len_stride, half_t* out, const int32_t* starts, hipStream_t stream) {
    if (B < 1 || L < 1 || pos0 < 0 || (int64_t)pos0 + L > len_stride || hidden != heads * HD || kv_heads < 1 || kv_heads > heads ||
        heads % kv_heads || !qkv || !Kc || !Vc || !out)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(B * heads), (unsigned)((pos0 + L - 1) / AQ - pos0 / AQ + 1));      // blocks pos0 / 64 .. (pos0 + L - 1) / 64
    const bool grouped = kv_heads != heads;
    if (grouped && starts)
        hipLaunchKernelGGL((llm_prefill_attn_kernel<true, true, true>), grid, dim3(256), 0, stream, qkv, L, hidden, heads, Kc, Vc, len_stride,
                           out, starts, kv_heads, pos0);
    else if (grouped)
        hipLaunchKernelGGL((llm_prefill_attn_kernel<false, true, true>), grid, dim3(256), 0, stream, qkv, L, hidden, heads, Kc, Vc, len_stride,
                           out, nullptr, kv_heads, pos0);
    else if (starts)
        hipLaunchKernelGGL((llm_prefill_attn_kernel<true, false, true>), grid, dim3(256), 0, stream, qkv, L, hidden, heads, Kc, Vc, len_stride,
                           out, starts, heads, pos0);
    else
        hipLaunchKernelGGL((llm_prefill_attn_kernel<false, false, true>), grid, dim3(256), 0, stream, qkv, L, hidden, heads, Kc, Vc, len_stride,
                           out, nullptr, heads, pos0);
    return hipGetLastError();
}

hipError_t launch_kv_broadcast(const half_t* srcK, const half_t* srcV, int64_t src_stride, int P, int B, int kv_heads, const int32_t* starts,
                               half_t* dstK, half_t* dstV, int64_t dst_stride, hipStream_t stream) {
    if (B < 1 || kv_heads < 1 || P < 1 || P > src_stride || P > dst_stride || !srcK || !srcV || !dstK || !dstV) return hipErrorInvalidValue;
    const int64_t threads = (int64_t)B * kv_heads * P * 16;
    hipLaunchKernelGGL(llm_kv_broadcast_kernel, dim3((unsigned)((threads + 255) / 256), 2), dim3(256), 0, stream, srcK, srcV, src_stride, P, B,
                       kv_heads, starts, dstK, dstV, dst_stride);
    return hipGetLastError();
}

hipError_t launch_prefill_swiglu(const half_t* gu, int64_t rows, int mlp, half_t* act, hipStream_t stream) {
    if (rows < 1 || mlp < 16 || mlp % 16 || !gu || !act) return hipErrorInvalidValue;
    const int64_t threads = rows * (mlp / 8);
    hipLaunchKernelGGL(llm_prefill_swiglu_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, gu, rows, mlp, act);
    return hipGetLastError();
}

}  // namespace cgpt
