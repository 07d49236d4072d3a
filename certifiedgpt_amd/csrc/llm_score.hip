// llm_score.hip -- the kernels of the native answer scoring (cgpt_llm_score, include/cgpt.h): embedding gather of the answer
// tokens, rotary + attention of the "tail" rows over the shared prompt cache, label-smoothed cross-entropy over the vocabulary.
// The GEMMs and the row-wise kernels between them are the prefill's (llm_prefill.hip, launch_gemm); llm.hip strings the launches.
//
// Reference call replaced: `MiniGPTBase.multi_select` (minigpt_base.py:451-467), which runs `forward(..., reduction='none')` --
// one whole LlamaForCausalLM forward over prompt + answer and CrossEntropyLoss(label_smoothing=0.1) on `logits.float()`
// (modeling_llama.py:101-123) -- once per candidate.  Here the prompt is prefilled once (cgpt_llm_prefill) and all candidates are
// scored on its cache: candidate c contributes T_c - 1 tail rows (its tokens 0 .. T_c - 2 at rotary positions L ..), which attend
// over the prompt's cache rows and over the rotated keys of their own candidate's earlier tail rows.  Those keys and values live
// in LDS only: NO cache row is written.
// Rounding follows the token step (llm_step.hip: llm_attn_kernel): rotary products and their sum in fp16, scores, probabilities and
// sums in fp32.  Plain vector stores, no atomics, fixed summation orders: a (row, candidate) result depends on nothing but that
// row's prompt cache and that candidate's tokens -- not on the batch, not on the other candidates, not on the launch.
//
// Per-row prompts and candidates (cgpt_llm_score_ragged): every kernel has a RAGGED instantiation.  Row b is left-padded by start[b]
// positions (device array, clamped into 0 .. L-1 as the ragged prefill clamps it) and the attention works in row-relative coordinates:
// the head's cache pointers move by start[b], the chunk walk runs over len[b] = L - start[b] keys and tail row j is rotated at
// len[b] + j, so a padded row walks the keys of the row run alone in the same order.  The token table is [B, C, tmax] and a device
// array len[B, C] holds each row's real length of each candidate (clamped into 1 .. T_c); the geometry `ScoreCands` stays uniform over
// the rows, T_c being the longest length of candidate c.  A row shorter than T_c still runs its surplus tail rows (row-independent
// work on finite inputs: their tokens are read through clamp_token); the cross-entropy of a token j >= len[b, c] is written as 0 and
// the sum leaves it out.  The plain instantiations read neither array and compile to the code they were.
#include <math.h>

#include "llm.h"

namespace cgpt {

namespace {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
constexpr int HD = 128;
constexpr int KC = 64;                                       // prompt keys staged per chunk

__device__ __forceinline__ float rf16(float v) { return (float)(half_t)v; }
// fp16(a * b) as a value of its own (llm_step.hip: kept from contracting into a fused multiply-add, which would skip the rounding)
__device__ __forceinline__ float mul_f16(float a, float b) {
    float r = rf16(a * b);
    asm volatile("" : "+v"(r));
    return r;
}

// tail slot s (0 .. S-1) -> its candidate c and token index j: off[c] <= s < off[c + 1] (candidates of one token own no slot)
__device__ __forceinline__ void slot_of(const ScoreCands& t, int s, int& c, int& j) {
    c = 0;
    while (c + 1 < t.n && t.off[c + 1] <= s) ++c;
    j = s - t.off[c];
}

__device__ __forceinline__ long long clamp_token(long long tok, int vocab) { return (tok < 0 || tok >= vocab) ? 0 : tok; }

// h[r, :] = embed[token, :] for tail row r = b * S + s; one workgroup per row.
// RAGGED: row b = blockIdx.x / S reads its own slice of the table [B, C, tmax].
template <bool RAGGED>
__global__ __launch_bounds__(256) void llm_score_embed_kernel(const long long* __restrict__ cand_tokens, ScoreCands t,
                                                              const half_t* __restrict__ table, int vocab, int hidden,
                                                              half_t* __restrict__ h) {
    const int S = t.off[t.n];
    int c, j;
    slot_of(t, (int)(blockIdx.x % S), c, j);
    if (RAGGED) cand_tokens += (int64_t)(blockIdx.x / S) * t.n * t.tmax;
    const long long tok = clamp_token(cand_tokens[(int64_t)c * t.tmax + j], vocab);
    const h16x8* src = reinterpret_cast<const h16x8*>(table + tok * hidden);
    h16x8* dst = reinterpret_cast<h16x8*>(h + (int64_t)blockIdx.x * hidden);
    for (int i = threadIdx.x; i < hidden / 8; i += 256) dst[i] = src[i];
}

// Rotary + attention of the S tail rows of one (prompt row, head): one workgroup of four wavefronts.
//   setup     every tail row's q and k are rotated at position L + j (x cos + rotate_half(x) sin, products and sum in fp16) and kept
//             in LDS with its v: the tail's keys and values exist nowhere else
//   prompt    cache rows 0 .. L-1 of the head are staged ONCE, in chunks of 64 keys (K and V, 16-byte loads, 32 KiB), and every
//             query of the workgroup attends over the staged chunk: the S queries share one read of the prompt's K / V
//   tail      query (c, j) then attends over tail keys (c, 0 .. j) of its own candidate
// A wavefront owns queries wave, wave + 4, ...  Attending is llm_attn_kernel's arithmetic on at most 64 keys -- lane (kk, dc) takes
// keys 4 i + kk and dims dc .. dc + 7, fp32 dot products reduced over the 16 lanes of a key, then the maximum, then
// p = exp(score - max) and p . V -- combined across chunks by the usual rescaling (m, l, acc) <- (max, l e^(m - max) + sum p,
// acc e^(m - max) + sum p v).  The state of a query sits in LDS between chunks; every lane reads back only addresses it wrote
// itself (lanes that share a dim group hold equal values after the butterflies), so no barrier inside a wavefront is needed.
// The chunk grid depends on L alone and the tail walk on (c, j) alone: a query's key order is fixed by (L, candidate, j).
// GROUPED (grouped-query attention): query head h reads K/V head kh = h / (heads / kv_heads) -- of the
// [B, kv_heads, len_stride, 128] cache, and of the tail rows' k / v in a projection row hidden + 2 kv_heads 128 wide.  The G heads of a
// group do not share a staged chunk here.  The plain instantiation never reads kv_heads.
// RAGGED (left-padded rows): s = start[b] clamped into 0 .. L-1; the head's K / V pointers move by s (s * 128 halfs: the 16-byte loads
// stay aligned) and L stands for len = L - s below -- the chunk walk covers the row's len real keys from its first one, tail row j
// is rotated at len + j.  The chunk grid and the key order of a row depend on len alone; cache rows below s are never read.  LDS use
// depends on S only.  The plain instantiation never reads starts.
template <bool GROUPED, bool RAGGED>
__global__ __launch_bounds__(256) void llm_score_attn_kernel(const half_t* __restrict__ qkv, ScoreCands t, int L, int hidden, int heads,
                                                             const half_t* __restrict__ Kc, const half_t* __restrict__ Vc,
                                                             int64_t len_stride, const half_t* __restrict__ rope,
                                                             half_t* __restrict__ out, int kv_heads, const int* __restrict__ starts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int S = t.off[t.n];
    half_t* ks = reinterpret_cast<half_t*>(smem);             // [KC][128] staged prompt keys
    half_t* vs = ks + KC * HD;                                // [KC][128] staged prompt values
    half_t* tk = vs + KC * HD;                                // [S][128] rotated tail keys
    half_t* tv = tk + S * HD;                                 // [S][128] tail values
    half_t* tq = tv + S * HD;                                 // [S][128] rotated tail queries
    float* acc = reinterpret_cast<float*>(tq + S * HD);       // [S][128] running sum of p v
    float* ml = acc + S * HD;                                 // [S][2]   running maximum, running sum of p
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row0 = (int64_t)b * S;
    const int kh = GROUPED ? h / (heads / kv_heads) : h;
    const int64_t ldq = GROUPED ? hidden + 2 * kv_heads * HD : 3 * hidden;
    const half_t* Kh = Kc + (int64_t)(b * (GROUPED ? kv_heads : heads) + kh) * len_stride * HD;
    const half_t* Vh = Vc + (int64_t)(b * (GROUPED ? kv_heads : heads) + kh) * len_stride * HD;
    if (RAGGED) {
        const int s0 = min(max(starts[b], 0), L - 1);
        Kh += (int64_t)s0 * HD;
        Vh += (int64_t)s0 * HD;
        L -= s0;
    }

    for (int i = tid; i < S * 64; i += 256) {                 // thread (s, p) owns the rotary pair (p, p + 64) of tail row s
        const int s = i >> 6, p = i & 63;
        int c, j;
        slot_of(t, s, c, j);
        const half_t* q = qkv + (row0 + s) * ldq + h * HD;
        const half_t* k = qkv + (row0 + s) * ldq + hidden + kh * HD;
        const half_t* v = k + (GROUPED ? kv_heads * HD : hidden);
        const half_t* rp = rope + (int64_t)(L + j) * HD;
        const float cs = (float)rp[p], sn = (float)rp[64 + p];
        const float q0 = (float)q[p], q1 = (float)q[p + 64], k0 = (float)k[p], k1 = (float)k[p + 64];
        tq[s * HD + p] = (half_t)(mul_f16(q0, cs) - mul_f16(q1, sn));
        tq[s * HD + p + 64] = (half_t)(mul_f16(q1, cs) + mul_f16(q0, sn));
        tk[s * HD + p] = (half_t)(mul_f16(k0, cs) - mul_f16(k1, sn));
        tk[s * HD + p + 64] = (half_t)(mul_f16(k1, cs) + mul_f16(k0, sn));
        tv[s * HD + p] = v[p];
        tv[s * HD + p + 64] = v[p + 64];
    }
    for (int i = tid; i < S * HD; i += 256) acc[i] = 0.0f;
    for (int i = tid; i < S; i += 256) {
        ml[2 * i] = -INFINITY;
        ml[2 * i + 1] = 0.0f;
    }

    const int kk = lane >> 4, dc = (lane & 15) * 8;           // key within a group of 4, first of the lane's 8 dims
    const float scale = 0.08838834764831845f;                 // 1 / sqrt(128)
    // query s attends over keys 0 .. nk-1 (1 <= nk <= 64) of `keys` / `vals` ([nk][128] in LDS) and updates its state
    auto attend = [&](int s, const half_t* keys, const half_t* vals, int nk) {
        float qr[8];
        {
            const h16x8 qv = *reinterpret_cast<const h16x8*>(tq + s * HD + dc);
#pragma unroll
            for (int e = 0; e < 8; ++e) qr[e] = (float)qv[e];
        }
        float d[KC / 4];
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < KC / 4; ++i) {
            d[i] = -INFINITY;
            if (4 * i < nk) {                                 // wave-uniform
                const int key = 4 * i + kk;
                float x = 0.0f;
                if (key < nk) {
                    const h16x8 kv = *reinterpret_cast<const h16x8*>(keys + key * HD + dc);
#pragma unroll
                    for (int e = 0; e < 8; ++e) x += qr[e] * (float)kv[e];
                }
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) x += __shfl_xor(x, o);
                if (key < nk) {
                    d[i] = x * scale;
                    mx = fmaxf(mx, d[i]);
                }
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_old = ml[2 * s], l_old = ml[2 * s + 1];
        const float m_new = fmaxf(m_old, mx);                 // finite: key 0 of every walk exists
        const float alpha = expf(m_old - m_new);              // 0 on the first walk (m_old = -inf)
        float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float l = 0.0f;
#pragma unroll
        for (int i = 0; i < KC / 4; ++i) {
            const int key = 4 * i + kk;
            if (key < nk) {
                const float p = expf(d[i] - m_new);
                const h16x8 vv = *reinterpret_cast<const h16x8*>(vals + key * HD + dc);
                l += p;
#pragma unroll
                for (int e = 0; e < 8; ++e) a[e] += p * (float)vv[e];
            }
        }
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            a[e] += __shfl_xor(a[e], 16);
            a[e] += __shfl_xor(a[e], 32);
        }
        // the four lanes of a dim group hold equal values: each writes, and later reads back, the same words
        ml[2 * s] = m_new;
        ml[2 * s + 1] = l_old * alpha + l;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[s * HD + dc + e] = acc[s * HD + dc + e] * alpha + a[e];
    };

    for (int k0 = 0; k0 < L; k0 += KC) {
        __syncthreads();                                      // set-up done / the previous chunk has been read by every wave
        const int nk = min(KC, L - k0);
        for (int i = tid; i < nk * 16; i += 256) {            // nk keys x 16 chunks of 16 bytes, K and V
            const int key = i >> 4, d8 = (i & 15) * 8;
            *reinterpret_cast<h16x8*>(ks + key * HD + d8) = *reinterpret_cast<const h16x8*>(Kh + (int64_t)(k0 + key) * HD + d8);
            *reinterpret_cast<h16x8*>(vs + key * HD + d8) = *reinterpret_cast<const h16x8*>(Vh + (int64_t)(k0 + key) * HD + d8);
        }
        __syncthreads();
        for (int s = wave; s < S; s += 4) attend(s, ks, vs, nk);
    }
    for (int s = wave; s < S; s += 4) {                       // the query's own candidate: tail keys (c, 0 .. j); j < 64 as S <= 64
        int c, j;
        slot_of(t, s, c, j);
        attend(s, tk + t.off[c] * HD, tv + t.off[c] * HD, j + 1);
        if (kk == 0) {
            const float l = ml[2 * s + 1];
            h16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (half_t)(acc[s * HD + dc + e] / l);
            *reinterpret_cast<h16x8*>(out + (row0 + s) * hidden + h * HD + dc) = o;
        }
    }
}

__device__ __forceinline__ void load8(const float* p, float* v) {
    const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void load8(const half_t* p, float* v) {
    const h16x8 a = *reinterpret_cast<const h16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)a[e];
}

// sum over the workgroup in a fixed order: wave butterfly, then the four wave sums in order (llm_rmsnorm_kernel's reduction)
__device__ __forceinline__ float block_sum(float v, float* wsum) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                                          // wsum may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// CrossEntropyLoss(label_smoothing = eps) of ONE logits row z (fp32 values; fp16 logits are widened first, as HF's `.float()`)
// against one target:  ce = lse(z) - (1 - eps) z[target] - eps mean(z),  lse = max + log(sum exp(z - max)).  One workgroup per
// row, two passes over it (the second one hits L2), all statistics in fp32, per-thread strided sums combined by block_sum.
//   FIRST: workgroup (b, c) reads the fp32 row b and scores token 0 of candidate c
//   else:  workgroup i reads fp16 row i of `logits`, which is tail row row0 + i = (b, c, j), and scores token j + 1
// RAGGED: the token comes from row b's slice of the table [B, C, tmax]; a token at or past the row's own length of the candidate
// (cand_lens[b, c] clamped into 1 .. T_c) has its slot written as 0 and nothing else done -- uniform over the workgroup.
template <typename T, bool FIRST, bool RAGGED>
__global__ __launch_bounds__(256) void llm_score_ce_kernel(const T* __restrict__ logits, int vocab,
                                                           const long long* __restrict__ cand_tokens, ScoreCands t, int64_t row0,
                                                           float eps, float* __restrict__ ce, const int* __restrict__ cand_lens) {
    __shared__ float wsum[4];
    const int S = t.off[t.n];
    int64_t b, src;
    int c, j;
    if (FIRST) {
        b = blockIdx.x / t.n;
        c = (int)(blockIdx.x % t.n);
        j = 0;
        src = b;
    } else {
        const int64_t r = row0 + blockIdx.x;
        b = r / S;
        slot_of(t, (int)(r % S), c, j);
        j += 1;
        src = blockIdx.x;
    }
    if (RAGGED) {
        const int Tc = t.off[c + 1] - t.off[c] + 1;
        if (j >= min(max(cand_lens[b * t.n + c], 1), Tc)) {
            if (threadIdx.x == 0) ce[b * (S + t.n) + t.off[c] + c + j] = 0.0f;
            return;
        }
        cand_tokens += b * t.n * t.tmax;
    }
    const T* z = logits + src * vocab;
    float mx = -INFINITY, sz = 0.0f;
    for (int i = threadIdx.x; i < vocab / 8; i += 256) {
        float v[8];
        load8(z + 8 * i, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            mx = fmaxf(mx, v[e]);
            sz += v[e];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(wsum[0], wsum[1]), fmaxf(wsum[2], wsum[3]));
    sz = block_sum(sz, wsum);
    float se = 0.0f;
    for (int i = threadIdx.x; i < vocab / 8; i += 256) {
        float v[8];
        load8(z + 8 * i, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) se += expf(v[e] - mx);
    }
    se = block_sum(se, wsum);
    if (threadIdx.x == 0) {
        const long long tok = clamp_token(cand_tokens[(int64_t)c * t.tmax + j], vocab);
        const float zt = (float)z[tok];
        const float lse = mx + logf(se);
        ce[b * (S + t.n) + t.off[c] + c + j] = (lse - (1.0f - eps) * zt) - eps * (sz / (float)vocab);
    }
}

// out[b, c] = the candidate's per-token values added in token order; one thread per (b, c).  RAGGED: the row's own tokens only.
template <bool RAGGED>
__global__ __launch_bounds__(256) void llm_score_sum_kernel(const float* __restrict__ ce, ScoreCands t, int B, float* __restrict__ out,
                                                            const int* __restrict__ cand_lens) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= B * t.n) return;
    const int b = id / t.n, c = id % t.n;
    int T = t.off[c + 1] - t.off[c] + 1;
    if (RAGGED) T = min(max(cand_lens[id], 1), T);
    const float* src = ce + (int64_t)b * (t.off[t.n] + t.n) + t.off[c] + c;
    float s = 0.0f;
    for (int j = 0; j < T; ++j) s += src[j];
    out[id] = s;
}

size_t attn_lds_bytes(int S) { return (size_t)2 * KC * HD * sizeof(half_t) + (size_t)S * (3 * HD * sizeof(half_t) + HD * sizeof(float) + 2 * sizeof(float)); }

bool cands_ok(const ScoreCands& t) {
    if (t.n < 1 || t.n > SCORE_MAX_CANDS || t.tmax < 1 || t.off[0] != 0) return false;
    for (int c = 0; c < t.n; ++c)
        if (t.off[c + 1] < t.off[c] || t.off[c + 1] - t.off[c] + 1 > t.tmax) return false;
    return t.off[t.n] <= SCORE_MAX_TAIL;
}

}  // namespace

hipError_t score_prepare() {
    const void* kernels[4] = {reinterpret_cast<const void*>(llm_score_attn_kernel<false, false>),
                              reinterpret_cast<const void*>(llm_score_attn_kernel<true, false>),
                              reinterpret_cast<const void*>(llm_score_attn_kernel<false, true>),
                              reinterpret_cast<const void*>(llm_score_attn_kernel<true, true>)};
    for (const void* k : kernels) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attn_lds_bytes(SCORE_MAX_TAIL));
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_score_embed(const long long* cand_tokens, const ScoreCands& t, int B, const half_t* table, int vocab, int hidden,
                              half_t* h, hipStream_t stream, bool per_row) {
    if (!cands_ok(t) || t.off[t.n] < 1 || B < 1 || hidden < 8 || hidden % 8 || !cand_tokens || !table || !h) return hipErrorInvalidValue;
    if (per_row)
        hipLaunchKernelGGL(llm_score_embed_kernel<true>, dim3((unsigned)(B * t.off[t.n])), dim3(256), 0, stream, cand_tokens, t, table, vocab,
                           hidden, h);
    else
        hipLaunchKernelGGL(llm_score_embed_kernel<false>, dim3((unsigned)(B * t.off[t.n])), dim3(256), 0, stream, cand_tokens, t, table, vocab,
                           hidden, h);
    return hipGetLastError();
}

template <bool GROUPED, bool RAGGED>
static void score_attn_launch(const half_t* qkv, const ScoreCands& t, int B, int L, int hidden, int heads, int kv_heads, const half_t* Kc,
                              const half_t* Vc, int64_t len_stride, const half_t* rope, half_t* out, const int32_t* starts, hipStream_t stream) {
    hipLaunchKernelGGL((llm_score_attn_kernel<GROUPED, RAGGED>), dim3((unsigned)(B * heads)), dim3(256), attn_lds_bytes(t.off[t.n]), stream, qkv,
                       t, L, hidden, heads, Kc, Vc, len_stride, rope, out, kv_heads, starts);
}

hipError_t launch_score_attention(const half_t* qkv, const ScoreCands& t, int B, int L, int hidden, int heads, int kv_heads, const half_t* Kc,
                                  const half_t* Vc, int64_t len_stride, const half_t* rope, half_t* out, hipStream_t stream,
                                  const int32_t* starts) {
    if (!cands_ok(t) || t.off[t.n] < 1 || B < 1 || L < 1 || L > len_stride || hidden != heads * HD || kv_heads < 1 || kv_heads > heads ||
        heads % kv_heads || !qkv || !Kc || !Vc || !rope || !out)
        return hipErrorInvalidValue;
    const bool grouped = kv_heads != heads;
    if (grouped && starts)
        score_attn_launch<true, true>(qkv, t, B, L, hidden, heads, kv_heads, Kc, Vc, len_stride, rope, out, starts, stream);
    else if (grouped)
        score_attn_launch<true, false>(qkv, t, B, L, hidden, heads, kv_heads, Kc, Vc, len_stride, rope, out, nullptr, stream);
    else if (starts)
        score_attn_launch<false, true>(qkv, t, B, L, hidden, heads, heads, Kc, Vc, len_stride, rope, out, starts, stream);
    else
        score_attn_launch<false, false>(qkv, t, B, L, hidden, heads, heads, Kc, Vc, len_stride, rope, out, nullptr, stream);
    return hipGetLastError();
}

hipError_t launch_score_ce_first(const float* first_logits, int vocab, const long long* cand_tokens, const ScoreCands& t, int B,
                                 float smoothing, float* ce, hipStream_t stream, const int32_t* row_lens) {
    if (!cands_ok(t) || B < 1 || vocab < 8 || vocab % 8 || !first_logits || !cand_tokens || !ce) return hipErrorInvalidValue;
    if (row_lens)
        hipLaunchKernelGGL((llm_score_ce_kernel<float, true, true>), dim3((unsigned)(B * t.n)), dim3(256), 0, stream, first_logits, vocab,
                           cand_tokens, t, (int64_t)0, smoothing, ce, row_lens);
    else
        hipLaunchKernelGGL((llm_score_ce_kernel<float, true, false>), dim3((unsigned)(B * t.n)), dim3(256), 0, stream, first_logits, vocab,
                           cand_tokens, t, (int64_t)0, smoothing, ce, row_lens);
    return hipGetLastError();
}

hipError_t launch_score_ce_tail(const half_t* logits, int vocab, const long long* cand_tokens, const ScoreCands& t, int64_t row0,
                                int64_t rows, float smoothing, float* ce, hipStream_t stream, const int32_t* row_lens) {
    if (!cands_ok(t) || t.off[t.n] < 1 || rows < 1 || row0 < 0 || vocab < 8 || vocab % 8 || !logits || !cand_tokens || !ce)
        return hipErrorInvalidValue;
    if (row_lens)
        hipLaunchKernelGGL((llm_score_ce_kernel<half_t, false, true>), dim3((unsigned)rows), dim3(256), 0, stream, logits, vocab, cand_tokens, t,
                           row0, smoothing, ce, row_lens);
    else
        hipLaunchKernelGGL((llm_score_ce_kernel<half_t, false, false>), dim3((unsigned)rows), dim3(256), 0, stream, logits, vocab, cand_tokens, t,
                           row0, smoothing, ce, row_lens);
    return hipGetLastError();
}

hipError_t launch_score_sum(const float* ce, const ScoreCands& t, int B, float* out, hipStream_t stream, const int32_t* row_lens) {
    if (!cands_ok(t) || B < 1 || !ce || !out) return hipErrorInvalidValue;
    if (row_lens)
        hipLaunchKernelGGL(llm_score_sum_kernel<true>, dim3((unsigned)((B * t.n + 255) / 256)), dim3(256), 0, stream, ce, t, B, out, row_lens);
    else
        hipLaunchKernelGGL(llm_score_sum_kernel<false>, dim3((unsigned)((B * t.n + 255) / 256)), dim3(256), 0, stream, ce, t, B, out, row_lens);
    return hipGetLastError();
}

}  // namespace cgpt
