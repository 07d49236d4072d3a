// llm_beam.hip -- beam search on the native LLaMA engine (beams="hip"; include/cgpt.h: "Beam search").
//
// Reference call replaced: HF `generate(num_beams=k, length_penalty=..., do_sample=False, early_stopping=False)` -- transformers 5.x
// `_beam_search`, a fixed-shape tensor algorithm -- as MiniGPT-4's demo calls it with its first slider.  The law is stated once in
// llm_laws.py (`beam_step_law`).  Two kernels:
//
// llm_attn_beam_kernel: the token step's rotary + K/V append + one-query attention (llm_attn_kernel in llm_step.hip) for beam rows.  The k
// beams of an image share its prompt, so the prompt cache holds ONE row per image; what the beams generate lives in a beam cache of
// generated positions only, and HF's physical `reorder_cache` is an ancestry table: key s < t of beam row r is read from beam row
// anc[r][s].  No K/V byte moves.  The arithmetic and the key order are llm_attn_kernel's (groups of four keys from key 0, fp32 dot
// products with the 16-lane butterfly, the maximum, expf(sc - mx) and acc += p * v in key order, the same final shuffles): the
// indirection changes where a byte comes from, never the order of a sum, so a row gives the bits llm_attn_kernel gives on the
// physically gathered cache.
//
// llm_beam_select_kernel: law steps 1-7 in the slot of llm_select_kernel, one workgroup of 256 threads per image.
// Rounding sequence of a candidate score (what tests/test_gpu_llm_beam.py derives its margin from):
//   lse_j = m_j + log(S_j) in float64, m_j = the row's fp32 maximum (exact), S_j = sum_v exp((double)l[j, v] - m_j) in float64
//   lp    = fp32((double)l[j, v] - lse_j)            ONE fp32 rounding          (EOS columns: -inf while mask_eos)
//   c     = running[j] + lp in fp32                  ONE fp32 rounding          (running: the fp32 state the select before wrote)
//   a pool entrant's score = c / divisor in fp32     ONE more (IEEE division); divisor = fp32((i + 1) ** length_penalty), formed on
//   the host in float64 (1 for a penalty of 0, the integer i + 1 for a penalty of 1), so the kernel evaluates no power.
//   Step 7 divides running'[0] the same way.  Comparisons are exact on these fp32 values; ties go to the lowest flat index j V + v.
// Summation order of S_j, fixed, so that replays are bit-identical: thread t adds its columns t, t + 256, t + 512, ... in ascending
// order; the 64 partials of a wave are added by the xor butterfly 32, 16, 8, 4, 2, 1; the four wave sums are added as
// ((w0 + w1) + w2) + w3.  Against the float64 law this leaves about 1e-15 relative in lse: nothing beside the fp32 roundings above.
// The top K: K rounds of a block-wide first-maximum in the order (value descending, flat index ascending).  A thread holds the first
// maximum of its own candidates (scores re-formed from the logits, re-read from L2) that come after its last pick; a round reduces
// the 256 and only the owner of the pick scans its candidates again.  Nothing is marked and no row is held in LDS: any vocabulary up
// to 131 072 works.
// One thread then does the serial part on K <= 72 candidates (finished flags, the next k beams, the pool merge, `open`); all threads
// copy the token, ancestry and pool rows, gathered by parent from the state BEFORE into the state AFTER (two buffers, never in place).
// Plain vector loads and stores only; nothing is atomic.
#include <math.h>

#include <string>

#include "../../include/cgpt.h"
#include "common_host.h"
#include "llm_beam.h"

using namespace cgpt;

namespace {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
constexpr int HD = 128;
constexpr float NEG = -1.0e9f;

__device__ __forceinline__ float rf16(float v) { return (float)(half_t)v; }
// fp16(a * b) as a value of its own (see llm_step.hip: the compiler must not contract it into an fma)
__device__ __forceinline__ float mul_f16(float a, float b) {
    float r = rf16(a * b);
    asm volatile("" : "+v"(r));
    return r;
}

// One wavefront per (beam row, head).  Row r belongs to image b = r / k.  Key index t over 0 .. pos, pos = L + tg:
//   t < L          prompt cache row t of image b           L <= t < pos    beam cache row t - L of beam row anc[r][t - L]
//   t == pos       the row's own new key / value, from LDS (also stored to beam cache row tg of row r, the only row written)
__global__ __launch_bounds__(64) void llm_attn_beam_kernel(BeamAttnArgs a) {
    extern __shared__ float asmem[];                   // [128] rotated query, [128 + 128] halfs: the new key and value, [pos + 1] scores
    float* qs = asmem;
    half_t* knew = reinterpret_cast<half_t*>(asmem + HD);
    half_t* vnew = knew + HD;
    float* sc = asmem + 2 * HD;
    const int r = blockIdx.x / a.heads, h = blockIdx.x % a.heads, lane = threadIdx.x;
    const int b = r / a.k;
    const int hidden = a.hidden, L = a.L, pos = a.L + a.t;
    const half_t* q = a.qkv + (int64_t)r * 3 * hidden + h * HD;
    const half_t* k = q + hidden;
    const half_t* v = k + hidden;
    const half_t* Kph = a.Kp + (int64_t)(b * a.heads + h) * a.prompt_stride * HD;
    const half_t* Vph = a.Vp + (int64_t)(b * a.heads + h) * a.prompt_stride * HD;
    const int32_t* anc = a.anc + (int64_t)r * a.ld_anc;

    {   // lane i owns the rotary pair (i, i + 64)
        const float c = (float)a.rope[(int64_t)pos * HD + lane], s = (float)a.rope[(int64_t)pos * HD + 64 + lane];
        const float q0 = (float)q[lane], q1 = (float)q[lane + 64], k0 = (float)k[lane], k1 = (float)k[lane + 64];
        qs[lane] = rf16(mul_f16(q0, c) - mul_f16(q1, s));
        qs[lane + 64] = rf16(mul_f16(q1, c) + mul_f16(q0, s));
        const half_t r0 = (half_t)(mul_f16(k0, c) - mul_f16(k1, s)), r1 = (half_t)(mul_f16(k1, c) + mul_f16(k0, s));
        const half_t v0 = v[lane], v1 = v[lane + 64];
        half_t* Kw = a.Kb + ((int64_t)(r * a.heads + h) * a.beam_stride + a.t) * HD;
        half_t* Vw = a.Vb + ((int64_t)(r * a.heads + h) * a.beam_stride + a.t) * HD;
        Kw[lane] = knew[lane] = r0;
        Kw[lane + 64] = knew[lane + 64] = r1;
        Vw[lane] = vnew[lane] = v0;
        Vw[lane + 64] = vnew[lane + 64] = v1;
    }
    __syncthreads();                                   // key `pos` is attended from LDS: the cache row just stored is not read back

    const int n = pos + 1;
    const int kk = lane >> 4, dc = (lane & 15) * 8;    // key within a group of 4, first of the lane's 8 dims
    // where key t < pos lives: the offset of its 128-vector in the prompt cache (t < L) or in the beam cache
    auto beam_off = [&](int t) {
        const int s = t - L;
        const int src = min(max(anc[s], 0), a.rows - 1);
        return ((int64_t)(src * a.heads + h) * a.beam_stride + s) * HD;
    };
    float qr[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) qr[e] = qs[dc + e];
    const float scale = 0.08838834764831845f;          // 1 / sqrt(128)
    float mx = -INFINITY;
    for (int t0 = 0; t0 < n; t0 += 4) {
        const int t = t0 + kk;
        float d = 0.0f;
        if (t < n) {
            const h16x8 kv = *reinterpret_cast<const h16x8*>(t == pos ? knew + dc : t < L ? Kph + (int64_t)t * HD + dc : a.Kb + beam_off(t) + dc);
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
            const h16x8 vv = *reinterpret_cast<const h16x8*>(t == pos ? vnew + dc : t < L ? Vph + (int64_t)t * HD + dc : a.Vb + beam_off(t) + dc);
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
        *reinterpret_cast<h16x8*>(a.out + (int64_t)r * hidden + h * HD + dc) = o;
    }
}

__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double t = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return t;
}
__device__ __forceinline__ float block_max(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float t = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    return t;
}
// does candidate (v, i) come before (w, j) in the order (value descending, flat index ascending)?
__device__ __forceinline__ bool before(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

__global__ __launch_bounds__(256) void llm_beam_select_kernel(BeamSelectArgs a) {
    __shared__ double lse[BEAM_MAX];
    __shared__ float run[BEAM_MAX];
    __shared__ double redd[4];
    __shared__ float redf[4];
    __shared__ float bv[4];
    __shared__ int bi[4];
    __shared__ float cval[BEAM_MAX_KEEP];
    __shared__ int cidx[BEAM_MAX_KEEP];
    __shared__ int s_parent[BEAM_MAX], s_tok[BEAM_MAX];    // the new beams: parent (local) and token
    __shared__ int s_pool[BEAM_MAX];                       // the new pool slots: old slot j (< k) or k + rank of an entrant
    const int b = blockIdx.x, tid = threadIdx.x;
    const int k = a.k, V = a.vocab, K = a.keep, n = a.n, i = a.step;
    const int row0 = b * k;

    // ---- step 1: the normaliser of every beam row, float64, fixed order (file header)
    for (int j = 0; j < k; ++j) {
        const float* s = a.src + (int64_t)(a.shared ? b : row0 + j) * a.lds;
        float m = -INFINITY;
        for (int v = tid; v < V; v += 256) m = fmaxf(m, s[v]);
        m = block_max(m, redf);
        double sum = 0.0;
        for (int v = tid; v < V; v += 256) sum += exp((double)s[v] - (double)m);
        sum = block_sum(sum, redd);
        if (tid == 0) {
            lse[j] = (double)m + log(sum);
            run[j] = a.first ? (j == 0 ? 0.0f : NEG) : a.in.running[row0 + j];
        }
    }
    __syncthreads();

    // ---- steps 2-3: K rounds of the first maximum among the candidates after the previous pick
    auto score = [&](int j, int v) {
        if (a.mask_eos)
            for (int e = 0; e < a.eos.n; ++e)
                if (a.eos.id[e] == v) return -INFINITY;
        const float lp = (float)((double)a.src[(int64_t)(a.shared ? b : row0 + j) * a.lds + v] - lse[j]);
        return run[j] + lp;
    };
    // Every thread keeps the first maximum among ITS candidates (columns tid, tid + 256, ... of every beam row) that come after its
    // own last pick; a round takes the first maximum of the 256 and only the thread that owned it scans its candidates again.  A
    // thread's candidate between its last pick and the round's pick would have won an earlier round, so each round's pick is the first
    // maximum among everything not yet picked: the order a full rescan per round gives, at one scan plus K partial ones.
    auto scan = [&](float tv, int ti, float& best, int& idx) {
        best = -INFINITY;
        idx = 0x7fffffff;
        for (int j = 0; j < k; ++j)
            for (int v = tid; v < V; v += 256) {
                const float c = score(j, v);
                const int f = j * V + v;
                if (!before(tv, ti, c, f)) continue;                       // picked in an earlier round (or NaN)
                if (idx == 0x7fffffff || before(c, f, best, idx)) { best = c; idx = f; }
            }
    };
    float best;
    int idx;
    scan(INFINITY, -1, best, idx);
    for (int r = 0; r < K; ++r) {
        float wb = best;
        int wi = idx;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(wb, o);
            const int oi = __shfl_xor(wi, o);
            if (oi != 0x7fffffff && (wi == 0x7fffffff || before(ov, oi, wb, wi))) { wb = ov; wi = oi; }
        }
        if ((tid & 63) == 0) { bv[tid >> 6] = wb; bi[tid >> 6] = wi; }
        __syncthreads();
        wb = bv[0]; wi = bi[0];
        for (int w = 1; w < 4; ++w)
            if (bi[w] != 0x7fffffff && (wi == 0x7fffffff || before(bv[w], bi[w], wb, wi))) { wb = bv[w]; wi = bi[w]; }
        const bool none = wi == 0x7fffffff;                                // fewer than K comparable values (NaN logits): stay in bounds
        if (tid == 0) { cval[r] = none ? -INFINITY : wb; cidx[r] = none ? 0 : wi; }
        if (!none && wi == idx) scan(wb, wi, best, idx);                   // the owner moves on to its next candidate
        __syncthreads();
    }

    // ---- steps 4-7, one thread
    const BeamState& in = a.in;
    const BeamState& out = a.out;
    if (tid == 0) {
        const bool last = i == n - 1;
        bool fin[BEAM_MAX_KEEP];
        for (int r = 0; r < K; ++r) {
            const long long tok = cidx[r] % V;
            bool f = last;
            for (int e = 0; e < a.eos.n; ++e) f = f || a.eos.id[e] == tok;
            fin[r] = f;
        }
        int q = 0;                                                         // step 5: (fin ascending, rank ascending)
        for (int pass = 0; pass < 2 && q < k; ++pass)
            for (int r = 0; r < K && q < k; ++r)
                if (fin[r] == (pass == 1)) {
                    out.running[row0 + q] = cval[r];
                    s_parent[q] = cidx[r] / V;
                    s_tok[q] = cidx[r] % V;
                    ++q;
                }
        const float run0 = out.running[row0];
        const int was_open = a.first ? 1 : in.open[b];
        float ps[BEAM_MAX];
        int pf[BEAM_MAX], pl[BEAM_MAX];
        for (int j = 0; j < k; ++j) {
            ps[j] = a.first ? NEG : in.pool_score[row0 + j];
            pf[j] = a.first ? 0 : in.pool_fin[row0 + j];
            pl[j] = a.first ? 0 : in.pool_len[row0 + j];
        }
        float ns[BEAM_MAX];
        int nf[BEAM_MAX], nl[BEAM_MAX];
        if (was_open) {                                                    // step 6: old slots first, then the entrants by rank
            float ms[2 * BEAM_MAX];
            int mc[2 * BEAM_MAX], cnt = k;
            for (int j = 0; j < k; ++j) { ms[j] = ps[j]; mc[j] = j; }
            for (int r = 0; r < k; ++r)
                if (fin[r]) { ms[cnt] = __fdiv_rn(cval[r], a.divisor); mc[cnt] = k + r; ++cnt; }
            bool used[2 * BEAM_MAX];
            for (int m = 0; m < cnt; ++m) used[m] = false;
            for (int s = 0; s < k; ++s) {
                int pick = -1;
                for (int m = 0; m < cnt; ++m)
                    if (!used[m] && (pick < 0 || ms[m] > ms[pick])) pick = m;      // strict: the first of equal scores stays
                used[pick] = true;
                ns[s] = ms[pick];
                s_pool[s] = mc[pick];
                if (mc[pick] < k) { nf[s] = pf[mc[pick]]; nl[s] = pl[mc[pick]]; }
                else { nf[s] = 1; nl[s] = i + 1; }
            }
        } else {
            for (int j = 0; j < k; ++j) { ns[j] = ps[j]; nf[j] = pf[j]; nl[j] = pl[j]; s_pool[j] = j; }
        }
        bool all = true;
        float worst = INFINITY;
        for (int j = 0; j < k; ++j) {
            out.pool_score[row0 + j] = ns[j];
            out.pool_fin[row0 + j] = nf[j];
            out.pool_len[row0 + j] = nl[j];
            all = all && nf[j] != 0;
            worst = fminf(worst, ns[j]);
        }
        if (!all) worst = NEG;
        const int open = (was_open && __fdiv_rn(run0, a.divisor) > worst) ? 1 : 0;   // step 7
        out.open[b] = open;
        for (int j = 0; j < k; ++j) {
            a.next_tok[row0 + j] = s_tok[j];
            a.parents[row0 + j] = s_parent[j];
        }
        if (a.scores_out) a.scores_out[b] = ns[0];
        if (a.trace) {
            float* t = a.trace + (int64_t)b * (5 * k + 1);
            for (int j = 0; j < k; ++j) {
                t[j] = out.running[row0 + j];
                t[k + j] = (float)s_parent[j];
                t[2 * k + j] = (float)s_tok[j];
                t[3 * k + j] = ns[j];
                t[4 * k + j] = (float)nf[j];
            }
            t[5 * k] = (float)open;
        }
    }
    __syncthreads();

    // ---- the rows, gathered by parent from the state before: column c < i from the parent, column i the new token, pad behind
    for (int e = tid; e < k * n; e += 256) {
        const int j = e / n, c = e % n;
        const int par = row0 + s_parent[j];
        out.tokens[(int64_t)(row0 + j) * n + c] = c < i ? in.tokens[(int64_t)par * n + c] : c == i ? (long long)s_tok[j] : a.pad;
        out.anc[(int64_t)(row0 + j) * n + c] = c < i ? in.anc[(int64_t)par * n + c] : row0 + j;
        long long ptok;
        const int src = s_pool[j];
        if (src < k) ptok = a.first ? a.pad : in.pool_seq[(int64_t)(row0 + src) * n + c];
        else {                                                             // an entrant: rank src - k, whose parent is cidx / V
            const int rp = row0 + cidx[src - k] / V;
            ptok = c < i ? in.tokens[(int64_t)rp * n + c] : c == i ? (long long)(cidx[src - k] % V) : a.pad;
        }
        out.pool_seq[(int64_t)(row0 + j) * n + c] = ptok;
        if (j == 0 && a.tokens_out) a.tokens_out[(int64_t)b * n + c] = ptok;
    }
}

// dst[r, 0 .. cols) = src[r / k, 0 .. cols): an image's prefill logits for each of its k beam rows
__global__ __launch_bounds__(256) void llm_beam_spread_kernel(const float* __restrict__ src, int64_t lds, float* __restrict__ dst, int64_t ldd,
                                                              int cols, int k) {
    const float* s = src + (int64_t)(blockIdx.x / k) * lds;
    float* d = dst + (int64_t)blockIdx.x * ldd;
    for (int j = blockIdx.y * 256 + threadIdx.x; j < cols; j += 256 * gridDim.y) d[j] = s[j];
}

}  // namespace

namespace cgpt {

hipError_t launch_llm_beam_attn(const BeamAttnArgs& a, hipStream_t st) {
    const size_t lds = (size_t)(2 * HD + a.L + a.t + 1) * sizeof(float);
    hipLaunchKernelGGL(llm_attn_beam_kernel, dim3(a.rows * a.heads), dim3(64), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_llm_beam_select(const BeamSelectArgs& a, int images, hipStream_t st) {
    hipLaunchKernelGGL(llm_beam_select_kernel, dim3(images), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_llm_beam_spread(const float* src, int64_t lds, float* dst, int64_t ldd, int cols, int rows, int k, hipStream_t st) {
    hipLaunchKernelGGL(llm_beam_spread_kernel, dim3(rows, 8), dim3(256), 0, st, src, lds, dst, ldd, cols, k);
    return hipGetLastError();
}

}  // namespace cgpt

extern "C" {

cgpt_status cgpt_llm_beam_select_logits(const float* logits_dev, int64_t ld, int32_t B, int32_t k, int32_t V, int32_t step, int32_t num_new,
                                        int32_t min_new, const int64_t* eos_ids_host, int32_t num_eos, int64_t pad_id, float length_penalty,
                                        const float* running_in_dev, const int64_t* tokens_in_dev, const int32_t* anc_in_dev,
                                        const float* pool_score_in_dev, const int32_t* pool_fin_in_dev, const int32_t* pool_len_in_dev,
                                        const int64_t* pool_seq_in_dev, const int32_t* open_in_dev, float* running_out_dev,
                                        int64_t* tokens_out_dev, int32_t* anc_out_dev, float* pool_score_out_dev, int32_t* pool_fin_out_dev,
                                        int32_t* pool_len_out_dev, int64_t* pool_seq_out_dev, int32_t* open_out_dev, int64_t* next_tokens_dev,
                                        int32_t* parents_dev, void* stream) {
    const std::string who = "cgpt_llm_beam_select_logits";
    if (!logits_dev || !running_in_dev || !tokens_in_dev || !anc_in_dev || !pool_score_in_dev || !pool_fin_in_dev || !pool_len_in_dev ||
        !pool_seq_in_dev || !open_in_dev || !running_out_dev || !tokens_out_dev || !anc_out_dev || !pool_score_out_dev ||
        !pool_fin_out_dev || !pool_len_out_dev || !pool_seq_out_dev || !open_out_dev || !next_tokens_dev || !parents_dev)
        return cgpt_fail(CGPT_ERR_INVALID, who + ": null argument");
    if (k < BEAM_MIN || k > BEAM_MAX)
        return cgpt_fail(CGPT_ERR_INVALID, who + ": num_beams " + std::to_string(k) + " outside " + std::to_string(BEAM_MIN) + ".." +
                                               std::to_string(BEAM_MAX));
    if (num_eos < 0 || num_eos > MAX_EOS || (num_eos > 0 && !eos_ids_host)) return cgpt_fail(CGPT_ERR_INVALID, who + ": at most 8 EOS ids");
    const int K = (num_eos + 1 > 2 ? num_eos + 1 : 2) * k;
    if (B < 1 || V < K + num_eos || V > BEAM_MAX_VOCAB || ld < V || num_new < 1 || step < 0 || step >= num_new || min_new < 0)
        return cgpt_fail(CGPT_ERR_INVALID, who + ": B >= 1, K + num_eos <= V <= 131072 (K = max(2, 1 + num_eos) * num_beams), ld >= V, 0 <= step < num_new");
    if (!(length_penalty == length_penalty) || fabsf(length_penalty) == INFINITY)
        return cgpt_fail(CGPT_ERR_INVALID, who + ": length_penalty is not finite");
    BeamSelectArgs a{};
    a.src = logits_dev; a.lds = ld; a.shared = 0; a.vocab = V; a.k = k; a.keep = K; a.n = num_new; a.step = step; a.first = 0;
    a.mask_eos = (step < min_new && num_eos > 0) ? 1 : 0;
    a.eos.n = num_eos;
    for (int e = 0; e < num_eos; ++e) a.eos.id[e] = eos_ids_host[e];
    a.pad = pad_id;
    a.divisor = (float)pow((double)(step + 1), (double)length_penalty);
    a.in = BeamState{const_cast<float*>(running_in_dev), (long long*)tokens_in_dev, const_cast<int32_t*>(anc_in_dev),
                     const_cast<float*>(pool_score_in_dev), const_cast<int32_t*>(pool_fin_in_dev), const_cast<int32_t*>(pool_len_in_dev),
                     (long long*)pool_seq_in_dev, const_cast<int32_t*>(open_in_dev)};
    a.out = BeamState{running_out_dev, (long long*)tokens_out_dev, anc_out_dev, pool_score_out_dev, pool_fin_out_dev, pool_len_out_dev,
                      (long long*)pool_seq_out_dev, open_out_dev};
    a.next_tok = (long long*)next_tokens_dev;
    a.parents = parents_dev;
    const hipError_t e = launch_llm_beam_select(a, B, (hipStream_t)stream);
    if (e != hipSuccess) return cgpt_fail(CGPT_ERR_HIP, who + ": launch -> " + hipGetErrorString(e));
    return CGPT_OK;
}

}  // extern "C"
