// llm_sample.hip -- the sampled token select of the native LLaMA engine (sample="hip"; include/cgpt.h, "Sampled decoding").
//
// Reference call replaced: HF `generate(do_sample=True, temperature, top_k, top_p, repetition_penalty)` as `Chat.answer_prepare`
// calls it -- RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper, softmax and
// torch.multinomial on the device-global generator.  Here one kernel per select, in the slot of llm_select_kernel (llm_step.hip), draws
// from a counter-based stream: the uniform of a row is a function of (seed, draw id, step) alone (philox.h, PHILOX_WORD_SAMPLE).
//
// The law (`sample_token_law` in minigpt4.py states it in float64), on one fp32 logits row:
//   1. EOS columns read as -inf while mask_eos          2. every distinct earlier token of the row is penalised once
//      (l > 0 ? l / pen : l * pen)                        3. l / T          4. keep l >= the k-th largest value (ties included)
//   5. softmax over what is kept                          6. keep p >= p_(n), n the smallest count whose sorted mass reaches top_p
//      (ties included)                                    7. inverse CDF in vocabulary index order at u * kept_mass.
// No sort: both cuts are thresholds on the order-preserving integer image of the fp32 value (`okey`), found by bisection over its 32
// bits -- each round one block-wide masked count (top-k) or masked sum (top-p) over the row, re-read from L2.  A row is never held
// in LDS: 128 256 columns do not fit.
//
// Precision: steps 1-3 and both thresholds are fp32 (IEEE divide and multiply), as the logits are; the softmax weights
// exp(l / T - max) and every sum of them are float64, so what separates the kernel's masses from the float64 law is the fp32
// penalty quotient of the few penalised columns and the fp32 rounding of the reported kept mass -- not the vocabulary's size.
// Summation order, fixed, so that replays are bit-identical and the tolerance of tests/test_gpu_llm_sample.py can be derived:
//   masked sums:  thread t adds its columns t, t + 256, t + 512, ... in ascending order (excluded columns add 0.0); the 64 partials
//                 of a wave are added by the xor butterfly 32, 16, 8, 4, 2, 1; the four wave sums are added as ((w0 + w1) + w2) + w3.
//   inverse CDF:  thread t adds the kept columns of the contiguous chunk [t L, (t + 1) L), L = ceil(V / 256), in ascending order;
//                 thread 0 adds the 256 chunk sums in chunk order, finds the chunk in which the running sum passes u * total and
//                 walks that chunk, adding its columns again in the same order.
// Plain loads and stores only; nothing is atomic.
#include <math.h>

#include <string>

#include "../../include/cgpt.h"
#include "common_host.h"
#include "llm_select.h"
#include "philox.h"

using namespace cgpt;

namespace {

constexpr int HASH = 2048;                         // open-addressing table of the special columns (<= 1024 entries)
constexpr unsigned KEY_MIN_FINITE = 0x00800000u;   // okey(-FLT_MAX); okey(-inf) = 0x007fffff lies below: -inf is never kept

// fp32 -> uint32, order preserving (-0 as +0)
__device__ __forceinline__ unsigned okey(float x) {
    unsigned b = __float_as_uint(x);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float okey_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
__device__ __forceinline__ unsigned hash_slot(int j) { return ((unsigned)j * 2654435761u) >> 21; }

// The row after steps 1-3: column j is its logit unless the column is special (EOS-masked or an earlier token of the row), whose
// value the table holds; then the temperature.
struct RowView {
    const float* s;
    const unsigned* bits;
    const int* hkey;
    const float* hval;
    bool special, temper;
    float T;
};
// steps 1-2: the value before the temperature
__device__ __forceinline__ float row_raw(const RowView& r, int j) {
    float v = r.s[j];
    if (r.special && ((r.bits[j >> 5] >> (j & 31)) & 1u)) {
        unsigned h = hash_slot(j);
        while (r.hkey[h] != j) h = (h + 1) & (HASH - 1);
        v = r.hval[h];
    }
    return v;
}
// steps 1-3 in fp32: what the two cuts order the columns by
__device__ __forceinline__ float row_value(const RowView& r, int j) {
    const float v = row_raw(r, j);
    return r.temper ? v / r.T : v;
}
// The softmax weight of a column, exp(l / T - m), in float64 from the fp32 value of steps 1-2: the fp32 quotient l / T would carry
// its rounding (6e-8 |l / T|) into every weight.  m is any constant near the row's maximum; it cancels in every comparison.
__device__ __forceinline__ double row_weight(const RowView& r, float raw, double m) {
    return exp((r.temper ? (double)raw / (double)r.T : (double)raw) - m);
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
__device__ __forceinline__ int block_sum(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const int t = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return t;
}
__device__ __forceinline__ unsigned block_max(unsigned v, unsigned* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const unsigned t = max(max(red[0], red[1]), max(red[2], red[3]));
    __syncthreads();
    return t;
}

// One workgroup per row, in the slot of llm_select_kernel and with its bookkeeping (CGPT_SELECT_TAIL): GUARD and STOP as there.
template <bool GUARD, bool STOP>
__global__ __launch_bounds__(256) void llm_sample_kernel(SelectArgs a, StopArg<STOP> stop, SampleLaw law, SampleIo io) {
    __shared__ unsigned bits[SAMPLE_MAX_VOCAB / 32];
    __shared__ int hkey[HASH];
    __shared__ float hval[HASH];
    __shared__ int ptok[SAMPLE_MAX_SPECIAL];
    __shared__ float praw[SAMPLE_MAX_SPECIAL];
    __shared__ double part[256];
    __shared__ double redf[4];
    __shared__ int redi[4];
    __shared__ unsigned redu[4];
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    if constexpr (GUARD) {
        if (!a.first && *a.live == 0) {                                     // a dead select, as in llm_select_kernel
            if (tid == 0) {
                a.tokens_out[(int64_t)row * a.ld_tokens] = a.pad;
                a.next_tok[row] = a.pad;
            }
            return;
        }
    }
    const int V = a.vocab;
    const float* s = a.src + (int64_t)row * a.lds;
    if (a.dst) {                                                            // the logits the sampler sees: EOS-masked, nothing else
        float* d = a.dst + (int64_t)row * a.ldd;
        for (int j = tid; j < V; j += 256) {
            float v = s[j];
            if (a.mask_eos)
                for (int e = 0; e < a.eos.n; ++e)
                    if (a.eos.id[e] == j) v = -INFINITY;
            d[j] = v;
        }
        __syncthreads();
    }
    // ---- steps 1 and 2: the special columns, one table entry each (a repeated id is penalised once; a masked column stays -inf)
    const int nprev = law.penalty != 1.0f ? io.num_prev : 0;
    const int neos = a.mask_eos ? a.eos.n : 0;
    const bool special = nprev + neos > 0;
    if (special) {
        for (int w = tid; w < (V + 31) / 32; w += 256) bits[w] = 0u;
        for (int h = tid; h < HASH; h += 256) hkey[h] = -1;
        for (int p = tid; p < nprev; p += 256) {
            const long long t = io.prev[(int64_t)row * io.ld_prev + p];
            const bool ok = t >= 0 && t < V;
            ptok[p] = ok ? (int)t : -1;
            praw[p] = ok ? s[t] : 0.0f;
        }
        __syncthreads();
        if (tid == 0) {
            for (int e = 0; e < neos + nprev; ++e) {
                int j;
                float v;
                if (e < neos) {
                    const long long id = a.eos.id[e];
                    if (id < 0 || id >= V) continue;
                    j = (int)id;
                    v = -INFINITY;
                } else {
                    j = ptok[e - neos];
                    if (j < 0) continue;
                    const float l = praw[e - neos];
                    v = l > 0.0f ? l / law.penalty : l * law.penalty;
                }
                unsigned h = hash_slot(j);
                while (hkey[h] != -1 && hkey[h] != j) h = (h + 1) & (HASH - 1);
                if (hkey[h] == j) continue;
                hkey[h] = j;
                hval[h] = v;
                bits[j >> 5] |= 1u << (j & 31);
            }
        }
        __syncthreads();
    }
    const RowView r{s, bits, hkey, hval, special, law.do_sample && law.temperature != 1.0f, law.temperature};

    int token = 0, kept = 1;
    float u = 0.0f, mass = 1.0f;
    if (!law.do_sample) {
        // ---- steps 1-2, then the first-max arg-max of llm_select_kernel
        float best = -INFINITY;
        int idx = 0x7fffffff;
        for (int j = tid; j < V; j += 256) {
            const float v = row_value(r, j);
            if (idx == 0x7fffffff || v > best) { best = v; idx = j; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o);
            const int oi = __shfl_xor(idx, o);
            if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
        }
        if ((tid & 63) == 0) { bv[tid >> 6] = best; bi[tid >> 6] = idx; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w)
                if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
            token = idx;
        }
    } else {
        unsigned km = 0u;
        for (int j = tid; j < V; j += 256) km = max(km, okey(row_value(r, j)));
        const unsigned kmax = block_max(km, redu);
        const double m = (double)okey_value(kmax);
        // ---- step 4: tk = the k-th largest key = the largest t with count(key >= t) >= k
        unsigned tk = KEY_MIN_FINITE;
        if (law.top_k > 0 && law.top_k < V) {
            unsigned t = 0u;
            for (int bit = 31; bit >= 0; --bit) {
                const unsigned cand = t | (1u << bit);
                if (cand > kmax) continue;                                  // the count would be 0
                int c = 0;
                for (int j = tid; j < V; j += 256) c += okey(row_value(r, j)) >= cand ? 1 : 0;
                if (block_sum(c, redi) >= law.top_k) t = cand;
            }
            tk = max(t, KEY_MIN_FINITE);
        }
        // ---- step 5: Z = the softmax denominator over the top-k set (weights exp(l - max))
        double z = 0.0;
        for (int j = tid; j < V; j += 256) {
            const float raw = row_raw(r, j);
            z += okey(r.temper ? raw / r.T : raw) >= tk ? row_weight(r, raw, m) : 0.0;
        }
        const double Z = block_sum(z, redf);
        // ---- step 6: t2 = the largest t whose mass S(t) = sum of the weights with key >= max(t, tk) reaches top_p Z.  S(t) = Z for
        // t <= tk, bit for bit (the same sum), so those rounds are accepted without a pass.
        unsigned t2 = tk;
        double M = Z;
        if (law.top_p < 1.0f) {
            const double need = (double)law.top_p * Z;
            unsigned t = 0u;
            for (int bit = 31; bit >= 0; --bit) {
                const unsigned cand = t | (1u << bit);
                if (cand > kmax) continue;
                if (cand <= tk) { t = cand; continue; }
                double sm = 0.0;
                for (int j = tid; j < V; j += 256) {
                    const float raw = row_raw(r, j);
                    sm += okey(r.temper ? raw / r.T : raw) >= cand ? row_weight(r, raw, m) : 0.0;
                }
                const double S = block_sum(sm, redf);
                if (S >= need) { t = cand; M = S; }
            }
            t2 = max(t, tk);
        }
        // ---- step 7: chunk sums in index order, then the walk
        const int L = (V + 255) / 256;
        const int lo = min(V, tid * L), hi = min(V, lo + L);
        double ps = 0.0;
        int cnt = 0;
        for (int j = lo; j < hi; ++j) {
            const float raw = row_raw(r, j);
            if (okey(r.temper ? raw / r.T : raw) >= t2) { ps += row_weight(r, raw, m); ++cnt; }
        }
        part[tid] = ps;
        cnt = block_sum(cnt, redi);                                         // its barriers also publish `part`
        if (tid == 0) {
            if (io.uniforms_in) {
                u = io.uniforms_in[row];
            } else {
                const unsigned long long id = (unsigned long long)io.draw_ids[row], seed = *io.seed;
                const u32x4 w = philox4x32_10((uint32_t)io.step, PHILOX_WORD_SAMPLE, (uint32_t)id, (uint32_t)(id >> 32), (uint32_t)seed,
                                              (uint32_t)(seed >> 32));
                u = (float)(w.x >> 8) * 5.9604644775390625e-08f;            // 2^-24
            }
            double total = 0.0;
            for (int c = 0; c < 256; ++c) total += part[c];
            const double target = (double)u * total;
            double run = 0.0;
            int c = 0;
            for (; c < 255; ++c) {
                if (run + part[c] > target) break;
                run += part[c];
            }
            const int clo = min(V, c * L), chi = min(V, clo + L);
            int last = -1;
            double local = 0.0;
            token = -1;
            for (int j = clo; j < chi; ++j) {
                const float raw = row_raw(r, j);
                if (okey(r.temper ? raw / r.T : raw) >= t2) {
                    last = j;
                    local += row_weight(r, raw, m);
                    if (run + local > target) { token = j; break; }
                }
            }
            if (token < 0) token = last;
            for (int j = V - 1; token < 0 && j >= 0; --j)                   // unreachable for finite rows: the last kept column
                if (okey(row_value(r, j)) >= t2) token = j;
            if (token < 0) token = 0;
            kept = cnt;
            mass = (float)(M / Z);
        }
    }
    if (tid == 0) {
        if (io.uniforms_out) io.uniforms_out[row] = u;
        if (io.kept_count_out) io.kept_count_out[row] = kept;
        if (io.kept_mass_out) io.kept_mass_out[row] = mass;
        CGPT_SELECT_TAIL(STOP, row, token, a.first, a.eos, a.pad, a.unfinished, a.tokens_out, a.ld_tokens, a.next_tok, stop);
    }
}

}  // namespace

namespace cgpt {

hipError_t launch_llm_sample(bool guard, const StopSeqs* stop, const SelectArgs& a, const SampleLaw& law, const SampleIo& io, int rows,
                             hipStream_t st) {
    if (guard && stop)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(llm_sample_kernel<true, true>), dim3(rows), dim3(256), 0, st, a, *stop, law, io);
    else if (guard)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(llm_sample_kernel<true, false>), dim3(rows), dim3(256), 0, st, a, NoStop{}, law, io);
    else if (stop)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(llm_sample_kernel<false, true>), dim3(rows), dim3(256), 0, st, a, *stop, law, io);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(llm_sample_kernel<false, false>), dim3(rows), dim3(256), 0, st, a, NoStop{}, law, io);
    return hipGetLastError();
}

cgpt_status check_sample_params(const std::string& who, const cgpt_llm_sample_params& p, int vocab, int num_prev, int num_eos,
                                SampleLaw* out) {
    if (p.struct_size != (int32_t)sizeof(cgpt_llm_sample_params))
        return cgpt_fail(CGPT_ERR_INVALID, who + ": params.struct_size is not sizeof(cgpt_llm_sample_params)");
    if (p.do_sample != 0 && p.do_sample != 1) return cgpt_fail(CGPT_ERR_INVALID, who + ": do_sample must be 0 or 1");
    if (!(p.temperature > 0.0f) || isinf(p.temperature)) return cgpt_fail(CGPT_ERR_INVALID, who + ": temperature must be > 0 and finite");
    if (!(p.top_p > 0.0f && p.top_p <= 1.0f)) return cgpt_fail(CGPT_ERR_INVALID, who + ": top_p must lie in (0, 1]");
    if (p.top_k < 0) return cgpt_fail(CGPT_ERR_INVALID, who + ": top_k must be >= 0 (0: off)");
    if (!(p.repetition_penalty > 0.0f) || isinf(p.repetition_penalty))
        return cgpt_fail(CGPT_ERR_INVALID, who + ": repetition_penalty must be > 0 and finite");
    if (vocab < 1 || vocab > SAMPLE_MAX_VOCAB)
        return cgpt_fail(CGPT_ERR_INVALID, who + ": the sampler takes a vocabulary of 1.." + std::to_string(SAMPLE_MAX_VOCAB));
    if (num_prev < 0 || num_prev + num_eos > SAMPLE_MAX_SPECIAL)
        return cgpt_fail(CGPT_ERR_INVALID, who + ": earlier tokens + EOS ids of one select exceed " + std::to_string(SAMPLE_MAX_SPECIAL));
    *out = SampleLaw{p.do_sample, p.temperature, p.top_k, p.top_p, p.repetition_penalty};
    return CGPT_OK;
}

}  // namespace cgpt

cgpt_status cgpt_llm_sample_logits(const float* logits_dev, int64_t ld, int32_t B, int32_t V, const int64_t* prev_tokens_dev,
                                   int64_t ld_prev, int32_t num_prev, int32_t step, int32_t mask_eos, const int64_t* eos_ids_host,
                                   int32_t num_eos, int64_t pad_id, int32_t* unfinished_dev, cgpt_llm_sample_params params,
                                   const int64_t* draw_ids_dev, const uint64_t* seed_dev, const float* uniforms_in_dev,
                                   int64_t* tokens_out_dev, float* uniforms_out_dev, int32_t* kept_count_out_dev,
                                   float* kept_mass_out_dev, void* stream) {
    const std::string who = "cgpt_llm_sample_logits";
    if (!logits_dev || !tokens_out_dev || !unfinished_dev) return cgpt_fail(CGPT_ERR_INVALID, who + ": null logits, tokens_out or unfinished");
    if (num_eos < 0 || num_eos > MAX_EOS || (num_eos > 0 && !eos_ids_host))
        return cgpt_fail(CGPT_ERR_INVALID, who + ": at most 8 EOS ids, and not null when there are any");
    SampleLaw law;
    cgpt_status s = check_sample_params(who, params, V, num_prev, num_eos, &law);
    if (s != CGPT_OK) return s;
    if (B < 1 || ld < V || (num_prev > 0 && (!prev_tokens_dev || ld_prev < num_prev)))
        return cgpt_fail(CGPT_ERR_INVALID, who + ": B >= 1, ld >= V, and num_prev tokens per row (ld_prev >= num_prev)");
    if (!uniforms_in_dev && (!draw_ids_dev || !seed_dev))
        return cgpt_fail(CGPT_ERR_INVALID, who + ": null draw_ids_dev / seed_dev without uniforms_in_dev");
    SelectArgs a{};
    a.src = logits_dev; a.lds = ld; a.dst = nullptr; a.ldd = 0; a.vocab = V; a.mask_eos = (mask_eos && num_eos > 0) ? 1 : 0;
    a.eos.n = num_eos;
    for (int e = 0; e < num_eos; ++e) a.eos.id[e] = eos_ids_host[e];
    a.pad = pad_id; a.first = 0; a.unfinished = unfinished_dev; a.tokens_out = (long long*)tokens_out_dev; a.ld_tokens = 1;
    a.next_tok = (long long*)tokens_out_dev; a.live = nullptr;
    SampleIo io{(const long long*)prev_tokens_dev, ld_prev, num_prev, step, (const long long*)draw_ids_dev,
                (const unsigned long long*)seed_dev, uniforms_in_dev, uniforms_out_dev, kept_count_out_dev, kept_mass_out_dev};
    hipError_t e = launch_llm_sample(false, nullptr, a, law, io, B, (hipStream_t)stream);
    if (e != hipSuccess) return cgpt_fail(CGPT_ERR_HIP, who + ": launch -> " + hipGetErrorString(e));
    return CGPT_OK;
}
