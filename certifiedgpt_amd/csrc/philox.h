// philox.h -- counter-based Gaussian stream of the build (product side; oracle/philox.py restates it).
//
// Replaces `torch.randn_like(batch, device='cuda') * sigma` (reference randomized_smoothing/smoothing.py:96),
// whose device-global stream depends on batch size and device count.  Element e of Monte-Carlo sample s under
// seed S uses Philox4x32-10(counter = (e/4, hi_word, s_lo, s_hi), key = (S_lo, S_hi)); words (r0,r1) and (r2,r3)
// feed one Box-Muller pair each, so any partition of the sample range over batches / GPUs sees the same draws.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cgpt {

struct u32x4 { uint32_t x, y, z, w; };

// Counter word 1 (`hi_word`) names the stream, so that no two uses of one (seed, id) share a draw:
//   0  the Monte-Carlo noise of a sample (cgpt_sample_counts, cgpt_noise_batch, ...)
//   1  the synthetic weights (cgpt_init_synthetic_weights)
//   2  the processor noise
//   3  the sampled decode: counter = (step, 3, draw id lo, draw id hi), word 0 -> one uniform per row and step (llm_sample.hip)
constexpr uint32_t PHILOX_WORD_NOISE = 0, PHILOX_WORD_WEIGHTS = 1, PHILOX_WORD_PROCESSOR = 2, PHILOX_WORD_SAMPLE = 3;

__host__ __device__ inline u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                               uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return u32x4{c0, c1, c2, c3};
}

// 4 standard normals for element group g of `stream` (a sample index or a tensor id).
__device__ inline float4 normal4(uint64_t seed, uint64_t stream, uint32_t g, uint32_t hi_word) {
    const u32x4 r = philox4x32_10(g, hi_word, (uint32_t)stream, (uint32_t)(stream >> 32),
                                  (uint32_t)seed, (uint32_t)(seed >> 32));
    const float k = 5.9604644775390625e-08f;  // 2^-24
    const float u1a = (float)((r.x >> 8) + 1u) * k, u2a = (float)(r.y >> 8) * k;
    const float u1b = (float)((r.z >> 8) + 1u) * k, u2b = (float)(r.w >> 8) * k;
    const float ra = sqrtf(-2.0f * logf(u1a)), rb = sqrtf(-2.0f * logf(u1b));
    float sa, ca, sb, cb;
    sincospif(2.0f * u2a, &sa, &ca);
    sincospif(2.0f * u2b, &sb, &cb);
    return make_float4(ra * ca, ra * sa, rb * cb, rb * sb);
}

// 4 uniforms in [0, 1) from the same Philox block: element e takes word e % 4, u = (word >> 8) * 2^-24 (24 bits, exact in
// fp32).  The uniform law of the reference's fine-tuning noise, `image + torch.rand_like(image) * noise_level`
// (agents/minigpt4_finetune_agent.py:142-147), is x + level * u.
__device__ inline float4 uniform4(uint64_t seed, uint64_t stream, uint32_t g, uint32_t hi_word) {
    const u32x4 r = philox4x32_10(g, hi_word, (uint32_t)stream, (uint32_t)(stream >> 32),
                                  (uint32_t)seed, (uint32_t)(seed >> 32));
    const float k = 5.9604644775390625e-08f;  // 2^-24
    return make_float4((float)(r.x >> 8) * k, (float)(r.y >> 8) * k, (float)(r.z >> 8) * k, (float)(r.w >> 8) * k);
}

// Noise law of a noisy kernel instantiation; GAUSSIAN and UNIFORM carry the values of CGPT_NOISE_* (include/cgpt.h).
enum NoiseLaw { NOISE_NONE = -1, NOISE_GAUSSIAN = 0, NOISE_UNIFORM = 1 };

// The 4 unit draws of element group g under LAW (GAUSSIAN or UNIFORM); the caller adds scale * draw.
template <int LAW>
__device__ inline float4 noise4(uint64_t seed, uint64_t stream, uint32_t g, uint32_t hi_word) {
    if constexpr (LAW == NOISE_UNIFORM) return uniform4(seed, stream, g, hi_word);
    else return normal4(seed, stream, g, hi_word);
}

}  // namespace cgpt
