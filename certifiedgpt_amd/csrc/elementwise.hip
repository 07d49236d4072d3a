// elementwise.hip -- the HBM-bound kernels of the hot path: Gaussian / uniform perturbation fused with the patch-embed
// im2col, LayerNorm, CLS/pos rows, query-token broadcast, mean pool, argmax + vote histogram, weight fills/casts.
//
// Reference ops replaced: smoothing.py:95-98,101-105 (repeat + randn*sigma; argmax(1); _count_arr),
// eva_vit.py:162,168 + base_model.py:281-287 (LayerNorm), eva_vit.py:337-340 (CLS concat + pos_embed),
// minigpt4.py:132 (query_tokens.expand), Qformer.py:106 (embeddings LayerNorm).
#include "kernels.h"
#include "philox.h"
#include "stats.h"

namespace cgpt {

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ------------------------------------------------------------------------------------------ LayerNorm
// One wave per row; the row lives in registers (NCH float2 per lane) between the mean, the centred variance
// and the normalise pass, so x is read from HBM exactly once.  Requires D even and D <= NCH*128.
// With `delta` (fp16) the kernel first applies the pending residual update x += delta and writes x back: the
// reference's `x = x + attn(...)` / `x = x + mlp(...)` (eva_vit.py:180-181), where under autocast the branch output is
// an fp16 tensor added to the fp32 stream -- done here instead of as a read-modify-write in the GEMM epilogue.
// Two pending updates (delta, then delta2, added in that order) and keep_x (normalise x + delta [+ delta2] but leave x as it
// is) let a transformer block write the fp32 stream ONCE: LN1 reads x + (previous fc2 output) without writing, LN2 reads
// x + (previous fc2 output) + (this block's proj output) and writes the sum -- same additions in the same order.
template <int NCH>
__global__ __launch_bounds__(256) void layernorm_kernel(float* __restrict__ x, int64_t ldx,
                                                        const half_t* __restrict__ delta, int64_t ldd,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps,
                                                        half_t* __restrict__ y16, int64_t ldy16,
                                                        float* __restrict__ y32, int64_t ldy32, int64_t rows, int D,
                                                        const half_t* __restrict__ delta2, int64_t ldd2, int keep_x) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float* xr = x + row * ldx;
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    float2 v[NCH];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int col = c * 128 + lane * 2;
        v[c] = (col < D) ? *reinterpret_cast<const float2*>(xr + col) : make_float2(0.f, 0.f);
        if (delta && col < D) {
            const f16x2 d = *reinterpret_cast<const f16x2*>(delta + row * ldd + col);
            v[c].x += (float)d[0];
            v[c].y += (float)d[1];
        }
        if (delta2 && col < D) {
            const f16x2 d = *reinterpret_cast<const f16x2*>(delta2 + row * ldd2 + col);
            v[c].x += (float)d[0];
            v[c].y += (float)d[1];
        }
        if ((delta || delta2) && !keep_x && col < D) *reinterpret_cast<float2*>(xr + col) = v[c];
        s += v[c].x + v[c].y;
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int col = c * 128 + lane * 2;
        if (col < D) {
            const float dx = v[c].x - mean, dy = v[c].y - mean;
            q += dx * dx + dy * dy;
        }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int col = c * 128 + lane * 2;
        if (col < D) {
            const float2 gm = *reinterpret_cast<const float2*>(gamma + col);
            const float2 bt = *reinterpret_cast<const float2*>(beta + col);
            const float a = (v[c].x - mean) * rstd * gm.x + bt.x;
            const float b = (v[c].y - mean) * rstd * gm.y + bt.y;
            if (y16) {
                *reinterpret_cast<f16x2*>(y16 + row * ldy16 + col) = f16x2{(half_t)a, (half_t)b};
            }
            if (y32) *reinterpret_cast<float2*>(y32 + row * ldy32 + col) = make_float2(a, b);
        }
    }
}


// 16-byte variant for D % 128 == 0: one row per HALF-wave (32 lanes x NCH float4), two rows per wave; the row still lives
// in registers between the three passes.  Wider accesses than the float2 kernel (16 B per lane instead of 8 B).
template <int NCH>
__device__ __forceinline__ void layernorm4_body(float* __restrict__ x, int64_t ldx,
                                                         const half_t* __restrict__ delta, int64_t ldd,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float eps, half_t* __restrict__ y16, int64_t ldy16,
                                                         float* __restrict__ y32, int64_t ldy32, int64_t rows, int D,
                                                         const half_t* __restrict__ delta2, int64_t ldd2, int keep_x) {
    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
    const int l32 = threadIdx.x & 31;
    const int64_t row = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
    const bool live = row < rows;                        // keep the whole wave in the shuffles
    const int64_t rr = live ? row : rows - 1;
    float* xr = x + rr * ldx;
    float4 v[NCH];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int col = c * 128 + l32 * 4;
        {
            typedef float f32x4nt __attribute__((ext_vector_type(4)));
            const f32x4nt t = __builtin_nontemporal_load(reinterpret_cast<const f32x4nt*>(xr + col));
            v[c] = make_float4(t[0], t[1], t[2], t[3]);
        }
        if (delta) {
            const f16x4 d = __builtin_nontemporal_load(reinterpret_cast<const f16x4*>(delta + rr * ldd + col));
            v[c].x += (float)d[0]; v[c].y += (float)d[1]; v[c].z += (float)d[2]; v[c].w += (float)d[3];
        }
        if (delta2) {
            const f16x4 d = __builtin_nontemporal_load(reinterpret_cast<const f16x4*>(delta2 + rr * ldd2 + col));
            v[c].x += (float)d[0]; v[c].y += (float)d[1]; v[c].z += (float)d[2]; v[c].w += (float)d[3];
        }
        if ((delta || delta2) && !keep_x && live) {
            typedef float f32x4nt __attribute__((ext_vector_type(4)));
            __builtin_nontemporal_store(f32x4nt{v[c].x, v[c].y, v[c].z, v[c].w}, reinterpret_cast<f32x4nt*>(xr + col));
        }
        s += (v[c].x + v[c].y) + (v[c].z + v[c].w);
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)D;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const float a = v[c].x - mean, b = v[c].y - mean, cc = v[c].z - mean, d = v[c].w - mean;
        q += (a * a + b * b) + (cc * cc + d * d);
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = rsqrtf(q / (float)D + eps);
    if (!live) return;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int col = c * 128 + l32 * 4;
        const float4 gm = *reinterpret_cast<const float4*>(gamma + col);
        const float4 bt = *reinterpret_cast<const float4*>(beta + col);
        const float o0 = (v[c].x - mean) * rstd * gm.x + bt.x, o1 = (v[c].y - mean) * rstd * gm.y + bt.y;
        const float o2 = (v[c].z - mean) * rstd * gm.z + bt.z, o3 = (v[c].w - mean) * rstd * gm.w + bt.w;
        if (y16) *reinterpret_cast<f16x4*>(y16 + row * ldy16 + col) = f16x4{(half_t)o0, (half_t)o1, (half_t)o2, (half_t)o3};
        if (y32) *reinterpret_cast<float4*>(y32 + row * ldy32 + col) = make_float4(o0, o1, o2, o3);
    }
}

#define CGPT_LN4_ARGS float* __restrict__ x, int64_t ldx, const half_t* __restrict__ delta, int64_t ldd, const float* __restrict__ gamma, \
                      const float* __restrict__ beta, float eps, half_t* __restrict__ y16, int64_t ldy16, float* __restrict__ y32, \
                      int64_t ldy32, int64_t rows, int D, const half_t* __restrict__ delta2, int64_t ldd2, int keep_x
#define CGPT_LN4_PASS x, ldx, delta, ldd, gamma, beta, eps, y16, ldy16, y32, ldy32, rows, D, delta2, ldd2, keep_x
template <int NCH>
__global__ __launch_bounds__(256) void layernorm4_kernel(CGPT_LN4_ARGS) { layernorm4_body<NCH>(CGPT_LN4_PASS); }
// The ViT-G width (D = 1408, NCH = 11) with amdgpu_waves_per_eu(6, 8): 80 instead of 86 VGPRs, six waves per SIMD instead of five:
// 187 -> 181 us per launch in the model (7: 72 VGPRs with 2 spilled, no further gain; 8: 64 VGPRs, 6 spilled, slower).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6, 8))) void layernorm4_vitg_kernel(CGPT_LN4_ARGS) {
    layernorm4_body<11>(CGPT_LN4_PASS);
}

// The 16-byte path again, scheduled for the memory system (ln_kernel = 1, the default; layernorm4_body above is ln_kernel = 0).
// Same row -> lane mapping and the same floating-point operations in the same order as layernorm4_body, so the bits are the
// same; what differs is when memory is touched:
//  * the form (delta / delta2 / store x / y16 / y32) is a template parameter: no branch in any loop, so hipcc can hoist loads;
//  * the global loads of a row (x, delta, delta2: NCH x (16 + 8 + 8) B per lane) all stand before the first use and are waited
//    for with counted vmcnt (hipcc holds the last 6 of LN1's 22 and 8 of LN2's 33 back until the first return, for registers);
//    the fp32 stream store leaves after the statistics, behind the row's last load;
//  * gamma and beta are staged once per workgroup in LDS (ds_read_b128 counts on lgkmcnt, so pass 3 never waits for its own
//    stores, which a global load there would: vmcnt counts loads and stores together), and a workgroup walks row groups in a
//    grid-stride loop so that the staging is paid once per ~6 groups.
// SPLIT = 0: loads issued chunk by chunk (x, delta, delta2 of chunk c together); SPLIT = 1: two halves of the row, each as
// x.. delta.. delta2.., the second half's loads issued before the first half's arithmetic.  WAVES = waves per SIMD asked for.
template <int NCH, bool HAS_D, bool HAS_D2, bool STORE_X, bool Y16, bool Y32, int SPLIT>
__device__ __forceinline__ void layernorm4_rows_body(float* __restrict__ x, int64_t ldx, const half_t* __restrict__ delta, int64_t ldd,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                     half_t* __restrict__ y16, int64_t ldy16, float* __restrict__ y32, int64_t ldy32,
                                                     int64_t rows, const half_t* __restrict__ delta2, int64_t ldd2) {
    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
    typedef float f32x4nt __attribute__((ext_vector_type(4)));
    constexpr int D = NCH * 128, HALF = (NCH + 1) / 2;
    __shared__ float4 gb[2 * NCH * 32];                    // gamma, then beta
    for (int i = threadIdx.x; i < NCH * 32; i += 256) {
        gb[i] = reinterpret_cast<const float4*>(gamma)[i];
        gb[NCH * 32 + i] = reinterpret_cast<const float4*>(beta)[i];
    }
    __syncthreads();
    const int l32 = threadIdx.x & 31;
    const int64_t groups = (rows + 7) >> 3;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {            // uniform per workgroup: every wave stays in the shuffles
        const int64_t row = g * 8 + (threadIdx.x >> 5);
        const bool live = row < rows;
        const int64_t rr = live ? row : rows - 1;                       // a dead half-wave reads the last row and stores nothing
        float* xr = x + rr * ldx + l32 * 4;
        const half_t* dr = HAS_D ? delta + rr * ldd + l32 * 4 : nullptr;
        const half_t* er = HAS_D2 ? delta2 + rr * ldd2 + l32 * 4 : nullptr;
        f32x4nt xv[NCH];
        f16x4 dv[NCH], ev[NCH];
        if constexpr (SPLIT == 0) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                xv[c] = __builtin_nontemporal_load(reinterpret_cast<const f32x4nt*>(xr + c * 128));
                if constexpr (HAS_D) dv[c] = __builtin_nontemporal_load(reinterpret_cast<const f16x4*>(dr + c * 128));
                if constexpr (HAS_D2) ev[c] = __builtin_nontemporal_load(reinterpret_cast<const f16x4*>(er + c * 128));
            }
        } else {
            constexpr int H = HALF;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c0 = h ? H : 0, c1 = h ? NCH : H;
#pragma unroll
                for (int c = c0; c < c1; ++c) xv[c] = __builtin_nontemporal_load(reinterpret_cast<const f32x4nt*>(xr + c * 128));
                if constexpr (HAS_D) {
#pragma unroll
                    for (int c = c0; c < c1; ++c) dv[c] = __builtin_nontemporal_load(reinterpret_cast<const f16x4*>(dr + c * 128));
                }
                if constexpr (HAS_D2) {
#pragma unroll
                    for (int c = c0; c < c1; ++c) ev[c] = __builtin_nontemporal_load(reinterpret_cast<const f16x4*>(er + c * 128));
                }
            }
        }
        float4 v[NCH];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            v[c] = make_float4(xv[c][0], xv[c][1], xv[c][2], xv[c][3]);
            if constexpr (HAS_D) { v[c].x += (float)dv[c][0]; v[c].y += (float)dv[c][1]; v[c].z += (float)dv[c][2]; v[c].w += (float)dv[c][3]; }
            if constexpr (HAS_D2) { v[c].x += (float)ev[c][0]; v[c].y += (float)ev[c][1]; v[c].z += (float)ev[c][2]; v[c].w += (float)ev[c][3]; }
            s += (v[c].x + v[c].y) + (v[c].z + v[c].w);
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o);
        const float mean = s / (float)D;
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const float a = v[c].x - mean, b = v[c].y - mean, cc = v[c].z - mean, d = v[c].w - mean;
            q += (a * a + b * b) + (cc * cc + d * d);
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) q += __shfl_xor(q, o);
        const float rstd = rsqrtf(q / (float)D + eps);
        if (live) {
            if constexpr (STORE_X) {
#pragma unroll
                for (int c = 0; c < NCH; ++c)
                    __builtin_nontemporal_store(f32x4nt{v[c].x, v[c].y, v[c].z, v[c].w}, reinterpret_cast<f32x4nt*>(xr + c * 128));
            }
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const int col = c * 128 + l32 * 4;
                const float4 gm = gb[c * 32 + l32];
                const float4 bt = gb[NCH * 32 + c * 32 + l32];
                float o0 = (v[c].x - mean) * rstd * gm.x + bt.x, o1 = (v[c].y - mean) * rstd * gm.y + bt.y;
                float o2 = (v[c].z - mean) * rstd * gm.z + bt.z, o3 = (v[c].w - mean) * rstd * gm.w + bt.w;
                // keep the fp32 result as its own value: with the output type known at compile time hipcc otherwise fuses the fma and
                // the fp16 convert into v_fma_mix*_f16 (ONE rounding); layernorm4_body rounds to fp32 first, then to fp16
                asm volatile("" : "+v"(o0), "+v"(o1), "+v"(o2), "+v"(o3));
                if constexpr (Y16) *reinterpret_cast<f16x4*>(y16 + row * ldy16 + col) = f16x4{(half_t)o0, (half_t)o1, (half_t)o2, (half_t)o3};
                if constexpr (Y32) *reinterpret_cast<float4*>(y32 + row * ldy32 + col) = make_float4(o0, o1, o2, o3);
            }
        }
    }
}

#define CGPT_LNR_ARGS float* __restrict__ x, int64_t ldx, const half_t* __restrict__ delta, int64_t ldd, const float* __restrict__ gamma, \
                      const float* __restrict__ beta, float eps, half_t* __restrict__ y16, int64_t ldy16, float* __restrict__ y32, \
                      int64_t ldy32, int64_t rows, const half_t* __restrict__ delta2, int64_t ldd2
template <int NCH, bool HAS_D, bool HAS_D2, bool STORE_X, bool Y16, bool Y32, int SPLIT, int WAVES>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WAVES, 8))) void layernorm4_rows_kernel(CGPT_LNR_ARGS) {
    layernorm4_rows_body<NCH, HAS_D, HAS_D2, STORE_X, Y16, Y32, SPLIT>(x, ldx, delta, ldd, gamma, beta, eps, y16, ldy16, y32, ldy32, rows,
                                                                      delta2, ldd2);
}

// x[row, :] += delta[row, :]  (the last block's pending residual update, when no LayerNorm follows on those rows)
__global__ __launch_bounds__(256) void add_delta_kernel(float* __restrict__ x, int64_t ldx, const half_t* __restrict__ delta,
                                                        int64_t ldd, int64_t rows, int D, int skip_mod) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;       // one float2 per thread
    const int half_d = D >> 1;
    if (i >= rows * half_d) return;
    const int64_t r = i / half_d;
    if (skip_mod > 0 && r % skip_mod == 0) return;                           // rows already updated (the CLS rows)
    const int col = (int)(i - r * half_d) * 2;
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    float2 v = *reinterpret_cast<const float2*>(x + r * ldx + col);
    const f16x2 d = *reinterpret_cast<const f16x2*>(delta + r * ldd + col);
    v.x += (float)d[0];
    v.y += (float)d[1];
    *reinterpret_cast<float2*>(x + r * ldx + col) = v;
}

// ------------------------------------------------------------------ noise (+ im2col of the patch embedding)
// Destination of pixel (c, y, x) in the im2col matrix: row = b*P + (y/ps)*(img/ps) + x/ps,
// column = c*ps*ps + (y%ps)*ps + x%ps   (= the flattening of Conv2d weight [D,3,ps,ps], eva_vit.py:202).
// Sample index of batch row b: first_sample + b for b < na, else first_b + (b - na) (two index ranges in one batch:
// the selection and estimation draws of Smooth.certify, smoothing.py:44,48).
// Several images (per > 0): the rows of ALL images form one image-major sequence, image i owning rows [i*per, (i+1)*per)
// with the same two-range split; it reads the clean image src + i*3*img*img and shifts both ranges by i*img_stride sample
// indices.  A batch is any window of that sequence: batch row b is sequence row row0 + b, so batches need not start or end
// at image boundaries (the batch size can then be chosen for the GEMMs' tile quantisation, not for the image's draw count).
// One workgroup per (batch row b, patch row py): it reads the 3 x ps image rows of that patch row with coalesced float4
// loads, adds the noise, and stages the fp16 values of the img/ps patches in LDS as [patch][c*ps*ps + iy*ps + ix]; every
// patch row of A (3*ps*ps contiguous halfs = 1176 B at ps = 14) then leaves in 8-byte vector stores, one row after the other
// (the direct form wrote 2-byte stores scattered over img/ps rows per pixel group).  The noise of pixel group `grp` depends
// only on (seed, sample, grp), so the values are the ones the direct form produced.
// LAW: NOISE_NONE (plain im2col), NOISE_GAUSSIAN (x + sigma * z) or NOISE_UNIFORM (x + sigma * u, u in [0,1); philox.h).
template <int LAW>
__global__ __launch_bounds__(256) void im2col_kernel(const float* __restrict__ src, int img, int ps,
                                                     int64_t first_sample, int na, int64_t first_b, int nb, float sigma,
                                                     uint64_t seed, half_t* __restrict__ A, int64_t lda, int per,
                                                     int64_t img_stride, int64_t row0) {
    constexpr bool NOISE = LAW != NOISE_NONE;
    extern __shared__ __attribute__((aligned(16))) half_t patch_lds[];   // [pw][kp]
    const int pw = img / ps, kp = 3 * ps * ps;
    const int b = blockIdx.x / pw, py = blockIdx.x - b * pw;
    // NOISE: src is the clean image(s) x[.,3,img,img]; else src is the batch [nb,3,img,img]
    const int64_t rs = row0 + b;                                 // row in the sequence of all images
    const int im = (NOISE && per > 0) ? (int)(rs / per) : 0, j = (NOISE && per > 0) ? (int)(rs - (int64_t)im * per) : b;
    const float* image = src + (NOISE ? (int64_t)im : (int64_t)b) * 3 * img * img;
    const int64_t sample = NOISE ? (j < na ? first_sample + j : first_b + (j - na)) + im * img_stride : 0;
    const int xg_per_row = img >> 2, groups = 3 * ps * xg_per_row;        // float4 groups of this patch row
    for (int g = threadIdx.x; g < groups; g += 256) {
        const int c = g / (ps * xg_per_row), r = g - c * ps * xg_per_row;
        const int iy = r / xg_per_row, x0 = (r - iy * xg_per_row) << 2;
        const int e = (c * img + py * ps + iy) * img + x0;                // element index in the image; e/4 = noise group
        float4 px = *reinterpret_cast<const float4*>(image + e);
        if constexpr (NOISE) {
            const float4 z = noise4<LAW>(seed, (uint64_t)sample, (uint32_t)(e >> 2), 0u);
            // explicit fma: the fused path and cgpt_noise_batch must round identically (bit-identical votes)
            px.x = __fmaf_rn(sigma, z.x, px.x); px.y = __fmaf_rn(sigma, z.y, px.y);
            px.z = __fmaf_rn(sigma, z.z, px.z); px.w = __fmaf_rn(sigma, z.w, px.w);
            // keep the fp32 sum as its own value: otherwise hipcc fuses fma + f16 convert into v_fma_mixlo_f16 (ONE
            // rounding), while the reference rounds batch + noise to fp32 first and autocast then casts to fp16.
            asm volatile("" : "+v"(px.x), "+v"(px.y), "+v"(px.z), "+v"(px.w));
        }
        const float vals[4] = {px.x, px.y, px.z, px.w};
        const int col0 = c * ps * ps + iy * ps;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = x0 + k;
            const int pxi = x / ps, ix = x - pxi * ps;
            patch_lds[pxi * kp + col0 + ix] = (half_t)vals[k];
        }
    }
    __syncthreads();
    half_t* out = A + ((int64_t)b * pw * pw + (int64_t)py * pw) * lda;   // first of this block's pw rows of A
    if ((kp & 3) == 0 && (lda & 3) == 0) {
        typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
        const int q4 = kp >> 2;
        for (int i = threadIdx.x; i < pw * q4; i += 256) {
            const int pxi = i / q4, q = i - pxi * q4;
            *reinterpret_cast<f16x4*>(out + (int64_t)pxi * lda + q * 4) = *reinterpret_cast<const f16x4*>(patch_lds + pxi * kp + q * 4);
        }
    } else {
        for (int i = threadIdx.x; i < pw * kp; i += 256) {
            const int pxi = i / kp, q = i - pxi * kp;
            out[(int64_t)pxi * lda + q] = patch_lds[pxi * kp + q];
        }
    }
}

// out[b] = x + sigma * draw under LAW (NOISE_GAUSSIAN or NOISE_UNIFORM), with the fused path's single fma rounding.
template <int LAW>
__global__ __launch_bounds__(256) void noise_batch_kernel(const float* __restrict__ x, int64_t chw,
                                                          int64_t first_sample, int64_t num, float sigma,
                                                          uint64_t seed, float* __restrict__ out) {
    const int64_t groups = (chw + 3) / 4;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= groups * num) return;
    const int64_t b = gid / groups, grp = gid - b * groups;
    const float4 z = noise4<LAW>(seed, (uint64_t)(first_sample + b), (uint32_t)grp, 0u);
    const float zz[4] = {z.x, z.y, z.z, z.w};
    const int64_t e = grp * 4;
    if (e + 3 < chw && (chw & 3) == 0) {
        const float4 px = *reinterpret_cast<const float4*>(x + e);
        *reinterpret_cast<float4*>(out + b * chw + e) =
            make_float4(__fmaf_rn(sigma, zz[0], px.x), __fmaf_rn(sigma, zz[1], px.y), __fmaf_rn(sigma, zz[2], px.z),
                        __fmaf_rn(sigma, zz[3], px.w));
    } else {
        for (int k = 0; k < 4 && e + k < chw; ++k) out[b * chw + e + k] = __fmaf_rn(sigma, zz[k], x[e + k]);
    }
}

// One step of the random-gradient-free (RGF) black-box attack against the smoothed classifier (BASELINE configs[4]; the
// reference describes it in prose only, README.md:62-64,108-120 -- this update rule is build-side):
//   g[e]   = sum_i coeff[i] * u_{first_dir+i}[e]         (u_s = the N(0,1) draw of sample index s in the noise stream,
//                                                         i.e. exactly the direction cgpt_noise_batch(x, s, 1, delta) added)
//   out[e] = clamp(x_adv[e] + lr * sign(g[e]),  x_clean[e] - eps,  x_clean[e] + eps)
// Separate multiply and add (no contraction), directions in index order: the CPU oracle reproduces the sum bit for bit.
struct RgfCoeffs { float c[CGPT_RGF_MAX_DIRS]; };
__global__ __launch_bounds__(256) void rgf_step_kernel(const float* __restrict__ x_adv, const float* __restrict__ x_clean,
                                                       int64_t chw, int64_t first_dir, int q, RgfCoeffs coeffs, float lr,
                                                       float eps, uint64_t seed, float* __restrict__ out) {
    const int64_t grp = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (grp >= (chw + 3) / 4) return;
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < q; ++i) {
        const float4 z = normal4(seed, (uint64_t)(first_dir + i), (uint32_t)grp, 0u);
        const float zz[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = __fadd_rn(g[k], __fmul_rn(coeffs.c[i], zz[k]));
    }
    const int64_t e = grp * 4;
    for (int k = 0; k < 4 && e + k < chw; ++k) {
        const float sg = g[k] > 0.f ? 1.f : (g[k] < 0.f ? -1.f : 0.f);
        const float c = x_clean[e + k];
        const float v = __fadd_rn(x_adv[e + k], __fmul_rn(lr, sg));
        out[e + k] = fminf(fmaxf(v, c - eps), c + eps);
    }
}

__global__ void cls_rows_kernel(const float* __restrict__ cls, const float* __restrict__ pos,
                                float* __restrict__ resid, int64_t ld, int T, int nb, int D) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb * D) return;
    const int b = i / D, n = i - b * D;
    resid[(int64_t)b * T * ld + n] = cls[n] + pos[n];
}

__global__ void broadcast_rows_kernel(const float* __restrict__ src, int rows, int D, int nb,
                                      float* __restrict__ dst32, int64_t ld32, half_t* __restrict__ dst16, int64_t ld16) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)nb * rows * D) return;
    const int n = (int)(i % D);
    const int64_t br = i / D;                     // b*rows + r
    const float v = src[(br % rows) * D + n];
    dst32[br * ld32 + n] = v;
    dst16[br * ld16 + n] = (half_t)v;
}

__global__ void mean_rows_kernel(const float* __restrict__ src, int64_t lds, int rows, int D, int nb,
                                 half_t* __restrict__ dst16, int64_t ld16) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb * D) return;
    const int b = i / D, n = i - b * D;
    float s = 0.f;
    for (int r = 0; r < rows; ++r) s += src[((int64_t)b * rows + r) * lds + n];
    dst16[(int64_t)b * ld16 + n] = (half_t)(s / (float)rows);
}

// ------------------------------------------------------------------------------- argmax + vote histogram
// One wave per sample.  Each lane scans classes lane, lane+64, ... keeping the first maximum (strict >),
// then a 6-step xor-shuffle butterfly keeps (larger value, then smaller index): ndarray/tensor argmax semantics
// "first maximal index" (smoothing.py:97).  Lane 0 adds the vote with one 64-bit atomic (smoothing.py:98,101-105).
// per > 0: image-major batch of several images (see im2col_kernel): image i = s / per votes into counts + i*2K (first
// range) or counts_b + i*2K (second range): a [images, 2, K] table when counts_b = counts + K.
__global__ __launch_bounds__(256) void vote_kernel(const float* __restrict__ logits, int64_t ld, int64_t num, int K,
                                                   unsigned long long* __restrict__ counts, int64_t na,
                                                   unsigned long long* __restrict__ counts_b, int per, int64_t row0) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= num) return;
    const float* row = logits + s * ld;
    // torch.argmax / numpy argmax semantics (smoothing.py:97): a NaN ranks above every number, ties go to the lower index
    auto beats = [](float v, int i, float bv, int bi) {
        const bool vn = v != v, bn = bv != bv;
        if (vn != bn) return vn;
        if (vn) return i < bi;
        return v > bv || (v == bv && i < bi);
    };
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int k = lane; k < K; k += 64) {
        const float v = row[k];
        if (bi == 0x7fffffff || beats(v, k, best, bi)) { best = v; bi = k; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (beats(ov, oi, best, bi)) { best = ov; bi = oi; }
    }
    const int64_t rs = row0 + s;
    const int64_t im = per > 0 ? rs / per : 0, j = per > 0 ? rs - im * per : s;
    if (lane == 0) atomicAdd((j < na ? counts : counts_b) + im * 2 * K + bi, 1ull);   // rows >= na belong to the second range
}

// The vote of rows whose class is already known (the labels of the trie-constrained decode): counts[labels[i]] += 1, one thread per
// label, one 64-bit atomic each.  A label outside 0 .. K-1 is not counted.
__global__ __launch_bounds__(256) void vote_labels_kernel(const int* __restrict__ labels, int64_t num, int K,
                                                          unsigned long long* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= num) return;
    const int l = labels[i];
    if (l >= 0 && l < K) atomicAdd(counts + l, 1ull);
}


// ------------------------------------------------------------------- device-side finalisation of certify / predict
// One wave.  Smooth.certify lines 46-56 (smoothing.py): cAHat = first maximal index of the selection histogram
// (64 lanes scan K/64 classes each, then a 6-step xor-shuffle butterfly keeps (larger count, then smaller index)),
// nA = estimation[cAHat], Clopper-Pearson lower bound and the radius of the noise law (stats.h radius(): sigma * Phi^-1 or
// sigma * (p - 1/2)) in float64 by lane 0 (the same code the host path runs).  Smooth.predict lines 73-79: top-2 counts by two butterflies, two-sided binomial test.
// out[0] = label (as double), out[1] = radius (certify) or p-value (predict).
__global__ __launch_bounds__(64) void finalize_kernel(const long long* __restrict__ csel, const long long* __restrict__ cest,
                                                      int K, long long n, double alpha, double sigma, int law, int predict,
                                                      double* __restrict__ out) {
    const int lane = threadIdx.x;
    auto wave_argmax = [&](const long long* c, int skip) {
        long long best = -1;
        int bi = 0x7fffffff;
        for (int k = lane; k < K; k += 64) {
            if (k == skip) continue;
            const long long v = c[k];
            if (v > best) { best = v; bi = k; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const long long ov = __shfl_xor(best, o);
            const int oi = __shfl_xor(bi, o);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        return bi;
    };
    if (!predict) {
        const int cAHat = wave_argmax(csel, -1);
        if (lane == 0) {
            const long long nA = cest[cAHat];
            const double pABar = cgpt_stats::cp_lower_bound(nA, n, alpha);
            if (pABar < 0.5) { out[0] = -1.0; out[1] = 0.0; }
            else { out[0] = (double)cAHat; out[1] = cgpt_stats::radius(law, pABar, sigma); }
        }
    } else {
        const int i1 = wave_argmax(cest, -1);
        const int i2 = wave_argmax(cest, i1);
        if (lane == 0) {
            const long long c1 = cest[i1], c2 = cest[i2];
            const double pv = cgpt_stats::binom_test_two_sided(c1, c1 + c2, 0.5);
            out[0] = pv > alpha ? -1.0 : (double)i1;
            out[1] = pv;
        }
    }
}

// ------------------------------------------------------------------------------------- fills and casts
__global__ void fill_normal_kernel(void* dst, int is_f16, int64_t rows, int64_t cols, int64_t ld, float mean,
                                   float stdv, uint64_t seed, uint64_t tensor_id) {
    const int64_t groups = (rows * cols + 3) / 4;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= groups) return;
    const float4 z = normal4(seed, tensor_id, (uint32_t)gid, 1u + (uint32_t)(gid >> 32));
    const float zz[4] = {z.x, z.y, z.z, z.w};
    for (int k = 0; k < 4; ++k) {
        const int64_t e = gid * 4 + k;
        if (e >= rows * cols) break;
        const int64_t r = e / cols, c = e - r * cols;
        const float v = mean + stdv * zz[k];
        if (is_f16) reinterpret_cast<half_t*>(dst)[r * ld + c] = (half_t)v;
        else reinterpret_cast<float*>(dst)[r * ld + c] = v;
    }
}

__global__ void fill_const_kernel(float* dst, int64_t n, float v) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = v;
}

__global__ void f32_to_f16_kernel(const float* src, int64_t lds, half_t* dst, int64_t ldd, int64_t rows, int64_t cols) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cols) return;
    const int64_t r = i / cols, c = i - r * cols;
    dst[r * ldd + c] = (half_t)src[r * lds + c];
}

__global__ void f16_to_f32_kernel(const half_t* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int64_t cols) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cols) return;
    const int64_t r = i / cols, c = i - r * cols;
    dst[r * ldd + c] = (float)src[r * lds + c];
}

inline unsigned blocks_for(int64_t n, int per = 256) { return (unsigned)((n + per - 1) / per); }

}  // namespace

hipError_t launch_add_delta(float* x, int64_t ldx, const half_t* delta, int64_t ldd, int64_t rows, int D,
                            hipStream_t stream, int skip_mod) {
    if (rows <= 0) return hipSuccess;
    if ((D & 1) || (ldx & 1) || (ldd & 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(add_delta_kernel, dim3(blocks_for(rows * (D >> 1))), dim3(256), 0, stream, x, ldx, delta, ldd, rows, D, skip_mod);
    return hipGetLastError();
}

int g_ln_kernel = 1;

namespace {

struct LnArgs {
    float* x; int64_t ldx; const half_t* delta; int64_t ldd; const float* gamma; const float* beta; float eps;
    half_t* y16; int64_t ldy16; float* y32; int64_t ldy32; int64_t rows; const half_t* delta2; int64_t ldd2; hipStream_t stream;
};

inline hipError_t ln_device_cus(int& cus) {
    constexpr int kMaxDevicesLn = 64;
    static int table[kMaxDevicesLn] = {0};
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    if (dev < 0 || dev >= kMaxDevicesLn) return hipErrorInvalidDevice;
    if (table[dev] == 0) {
        int n = 0;
        if (hipError_t e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev); e != hipSuccess) return e;
        table[dev] = n > 0 ? n : 256;
    }
    cus = table[dev];
    return hipSuccess;
}

// One resident workgroup (4 waves, one per SIMD) per wave slot: WAVES workgroups per CU walk the row groups.
template <int NCH, bool HAS_D, bool HAS_D2, bool STORE_X, bool Y16, bool Y32, int SPLIT, int WAVES>
hipError_t launch_ln_rows(const LnArgs& a) {
    int cus = 0;
    if (hipError_t e = ln_device_cus(cus); e != hipSuccess) return e;
    const int64_t groups = (a.rows + 7) / 8, resident = (int64_t)cus * WAVES;
    hipLaunchKernelGGL((layernorm4_rows_kernel<NCH, HAS_D, HAS_D2, STORE_X, Y16, Y32, SPLIT, WAVES>),
                       dim3((unsigned)(groups < resident ? groups : resident)), dim3(256), 0, a.stream, a.x, a.ldx, a.delta, a.ldd, a.gamma,
                       a.beta, a.eps, a.y16, a.ldy16, a.y32, a.ldy32, a.rows, a.delta2, a.ldd2);
    return hipGetLastError();
}

// The forms the library launches at the ViT-G width (model.hip forward()); `variant` = ln_kernel (1 = the kept schedule per form,
// measured in profiles/r07/layernorm_rewrite.txt; lab builds: 10 + 3 * SPLIT + (WAVES - 4)).  false: no fast kernel for this form.
template <bool HAS_D, bool HAS_D2, bool STORE_X, int SPLIT, int WAVES>
bool launch_ln_vitg_form(const LnArgs& a, int variant, hipError_t& e) {
    if (variant == 1) { e = launch_ln_rows<11, HAS_D, HAS_D2, STORE_X, true, false, SPLIT, WAVES>(a); return true; }
#ifdef CGPT_LAB
#define CGPT_LNV(V, S, W) if (variant == V) { e = launch_ln_rows<11, HAS_D, HAS_D2, STORE_X, true, false, S, W>(a); return true; }
    CGPT_LNV(10, 0, 4) CGPT_LNV(11, 0, 5) CGPT_LNV(12, 0, 6) CGPT_LNV(13, 1, 4) CGPT_LNV(14, 1, 5) CGPT_LNV(15, 1, 6)
#undef CGPT_LNV
#endif
    return false;
}

// SPLIT, WAVES kept per form (profiles/r07/layernorm_rewrite.txt): the most waves that hold the row's loads without scratch --
// 74 VGPRs / 6 waves without an update, 94 / 5 with one, 117 / 4 with two or with the stream store.  One wave more spills and loses the gain.
#define CGPT_LN_KEPT_PLAIN 0, 6
#define CGPT_LN_KEPT_LN1 0, 5
#define CGPT_LN_KEPT_LN2 0, 4
// Every other form and every other width keeps layernorm4_body (the Q-Former's post-LNs, 8 160 rows of 768, were slower in the rows
// kernel: 13.9 against 12.0 us -- at one row group per workgroup the LDS staging is not paid back).
bool launch_ln_fast(const LnArgs& a, int nch, bool store, int variant, hipError_t& e) {
    const bool d = a.delta != nullptr, d2 = a.delta2 != nullptr;
    if (nch == 11 && a.y16 && !a.y32) {
        if (!d && !d2) return launch_ln_vitg_form<false, false, false, CGPT_LN_KEPT_PLAIN>(a, variant, e);     // block 0 LN1
        if (d && !d2 && !store) return launch_ln_vitg_form<true, false, false, CGPT_LN_KEPT_LN1>(a, variant, e);   // LN1
        if (d && d2 && store) return launch_ln_vitg_form<true, true, true, CGPT_LN_KEPT_LN2>(a, variant, e);       // LN2
        if (!d && d2 && store) return launch_ln_vitg_form<false, true, true, CGPT_LN_KEPT_LN2>(a, variant, e);     // block 0 LN2
        if (d && !d2 && store) return launch_ln_vitg_form<true, false, true, CGPT_LN_KEPT_LN2>(a, variant, e);     // ln_vision
        return false;
    }
    return false;
}

}  // namespace

hipError_t launch_layernorm(float* x, int64_t ldx, const half_t* delta, int64_t ldd, const float* gamma,
                            const float* beta, float eps, half_t* y16, int64_t ldy16, float* y32, int64_t ldy32,
                            int64_t rows, int D, hipStream_t stream, const half_t* delta2, int64_t ldd2, int keep_x) {
    if (rows <= 0) return hipSuccess;
    if (D <= 0 || (D & 1) || D > 32 * 128 || (ldx & 1) || (ldy16 & 1) || (ldy32 & 1) || (ldd & 1) || (ldd2 & 1)) return hipErrorInvalidValue;
    // 16-byte path: D a multiple of 128 (1408 = 11 x 128, 768 = 6 x 128, 4096) and 16-byte aligned rows
    if ((D % 128) == 0 && D / 128 <= 32 && (ldx % 4) == 0 && (ldd % 4) == 0 && (ldd2 % 4) == 0 && (ldy16 % 4) == 0 && (ldy32 % 4) == 0) {
        if (g_ln_kernel != 0) {
            const LnArgs a{x, ldx, delta, ldd, gamma, beta, eps, y16, ldy16, y32, ldy32, rows, delta2, ldd2, stream};
            hipError_t e = hipSuccess;
            if (launch_ln_fast(a, D / 128, (delta || delta2) && !keep_x, g_ln_kernel, e)) return e;
        }
        dim3 grid4((unsigned)((rows + 7) / 8)), block4(256);
#define CGPT_LN4(NCH) hipLaunchKernelGGL(layernorm4_kernel<NCH>, grid4, block4, 0, stream, x, ldx, delta, ldd, gamma, beta, eps, \
                                         y16, ldy16, y32, ldy32, rows, D, delta2, ldd2, keep_x)
        const int n = D / 128;
        if (n <= 1) CGPT_LN4(1);
        else if (n <= 6) { if (n == 6) CGPT_LN4(6); else goto generic; }
        else if (n == 11) hipLaunchKernelGGL(layernorm4_vitg_kernel, grid4, block4, 0, stream, x, ldx, delta, ldd, gamma, beta, eps,
                                             y16, ldy16, y32, ldy32, rows, D, delta2, ldd2, keep_x);
        else if (n == 32) CGPT_LN4(32);
        else goto generic;
#undef CGPT_LN4
        return hipGetLastError();
    }
generic:
    dim3 grid((unsigned)((rows + 3) / 4)), block(256);
#define CGPT_LN(NCH) hipLaunchKernelGGL(layernorm_kernel<NCH>, grid, block, 0, stream, x, ldx, delta, ldd, gamma, beta, eps, \
                                        y16, ldy16, y32, ldy32, rows, D, delta2, ldd2, keep_x)
    if (D <= 2 * 128) CGPT_LN(2);
    else if (D <= 6 * 128) CGPT_LN(6);
    else if (D <= 11 * 128) CGPT_LN(11);
    else if (D <= 16 * 128) CGPT_LN(16);
    else CGPT_LN(32);
#undef CGPT_LN
    return hipGetLastError();
}

hipError_t launch_noise_im2col(const float* x, int img, int ps, int64_t first_sample, int na, int64_t first_b, int nb,
                               float sigma, uint64_t seed, half_t* A, int64_t lda, hipStream_t stream, int per,
                               int64_t img_stride, int64_t row0, int law) {
    if (nb <= 0) return hipSuccess;
    if ((img & 3) || (img % ps) || (law != NOISE_GAUSSIAN && law != NOISE_UNIFORM)) return hipErrorInvalidValue;
    const int pw = img / ps;
    hipLaunchKernelGGL(law == NOISE_UNIFORM ? im2col_kernel<NOISE_UNIFORM> : im2col_kernel<NOISE_GAUSSIAN>, dim3((unsigned)(nb * pw)),
                       dim3(256), (size_t)pw * 3 * ps * ps * sizeof(half_t), stream, x, img, ps, first_sample, na, first_b, nb, sigma,
                       seed, A, lda, per, img_stride, row0);
    return hipGetLastError();
}

hipError_t launch_im2col(const float* images, int img, int ps, int nb, half_t* A, int64_t lda, hipStream_t stream) {
    if (nb <= 0) return hipSuccess;
    if ((img & 3) || (img % ps)) return hipErrorInvalidValue;
    const int pw = img / ps;
    hipLaunchKernelGGL(im2col_kernel<NOISE_NONE>, dim3((unsigned)(nb * pw)), dim3(256), (size_t)pw * 3 * ps * ps * sizeof(half_t), stream,
                       images, img, ps, (int64_t)0, nb, (int64_t)0, nb, 0.0f, (uint64_t)0, A, lda, 0, (int64_t)0, (int64_t)0);
    return hipGetLastError();
}

hipError_t launch_noise_batch(const float* x, int64_t chw, int64_t first_sample, int64_t num, float sigma,
                              uint64_t seed, float* out, hipStream_t stream, int law) {
    if (law != NOISE_GAUSSIAN && law != NOISE_UNIFORM) return hipErrorInvalidValue;
    if (num <= 0) return hipSuccess;
    const int64_t n = ((chw + 3) / 4) * num;
    hipLaunchKernelGGL(law == NOISE_UNIFORM ? noise_batch_kernel<NOISE_UNIFORM> : noise_batch_kernel<NOISE_GAUSSIAN>, dim3(blocks_for(n)),
                       dim3(256), 0, stream, x, chw, first_sample, num, sigma, seed, out);
    return hipGetLastError();
}

hipError_t launch_rgf_step(const float* x_adv, const float* x_clean, int64_t chw, int64_t first_dir, int q, const float* coeffs,
                           float lr, float eps, uint64_t seed, float* out, hipStream_t stream) {
    if (q < 0 || q > CGPT_RGF_MAX_DIRS) return hipErrorInvalidValue;
    RgfCoeffs c;
    for (int i = 0; i < CGPT_RGF_MAX_DIRS; ++i) c.c[i] = i < q ? coeffs[i] : 0.f;
    hipLaunchKernelGGL(rgf_step_kernel, dim3(blocks_for((chw + 3) / 4)), dim3(256), 0, stream, x_adv, x_clean, chw, first_dir, q,
                       c, lr, eps, seed, out);
    return hipGetLastError();
}

hipError_t launch_cls_rows(const float* cls, const float* pos, float* resid, int64_t ld, int T, int nb, int D,
                           hipStream_t stream) {
    hipLaunchKernelGGL(cls_rows_kernel, dim3(blocks_for((int64_t)nb * D)), dim3(256), 0, stream, cls, pos, resid, ld, T,
                       nb, D);
    return hipGetLastError();
}

hipError_t launch_broadcast_rows(const float* src, int rows, int D, int nb, float* dst32, int64_t ld32, half_t* dst16,
                                 int64_t ld16, hipStream_t stream) {
    hipLaunchKernelGGL(broadcast_rows_kernel, dim3(blocks_for((int64_t)nb * rows * D)), dim3(256), 0, stream, src, rows,
                       D, nb, dst32, ld32, dst16, ld16);
    return hipGetLastError();
}

hipError_t launch_mean_rows(const float* src, int64_t lds, int rows, int D, int nb, half_t* dst16, int64_t ld16,
                            hipStream_t stream) {
    hipLaunchKernelGGL(mean_rows_kernel, dim3(blocks_for((int64_t)nb * D)), dim3(256), 0, stream, src, lds, rows, D, nb,
                       dst16, ld16);
    return hipGetLastError();
}

hipError_t launch_vote(const float* logits, int64_t ld, int64_t num, int K, int64_t* counts, int64_t na, int64_t* counts_b,
                       hipStream_t stream, int per, int64_t row0) {
    if (num <= 0) return hipSuccess;
    hipLaunchKernelGGL(vote_kernel, dim3((unsigned)((num + 3) / 4)), dim3(256), 0, stream, logits, ld, num, K,
                       reinterpret_cast<unsigned long long*>(counts), na, reinterpret_cast<unsigned long long*>(counts_b), per, row0);
    return hipGetLastError();
}

hipError_t launch_vote_labels(const int* labels, int64_t num, int K, int64_t* counts, hipStream_t stream) {
    if (num <= 0) return hipSuccess;
    hipLaunchKernelGGL(vote_labels_kernel, dim3(blocks_for(num)), dim3(256), 0, stream, labels, num, K,
                       reinterpret_cast<unsigned long long*>(counts));
    return hipGetLastError();
}

hipError_t launch_finalize(const int64_t* csel, const int64_t* cest, int K, int64_t n, double alpha, double sigma, int predict,
                           double* out, hipStream_t stream, int law) {
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(64), 0, stream, reinterpret_cast<const long long*>(csel),
                       reinterpret_cast<const long long*>(cest), K, (long long)n, alpha, sigma, law, predict, out);
    return hipGetLastError();
}

hipError_t launch_fill_normal(void* dst, int is_f16, int64_t rows, int64_t cols, int64_t ld, float mean, float stdv,
                              uint64_t seed, uint64_t tensor_id, hipStream_t stream) {
    const int64_t groups = (rows * cols + 3) / 4;
    if (groups <= 0) return hipSuccess;
    hipLaunchKernelGGL(fill_normal_kernel, dim3(blocks_for(groups)), dim3(256), 0, stream, dst, is_f16, rows, cols, ld,
                       mean, stdv, seed, tensor_id);
    return hipGetLastError();
}

hipError_t launch_fill_const(float* dst, int64_t n, float v, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(fill_const_kernel, dim3(blocks_for(n)), dim3(256), 0, stream, dst, n, v);
    return hipGetLastError();
}

hipError_t launch_f32_to_f16(const float* src, int64_t lds, half_t* dst, int64_t ldd, int64_t rows, int64_t cols,
                             hipStream_t stream) {
    if (rows * cols <= 0) return hipSuccess;
    hipLaunchKernelGGL(f32_to_f16_kernel, dim3(blocks_for(rows * cols)), dim3(256), 0, stream, src, lds, dst, ldd, rows,
                       cols);
    return hipGetLastError();
}

hipError_t launch_f16_to_f32(const half_t* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int64_t cols,
                             hipStream_t stream) {
    if (rows * cols <= 0) return hipSuccess;
    hipLaunchKernelGGL(f16_to_f32_kernel, dim3(blocks_for(rows * cols)), dim3(256), 0, stream, src, lds, dst, ldd, rows,
                       cols);
    return hipGetLastError();
}

}  // namespace cgpt
