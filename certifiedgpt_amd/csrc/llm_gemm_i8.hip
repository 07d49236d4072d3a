// llm_gemm_i8.hip -- the int8-activation linear of an activations-int8 handle (cgpt_llm_config_act.act_format = 1):
// row-wise int8 activations against the row-wise int8 weights of an int8 handle, int32 accumulation on v_mfma_i32_16x16x64_i8, and a
// mixed-precision term for the outlier features of every row.  The law, per input row x[K] (fp16), weight q[N, K] with fp16 row scales
// s_w[N], threshold t:
//   1. k is an outlier iff t > 0 and |x_k| >= t
//   2. s_a = max_{k not outlier} |x_k| / 127                          fp32 division, correctly rounded; kept in fp32
//   3. a_k = clamp(rint(fp32(x_k) / s_a), -127, 127), 0 for outliers; the whole row 0 when s_a == 0
//   4. acc_n = sum_k a_k q_nk                                          int32: exact in any order (127^2 K < 2^31 for K <= 65536)
//   5. y_n = fp32(acc_n) * (s_a * fp32(s_w[n]))                        two fp32 multiplies, the inner one first
//   6. o_n = sum_{k outlier, ascending} fp32(x_k) * fp32(W'_nk),  W'_nk = fp16(q_nk) * s_w[n] (one fp16 multiply); sequential fp32
//      from 0.0f; every product is exact in fp32
//   7. v_n = y_n + o_n, then the epilogue rounds where the fp16 decode GEMM's does (DEC_F16 / DEC_F16_RESID / DEC_SWIGLU, llm.h)
// Because step 4 is exact, a row's result does not depend on the tile shape, the K split or the row tile it sits in: the token step,
// the prefill and the scoring pass compute the same linear bit for bit, and the whole is pinned bit for bit against plain torch
// (`llm_int8_linear`, minigpt4.py; tests/test_gpu_llm_act_int8.py).
//
// Two kernels and a combine:
//   llm_act_quant_kernel  one workgroup per row: steps 1-3, the row's outlier list (count + up to `cap` entries (k, fp16 bits) in
//                         ascending k: a prefix count per pass, wave and lane -- no atomics in the order), four statistics counters.
//                         A row with more than `cap` outliers keeps its first `cap` and is counted in overflow_rows; the ones past the
//                         cap are dropped (their codes are 0): the result is finite, memory-safe and NOT the law's -- callers raise.
//   llm_i8_gemm_kernel    decode_gemm_kernel (llm_gemm.hip) moved to int8: tile 256 rows x 64 columns x 128 BYTES of K, the same
//                         [rows][128 B] LDS image with the 16-byte chunk index XOR (row >> 1) & 7, 8 waves x (2 x 4) tiles of
//                         v_mfma_i32_16x16x64_i8; both operands are copied as bytes (no conversion in the staging thread).  A lane
//                         hands the instruction the SAME 16-byte chunk of its A row and of its W row, so whichever k the hardware
//                         assigns to a lane's bytes, every k of the tile is multiplied with its partner exactly once.  blockIdx.y
//                         walks 256-row tiles of A: one launch serves the token step (one tile) and the prefill (M = B L).
//   llm_i8_combine_kernel split-K slices write int32 slabs; this adds them in slice order (any order is exact) and applies 5-7.
// The slice count is a function of (N, K) only and 1 when there is more than one row tile.  Steps 5-7 are ONE device function used by
// the GEMM's store (one slice) and by the combine.
// GUARD: as everywhere in the token step, the kernel reads *live first and returns when it is 0.
#include "gemm_common.h"
#include "llm.h"

namespace cgpt {

namespace {

constexpr int IBM = 256, IBN = 64, IBK = 128;            // IBK in bytes = int8 elements
constexpr int ISTAGE = IBM * IBK + IBN * IBK;            // bytes per LDS stage: A image + W image = 40 KiB
constexpr int ILDS_BYTES = 2 * ISTAGE;
constexpr int kI8TargetBlocks = 256;

typedef signed char i8x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 q_h16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float i8_round_f16(float v) { return (float)(half_t)v; }
__device__ __forceinline__ float i8_silu_f16(float g) { return i8_round_f16(g / (1.0f + expf(-g))); }

// ------------------------------------------------------------------------------------------------- the quantiser
template <bool GUARD>
__global__ __launch_bounds__(256) void llm_act_quant_kernel(const half_t* __restrict__ x, int K, float thr, int cap,
                                                            signed char* __restrict__ a8, float* __restrict__ sa,
                                                            uint32_t* __restrict__ lists, unsigned long long* __restrict__ counters,
                                                            const int* __restrict__ live) {
    __shared__ float wmax[4];
    __shared__ int wcnt[4];
    if constexpr (GUARD)
        if (*live == 0) return;
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const q_h16x8* src = reinterpret_cast<const q_h16x8*>(x + (int64_t)row * K);
    const bool split = thr > 0.0f;
    float amax = 0.0f;
    for (int i = tid; i < K / 8; i += 256) {
        const q_h16x8 v = src[i];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float f = fabsf((float)v[e]);
            if (!(split && f >= thr)) amax = fmaxf(amax, f);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    if (lane == 0) wmax[wave] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    const float s = __fdiv_rn(amax, 127.0f);
    if (tid == 0) sa[row] = s;

    i8x16* dst = reinterpret_cast<i8x16*>(a8 + (int64_t)row * K);
    uint32_t* list = lists + (int64_t)row * (cap + 1);
    int base = 0;                                          // outliers of the earlier passes (block-uniform)
    const int passes = (K / 16 + 255) / 256;
    for (int ps = 0; ps < passes; ++ps) {                  // pass ps covers chunks 256 ps .. 256 ps + 255: ascending k in thread order
        const int i = ps * 256 + tid;
        const bool in = i < K / 16;
        q_h16x8 lo{}, hi{};
        if (in) { lo = src[2 * i]; hi = src[2 * i + 1]; }
        i8x16 o;
        int mine = 0;
        uint32_t mask = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float f = (float)(e < 8 ? lo[e] : hi[e - 8]);
            const bool out = in && split && fabsf(f) >= thr;
            const float t = fminf(fmaxf(rintf(__fdiv_rn(f, s)), -127.0f), 127.0f);
            o[e] = (out || s == 0.0f) ? (signed char)0 : (signed char)(int)t;
            if (out) { mask |= 1u << e; ++mine; }
        }
        if (in) dst[i] = o;
        // exclusive prefix of `mine` over the wave, then over the waves
        int incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wcnt[wave] = incl;
        __syncthreads();
        int before = base + incl - mine;
        for (int w = 0; w < wave; ++w) before += wcnt[w];
        const int total = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        if (mine) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if (mask & (1u << e)) {
                    if (before < cap) {
                        const half_t hv = e < 8 ? lo[e] : hi[e - 8];
                        const uint32_t bits = (uint32_t)__builtin_bit_cast(unsigned short, hv);
                        list[1 + before] = (uint32_t)(i * 16 + e) | (bits << 16);
                    }
                    ++before;
                }
            }
        }
        base += total;
        __syncthreads();                                   // wcnt is rewritten by the next pass
    }
    if (tid == 0) {
        list[0] = (uint32_t)min(base, cap);
        atomicAdd(&counters[0], 1ull);
        if (base) {
            atomicAdd(&counters[1], (unsigned long long)base);
            atomicMax(&counters[2], (unsigned long long)base);
        }
        if (base > cap) atomicAdd(&counters[3], 1ull);
    }
}

// ------------------------------------------------------------------------------------------------- steps 5-7 and the stores
// v = fp32(acc) * (s_a * fp32(s_w[n])) + o: the products and the sum are values of their own (nothing is contracted into an fma).
__device__ __forceinline__ float i8_value(const I8GemmParams& p, int64_t m, int n, int acc) {
    const float sw = (float)p.wscale[n];
    float sc = p.sa[m] * sw;
    asm volatile("" : "+v"(sc));
    float y = (float)acc * sc;
    asm volatile("" : "+v"(y));
    const uint32_t* list = p.lists + m * (p.cap + 1);
    const int cnt = (int)list[0];
    if (cnt == 0) return y + 0.0f;
    const half_t swh = p.wscale[n];
    const signed char* qrow = p.W + (int64_t)n * p.ldw;
    float o = 0.0f;
    for (int i = 0; i < cnt; ++i) {
        const uint32_t e = list[1 + i];
        const int k = (int)(e & 0xffffu);
        const half_t xv = __builtin_bit_cast(half_t, (unsigned short)(e >> 16));
        half_t wp = (half_t)(short)qrow[k] * swh;          // W' = fp16(q) * s_w: one fp16 multiply
        asm volatile("" : "+v"(wp));
        float pr = (float)xv * (float)wp;                  // exact in fp32
        asm volatile("" : "+v"(pr));
        o += pr;
    }
    return y + o;
}

template <int EPI>
__device__ __forceinline__ void i8_store(const I8GemmParams& p, int64_t m, int n, float v) {
    if constexpr (EPI == DEC_F16) {
        p.out[m * p.ldo + n] = (half_t)v;
    } else {  // DEC_F16_RESID
        const float r = (float)p.resid[m * p.ldr + n];
        p.out[m * p.ldo + n] = (half_t)(i8_round_f16(v) + r);
    }
}
__device__ __forceinline__ void i8_store_swiglu(const I8GemmParams& p, int64_t m, int c, float gate, float up) {
    const float s = i8_silu_f16(i8_round_f16(gate));
    p.out[m * p.ldo + c] = (half_t)(s * i8_round_f16(up));
}

// ------------------------------------------------------------------------------------------------- the GEMM
template <int EPI, bool GUARD>
__global__ __launch_bounds__(512) void llm_i8_gemm_kernel(I8GemmParams p, int tiles_n, int splitk, const int* __restrict__ live) {
    extern __shared__ __attribute__((aligned(16))) signed char ismem[];   // [2 stages][A 256 x 128 B | W 64 x 128 B]
    if constexpr (GUARD)
        if (*live == 0) return;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int r15 = lane & 15, g = lane >> 4;
    const int tn = blockIdx.x % tiles_n, slice = blockIdx.x / tiles_n;
    const int64_t row0 = (int64_t)blockIdx.y * IBM;        // first row of this workgroup's row tile
    const int Mt = (int)((int64_t)p.M - row0 < IBM ? (int64_t)p.M - row0 : IBM);
    const int nkt = p.K / IBK;
    const int kt0 = (int)((int64_t)slice * nkt / splitk), kt1 = (int)((int64_t)(slice + 1) * nkt / splitk);
    const bool active = wave * 32 < Mt;                    // wave-uniform

    // ---- staging: thread -> row tid / 8 (+ 64 i for A), 16-byte chunk tid % 8.  A is readable for whole 256-row tiles.
    const int ld_row = tid >> 3, ld_chunk = tid & 7;
    const signed char* a_src = p.A + (row0 + ld_row) * p.lda + ld_chunk * 16;
    const signed char* w_src = p.W + (int64_t)(tn * IBN + ld_row) * p.ldw + ld_chunk * 16;
    const int64_t a_step = 64 * p.lda;
    const int wr_off = ld_row * IBK + ((ld_chunk ^ ((ld_row >> 1) & 7)) << 4);   // + 64 rows keeps the swizzle term

    const int sw = (r15 >> 1) & 7;
    const int k_off0 = ((g ^ sw) << 4), k_off1 = (((4 + g) ^ sw) << 4);
    const int a_rd = (wave * 32 + r15) * IBK;
    const int b_rd = IBM * IBK + r15 * IBK;

    i32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = i32x4{0, 0, 0, 0};

    i32x4 ra[4], rb;
    if (kt0 < kt1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) ra[i] = *reinterpret_cast<const i32x4*>(a_src + i * a_step + (int64_t)kt0 * IBK);
        rb = *reinterpret_cast<const i32x4*>(w_src + (int64_t)kt0 * IBK);
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<i32x4*>(ismem + wr_off + i * 64 * IBK) = ra[i];
        *reinterpret_cast<i32x4*>(ismem + IBM * IBK + wr_off) = rb;
    }
    __syncthreads();

    for (int kt = kt0; kt < kt1; ++kt) {
        const signed char* st = ismem + ((kt - kt0) & 1) * ISTAGE;
        const bool more = (kt + 1 < kt1);
        if (more) {
#pragma unroll
            for (int i = 0; i < 4; ++i) ra[i] = *reinterpret_cast<const i32x4*>(a_src + i * a_step + (int64_t)(kt + 1) * IBK);
            rb = *reinterpret_cast<const i32x4*>(w_src + (int64_t)(kt + 1) * IBK);
        }
        if (active) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int ko = ks ? k_off1 : k_off0;
                i32x4 af[2], bf[4];
#pragma unroll
                for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const i32x4*>(st + a_rd + i * 16 * IBK + ko);
#pragma unroll
                for (int j = 0; j < 4; ++j) bf[j] = *reinterpret_cast<const i32x4*>(st + b_rd + j * 16 * IBK + ko);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[i], bf[j], acc[i][j], 0, 0, 0);
            }
        }
        if (more) {
            signed char* dn = ismem + ((kt + 1 - kt0) & 1) * ISTAGE;
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<i32x4*>(dn + wr_off + i * 64 * IBK) = ra[i];
            *reinterpret_cast<i32x4*>(dn + IBM * IBK + wr_off) = rb;
        }
        __syncthreads();
    }
    if (!active) return;

    // ---- C/D map of v_mfma_*_16x16x*: column = lane & 15, row = 4 * (lane >> 4) + reg (the same for every data type)
    const int m_base = wave * 32 + 4 * g;
    const int n_base = tn * IBN + r15;
    if (splitk > 1) {                                      // one row tile only (launch_i8_gemm): row0 == 0
        int* slab = p.slabs + (int64_t)slice * IBM * p.N;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m_base + i * 16 + r;
                if (m >= Mt) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) slab[(int64_t)m * p.N + n_base + j * 16] = acc[i][j][r];
            }
        return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ml = m_base + i * 16 + r;
            if (ml >= Mt) continue;
            const int64_t m = row0 + ml;
            if constexpr (EPI == DEC_SWIGLU) {
#pragma unroll
                for (int j = 0; j < 4; j += 2)
                    i8_store_swiglu(p, m, tn * (IBN / 2) + (j / 2) * 16 + r15, i8_value(p, m, n_base + j * 16, acc[i][j][r]),
                                    i8_value(p, m, n_base + (j + 1) * 16, acc[i][j + 1][r]));
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) i8_store<EPI>(p, m, n_base + j * 16, i8_value(p, m, n_base + j * 16, acc[i][j][r]));
            }
        }
}

// out = epilogue(law(slab 0 + slab 1 + ... + slab splitk-1)), added in slice order.  One thread per 4 consecutive output columns.
template <int EPI, bool GUARD>
__global__ __launch_bounds__(256) void llm_i8_combine_kernel(I8GemmParams p, int splitk, const int* __restrict__ live) {
    if constexpr (GUARD)
        if (*live == 0) return;
    const int ncols = (EPI == DEC_SWIGLU) ? p.N / 2 : p.N;
    const int per_row = ncols / 4;
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (int64_t)p.M * per_row) return;
    const int m = (int)(id / per_row), c = (int)(id % per_row) * 4;
    const int64_t slab_stride = (int64_t)IBM * p.N;
    if constexpr (EPI == DEC_SWIGLU) {
        const int ng = (c >> 4) * 32 + (c & 15);                       // gate column of the interleaved product; up = + 16
        const int* s = p.slabs + (int64_t)m * p.N + ng;
        i32x4 gv = *reinterpret_cast<const i32x4*>(s), uv = *reinterpret_cast<const i32x4*>(s + 16);
        for (int k = 1; k < splitk; ++k) {
            gv += *reinterpret_cast<const i32x4*>(s + k * slab_stride);
            uv += *reinterpret_cast<const i32x4*>(s + k * slab_stride + 16);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) i8_store_swiglu(p, m, c + e, i8_value(p, m, ng + e, gv[e]), i8_value(p, m, ng + 16 + e, uv[e]));
    } else {
        const int* s = p.slabs + (int64_t)m * p.N + c;
        i32x4 v = *reinterpret_cast<const i32x4*>(s);
        for (int k = 1; k < splitk; ++k) v += *reinterpret_cast<const i32x4*>(s + k * slab_stride);
#pragma unroll
        for (int e = 0; e < 4; ++e) i8_store<EPI>(p, m, c + e, i8_value(p, m, c + e, v[e]));
    }
}

template <int EPI, bool GUARD>
hipError_t i8_launch_epi(const I8GemmParams& p, int splitk, int row_tiles, const int* live, hipStream_t stream) {
    const int tiles_n = p.N / IBN;
    hipLaunchKernelGGL((llm_i8_gemm_kernel<EPI, GUARD>), dim3(tiles_n * splitk, row_tiles), dim3(512), ILDS_BYTES, stream, p, tiles_n, splitk, live);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || splitk == 1) return e;
    const int ncols = (EPI == DEC_SWIGLU) ? p.N / 2 : p.N;
    const int64_t threads = (int64_t)p.M * (ncols / 4);
    hipLaunchKernelGGL((llm_i8_combine_kernel<EPI, GUARD>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, p, splitk, live);
    return hipGetLastError();
}

template <bool GUARD>
hipError_t i8_launch_guard(int epilogue, const I8GemmParams& p, int splitk, int row_tiles, const int* live, hipStream_t stream) {
    switch (epilogue) {
        case DEC_F16: return i8_launch_epi<DEC_F16, GUARD>(p, splitk, row_tiles, live, stream);
        case DEC_F16_RESID: return i8_launch_epi<DEC_F16_RESID, GUARD>(p, splitk, row_tiles, live, stream);
        case DEC_SWIGLU: return i8_launch_epi<DEC_SWIGLU, GUARD>(p, splitk, row_tiles, live, stream);
        default: return hipErrorInvalidValue;
    }
}

template <bool GUARD>
hipError_t i8_prepare_guard() {
    const void* kernels[3] = {reinterpret_cast<const void*>(llm_i8_gemm_kernel<DEC_F16, GUARD>),
                              reinterpret_cast<const void*>(llm_i8_gemm_kernel<DEC_F16_RESID, GUARD>),
                              reinterpret_cast<const void*>(llm_i8_gemm_kernel<DEC_SWIGLU, GUARD>)};
    for (const void* k : kernels) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, ILDS_BYTES);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t i8_gemm_prepare() {
    const hipError_t e = i8_prepare_guard<false>();
    return e != hipSuccess ? e : i8_prepare_guard<true>();
}

int i8_gemm_splitk(int N, int K) {
    const int tiles = N / IBN, nkt = K / IBK;
    int s = 1;
    while (s < 8 && tiles * s * 2 <= kI8TargetBlocks && nkt / (s * 2) >= 4) s *= 2;   // a slice is at least 4 K-tiles deep
    return s;
}

size_t i8_gemm_slab_bytes(int N, int K) {
    const int s = i8_gemm_splitk(N, K);
    return s > 1 ? (size_t)s * IBM * (size_t)N * sizeof(int) : 0;
}

hipError_t launch_act_quant(const half_t* x, int64_t rows, int K, float threshold, int cap, signed char* a8, float* sa, uint32_t* lists,
                            unsigned long long* counters, hipStream_t stream, const int* live) {
    if (rows < 1 || rows > 0x7fffffff || K < IBK || K % IBK || K > 65536 || cap < 1 || cap > 1024 || !x || !a8 || !sa || !lists || !counters)
        return hipErrorInvalidValue;
    if (live)
        hipLaunchKernelGGL(llm_act_quant_kernel<true>, dim3((unsigned)rows), dim3(256), 0, stream, x, K, threshold, cap, a8, sa, lists, counters, live);
    else
        hipLaunchKernelGGL(llm_act_quant_kernel<false>, dim3((unsigned)rows), dim3(256), 0, stream, x, K, threshold, cap, a8, sa, lists, counters,
                           nullptr);
    return hipGetLastError();
}

hipError_t launch_i8_gemm(int epilogue, const I8GemmParams& p, hipStream_t stream, const int* live) {
    if (p.M < 1 || p.N < IBN || p.N % IBN || p.K < IBK || p.K % IBK || p.K > 65536 || p.cap < 1 || p.cap > 1024 || !p.A || !p.W || !p.wscale ||
        !p.sa || !p.lists || !p.out)
        return hipErrorInvalidValue;
    if (epilogue == DEC_F16_RESID && !p.resid) return hipErrorInvalidValue;
    const int64_t row_tiles = ((int64_t)p.M + IBM - 1) / IBM;
    if (row_tiles > 65535) return hipErrorInvalidValue;
    const int splitk = row_tiles > 1 ? 1 : i8_gemm_splitk(p.N, p.K);
    if (splitk > 1 && !p.slabs) return hipErrorInvalidValue;
    return live ? i8_launch_guard<true>(epilogue, p, splitk, (int)row_tiles, live, stream)
                : i8_launch_guard<false>(epilogue, p, splitk, (int)row_tiles, nullptr, stream);
}

}  // namespace cgpt
