// llm_gemm.hip -- the decode-shape GEMM of the LLaMA token step: C[M <= 256, N] = A[M, K] * W[N, K]^T, fp16 operands, fp32
// accumulation, epilogues that round where HF's fp16 eager model rounds (llm.h, DESIGN.md "LLaMA decode steps").
//
// Why another GEMM: a token step of a 200-row Monte-Carlo batch multiplies ONE row tile by 33-180 MB of weights.  The ViT
// dispatch (gemm.hip) sends M < 1024 to 128x128 tiles: 64 workgroups at N = 4096, a quarter of the chip, and the weight stream
// runs at what 64 CUs can pull.  Here a workgroup owns 64 weight rows (columns of C) x all 256 rows of A x one K slice, so
// N = 4096 is 64 column tiles x 4 K slices = 256 workgroups; N = 12288 / 22016 / 32000 are 192 / 344 / 500 workgroups of the
// whole K.  The weights are read exactly once; the A tile (<= 2 MB per slice, L2-resident) is re-read by every column tile.
//
// Tile 256 x 64 x 64, 8 waves, wave w owns rows 32w .. 32w+31 x the 64 columns = 2 x 4 tiles of v_mfma_f32_16x16x32_f16
// (waves whose rows lie at or past M stage their share and skip the MFMAs).  LDS images and the register-staged double buffer
// are those of gemm.hip's 128x128 kernel: [rows][64 halfs], 16-byte chunk index XOR (row >> 1) & 7.
//
// Split-K is deterministic by construction: slice s of a column tile writes its fp32 partial tile to slab s with plain vector
// stores, and decode_combine_kernel (a second launch: the kernel boundary is the release / acquire) adds slabs 0, 1, 2, ... in
// that order and applies the epilogue.  The number of slices depends on (N, K) only, so a row's result does not depend on M,
// on its neighbours, or on the launch.
//
// W8 (the second template parameter, int8 handles of llm.hip): W is the row-wise absmax int8 matrix q[N, K] with one fp16 scale per
// row.  Only the W staging differs: a thread loads the 8 bytes of its chunk, converts them to fp16 exactly (|q| <= 127) and forms
// W'[n, k] = fp16(q) * s_n with ONE packed fp16 multiply per pair -- the thread's row never changes, so s_n is one register loaded
// once -- and writes the same swizzled LDS image.  From there on the kernel is the fp16 kernel on W' (DESIGN.md 4.4.3).
//
// GUARD (the last template parameter, cgpt_llm_set_early_stop): the kernel reads *live -- one int, uniform over the
// grid, written by an earlier launch of the same stream -- before anything else and returns when it is 0: no load, no LDS write, no
// barrier, no store.  GUARD = false never looks at `live` (null) and is the kernel as it was: every other caller takes it.
#include "gemm_common.h"
#include "llm.h"

namespace cgpt {

namespace {

constexpr int DBM = 256, DBN = 64, DBK = 64;
constexpr int DSTAGE = DBM * DBK + DBN * DBK;            // halfs per LDS stage: A image + W image = 40 KiB
constexpr int DLDS_BYTES = 2 * DSTAGE * (int)sizeof(half_t);
constexpr int kTargetBlocks = 256;                       // one workgroup per CU of an MI355X; a constant, so that the slice
                                                         // count (and with it the summation order) is a property of the shape

__device__ __forceinline__ float round_f16(float v) { return (float)(half_t)v; }

__device__ __forceinline__ float silu_f16(float g) {     // silu on an fp16 value as torch evaluates it: fp32 inside, fp16 out
    return round_f16(g / (1.0f + expf(-g)));
}

template <int EPI>
__device__ __forceinline__ void decode_store(const DecodeGemmParams& p, int m, int n, float v) {
    if constexpr (EPI == DEC_F16) {
        reinterpret_cast<half_t*>(p.out)[(int64_t)m * p.ldo + n] = (half_t)v;
    } else if constexpr (EPI == DEC_F16_RESID) {
        const float r = (float)p.resid[(int64_t)m * p.ldr + n];
        reinterpret_cast<half_t*>(p.out)[(int64_t)m * p.ldo + n] = (half_t)(round_f16(v) + r);
    } else {  // DEC_F32
        reinterpret_cast<float*>(p.out)[(int64_t)m * p.ldo + n] = round_f16(v);
    }
}
__device__ __forceinline__ void decode_store_swiglu(const DecodeGemmParams& p, int m, int c, float gate, float up) {
    const float s = silu_f16(round_f16(gate));
    reinterpret_cast<half_t*>(p.out)[(int64_t)m * p.ldo + c] = (half_t)(s * round_f16(up));
}

typedef signed char i8x8 __attribute__((ext_vector_type(8)));

// W'[n, k .. k+7] = fp16(q) * s_n: the conversion is exact, the product is rounded once.  The barrier keeps the product a value of
// its own (nothing may be contracted or reassociated into it).
__device__ __forceinline__ f16x8 dequant8(i8x8 q, half_t s) {
    f16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (half_t)(short)q[e];
    v = v * s;
    asm volatile("" : "+v"(v));
    return v;
}

template <int EPI, bool W8, bool GUARD>
__global__ __launch_bounds__(512) void decode_gemm_kernel(DecodeGemmParams p, int tiles_n, int splitk, const half_t* __restrict__ wscale,
                                                          const int* __restrict__ live) {
    extern __shared__ __attribute__((aligned(16))) half_t dsmem[];   // [2 stages][A 256x64 | W 64x64]
    if constexpr (GUARD)
        if (*live == 0) return;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int r15 = lane & 15, g = lane >> 4;
    const int tn = blockIdx.x % tiles_n, slice = blockIdx.x / tiles_n;
    const int nkt = p.K / DBK;
    const int kt0 = (int)((int64_t)slice * nkt / splitk), kt1 = (int)((int64_t)(slice + 1) * nkt / splitk);
    const bool active = wave * 32 < p.M;                 // wave-uniform

    // ---- staging: thread -> row tid/8 (+ 64 i for A), 16-byte chunk tid%8
    const int ld_row = tid >> 3, ld_chunk = tid & 7;
    const half_t* a_src = p.A + (int64_t)ld_row * p.lda + ld_chunk * 8;
    const half_t* w_src = p.W + (int64_t)(tn * DBN + ld_row) * p.ldw + ld_chunk * 8;
    // W8: p.W points at int8 elements (ldw counts them); the row's scale is loaded once
    const signed char* q_src = reinterpret_cast<const signed char*>(p.W) + (int64_t)(tn * DBN + ld_row) * p.ldw + ld_chunk * 8;
    half_t wsc = (half_t)0.0f;
    if constexpr (W8) wsc = wscale[tn * DBN + ld_row];
    const int64_t a_step = 64 * p.lda;
    const int wr_off = ld_row * DBK + ((ld_chunk ^ ((ld_row >> 1) & 7)) << 3);   // +64 rows keeps the swizzle term

    const int sw = (r15 >> 1) & 7;
    const int k_off0 = ((g ^ sw) << 3), k_off1 = (((4 + g) ^ sw) << 3);
    const int a_rd = (wave * 32 + r15) * DBK;
    const int b_rd = DBM * DBK + r15 * DBK;

    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    f16x8 ra[4], rb;
    i8x8 rq;
    if (kt0 < kt1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) ra[i] = *reinterpret_cast<const f16x8*>(a_src + i * a_step + (int64_t)kt0 * DBK);
        if constexpr (W8) rq = *reinterpret_cast<const i8x8*>(q_src + (int64_t)kt0 * DBK);
        else rb = *reinterpret_cast<const f16x8*>(w_src + (int64_t)kt0 * DBK);
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<f16x8*>(dsmem + wr_off + i * 64 * DBK) = ra[i];
        if constexpr (W8) rb = dequant8(rq, wsc);
        *reinterpret_cast<f16x8*>(dsmem + DBM * DBK + wr_off) = rb;
    }
    __syncthreads();

    for (int kt = kt0; kt < kt1; ++kt) {
        const half_t* st = dsmem + ((kt - kt0) & 1) * DSTAGE;
        const bool more = (kt + 1 < kt1);
        if (more) {
#pragma unroll
            for (int i = 0; i < 4; ++i) ra[i] = *reinterpret_cast<const f16x8*>(a_src + i * a_step + (int64_t)(kt + 1) * DBK);
            if constexpr (W8) rq = *reinterpret_cast<const i8x8*>(q_src + (int64_t)(kt + 1) * DBK);
            else rb = *reinterpret_cast<const f16x8*>(w_src + (int64_t)(kt + 1) * DBK);
        }
        if (active) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int ko = ks ? k_off1 : k_off0;
                f16x8 af[2], bf[4];
#pragma unroll
                for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const f16x8*>(st + a_rd + i * 16 * DBK + ko);
#pragma unroll
                for (int j = 0; j < 4; ++j) bf[j] = *reinterpret_cast<const f16x8*>(st + b_rd + j * 16 * DBK + ko);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
            }
        }
        if (more) {
            half_t* dn = dsmem + ((kt + 1 - kt0) & 1) * DSTAGE;
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<f16x8*>(dn + wr_off + i * 64 * DBK) = ra[i];
            if constexpr (W8) rb = dequant8(rq, wsc);
            *reinterpret_cast<f16x8*>(dn + DBM * DBK + wr_off) = rb;
        }
        __syncthreads();
    }
    if (!active) return;

    // ---- C/D map of v_mfma_f32_16x16x32: column = lane & 15, row = 4 * (lane >> 4) + reg
    const int m_base = wave * 32 + 4 * g;
    const int n_base = tn * DBN + r15;
    if (splitk > 1) {
        float* slab = p.slabs + (int64_t)slice * DBM * p.N;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m_base + i * 16 + r;
                if (m >= p.M) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) slab[(int64_t)m * p.N + n_base + j * 16] = acc[i][j][r];
            }
        return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m_base + i * 16 + r;
            if (m >= p.M) continue;
            if constexpr (EPI == DEC_SWIGLU) {
#pragma unroll
                for (int j = 0; j < 4; j += 2)
                    decode_store_swiglu(p, m, tn * (DBN / 2) + (j / 2) * 16 + r15, acc[i][j][r], acc[i][j + 1][r]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) decode_store<EPI>(p, m, n_base + j * 16, acc[i][j][r]);
            }
        }
}

// out = epilogue(slab 0 + slab 1 + ... + slab splitk-1), summed in that order.  One thread per 4 consecutive output columns.
template <int EPI, bool GUARD>
__global__ __launch_bounds__(256) void decode_combine_kernel(DecodeGemmParams p, int splitk, const int* __restrict__ live) {
    if constexpr (GUARD)
        if (*live == 0) return;
    const int ncols = (EPI == DEC_SWIGLU) ? p.N / 2 : p.N;
    const int per_row = ncols / 4;
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (int64_t)p.M * per_row) return;
    const int m = (int)(id / per_row), c = (int)(id % per_row) * 4;
    const int64_t slab_stride = (int64_t)DBM * p.N;
    if constexpr (EPI == DEC_SWIGLU) {
        const int ng = (c >> 4) * 32 + (c & 15);                       // gate column of the interleaved product; up = + 16
        const float* s = p.slabs + (int64_t)m * p.N + ng;
        f32x4 gv = *reinterpret_cast<const f32x4*>(s), uv = *reinterpret_cast<const f32x4*>(s + 16);
        for (int k = 1; k < splitk; ++k) {
            gv += *reinterpret_cast<const f32x4*>(s + k * slab_stride);
            uv += *reinterpret_cast<const f32x4*>(s + k * slab_stride + 16);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) decode_store_swiglu(p, m, c + e, gv[e], uv[e]);
    } else {
        const float* s = p.slabs + (int64_t)m * p.N + c;
        f32x4 v = *reinterpret_cast<const f32x4*>(s);
        for (int k = 1; k < splitk; ++k) v += *reinterpret_cast<const f32x4*>(s + k * slab_stride);
#pragma unroll
        for (int e = 0; e < 4; ++e) decode_store<EPI>(p, m, c + e, v[e]);
    }
}

template <int EPI, bool W8, bool GUARD>
hipError_t launch_epi(const DecodeGemmParams& p, int splitk, const half_t* wscale, const int* live, hipStream_t stream) {
    const int tiles_n = p.N / DBN;
    hipLaunchKernelGGL((decode_gemm_kernel<EPI, W8, GUARD>), dim3(tiles_n * splitk), dim3(512), DLDS_BYTES, stream, p, tiles_n, splitk, wscale,
                       live);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || splitk == 1) return e;
    const int ncols = (EPI == DEC_SWIGLU) ? p.N / 2 : p.N;
    const int64_t threads = (int64_t)p.M * (ncols / 4);
    hipLaunchKernelGGL((decode_combine_kernel<EPI, GUARD>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, p, splitk, live);
    return hipGetLastError();
}

template <bool GUARD>
hipError_t launch_guard(int epilogue, const DecodeGemmParams& p, int splitk, const half_t* wscale, const int* live, hipStream_t stream) {
    if (wscale) {                                          // int8 weights: the three layer epilogues (lm_head stays fp16)
        switch (epilogue) {
            case DEC_F16: return launch_epi<DEC_F16, true, GUARD>(p, splitk, wscale, live, stream);
            case DEC_F16_RESID: return launch_epi<DEC_F16_RESID, true, GUARD>(p, splitk, wscale, live, stream);
            case DEC_SWIGLU: return launch_epi<DEC_SWIGLU, true, GUARD>(p, splitk, wscale, live, stream);
            default: return hipErrorInvalidValue;
        }
    }
    switch (epilogue) {
        case DEC_F16: return launch_epi<DEC_F16, false, GUARD>(p, splitk, nullptr, live, stream);
        case DEC_F16_RESID: return launch_epi<DEC_F16_RESID, false, GUARD>(p, splitk, nullptr, live, stream);
        case DEC_SWIGLU: return launch_epi<DEC_SWIGLU, false, GUARD>(p, splitk, nullptr, live, stream);
        case DEC_F32: return launch_epi<DEC_F32, false, GUARD>(p, splitk, nullptr, live, stream);
        default: return hipErrorInvalidValue;
    }
}

template <bool GUARD>
hipError_t prepare_guard() {
    const void* kernels[7] = {reinterpret_cast<const void*>(decode_gemm_kernel<DEC_F16, false, GUARD>),
                              reinterpret_cast<const void*>(decode_gemm_kernel<DEC_F16_RESID, false, GUARD>),
                              reinterpret_cast<const void*>(decode_gemm_kernel<DEC_SWIGLU, false, GUARD>),
                              reinterpret_cast<const void*>(decode_gemm_kernel<DEC_F32, false, GUARD>),
                              reinterpret_cast<const void*>(decode_gemm_kernel<DEC_F16, true, GUARD>),
                              reinterpret_cast<const void*>(decode_gemm_kernel<DEC_F16_RESID, true, GUARD>),
                              reinterpret_cast<const void*>(decode_gemm_kernel<DEC_SWIGLU, true, GUARD>)};
    for (const void* k : kernels) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, DLDS_BYTES);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t decode_gemm_prepare() {
    const hipError_t e = prepare_guard<false>();
    return e != hipSuccess ? e : prepare_guard<true>();
}

int decode_gemm_splitk(int N, int K) {
    const int tiles = N / DBN, nkt = K / DBK;
    int s = 1;
    while (s < 8 && tiles * s * 2 <= kTargetBlocks && nkt / (s * 2) >= 4) s *= 2;   // a slice is at least 4 K-tiles deep
    return s;
}

size_t decode_gemm_slab_bytes(int N, int K) {
    const int s = decode_gemm_splitk(N, K);
    return s > 1 ? (size_t)s * DBM * (size_t)N * sizeof(float) : 0;
}

hipError_t launch_decode_gemm(int epilogue, const DecodeGemmParams& p, hipStream_t stream, const half_t* wscale, const int* live) {
    if (p.M < 1 || p.M > DBM || p.N < DBN || p.N % DBN || p.K < DBK || p.K % DBK || !p.A || !p.W || !p.out)
        return hipErrorInvalidValue;
    if (epilogue == DEC_F16_RESID && !p.resid) return hipErrorInvalidValue;
    const int splitk = decode_gemm_splitk(p.N, p.K);
    if (splitk > 1 && !p.slabs) return hipErrorInvalidValue;
    return live ? launch_guard<true>(epilogue, p, splitk, wscale, live, stream) : launch_guard<false>(epilogue, p, splitk, wscale, nullptr, stream);
}

}  // namespace cgpt
