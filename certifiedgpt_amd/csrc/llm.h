// llm.h -- launchers of the LLaMA decode-step kernels (llm_gemm.hip, llm.hip).  All enqueue on `stream`, no host sync.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace cgpt {

// ------------------------------------------------------------------------------------- decode-shape GEMM
// C[M,N] = A[M,K] * W[N,K]^T for M <= 256 (one row tile), fp16 operands, fp32 accumulation.  One workgroup owns 64 columns x
// all rows x one K slice; `splitk` slices (a function of N and K only, never of M) write fp32 slabs that a second launch adds
// in slice order 0, 1, 2, ... -- no atomics, so a value depends on nothing but (row of A, column of W): not on M, not on the
// launch.  Requirements: A readable for 256 rows (lda elements apart), W readable for round_up(N, 64) rows, K % 64 == 0,
// N % 64 == 0 (DEC_SWIGLU: W holds gate / up rows interleaved in blocks of 16, N = 2 * columns of out).
enum DecodeEpilogue {
    DEC_F16 = 0,        // out_f16 = fp16(acc)
    DEC_F16_RESID = 1,  // out_f16 = fp16(fp16(acc) + resid_f16)          (resid may alias out)
    DEC_SWIGLU = 2,     // out_f16[m, c] = fp16(fp16(silu(fp16(acc_gate))) * fp16(acc_up))
    DEC_F32 = 3         // out_f32 = float(fp16(acc))                     (HF: fp16 logits, then .float())
};
struct DecodeGemmParams {
    const half_t* A; int64_t lda;
    const half_t* W; int64_t ldw;
    void* out; int64_t ldo;
    const half_t* resid; int64_t ldr;
    float* slabs;                 // [splitk][256][N] fp32 workspace (used when splitk > 1)
    int M, N, K;
};
int decode_gemm_splitk(int N, int K);                       // slices this shape runs with
size_t decode_gemm_slab_bytes(int N, int K);                // workspace the shape needs (0 when splitk == 1)
// Allows the kernels their 80 KiB of dynamic LDS on the CURRENT device.  Call once per device before the first launch, outside any
// stream capture (cgpt_llm_create does): launch_decode_gemm itself then only launches.
hipError_t decode_gemm_prepare();
hipError_t launch_decode_gemm(int epilogue, const DecodeGemmParams& p, hipStream_t stream);

}  // namespace cgpt
