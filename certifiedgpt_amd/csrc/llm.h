// llm.h -- launchers of the LLaMA decode-step kernels (llm_gemm.hip, llm_step.hip, ...).  All enqueue on `stream`, no host sync.
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
// wscale != null: W points at the row-wise absmax int8 matrix q[N, K] (ldw in int8 elements) and wscale at its N fp16 row scales;
// the product is bit for bit that of the fp16 call on W'[n, k] = fp16(q[n, k]) * wscale[n] (one fp16 multiply).  Not with DEC_F32.
// live != null (early stop): a device int, uniform over the call, written by an earlier launch of `stream`; both
// launches take their guarded instantiation, which reads it first and does nothing when it is 0.  null: the kernels as they were.
hipError_t launch_decode_gemm(int epilogue, const DecodeGemmParams& p, hipStream_t stream, const half_t* wscale = nullptr,
                              const int* live = nullptr);

// ------------------------------------------------------------------------------------- int8-activation linear (llm_gemm_i8.hip)
// The W8A8 linear with a per-row outlier split (the law is written out at the top of llm_gemm_i8.hip).  Two launches
// per linear: the quantiser turns fp16 rows into int8 codes, one fp32 scale per row and the row's outlier list; the GEMM multiplies the
// codes with the int8 weight rows on the int8 MFMA into int32 and applies scales, outlier term and epilogue.  Integer accumulation is
// exact, so a result does not depend on M, the row tile, the K split or the launch.
//   x [rows, K] fp16 (rows K apart) -> a8 [rows, K] int8, sa [rows] fp32, lists [rows][cap + 1] uint32: word 0 = entries kept
//   (<= cap), word 1 + i = k | fp16 bits << 16 in ascending k.  counters[4]: rows, outliers, max outliers of a row, rows with more
//   than `cap` outliers (those keep their first `cap`; their result is finite but not the law's).  K % 128 == 0, K <= 65536, cap 1..1024.
hipError_t launch_act_quant(const half_t* x, int64_t rows, int K, float threshold, int cap, signed char* a8, float* sa, uint32_t* lists,
                            unsigned long long* counters, hipStream_t stream, const int* live = nullptr);
struct I8GemmParams {
    const signed char* A; int64_t lda;      // int8 codes, readable for round_up(M, 256) rows
    const float* sa;                        // [M]
    const uint32_t* lists; int cap;         // [M][cap + 1]
    const signed char* W; int64_t ldw;      // q [N, K]
    const half_t* wscale;                   // [N]
    half_t* out; int64_t ldo;
    const half_t* resid; int64_t ldr;       // DEC_F16_RESID (may alias out)
    int* slabs;                             // [splitk][256][N] int32 workspace (used when there is one row tile and splitk > 1)
    int M, N, K;
};
int i8_gemm_splitk(int N, int K);                           // slices a one-row-tile call of this shape runs with (more row tiles: 1)
size_t i8_gemm_slab_bytes(int N, int K);
hipError_t i8_gemm_prepare();                               // dynamic-LDS limit on the CURRENT device, outside any capture
// DEC_F16, DEC_F16_RESID or DEC_SWIGLU; N % 64 == 0, K % 128 == 0; any M >= 1 (256-row tiles on the grid's second dimension).
hipError_t launch_i8_gemm(int epilogue, const I8GemmParams& p, hipStream_t stream, const int* live = nullptr);

// ------------------------------------------------------------------------------------- token step (llm_step.hip)
// One launcher per kernel (the arg-max select's is llm_select.h's).  `rows` <= 256 fp16 rows, `hidden` (a multiple of 8) elements apart.
// live as for launch_decode_gemm.  h[r, :] = table[tokens[r], :] (a token outside the table reads row 0);  y[r, :] = LlamaRMSNorm(x[r, :]) * w
hipError_t launch_llm_embed(const long long* tokens, const half_t* table, int vocab, int hidden, half_t* h, int rows, hipStream_t stream, const int* live = nullptr);
hipError_t launch_llm_rmsnorm(const half_t* x, const half_t* w, int hidden, float eps, half_t* y, int rows, hipStream_t stream, const int* live = nullptr);
// table[pos][0..63 | 64..127] = fp16(cos | sin(pos * inv_freq[i])) for pos < positions; inv_freq holds 64 device floats.
hipError_t launch_llm_rope_table(const float* inv_freq, half_t* table, int positions, hipStream_t stream);
// Rotary + K/V append at buffer position `pos` + one-query attention over the row's keys, for every (row, head); out [rows, hidden].
// G = 0: the plain kernel, qkv rows 3 hidden wide, Kc / Vc [rows, heads, len_stride, 128].  G in {1, 2, 4, 8}: the grouped kernel,
// kv_heads = heads / G, layouts as for the prefill below.  starts != null (device, [rows]): left padding, clamped into 0 .. min(smax, pos).
// Dynamic LDS: llm_step_attn_lds_bytes(G, pos + 1); llm_step_prepare(G, max_len) allows it up to max_len (per device, outside a capture).
struct StepAttnArgs {
    int G; const half_t* qkv; int hidden, heads; half_t *Kc, *Vc; int64_t len_stride;
    const half_t* rope; int pos; half_t* out; const int32_t* starts; int smax; const int* live;
};
size_t llm_step_attn_lds_bytes(int G, int positions);
hipError_t llm_step_prepare(int G, int max_len);
hipError_t launch_llm_step_attention(const StepAttnArgs& a, int rows, hipStream_t stream);
// The weight law of an int8 handle on w [rows, K] (K % 16 == 0): q and one fp16 scale per row.  Row r goes to row r (interleave < 0)
// or to row 32 (r / 16) + 16 interleave + r % 16 of q / scales (the gate / up fusion).
hipError_t launch_llm_quant_rows(const half_t* w, int rows, int K, int interleave, signed char* q, half_t* scales, hipStream_t stream);
// out[n, k] = fp16(q[n, k]) * scales[n] for all round_up(N, 256) rows of an int8 matrix (pad rows come out as zeros).
hipError_t launch_llm_dequant(const signed char* q, const half_t* scales, int N, int K, half_t* out, hipStream_t stream);
// After a select: *live = any(unfinished[0 .. rows)), *live_steps = (first ? 0 : *live_steps) + (*live & more).  rows <= 256.
hipError_t launch_llm_live(const int* unfinished, int rows, int first, int more, int* live, int* live_steps, hipStream_t stream);

// ------------------------------------------------------------------------------------- prefill (llm_prefill.hip)
// Token row r = b * L + p of B prompts of L positions.  All fp16, rows `hidden` (or 3 hidden / 2 mlp / mlp) elements apart.
// kv_heads (rope, attention, scoring attention): == heads is the plain layout and the plain kernel instantiations; a divisor of heads
// below it is grouped-query attention -- qkv rows are hidden + 2 kv_heads 128 wide (q, then k, then v), Kc / Vc are
// [B, kv_heads, len_stride, 128], query head h reads K/V head h / (heads / kv_heads).
// x_out[r] = fp16(x[s] + delta[s]) (delta may be null), y[r] = LlamaRMSNorm(x_out[r]) * w, with s = r * src_mul + src_add
// (identity: 1, 0; the last position of every prompt: L, L - 1).  x_out may alias x.
hipError_t launch_prefill_addnorm(const half_t* x, const half_t* delta, int64_t src_mul, int64_t src_add, const half_t* w, int hidden,
                                  float eps, half_t* x_out, half_t* y, int64_t rows, hipStream_t stream);
// Rotates q in place in qkv [B L, 3 hidden] and writes rotated k and v to rows 0 .. L-1 of Kc / Vc [B, heads, len_stride, 128].
// starts (device, [B] int32, or null = no padding): row b is left-padded by start[b] positions (clamped into 0 .. L-1); its real
// tokens sit at buffer positions start[b] .. L-1 and take rotary rows 0 ..; pad positions are not rotated and not written to the cache.
hipError_t launch_prefill_rope(half_t* qkv, int B, int L, int hidden, int heads, int kv_heads, half_t* Kc, half_t* Vc, int64_t len_stride,
                               const half_t* rope, const int32_t* starts, hipStream_t stream);
// out[B L, hidden] = causal softmax(q . K^T / sqrt(128)) . V per head, q from qkv (already rotated), K / V rows 0 .. L-1 of the cache.
// starts as above: row b attends over cache rows start[b] .. p only, walked from start[b]; pad rows of `out` are written as zeros.
hipError_t launch_prefill_attention(const half_t* qkv, int B, int L, int hidden, int heads, int kv_heads, const half_t* Kc, const half_t* Vc,
                                    int64_t len_stride, half_t* out, const int32_t* starts, hipStream_t stream);
// The two launchers above for L positions that FOLLOW pos0 positions whose cache rows exist (cgpt_llm_prefill_from): qkv / out hold the
// B L new rows; token row p is rotated at pos0 + p (starts: pos0 + p - start[b], start clamped into 0 .. L-1) and written to cache row
// pos0 + p; its query attends over cache rows 0 .. pos0 + p (starts: start[b] ..).  The attention tiles the queries by absolute
// position, so a row's output has the bits launch_prefill_attention gives it on the whole prompt of pos0 + L positions.
hipError_t launch_prefill_rope_from(half_t* qkv, int B, int pos0, int L, int hidden, int heads, int kv_heads, half_t* Kc, half_t* Vc,
                                    int64_t len_stride, const half_t* rope, const int32_t* starts, hipStream_t stream);
hipError_t launch_prefill_attention_from(const half_t* qkv, int B, int pos0, int L, int hidden, int heads, int kv_heads, const half_t* Kc,
                                         const half_t* Vc, int64_t len_stride, half_t* out, const int32_t* starts, hipStream_t stream);
// Rows 0 .. P-1 of srcK / srcV [1, kv_heads, src_stride, 128] -> rows s_b .. s_b + P - 1 of every row b of dstK / dstV
// [B, kv_heads, dst_stride, 128]; s_b = start[b] clamped into 0 .. dst_stride - P, 0 without starts.  16-byte copies, nothing else written.
hipError_t launch_kv_broadcast(const half_t* srcK, const half_t* srcV, int64_t src_stride, int P, int B, int kv_heads, const int32_t* starts,
                               half_t* dstK, half_t* dstV, int64_t dst_stride, hipStream_t stream);
// act[rows, mlp] = fp16(fp16(silu(gate)) * up) from gu [rows, 2 mlp] with gate / up columns interleaved in blocks of 16.
hipError_t launch_prefill_swiglu(const half_t* gu, int64_t rows, int mlp, half_t* act, hipStream_t stream);

// ------------------------------------------------------------------------------------- answer scoring (llm_score.hip)
// C candidate answers of T_c tokens each are scored on ONE prefilled prompt of L positions per row.  Token 0 of a candidate is
// predicted by the prompt's last position; token j >= 1 by "tail row" j - 1: input token j - 1 of the candidate at rotary position
// L + j - 1.  A prompt row b has S = sum_c (T_c - 1) tail rows, tail row r = b * S + off[c] + j everywhere below.
constexpr int SCORE_MAX_CANDS = 64;      // candidates of one call
constexpr int SCORE_MAX_TAIL = 64;       // tail rows per prompt row (the attention kernel keeps their state in LDS)
struct ScoreCands {                      // passed by value: nothing is copied to the device by the host
    int n;                               // C
    int tmax;                            // row length of the token table [C, tmax] ([B, C, tmax] with per-row candidates)
    int off[SCORE_MAX_CANDS + 1];        // off[c] = sum of (T_c' - 1) over c' < c; off[n] = S.  T_c = off[c + 1] - off[c] + 1
};
// Sets the attention kernel's dynamic-LDS limit on the CURRENT device (once per device, outside any capture).
hipError_t score_prepare();
// Per-row prompts and candidates (cgpt_llm_score_ragged): `starts` / `row_lens` / `per_row` below select the RAGGED instantiations;
// null / false are the plain kernels, which read neither array.
//   starts   (device, [B] int32): row b is left-padded by start[b] positions (clamped into 0 .. L-1), see launch_prefill_rope
//   row_lens (device, [B, C] int32): row b's real length of candidate c (clamped into 1 .. T_c); the token table is then
//            [B, C, tmax] and T_c of `t` the longest length of candidate c over the rows
// h[r, :] = embed[token of tail row r, :]; a token outside the table reads row 0.  per_row: the table is [B, C, tmax].
hipError_t launch_score_embed(const long long* cand_tokens, const ScoreCands& t, int B, const half_t* table, int vocab, int hidden,
                              half_t* h, hipStream_t stream, bool per_row = false);
// Rotary + attention of the tail rows: out[r, head] = softmax(q_r . [K_prompt(b, 0..L-1); k_tail(b, c, 0..j)] / sqrt(128)) . V alike,
// q / k / v from qkv [B S, 3 hidden] (not modified).  Kc / Vc are read (rows 0 .. L-1) and NEVER written.
// starts: the prompt keys of row b are cache rows start[b] .. L-1 (rows below are never read), tail row j is rotated at L - start[b] + j.
hipError_t launch_score_attention(const half_t* qkv, const ScoreCands& t, int B, int L, int hidden, int heads, int kv_heads, const half_t* Kc,
                                  const half_t* Vc, int64_t len_stride, const half_t* rope, half_t* out, hipStream_t stream,
                                  const int32_t* starts = nullptr);
// ce[b, tok(c) + j] = label-smoothed cross-entropy of one logits row against token j of candidate c, tok(c) = off[c] + c, a row of
// ce holding S + C values.  first: token 0 of every candidate on the fp32 rows first_logits[b] (B x C workgroups).  tail: `rows`
// fp16 logits rows, the tail rows row0 .. row0 + rows - 1 (row r predicts token j + 1 of its candidate).
// row_lens: ce[b, tok(c) + j] = 0 for j >= the row's length of candidate c.
hipError_t launch_score_ce_first(const float* first_logits, int vocab, const long long* cand_tokens, const ScoreCands& t, int B,
                                 float smoothing, float* ce, hipStream_t stream, const int32_t* row_lens = nullptr);
hipError_t launch_score_ce_tail(const half_t* logits, int vocab, const long long* cand_tokens, const ScoreCands& t, int64_t row0,
                                int64_t rows, float smoothing, float* ce, hipStream_t stream, const int32_t* row_lens = nullptr);
// out[b, c] = ce[b, tok(c)] + ... + ce[b, tok(c) + T_c - 1], added in token order.  row_lens: the row's own tokens only.
hipError_t launch_score_sum(const float* ce, const ScoreCands& t, int B, float* out, hipStream_t stream, const int32_t* row_lens = nullptr);

}  // namespace cgpt
