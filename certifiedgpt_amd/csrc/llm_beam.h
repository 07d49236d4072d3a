// llm_beam.h -- launchers of the beam-search kernels (llm_beam.hip): the ancestry step attention and the beam select.  The law is
// stated once in llm_laws.py (`beam_step_law`) and in DESIGN.md 4.4.13.  All enqueue on `stream`, no host sync.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "llm_select.h"

namespace cgpt {

constexpr int BEAM_MIN = 2, BEAM_MAX = 8;                // beams per image
constexpr int BEAM_MAX_KEEP = (1 + MAX_EOS) * BEAM_MAX;  // K = max(2, 1 + E) k <= 72
constexpr int BEAM_MAX_VOCAB = 131072;

// The token step's rotary + K/V append + one-query attention for `rows` = images x k beam rows (llm_attn_beam_kernel).
//   Kp / Vp  [images, heads, prompt_stride, 128]: the prompt cache, rows 0 .. L-1 read, never written
//   Kb / Vb  [rows, heads, beam_stride, 128]: generated positions only; row t of beam row r is the only row written
//   anc      [rows, ld_anc] int32: anc[r][s] = the beam row whose cache row s belongs to the hypothesis living in row r (s < t read;
//            a value outside 0 .. rows-1 is clamped into it, so nothing outside the beam cache is ever read)
struct BeamAttnArgs {
    const half_t* qkv; int hidden, heads, k;
    const half_t *Kp, *Vp; int64_t prompt_stride;
    half_t *Kb, *Vb; int64_t beam_stride;
    const int32_t* anc; int64_t ld_anc;
    const half_t* rope; int L, t, rows;
    half_t* out;
};
hipError_t launch_llm_beam_attn(const BeamAttnArgs& a, hipStream_t stream);

// The state of `images` x k beams between two selects.  A select reads `in` and writes `out` (never in place: rows are gathered by
// parent); a first select reads no `in` at all.
struct BeamState {
    float* running;            // [images k]
    long long* tokens;         // [images k, n]   the beams' generated tokens, pad behind them
    int32_t* anc;              // [images k, n]   ancestry rows, see BeamAttnArgs
    float* pool_score;         // [images k]
    int32_t* pool_fin;         // [images k]
    int32_t* pool_len;         // [images k]
    long long* pool_seq;       // [images k, n]
    int32_t* open;             // [images]
};
struct BeamSelectArgs {
    const float* src; int64_t lds;         // logits of beam row r: src[r * lds + 0 .. vocab); shared != 0: src[(r / k) * lds + ...],
    int shared;                            // one row per image (the prefill's logits, which every beam of the image reads)
    int vocab, k, keep, n, step;           // keep = K; step = i
    int first;                             // != 0: the state before is the initial one and `in` is not read
    int mask_eos; EosIds eos; long long pad;
    float divisor;                         // fp32((step + 1) ** length_penalty), formed on the host in float64
    BeamState in, out;
    long long* next_tok;                   // [images k]   the token every new beam feeds to the next step
    int32_t* parents;                      // [images k]   local index 0 .. k-1 of the beam each new beam continues
    long long* tokens_out; float* scores_out;   // [images, n] / [images] or null: pool slot 0 after this select
    float* trace;                          // [images, 5 k + 1] or null: running, parents, tokens, pool scores, pool flags, open
};
hipError_t launch_llm_beam_select(const BeamSelectArgs& a, int images, hipStream_t stream);
// dst[r * ldd + 0 .. cols) = src[(r / k) * lds + 0 .. cols) for r < rows (fp32): an image's row for each of its k beam rows
hipError_t launch_llm_beam_spread(const float* src, int64_t lds, float* dst, int64_t ldd, int cols, int rows, int k, hipStream_t stream);

}  // namespace cgpt
