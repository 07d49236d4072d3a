// llm_select.h -- what the two token-select kernels share: the by-value id tables, the bookkeeping tail of one select
// (llm_select_kernel in llm_step.hip: arg-max; llm_sample_kernel in llm_sample.hip: the sampling law) and the selects' launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <type_traits>

#include "../../include/cgpt.h"

namespace cgpt {

constexpr int MAX_EOS = 8;
struct EosIds { long long id[MAX_EOS]; int n; };
// Stop sequences (cgpt_llm_set_stop_sequences), by value like EosIds: sequence s is id[s][0 .. len[s]).  `col` is the
// select's index i, which the greedy entry fills in per launch.  A select without them takes the empty NoStop.
constexpr int MAX_STOP = 8, MAX_STOP_LEN = 8;
struct StopSeqs { long long id[MAX_STOP][MAX_STOP_LEN]; int len[MAX_STOP]; int n; int col; };
struct NoStop {};
template <bool STOP> using StopArg = std::conditional_t<STOP, StopSeqs, NoStop>;

// The bookkeeping tail of one select, run by ONE thread of the row's workgroup once the row's token `idx` is known: pad once the row
// has finished, EOS, the STOP match (the row's earlier tokens are read back from tokens_out, columns col - 1, col - 2, ...; a
// sequence longer than col + 1 is skipped, so nothing left of column 0 is ever read), then `unfinished`, tokens_out and next_tok.
// A macro, not a function: handed to a function by reference, the by-value StopSeqs kernel argument is copied into registers whole
// (llm_select_kernel<., true>: 44 -> 106 SGPRs, 8 -> 7 waves per SIMD), and the arg-max select must stay the code it was.
#define CGPT_SELECT_TAIL(STOP, row, idx, first, eos, pad, unfinished, tokens_out, ld_tokens, next_tok, stop)                        \
    do {                                                                                                                            \
        int u = (first) ? 1 : (unfinished)[row];                                                                                    \
        const long long tok = u ? (long long)(idx) : (pad);                                                                         \
        for (int e = 0; e < (eos).n; ++e)                                                                                           \
            if (tok == (eos).id[e]) u = 0;                                                                                          \
        if constexpr (STOP) {                                                                                                       \
            if (u) {                                                                                                                \
                const long long* t = (tokens_out) + (int64_t)(row) * (ld_tokens); /* column `col`; t[-j] is column col - j */       \
                _Pragma("unroll") for (int q = 0; q < MAX_STOP; ++q) {                                                              \
                    const int len = q < (stop).n ? (stop).len[q] : 0;                                                               \
                    if (len < 1 || len > (stop).col + 1) continue;                                                                  \
                    bool match = true;                                                                                              \
                    _Pragma("unroll") for (int k = 0; k < MAX_STOP_LEN; ++k) /* element k sits len - 1 - k columns back */          \
                        if (k < len) match = match && (k == len - 1 ? tok : t[k - (len - 1)]) == (stop).id[q][k];                   \
                    if (match) u = 0;                                                                                               \
                }                                                                                                                   \
            }                                                                                                                       \
        }                                                                                                                           \
        (unfinished)[row] = u;                                                                                                      \
        (tokens_out)[(int64_t)(row) * (ld_tokens)] = tok;                                                                           \
        (next_tok)[row] = tok;                                                                                                      \
    } while (0)

// ------------------------------------------------------------------------------------- sampled select (llm_sample.hip)
// The settings of one sampled select (cgpt_llm_sample_params without its size word) and everything else the sampler reads or writes
// beyond the arg-max select's arguments.  The law is stated once in minigpt4.py (`sample_token_law`) and in DESIGN.md 4.4.10.
constexpr int SAMPLE_MAX_VOCAB = 131072;     // one bit per column in LDS
constexpr int SAMPLE_MAX_SPECIAL = 1024;     // EOS ids + earlier tokens of a row that one select can treat (LDS tables)
struct SampleLaw { int do_sample; float temperature; int top_k; float top_p; float penalty; };
struct SampleIo {
    const long long* prev; int64_t ld_prev; int num_prev;      // the row's earlier tokens: prev[row * ld_prev + 0 .. num_prev)
    int step;                                                  // Philox counter word 0
    const long long* draw_ids;                                 // [B] device, read when the kernel runs
    const unsigned long long* seed;                            // one device word, likewise
    const float* uniforms_in;                                  // [B] or null: replaces the Philox draw
    float* uniforms_out; int* kept_count_out; float* kept_mass_out;   // [B] each, or null
};
struct SelectArgs {                                            // the arguments of llm_select_kernel
    const float* src; int64_t lds; float* dst; int64_t ldd; int vocab; int mask_eos; EosIds eos; long long pad; int first;
    int* unfinished; long long* tokens_out; int64_t ld_tokens; long long* next_tok; const int* live;
};
// One workgroup per row.  guard: the early-stop instantiation (reads *live); stop != null: the stop-sequence instantiation.
// launch_llm_select is the arg-max select (llm_step.hip); its kernel takes the struct's fields as positional arguments.
hipError_t launch_llm_sample(bool guard, const StopSeqs* stop, const SelectArgs& a, const SampleLaw& law, const SampleIo& io, int rows,
                             hipStream_t stream);
hipError_t launch_llm_select(bool guard, const StopSeqs* stop, const SelectArgs& a, int rows, hipStream_t stream);

// The checks every sampling entry makes before any launch (CGPT_ERR_INVALID naming `who`), and the settings as the kernel takes them.
cgpt_status check_sample_params(const std::string& who, const cgpt_llm_sample_params& p, int vocab, int num_prev, int num_eos,
                                SampleLaw* out);

// ------------------------------------------------------------------------------------- trie-constrained select (llm_trie.hip)
// The law is stated once in llm_laws.py (`constrained_select_law`) and in DESIGN.md 4.4.12.  The tables are the CSR trie
// cgpt_llm_trie_check validates (device pointers here); `node` is the row's position in it, [rows] int32 like `unfinished`.
constexpr int TRIE_MAX_NODES = 1 << 20, TRIE_MAX_DEPTH = 32;
struct TrieArgs {
    const float* src; int64_t lds;                                               // the logits select reads: src[row * lds + token]
    const int *child_begin, *child_tok, *child_node, *leaf_class; int nodes;
    long long pad; int first;
    int* node; int* unfinished; long long* tokens_out; int64_t ld_tokens; long long* next_tok; int* labels_out; const int* live;
};
// One workgroup per row.  guard: the early-stop instantiation (reads *live).
hipError_t launch_llm_trie_select(bool guard, const TrieArgs& a, int rows, hipStream_t stream);
// dst[r * ldd + 0 .. cols) = src[r * lds + 0 .. cols) for r < rows (fp32)
hipError_t launch_llm_copy_rows(const float* src, int64_t lds, float* dst, int64_t ldd, int cols, int rows, hipStream_t stream);

}  // namespace cgpt
