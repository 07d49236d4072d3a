// llm.hip -- the LLaMA engine behind MiniGPT-4's decode, host side: the handle, the launch sequences (token step, prefill, scoring,
// greedy loop) and the C-ABI (include/cgpt.h, "LLaMA decode steps").  No kernel lives here: the step's are llm_step.hip's.
//
// Reference call replaced: every forward after the prefill inside `self.llama_model.generate(...)`
// (graphs/models/minigpt4/models/minigpt_base.py:418-431, greedy: do_sample=False, num_beams=1), i.e. HF LlamaForCausalLM
// on one new token per row with a K/V cache.  The prefill is the caller's (the model's own forward; its K/V are used in place) or
// cgpt_llm_prefill below: the same layer sequence on B x L token rows, large-shape GEMMs (gemm.hip) and llm_prefill.hip's kernels.
// cgpt_llm_score (`MiniGPTBase.multi_select`, minigpt_base.py:451-467) runs that sequence once more on the answer tokens of all
// candidates, on the prompt cache the prefill left and without writing to it (llm_score.hip).  No sequence here synchronises,
// allocates or copies from the host after cgpt_llm_create, so a whole greedy loop can be captured into one graph.
// int8 handles hold the seven layer linears as row-wise absmax int8 with one fp16 scale per row: gemm() reads
// them in place, big_gemm() expands one matrix into the fp16 scratch right before its GEMM.  Activations-int8 handles (DESIGN.md
// 4.4.7) quantise the rows and run the int8 GEMM instead, in those two functions only; lm_head stays fp16 and there is no scratch.
#include <math.h>
#include <stddef.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "../../include/cgpt.h"
#include "common_host.h"
#include "llm.h"
#include "llm_beam.h"
#include "llm_select.h"

using namespace cgpt;

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return cgpt_fail(CGPT_ERR_HIP, std::string(#expr) + " -> " + hipGetErrorString(e_));       \
    } while (0)
#define CGCHK(expr)                         \
    do {                                    \
        cgpt_status s_ = (expr);            \
        if (s_ != CGPT_OK) return s_;       \
    } while (0)

namespace {

constexpr int HD = 128;                // head size the attention kernels are written for
constexpr int MAX_ROWS = 256;          // one GEMM row tile
constexpr size_t LDS_PER_CU = 160 * 1024;           // gfx950

// The config a handle keeps: the caller's cgpt_llm_config and the switches of cgpt_llm_config_gqa (0 for a plain config).
struct LlmCfg : cgpt_llm_config {
    int32_t grouped_kv = 0;
    int32_t act_format = 0;                // cgpt_llm_config_act: 1 = int8 activations with the outlier split
    float act_threshold = 6.0f;
    int32_t outlier_cap = 64;
};

// One fused layer matrix [up256(N)][K]: fp16 (`w`) on an fp16 handle; int8 `q` with one fp16 scale per row (`s`) on an int8 handle.
struct Mat {
    half_t* w = nullptr;
    signed char* q = nullptr;
    half_t* s = nullptr;
};
struct Layer {
    Mat wqkv, wo, wgu, wdown;
    half_t *ln1 = nullptr, *ln2 = nullptr;
};

}  // namespace

struct cgpt_llm {
    LlmCfg cfg;
    std::set<std::string> loaded;
    size_t expected = 0;
    std::vector<void*> allocs;             // every device buffer of the handle, freed at destroy
    int64_t weight_bytes = 0;              // matrices, scales and scratch, as allocated (cgpt_llm_weight_bytes)
    std::vector<Layer> layers;
    half_t *embed = nullptr, *norm = nullptr, *lm_head = nullptr, *rope = nullptr;
    // int8 handles: the prefill's ONE fp16 expansion of the layer matrix its next GEMM reads (stream order makes one enough)
    half_t* scratch = nullptr;
    half_t *h = nullptr, *xn = nullptr, *qkv = nullptr, *attn = nullptr, *act = nullptr;
    float *slabs = nullptr, *logits = nullptr;
    long long* tok = nullptr;
    int* unfinished = nullptr;
    // activations-int8 handles: codes, row scales and outlier lists of the rows the next int8 GEMM reads -- 256 rows for the token step,
    // `p_rows` for the prefill / scoring workspace (one set each: stream order makes one enough) -- and the four statistics counters
    signed char *a8 = nullptr, *p_a8 = nullptr;
    float *sa = nullptr, *p_sa = nullptr;
    uint32_t *lists = nullptr, *p_lists = nullptr;
    unsigned long long* act_counters = nullptr;
    // early stop (cgpt_llm_set_early_stop): `live` = 1 while some row of the running greedy call is unfinished, `live_steps` = the
    // token steps of that call that ran; both written by llm_live_kernel only.  With early stop off nothing on the device maintains
    // them: the last call's count (num_new - 1, every step runs) is kept in `off_steps`, and `last_on` says which of the two holds.
    int *live = nullptr, *live_steps = nullptr;
    int early_stop = 0, last_on = 0, off_steps = 0;
    StopSeqs stop{};                       // cgpt_llm_set_stop_sequences: n = 0 (none) after create; read when a greedy call enqueues
    // cgpt_llm_set_trie: the candidate trie of the constrained decode, four int32 tables in one allocation; t_nodes = 0 (none) after
    // create; read when a constrained call enqueues.  Replaced tables stay in `allocs`: a captured call replays on their addresses.
    const int *t_begin = nullptr, *t_tok = nullptr, *t_node = nullptr, *t_leaf = nullptr;
    int t_nodes = 0, t_depth = 0;
    int* trie_node = nullptr;              // [max_batch]: the trie node every row of the running constrained call stands on
    // beam search (cgpt_llm_beam_reserve): the two state sets the selects of a beam call alternate between (select i reads set i & 1
    // and writes the other), for bm_rows beam rows and bm_elems = rows x num_new token / ancestry entries.  Replaced sets stay in `allocs`.
    int64_t bm_rows = 0, bm_elems = 0;
    BeamState bm[2]{};
    int32_t* bm_parents = nullptr;
    // prefill workspace (cgpt_llm_prefill_reserve): `p_rows` token rows, a multiple of 256.  A workspace that a larger one replaced
    // stays allocated (in `allocs`) until destroy: a graph captured earlier still holds its addresses.
    int64_t p_rows = 0;
    half_t *p_h = nullptr, *p_xn = nullptr, *p_qkv = nullptr, *p_attn = nullptr, *p_proj = nullptr, *p_gu = nullptr, *p_act = nullptr;
    // scoring workspace (cgpt_llm_score_reserve) beside the prefill workspace, which holds the tail rows: fp16 logits of `s_rows`
    // tail rows (a multiple of 256; more rows run in chunks) and `s_ce` per-token cross-entropies.  Replaced buffers stay in `allocs`.
    int64_t s_rows = 0, s_ce = 0;
    half_t* s_logits = nullptr;
    float* s_ce_buf = nullptr;
};

namespace {

// columns of the fused q/k/v projection: hidden + 2 kv_heads 128 (3 hidden on a plain handle, where kv_heads == heads)
inline int qkv_width(const cgpt_llm_config& c) { return c.hidden + 2 * c.kv_heads * HD; }

cgpt_status dev_zalloc(cgpt_llm* m, size_t bytes, void** out) {
    HIPCHK(hipMalloc(out, bytes));
    m->allocs.push_back(*out);
    HIPCHK(hipMemset(*out, 0, bytes));
    return CGPT_OK;
}

cgpt_status ready(cgpt_llm* m, const char* who) {
    if (m->loaded.size() != m->expected)
        return cgpt_fail(CGPT_ERR_STATE, std::string(who) + ": " + std::to_string(m->expected - m->loaded.size()) + " of " +
                                             std::to_string(m->expected) + " weights have not been loaded");
    return CGPT_OK;
}

cgpt_status check_cache(cgpt_llm* m, const char* who, int B, int last_pos, void* const* k, void* const* v, int64_t len_stride) {
    if (!k || !v) return cgpt_fail(CGPT_ERR_INVALID, std::string(who) + ": null K/V pointer table");
    if (B < 1 || B > m->cfg.max_batch) return cgpt_fail(CGPT_ERR_INVALID, std::string(who) + ": rows outside 1..max_batch");
    if (last_pos < 0 || last_pos >= len_stride || last_pos >= m->cfg.max_len)
        return cgpt_fail(CGPT_ERR_INVALID, std::string(who) + ": position outside the cache (kv_len_stride) or max_len");
    for (int l = 0; l < m->cfg.layers; ++l)
        if (!k[l] || !v[l]) return cgpt_fail(CGPT_ERR_INVALID, std::string(who) + ": null K/V buffer");
    return CGPT_OK;
}

// A grower's buffers (prefill / score / beam reserve), built beside the ones in use: add() allocates and zeroes (nothing after a
// failure); commit() synchronises and hands them to `allocs`, or frees all of them on any failure.  Then the caller swaps them in.
struct Staging {
    std::vector<void*> made;
    hipError_t e = hipSuccess;
    template <typename T>
    void add(T** out, size_t bytes) {
        if (e != hipSuccess || (e = hipMalloc((void**)out, bytes)) != hipSuccess) return;
        made.push_back(*out);
        e = hipMemset(*out, 0, bytes);
    }
    cgpt_status commit(cgpt_llm* m, const std::string& who) {
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) {
            for (void* p : made) (void)hipFree(p);
            return cgpt_fail(CGPT_ERR_HIP, who + ": workspace allocation failed -> " + hipGetErrorString(e));
        }
        m->allocs.insert(m->allocs.end(), made.begin(), made.end());
        return CGPT_OK;
    }
};

// The int8 GEMM on what launch_act_quant left in a8 / sa / lists: rows K apart on both sides, the residual laid out as the result.
I8GemmParams i8_params(const signed char* a8, const float* sa, const uint32_t* lists, int cap, const signed char* Wq, const half_t* Ws,
                       void* out, int64_t ldo, const half_t* resid, void* slabs, int64_t M, int N, int K) {
    return I8GemmParams{a8, K, sa, lists, cap, Wq, K, Ws, (half_t*)out, ldo, resid, ldo, (int*)slabs, (int)M, N, K};
}

cgpt_status gemm(cgpt_llm* m, int epi, const half_t* A, int K, const Mat& W, int N, void* out, int64_t ldo, const half_t* resid,
                 int B, hipStream_t st, const int* live = nullptr) {
    const LlmCfg& c = m->cfg;
    if (c.act_format && W.q) {                             // a layer linear of an activations-int8 handle: quantise the rows, int8 GEMM
        HIPCHK(launch_act_quant(A, B, K, c.act_threshold, c.outlier_cap, m->a8, m->sa, m->lists, m->act_counters, st, live));
        HIPCHK(launch_i8_gemm(epi, i8_params(m->a8, m->sa, m->lists, c.outlier_cap, W.q, W.s, out, ldo, resid, m->slabs, B, N, K), st, live));
        return CGPT_OK;
    }
    const DecodeGemmParams p{A, K, W.q ? reinterpret_cast<const half_t*>(W.q) : W.w, K, out, ldo, resid, ldo, m->slabs, B, N, K};
    HIPCHK(launch_decode_gemm(epi, p, st, W.q ? W.s : nullptr, live));
    return CGPT_OK;
}

// One token step on rows 0..B-1: tokens -> logits (fp32, row stride ld_logits).
// starts (device, or null): per-row left padding, clamped into 0 .. smax, see llm_attn_kernel.
// live (m->live, or null: the plain kernels): every launch is the guarded instantiation on it (a greedy call with early stop on).
// beam != null (plain handles without `live` only): the B rows are images x k beam rows, kp / vp / len_stride the BEAM caches,
// pos = L + t, and the attention is llm_attn_beam_kernel on the prompt caches and the ancestry table `beam` names.
struct BeamStep {
    void* const* pk; void* const* pv; int64_t prompt_stride;
    const int32_t* anc; int64_t ld_anc;
    int k, L, t;
};
cgpt_status run_step(cgpt_llm* m, const int* live, const long long* tokens, int B, int pos, const int32_t* starts, int smax, void* const* kp,
                     void* const* vp, int64_t len_stride, float* logits, int64_t ld_logits, hipStream_t st, const BeamStep* beam = nullptr) {
    const LlmCfg& c = m->cfg;
    const int H = c.hidden, NQ = qkv_width(c);
    HIPCHK(launch_llm_embed(tokens, m->embed, c.vocab, H, m->h, B, st, live));
    for (int l = 0; l < c.layers; ++l) {
        const Layer& L = m->layers[l];
        HIPCHK(launch_llm_rmsnorm(m->h, L.ln1, H, c.rms_eps, m->xn, B, st, live));
        CGCHK(gemm(m, DEC_F16, m->xn, H, L.wqkv, NQ, m->qkv, NQ, nullptr, B, st, live));
        if (beam) {
            BeamAttnArgs a{m->qkv, H, c.heads, beam->k, (const half_t*)beam->pk[l], (const half_t*)beam->pv[l], beam->prompt_stride,
                           (half_t*)kp[l], (half_t*)vp[l], len_stride, beam->anc, beam->ld_anc, m->rope, beam->L, beam->t, B, m->attn};
            HIPCHK(launch_llm_beam_attn(a, st));
        } else {
            const StepAttnArgs a{c.grouped_kv ? c.heads / c.kv_heads : 0, m->qkv, H, c.heads, (half_t*)kp[l], (half_t*)vp[l], len_stride,
                                 m->rope, pos, m->attn, starts, smax, live};
            HIPCHK(launch_llm_step_attention(a, B, st));
        }
        CGCHK(gemm(m, DEC_F16_RESID, m->attn, H, L.wo, H, m->h, H, m->h, B, st, live));
        HIPCHK(launch_llm_rmsnorm(m->h, L.ln2, H, c.rms_eps, m->xn, B, st, live));
        CGCHK(gemm(m, DEC_SWIGLU, m->xn, H, L.wgu, 2 * c.mlp, m->act, c.mlp, nullptr, B, st, live));
        CGCHK(gemm(m, DEC_F16_RESID, m->act, c.mlp, L.wdown, H, m->h, H, m->h, B, st, live));
    }
    HIPCHK(launch_llm_rmsnorm(m->h, m->norm, H, c.rms_eps, m->xn, B, st, live));
    return gemm(m, DEC_F32, m->xn, H, Mat{m->lm_head}, c.vocab, logits, ld_logits, nullptr, B, st, live);
}

// C[M, N] = A[M, K] * W[N, K]^T, fp16 result of the fp32 sum, through the large-shape GEMM of the ViT (gemm.hip / gemm9.hip).
// On an int8 handle the matrix is first expanded into the handle's scratch (all up256(N) rows, pad rows zeros), on the same stream:
// the expansion of the next matrix is ordered behind this GEMM, so one scratch serves every layer.
cgpt_status big_gemm(cgpt_llm* m, const half_t* A, int K, const Mat& Wm, int N, half_t* out, int64_t M, hipStream_t st) {
    const LlmCfg& c = m->cfg;
    const half_t* W = Wm.w;
    if (c.act_format && Wm.q) {     // activations-int8 handle: the token step's two launches on M rows (row tiles on the grid's second
        HIPCHK(launch_act_quant(A, M, K, c.act_threshold, c.outlier_cap, m->p_a8, m->p_sa, m->p_lists, m->act_counters, st));
        HIPCHK(launch_i8_gemm(DEC_F16, i8_params(m->p_a8, m->p_sa, m->p_lists, c.outlier_cap, Wm.q, Wm.s, out, N, nullptr, m->slabs, M, N, K), st));
        return CGPT_OK;
    }
    if (Wm.q) {
        HIPCHK(launch_llm_dequant(Wm.q, Wm.s, N, K, m->scratch, st));
        W = m->scratch;
    }
    GemmParams p{};
    p.A = A; p.lda = K; p.W = W; p.ldw = K; p.bias = nullptr; p.out = out; p.ldo = N; p.aux = nullptr; p.ldaux = 0;
    p.M = (int)M; p.N = N; p.K = K; p.patches = 0;
    HIPCHK(launch_gemm(EPI_F16, p, st));
    return CGPT_OK;
}

// The layers of the prefill and of the scoring pass on M token rows of the prefill workspace: x (layer 0's input rows) -> m->p_h,
// with the last layer's down projection left PENDING in m->p_proj: the residual stream stays fp16 as in HF, and a projection's output
// is added by the NEXT add + RMSNorm pass.  attention(l) enqueues what turns m->p_qkv into m->p_attn and returns the launch's error.
template <typename Attn>
cgpt_status run_layers(cgpt_llm* m, const half_t* x, int64_t M, hipStream_t st, Attn attention) {
    const cgpt_llm_config& c = m->cfg;
    const int H = c.hidden, F = c.mlp;
    const half_t* pending = nullptr;
    for (int l = 0; l < c.layers; ++l) {
        const Layer& Lw = m->layers[l];
        HIPCHK(launch_prefill_addnorm(x, pending, 1, 0, Lw.ln1, H, c.rms_eps, m->p_h, m->p_xn, M, st));
        x = m->p_h;
        CGCHK(big_gemm(m, m->p_xn, H, Lw.wqkv, qkv_width(c), m->p_qkv, M, st));
        HIPCHK(attention(l));
        CGCHK(big_gemm(m, m->p_attn, H, Lw.wo, H, m->p_proj, M, st));
        HIPCHK(launch_prefill_addnorm(m->p_h, m->p_proj, 1, 0, Lw.ln2, H, c.rms_eps, m->p_h, m->p_xn, M, st));
        CGCHK(big_gemm(m, m->p_xn, H, Lw.wgu, 2 * F, m->p_gu, M, st));
        HIPCHK(launch_prefill_swiglu(m->p_gu, M, F, m->p_act, st));
        CGCHK(big_gemm(m, m->p_act, F, Lw.wdown, H, m->p_proj, M, st));
        pending = m->p_proj;
    }
    return CGPT_OK;
}

// The prefill of B prompts of L positions: embeds [B, L, hidden] -> cache rows 0 .. L-1 of every layer, last-position logits.
// starts (device, or null): row b is left-padded by start[b] positions.  Only the rotary and attention kernels look at it; pad
// rows pass through the row-independent kernels and GEMMs like any other row (zero embeds stay zeros).  pos0 > 0
// (cgpt_llm_prefill_from): the L positions follow pos0 positions whose cache rows exist; rotary and attention are the _from twins.
cgpt_status run_prefill(cgpt_llm* m, const half_t* embeds, int B, int L, const int32_t* starts, void* const* kp, void* const* vp,
                        int64_t len_stride, float* logits, hipStream_t st, int pos0 = 0) {
    const cgpt_llm_config& c = m->cfg;
    const int H = c.hidden;
    CGCHK(run_layers(m, embeds, (int64_t)B * L, st, [&](int l) {
        half_t *K = (half_t*)kp[l], *V = (half_t*)vp[l];
        const hipError_t e = pos0 > 0 ? launch_prefill_rope_from(m->p_qkv, B, pos0, L, H, c.heads, c.kv_heads, K, V, len_stride, m->rope, starts, st)
                                      : launch_prefill_rope(m->p_qkv, B, L, H, c.heads, c.kv_heads, K, V, len_stride, m->rope, starts, st);
        if (e != hipSuccess) return e;
        return pos0 > 0 ? launch_prefill_attention_from(m->p_qkv, B, pos0, L, H, c.heads, c.kv_heads, K, V, len_stride, m->p_attn, starts, st)
                        : launch_prefill_attention(m->p_qkv, B, L, H, c.heads, c.kv_heads, K, V, len_stride, m->p_attn, starts, st);
    }));
    // tail, as run_step ends: the last position's row of every prompt (with its pending update) into the step workspace
    HIPCHK(launch_prefill_addnorm(m->p_h, m->p_proj, L, L - 1, m->norm, H, c.rms_eps, m->h, m->xn, B, st));
    return gemm(m, DEC_F32, m->xn, H, Mat{m->lm_head}, c.vocab, logits, c.vocab, nullptr, B, st);
}

constexpr int64_t SCORE_LOGIT_ROWS = 4096;                 // tail rows whose fp16 logits are held at once (262 MB at 32 000 columns)

// All candidates of `t` on the prompt cache rows 0 .. L-1 of B prompt rows: out[b, c] = summed label-smoothed cross-entropy.
// run_prefill's layers on the R = B S tail rows with the tail attention in place of rotary + cache write + causal attention; then
// lm_head and the cross-entropy in chunks of the reserved logits rows.  No cache row is written.  starts / row_lens: see llm.h.
cgpt_status run_score(cgpt_llm* m, const float* first_logits, int B, int L, const int32_t* starts, const long long* cand_tokens,
                      const int32_t* row_lens, const ScoreCands& t, float eps, void* const* kp, void* const* vp, int64_t len_stride,
                      float* out, hipStream_t st) {
    const cgpt_llm_config& c = m->cfg;
    const int H = c.hidden, S = t.off[t.n];
    const int64_t R = (int64_t)B * S;
    HIPCHK(launch_score_ce_first(first_logits, c.vocab, cand_tokens, t, B, eps, m->s_ce_buf, st, row_lens));
    if (S > 0) {
        HIPCHK(launch_score_embed(cand_tokens, t, B, m->embed, c.vocab, H, m->p_h, st, row_lens != nullptr));
        CGCHK(run_layers(m, m->p_h, R, st, [&](int l) {
            return launch_score_attention(m->p_qkv, t, B, L, H, c.heads, c.kv_heads, (const half_t*)kp[l], (const half_t*)vp[l], len_stride, m->rope,
                                          m->p_attn, st, starts);
        }));
        HIPCHK(launch_prefill_addnorm(m->p_h, m->p_proj, 1, 0, m->norm, H, c.rms_eps, m->p_h, m->p_xn, R, st));
        for (int64_t r0 = 0; r0 < R; r0 += m->s_rows) {        // chunks begin at multiples of 256 rows: whole GEMM row tiles
            const int64_t n = std::min(m->s_rows, R - r0);
            CGCHK(big_gemm(m, m->p_xn + r0 * H, H, Mat{m->lm_head}, c.vocab, m->s_logits, n, st));
            HIPCHK(launch_score_ce_tail(m->s_logits, c.vocab, cand_tokens, t, r0, n, eps, m->s_ce_buf, st, row_lens));
        }
    }
    HIPCHK(launch_score_sum(m->s_ce_buf, t, B, out, st, row_lens));
    return CGPT_OK;
}

}  // namespace

extern "C" {

cgpt_status cgpt_llm_create(const cgpt_llm_config* cfg, cgpt_llm_handle* out) {
    if (!cfg || !out) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: null argument");
    // three sizes are valid: the struct up to max_len (callers built before weight_format existed: fp16), the whole struct, and
    // cgpt_llm_config_gqa (the struct is then the `base` of one, and the switches behind it are read)
    constexpr int32_t kOldSize = (int32_t)offsetof(cgpt_llm_config, weight_format);
    constexpr int32_t kGqaSize = (int32_t)sizeof(cgpt_llm_config_gqa);
    constexpr int32_t kActSize = (int32_t)sizeof(cgpt_llm_config_act);
    static_assert(offsetof(cgpt_llm_config_act, act_format) == sizeof(cgpt_llm_config_gqa) && sizeof(cgpt_llm_config_act) % 8 == 0,
                  "the activation fields follow the gqa struct without padding");
    static_assert(offsetof(cgpt_llm_config_gqa, grouped_kv) == sizeof(cgpt_llm_config), "the switches follow the base without padding");
    if (cfg->struct_size != (int32_t)sizeof(cgpt_llm_config) && cfg->struct_size != kGqaSize && cfg->struct_size != kOldSize &&
        cfg->struct_size != kActSize)
        return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: cgpt_llm_config.struct_size mismatch (header/library drift)");
    LlmCfg c{};
    memcpy(static_cast<cgpt_llm_config*>(&c), cfg, std::min((size_t)cfg->struct_size, sizeof(cgpt_llm_config)));
    if (cfg->struct_size == kOldSize) c.weight_format = CGPT_LLM_W_F16;
    if (cfg->struct_size == kGqaSize || cfg->struct_size == kActSize) {
        const cgpt_llm_config_gqa* ext = reinterpret_cast<const cgpt_llm_config_gqa*>(cfg);
        if (ext->reserved != 0) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: cgpt_llm_config_gqa.reserved must be 0");
        c.grouped_kv = ext->grouped_kv;
    }
    c.act_format = 0;
    if (cfg->struct_size == kActSize) {
        const cgpt_llm_config_act* act = reinterpret_cast<const cgpt_llm_config_act*>(cfg);
        if (act->reserved2 != 0) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: cgpt_llm_config_act.reserved2 must be 0");
        if (act->act_format != CGPT_LLM_A_F16 && act->act_format != CGPT_LLM_A_INT8)
            return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: act_format must be CGPT_LLM_A_F16 (0) or CGPT_LLM_A_INT8 (1)");
        c.act_format = act->act_format;
        if (c.act_format) {
            c.act_threshold = act->act_threshold;
            c.outlier_cap = act->outlier_cap;
        }
    }
    c.struct_size = (int32_t)sizeof(cgpt_llm_config);
    if (c.weight_format != CGPT_LLM_W_F16 && c.weight_format != CGPT_LLM_W_INT8)
        return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: weight_format must be CGPT_LLM_W_F16 (0) or CGPT_LLM_W_INT8 (1)");
    if (c.act_format) {
        if (c.weight_format != CGPT_LLM_W_INT8)
            return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: act_format = CGPT_LLM_A_INT8 needs weight_format = CGPT_LLM_W_INT8 (int8 "
                                               "activations multiply int8 weights)");
        if (!(fabsf(c.act_threshold) <= 3.0e38f)) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: act_threshold must be finite");
        if (c.outlier_cap < 1 || c.outlier_cap > 1024) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: outlier_cap must be 1..1024");
        if (c.hidden % 128 || c.mlp % 128 || c.mlp > 65536)
            return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: act_format = CGPT_LLM_A_INT8 needs hidden and mlp multiples of 128 (one "
                                               "K-tile of the int8 kernel is 128 bytes) and mlp <= 65536");
    }
    if (c.head_dim != HD) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: head_dim must be 128");
    if (c.grouped_kv != 0 && c.grouped_kv != 1) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: grouped_kv must be 0 or 1");
    if (c.heads < 1 || (!c.grouped_kv && c.kv_heads != c.heads))
        return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: kv_heads must equal heads (grouped-query attention needs grouped_kv = 1)");
    if (c.grouped_kv) {
        const int G = (c.kv_heads >= 1 && c.kv_heads <= c.heads && c.heads % c.kv_heads == 0) ? c.heads / c.kv_heads : 0;
        if (G != 1 && G != 2 && G != 4 && G != 8)
            return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: grouped_kv needs 1 <= kv_heads <= heads, heads % kv_heads == 0 and "
                                               "heads / kv_heads in {1, 2, 4, 8}");
    }
    if (c.hidden < 64 || c.hidden % 64 || c.hidden != c.heads * HD)
        return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: hidden must be heads * 128 and a multiple of 64");
    if (c.layers < 1 || c.mlp < 64 || c.mlp % 64 || c.vocab < 64 || c.vocab % 64)
        return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: layers >= 1, mlp and vocab multiples of 64");
    if (c.max_batch < 1 || c.max_batch > MAX_ROWS) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: max_batch must be 1..256");
    if (c.max_len < 1 || c.max_len > 8192) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: max_len must be 1..8192");
    if (!(c.rms_eps > 0.0f) || !(c.rope_theta > 0.0f)) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: rms_eps and rope_theta must be positive");
    const int G = c.grouped_kv ? c.heads / c.kv_heads : 0;        // the step attention's kernel family (StepAttnArgs)
    if (G && llm_step_attn_lds_bytes(G, c.max_len) > LDS_PER_CU)
        return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: grouped_kv with heads / kv_heads = " + std::to_string(G) +
                                               " and max_len = " + std::to_string(c.max_len) + " needs " +
                                               std::to_string(llm_step_attn_lds_bytes(G, c.max_len)) +
                                               " bytes of LDS for the token step's scores, a CU has 163840: lower max_len");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return cgpt_fail(CGPT_ERR_NO_DEVICE, "cgpt_llm_create: no HIP device visible (this library has no CPU fallback)");
    if (c.device < 0 || c.device >= ndev) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_create: bad device ordinal");
    HIPCHK(hipSetDevice(c.device));
    HIPCHK(decode_gemm_prepare());                        // kernel attributes now: nothing but launches is left for a captured stream
    HIPCHK(score_prepare());
    if (c.act_format) HIPCHK(i8_gemm_prepare());
    HIPCHK(llm_step_prepare(G, c.max_len));               // the grouped step attention's dynamic LDS, for this handle's longest row
    cgpt_llm* m = new cgpt_llm();
    m->cfg = c;
    m->layers.resize(c.layers);
    m->expected = 3 + (size_t)c.layers * 9;
    const size_t H = c.hidden, F = c.mlp, V = c.vocab, hs = sizeof(half_t), NQ = (size_t)qkv_width(c);
    auto up256 = [](size_t n) { return (n + 255) / 256 * 256; };   // the prefill's GEMM reads whole 256-row tiles of W (pad rows: zeros)
    auto fail = [&](cgpt_status s) { cgpt_llm_destroy(m); return s; };
    cgpt_status s = CGPT_OK;
    auto za = [&](size_t bytes, void* out_ptr) { if (s == CGPT_OK) s = dev_zalloc(m, bytes, (void**)out_ptr); };
    const bool int8 = c.weight_format == CGPT_LLM_W_INT8;
    auto counted = [&](size_t bytes, void* out_ptr) { za(bytes, out_ptr); m->weight_bytes += (int64_t)bytes; };
    // a layer matrix [up256(N)][K]: fp16, or int8 with up256(N) fp16 row scales (pad rows: q = 0, s = 0)
    auto mat = [&](Mat& W, size_t N, size_t K) {
        if (int8) { counted(up256(N) * K, &W.q); counted(up256(N) * hs, &W.s); }
        else counted(up256(N) * K * hs, &W.w);
    };
    counted(V * H * hs, &m->embed);
    za(H * hs, &m->norm);
    // lm_head is read by the large-shape GEMM too (cgpt_llm_score): whole 256-row tiles, pad rows zeros.  Counted without them.
    za(up256(V) * H * hs, &m->lm_head);
    m->weight_bytes += (int64_t)(V * H * hs);
    for (Layer& L : m->layers) {
        mat(L.wqkv, NQ, H);
        mat(L.wo, H, H);
        mat(L.wgu, 2 * F, H);
        mat(L.wdown, H, F);
        za(H * hs, &L.ln1);
        za(H * hs, &L.ln2);
    }
    if (int8 && !c.act_format)                            // the largest fused layer matrix, up256(2 mlp) x hidden at LLaMA's shapes
        counted(std::max(std::max(up256(NQ) * H, up256(2 * F) * H), up256(H) * std::max(H, F)) * hs, &m->scratch);
    // activations: whole 256-row tiles (the GEMM stages every row of its tile; rows past the batch hold zeros)
    za(MAX_ROWS * H * hs, &m->h);
    za(MAX_ROWS * H * hs, &m->xn);
    za(MAX_ROWS * NQ * hs, &m->qkv);
    za(MAX_ROWS * H * hs, &m->attn);
    za(MAX_ROWS * F * hs, &m->act);
    za(MAX_ROWS * V * sizeof(float), &m->logits);
    za(MAX_ROWS * sizeof(long long), &m->tok);
    za(MAX_ROWS * sizeof(int), &m->unfinished);
    za(sizeof(int), &m->live);
    za(sizeof(int), &m->live_steps);
    size_t slab = 0;
    const int shapes[5][2] = {{(int)NQ, (int)H}, {(int)H, (int)H}, {(int)(2 * F), (int)H}, {(int)H, (int)F}, {(int)V, (int)H}};
    for (auto& sh : shapes) slab = std::max(slab, decode_gemm_slab_bytes(sh[0], sh[1]));
    if (c.act_format) {                                   // the int32 slabs of the int8 GEMM share the buffer; codes, scales, lists
        for (int i = 0; i < 4; ++i) slab = std::max(slab, i8_gemm_slab_bytes(shapes[i][0], shapes[i][1]));
        za(MAX_ROWS * std::max(H, F), &m->a8);
        za(MAX_ROWS * sizeof(float), &m->sa);
        za(MAX_ROWS * (size_t)(c.outlier_cap + 1) * sizeof(uint32_t), &m->lists);
        za(4 * sizeof(unsigned long long), &m->act_counters);
    }
    za(std::max(slab, (size_t)16), &m->slabs);
    za((size_t)c.max_len * HD * hs, &m->rope);
    float* inv_freq = nullptr;
    za(64 * sizeof(float), &inv_freq);
    if (s != CGPT_OK) return fail(s);
    float inv_host[64];
    for (int i = 0; i < 64; ++i) inv_host[i] = 1.0f / powf(c.rope_theta, (float)(2 * i) / (float)HD);
    if (hipMemcpy(inv_freq, inv_host, sizeof(inv_host), hipMemcpyHostToDevice) != hipSuccess)
        return fail(cgpt_fail(CGPT_ERR_HIP, "cgpt_llm_create: inv_freq upload failed"));
    if (launch_llm_rope_table(inv_freq, m->rope, c.max_len, 0) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(cgpt_fail(CGPT_ERR_HIP, "cgpt_llm_create: rotary table kernel failed"));
    *out = m;
    return CGPT_OK;
}

cgpt_status cgpt_llm_destroy(cgpt_llm_handle h) {
    if (!h) return CGPT_OK;
    (void)hipSetDevice(h->cfg.device);
    (void)hipDeviceSynchronize();
    for (void* p : h->allocs) (void)hipFree(p);
    delete h;
    return CGPT_OK;
}

cgpt_status cgpt_llm_weight_bytes(cgpt_llm_handle h, int64_t* out) {
    if (!h || !out) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_weight_bytes: null argument");
    *out = h->weight_bytes;
    return CGPT_OK;
}

cgpt_status cgpt_llm_act_stats(cgpt_llm_handle h, int64_t* out_host) {
    if (!h || !out_host) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_act_stats: null argument");
    for (int i = 0; i < 4; ++i) out_host[i] = 0;
    if (!h->cfg.act_format) return CGPT_OK;
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipDeviceSynchronize());
    unsigned long long v[4];
    HIPCHK(hipMemcpy(v, h->act_counters, sizeof(v), hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(h->act_counters, 0, sizeof(v)));
    for (int i = 0; i < 4; ++i) out_host[i] = (int64_t)v[i];
    return CGPT_OK;
}

int32_t cgpt_llm_linear_i8_slices(int64_t N, int64_t K) {
    if (N < 64 || N % 64 || N > (1 << 24) || K < 128 || K % 128 || K > 65536) return -1;
    return i8_gemm_splitk((int)N, (int)K);
}

int64_t cgpt_llm_linear_i8_workspace(int64_t M, int64_t N, int64_t K, int32_t outlier_cap, int64_t* offsets_out) {
    if (M < 1 || M > (1 << 24) || outlier_cap < 1 || outlier_cap > 1024 || cgpt_llm_linear_i8_slices(N, K) < 0) return -1;
    const int64_t rows = (M + 255) / 256 * 256;
    auto up = [](int64_t b) { return (b + 255) / 256 * 256; };
    int64_t off[5];
    off[0] = 0;
    off[1] = 256;
    off[2] = off[1] + up(rows * K);
    off[3] = off[2] + up(rows * 4);
    off[4] = off[3] + up(rows * (int64_t)(outlier_cap + 1) * 4);
    const int64_t total = off[4] + up(M <= 256 ? (int64_t)i8_gemm_slab_bytes((int)N, (int)K) : 0);
    if (offsets_out)
        for (int i = 0; i < 5; ++i) offsets_out[i] = off[i];
    return total;
}

cgpt_status cgpt_llm_linear_i8(const void* A_dev, const void* q_dev, const void* sw_dev, int64_t M, int64_t N, int64_t K, float threshold,
                               int32_t outlier_cap, int32_t epilogue, const void* resid_dev, void* out_dev, int64_t out_bytes,
                               void* workspace_dev, int64_t workspace_bytes, void* stream) {
    if (!A_dev || !q_dev || !sw_dev || !out_dev || !workspace_dev) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_linear_i8: null argument");
    int64_t off[5];
    const int64_t need = cgpt_llm_linear_i8_workspace(M, N, K, outlier_cap, off);
    if (need < 0)
        return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_linear_i8: bad sizes (1 <= M <= 2^24, N a multiple of 64, K a multiple of 128 up to "
                                           "65536, outlier_cap 1..1024)");
    if (epilogue != DEC_F16 && epilogue != DEC_F16_RESID && epilogue != DEC_SWIGLU)
        return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_linear_i8: epilogue must be 0 (fp16), 1 (fp16 + resid) or 2 (SwiGLU)");
    if (epilogue == DEC_F16_RESID && !resid_dev) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_linear_i8: epilogue 1 needs resid_dev");
    if (!(fabsf(threshold) <= 3.0e38f)) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_linear_i8: threshold must be finite");
    const int64_t ncols = epilogue == DEC_SWIGLU ? N / 2 : N;
    if (out_bytes < M * ncols * (int64_t)sizeof(half_t))
        return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_linear_i8: out_bytes " + std::to_string(out_bytes) + " < " +
                                               std::to_string(M * ncols * (int64_t)sizeof(half_t)) + " the result needs");
    if (workspace_bytes < need)
        return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_linear_i8: workspace_bytes " + std::to_string(workspace_bytes) + " < " +
                                               std::to_string(need) + " (cgpt_llm_linear_i8_workspace)");
    if ((uintptr_t)workspace_dev % 256) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_linear_i8: workspace_dev must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace_dev;
    HIPCHK(i8_gemm_prepare());
    HIPCHK(hipMemsetAsync(ws + off[0], 0, 4 * sizeof(unsigned long long), st));
    HIPCHK(launch_act_quant((const half_t*)A_dev, M, (int)K, threshold, outlier_cap, (signed char*)(ws + off[1]), (float*)(ws + off[2]),
                            (uint32_t*)(ws + off[3]), (unsigned long long*)(ws + off[0]), st));
    const I8GemmParams p = i8_params((const signed char*)(ws + off[1]), (const float*)(ws + off[2]), (const uint32_t*)(ws + off[3]), outlier_cap,
                                     (const signed char*)q_dev, (const half_t*)sw_dev, out_dev, ncols, (const half_t*)resid_dev, ws + off[4], M, (int)N, (int)K);
    HIPCHK(launch_i8_gemm(epilogue, p, st));
    return CGPT_OK;
}

cgpt_status cgpt_llm_load_weight_f16(cgpt_llm_handle h, const char* name, const void* data_dev, int64_t numel, void* stream) {
    if (!h || !name || !data_dev) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_load_weight_f16: null argument");
    const cgpt_llm_config& c = h->cfg;
    const int64_t H = c.hidden, F = c.mlp, V = c.vocab, KV = (int64_t)c.kv_heads * HD;       // KV == H on a plain handle
    hipStream_t st = (hipStream_t)stream;
    const std::string n(name);
    half_t* dst = nullptr;
    const Mat* mat = nullptr;                              // a layer linear: `row0` = its first row in the fused matrix, K = its columns
    int64_t want = 0, row0 = 0, K = 0;
    int interleave = -1;                                   // 0 = gate, 1 = up: rows go to alternate blocks of 16
    if (n == "model.embed_tokens.weight") { dst = h->embed; want = V * H; }
    else if (n == "model.norm.weight") { dst = h->norm; want = H; }
    else if (n == "lm_head.weight") { dst = h->lm_head; want = V * H; }
    else {
        int li = -1, used = 0;
        if (sscanf(name, "model.layers.%d.%n", &li, &used) != 1 || li < 0 || li >= c.layers)
            return cgpt_fail(CGPT_ERR_NOT_FOUND, "cgpt_llm_load_weight_f16: unknown weight '" + n + "'");
        const std::string rest(name + used);
        Layer& L = h->layers[li];
        if (rest == "self_attn.q_proj.weight") { mat = &L.wqkv; want = H * H; K = H; }
        else if (rest == "self_attn.k_proj.weight") { mat = &L.wqkv; row0 = H; want = KV * H; K = H; }
        else if (rest == "self_attn.v_proj.weight") { mat = &L.wqkv; row0 = H + KV; want = KV * H; K = H; }
        else if (rest == "self_attn.o_proj.weight") { mat = &L.wo; want = H * H; K = H; }
        else if (rest == "mlp.gate_proj.weight") { mat = &L.wgu; want = F * H; K = H; interleave = 0; }
        else if (rest == "mlp.up_proj.weight") { mat = &L.wgu; want = F * H; K = H; interleave = 1; }
        else if (rest == "mlp.down_proj.weight") { mat = &L.wdown; want = H * F; K = F; }
        else if (rest == "input_layernorm.weight") { dst = L.ln1; want = H; }
        else if (rest == "post_attention_layernorm.weight") { dst = L.ln2; want = H; }
        else return cgpt_fail(CGPT_ERR_NOT_FOUND, "cgpt_llm_load_weight_f16: unknown weight '" + n + "'");
    }
    if (numel != want)
        return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_load_weight_f16: '" + n + "' expects " + std::to_string(want) + " elements, got " +
                                               std::to_string(numel));
    HIPCHK(hipSetDevice(c.device));
    if (mat && mat->q) {                                   // int8 handle: quantise the caller's rows straight into the fused matrix
        HIPCHK(launch_llm_quant_rows((const half_t*)data_dev, (int)(want / K), (int)K, interleave, mat->q + row0 * K, mat->s + row0, st));
        h->loaded.insert(n);
        return CGPT_OK;
    }
    if (mat) dst = mat->w + row0 * K;
    if (interleave < 0) {
        HIPCHK(hipMemcpyAsync(dst, data_dev, (size_t)want * sizeof(half_t), hipMemcpyDeviceToDevice, st));
    } else {                                               // 16 source rows -> rows 32 t + 16 * interleave .. of the fused matrix
        const size_t blk = (size_t)16 * H * sizeof(half_t);
        HIPCHK(hipMemcpy2DAsync(dst + (int64_t)interleave * 16 * H, 2 * blk, data_dev, blk, blk, (size_t)(F / 16),
                                hipMemcpyDeviceToDevice, st));
    }
    h->loaded.insert(n);
    return CGPT_OK;
}

// The plain and the _ragged entries share one body each: `who` names the entry in messages, starts == null is the plain one.
static cgpt_status llm_step_entry(const char* who, cgpt_llm_handle h, const int64_t* tokens_dev, int32_t B, int32_t pos,
                                  const int32_t* starts_dev, void* const* k_ptrs_host, void* const* v_ptrs_host, int64_t kv_len_stride,
                                  float* logits_dev, void* stream) {
    if (!h || !tokens_dev || !logits_dev) return cgpt_fail(CGPT_ERR_INVALID, std::string(who) + ": null argument");
    CGCHK(ready(h, who));
    HIPCHK(hipSetDevice(h->cfg.device));
    CGCHK(check_cache(h, who, B, pos, k_ptrs_host, v_ptrs_host, kv_len_stride));
    return run_step(h, nullptr, (const long long*)tokens_dev, B, pos, starts_dev, pos, k_ptrs_host, v_ptrs_host, kv_len_stride, logits_dev,
                    h->cfg.vocab, (hipStream_t)stream);
}

cgpt_status cgpt_llm_step(cgpt_llm_handle h, const int64_t* tokens_dev, int32_t B, int32_t pos, void* const* k_ptrs_host,
                          void* const* v_ptrs_host, int64_t kv_len_stride, float* logits_dev, void* stream) {
    return llm_step_entry("cgpt_llm_step", h, tokens_dev, B, pos, nullptr, k_ptrs_host, v_ptrs_host, kv_len_stride, logits_dev, stream);
}

cgpt_status cgpt_llm_step_ragged(cgpt_llm_handle h, const int64_t* tokens_dev, int32_t B, int32_t pos, const int32_t* starts_dev,
                                 void* const* k_ptrs_host, void* const* v_ptrs_host, int64_t kv_len_stride, float* logits_dev,
                                 void* stream) {
    if (!starts_dev) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_step_ragged: null starts_dev");
    return llm_step_entry("cgpt_llm_step_ragged", h, tokens_dev, B, pos, starts_dev, k_ptrs_host, v_ptrs_host, kv_len_stride, logits_dev,
                          stream);
}

static cgpt_status llm_greedy_entry(const char* who_c, cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t prompt_len,
                                    const int32_t* starts_dev, int32_t num_new, int32_t min_new, const int64_t* eos_ids_host,
                                    int32_t num_eos, int64_t pad_id, void* const* k_ptrs_host, void* const* v_ptrs_host,
                                    int64_t kv_len_stride, int64_t* tokens_out_dev, float* step_logits_out_dev, void* stream,
                                    const cgpt_llm_sample_params* sample = nullptr, const int64_t* draw_ids_dev = nullptr,
                                    const uint64_t* seed_dev = nullptr, bool constrained = false, int32_t* labels_out_dev = nullptr) {
    const std::string who(who_c);
    if (!h || !first_logits_dev || !tokens_out_dev) return cgpt_fail(CGPT_ERR_INVALID, who + ": null argument");
    if (constrained) {                                     // the constrained entries: only the select launch differs
        if (!labels_out_dev) return cgpt_fail(CGPT_ERR_INVALID, who + ": null labels_out_dev");
        if (h->t_nodes == 0) return cgpt_fail(CGPT_ERR_INVALID, who + ": no trie is set on the handle (cgpt_llm_set_trie)");
        if (num_new != h->t_depth)
            return cgpt_fail(CGPT_ERR_INVALID, who + ": num_new " + std::to_string(num_new) + " is not the trie's depth " +
                                                   std::to_string(h->t_depth));
    }
    SampleLaw law{};                                       // the sampling entries (sample != null): only the select launch differs
    if (sample) {
        if (!draw_ids_dev || !seed_dev) return cgpt_fail(CGPT_ERR_INVALID, who + ": null draw_ids_dev or seed_dev");
        CGCHK(check_sample_params(who, *sample, h->cfg.vocab, num_new > 0 ? num_new - 1 : 0, num_eos > 0 ? num_eos : 0, &law));
    }
    if (num_new < 1 || prompt_len < 1 || min_new < 0 || num_eos < 0 || num_eos > MAX_EOS || (num_eos > 0 && !eos_ids_host))
        return cgpt_fail(CGPT_ERR_INVALID, who + ": bad lengths (num_new, prompt_len >= 1; at most 8 EOS ids)");
    CGCHK(ready(h, who_c));
    HIPCHK(hipSetDevice(h->cfg.device));
    // the last step appends at prompt_len + num_new - 2; with num_new == 1 no step runs but the table must still be sane
    CGCHK(check_cache(h, who_c, B, num_new > 1 ? prompt_len + num_new - 2 : 0, k_ptrs_host, v_ptrs_host,
                      num_new > 1 ? kv_len_stride : 1));
    hipStream_t st = (hipStream_t)stream;
    EosIds eos{};
    eos.n = num_eos;
    for (int e = 0; e < num_eos; ++e) eos.id[e] = eos_ids_host[e];
    const int V = h->cfg.vocab;
    const int64_t ld_out = (int64_t)num_new * V;
    const bool early = h->early_stop != 0;                 // read now: a captured call keeps the setting it was captured under
    StopSeqs stop = h->stop;                               // likewise; `col` is set per select below
    h->last_on = early ? 1 : 0;
    h->off_steps = num_new - 1;
    for (int i = 0; i < num_new; ++i) {
        const bool own = i > 0 && step_logits_out_dev;     // the step before wrote its logits into the caller's buffer
        const float* src = i == 0 ? first_logits_dev : own ? step_logits_out_dev + (int64_t)i * V : h->logits;
        const int64_t lds = own ? ld_out : (int64_t)V;
        const int mask = (i < min_new && num_eos > 0) ? 1 : 0;
        float* dst = step_logits_out_dev && (i == 0 || mask) ? step_logits_out_dev + (int64_t)i * V : nullptr;
        stop.col = i;
        const int first = i == 0 ? 1 : 0;
        const int* live = early ? h->live : nullptr;
        const SelectArgs a{src, lds, dst, ld_out, V, mask, eos, (long long)pad_id, first, h->unfinished,
                           (long long*)tokens_out_dev + i, (int64_t)num_new, h->tok, live};
        if (constrained) {                                 // tables as the handle holds them now: a captured call keeps them
            if (i == 0 && step_logits_out_dev) HIPCHK(launch_llm_copy_rows(first_logits_dev, V, step_logits_out_dev, ld_out, V, B, st));
            TrieArgs ta{src, lds, h->t_begin, h->t_tok, h->t_node, h->t_leaf, h->t_nodes, a.pad, first, h->trie_node,
                        h->unfinished, a.tokens_out, a.ld_tokens, h->tok, labels_out_dev, live};
            HIPCHK(launch_llm_trie_select(early, ta, B, st));
        } else if (sample) {
            SampleIo io{(const long long*)tokens_out_dev, (int64_t)num_new, i, i, (const long long*)draw_ids_dev,
                        (const unsigned long long*)seed_dev, nullptr, nullptr, nullptr, nullptr};
            HIPCHK(launch_llm_sample(early, stop.n > 0 ? &stop : nullptr, a, law, io, B, st));
        } else {
            HIPCHK(launch_llm_select(early, stop.n > 0 ? &stop : nullptr, a, B, st));
        }
        if (early) HIPCHK(launch_llm_live(h->unfinished, B, first, i + 1 < num_new ? 1 : 0, h->live, h->live_steps, st));
        if (i + 1 == num_new) break;
        float* next = step_logits_out_dev ? step_logits_out_dev + (int64_t)(i + 1) * V : h->logits;
        CGCHK(run_step(h, live, h->tok, B, prompt_len + i, starts_dev, prompt_len - 1, k_ptrs_host, v_ptrs_host, kv_len_stride, next,
                       step_logits_out_dev ? ld_out : (int64_t)V, st));
    }
    return CGPT_OK;
}

cgpt_status cgpt_llm_greedy(cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t prompt_len, int32_t num_new,
                            int32_t min_new, const int64_t* eos_ids_host, int32_t num_eos, int64_t pad_id, void* const* k_ptrs_host,
                            void* const* v_ptrs_host, int64_t kv_len_stride, int64_t* tokens_out_dev, float* step_logits_out_dev,
                            void* stream) {
    return llm_greedy_entry("cgpt_llm_greedy", h, first_logits_dev, B, prompt_len, nullptr, num_new, min_new, eos_ids_host, num_eos, pad_id,
                            k_ptrs_host, v_ptrs_host, kv_len_stride, tokens_out_dev, step_logits_out_dev, stream);
}

cgpt_status cgpt_llm_greedy_ragged(cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t prompt_len,
                                   const int32_t* starts_dev, int32_t num_new, int32_t min_new, const int64_t* eos_ids_host,
                                   int32_t num_eos, int64_t pad_id, void* const* k_ptrs_host, void* const* v_ptrs_host,
                                   int64_t kv_len_stride, int64_t* tokens_out_dev, float* step_logits_out_dev, void* stream) {
    if (!starts_dev) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_greedy_ragged: null starts_dev");
    return llm_greedy_entry("cgpt_llm_greedy_ragged", h, first_logits_dev, B, prompt_len, starts_dev, num_new, min_new, eos_ids_host,
                            num_eos, pad_id, k_ptrs_host, v_ptrs_host, kv_len_stride, tokens_out_dev, step_logits_out_dev, stream);
}

cgpt_status cgpt_llm_sample(cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t prompt_len, int32_t num_new,
                            int32_t min_new, const int64_t* eos_ids_host, int32_t num_eos, int64_t pad_id, void* const* k_ptrs_host,
                            void* const* v_ptrs_host, int64_t kv_len_stride, int64_t* tokens_out_dev, float* step_logits_out_dev,
                            cgpt_llm_sample_params params, const int64_t* draw_ids_dev, const uint64_t* seed_dev, void* stream) {
    return llm_greedy_entry("cgpt_llm_sample", h, first_logits_dev, B, prompt_len, nullptr, num_new, min_new, eos_ids_host, num_eos, pad_id,
                            k_ptrs_host, v_ptrs_host, kv_len_stride, tokens_out_dev, step_logits_out_dev, stream, &params, draw_ids_dev,
                            seed_dev);
}

cgpt_status cgpt_llm_sample_ragged(cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t prompt_len,
                                   const int32_t* starts_dev, int32_t num_new, int32_t min_new, const int64_t* eos_ids_host,
                                   int32_t num_eos, int64_t pad_id, void* const* k_ptrs_host, void* const* v_ptrs_host,
                                   int64_t kv_len_stride, int64_t* tokens_out_dev, float* step_logits_out_dev,
                                   cgpt_llm_sample_params params, const int64_t* draw_ids_dev, const uint64_t* seed_dev, void* stream) {
    if (!starts_dev) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_sample_ragged: null starts_dev");
    return llm_greedy_entry("cgpt_llm_sample_ragged", h, first_logits_dev, B, prompt_len, starts_dev, num_new, min_new, eos_ids_host,
                            num_eos, pad_id, k_ptrs_host, v_ptrs_host, kv_len_stride, tokens_out_dev, step_logits_out_dev, stream, &params,
                            draw_ids_dev, seed_dev);
}

cgpt_status cgpt_llm_constrained(cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t prompt_len, int32_t num_new,
                                 int64_t pad_id, void* const* k_ptrs_host, void* const* v_ptrs_host, int64_t kv_len_stride,
                                 int64_t* tokens_out_dev, float* step_logits_out_dev, int32_t* labels_out_dev, void* stream) {
    return llm_greedy_entry("cgpt_llm_constrained", h, first_logits_dev, B, prompt_len, nullptr, num_new, 0, nullptr, 0, pad_id, k_ptrs_host,
                            v_ptrs_host, kv_len_stride, tokens_out_dev, step_logits_out_dev, stream, nullptr, nullptr, nullptr, true,
                            labels_out_dev);
}

cgpt_status cgpt_llm_constrained_ragged(cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t prompt_len,
                                        const int32_t* starts_dev, int32_t num_new, int64_t pad_id, void* const* k_ptrs_host,
                                        void* const* v_ptrs_host, int64_t kv_len_stride, int64_t* tokens_out_dev,
                                        float* step_logits_out_dev, int32_t* labels_out_dev, void* stream) {
    if (!starts_dev) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_constrained_ragged: null starts_dev");
    return llm_greedy_entry("cgpt_llm_constrained_ragged", h, first_logits_dev, B, prompt_len, starts_dev, num_new, 0, nullptr, 0, pad_id,
                            k_ptrs_host, v_ptrs_host, kv_len_stride, tokens_out_dev, step_logits_out_dev, stream, nullptr, nullptr, nullptr,
                            true, labels_out_dev);
}

// ---- beam search (llm_beam.hip; include/cgpt.h: "Beam search")
cgpt_status cgpt_llm_beam_reserve(cgpt_llm_handle h, int32_t max_images, int32_t k, int32_t num_new) {
    const std::string who = "cgpt_llm_beam_reserve";
    if (!h) return cgpt_fail(CGPT_ERR_INVALID, who + ": null handle");
    if (k < BEAM_MIN || k > BEAM_MAX)
        return cgpt_fail(CGPT_ERR_INVALID, who + ": num_beams " + std::to_string(k) + " outside " + std::to_string(BEAM_MIN) + ".." +
                                               std::to_string(BEAM_MAX));
    if (max_images < 1 || (int64_t)max_images * k > h->cfg.max_batch)
        return cgpt_fail(CGPT_ERR_INVALID, who + ": " + std::to_string(max_images) + " images x " + std::to_string(k) +
                                               " beams outside 1..max_batch = " + std::to_string(h->cfg.max_batch) + " rows");
    if (num_new < 1 || num_new > h->cfg.max_len) return cgpt_fail(CGPT_ERR_INVALID, who + ": num_new outside 1..max_len");
    const int64_t rows = (int64_t)max_images * k, elems = rows * num_new;
    if (rows <= h->bm_rows && elems <= h->bm_elems) return CGPT_OK;    // grows only; a second call with the same sizes does nothing
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t R = (size_t)std::max(rows, h->bm_rows), E = (size_t)std::max(elems, h->bm_elems);
    Staging stage;
    BeamState fresh[2]{};                                              // complete before it takes the old sets' place
    for (BeamState& s : fresh) {
        stage.add(&s.running, R * sizeof(float));
        stage.add(&s.tokens, E * sizeof(long long));
        stage.add(&s.anc, E * sizeof(int32_t));
        stage.add(&s.pool_score, R * sizeof(float));
        stage.add(&s.pool_fin, R * sizeof(int32_t));
        stage.add(&s.pool_len, R * sizeof(int32_t));
        stage.add(&s.pool_seq, E * sizeof(long long));
        stage.add(&s.open, R * sizeof(int32_t));
    }
    int32_t* parents = nullptr;
    stage.add(&parents, R * sizeof(int32_t));
    CGCHK(stage.commit(h, who));
    h->bm[0] = fresh[0]; h->bm[1] = fresh[1]; h->bm_parents = parents;
    h->bm_rows = (int64_t)R; h->bm_elems = (int64_t)E;
    return CGPT_OK;
}

// The checks a beam step and the beam loop share: the handle, the rows, both cache sets.  last_t: the last generated position appended.
static cgpt_status beam_check(const std::string& who, cgpt_llm_handle h, int32_t B, int32_t k, int32_t L, int32_t last_t, bool steps,
                              void* const* pk, void* const* pv, int64_t prompt_stride, void* const* bk, void* const* bv, int64_t beam_stride) {
    if (h->cfg.grouped_kv) return cgpt_fail(CGPT_ERR_INVALID, who + ": a grouped_kv handle is not supported (beam search runs on plain handles)");
    if (k < BEAM_MIN || k > BEAM_MAX)
        return cgpt_fail(CGPT_ERR_INVALID, who + ": num_beams " + std::to_string(k) + " outside " + std::to_string(BEAM_MIN) + ".." +
                                               std::to_string(BEAM_MAX));
    if (B < 1 || (int64_t)B * k > h->cfg.max_batch)
        return cgpt_fail(CGPT_ERR_INVALID, who + ": B * num_beams = " + std::to_string(B) + " * " + std::to_string(k) + " outside 1..max_batch = " +
                                               std::to_string(h->cfg.max_batch));
    if (L < 1 || last_t < 0 || (int64_t)L + last_t >= h->cfg.max_len)
        return cgpt_fail(CGPT_ERR_INVALID, who + ": prompt_len >= 1, t >= 0 and prompt_len + t < max_len are required");
    if (!pk || !pv) return cgpt_fail(CGPT_ERR_INVALID, who + ": null prompt K/V pointer table");
    if (L > prompt_stride) return cgpt_fail(CGPT_ERR_INVALID, who + ": prompt_len exceeds prompt_stride");
    for (int l = 0; l < h->cfg.layers; ++l)
        if (!pk[l] || !pv[l]) return cgpt_fail(CGPT_ERR_INVALID, who + ": null prompt K/V buffer");
    if (steps) {
        if (!bk || !bv) return cgpt_fail(CGPT_ERR_INVALID, who + ": null beam K/V pointer table");
        if (last_t >= beam_stride) return cgpt_fail(CGPT_ERR_INVALID, who + ": generated position outside the beam cache (beam_stride)");
        for (int l = 0; l < h->cfg.layers; ++l)
            if (!bk[l] || !bv[l]) return cgpt_fail(CGPT_ERR_INVALID, who + ": null beam K/V buffer");
    }
    return CGPT_OK;
}

cgpt_status cgpt_llm_beam_step(cgpt_llm_handle h, const int64_t* tokens_dev, int32_t B, int32_t k, int32_t prompt_len, int32_t t,
                               const int32_t* anc_dev, int64_t anc_ld, void* const* prompt_k_ptrs_host, void* const* prompt_v_ptrs_host,
                               int64_t prompt_stride, void* const* beam_k_ptrs_host, void* const* beam_v_ptrs_host, int64_t beam_stride,
                               float* logits_dev, void* stream) {
    const std::string who = "cgpt_llm_beam_step";
    if (!h || !tokens_dev || !logits_dev || !anc_dev) return cgpt_fail(CGPT_ERR_INVALID, who + ": null argument");
    if (anc_ld < t) return cgpt_fail(CGPT_ERR_INVALID, who + ": anc_ld < t");
    CGCHK(beam_check(who, h, B, k, prompt_len, t, true, prompt_k_ptrs_host, prompt_v_ptrs_host, prompt_stride, beam_k_ptrs_host,
                     beam_v_ptrs_host, beam_stride));
    CGCHK(ready(h, who.c_str()));
    HIPCHK(hipSetDevice(h->cfg.device));
    const BeamStep bs{prompt_k_ptrs_host, prompt_v_ptrs_host, prompt_stride, anc_dev, anc_ld, k, prompt_len, t};
    return run_step(h, nullptr, (const long long*)tokens_dev, B * k, prompt_len + t, nullptr, 0, beam_k_ptrs_host, beam_v_ptrs_host, beam_stride,
                           logits_dev, h->cfg.vocab, (hipStream_t)stream, &bs);
}

cgpt_status cgpt_llm_beam(cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t k, int32_t prompt_len, int32_t num_new,
                          int32_t min_new, const int64_t* eos_ids_host, int32_t num_eos, int64_t pad_id, float length_penalty,
                          void* const* prompt_k_ptrs_host, void* const* prompt_v_ptrs_host, int64_t prompt_stride,
                          void* const* beam_k_ptrs_host, void* const* beam_v_ptrs_host, int64_t beam_stride, int64_t* tokens_out_dev,
                          float* scores_out_dev, float* step_logits_out_dev, float* trace_out_dev, void* stream) {
    const std::string who = "cgpt_llm_beam";
    if (!h || !first_logits_dev || !tokens_out_dev) return cgpt_fail(CGPT_ERR_INVALID, who + ": null argument");
    if (num_new < 1 || min_new < 0 || num_eos < 0 || num_eos > MAX_EOS || (num_eos > 0 && !eos_ids_host))
        return cgpt_fail(CGPT_ERR_INVALID, who + ": bad lengths (num_new >= 1, min_new >= 0; at most 8 EOS ids)");
    if (!(length_penalty == length_penalty) || fabsf(length_penalty) == INFINITY)
        return cgpt_fail(CGPT_ERR_INVALID, who + ": length_penalty is not finite");
    CGCHK(beam_check(who, h, B, k, prompt_len, num_new > 1 ? num_new - 2 : 0, num_new > 1, prompt_k_ptrs_host, prompt_v_ptrs_host,
                     prompt_stride, beam_k_ptrs_host, beam_v_ptrs_host, beam_stride));
    const int V = h->cfg.vocab, K = std::max(2, 1 + num_eos) * k;
    if (V < K + num_eos || V > BEAM_MAX_VOCAB)           // K unmasked columns in beam 0's row: the -1e9 beams never enter select 0's top K
        return cgpt_fail(CGPT_ERR_INVALID, who + ": the vocabulary must hold K + num_eos columns, K = max(2, 1 + num_eos) * num_beams = " +
                                               std::to_string(K) + ", and at most " + std::to_string(BEAM_MAX_VOCAB));
    if (h->early_stop) return cgpt_fail(CGPT_ERR_STATE, who + ": early stop is set on the handle (beam search runs every step)");
    if (h->stop.n > 0) return cgpt_fail(CGPT_ERR_STATE, who + ": stop sequences are set on the handle (beam search finishes on EOS ids only)");
    const int rows = B * k;
    if (rows > h->bm_rows || (int64_t)rows * num_new > h->bm_elems)
        return cgpt_fail(CGPT_ERR_STATE, who + ": the beam state is not reserved for " + std::to_string(B) + " images x " + std::to_string(k) +
                                             " beams x " + std::to_string(num_new) + " tokens (cgpt_llm_beam_reserve)");
    CGCHK(ready(h, who.c_str()));
    HIPCHK(hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    BeamSelectArgs a{};
    a.vocab = V; a.k = k; a.keep = K; a.n = num_new; a.pad = pad_id;
    a.eos.n = num_eos;
    for (int e = 0; e < num_eos; ++e) a.eos.id[e] = eos_ids_host[e];
    a.next_tok = h->tok;
    a.parents = h->bm_parents;
    const int64_t ld_out = (int64_t)num_new * V;
    h->last_on = 0;
    h->off_steps = num_new - 1;
    for (int i = 0; i < num_new; ++i) {
        if (i == 0 && step_logits_out_dev) HIPCHK(launch_llm_beam_spread(first_logits_dev, V, step_logits_out_dev, ld_out, V, rows, k, st));
        if (step_logits_out_dev) { a.src = step_logits_out_dev + (int64_t)i * V; a.lds = ld_out; a.shared = 0; }
        else if (i == 0) { a.src = first_logits_dev; a.lds = V; a.shared = 1; }
        else { a.src = h->logits; a.lds = V; a.shared = 0; }
        a.step = i;
        a.first = i == 0 ? 1 : 0;
        a.mask_eos = (i < min_new && num_eos > 0) ? 1 : 0;
        a.divisor = (float)pow((double)(i + 1), (double)length_penalty);
        a.in = h->bm[i & 1];
        a.out = h->bm[(i + 1) & 1];
        const bool last = i + 1 == num_new;
        a.tokens_out = last ? (long long*)tokens_out_dev : nullptr;
        a.scores_out = last ? scores_out_dev : nullptr;
        a.trace = trace_out_dev ? trace_out_dev + (int64_t)i * B * (5 * k + 1) : nullptr;
        HIPCHK(launch_llm_beam_select(a, B, st));
        if (last) break;
        float* next = step_logits_out_dev ? step_logits_out_dev + (int64_t)(i + 1) * V : h->logits;
        const BeamStep bs{prompt_k_ptrs_host, prompt_v_ptrs_host, prompt_stride, a.out.anc, num_new, k, prompt_len, i};
        CGCHK(run_step(h, nullptr, h->tok, rows, prompt_len + i, nullptr, 0, beam_k_ptrs_host, beam_v_ptrs_host, beam_stride, next,
                              step_logits_out_dev ? ld_out : (int64_t)V, st, &bs));
    }
    return CGPT_OK;
}

cgpt_status cgpt_llm_set_trie(cgpt_llm_handle h, const int32_t* child_begin, const int32_t* child_tok, const int32_t* child_node,
                              const int32_t* leaf_class, int32_t nodes, int32_t edges) {
    const std::string who = "cgpt_llm_set_trie";
    if (!h) return cgpt_fail(CGPT_ERR_INVALID, who + ": null handle");
    if (nodes == 0) {                                      // cleared; the old tables stay allocated for the graphs that hold them
        h->t_begin = h->t_tok = h->t_node = h->t_leaf = nullptr;
        h->t_nodes = h->t_depth = 0;
        return CGPT_OK;
    }
    int32_t depth = 0;                                     // the tables are checked first: it takes no device to refuse them
    CGCHK(cgpt_llm_trie_check(child_begin, child_tok, child_node, leaf_class, nodes, edges, h->cfg.vocab, &depth));
    HIPCHK(hipSetDevice(h->cfg.device));
    if (!h->trie_node) CGCHK(dev_zalloc(h, (size_t)h->cfg.max_batch * sizeof(int), (void**)&h->trie_node));
    int* t = nullptr;                                      // [nodes + 1 | edges | edges | nodes]
    const size_t n1 = (size_t)nodes + 1, ne = (size_t)edges;
    CGCHK(dev_zalloc(h, (n1 + 2 * ne + (size_t)nodes) * sizeof(int), (void**)&t));
    HIPCHK(hipMemcpy(t, child_begin, n1 * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t + n1, child_tok, ne * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t + n1 + ne, child_node, ne * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t + n1 + 2 * ne, leaf_class, (size_t)nodes * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
    h->t_begin = t; h->t_tok = t + n1; h->t_node = t + n1 + ne; h->t_leaf = t + n1 + 2 * ne;   // complete or not at all
    h->t_nodes = nodes;
    h->t_depth = depth;
    return CGPT_OK;
}

cgpt_status cgpt_llm_set_early_stop(cgpt_llm_handle h, int32_t on) {
    if (!h) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_set_early_stop: null handle");
    if (on != 0 && on != 1) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_set_early_stop: the value must be 0 or 1");
    h->early_stop = on;
    return CGPT_OK;
}

cgpt_status cgpt_llm_set_stop_sequences(cgpt_llm_handle h, const int64_t* ids_host, const int32_t* lens_host, int32_t n) {
    const std::string who = "cgpt_llm_set_stop_sequences";            // the arrays are checked first: it takes no device to refuse them
    if (n < 0 || n > MAX_STOP) return cgpt_fail(CGPT_ERR_INVALID, who + ": " + std::to_string(n) + " sequences (0.." + std::to_string(MAX_STOP) + ")");
    if (n > 0 && (!ids_host || !lens_host)) return cgpt_fail(CGPT_ERR_INVALID, who + ": null ids_host / lens_host with n > 0");
    StopSeqs t{};
    int64_t at = 0;
    for (int q = 0; q < n; ++q) {
        const int len = lens_host[q];
        if (len < 1 || len > MAX_STOP_LEN)
            return cgpt_fail(CGPT_ERR_INVALID, who + ": sequence " + std::to_string(q) + " has " + std::to_string(len) + " tokens (1.." +
                                                   std::to_string(MAX_STOP_LEN) + ")");
        for (int j = 0; j < len; ++j) {
            if (ids_host[at + j] < 0)
                return cgpt_fail(CGPT_ERR_INVALID, who + ": sequence " + std::to_string(q) + " holds a negative token id");
            t.id[q][j] = ids_host[at + j];
        }
        t.len[q] = len;
        at += len;
    }
    t.n = n;
    if (!h) return cgpt_fail(CGPT_ERR_INVALID, who + ": null handle");
    h->stop = t;                                           // complete or not at all: a refused call leaves the handle as it was
    return CGPT_OK;
}

cgpt_status cgpt_llm_live_steps(cgpt_llm_handle h, int32_t* out_host, void* stream) {
    if (!h || !out_host) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_live_steps: null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    int v = h->off_steps;
    if (h->last_on) HIPCHK(hipMemcpy(&v, h->live_steps, sizeof(int), hipMemcpyDeviceToHost));
    *out_host = v;
    return CGPT_OK;
}

// Grows the prefill workspace to `rows` token rows (a multiple of 256); `who` names the entry in messages.
static cgpt_status grow_workspace(cgpt_llm_handle h, int64_t rows, const std::string& who) {
    if (rows <= h->p_rows) return CGPT_OK;                 // grows only; a second call with the same sizes does nothing
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t H = h->cfg.hidden, F = h->cfg.mlp, hs = sizeof(half_t);
    const size_t cols[7] = {H, H, (size_t)qkv_width(h->cfg), H, H, 2 * F, F};
    Staging stage;                                         // the larger workspace takes the old one's place only when it is complete
    half_t* fresh[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < 7; ++i) stage.add(&fresh[i], (size_t)rows * cols[i] * hs);
    // activations-int8 handles: codes, row scales and outlier lists for the same rows
    signed char* a8 = nullptr;
    float* sa = nullptr;
    uint32_t* lists = nullptr;
    if (h->cfg.act_format) {
        stage.add(&a8, (size_t)rows * std::max(H, F));
        stage.add(&sa, (size_t)rows * sizeof(float));
        stage.add(&lists, (size_t)rows * (size_t)(h->cfg.outlier_cap + 1) * sizeof(uint32_t));
    }
    CGCHK(stage.commit(h, who));
    half_t** bufs[7] = {&h->p_h, &h->p_xn, &h->p_qkv, &h->p_attn, &h->p_proj, &h->p_gu, &h->p_act};
    for (int i = 0; i < 7; ++i) *bufs[i] = fresh[i];
    if (h->cfg.act_format) { h->p_a8 = a8; h->p_sa = sa; h->p_lists = lists; }
    h->p_rows = rows;
    return CGPT_OK;
}

cgpt_status cgpt_llm_prefill_reserve(cgpt_llm_handle h, int32_t max_rows, int32_t max_prompt_len) {
    if (!h) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_prefill_reserve: null handle");
    if (max_rows < 1 || max_rows > h->cfg.max_batch || max_prompt_len < 1 || max_prompt_len > h->cfg.max_len)
        return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_prefill_reserve: rows outside 1..max_batch or prompt length outside 1..max_len");
    return grow_workspace(h, ((int64_t)max_rows * max_prompt_len + 255) / 256 * 256, "cgpt_llm_prefill_reserve");
}

static cgpt_status llm_prefill_entry(const char* who_c, cgpt_llm_handle h, const void* embeds_dev, int32_t B, int32_t L,
                                     const int32_t* starts_dev, void* const* k_ptrs_host, void* const* v_ptrs_host,
                                     int64_t kv_len_stride, float* logits_dev, void* stream) {
    const std::string who(who_c);
    if (!h || !embeds_dev || !logits_dev) return cgpt_fail(CGPT_ERR_INVALID, who + ": null argument");
    if (L < 1) return cgpt_fail(CGPT_ERR_INVALID, who + ": prompt length must be at least 1");
    CGCHK(check_cache(h, who_c, B, L - 1, k_ptrs_host, v_ptrs_host, kv_len_stride));
    CGCHK(ready(h, who_c));
    if ((int64_t)B * L > h->p_rows)
        return cgpt_fail(CGPT_ERR_STATE, who + ": " + std::to_string((int64_t)B * L) + " token rows, the reserved workspace holds " +
                                             std::to_string(h->p_rows) + " (call cgpt_llm_prefill_reserve outside any capture first)");
    HIPCHK(hipSetDevice(h->cfg.device));
    return run_prefill(h, (const half_t*)embeds_dev, B, L, starts_dev, k_ptrs_host, v_ptrs_host, kv_len_stride, logits_dev,
                       (hipStream_t)stream);
}

cgpt_status cgpt_llm_prefill(cgpt_llm_handle h, const void* embeds_dev, int32_t B, int32_t L, void* const* k_ptrs_host,
                             void* const* v_ptrs_host, int64_t kv_len_stride, float* logits_dev, void* stream) {
    return llm_prefill_entry("cgpt_llm_prefill", h, embeds_dev, B, L, nullptr, k_ptrs_host, v_ptrs_host, kv_len_stride, logits_dev, stream);
}

cgpt_status cgpt_llm_prefill_ragged(cgpt_llm_handle h, const void* embeds_dev, int32_t B, int32_t L, const int32_t* starts_dev,
                                    void* const* k_ptrs_host, void* const* v_ptrs_host, int64_t kv_len_stride, float* logits_dev,
                                    void* stream) {
    if (!starts_dev) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_prefill_ragged: null starts_dev");
    return llm_prefill_entry("cgpt_llm_prefill_ragged", h, embeds_dev, B, L, starts_dev, k_ptrs_host, v_ptrs_host, kv_len_stride,
                             logits_dev, stream);
}

cgpt_status cgpt_llm_prefill_from(cgpt_llm_handle h, const void* embeds_dev, int32_t B, int32_t pos0, int32_t Ln, const int32_t* starts_dev,
                                  void* const* k_ptrs_host, void* const* v_ptrs_host, int64_t kv_len_stride, float* logits_dev,
                                  void* stream) {
    const std::string who("cgpt_llm_prefill_from");
    // what can be judged without the handle comes first, so that each refusal names its own argument
    if (Ln < 1 || pos0 < 0) return cgpt_fail(CGPT_ERR_INVALID, who + ": Ln must be at least 1 and pos0 at least 0");
    if ((int64_t)pos0 + Ln > kv_len_stride) return cgpt_fail(CGPT_ERR_INVALID, who + ": pos0 + Ln exceeds kv_len_stride");
    if (!h || !embeds_dev || !logits_dev) return cgpt_fail(CGPT_ERR_INVALID, who + ": null argument");
    if ((int64_t)pos0 + Ln > h->cfg.max_len) return cgpt_fail(CGPT_ERR_INVALID, who + ": pos0 + Ln exceeds max_len");
    CGCHK(check_cache(h, who.c_str(), B, pos0 + Ln - 1, k_ptrs_host, v_ptrs_host, kv_len_stride));
    CGCHK(ready(h, who.c_str()));
    if ((int64_t)B * Ln > h->p_rows)
        return cgpt_fail(CGPT_ERR_STATE, who + ": " + std::to_string((int64_t)B * Ln) + " token rows, the reserved workspace holds " +
                                             std::to_string(h->p_rows) + " (call cgpt_llm_prefill_reserve outside any capture first)");
    HIPCHK(hipSetDevice(h->cfg.device));
    return run_prefill(h, (const half_t*)embeds_dev, B, Ln, starts_dev, k_ptrs_host, v_ptrs_host, kv_len_stride, logits_dev,
                       (hipStream_t)stream, pos0);
}

cgpt_status cgpt_llm_kv_broadcast(cgpt_llm_handle h, void* const* src_k_ptrs_host, void* const* src_v_ptrs_host, int64_t src_len_stride,
                                  int32_t P, int32_t B, const int32_t* starts_dev, void* const* dst_k_ptrs_host,
                                  void* const* dst_v_ptrs_host, int64_t dst_len_stride, void* stream) {
    const std::string who("cgpt_llm_kv_broadcast");
    if (P < 1) return cgpt_fail(CGPT_ERR_INVALID, who + ": P must be at least 1");
    if (P > src_len_stride) return cgpt_fail(CGPT_ERR_INVALID, who + ": P exceeds src_len_stride");
    if (P > dst_len_stride) return cgpt_fail(CGPT_ERR_INVALID, who + ": P exceeds dst_len_stride");
    if (!h) return cgpt_fail(CGPT_ERR_INVALID, who + ": null handle");
    if (P > h->cfg.max_len) return cgpt_fail(CGPT_ERR_INVALID, who + ": P exceeds max_len");
    CGCHK(check_cache(h, who.c_str(), 1, P - 1, src_k_ptrs_host, src_v_ptrs_host, src_len_stride));
    CGCHK(check_cache(h, who.c_str(), B, P - 1, dst_k_ptrs_host, dst_v_ptrs_host, dst_len_stride));
    HIPCHK(hipSetDevice(h->cfg.device));
    for (int l = 0; l < h->cfg.layers; ++l)
        HIPCHK(launch_kv_broadcast((const half_t*)src_k_ptrs_host[l], (const half_t*)src_v_ptrs_host[l], src_len_stride, P, B, h->cfg.kv_heads,
                                   starts_dev, (half_t*)dst_k_ptrs_host[l], (half_t*)dst_v_ptrs_host[l], dst_len_stride, (hipStream_t)stream));
    return CGPT_OK;
}

cgpt_status cgpt_llm_score_reserve(cgpt_llm_handle h, int32_t max_rows, int32_t max_tail_rows) {
    if (!h) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_score_reserve: null handle");
    if (max_rows < 1 || max_rows > h->cfg.max_batch || max_tail_rows < 1 || max_tail_rows > SCORE_MAX_TAIL)
        return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_score_reserve: rows outside 1..max_batch or tail rows outside 1.." +
                                               std::to_string(SCORE_MAX_TAIL));
    const int64_t rows = ((int64_t)max_rows * max_tail_rows + 255) / 256 * 256;
    CGCHK(grow_workspace(h, rows, "cgpt_llm_score_reserve"));      // the tail rows run on the prefill workspace
    HIPCHK(hipSetDevice(h->cfg.device));
    const int64_t lrows = std::min(rows, SCORE_LOGIT_ROWS), nce = (int64_t)max_rows * (max_tail_rows + SCORE_MAX_CANDS);
    Staging stage;                                         // as the prefill workspace: beside the buffers in use
    half_t* logits = nullptr;
    float* ce = nullptr;
    if (lrows > h->s_rows) stage.add(&logits, (size_t)lrows * h->cfg.vocab * sizeof(half_t));
    if (nce > h->s_ce) stage.add(&ce, (size_t)nce * sizeof(float));
    CGCHK(stage.commit(h, "cgpt_llm_score_reserve"));
    if (logits) { h->s_logits = logits; h->s_rows = lrows; }
    if (ce) { h->s_ce_buf = ce; h->s_ce = nce; }
    return CGPT_OK;
}

// The plain and the _ragged entry share one body: `who_c` names the entry in messages, starts_dev == null is the plain one.
static cgpt_status llm_score_entry(const char* who_c, cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t prompt_len,
                                   const int32_t* starts_dev, const int64_t* cand_tokens_dev, const int32_t* cand_lens_dev,
                                   const int32_t* cand_lens_host, int32_t C, int32_t Tmax, float label_smoothing, void* const* k_ptrs_host,
                                   void* const* v_ptrs_host, int64_t kv_len_stride, float* out_dev, void* stream) {
    const std::string who(who_c);
    if (!h || !first_logits_dev || !cand_tokens_dev || !cand_lens_host || !out_dev) return cgpt_fail(CGPT_ERR_INVALID, who + ": null argument");
    if (C < 1 || C > SCORE_MAX_CANDS || Tmax < 1)
        return cgpt_fail(CGPT_ERR_INVALID, who + ": candidates outside 1.." + std::to_string(SCORE_MAX_CANDS) + " or Tmax < 1");
    if (!(label_smoothing >= 0.0f && label_smoothing < 1.0f)) return cgpt_fail(CGPT_ERR_INVALID, who + ": label_smoothing outside [0, 1)");
    ScoreCands t{};
    t.n = C;
    t.tmax = Tmax;
    for (int c = 0; c < C; ++c) {
        if (cand_lens_host[c] < 1 || cand_lens_host[c] > Tmax)
            return cgpt_fail(CGPT_ERR_INVALID, who + ": candidate " + std::to_string(c) + " has a length outside 1..Tmax");
        t.off[c + 1] = t.off[c] + cand_lens_host[c] - 1;
        if (t.off[c + 1] > SCORE_MAX_TAIL)
            return cgpt_fail(CGPT_ERR_INVALID, who + ": more than " + std::to_string(SCORE_MAX_TAIL) + " tail rows (sum of lengths - 1) per prompt row");
    }
    if (prompt_len < 1 || (int64_t)prompt_len + Tmax - 1 > h->cfg.max_len)
        return cgpt_fail(CGPT_ERR_INVALID, who + ": prompt_len < 1 or prompt_len + Tmax - 1 > max_len (the rotary table)");
    CGCHK(check_cache(h, who_c, B, prompt_len - 1, k_ptrs_host, v_ptrs_host, kv_len_stride));
    CGCHK(ready(h, who_c));
    const int64_t R = (int64_t)B * t.off[C];
    if (R > h->p_rows || (R > 0 && h->s_rows < 1) || (int64_t)B * (t.off[C] + C) > h->s_ce)
        return cgpt_fail(CGPT_ERR_STATE, who + ": " + std::to_string(R) + " tail rows of " + std::to_string(C) +
                                             " candidates exceed the reserved workspace (call cgpt_llm_score_reserve outside any capture first)");
    HIPCHK(hipSetDevice(h->cfg.device));
    return run_score(h, first_logits_dev, B, prompt_len, starts_dev, (const long long*)cand_tokens_dev, cand_lens_dev, t, label_smoothing,
                     k_ptrs_host, v_ptrs_host, kv_len_stride, out_dev, (hipStream_t)stream);
}

cgpt_status cgpt_llm_score(cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t prompt_len, const int64_t* cand_tokens_dev,
                           const int32_t* cand_lens_host, int32_t C, int32_t Tmax, float label_smoothing, void* const* k_ptrs_host,
                           void* const* v_ptrs_host, int64_t kv_len_stride, float* out_dev, void* stream) {
    return llm_score_entry("cgpt_llm_score", h, first_logits_dev, B, prompt_len, nullptr, cand_tokens_dev, nullptr, cand_lens_host, C, Tmax,
                           label_smoothing, k_ptrs_host, v_ptrs_host, kv_len_stride, out_dev, stream);
}

cgpt_status cgpt_llm_score_ragged(cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t prompt_len,
                                  const int32_t* starts_dev, const int64_t* cand_tokens_dev, const int32_t* cand_lens_dev,
                                  const int32_t* cand_lens_host, int32_t C, int32_t Tmax, float label_smoothing, void* const* k_ptrs_host,
                                  void* const* v_ptrs_host, int64_t kv_len_stride, float* out_dev, void* stream) {
    if (!starts_dev || !cand_lens_dev) return cgpt_fail(CGPT_ERR_INVALID, "cgpt_llm_score_ragged: null starts_dev or cand_lens_dev");
    return llm_score_entry("cgpt_llm_score_ragged", h, first_logits_dev, B, prompt_len, starts_dev, cand_tokens_dev, cand_lens_dev,
                           cand_lens_host, C, Tmax, label_smoothing, k_ptrs_host, v_ptrs_host, kv_len_stride, out_dev, stream);
}

}  // extern "C"
