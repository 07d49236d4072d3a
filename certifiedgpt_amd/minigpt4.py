"""MiniGPT4Classifier -- full MiniGPT-4 (`generate`) as the base classifier of `Smooth` (BASELINE configs[2]).

Mirrors `MiniGPTBase.generate` (graphs/models/minigpt4/models/minigpt_base.py:374-448) and `get_context_emb` (:75-89):

    encode_img(images)            -> libcgpt.so  (cgpt_encode_img / cgpt_encode_img_noisy: HIP noise + ViT-G + Q-Former +
                                                  llama_proj straight into the buffer the LLM reads; minigpt4.py:121-149)
    prompt splice + left padding  -> this file, PyTorch-ROCm tensors (minigpt_base.py:401-416)
    llama_model.generate(...)     -> Hugging Face `generate` on PyTorch-ROCm, greedy, <= max_new_tokens (:418-431);
                                     the LLM is a frozen decoder loaded BY LOCAL PATH by the caller (base_model.py:181-247) --
                                     nothing is downloaded here
    decode + clean-up             -> this file (:441-448)
    answer -> class               -> agents/label_adapter.AnswerLabelMap (the "decoder-to-label" mapping, README.md:28-29)
    argmax / vote histogram       -> libcgpt.so (cgpt_vote: wavefront arg-max + 64-bit atomics)

The LLM decode is memory-bound PyTorch work and stays outside the MFMA-roofline claim; what this class adds
for the Monte-Carlo loop is that the N noisy copies of one image share ONE text prompt: the prompt segments are tokenised and
embedded once per call and broadcast, and because every row then has the same length there is no padding and the attention
mask is all ones (identical to what the reference's left-padding produces for equal lengths).

`Smooth` sees the engine interface (`sample_counts`), so noise generation stays fused into the patch-embed operand.

What the LLaMA path is specified to compute (stop rule, sampling law, int8 laws, the grouped-query twin, padding) is stated in
llm_laws.py; the ctypes binding of the native engine (`_HipDecoder`, `_LinearRoute`) is llm_engine.py.  Their names stay importable
from this module, and the classifier resolves `_HipDecoder`, `_LinearRoute`, `vote` and `vote_labels` through this module's globals.
"""
import torch

from .classifier import vote, vote_labels
from .llm_engine import _HipDecoder, _LinearRoute, _rope_theta, hip_decode_unsupported    # noqa: F401  (resolved through this module's globals)
from .llm_laws import (GQA_RATIOS, LAYER_LINEARS, MAX_STOP_LEN, MAX_STOP_SEQS, PHILOX_WORD_SAMPLE, SAMPLE_FIELDS,    # noqa: F401
                       SAMPLE_HF_DEFAULTS, _ActInt8Linear, _as_rows, _philox4x32_10, act_int8_twin, apply_stop_sequences,
                       check_sample_settings, check_stop_words_ids, dequantize_rows_int8, expand_kv_state_dict, fp16_ulp,
                       greedy_decode_parity, int8_state_dict, left_pad_embeds, llm_int8_linear, pack_row_candidates,
                       quantize_act_rows_int8, quantize_rows_int8, sample_token_law, sample_uniform, shared_prefix_len,
                       stop_finish_columns, stop_sequences_criteria)
from .llm_laws import (TRIE_MAX_DEPTH, TRIE_MAX_NODES, AnswerTrie, allowed_tokens_fn, build_answer_trie,    # noqa: F401
                       constrained_decode_law, constrained_select_law, trie_walk)
from .llm_laws import (BEAM_FIELDS, BEAM_HF_DEFAULTS, BEAM_MAX, BEAM_MIN, BEAM_NEG, beam_decode_law, beam_init_state, beam_keep,    # noqa: F401
                       beam_length_divisor, beam_step_law, check_beam_settings)

IMAGE_PLACEHOLDER = "<ImageHere>"


def prepare_texts(questions):
    """`MiniGPT4EvalAgent.prepare_texts` with CONV_VISION_minigptv2 (agents/minigpt4_eval_agent.py:265-271; conversation.py:130-137:
    system "", roles ("<s>[INST] ", " [/INST]"), sep ""): one user turn, assistant turn left open."""
    return ["<s>[INST] " + q + " [/INST]" for q in questions]


def clean_answer(text: str) -> str:
    """Post-processing of a decoded sequence, minigpt_base.py:444-447."""
    text = text.split("</s>")[0]
    text = text.replace("<s>", "")
    return text.split(r"[/INST]")[-1].strip()


class WordHashTokenizer:
    """Stand-in for LlamaTokenizer where no tokenizer model file exists (the container has no Vicuna directory and nothing is
    ever downloaded): words map to ids by a stable hash into [3, vocab_size), id k decodes to the word "w<k>" (token-id strings
    as answers).  It offers exactly the tokenizer surface `MiniGPTBase` uses: `__call__(text, return_tensors="pt",
    add_special_tokens=...)` -> object with `.input_ids` / `.to(device)`, and `decode(ids, skip_special_tokens=True)`.
    Used by the tests and by `bench.py --workload minigpt4` (synthetic decoder of the Vicuna-7B architecture)."""
    pad_token_id, bos_token_id, eos_token_id = 0, 1, 2

    class _Encoding:
        def __init__(self, ids):
            self.input_ids = ids
            self.attention_mask = torch.ones_like(ids)

        def to(self, device):
            self.input_ids = self.input_ids.to(device)
            self.attention_mask = self.attention_mask.to(device)
            return self

    def __init__(self, vocab_size=96):
        self.vocab_size = int(vocab_size)

    def _word_id(self, w):
        h = 0
        for ch in w:
            h = (h * 131 + ord(ch)) % 1000003
        return 3 + h % (self.vocab_size - 3)

    def __call__(self, text, return_tensors="pt", add_special_tokens=True, **_):
        ids = [self._word_id(w) for w in text.split()]
        if add_special_tokens:
            ids = [self.bos_token_id] + ids
        return self._Encoding(torch.tensor([ids], dtype=torch.long))

    def decode(self, ids, skip_special_tokens=True):
        out = []
        for t in ids.tolist():
            if t in (self.pad_token_id, self.bos_token_id):
                if not skip_special_tokens:
                    out.append("<s>" if t == self.bos_token_id else "<pad>")
            elif t == self.eos_token_id:
                out.append("</s>")                       # the reference splits on the literal stop sign, minigpt_base.py:445
            else:
                out.append(f"w{t}")
        return " ".join(out)


class _Prefix:
    """shared_prefix: the P positions every row of a call shares -- their token `ids` (a tuple, the LRU key) and their one-row caches,
    per layer `k` / `v` [1, kv_heads, P, 128]."""

    def __init__(self, ids, k, v):
        self.ids, self.k, self.v = ids, list(k), list(v)

    @property
    def P(self):
        return len(self.ids)

    def clone(self):
        return _Prefix(self.ids, [t.clone() for t in self.k], [t.clone() for t in self.v])

    def hold(self, other):
        """Take `other`'s caches (same P) in place -- the static copy a captured graph reads; nothing is copied when it holds them."""
        if self.ids != other.ids:
            for dst, src in zip(self.k + self.v, other.k + other.v):
                dst.copy_(src)
            self.ids = other.ids


class MiniGPT4Classifier:
    """:param encoder: a `HipClassifier(mode="encode_img")` (or any object with `encode_img(images) -> (emb, atts)` and
               `encode_img_noisy(x, first_sample, num, sigma, seed) -> emb`, emb = [B, queries, llm_hidden])
       :param llama_model: a causal LM with `.generate(inputs_embeds=..., attention_mask=...)` and an input embedding table
               (`get_input_embeddings()`), e.g. `LlamaForCausalLM.from_pretrained(<local path>, torch_dtype=torch.float16)`
       :param llama_tokenizer: its tokenizer (`__call__(text, return_tensors="pt", add_special_tokens=...)`, `decode`)
       :param prompt: the text every noisy copy is asked, containing one `<ImageHere>`
       :param label_map: `AnswerLabelMap` -- frozen when torch.distributed is initialised (see label_adapter.py)
       :param ragged: "hf" (default) | "hip" -- who decodes a call whose rows carry DIFFERENT texts (left padding + mask); see __init__
       :param prompt_bucket: None | int >= 1 (with ragged="hip") -- padded prompt lengths are rounded up to a multiple of it
       :param weights: "fp16" (default) | "int8" (with decode="hip" and prefill="hip") -- how the native engine holds the layer linears
       :param activations: "fp16" (default) | "int8" (with decode="hip", prefill="hip" and weights="int8") -- the LLM.int8() forward
       :param int8_threshold: outlier threshold of activations="int8" (6.0: HF's llm_int8_threshold default; <= 0: no outlier split)
       :param outlier_cap: outliers kept per activation row under activations="int8" (1..1024; more in a row is a RuntimeError)
       :param early_stop: False (default) | True (with decode="hip") -- the native token steps do no work once every row has its EOS
       :param grouped_kv: False (default) | True (with decode="hip") -- the native engine takes a grouped-query decoder; see __init__
       :param sample: "hf" (default) | "hip" (with decode="hip") -- who decodes a call with do_sample / a repetition penalty; see __init__
       :param shared_prefix: False (default) | True (with decode="hip" and prefill="hip") -- the positions in front of the image tokens
               are prefilled once per template instead of once per row; same tokens; see __init__
       :param stop_words_ids: None (default) | up to 8 token-id sequences of 1..8 tokens -- a row finishes when its answer ends in one
       :param stop_text: None (default) | str -- every decoded answer is cut at its first occurrence (the reference's "###")
       :param end_sym: text appended to every candidate answer of `multi_select` ("\n": the reference's default; its VQA configs: "###")
       :param label_smoothing: of the answer loss (0.1: modeling_llama.py:105)
       :param score: "hf" (default) | "hip" -- who computes the answer losses of `multi_select`; see __init__
       :param classify: "generate" (default) | "multi_select" | "constrained" -- what the base classifier of `Smooth` does with a
               batch; see __init__
       :param constrain: "hf" (default) | "hip" (with decode="hip") -- who runs the decode of classify="constrained"; see __init__
       :param beams: "hf" (default) | "hip" (with decode="hip" and prefill="hip") -- who decodes a call with num_beams > 1; see __init__
       :param candidates: the answers `classify="multi_select"` ranks and `classify="constrained"` decodes among (default:
               `label_map.answers`, in class-id order)

    `prompt` is a plain attribute: assigning a new prompt between two images (`clf.prompt = ...`) is the supported way to ask a
    per-image question (VQA: one question per image).  Under decode="graph" / "hip" every new prompt LENGTH captures a graph of its
    own; with ragged="hip", prompt_bucket=k all prompts whose length rounds up to the same multiple of k replay one graph.
    """

    noise_laws = ("gaussian", "uniform")       # passed through to encoder.encode_img_noisy

    def __init__(self, encoder, llama_model, llama_tokenizer, prompt, label_map, max_new_tokens=20, max_batch=None,
                 generate_kwargs=None, decode="hf", prefill_linear="torch", prefill="model", ragged="hf", prompt_bucket=None,
                 weights="fp16", end_sym="\n", label_smoothing=0.1, score="hf", classify="generate", candidates=None,
                 early_stop=False, grouped_kv=False, activations="fp16", int8_threshold=6.0, outlier_cap=64, stop_words_ids=None,
                 stop_text=None, sample="hf", shared_prefix=False, constrain="hf", beams="hf"):
        self.encoder = encoder
        self.llama_model = llama_model
        self.llama_tokenizer = llama_tokenizer
        self.prompt = prompt
        self.label_map = label_map
        self.num_classes = label_map.num_classes
        self.max_new_tokens = int(max_new_tokens)
        self.max_batch = int(max_batch or getattr(encoder, "max_batch", 16))
        # the reference's fixed generation arguments, minigpt_base.py:379-388,418-431
        self.generate_kwargs = dict(num_beams=1, min_length=1, top_p=0.9, repetition_penalty=1, length_penalty=1,
                                    temperature=1, do_sample=False)
        self.generate_kwargs.update(generate_kwargs or {})
        self.last_answers = []
        # decode = "hf": `llama_model.generate(...)` exactly as the reference calls it (minigpt_base.py:418-431).
        # decode = "graph": the same greedy decode -- the model's own forward for the prefill and for every step, a DynamicCache, EOS
        #   suppressed on the first `min_length` generated tokens (the reference's semantics, see hf_generate_kwargs), pad after EOS -- written as a fixed-length loop without host round trips and
        #   replayed from ONE hipGraph per (batch, prompt length); shared prompts on a HIP device only, everything else takes "hf".
        #   Parity with HF generate (tests/test_gpu_fullsize.py, Vicuna-7B widths, 200 rows x 20 tokens): run eagerly the loop gives HF's
        #   tokens and logits bit for bit; under graph capture other vendor kernels get picked, so logits move by fp16 rounding and a row
        #   may leave HF's trajectory at a step where HF's own top-2 margin is within that noise (near-tied logits of a random-init
        #   decoder) -- every decisive row gives the identical answer.
        # prefill_linear = "cgpt" (with decode = "graph"): the decoder's bias-free fp16 linears run the prefill's rows through this
        #   library's GEMM (see _LinearRoute); same arithmetic contract (fp16 operands, fp32 accumulation, fp16 result), other rounding
        #   order than the vendor library: first-token logits within 4 fp16 ulp, same decisive-row rule.
        # decode = "hip": the prefill as under "graph" (routed or not), then every token step in this library's own kernels
        #   (csrc/llm_step.hip, csrc/llm_gemm.hip: RMSNorm, decode-shape GEMMs, rotary + K/V append + one-query attention, token select) on the K/V the
        #   prefill wrote, captured into the same kind of graph.  Opt-in; a decoder the kernels do not support is a ValueError here,
        #   never another engine.  Parity: tests/test_gpu_llm_decode.py (teacher-forced logit error against HF's own fp16 error).
        # prefill = "hip" (with decode = "hip" only; anything else is a ValueError, never silently another engine): the prefill too
        #   runs in this library (csrc/llm_prefill.hip + the large-shape GEMM): no HF forward, no DynamicCache; `prefill_linear` is
        #   ignored and no linear is routed.  prefill = "model" (default): the model's own forward, as described above.
        #   Parity: tests/test_gpu_llm_prefill.py (logits and every cache row against HF's own fp16 error).
        # ragged = "hip" (with decode = "hip" AND prefill = "hip" only; anything else is a ValueError): rows with different texts are
        #   left-padded as the reference pads them (minigpt_base.py:407-416) and run through the native engine's _ragged entries with
        #   a per-row start offset held in device memory (include/cgpt.h), from one captured graph per (batch, padded length): no HF
        #   call.  A padded row's tokens are bit for bit those of the row run alone without padding (tests/test_gpu_llm_ragged.py).
        #   ragged = "hf" (default): such calls take HF `generate` with the attention mask, as before.
        # prompt_bucket = k (with ragged = "hip" only): padded lengths are rounded up to a multiple of k, and a SHARED prompt is padded
        #   the same way (one common start), so prompts of different lengths replay one graph per bucket.  None: shared prompts take
        #   the unpadded path, unchanged.
        # weights = "int8" (with decode = "hip" AND prefill = "hip" only; anything else is a ValueError): the native engine holds the
        #   seven linears of every layer as row-wise absmax int8 with one fp16 scale per row (`quantize_rows_int8`; the weight law of the
        #   reference's `low_resource: true` -> load_in_8bit), quantised on the device at load; activations stay fp16.  Half the
        #   engine's weight bytes (decode_stats["weight_bytes"]).  Every token is, bit for bit, what the fp16 native engine gives on
        #   the model whose layer linears are `int8_state_dict(llama_model)` (tests/test_gpu_llm_int8.py).  With the model's own
        #   prefill the prompt would run on W and the steps on W': a mixed model, hence the ValueError.  Works with ragged = "hip" and
        #   prompt_bucket.  weights = "fp16" (default): the engine's own fp16 copies, as before.
        # activations = "int8" (with decode = "hip", prefill = "hip" AND weights = "int8"; anything else is a ValueError naming what is
        #   missing): the layer linears run the LLM.int8() forward the reference's `low_resource: true` configs select -- row-wise int8
        #   activations against the int8 weights on the int8 MFMA, int32 accumulation, and every row's features of magnitude >=
        #   int8_threshold multiplied in fp32 against W' instead (`llm_int8_linear`).  The outlier set is per ROW, not
        #   per batch as in bitsandbytes: a row's result depends on that row alone.  The oracle is `act_int8_twin(llama_model)`
        #   (tests/test_gpu_llm_act_int8.py); parity with bitsandbytes itself is not pinned.  No fp16 scratch: weight_bytes drops by
        #   it.  A row with more than outlier_cap outliers is a RuntimeError from `last_act_stats()`, which generate and the native
        #   scoring call where they read their results.  Works with ragged = "hip", prompt_bucket, early_stop, grouped_kv and
        #   score = "hip".  activations = "fp16" (default): as before.
        # early_stop = True (with decode = "hip" only; anything else is a ValueError): once every row of a batch has produced an EOS,
        #   the remaining token steps of the native greedy loop do no work (cgpt_llm_set_early_stop, DESIGN.md 4.4.5: a flag on the
        #   device that every step kernel reads first; the captured graph keeps all its launches and one graph serves every finishing
        #   step).  Tokens and answers are bit for bit those with it off; `last_live_steps()` tells how many steps ran.  Works with
        #   either prefill, with ragged = "hip" and with weights = "int8".  early_stop = False (default): every step runs, as before.
        # grouped_kv = True (with decode = "hip" only; anything else is a ValueError): the native engine runs grouped-query attention
        #   (cgpt_llm_config_gqa.grouped_kv): a decoder with fewer K/V heads than query heads -- heads / kv_heads in
        #   {1, 2, 4, 8}: Llama-3-8B's 32 / 8 -- is accepted, every K/V buffer is [rows, kv_heads, positions, 128] (1 / G of the pool),
        #   and the token step reads a K/V head once for the G query heads that share it.  Works with either prefill (HF's cache holds
        #   the un-repeated heads too), ragged = "hip", prompt_bucket, weights = "int8", early_stop and score = "hip".  Every result is
        #   what the engine gives on the multi-head twin `expand_kv_state_dict(llama_model)` (tests/test_gpu_llm_gqa.py).
        #   grouped_kv = False (default): as before, a grouped-query decoder is a ValueError.
        # stop_words_ids = [[ids], ...] (any decode): PER-ROW stop sequences of the greedy decode (the reference's
        #   argument, minigpt_base.py:387-394, whose criterion conversation.py:96-107 fires only when all rows stop at once): a row
        #   finishes at the first generated token that is an EOS id or completes one of the sequences; the finishing tokens stay and
        #   pad ids follow, as after an EOS (`stop_finish_columns` is the rule, and every engine gives `apply_stop_sequences` of its
        #   own decode without them, bit for bit).  decode = "hip": handed to the engine once, here (cgpt_llm_set_stop_sequences: the
        #   select kernel looks back in its own token table), and a finished row counts for early_stop; decode = "graph": the same
        #   rule in tensor ops on the loop's step tokens; decode = "hf" and every HF fallback: a StoppingCriteria that answers per row.
        #   An int entry is a one-token sequence.  None (default): every path is what it was.
        # sample = "hip" (with decode = "hip" only; anything else is a ValueError): a call whose generation arguments differ from the
        #   greedy ones ONLY in do_sample, temperature, top_k, top_p and repetition_penalty -- `Chat.answer`'s do_sample=True,
        #   top_p=0.9, repetition_penalty=1.05, temperature=1.0 with HF's default top_k=50 -- stays on the native engine: the select
        #   kernel is replaced by a sampler (csrc/llm_sample.hip; `sample_token_law` is the law) whose uniform is a
        #   function of (seed, draw id, step) alone.  `sample_counts` / `sample_counts_pair` give row r of sample index i the draw id
        #   i and the call's seed, so a row's answer is a function of (image, seed, sample index) and counts do not depend on the
        #   batch size or on how the range is split; `generate` / `__call__` take ids from a running counter (`reset_draws`).  Works
        #   with either prefill, ragged = "hip", weights / activations = "int8", grouped_kv, early_stop and stop_words_ids; counted in
        #   decode_stats["hip_sampled"].  sample = "hf" (default): such calls take HF `generate` and torch's generator, as before.
        # shared_prefix = True (with decode = "hip" AND prefill = "hip" only; anything else is a ValueError): a prompt is
        #   segs[0] | image tokens | segs[1], and everything in segs[0] -- <s>, the template's opening, "<Img>", a system text --
        #   precedes the image, so under causal attention its hidden states and K/V rows are the same for every row of a call and for
        #   every image asked through the same template.  A native call whose rows share their first segment's TOKENS
        #   (`shared_prefix_len`; a shared prompt always, per-row texts under ragged = "hip" when their first segments agree) prefills
        #   those P positions ONCE, on one row, into a one-row cache kept in an LRU of `max_prefixes` entries keyed by the token ids
        #   (eagerly, outside any capture), and the captured graph copies it into every row (cgpt_llm_kv_broadcast) and prefills only
        #   image tokens + segs[1] on top of it (cgpt_llm_prefill_from).  Tokens, logits and caches are bit for bit
        #   those without the flag (tests/test_gpu_llm_prefix.py): the steps, early_stop, stop sequences and the sampler see a complete
        #   cache.  The suffix is padded so that P + its length is the padded length without the flag: the K/V pool and "one graph
        #   per bucket" stay.  Counted in decode_stats["hip_prefix_prefills"] (misses) / ["hip_prefix_hits"].  The scoring paths keep
        #   their whole-prompt prefill.  shared_prefix = False (default): every path launches what it launched before.
        # stop_text = "###": `_decode_outputs` cuts every decoded text at its first occurrence before `clean_answer`
        #   (`Chat.answer`'s `split('###')[0]`) -- at the text level because "###" tokenises differently after different words.
        # score = "hf" (default): `multi_select` / `answer_losses_from_embeds` run the model's own forward once per candidate over the
        #   concatenated prompt + answer embeds, as the reference does (works on the CPU); counted in decode_stats["hf_score_forwards"].
        # score = "hip" (with decode = "hip" AND prefill = "hip" only; anything else is a ValueError, never another engine): ONE native
        #   prefill of the prompt, then every candidate on its cache (cgpt_llm_score, csrc/llm_score.hip: tail attention over the shared
        #   prompt keys + fused label-smoothed cross-entropy); counted in decode_stats["hip_scores"].  Taken when the call is on the
        #   device, every row shares one text and every row gets the same candidate list (the smoothing case); any other call takes the
        #   "hf" path and is counted in decode_stats["hf_score_fallbacks"] -- the policy ragged = "hf" has for `generate`.  Works with
        #   weights = "int8".  Parity: tests/test_gpu_llm_score.py.
        #   With ragged = "hip" a call whose rows carry different texts or different candidates (`answers[c][b]`, the reference's
        #   `multi_select` interface), or any call under prompt_bucket, stays on the engine too: the prompts are left-padded as for
        #   `generate`, prefilled by cgpt_llm_prefill_ragged and scored by cgpt_llm_score_ragged on a per-row candidate table
        #   (`pack_row_candidates`); counted in decode_stats["hip_ragged_scores"].  A padded row's sums are bit for bit those of the
        #   row scored alone (tests/test_gpu_llm_score_ragged.py); candidate c is divided by (longest prompt + longest answer c - 1),
        #   the reference's right-padded length.  Still the "hf" path, counted as a fallback: off the device, beyond the engine's
        #   limits (rows, 64 candidates, 64 tail rows, max_len), an answer token equal to the pad id.  With ragged = "hf" nothing
        #   changes: per-row calls take the model's forward.
        # classify = "multi_select": `__call__`, `sample_counts` and `sample_counts_pair` score `candidates` (default: the label map's
        #   answers, in class-id order; at least 2, at most num_classes - 1) instead of generating: logits [B, num_classes] hold -loss in
        #   column i for candidate i and -inf in column `other_id`, so every row votes for a known class.  classify = "generate"
        #   (default): as before.
        # classify = "constrained": the greedy decode restricted to `candidates`: at every step the arg-max runs over
        #   the tokens that continue some candidate -- a trie over the tokens of `answer + end_sym` (`_answer_tokens`, the format
        #   `multi_select` scores), HF's `prefix_allowed_tokens_fn`; `constrained_select_law` is the law -- and a row stops when it has
        #   spelled a whole candidate: `depth` = the longest candidate's tokens are generated, whatever the number of candidates, every
        #   row votes for a known class (never `other_id`), and the class id is the trie leaf's.  The prompt is `generate`'s.  The trie
        #   is built once, here (`build_answer_trie`: at most 2**20 nodes and 32 tokens per candidate; no candidate may be a prefix of
        #   another); generation arguments that ask for anything but the plain arg-max are a ValueError here, never another law, and
        #   stop_words_ids / stop_text belong to `generate()`: the constrained call ignores them.
        #   constrain = "hf" (default): `llama_model.generate(..., prefix_allowed_tokens_fn=allowed_tokens_fn(trie))`; works on the
        #   CPU; counted in decode_stats["hf_constrained"].  constrain = "hip" (with decode = "hip"; anything else is a ValueError): the
        #   native loop with the trie select in the arg-max's place (csrc/llm_trie.hip), after either prefill, from the captured graph;
        #   composes with prefill = "hip", ragged = "hip", prompt_bucket, shared_prefix, weights / activations = "int8", grouped_kv and
        #   early_stop (only the select differs); `sample_counts` / `sample_counts_pair` then vote from the device labels
        #   (cgpt_vote_labels) and read nothing back per batch.  Counted in decode_stats["hip_constrained"]; a call the engine cannot
        #   take (off the device, more rows than max_batch, per-row texts without ragged = "hip") takes the "hf" path and is counted in
        #   decode_stats["hf_constrained_fallbacks"].
        # beams = "hip" (with decode = "hip" AND prefill = "hip" only; anything else is a ValueError): a `generate` / `__call__` /
        #   `sample_counts` call under classify = "generate" whose generation arguments differ from the greedy ones ONLY in num_beams
        #   (2..8) and length_penalty -- the first slider of MiniGPT-4's demo -- stays on the native engine (csrc/
        #   llm_beam.hip; `beam_step_law` / `beam_decode_law` are the law, HF 5.x `_beam_search` restated).  The prompt is prefilled
        #   once per IMAGE, not once per beam; the beams' generated positions live in a cache of their own and HF's reorder_cache is an
        #   ancestry table the step attention reads, so no K/V byte moves.  The loop runs in chunks of max_batch // num_beams images,
        #   all in the one captured graph per (batch, prompt length); counted in decode_stats["hip_beam"]; `last_beam_scores()` gives
        #   the winners' sequences_scores.  Works with weights / activations = "int8" and shared_prefix (the prefill is untouched).
        #   Out of scope, each a ValueError here: grouped_kv, ragged = "hip" / prompt_bucket, early_stop, stop_words_ids, and
        #   sample = "hip" with do_sample or a penalty in the generation arguments; early_stopping, num_return_sequences > 1 and beam
        #   groups are not among the arguments the native path reproduces and take HF `generate`.  classify = "multi_select" /
        #   "constrained" do not generate and ignore the switch.  beams = "hf" (default): num_beams > 1 takes HF `generate`, as before.
        assert decode in ("hf", "graph", "hip") and prefill_linear in ("torch", "cgpt")
        if prefill not in ("model", "hip"):
            raise ValueError(f'prefill={prefill!r}: expected "model" or "hip"')
        if prefill == "hip" and decode != "hip":
            raise ValueError(f'prefill="hip" needs decode="hip" (got decode={decode!r}): the native prefill feeds the native token steps')
        if ragged not in ("hf", "hip"):
            raise ValueError(f'ragged={ragged!r}: expected "hf" or "hip"')
        if ragged == "hip" and (decode != "hip" or prefill != "hip"):
            raise ValueError(f'ragged="hip" needs decode="hip" and prefill="hip" (got decode={decode!r}, prefill={prefill!r}): '
                             "left-padded rows run on the native prefill and the native token steps")
        if weights not in ("fp16", "int8"):
            raise ValueError(f'weights={weights!r}: expected "fp16" or "int8"')
        if weights == "int8" and (decode != "hip" or prefill != "hip"):
            raise ValueError(f'weights="int8" needs decode="hip" and prefill="hip" (got decode={decode!r}, prefill={prefill!r}): '
                             "int8 weights exist on the native engine only, and prompt and steps must run on the same weights")
        if activations not in ("fp16", "int8"):
            raise ValueError(f'activations={activations!r}: expected "fp16" or "int8"')
        if activations == "int8":
            missing = [kw for kw, ok in (('decode="hip"', decode == "hip"), ('prefill="hip"', prefill == "hip"),
                                         ('weights="int8"', weights == "int8")) if not ok]
            if missing:
                raise ValueError(f'activations="int8" needs {", ".join(missing)} (got decode={decode!r}, prefill={prefill!r}, '
                                 f"weights={weights!r}): int8 activations multiply the native engine's int8 weights, in the prompt and "
                                 "in the steps alike")
            if isinstance(outlier_cap, bool) or not isinstance(outlier_cap, int) or not 1 <= outlier_cap <= 1024:
                raise ValueError(f"outlier_cap={outlier_cap!r}: expected an int in 1..1024")
            if isinstance(int8_threshold, bool) or not isinstance(int8_threshold, (int, float)) or int8_threshold != int8_threshold \
                    or abs(int8_threshold) == float("inf"):
                raise ValueError(f"int8_threshold={int8_threshold!r}: expected a finite number (<= 0: no outlier split)")
        if not isinstance(early_stop, bool):
            raise ValueError(f"early_stop={early_stop!r}: expected False or True")
        if early_stop and decode != "hip":
            raise ValueError(f'early_stop=True needs decode="hip" (got decode={decode!r}): only the native token steps can be switched '
                             "off on the device")
        if sample not in ("hf", "hip"):
            raise ValueError(f'sample={sample!r}: expected "hf" or "hip"')
        if sample == "hip" and decode != "hip":
            raise ValueError(f'sample="hip" needs decode="hip" (got decode={decode!r}): the sampler takes the place of the native '
                             "engine's token select")
        if not isinstance(shared_prefix, bool):
            raise ValueError(f"shared_prefix={shared_prefix!r}: expected False or True")
        if shared_prefix and (decode != "hip" or prefill != "hip"):
            raise ValueError(f'shared_prefix=True needs decode="hip" and prefill="hip" (got decode={decode!r}, prefill={prefill!r}): '
                             "the prefix cache is filled and continued by the native prefill")
        stops = check_stop_words_ids(stop_words_ids)
        if stop_text is not None and (not isinstance(stop_text, str) or not stop_text):
            raise ValueError(f"stop_text={stop_text!r}: expected None or a non-empty str")
        if not isinstance(grouped_kv, bool):
            raise ValueError(f"grouped_kv={grouped_kv!r}: expected False or True")
        if grouped_kv and decode != "hip":
            raise ValueError(f'grouped_kv=True needs decode="hip" (got decode={decode!r}): grouped-query attention is a mode of the '
                             "native engine")
        if prompt_bucket is not None:
            if isinstance(prompt_bucket, bool) or not isinstance(prompt_bucket, int) or prompt_bucket < 1:
                raise ValueError(f"prompt_bucket={prompt_bucket!r}: expected None or an int >= 1")
            if ragged != "hip":
                raise ValueError(f'prompt_bucket={prompt_bucket} needs ragged="hip" (got ragged={ragged!r}): only the native engine pads '
                                 "a prompt up to a bucket length")
        if score not in ("hf", "hip"):
            raise ValueError(f'score={score!r}: expected "hf" or "hip"')
        if score == "hip" and (decode != "hip" or prefill != "hip"):
            raise ValueError(f'score="hip" needs decode="hip" and prefill="hip" (got decode={decode!r}, prefill={prefill!r}): '
                             "the candidates are scored on the cache the native prefill fills")
        if classify not in ("generate", "multi_select", "constrained"):
            raise ValueError(f'classify={classify!r}: expected "generate", "multi_select" or "constrained"')
        if constrain not in ("hf", "hip"):
            raise ValueError(f'constrain={constrain!r}: expected "hf" or "hip"')
        if constrain == "hip" and classify != "constrained":
            raise ValueError(f'constrain="hip" needs classify="constrained" (got classify={classify!r})')
        if constrain == "hip" and decode != "hip":
            raise ValueError(f'constrain="hip" needs decode="hip" (got decode={decode!r}): the trie select takes the place of the native '
                             "engine's token select")
        if not 0.0 <= float(label_smoothing) < 1.0:
            raise ValueError(f"label_smoothing={label_smoothing!r}: expected a value in [0, 1)")
        if candidates is not None and classify == "generate":
            raise ValueError('candidates need classify="multi_select" or "constrained" (classify="generate" maps free text through '
                             "label_map)")
        if classify != "generate":
            candidates = list(label_map.answers if candidates is None else candidates)
            if not 2 <= len(candidates) <= self.num_classes - 1:
                raise ValueError(f'classify="{classify}" needs at least 2 and at most num_classes - 1 = {self.num_classes - 1} '
                                 f"candidates (got {len(candidates)}): class id num_classes - 1 stays \"other\"")
        self.end_sym = end_sym
        self.label_smoothing = float(label_smoothing)
        self.score = score
        self.classify = classify
        self.constrain = constrain
        self.candidates = candidates
        self.decode = decode
        self.prefill = prefill
        self.ragged = ragged
        self.prompt_bucket = prompt_bucket
        self.prefill_linear = prefill_linear
        self.weights = weights
        self.early_stop = early_stop
        self.stop_words_ids = stops or None                 # the validated tuple of tuples; None when there is none
        self.stop_text = stop_text
        self.grouped_kv = grouped_kv
        self.shared_prefix = shared_prefix
        self.sample = sample
        self.beams = beams
        self._beam_scores = None                            # `last_beam_scores`
        self._draw_next, self._draw_seed = 0, 0             # `reset_draws`: the ids and the seed of calls that name no sample index
        self._draw_bufs = None                              # (ids [max_batch] int64, seed [1] int64) on the device, made at first use
        if sample == "hip":
            self._sample_settings()                         # a ValueError for a setting the sampler refuses comes now
        if beams not in ("hf", "hip"):
            raise ValueError(f'beams={beams!r}: expected "hf" or "hip"')
        if beams == "hip":                                  # every failing combination is named in ONE message
            bad = [what for what, fails in (
                (f'decode="hip" (got decode={decode!r})', decode != "hip"),
                (f'prefill="hip" (got prefill={prefill!r})', prefill != "hip"),
                ("grouped_kv=False (grouped-query handles are out of scope)", bool(grouped_kv)),
                ('ragged="hf" (left-padded prompts are out of scope)', ragged == "hip"),
                ("prompt_bucket=None (bucketed prompts are out of scope)", prompt_bucket is not None),
                ("early_stop=False (a beam search runs every step)", bool(early_stop)),
                ("stop_words_ids=None (beams finish on EOS ids only)", bool(stops)),
            ) if fails]
            if sample == "hip" and self._sample_settings() is not None:
                bad.append('no do_sample=True / repetition_penalty under sample="hip" (beam sampling and penalised beams are out of scope)')
            if bad:
                raise ValueError('beams="hip" needs ' + "; ".join(bad))
        # the keyword reaches the engine only when it is set (as `law` reaches an encoder)
        engine_kw = {"grouped_kv": True} if grouped_kv else {}
        self.activations, self.int8_threshold, self.outlier_cap = activations, float(int8_threshold), int(outlier_cap)
        if activations == "int8":
            engine_kw.update(activations="int8", int8_threshold=self.int8_threshold, outlier_cap=self.outlier_cap)
        self.trie = None
        if classify == "constrained":                       # every refusal comes now, before the engine is created
            if not self._greedy_defaults(native_sampler=False):
                raise ValueError(f'classify="constrained" is an arg-max over the candidates: generation arguments {self.generate_kwargs!r} '
                                 "(or the checkpoint's generation_config) ask for sampling, a penalty or another decoding mode")
            seqs = [tuple(self._answer_tokens(a).tolist()) for a in candidates]
            eos_ids, _ = self._eos_and_pad_ids()
            for a, seq in zip(candidates, seqs):
                if any(t in eos_ids for t in seq[:-1]):
                    raise ValueError(f"candidate {a!r} holds an end-of-sequence id before its last token (tokens {list(seq)}): HF's "
                                     "generate would end the row there")
            self.trie = build_answer_trie(seqs, int(llama_model.config.vocab_size), names=candidates)
        self._hip = _HipDecoder(llama_model, self.max_batch, weights=weights, early_stop=early_stop, **engine_kw) if decode == "hip" else None
        if self._hip is not None and stops:                 # none is the handle's state at create: nothing is called for it
            self._hip.set_stop_sequences(stops)
        if constrain == "hip":
            self._hip.set_trie(self.trie)
        self.routed_linears = (_LinearRoute.install(llama_model)
                               if (decode in ("graph", "hip") and prefill_linear == "cgpt" and prefill == "model") else 0)
        import collections
        self._graphs = collections.OrderedDict()            # LRU of captured decode graphs, see _generate_graph
        self.max_graphs = 4
        self._prefixes = collections.OrderedDict()          # shared_prefix: LRU of one-row prefix caches, see _prefix_entry
        self.max_prefixes = 4
        self._eos_mask = None
        self.decode_stats = {"graph_replays": 0, "graph_captures": 0, "graph_evictions": 0, "hf_calls": 0, "hf_fallback_kwargs": 0,
                             "hip_steps": 0,                      # token steps enqueued on the native engine (decode = "hip")
                             "hip_prefills": 0,                   # native prefills enqueued (prefill = "hip"), counted alike
                             "hf_score_forwards": 0,              # model forwards of score = "hf": one per candidate and call
                             "hip_scores": 0,                     # native scoring passes (score = "hip"): one per call
                             "hip_ragged_scores": 0,              # native per-row scoring passes (score = "hip", ragged = "hip")
                             "hf_score_fallbacks": 0,             # score = "hip" calls that took the "hf" path (see __init__)
                             "hip_sampled": 0,                    # decodes of the native sampler (sample = "hip"): one per call
                             "hip_prefix_prefills": 0,            # shared_prefix: one-row prefills of a prefix (LRU misses)
                             "hip_prefix_hits": 0,                # shared_prefix: calls that found their prefix in the LRU
                             "hip_constrained": 0,                # native constrained decodes (constrain = "hip"): one per call
                             "hf_constrained": 0,                 # constrained decodes through HF `generate`: one per call
                             "hf_constrained_fallbacks": 0,       # constrain = "hip" calls that took the "hf" path (see __init__)
                             "hip_beam": 0,                       # native beam searches (beams = "hip"): one per call
                             # bytes the native engine holds for weights, scales and scratch (None without one)
                             "weight_bytes": self._hip.weight_bytes if self._hip is not None else None}

    def last_act_stats(self):
        """activations="int8": {rows, outliers, max_outliers_per_row, overflow_rows} of the last native call (one device sync).
        RuntimeError when overflow_rows > 0, naming outlier_cap."""
        if self._hip is None or self.activations != "int8":
            raise RuntimeError('last_act_stats needs activations="int8"')
        return self._hip.act_stats()

    # ---- nn.Module-shaped surface used by Smooth (smoothing.py:42,71)
    def eval(self):
        if hasattr(self.llama_model, "eval"):
            self.llama_model.eval()
        return self

    @property
    def device(self):
        return next(self.llama_model.parameters()).device

    def embed_tokens(self, token_ids):
        """minigpt_base.py:366-371 (the LoRA-wrapped variant resolves to the same table)."""
        return self.llama_model.get_input_embeddings()(token_ids)

    # ---- minigpt_base.py:75-89
    def _segment_ids(self, prompt):
        """The token ids of the prompt's segments as the tokenizer returns them (host tensors [1, n])."""
        segs = prompt.split(IMAGE_PLACEHOLDER)
        return [self.llama_tokenizer(seg, return_tensors="pt", add_special_tokens=(i == 0)).input_ids
                for i, seg in enumerate(segs)]                         # only add bos to the first seg

    def _segment_tokens(self, prompt, device):
        return [t.to(device) for t in self._segment_ids(prompt)]

    def _segment_embeddings(self, prompt, device):
        return [self.embed_tokens(t) for t in self._segment_tokens(prompt, device)]

    def _prefix_entry(self, ids, device):
        """shared_prefix: the `_Prefix` whose token ids are `ids` (a tuple of ints, taken from the tokenizer's host output), from
        the LRU (`max_prefixes` entries, keyed by the ids) or, on a miss, from ONE native prefill of that row -- eager: the caller
        is outside any capture."""
        entry = self._prefixes.get(ids)
        if entry is not None:
            self._prefixes.move_to_end(ids)
            self.decode_stats["hip_prefix_hits"] += 1
            return entry
        while len(self._prefixes) >= max(1, int(self.max_prefixes)):
            self._prefixes.popitem(last=False)
        embs = self.embed_tokens(torch.tensor([list(ids)], dtype=torch.long, device=device)).contiguous()
        k_bufs, v_bufs = self._kv_buffers(embs, 1, len(ids))
        self._hip.prefill(embs, k_bufs, v_bufs)
        self.decode_stats["hip_prefix_prefills"] += 1
        entry = self._prefixes[ids] = _Prefix(ids, k_bufs, v_bufs)
        return entry

    def get_context_emb(self, prompt, img_list):
        seg_embs = self._segment_embeddings(prompt, img_list[0].device)
        assert len(seg_embs) == len(img_list) + 1, "Unmatched numbers of image placeholders and images."
        mixed = [emb for pair in zip(seg_embs[:-1], img_list) for emb in pair] + [seg_embs[-1]]
        return torch.cat(mixed, dim=1)

    # ---- minigpt_base.py:374-448 with encode_img's output given
    def _prompt_inputs(self, img_embeds, texts, allow_prefix=True):
        """The decoder's input for img_embeds [B, queries, hidden] + one prompt per row (or ONE str shared by all rows), as `generate`
        and the constrained decode take it: (embs, attention mask, starts or None, prefix or None, shared, native_pad).
        allow_prefix=False: the caller will not take the native engine, so `embs` must be the WHOLE prompts whatever shared_prefix says
        (HF `generate` knows no prefix cache)."""
        dtype = self.embed_tokens(torch.zeros(1, 1, dtype=torch.long, device=img_embeds.device)).dtype
        img_embeds = img_embeds.to(dtype)
        B = img_embeds.shape[0]
        shared = isinstance(texts, str) or len(set(texts)) == 1
        # the native engine takes left-padded rows only where it would take a shared prompt: on the device, greedy arguments
        native_pad = self.ragged == "hip" and img_embeds.is_cuda and self._greedy_defaults()
        starts = None
        # shared_prefix: on the calls the native engine takes, the rows' common first segment is held once (`prefix`, a `_Prefix`)
        # and `embs` are the suffixes: image tokens + second segment
        use_prefix = (allow_prefix and self.shared_prefix and img_embeds.is_cuda and bool(self._greedy_defaults())
                      and (shared or bool(native_pad)))
        prefix = None
        if shared:
            # shared prompt: segments embedded once and broadcast; equal lengths -> no padding, all-ones mask
            prompt = texts if isinstance(texts, str) else texts[0]
            toks = self._segment_ids(prompt) if use_prefix else []     # host tensors: reading the ids costs no device sync
            ids = tuple(toks[0][0].tolist()) if toks else ()
            if shared_prefix_len([ids]):
                assert len(toks) == 2, "Unmatched numbers of image placeholders and images."
                prefix = self._prefix_entry(ids, img_embeds.device)
                embs = torch.cat([img_embeds, self.embed_tokens(toks[1].to(img_embeds.device)).expand(B, -1, -1)], dim=1)
            else:
                segs = self._segment_embeddings(prompt, img_embeds.device)
                assert len(segs) == 2, "Unmatched numbers of image placeholders and images."
                embs = torch.cat([segs[0].expand(B, -1, -1), img_embeds, segs[1].expand(B, -1, -1)], dim=1)
            if native_pad and self.prompt_bucket:                      # padded up to the bucket: one graph for every length in it
                embs, attn_mask, starts = left_pad_embeds([embs], self.prompt_bucket, prefix=prefix.P if prefix else 0)
            else:
                attn_mask = torch.ones(embs.shape[:2], dtype=torch.int, device=embs.device)
        else:
            assert len(texts) == B
            row_toks = [self._segment_ids(t) for t in texts] if use_prefix else []       # host tensors, as above
            ids = tuple(row_toks[0][0][0].tolist()) if row_toks else ()
            if shared_prefix_len([t[0][0].tolist() for t in row_toks]):     # every row's first segment is `ids`
                assert all(len(t) == 2 for t in row_toks), "Unmatched numbers of image placeholders and images."
                prefix = self._prefix_entry(ids, img_embeds.device)
                batch_embs = [torch.cat([img_embeds[i][None], self.embed_tokens(t[1].to(img_embeds.device))], dim=1)
                              for i, t in enumerate(row_toks)]
            else:
                batch_embs = [self.get_context_emb(t, [img_embeds[i][None]]) for i, t in enumerate(texts)]
            embs, attn_mask, starts = left_pad_embeds(batch_embs, self.prompt_bucket if native_pad else None,
                                                      prefix=prefix.P if prefix else 0)                        # minigpt_base.py:407-416
            if not native_pad:
                starts = None
        return embs, attn_mask, starts, prefix, shared, native_pad

    @torch.no_grad()
    def generate_from_embeds(self, img_embeds, texts, draws=None):
        """img_embeds [B, queries, hidden] (any float dtype) + one prompt per row (or ONE str shared by all rows) -> list[str].
        draws (sample = "hip" only): (first draw id, seed) -- row r draws stream first + r; None: the running counter (`reset_draws`)."""
        embs, attn_mask, starts, prefix, shared, native_pad = self._prompt_inputs(img_embeds, texts)
        B = embs.shape[0]
        if self.decode in ("graph", "hip") and (shared or native_pad) and embs.is_cuda and self._greedy_defaults():
            if self._sample_settings() is not None:                     # written before the replay: the kernels read them when they run
                self._write_draws(B, draws, embs.device)
                self.decode_stats["hip_sampled"] += 1
            # without a prefix the call is the two-argument one it always was (callers wrap this method with that signature)
            beam = self._beam_settings() is not None                   # the graph then returns (tokens, sequences_scores)
            outputs = self._generate_graph(embs, starts, prefix) if prefix else self._generate_graph(embs, starts)
            if beam:
                outputs, self._beam_scores = outputs
                self.decode_stats["hip_beam"] += 1
            if self.activations == "int8":                              # the tokens are read next: the same sync
                self.last_act_stats()
        else:
            self.decode_stats["hf_calls"] += 1
            if self.decode in ("graph", "hip") and (shared or self.ragged == "hip") and embs.is_cuda:
                self.decode_stats["hf_fallback_kwargs"] += 1            # generation arguments outside the greedy whitelist
            outputs = self.llama_model.generate(inputs_embeds=embs, attention_mask=attn_mask, max_new_tokens=self.max_new_tokens,
                                                **self.hf_generate_kwargs())
        return self._decode_outputs(outputs)

    @torch.no_grad()
    def constrained_from_embeds(self, img_embeds, texts, return_logits=False):
        """classify = "constrained": img_embeds [B, queries, hidden] + one prompt per row (or ONE str) -> (labels [B] int32, tokens
        [B, depth] int64) on the embeds' device: labels[b] = the index in `candidates` of the answer row b spelled, tokens its
        tokens followed by pad ids.  Nothing is read back.  return_logits (the "hf" path only): also HF's raw per-step logits
        [B, steps, V]."""
        assert self.trie is not None, 'constrained_from_embeds needs classify="constrained"'
        # decided before the inputs are built: only the native engine may be handed a prompt whose shared prefix sits in a cache
        shared = isinstance(texts, str) or len(set(texts)) == 1
        native = (self.constrain == "hip" and not return_logits and img_embeds.is_cuda and img_embeds.shape[0] <= self.max_batch
                  and (shared or self.ragged == "hip"))
        embs, attn_mask, starts, prefix, _, _ = self._prompt_inputs(img_embeds, texts, allow_prefix=native)
        if native:
            tokens, labels = self._generate_graph(embs, starts, prefix, constrained=True)
            self.decode_stats["hip_constrained"] += 1
            return labels, tokens
        if self.constrain == "hip" and not return_logits:
            self.decode_stats["hf_constrained_fallbacks"] += 1
        self.decode_stats["hf_constrained"] += 1
        _, pad = self._eos_and_pad_ids()
        kw = self.hf_generate_kwargs()
        kw.pop("stopping_criteria", None)                              # stop sequences belong to generate(): the trie ends the rows
        kw.pop("min_new_tokens", None)                                 # and no EOS column is masked: the law reads the raw logits
        out = self.llama_model.generate(inputs_embeds=embs, attention_mask=attn_mask, max_new_tokens=self.trie.depth,
                                        prefix_allowed_tokens_fn=allowed_tokens_fn(self.trie, pad), return_dict_in_generate=True,
                                        output_logits=bool(return_logits), **kw)
        seq = out.sequences[:, -self.trie.depth:] if out.sequences.shape[1] > self.trie.depth else out.sequences
        tokens = torch.full((embs.shape[0], self.trie.depth), int(pad), dtype=torch.long, device=embs.device)
        tokens[:, :seq.shape[1]] = seq                                 # HF ends the call once every row has finished on an EOS
        walked = trie_walk(tokens, self.trie)
        if min(walked) < 0:                                            # e.g. a candidate token equal to the pad id HF appends
            b = walked.index(-1)
            raise RuntimeError(f'classify="constrained": row {b} of HF generate spells no candidate (tokens {tokens[b].tolist()})')
        labels = torch.tensor(walked, dtype=torch.int32, device=embs.device)
        if return_logits:
            return labels, tokens, torch.stack([l.float() for l in out.logits], dim=1)
        return labels, tokens

    def _decode_outputs(self, outputs):
        """minigpt_base.py:440-447."""
        answers = []
        for output_token in outputs:
            if output_token[0] == 0:
                output_token = output_token[1:]
            text = self.llama_tokenizer.decode(output_token, skip_special_tokens=True)
            if self.stop_text is not None:                             # Chat.answer: output_text.split('###')[0]
                text = text.split(self.stop_text)[0]
            answers.append(clean_answer(text))
        return answers

    # ---- greedy decode without host round trips (decode = "graph")
    # generation arguments the fixed-length greedy loop reproduces, with the values at which it does (None = any value: without
    # sampling and with one beam HF ignores it).  Anything else -- eos_token_id, stopping_criteria, no_repeat_ngram_size,
    # bad_words_ids, min_new_tokens, max_length, logits_processor, ... -- takes the HF path, so the same classifier never decodes
    # differently by `decode=`.
    _GREEDY_NEUTRAL = {"num_beams": 1, "do_sample": False, "repetition_penalty": 1, "min_length": None, "top_p": None,
                       "temperature": None, "length_penalty": None, "top_k": None}
    # fields of the checkpoint's own `generation_config` (generation_config.json; `generate` merges it under the call's arguments) that
    # create a logits processor, a stopping rule or another decoding mode, with the values at which they do nothing
    _CONFIG_NEUTRAL = {"repetition_penalty": (None, 1, 1.0), "no_repeat_ngram_size": (None, 0), "encoder_no_repeat_ngram_size": (None, 0),
                       "encoder_repetition_penalty": (None, 1, 1.0), "bad_words_ids": (None,), "suppress_tokens": (None,),
                       "begin_suppress_tokens": (None,), "forced_bos_token_id": (None,), "forced_eos_token_id": (None,),
                       "sequence_bias": (None,), "min_new_tokens": (None, 0), "num_beams": (None, 1), "num_beam_groups": (None, 1),
                       "do_sample": (None, False), "penalty_alpha": (None, 0, 0.0), "exponential_decay_length_penalty": (None,),
                       "renormalize_logits": (None, False), "remove_invalid_values": (None, False), "guidance_scale": (None, 1, 1.0),
                       "watermarking_config": (None,), "prompt_lookup_num_tokens": (None,), "stop_strings": (None,),
                       "diversity_penalty": (None, 0, 0.0), "max_time": (None,), "dola_layers": (None,)}

    def _greedy_defaults(self, native_sampler=None):
        """May this call take the fixed-length greedy loop?  Only when every argument of the call AND every field of the model's own
        generation_config (which `generate` applies wherever the call is silent) is one the loop reproduces; otherwise the HF path
        runs, so the same classifier never decodes differently by `decode=`.
        native_sampler (None: sample == "hip"): whether the sampling fields count as reproduced at any value.
        beams == "hip": num_beams in 2..8 with a finite length_penalty counts as reproduced too, unless the call also samples or
        penalises, or the call or the checkpoint sets early_stopping, num_return_sequences or num_beam_groups (`_beam_settings`)."""
        sampler = self.sample == "hip" if native_sampler is None else bool(native_sampler)
        beam = native_sampler is None and getattr(self, "beams", "hf") == "hip" and self._beam_settings() is not None
        if beam and self._sample_settings() is not None:
            return False
        for key, val in self.generate_kwargs.items():
            if key not in self._GREEDY_NEUTRAL:
                return False
            if sampler and key in SAMPLE_FIELDS:         # the native sampler takes these at any value it accepts
                continue
            if beam and key in BEAM_FIELDS:              # the native beam search takes these at the values `_beam_settings` accepted
                continue
            want = self._GREEDY_NEUTRAL[key]
            if want is not None and val != want:
                return False
        gen = getattr(self.llama_model, "generation_config", None)
        if gen is not None:
            for key, neutral in self._CONFIG_NEUTRAL.items():
                if key in self.generate_kwargs or (sampler and key in SAMPLE_FIELDS):
                    continue                                           # the call's argument wins over the checkpoint's field
                val = getattr(gen, key, None)
                if isinstance(val, (list, tuple, dict)) and len(val) == 0:
                    val = None
                if val not in neutral:
                    return False
        return True

    def _beam_settings(self):
        """beams = "hip": (num_beams, length_penalty) as `generate` would resolve them -- the call's argument, else the checkpoint's
        generation_config, else GenerationConfig's default, and so for early_stopping, num_return_sequences and num_beam_groups --
        when they ask for 2..8 beams with a finite length penalty and nothing else, else None (one beam: the greedy entries; anything
        `check_beam_settings` refuses, wherever it was set: HF `generate`).  None under beams = "hf"."""
        if getattr(self, "beams", "hf") != "hip":
            return None
        gen = getattr(self.llama_model, "generation_config", None)
        vals = {}
        for key, default in BEAM_HF_DEFAULTS.items():
            val = self.generate_kwargs.get(key)
            val = getattr(gen, key, None) if val is None else val
            vals[key] = default if val is None else val
        try:
            return check_beam_settings(**vals)
        except ValueError:
            return None

    def last_beam_scores(self):
        """beams = "hip": the `sequences_scores` of the last native beam search, [B] fp32 on the device (the winners' summed log
        probabilities over length ** length_penalty).  RuntimeError when none has run."""
        if self._beam_scores is None:
            raise RuntimeError('last_beam_scores: no native beam search (beams="hip", num_beams > 1) has run on this classifier')
        return self._beam_scores

    def _beam_chunks(self, logits, L, beam, min_new, eos_ids, pad, k_bufs, v_bufs, return_logits):
        """The native beam search on the prompt caches a prefill of B images left, in chunks of max_batch // num_beams images (the
        engine's workspace holds max_batch rows): each chunk reads ITS rows of the prompt caches through offset table pointers; the
        beam caches are allocated once, for the largest chunk, and reused in stream order."""
        k, lp = beam
        B, n = logits.shape[0], self.max_new_tokens
        per = self.max_batch // k
        if per < 1:
            raise ValueError(f"num_beams={k} > max_batch={self.max_batch}: the native engine's workspace holds max_batch beam rows")
        shape = (min(per, B) * k, self._hip.kv_heads, max(1, n - 1), 128)
        bk = [logits.new_empty(shape, dtype=torch.float16) for _ in range(self._hip.layers)]
        bv = [logits.new_empty(shape, dtype=torch.float16) for _ in range(self._hip.layers)]
        outs = []
        for c0 in range(0, B, per):
            c1 = min(B, c0 + per)
            rows = (c1 - c0) * k
            outs.append(self._hip.beam(logits[c0:c1], k, L, n, min_new, eos_ids, pad, lp, [t[c0:c1] for t in k_bufs],
                                       [t[c0:c1] for t in v_bufs], [t[:rows] for t in bk], [t[:rows] for t in bv],
                                       return_logits=return_logits))
        cat_dims = (0, 0, 0, 1)                                         # tokens, scores, step logits by row; the trace by image
        return tuple(torch.cat([o[j] for o in outs], dim=cat_dims[j]) for j in range(len(outs[0])))

    def _sample_settings(self):
        """sample = "hip": (do_sample, temperature, top_k, top_p, repetition_penalty) as `generate` would resolve them -- the call's
        argument, else the checkpoint's generation_config, else GenerationConfig's default -- or None when they amount to the plain
        arg-max (no sampling, no penalty), which stays on the greedy entries.  None under sample = "hf"."""
        if self.sample != "hip":
            return None
        gen = getattr(self.llama_model, "generation_config", None)
        vals = []
        for key in SAMPLE_FIELDS:
            val = self.generate_kwargs.get(key)
            val = getattr(gen, key, None) if val is None else val
            vals.append(SAMPLE_HF_DEFAULTS[key] if val is None else val)
        settings = check_sample_settings(vals)
        return settings if settings[0] or settings[4] != 1.0 else None

    def reset_draws(self, next=0, seed=None):
        """sample = "hip": calls that name no sample index (`generate`, `__call__`) draw streams next, next + 1, ... in row order, one
        per row, under `seed` (None: unchanged; 0 at construction).  A reset to the same values reproduces the calls that follow."""
        self._draw_next = int(next)
        if seed is not None:
            self._draw_seed = int(seed)

    def _write_draws(self, B, draws, device):
        """The persistent draw-id and seed tensors of the native sampler, set for the next decode of B rows."""
        if self._draw_bufs is None or self._draw_bufs[0].device != device:
            self._draw_bufs = (torch.zeros(self.max_batch, dtype=torch.int64, device=device),
                               torch.zeros(1, dtype=torch.int64, device=device))
        if draws is None:
            first, seed = self._draw_next, self._draw_seed
            self._draw_next += B
        else:
            first, seed = int(draws[0]), int(draws[1])
        seed &= 0xFFFFFFFFFFFFFFFF
        self._draw_bufs[0][:B].copy_(torch.arange(first, first + B, dtype=torch.int64, device=device))
        self._draw_bufs[1].fill_(seed - (1 << 64) if seed >= 1 << 63 else seed)     # the 64 bits, as int64
        return self._draw_bufs

    def _select(self, logits, L, min_new, eos_ids, pad, k_bufs, v_bufs, return_logits, starts=None, constrained=False):
        """The native loop after the prefill: the sampler under sample = "hip" when the settings ask for it, the arg-max otherwise;
        constrained: the trie select (tokens and labels)."""
        if constrained:
            return self._hip.constrained(logits, L, pad, k_bufs, v_bufs, return_logits=return_logits, starts=starts)
        settings = self._sample_settings()
        if settings is None:
            return self._hip.greedy(logits, L, self.max_new_tokens, min_new, eos_ids, pad, k_bufs, v_bufs, return_logits=return_logits,
                                    starts=starts)
        if self._draw_bufs is None or self._draw_bufs[0].device != logits.device:
            self._write_draws(logits.shape[0], None, logits.device)
        ids, seed = self._draw_bufs
        return self._hip.sample(logits, L, self.max_new_tokens, min_new, eos_ids, pad, k_bufs, v_bufs, settings, ids[:logits.shape[0]],
                                seed, return_logits=return_logits, starts=starts)

    def min_new_tokens(self):
        """Generated tokens before which EOS is suppressed.  The reference passes `min_length = 1` with `inputs_embeds`
        (minigpt_base.py:385) to transformers 4.30.0 (its pin, docker/tpu-docker:32), which counts GENERATED tokens in that call: the
        first token is never EOS and an answer is never empty.  Later versions subtract the embedded prompt's length from min_length
        (5.15: `_prepare_generated_length`, max(min_length - inputs_embeds.shape[1], 0) = 0).  This class ships the REFERENCE's
        semantics on both decode paths, whatever transformers is installed."""
        return int(self.generate_kwargs.get("min_length", 1) or 0)

    def hf_generate_kwargs(self):
        """`generate_kwargs` as handed to the installed `generate`: the reference's `min_length` travels as `min_new_tokens`, which
        means "generated tokens" in every transformers version (and takes precedence over min_length where both exist), and
        `min_length` itself is handed over as an explicit 0."""
        kw = dict(self.generate_kwargs)
        ml = kw.pop("min_length", None)
        if ml and "min_new_tokens" not in kw:
            kw["min_new_tokens"] = int(ml)
        # never SILENT on min_length: where the call says nothing `generate` applies the checkpoint's own generation_config.min_length,
        # which the greedy loop (min_new_tokens() above) would not see -- the two decode paths of one classifier would then differ
        kw["min_length"] = 0
        if self.stop_words_ids:                                        # the per-row rule on the HF path (see __init__)
            from transformers import StoppingCriteriaList
            kw["stopping_criteria"] = StoppingCriteriaList(list(kw.get("stopping_criteria") or []) +
                                                           list(stop_sequences_criteria(self.stop_words_ids)))
        return kw

    def _eos_and_pad_ids(self):
        """(eos ids, pad id) as `generate` resolves them: the checkpoint's generation_config, else its config; without a pad id the
        first EOS id, else 0."""
        llm = self.llama_model
        gen = getattr(llm, "generation_config", None)
        eos = getattr(gen, "eos_token_id", None)
        eos = getattr(llm.config, "eos_token_id", None) if eos is None else eos
        eos_ids = list(eos) if isinstance(eos, (list, tuple)) else ([eos] if eos is not None else [])
        pad = getattr(gen, "pad_token_id", None)
        pad = getattr(llm.config, "pad_token_id", None) if pad is None else pad
        pad = (eos_ids[0] if eos_ids else 0) if pad is None else pad
        return eos_ids, pad

    def _kv_buffers(self, embs, B, length):
        """One K and one V buffer per layer for the native engine, [B, kv_heads, length, 128] each, allocated by `embs.new_empty`:
        inside a capture they belong to the graph's pool."""
        shape = (B, self._hip.kv_heads, length, 128)
        return ([embs.new_empty(shape) for _ in range(self._hip.layers)], [embs.new_empty(shape) for _ in range(self._hip.layers)])

    def greedy_tokens(self, embs, return_logits=False, starts=None, prefix=None, constrained=False):
        """What `generate(inputs_embeds=embs, attention_mask=ones, max_new_tokens=n, do_sample=False, min_length=1, ...)` returns for
        prompts without padding, as a straight loop of the model's own forward calls: [B, n] token ids, pad_token_id after a row's
        EOS.  (HF additionally stops, and truncates, at the step where every row has finished; the extra columns here are pad ids,
        which decode to nothing.)  No data-dependent control flow: capturable as one graph.
        starts ([B] int32 on the device, prefill = "hip" only): row b of `embs` is left-padded by starts[b] positions (zeros); the
        result is what each row gives without its padding.
        prefix (a `_Prefix`, prefill = "hip" only): `embs` are the positions AFTER P positions
        every row shares; their one-row caches are copied into every row, the prefill continues at position P, and the result is
        what the whole prompts give.
        constrained (constrain = "hip" only): the trie select in the arg-max's place, `trie.depth` tokens instead of max_new_tokens
        -> (tokens [B, depth], labels [B] int32[, step logits])."""
        from transformers import DynamicCache
        from transformers.cache_utils import DynamicLayer

        class PreallocLayer(DynamicLayer):
            """DynamicLayer whose keys / values are exact-length views of buffers allocated once for prompt + new tokens: same
            values as the concatenating layer, without re-copying the whole cache at every step (4 ms of an 18-ms step at 200 rows
            x 32 layers; profiles/r03/minigpt4_decode.txt)."""

            def __init__(self, max_len):
                super().__init__()
                self.max_len, self.used, self.buf_k, self.buf_v = max_len, 0, None, None

            def update(self, key_states, value_states, *args, **kwargs):
                if self.buf_k is None:
                    b, h, _, d = key_states.shape
                    self.buf_k = key_states.new_empty((b, h, self.max_len, d))
                    self.buf_v = value_states.new_empty((b, h, self.max_len, d))
                    self.dtype, self.device, self.is_initialized = key_states.dtype, key_states.device, True
                n = key_states.shape[-2]
                self.buf_k[:, :, self.used:self.used + n] = key_states
                self.buf_v[:, :, self.used:self.used + n] = value_states
                self.used += n
                self.keys, self.values = self.buf_k[:, :, :self.used], self.buf_v[:, :, :self.used]
                return self.keys, self.values

        llm = self.llama_model
        eos_ids, pad = self._eos_and_pad_ids()
        B, L, _ = embs.shape
        assert not constrained or (self._hip is not None and self._hip.trie is not None), 'a constrained loop needs constrain="hip"'
        num_new = self.trie.depth if constrained else self.max_new_tokens
        if constrained:                                                # the trie ends the rows: no EOS id, no EOS mask
            eos_ids = []
        assert starts is None or self.prefill == "hip", 'left-padded rows need prefill="hip"'
        assert prefix is None or self.prefill == "hip", 'a shared prefix needs prefill="hip"'
        if self.prefill == "hip":                                      # the whole decode in this library: no HF forward, no DynamicCache
            assert B <= self.max_batch, f"{B} rows > max_batch {self.max_batch} (the native decoder's workspace)"
            if prefix is not None:                                     # the prompt is the P shared positions + these L
                P, pk, pv = prefix.P, prefix.k, prefix.v
                L += P
            beam = None if constrained else self._beam_settings()
            # what PreallocLayer allocates on the other path; under beams the generated positions live in the beam caches
            k_bufs, v_bufs = self._kv_buffers(embs, B, L if beam is not None else L + num_new)
            if prefix is not None:
                self._hip.kv_broadcast(pk, pv, P, k_bufs, v_bufs, starts=starts)
                logits = self._hip.prefill_from(embs.contiguous(), P, k_bufs, v_bufs, starts=starts)
            else:
                logits = self._hip.prefill(embs.contiguous(), k_bufs, v_bufs, starts=starts)
            self.decode_stats["hip_prefills"] += 1
            self.decode_stats["hip_steps"] += num_new - 1
            if beam is not None:                                       # (tokens, scores[, step logits, trace]): see `_beam_chunks`
                return self._beam_chunks(logits, L, beam, self.min_new_tokens() if eos_ids else 0, eos_ids, pad, k_bufs, v_bufs, return_logits)
            return self._select(logits, L, self.min_new_tokens() if eos_ids else 0, eos_ids, pad, k_bufs, v_bufs, return_logits, starts,
                                constrained=constrained)
        cache = DynamicCache(config=llm.config)
        cache.layers = [PreallocLayer(L + num_new) for _ in cache.layers] or cache.layers
        pos = torch.arange(L, device=embs.device).unsqueeze(0)
        out = llm(inputs_embeds=embs, position_ids=pos, past_key_values=cache, use_cache=True, logits_to_keep=1)
        logits = out.logits[:, -1, :].float()
        min_new = self.min_new_tokens() if eos_ids else 0              # MinNewTokensLengthLogitsProcessor: no EOS on the first tokens
        if min_new > 0:
            key = (str(embs.device), logits.shape[-1])
            if self._eos_mask is None or self._eos_mask[0] != key:     # built outside any capture (the warm-up run comes first)
                m = torch.zeros(logits.shape[-1], dtype=torch.bool)
                m[eos_ids] = True
                self._eos_mask = (key, m.to(embs.device))
        if self._hip is not None:                                      # decode = "hip": the loop below, in this library's kernels
            assert B <= self.max_batch, f"{B} rows > max_batch {self.max_batch} (the native decoder's workspace)"
            self.decode_stats["hip_steps"] += num_new - 1
            return self._select(logits.contiguous(), L, min_new, eos_ids, pad, [l.buf_k for l in cache.layers],
                                [l.buf_v for l in cache.layers], return_logits, constrained=constrained)
        unfinished = torch.ones(B, dtype=torch.long, device=embs.device)
        tokens, step_logits = [], []
        for i in range(self.max_new_tokens):
            if i < min_new:
                logits = logits.masked_fill(self._eos_mask[1], float("-inf"))
            if return_logits:
                step_logits.append(logits)
            nxt = logits.argmax(dim=-1)
            nxt = nxt * unfinished + pad * (1 - unfinished)
            tokens.append(nxt)
            for e in eos_ids:
                unfinished = unfinished * (nxt != e).long()
            for seq in self.stop_words_ids or ():                      # the row's last len(seq) step tokens against the sequence
                if len(seq) <= i + 1:
                    hit = tokens[i + 1 - len(seq)] == seq[0]
                    for k in range(1, len(seq)):
                        hit = hit & (tokens[i + 1 - len(seq) + k] == seq[k])
                    unfinished = unfinished * (~hit).long()
            if i + 1 == self.max_new_tokens:
                break
            pos = torch.full((1, 1), L + i, device=embs.device, dtype=torch.long)
            out = llm(input_ids=nxt[:, None], position_ids=pos, past_key_values=cache, use_cache=True, logits_to_keep=1)
            logits = out.logits[:, -1, :].float()
        if return_logits:                                              # tests: the per-step logits the argmax was taken on
            return torch.stack(tokens, dim=1), torch.stack(step_logits, dim=1)
        return torch.stack(tokens, dim=1)

    def _graph_key(self, embs, ragged=False, prefix=0, constrained=False):
        key = (embs.shape[0], embs.shape[1], embs.dtype, embs.device.index, self.max_new_tokens, bool(self.routed_linears), self.decode,
               self.prefill)
        key = key + ("ragged",) if ragged else key                    # a graph of the _ragged entries is never an unpadded one's
        key = key + ("prefix", int(prefix)) if prefix else key        # nor is one that continues P shared positions (`embs`: the rest)
        key = key + ("grouped_kv",) if self.grouped_kv else key
        key = key + ("early_stop",) if self.early_stop else key       # nor is one captured with early stop on one captured without
        key = key + ("stop", self.stop_words_ids) if self.stop_words_ids else key      # nor under one set of stop sequences another's
        if constrained:                                               # nor the trie select under one trie another's, or the arg-max's
            return key + ("constrained", self.trie.depth, id(self.trie))
        if self._beam_settings() is not None:                         # nor a beam search under one setting another's, or the arg-max's
            return key + ("beams",) + self._beam_settings()
        settings = self._sample_settings()
        return key + ("sample", settings) if settings is not None else key             # nor the sampler under one law another's

    def last_live_steps(self):
        """Token steps of the most recent native greedy decode (eager, or the last graph replay) that actually ran: max_new_tokens - 1
        with early_stop off, min(F, max_new_tokens - 1) with it on, F = the first select at which every row had produced an EOS.
        ONE host sync, which is why it is never read on its own after a replay.  RuntimeError when no native greedy decode has run."""
        if self._hip is None:
            raise RuntimeError('last_live_steps: no native engine (decode="hip") on this classifier')
        return self._hip.live_steps()

    def _generate_graph(self, embs, starts=None, prefix=None, constrained=False):
        """One captured hipGraph per (batch, prompt length, dtype, device, max_new_tokens, routed prefill, engine, prefill engine), kept in an LRU of
        `max_graphs` entries: a graph pins its private pool -- the pre-allocated K / V of every layer plus activations, ~6.7 GB of K / V
        alone at 200 rows x 32 layers x 64 positions -- and ragged last batches or new prompt lengths add entries; the least recently
        used one is dropped (graph and static tensors freed) before a new capture.
        starts (left-padded rows, see greedy_tokens): the graph is captured on a static copy that is refreshed before every replay, like
        the embeds -- the kernels read it when they run, so one graph per (batch, PADDED length) serves every mix of prompt lengths.
        prefix (shared_prefix, see greedy_tokens): the graph reads the prefix caches from static tensors of its own, which are
        refreshed before a replay only when they hold another prefix than the wanted one (the ids are compared on the host): with one
        template for a whole dataset nothing is copied.
        constrained (see greedy_tokens): the static output is the pair (tokens, labels)."""
        key = self._graph_key(embs, ragged=starts is not None, prefix=prefix.P if prefix else 0, constrained=constrained)
        entry = self._graphs.get(key)
        if entry is not None:
            self._graphs.move_to_end(key)
        if entry is None:
            while len(self._graphs) >= max(1, int(self.max_graphs)):
                _, old = self._graphs.popitem(last=False)
                del old
                self.decode_stats["graph_evictions"] += 1
                torch.cuda.empty_cache()                                # return the evicted graph's pool before capturing again
            static_in = embs.clone()
            static_starts = None if starts is None else starts.clone()
            static_prefix = None if prefix is None else prefix.clone()
            extra = {} if prefix is None else {"prefix": static_prefix}
            if constrained:
                extra["constrained"] = True
            side = torch.cuda.Stream(device=embs.device)
            side.wait_stream(torch.cuda.current_stream())
            import contextlib
            route = _LinearRoute.enabled() if self.routed_linears else contextlib.nullcontext()
            hip_steps = self.decode_stats["hip_steps"]                 # counted per replay below, not for warm-up and capture
            hip_prefills = self.decode_stats["hip_prefills"]
            with route:
                with torch.cuda.stream(side):                          # warm-up outside the capture (lazy initialisations)
                    self.greedy_tokens(static_in, starts=static_starts, **extra)
                torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                # No cyclic garbage may be finalised INSIDE the capture: a dropped classifier that sits in a reference cycle still owns
                # its engine and its graphs' private pools, and the device frees of their finalisers abort the process when they run
                # while a stream is capturing.  The model's own prefill allocates enough Python objects to start a collection there.
                import gc
                gc.collect()
                gc_was_on = gc.isenabled()
                gc.disable()
                try:
                    with torch.cuda.graph(graph):
                        static_out = self.greedy_tokens(static_in, starts=static_starts, **extra)
                finally:
                    if gc_was_on:
                        gc.enable()
            self.decode_stats["hip_steps"] = hip_steps
            self.decode_stats["hip_prefills"] = hip_prefills
            entry = (graph, static_in, static_out, static_starts, static_prefix)
            self._graphs[key] = entry
            self.decode_stats["graph_captures"] += 1
        graph, static_in, static_out, static_starts, static_prefix = entry
        static_in.copy_(embs)
        if static_starts is not None:
            static_starts.copy_(starts)
        if static_prefix is not None:
            static_prefix.hold(prefix)
        graph.replay()
        self.decode_stats["graph_replays"] += 1
        if self._hip is not None:
            self.decode_stats["hip_steps"] += (self.trie.depth if constrained else self.max_new_tokens) - 1
        if self.prefill == "hip":
            self.decode_stats["hip_prefills"] += 1
        return tuple(t.clone() for t in static_out) if isinstance(static_out, tuple) else static_out.clone()

    @torch.no_grad()
    def generate(self, images, texts, **_ignored):
        """`MiniGPTBase.generate(images, texts, ...)` -> list[str] (generation arguments are fixed at construction)."""
        img_embeds, _ = self.encoder.encode_img(images)
        return self.generate_from_embeds(img_embeds, texts)

    # ---- minigpt_base.py:451-467 with encode_img's output given
    def _answer_tokens(self, text):
        ids = self.llama_tokenizer(text + self.end_sym, return_tensors="pt", add_special_tokens=False).input_ids[0]
        if ids.numel() < 1:
            raise ValueError(f"candidate answer {text!r} + end_sym {self.end_sym!r} has no token")
        return ids

    def _prompt_embeds(self, prompt, img_embeds):
        """bos + the prompt's segments around the rows' image embeds, [rows, L, hidden]: the bos is added explicitly
        (minigpt_base.py:332-338) and every segment is tokenised with add_special_tokens=False (prompt_wrap, :118-129)."""
        dev = img_embeds.device
        segs = [self.embed_tokens(self.llama_tokenizer(seg, return_tensors="pt", add_special_tokens=False).input_ids.to(dev))
                for seg in prompt.split(IMAGE_PLACEHOLDER)]
        assert len(segs) == 2, "Unmatched numbers of image placeholders and images."
        bos = self.embed_tokens(torch.full((1, 1), int(self.llama_tokenizer.bos_token_id), dtype=torch.long, device=dev))
        rows = img_embeds.shape[0]
        return torch.cat([bos.expand(rows, -1, -1), segs[0].expand(rows, -1, -1), img_embeds, segs[1].expand(rows, -1, -1)], dim=1)

    @torch.no_grad()
    def answer_losses_from_embeds(self, img_embeds, texts, answers):
        """img_embeds [B, queries, hidden] + one prompt per row (or ONE str shared by all rows) + `answers[c][b]` = candidate c for
        row b (answers[c] may be ONE str for all rows) -> losses [B, C] fp32: `multi_select`'s `all_losses`.

        The loss law is the reference's, quirks included (`forward(..., reduction='none')`, minigpt_base.py:320-363 with
        preparing_embedding :254-318 -- for the loss: :295-350 -- and modeling_llama.py:101-123):
          * the sequence is bos + prompt segments around the image embeds + the tokens of `answer + end_sym`; prompt and answer are
            tokenised with add_special_tokens=False, the bos is added explicitly (minigpt_base.py:298-305, :332-338);
          * targets are the answer tokens only (-100 elsewhere, :343-350); an answer token equal to the tokenizer's pad id is masked
            out too (:312-314);
          * each token's loss is CrossEntropyLoss(reduction="none", label_smoothing=0.1) on `logits.float()` (modeling_llama.py:84,105);
          * the per-row loss is `.view(B, -1).mean(1)` (modeling_llama.py:122-123): the SUM over the answer tokens divided by
            (sequence length - 1), not by the number of answer tokens.  With L = prompt length including the bos and T_c = answer
            tokens the divisor is L + T_c - 1, per candidate (one forward each); if candidate c's answers (or the prompts) differ in
            length over the rows, T_c (L) is the longest, because `preparing_embedding` / `prompt_wrap` pad on the right (minigpt_base.py:132-143, :298-305).
        score="hf": one forward of the model per candidate over the concatenated embeds (CPU tensors work).  score="hip": see __init__."""
        dtype = self.embed_tokens(torch.zeros(1, 1, dtype=torch.long, device=img_embeds.device)).dtype
        img_embeds = img_embeds.to(dtype)
        B = img_embeds.shape[0]
        prompts = [texts] * B if isinstance(texts, str) else list(texts)
        assert len(prompts) == B
        answers = [[a] * B if isinstance(a, str) else list(a) for a in answers]
        assert answers and all(len(a) == B for a in answers), "answers[c][b]: one answer per candidate and row"
        if self.score == "hip":
            native = self._native_losses(img_embeds, prompts, answers)
            if native is not None:
                return native
            self.decode_stats["hf_score_fallbacks"] += 1
        dev = img_embeds.device
        if len(set(prompts)) == 1:
            cond = [self._prompt_embeds(prompts[0], img_embeds)]
            cond_rows = [(0, i) for i in range(B)]                     # (group, row within the group)
        else:
            cond = [self._prompt_embeds(t, img_embeds[i:i + 1]) for i, t in enumerate(prompts)]
            cond_rows = [(i, 0) for i in range(B)]
        lens = [int(cond[g].shape[1]) for g, _ in cond_rows]
        Lmax = max(lens)
        pad_id = getattr(self.llama_tokenizer, "pad_token_id", None)
        pad_emb = self.embed_tokens(torch.tensor([[0 if pad_id is None else int(pad_id)]], device=dev))[0, 0]
        loss_fct = torch.nn.CrossEntropyLoss(reduction="none", label_smoothing=self.label_smoothing)
        losses = []
        for cand in answers:
            toks = {a: self._answer_tokens(a).to(dev) for a in set(cand)}
            Tmax = max(int(t.numel()) for t in toks.values())
            total = Lmax + Tmax
            embs = pad_emb.expand(B, total, -1).clone()
            mask = torch.zeros((B, total), dtype=torch.int, device=dev)
            targets = torch.full((B, total), -100, dtype=torch.long, device=dev)
            for b, (g, r) in enumerate(cond_rows):                     # prompt, then the answer right behind it, then padding
                ids = toks[cand[b]]
                n, T = lens[b], int(ids.numel())
                embs[b, :n] = cond[g][r]
                embs[b, n:n + T] = self.embed_tokens(ids[None])[0]
                mask[b, :n + T] = 1
                targets[b, n:n + T] = ids if pad_id is None else ids.masked_fill(ids == pad_id, -100)
            logits = self.llama_model(inputs_embeds=embs, attention_mask=mask).logits.float()
            self.decode_stats["hf_score_forwards"] += 1
            V = logits.shape[-1]
            tok_loss = loss_fct(logits[:, :-1].reshape(-1, V), targets[:, 1:].reshape(-1))
            losses.append(tok_loss.view(B, -1).mean(1))
        return torch.stack(losses, dim=1)

    def _native_losses(self, img_embeds, prompts, answers):
        """score="hip": [B, C] losses from one native prefill and one native scoring pass, or None where the call is not the native
        path's (off the device, per-row texts or candidates without ragged="hip", more rows / candidates / tokens than the engine
        takes, an answer token equal to the pad id, which the reference masks out)."""
        B = img_embeds.shape[0]
        hip = self._hip
        if not img_embeds.is_cuda:
            return None
        shared = len(set(prompts)) == 1 and all(len(set(a)) == 1 for a in answers)
        if not shared or self.prompt_bucket:
            return self._native_losses_ragged(img_embeds, prompts, answers) if self.ragged == "hip" else None
        toks = [self._answer_tokens(a[0]) for a in answers]
        lens = [int(t.numel()) for t in toks]
        pad_id = getattr(self.llama_tokenizer, "pad_token_id", None)
        embs = self._prompt_embeds(prompts[0], img_embeds).contiguous()
        L, Tmax = int(embs.shape[1]), max(lens)
        if (B > self.max_batch or len(toks) > hip.MAX_CANDS or sum(t - 1 for t in lens) > hip.MAX_TAIL or L + Tmax - 1 > hip.MAX_LEN
                or (pad_id is not None and any(bool((t == pad_id).any()) for t in toks))):
            return None
        table = torch.zeros((len(toks), Tmax), dtype=torch.long)
        for c, t in enumerate(toks):
            table[c, :lens[c]] = t
        k_bufs, v_bufs = self._kv_buffers(embs, B, L)                   # the prompt's rows only: scoring appends nothing
        first = hip.prefill(embs, k_bufs, v_bufs)
        sums = hip.score(first, L, table.to(embs.device), lens, self.label_smoothing, k_bufs, v_bufs)
        self.decode_stats["hip_prefills"] += 1
        self.decode_stats["hip_scores"] += 1
        if self.activations == "int8":                                  # the losses are read next: the same sync
            self.last_act_stats()
        # the reference runs one forward per candidate, so each candidate's divisor is its own sequence length - 1
        return sums / torch.tensor([float(L + t - 1) for t in lens], device=sums.device)

    def _native_losses_ragged(self, img_embeds, prompts, answers):
        """ragged="hip", score="hip": per-row prompts and per-row candidates on the engine -- the prompts left-padded as the reference
        pads them for `generate` (prompt_bucket honoured), one ragged prefill, one ragged scoring pass (cgpt_llm_score_ragged) on the
        table `pack_row_candidates` builds.  None under `_native_losses`' rules."""
        B = img_embeds.shape[0]
        hip = self._hip
        texts = {a: self._answer_tokens(a) for cand in answers for a in set(cand)}     # every distinct answer tokenised once
        pad_id = getattr(self.llama_tokenizer, "pad_token_id", None)
        if pad_id is not None and any(bool((t == pad_id).any()) for t in texts.values()):
            return None
        table, row_lens, T, S = pack_row_candidates([[texts[a] for a in cand] for cand in answers])
        groups = {}                                                    # distinct prompt -> its rows, in first-seen order
        for b, p in enumerate(prompts):
            groups.setdefault(p, []).append(b)
        order = [b for rows in groups.values() for b in rows]
        batch_embs = [self._prompt_embeds(p, img_embeds[rows]) for p, rows in groups.items()]
        Lmax = max(int(e.shape[1]) for e in batch_embs)                # the longest prompt, bos included: the reference's padded length
        Lpad = -(-Lmax // self.prompt_bucket) * self.prompt_bucket if self.prompt_bucket else Lmax
        if B > self.max_batch or len(T) > hip.MAX_CANDS or S > hip.MAX_TAIL or Lpad + max(T) - 1 > hip.MAX_LEN:
            return None
        embs, _, starts = left_pad_embeds(batch_embs, self.prompt_bucket)
        if order != list(range(B)):                                    # left_pad_embeds stacks the groups: back to the call's row order
            inv = torch.empty(B, dtype=torch.long)
            inv[torch.tensor(order)] = torch.arange(B)
            inv = inv.to(embs.device)
            embs, starts = embs[inv].contiguous(), starts[inv].contiguous()
        L = int(embs.shape[1])
        k_bufs, v_bufs = self._kv_buffers(embs, B, L)
        first = hip.prefill(embs, k_bufs, v_bufs, starts=starts)
        sums = hip.score(first, L, table.to(embs.device), T, self.label_smoothing, k_bufs, v_bufs, starts=starts,
                         row_lens=row_lens.to(embs.device))
        self.decode_stats["hip_prefills"] += 1
        self.decode_stats["hip_ragged_scores"] += 1
        if self.activations == "int8":                                  # the losses are read next: the same sync
            self.last_act_stats()
        # the reference pads prompts and answers on the right and runs one forward per candidate: candidate c's divisor is the longest
        # prompt + the longest answer c over the rows - 1, for every row (answer_losses_from_embeds' docstring)
        return sums / torch.tensor([float(Lmax + t - 1) for t in T], device=sums.device)

    @torch.no_grad()
    def multi_select(self, images, texts, answers, num_cand=None):
        """`MiniGPTBase.multi_select(images, texts, answers, num_cand=None)` (minigpt_base.py:451-467): candidate ranks per row, best
        first -- `argsort` of the [B, C] answer losses (see `answer_losses_from_embeds` for the loss law), entries at or after
        `num_cand[i]` set to 9999 first."""
        img_embeds, _ = self.encoder.encode_img(images)
        losses = self.answer_losses_from_embeds(img_embeds, texts, answers)
        if num_cand is not None:
            for i in range(losses.shape[0]):
                losses[i, int(num_cand[i]):] = 9999
        return torch.argsort(losses, dim=-1).tolist()

    # ---- base classifier: [B,3,H,W] -> [B,num_classes] one-hot logits (smoothing.py:21,97)
    def _logits(self, answers, device):
        self.last_answers = answers
        return self.label_map.one_hot_logits(answers, device)

    def _classify_embeds(self, emb, device, draws=None):
        """One classifier batch from encode_img's output -> (logits [B, num_classes] on `device`, the rows' answer texts).
        classify="generate": one-hot of the generated answer's class.  classify="multi_select": -loss of candidate i in column i,
        -inf in column `other_id` (and in unused columns), so the top class is always a candidate.  classify="constrained": one-hot
        of the candidate the row spelled."""
        if self.classify == "generate":
            # the keyword travels only where it says something (sample = "hip"): subclasses that replace generate_from_embeds keep working
            kw = {"draws": draws} if draws is not None and self.sample == "hip" else {}
            answers = self.generate_from_embeds(emb, self.prompt, **kw)
            return self.label_map.one_hot_logits(answers, device), answers
        if self.classify == "constrained":
            labels, _ = self.constrained_from_embeds(emb, self.prompt)
            if self.constrain == "hip" and self.activations == "int8":  # the labels are read next: the same sync
                self.last_act_stats()
            return torch.nn.functional.one_hot(labels.long(), self.num_classes).float().to(device), self._label_texts(labels)
        losses = self.answer_losses_from_embeds(emb, self.prompt, self.candidates)
        logits = torch.full((losses.shape[0], self.num_classes), float("-inf"), dtype=torch.float32, device=losses.device)
        logits[:, :losses.shape[1]] = -losses
        answers = [self.candidates[i] for i in losses.argmin(dim=1).tolist()]
        return logits.to(device), answers

    def _label_texts(self, labels):
        """The candidates' texts of device labels (ONE host read)."""
        return [self.candidates[i] for i in labels.tolist()]

    def _constrained_counts(self, x, ranges, batch_size, sigma, seed, law):
        """constrain = "hip": the draws of `ranges` = [(first index, count, counts row), ...] -- contiguous index ranges -- in common
        classifier batches.  Per batch: encode_img_noisy -> graph replay -> vote_labels on the device labels; nothing is read back
        until the last batch is enqueued, then ONE host read of the kept labels fills `last_answers`."""
        bs = max(1, min(int(batch_size), self.max_batch))
        first, total, done, kept = ranges[0][0], sum(n for _, n, _ in ranges), 0, []
        while done < total:
            nb = min(bs, total - done)
            emb = self._encode_noisy(x, first + done, nb, sigma, seed, law)
            labels, _ = self.constrained_from_embeds(emb, self.prompt)
            lo, at = 0, 0                                              # rows of this batch, range by range
            for _, n, counts in ranges:
                hi = max(lo, min(nb, at + n - done))
                if hi > lo:
                    vote_labels(labels[lo:hi], counts)
                lo, at = hi, at + n
            kept.append(labels)
            done += nb
        if self.activations == "int8":                                  # the labels are read next: the same sync
            self.last_act_stats()
        self.last_answers = self._label_texts(torch.cat(kept)) if kept else []

    def __call__(self, images):
        out = []
        for lo in range(0, images.shape[0], self.max_batch):
            if self.classify == "generate":
                out.append(self._logits(self.generate(images[lo:lo + self.max_batch], self.prompt), images.device))
                continue
            emb, _ = self.encoder.encode_img(images[lo:lo + self.max_batch])
            logits, self.last_answers = self._classify_embeds(emb, images.device)
            out.append(logits)
        return torch.cat(out)

    def sample_counts_pair(self, x, first_a, num_a, first_b, num_b, batch_size, sigma, seed, law="gaussian"):
        """Selection + estimation draws of one `certify` (smoothing.py:44,48) in the same classifier batches: [2, num_classes] int64,
        identical to two `sample_counts` calls (a row's answer does not depend on its batch: tested)."""
        counts = torch.zeros((2, self.num_classes), dtype=torch.int64, device=x.device)
        if first_b != first_a + num_a:                                 # not one contiguous index range: two passes
            self.sample_counts(x, first_a, num_a, batch_size, sigma, seed, counts[0], law=law)
            self.sample_counts(x, first_b, num_b, batch_size, sigma, seed, counts[1], law=law)
            return counts
        if self.classify == "constrained" and self.constrain == "hip":
            self._constrained_counts(x, [(first_a, num_a, counts[0]), (first_b, num_b, counts[1])], batch_size, sigma, seed, law)
            return counts
        bs = max(1, min(int(batch_size), self.max_batch))
        total, done, answers = num_a + num_b, 0, []
        while done < total:
            nb = min(bs, total - done)
            emb = self._encode_noisy(x, first_a + done, nb, sigma, seed, law)
            logits, batch_answers = self._classify_embeds(emb, x.device, draws=(first_a + done, seed))
            na = max(0, min(nb, num_a - done))                         # rows of this batch that belong to the selection range
            if na > 0:
                vote(logits[:na], counts[0])
            if nb - na > 0:
                vote(logits[na:], counts[1])
            answers += batch_answers
            done += nb
        self.last_answers = answers
        return counts

    # ---- the `_sample_noise` engine (smoothing.py:81-99): noise fused into encode_img, vote in HIP
    def _encode_noisy(self, x, first, num, sigma, seed, law):
        # the law keyword reaches the encoder only when it is not the default: Gaussian-only encoders keep working
        kw = {} if law == "gaussian" else {"law": law}
        return self.encoder.encode_img_noisy(x, first, num, float(sigma), int(seed), **kw)

    def sample_counts(self, x, first_sample, num, batch_size, sigma, seed, counts=None, law="gaussian"):
        if counts is None:
            counts = torch.zeros(self.num_classes, dtype=torch.int64, device=x.device)
        if self.classify == "constrained" and self.constrain == "hip":
            self._constrained_counts(x, [(first_sample, num, counts)], batch_size, sigma, seed, law)
            return counts
        bs = max(1, min(int(batch_size), self.max_batch))
        done = 0
        while done < num:
            nb = min(bs, num - done)
            emb = self._encode_noisy(x, first_sample + done, nb, sigma, seed, law)
            logits, self.last_answers = self._classify_embeds(emb, x.device, draws=(first_sample + done, seed))
            vote(logits, counts)
            done += nb
        return counts
