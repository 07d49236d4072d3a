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
"""
import torch

from .classifier import vote

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


MAX_STOP_SEQS, MAX_STOP_LEN = 8, 8                                    # MAX_STOP, MAX_STOP_LEN of csrc/llm.hip


def _as_rows(table):
    return [[int(t) for t in row] for row in (table.tolist() if hasattr(table, "tolist") else table)]


def stop_finish_columns(tokens, eos_ids, stop_seqs):
    """The finishing rule of the greedy decode, stated once: for a [B, n] table of GENERATED tokens (tensor or
    nested lists) the first column i at which each row finishes -- token i is an EOS id, or tokens i-len+1 .. i equal a stop sequence
    of length len <= i + 1 (the prompt is embeddings and has no ids, so a longer sequence cannot match at select i).  len(row) for a
    row that never finishes.  min_length masks EOS logits, as in HF; it never suppresses a match."""
    eos = set(int(e) for e in (eos_ids.tolist() if hasattr(eos_ids, "tolist") else eos_ids))
    seqs = [s for s in _as_rows(stop_seqs if stop_seqs is not None else [])]
    cols = []
    for row in _as_rows(tokens):
        first = len(row)
        for i, t in enumerate(row):
            if t in eos or any(len(s) <= i + 1 and row[i + 1 - len(s):i + 1] == s for s in seqs):
                first = i
                break
        cols.append(first)
    return cols


def apply_stop_sequences(tokens, eos_ids, stop_seqs, pad):
    """`tokens` with every column after a row's finishing column (`stop_finish_columns`) replaced by `pad`; the finishing tokens
    stay, as HF keeps them.  Greedy rows are independent, so this applied to a decode WITHOUT stop sequences is, bit for bit, the
    decode with them.  A tensor gives a new tensor, nested lists a new list."""
    cols = stop_finish_columns(tokens, eos_ids, stop_seqs)
    if hasattr(tokens, "clone"):
        out = tokens.clone()
        for b, f in enumerate(cols):
            out[b, f + 1:] = int(pad)
        return out
    return [row[:f + 1] + [int(pad)] * (len(row) - f - 1) for row, f in zip(_as_rows(tokens), cols)]


# ---- the sampling law of sample="hip" (csrc/llm_sample.hip; include/cgpt.h: "Sampled decoding"), stated once: the oracle
PHILOX_WORD_SAMPLE = 3                                                # counter word 1 of the sampled decode's stream (csrc/philox.h)
SAMPLE_FIELDS = ("do_sample", "temperature", "top_k", "top_p", "repetition_penalty")
SAMPLE_HF_DEFAULTS = {"do_sample": False, "temperature": 1.0, "top_k": 50, "top_p": 1.0, "repetition_penalty": 1.0}   # GenerationConfig's


def _philox4x32_10(counter, key):
    c0, c1, c2, c3 = (int(c) & 0xFFFFFFFF for c in counter)
    k0, k1 = (int(k) & 0xFFFFFFFF for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def sample_uniform(seed, draw_id, step):
    """The uniform of draw `draw_id` at select `step` under `seed`: word 0 of Philox4x32-10(counter = (step, 3, id_lo, id_hi), key =
    (seed_lo, seed_hi)), its top 24 bits times 2^-24 -- in [0, 1), exact in fp32, a function of the three numbers alone."""
    seed, draw_id = int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw_id) & 0xFFFFFFFFFFFFFFFF
    word = _philox4x32_10((int(step), PHILOX_WORD_SAMPLE, draw_id & 0xFFFFFFFF, draw_id >> 32), (seed & 0xFFFFFFFF, seed >> 32))[0]
    return (word >> 8) * 2.0 ** -24


def sample_token_law(logits, prev_tokens, u, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, mask_eos_ids=(),
                     do_sample=True, dtype=torch.float64, details=False):
    """One sampled select on one logits row [V], in HF's processor order, evaluated in `dtype` (float64: the oracle of the kernel):
      1. the columns `mask_eos_ids` read as -inf;  2. every DISTINCT id of `prev_tokens` (the row's generated tokens so far) is
      penalised once, l > 0 ? l / pen : l * pen;  3. l / temperature;  4. top_k: keep l >= the k-th largest value (0 or >= V: off);
      5. softmax over what is kept;  6. top_p < 1: n = the smallest count whose descending cumulative mass is >= top_p, keep
      p >= p_(n);  7. the token is the first kept column, in index order, whose cumulative kept mass exceeds u * kept_mass.
    Both cuts keep the WHOLE group of equal values at their boundary (HF splits it by torch.sort's tie order), so the law does not
    depend on the order of the columns; a column at -inf is never kept.  do_sample=False: steps 1-2, then the first maximum.
    Returns (token, kept) -- kept a bool [V] -- or, with details=True, a dict with token, kept, p (the step-5 probabilities),
    kept_mass and, for the top-p cut, sorted_p / cum (the descending probabilities and their cumulative masses) and n (None without
    a cut)."""
    l = torch.as_tensor(logits).detach().cpu().to(dtype).clone().reshape(-1)
    V = l.numel()
    for e in mask_eos_ids:
        if 0 <= int(e) < V:
            l[int(e)] = float("-inf")
    pen = torch.tensor(float(repetition_penalty), dtype=dtype)
    if float(repetition_penalty) != 1.0:
        for t in sorted(set(int(t) for t in (prev_tokens.tolist() if hasattr(prev_tokens, "tolist") else prev_tokens))):
            if 0 <= t < V:
                l[t] = l[t] / pen if l[t] > 0 else l[t] * pen
    if not do_sample:
        token = int(torch.nonzero(l == l.max())[0])                            # the first maximum
        kept = torch.zeros(V, dtype=torch.bool)
        kept[token] = True
        if details:
            return {"token": token, "kept": kept, "p": kept.to(dtype), "kept_mass": 1.0, "sorted_p": None, "cum": None, "n": None}
        return token, kept
    l = l / torch.tensor(float(temperature), dtype=dtype)
    kept = l > float("-inf")
    if 0 < int(top_k) < V:
        kept &= l >= torch.sort(l, descending=True).values[int(top_k) - 1]
    w = torch.where(kept, torch.exp(l - l.max()), torch.zeros((), dtype=dtype))
    p = w / w.sum()
    srt = cum = n = None
    if float(top_p) < 1.0:
        srt = torch.sort(p, descending=True).values
        cum = torch.cumsum(srt, dim=0)
        hit = torch.nonzero(cum >= torch.tensor(float(top_p), dtype=dtype))
        n = int(hit[0]) + 1 if hit.numel() else int(kept.sum())
        kept &= p >= srt[n - 1]
    pk = torch.where(kept, p, torch.zeros((), dtype=dtype))
    cdf = torch.cumsum(pk, dim=0)
    mass = pk.sum()
    over = torch.nonzero(kept & (cdf > torch.tensor(float(u), dtype=dtype) * mass))
    token = int(over[0]) if over.numel() else int(torch.nonzero(kept)[-1])
    if details:
        return {"token": token, "kept": kept, "p": p, "kept_mass": float(mass), "sorted_p": srt, "cum": cum, "n": n}
    return token, kept


def check_sample_settings(settings):
    """(do_sample, temperature, top_k, top_p, repetition_penalty) as the native sampler takes them; ValueError naming the field for
    temperature <= 0, top_p outside (0, 1], top_k < 0 or repetition_penalty <= 0 (what cgpt_llm_sample refuses)."""
    do_sample, temperature, top_k, top_p, pen = settings
    if not isinstance(do_sample, (bool, int)):
        raise ValueError(f"do_sample={do_sample!r}: expected False or True")
    if not float(temperature) > 0 or float(temperature) == float("inf"):
        raise ValueError(f"temperature={temperature!r}: expected a finite value > 0")
    if isinstance(top_k, bool) or int(top_k) != top_k or int(top_k) < 0:
        raise ValueError(f"top_k={top_k!r}: expected an int >= 0 (0: off)")
    if not 0.0 < float(top_p) <= 1.0:
        raise ValueError(f"top_p={top_p!r}: expected a value in (0, 1]")
    if not float(pen) > 0 or float(pen) == float("inf"):
        raise ValueError(f"repetition_penalty={pen!r}: expected a finite value > 0")
    return bool(do_sample), float(temperature), int(top_k), float(top_p), float(pen)


def check_stop_words_ids(stop_words_ids):
    """The `stop_words_ids` keyword (the reference's name, minigpt_base.py:387) -> a tuple of token-id tuples: a list of token-id
    lists (or 1-d tensors, as conversation.py builds them), an int entry read as a one-token sequence, as the reference's `[2]` is.
    None -> ().  ValueError naming the offending entry for more than 8 sequences, a sequence outside 1..8 tokens or a negative id."""
    if stop_words_ids is None:
        return ()
    if isinstance(stop_words_ids, (str, bytes)) or not hasattr(stop_words_ids, "__iter__"):
        raise ValueError(f"stop_words_ids={stop_words_ids!r}: expected None or a list of token-id lists (a text goes to stop_text)")
    entries = stop_words_ids.tolist() if hasattr(stop_words_ids, "tolist") else list(stop_words_ids)
    if len(entries) > MAX_STOP_SEQS:
        raise ValueError(f"stop_words_ids: {len(entries)} sequences (at most {MAX_STOP_SEQS})")
    out = []
    for k, entry in enumerate(entries):
        entry = entry.tolist() if hasattr(entry, "tolist") else entry
        ids = [entry] if isinstance(entry, int) and not isinstance(entry, bool) else entry
        if isinstance(ids, (str, bytes)) or not isinstance(ids, (list, tuple)) or \
                any(isinstance(t, bool) or not isinstance(t, int) for t in ids):
            raise ValueError(f"stop_words_ids[{k}]={entry!r}: expected a list of token ids or one token id")
        if not 1 <= len(ids) <= MAX_STOP_LEN:
            raise ValueError(f"stop_words_ids[{k}]={entry!r}: {len(ids)} tokens (a sequence has 1..{MAX_STOP_LEN})")
        if min(ids) < 0:
            raise ValueError(f"stop_words_ids[{k}]={entry!r}: a negative token id")
        out.append(tuple(ids))
    return tuple(out)


def stop_sequences_criteria(stop_seqs):
    """The rule as a transformers StoppingCriteria for the HF path: a bool [B] per step, True for the rows whose generated tokens end
    in a sequence; `generate` marks such rows finished and pads them, as it does for an EOS.  With `inputs_embeds` and no input ids
    the ids `generate` hands over are the generated tokens only, which is what the rule compares."""
    from transformers import StoppingCriteria, StoppingCriteriaList

    class StopSequences(StoppingCriteria):
        def __init__(self, seqs):
            self.seqs = [list(s) for s in seqs]

        def __call__(self, input_ids, scores, **kwargs):
            done = torch.zeros(input_ids.shape[0], dtype=torch.bool, device=input_ids.device)
            for s in self.seqs:
                if len(s) <= input_ids.shape[1]:
                    want = torch.tensor(s, dtype=input_ids.dtype, device=input_ids.device)
                    done = done | (input_ids[:, input_ids.shape[1] - len(s):] == want).all(dim=1)
            return done

    return StoppingCriteriaList([StopSequences(stop_seqs)])


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


def left_pad_embeds(batch_embs, bucket=None):
    """Left padding of prompts of different lengths (minigpt_base.py:407-416): `batch_embs` is a list of tensors [n_i, len_i, hidden]
    (n_i rows that share one length; the reference's loop has n_i = 1) -> (embeds [B, L, hidden] with zeros on the pad positions,
    attention mask [B, L] int, starts [B] int32 = pad positions per row), B = sum n_i, L = the longest length, rounded up to a
    multiple of `bucket` when that is set.  Row b's real tokens sit at positions starts[b] .. L-1.  Pure tensor arithmetic on the
    inputs' device (CPU tensors work); a row with no real token is a ValueError."""
    if bucket is not None and (isinstance(bucket, bool) or not isinstance(bucket, int) or bucket < 1):
        raise ValueError(f"bucket={bucket!r}: expected None or an int >= 1")
    if not batch_embs:
        raise ValueError("left_pad_embeds: no rows")
    lens = [int(e.shape[1]) for e in batch_embs]
    if min(lens) < 1:
        raise ValueError(f"left_pad_embeds: row group {lens.index(min(lens))} has no real token (length 0)")
    L = max(lens)
    if bucket:
        L = (L + bucket - 1) // bucket * bucket
    first = batch_embs[0]
    B = sum(int(e.shape[0]) for e in batch_embs)
    embs = torch.zeros([B, L, first.shape[2]], dtype=first.dtype, device=first.device)
    attn_mask = torch.zeros([B, L], dtype=torch.int, device=first.device)
    starts = torch.empty([B], dtype=torch.int32, device=first.device)
    row = 0
    for emb, n in zip(batch_embs, lens):
        rows = int(emb.shape[0])
        embs[row:row + rows, L - n:] = emb
        attn_mask[row:row + rows, L - n:] = 1
        starts[row:row + rows] = L - n
        row += rows
    return embs, attn_mask, starts


def pack_row_candidates(cand_tokens):
    """Per-row candidates for the native scoring pass (cgpt_llm_score_ragged): `cand_tokens[c][b]` = the token ids (a sequence of
    ints or a 1-D tensor, at least one) of candidate c for row b -> (table [B, C, Tmax] int64 with zeros behind each real length,
    lens [B, C] int32 = the real lengths, T = [T_c] = the longest length of candidate c over the rows (a list of ints), S = the
    tail slots per row, sum of T_c - 1: a one-token candidate owns none).  Pure CPU arithmetic; the engine's limits (S <= 64,
    C <= 64) are the caller's to compare against.  A candidate without a token, or rows that disagree in number, are a ValueError."""
    if not cand_tokens:
        raise ValueError("pack_row_candidates: no candidate")
    rows = [[[int(v) for v in (ids.tolist() if hasattr(ids, "tolist") else ids)] for ids in cand] for cand in cand_tokens]
    B = len(rows[0])
    if B < 1 or any(len(cand) != B for cand in rows):
        raise ValueError("pack_row_candidates: cand_tokens[c][b] needs one token list per candidate and row, at least one row")
    for c, cand in enumerate(rows):
        for b, ids in enumerate(cand):
            if not ids:
                raise ValueError(f"pack_row_candidates: candidate {c} of row {b} has no token")
    T = [max(len(ids) for ids in cand) for cand in rows]
    table = torch.zeros((B, len(rows), max(T)), dtype=torch.long)
    lens = torch.empty((B, len(rows)), dtype=torch.int32)
    for c, cand in enumerate(rows):
        for b, ids in enumerate(cand):
            table[b, c, :len(ids)] = torch.tensor(ids, dtype=torch.long)
            lens[b, c] = len(ids)
    return table, lens, T, sum(t - 1 for t in T)


def greedy_decode_parity(hf_tokens, hf_scores, tokens, eps):
    """Compare a greedy decode `tokens` [B, n] with HF `generate`'s `hf_tokens` [B, <= n] row by row, given HF's per-step processed
    scores `hf_scores` [B, steps, V] (fp32).  Two greedy decoders of the SAME fp16 model can only part ways at a step where HF's own
    top-2 margin is within the logit noise of the two paths (another GEMM / attention kernel rounds the fp16 logits differently), after
    which the contexts differ and nothing more can be said about that row.  Returns a dict: `identical` rows, `decisive` rows (every
    step's margin > eps: these MUST be identical), `violations` = rows whose first divergence sits at a step with margin > eps."""
    B = hf_tokens.shape[0]
    S = min(hf_tokens.shape[1], tokens.shape[1], hf_scores.shape[1])
    top2 = hf_scores[:, :S].float().topk(2, dim=-1).values
    margin = top2[..., 0] - top2[..., 1]                                  # [B, S]; inf where only one candidate is finite
    margin = torch.nan_to_num(margin, nan=float("inf"))
    neq = tokens[:, :S] != hf_tokens[:, :S]
    diverged = neq.any(dim=1)
    first = torch.where(diverged, neq.float().argmax(dim=1), torch.zeros(B, dtype=torch.long, device=neq.device))
    m_at = margin.gather(1, first[:, None])[:, 0]
    violations = (diverged & (m_at > eps)).nonzero().flatten().tolist()
    decisive = (margin > eps).all(dim=1)
    return {"identical": int((~diverged).sum()), "diverged": int(diverged.sum()), "decisive": int(decisive.sum()),
            "decisive_identical": int((decisive & ~diverged).sum()), "violations": violations,
            "max_margin_at_divergence": float(m_at[diverged].max()) if bool(diverged.any()) else 0.0}


def fp16_ulp(x):
    """Spacing of fp16 at magnitude x (normal range)."""
    import math
    return 2.0 ** (math.floor(math.log2(max(float(x), 6.2e-5))) - 10)


# ---- the weight law of weights="int8" (csrc/llm.hip: llm_quant_rows_kernel; include/cgpt.h: CGPT_LLM_W_INT8), in plain torch
LAYER_LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
                 "mlp.down_proj")


def quantize_rows_int8(w):
    """Row-wise absmax int8 of an fp16 `nn.Linear.weight` [N, K] -> (q int8 [N, K], s fp16 [N]):
        s_n  = fp16(absmax_k |w_nk| / 127)                     the division in fp32, then one rounding to fp16
        q_nk = clamp(rint(fp32(w_nk) / fp32(s_n)), -127, 127)  fp32 division, round to nearest even; q = 0 where s_n = 0
    (a zero row, or an absmax so small that absmax / 127 underflows fp16).  Works on CPU tensors."""
    if w.dtype != torch.float16 or w.dim() != 2:
        raise ValueError(f"quantize_rows_int8: expected an fp16 matrix [N, K], got {w.dtype} {tuple(w.shape)}")
    s = (w.abs().amax(dim=1).float() / 127.0).to(torch.float16)
    sf = s.float()[:, None]
    live = sf != 0
    q = torch.round(w.float() / torch.where(live, sf, torch.ones_like(sf))).clamp_(-127, 127)
    return torch.where(live, q, torch.zeros_like(q)).to(torch.int8), s


def dequantize_rows_int8(q, s):
    """W'_nk = fp16(q_nk) * s_n as ONE fp16 multiply (q is exact in fp16): what an int8 handle multiplies by."""
    if q.dtype != torch.int8 or s.dtype != torch.float16 or q.dim() != 2 or tuple(s.shape) != (q.shape[0],):
        raise ValueError("dequantize_rows_int8: expected q int8 [N, K] and s fp16 [N]")
    return q.to(torch.float16) * s[:, None]


def int8_state_dict(llama_model, device=None):
    """The state dict of `llama_model` with the seven linears of every layer replaced by W' = dequantize(quantize(W)); everything else
    (embed_tokens, lm_head, the RMSNorm weights) as it is.  Loadable into an HF twin of the model: by the definition of
    weights="int8" the native engine on `llama_model` computes, bit for bit, what the fp16 native engine computes on that twin.
    device: where the law is evaluated (default: where each weight lives; "cpu" for the reference evaluation); the results go back to
    the weight's own device."""
    out = {}
    for name, w in llama_model.state_dict().items():
        if name.startswith("model.layers.") and name.endswith(".weight") and name.split(".", 3)[3][:-len(".weight")] in LAYER_LINEARS:
            src = w.detach().to(device or w.device)
            out[name] = dequantize_rows_int8(*quantize_rows_int8(src)).to(w.device)
        else:
            out[name] = w.detach().clone()
    return out


# ---- the activation law of activations="int8" (csrc/llm_gemm_i8.hip; include/cgpt.h: cgpt_llm_config_act), in plain torch: the oracle
def quantize_act_rows_int8(x, threshold=6.0):
    """Row-wise int8 codes of fp16 activations x [M, K] with a per-row outlier split -> (a int8 [M, K], s_a fp32 [M], outlier bool [M, K]):
        outlier_mk = threshold > 0 and |x_mk| >= threshold
        s_a[m]     = max over the row's non-outliers |x_mk| / 127        fp32 division; kept in fp32
        a_mk       = clamp(rint(fp32(x_mk) / s_a[m]), -127, 127)          round to nearest even; 0 for outliers; the row 0 where s_a = 0
    Every row is a function of that row alone.  Works on CPU tensors."""
    if x.dtype != torch.float16 or x.dim() != 2:
        raise ValueError(f"quantize_act_rows_int8: expected an fp16 matrix [M, K], got {x.dtype} {tuple(x.shape)}")
    xf = x.float()
    t = float(threshold)
    out = (xf.abs() >= t) if t > 0 else torch.zeros_like(xf, dtype=torch.bool)
    amax = torch.where(out, torch.zeros_like(xf), xf.abs()).amax(dim=1)
    s = amax / torch.full_like(amax, 127.0)                            # tensor / tensor: a true division on every device
    sf = s[:, None]
    live = (sf != 0) & ~out
    a = torch.round(xf / torch.where(sf != 0, sf, torch.ones_like(sf))).clamp_(-127, 127)
    return torch.where(live, a, torch.zeros_like(a)).to(torch.int8), s, out


def llm_int8_linear(x, q, s_w, threshold=6.0):
    """The linear of an activations-int8 handle on fp16 rows x [M, K] against int8 weights q [N, K] with fp16 row scales s_w [N]
    (`quantize_rows_int8`) -> v fp32 [M, N], before the epilogue's rounding:
        acc = a . q^T in integers (exact);   y = fp32(acc) * (s_a * fp32(s_w));
        o   = sum over the row's outliers in ascending k of fp32(x_k) * fp32(W'_nk), sequential fp32 from 0, W' = fp16(q) * s_w;
        v   = y + o.
    Plain torch on the tensors' device; the integer product runs in int64 on the CPU and in fp64 elsewhere (|acc| < 2^31: exact)."""
    if q.dtype != torch.int8 or s_w.dtype != torch.float16 or q.dim() != 2 or tuple(s_w.shape) != (q.shape[0],) or x.shape[-1] != q.shape[1]:
        raise ValueError("llm_int8_linear: expected x fp16 [M, K], q int8 [N, K] and s_w fp16 [N]")
    a, s_a, out = quantize_act_rows_int8(x, threshold)
    if x.is_cuda:
        acc = (a.double() @ q.double().t()).to(torch.int32)
    else:
        acc = (a.long() @ q.long().t()).to(torch.int32)
    y = acc.to(torch.float32) * (s_a[:, None] * s_w.float()[None, :])
    o = torch.zeros_like(y)
    cnt = out.sum(dim=1)
    most = int(cnt.max()) if out.numel() else 0
    if most:
        wp = dequantize_rows_int8(q, s_w).float()                      # [N, K]
        xf = x.float()
        # the j-th outlier of every row at once: a stable sort lists a row's outlier positions first, in ascending k
        order = torch.sort(out.to(torch.uint8), dim=1, descending=True, stable=True).indices[:, :most]
        for j in range(most):                                          # sequential fp32, ascending k; every product is exact in fp32
            kj = order[:, j]
            term = xf.gather(1, kj[:, None]) * wp[:, kj].t()
            o = torch.where((cnt > j)[:, None], o + term, o)
    return y + o


class _ActInt8Linear(torch.nn.Module):
    """A bias-free linear evaluated by the activation law: input cast to fp16, `llm_int8_linear`, fp16 of v, in the input's dtype."""

    def __init__(self, weight, threshold):
        super().__init__()
        q, s = quantize_rows_int8(weight.detach().to(torch.float16).cpu())      # the weight law's reference evaluation (as int8_state_dict's)
        self.register_buffer("q", q.to(weight.device), persistent=False)
        self.register_buffer("s_w", s.to(weight.device), persistent=False)
        self.weight = weight                                            # the parameter stays: the state dict is unchanged
        self.threshold = float(threshold)
        self.in_features, self.out_features, self.bias = weight.shape[1], weight.shape[0], None

    def forward(self, x):
        x2 = x.reshape(-1, x.shape[-1]).to(torch.float16)
        v = llm_int8_linear(x2, self.q, self.s_w, self.threshold).to(torch.float16)
        return v.to(x.dtype).reshape(*x.shape[:-1], self.out_features)


def act_int8_twin(llama_model, threshold=6.0):
    """A copy of an HF `LlamaForCausalLM` whose seven linears per layer evaluate the law of activations="int8" (`llm_int8_linear` on
    `quantize_rows_int8` of the fp16 weight, fp16 of the result): the oracle of the mode, in the role `int8_state_dict` and
    `expand_kv_state_dict` have.  Everything else (embed_tokens, lm_head, the norms, attention, every rounding of the model's dtype) is
    the copy's own, so an fp32 copy is the reference point and an fp16 copy is HF's fp16 evaluation of the same law.  The state dict
    is that of `llama_model`.  Works on CPU and GPU."""
    import copy
    twin = copy.deepcopy(llama_model)
    for layer in twin.model.layers:
        for name in LAYER_LINEARS:
            parent_name, attr = name.split(".")
            parent = getattr(layer, parent_name)
            lin = getattr(parent, attr)
            if lin.bias is not None:
                raise ValueError(f"act_int8_twin: {name} carries a bias (bias-free linears required)")
            setattr(parent, attr, _ActInt8Linear(lin.weight, threshold))
    return twin.eval()


GQA_RATIOS = (1, 2, 4, 8)                                              # heads / kv_heads the grouped kernels are instantiated for


def expand_kv_state_dict(llama_model):
    """The state dict of the multi-head twin of a grouped-query `llama_model`: every `k_proj` / `v_proj` weight [kv_heads * d, hidden]
    becomes [heads * d, hidden] with each head's block of d rows repeated G = heads / kv_heads times in `repeat_interleave` order
    (twin head h = K/V head h // G, which is HF's `repeat_kv`); everything else as it is.  Loadable into an HF model of the same
    config with `num_key_value_heads = num_attention_heads`, which then computes what the grouped model computes: the oracle of
    grouped_kv=True, in the role `int8_state_dict` has for weights="int8".  Plain torch; works on CPU tensors."""
    cfg = llama_model.config
    heads = int(cfg.num_attention_heads)
    kv = int(getattr(cfg, "num_key_value_heads", None) or heads)
    if kv < 1 or heads % kv:
        raise ValueError(f"expand_kv_state_dict: num_key_value_heads {kv} does not divide num_attention_heads {heads}")
    G = heads // kv
    out = {}
    for name, w in llama_model.state_dict().items():
        if name.endswith("self_attn.k_proj.weight") or name.endswith("self_attn.v_proj.weight"):
            d = w.shape[0] // kv
            out[name] = w.detach().view(kv, d, w.shape[1]).repeat_interleave(G, dim=0).reshape(heads * d, w.shape[1]).clone()
        else:
            out[name] = w.detach().clone()
    return out


class _LinearRoute:
    """Routes the bias-free fp16 `nn.Linear` layers of a frozen decoder through libcgpt's MFMA GEMM (`cgpt_linear_f16`, the kernel
    of the ViT's qkv / proj / MLP) for calls with at least `min_rows` rows, i.e. the PREFILL of a Monte-Carlo batch (200 rows x 44
    tokens = 8 800 rows); decode steps (one row per copy) stay with the vendor library.  One patch per module; the patch is inert
    outside `enabled()`, and the switch is a context variable (per thread / per task), so another thread or another classifier that
    calls the same shared decoder meanwhile is not routed.  Eligibility (fp16, contiguous, on the device, no bias, K in 64s, N in 256s)
    is re-checked at every call: after a `.to()`, a dtype change or a weight swap (a LoRA merge) the original forward runs."""
    import contextvars as _cv
    _active = _cv.ContextVar("cgpt_linear_route", default=False)

    @staticmethod
    def _eligible(m):
        w = m.weight
        return (m.bias is None and w.dtype == torch.float16 and w.is_cuda and w.is_contiguous()
                and w.shape == (m.out_features, m.in_features) and m.in_features % 64 == 0 and m.out_features % 256 == 0)

    @classmethod
    def install(cls, model, min_rows=1024):
        import ctypes as C
        from . import _lib
        L = _lib.lib()
        n = 0
        for m in model.modules():
            if not isinstance(m, torch.nn.Linear):
                continue
            if getattr(m, "_cgpt_routed", False):                       # patched by an earlier classifier on the same module
                n += 1
                continue
            if not cls._eligible(m):                                    # W must be readable for whole 256-row tiles, K in 64s
                continue
            orig = m.forward

            def fwd(x, m=m, orig=orig):
                rows = x.numel() // x.shape[-1] if x.shape[-1] else 0
                if (not cls._active.get() or rows < min_rows or x.dtype != torch.float16 or not x.is_cuda
                        or x.device != m.weight.device or not cls._eligible(m)):
                    return orig(x)
                K, N = m.in_features, m.out_features
                a = x.reshape(rows, K)
                if rows % 256 or not a.is_contiguous():                 # the kernel reads whole 256-row tiles: pad rows exist but are
                    pad = x.new_empty(((rows + 255) // 256 * 256, K))   # never stored from (their garbage stays in their own outputs)
                    pad[:rows].copy_(a)
                    a = pad
                out = x.new_empty((rows, N))
                st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                _lib.check(L.cgpt_linear_f16(C.c_void_p(a.data_ptr()), K, C.c_void_p(m.weight.data_ptr()), K, None,
                                             C.c_void_p(out.data_ptr()), N, None, N, rows, N, K, 0, st))
                return out.view(*x.shape[:-1], N)
            m.forward = fwd
            m._cgpt_routed = True
            n += 1
        return n

    @classmethod
    def enabled(cls):
        import contextlib

        @contextlib.contextmanager
        def ctx():
            token = cls._active.set(True)
            try:
                yield
            finally:
                cls._active.reset(token)
        return ctx()


def hip_decode_unsupported(llama_model, max_batch=None, grouped_kv=False, activations="fp16"):
    """Every property of `llama_model` (and of the classifier batch) that keeps it off the native token step (`decode="hip"`,
    csrc/llm.hip), as a list of sentences; empty = supported.  The step kernels are written for HF `LlamaForCausalLM` in fp16 on
    a HIP device: bias-free linears, RMSNorm, `rotate_half` rotary with the default (unscaled) rope_theta law, as many K/V heads
    as query heads, head size 128, SwiGLU, no sliding window -- Vicuna-7B / 13B.  ALL failing properties are collected, so one
    message names them all.
    grouped_kv=True (the engine's grouped-query mode): fewer K/V heads than query heads are accepted when they
    divide them and heads / kv_heads is 1, 2, 4 or 8 -- Llama-3-8B (32 / 8), Llama-2-70B's shape (64 / 8).
    activations="int8" (DESIGN.md 4.4.7): hidden_size and intermediate_size must be multiples of 128, because one K-tile of the int8
    kernel is 128 bytes -- 7B, 13B, Llama-3-8B and 70B all are."""
    cfg = getattr(llama_model, "config", None)
    bad = []
    if type(llama_model).__name__ != "LlamaForCausalLM" or cfg is None:
        return [f"architecture: {type(llama_model).__name__} (HF LlamaForCausalLM required)"]
    prm = next(llama_model.parameters())
    if not (prm.is_cuda and getattr(torch.version, "hip", None)):
        bad.append(f"device: {prm.device} (a HIP device is required)")
    dtypes = sorted({str(q.dtype) for q in llama_model.parameters()})
    if dtypes != ["torch.float16"]:
        bad.append(f"dtype: {', '.join(dtypes)} (torch.float16 required)")
    heads, hidden = int(cfg.num_attention_heads), int(cfg.hidden_size)
    head_dim = int(getattr(cfg, "head_dim", None) or hidden // heads)
    if head_dim != 128 or hidden != heads * 128:
        bad.append(f"head size: head_dim {head_dim} with hidden_size {hidden} / {heads} heads (head_dim 128 and hidden = heads x 128 required)")
    kv = int(getattr(cfg, "num_key_value_heads", None) or heads)
    if grouped_kv:
        if kv < 1 or heads % kv or heads // kv not in GQA_RATIOS:
            bad.append(f"K/V heads: num_key_value_heads {kv} with num_attention_heads {heads} (grouped_kv takes a count that divides "
                       f"the query heads with a ratio in {list(GQA_RATIOS)})")
    elif kv != heads:
        bad.append(f"K/V heads: num_key_value_heads {kv} != num_attention_heads {heads} (grouped-query attention is not supported)")
    with_bias = [n for n, m in llama_model.named_modules() if isinstance(m, torch.nn.Linear) and m.bias is not None]
    if getattr(cfg, "attention_bias", False) or getattr(cfg, "mlp_bias", False) or with_bias:
        bad.append(f"biases: {len(with_bias)} linear layers carry a bias (bias-free linears required)")
    rope = getattr(cfg, "rope_parameters", None) or getattr(cfg, "rope_scaling", None) or {}
    rope_type = rope.get("rope_type", rope.get("type", "default")) if isinstance(rope, dict) else str(rope)
    if rope_type != "default":
        bad.append(f"rotary law: rope type {rope_type!r} (only the default, unscaled rope_theta law is supported)")
    if getattr(cfg, "sliding_window", None):
        bad.append(f"sliding window: {cfg.sliding_window} (full attention required)")
    if getattr(cfg, "hidden_act", "silu") != "silu":
        bad.append(f"activation: {cfg.hidden_act} (SwiGLU with silu required)")
    for name, val in (("hidden_size", hidden), ("intermediate_size", int(cfg.intermediate_size)), ("vocab_size", int(cfg.vocab_size))):
        if val % 64:
            bad.append(f"shape: {name} {val} is not a multiple of 64")
    if activations == "int8":
        for name, val in (("hidden_size", hidden), ("intermediate_size", int(cfg.intermediate_size))):
            if val % 128:
                bad.append(f'shape: {name} {val} is not a multiple of 128 (activations="int8": one K-tile of the int8 kernel is 128 bytes)')
    if max_batch is not None and int(max_batch) > 256:
        bad.append(f"batch: max_batch {int(max_batch)} > 256 rows (one GEMM row tile)")
    eos = getattr(getattr(llama_model, "generation_config", None), "eos_token_id", None)      # as greedy_tokens resolves it
    eos = getattr(cfg, "eos_token_id", None) if eos is None else eos
    if isinstance(eos, (list, tuple)) and len(eos) > 8:
        bad.append(f"EOS ids: {len(eos)} end-of-sequence ids (the token select takes at most 8)")
    return bad


def _rope_theta(cfg):
    rope = getattr(cfg, "rope_parameters", None) or getattr(cfg, "rope_scaling", None) or {}
    theta = rope.get("rope_theta") if isinstance(rope, dict) else None
    return float(theta or getattr(cfg, "rope_theta", None) or 10000.0)


class _HipDecoder:
    """The native token step of a frozen LlamaForCausalLM (`cgpt_llm_*`, include/cgpt.h): validates the model, creates the handle
    and hands it the module's own fp16 parameters ONCE (the library keeps fused copies: 2 bytes per parameter more HBM, 13.5 GB at
    7B; a later change of the module's weights is not seen; with weights="int8" the seven linears of every layer are held as row-wise
    absmax int8 instead, quantised on the device at load, 7.2 GB at 7B -- see `quantize_rows_int8`).  `greedy` enqueues the whole loop after the prefill on the current
    stream -- no host sync, capturable -- on the K/V buffers the prefill filled, in place."""
    MAX_LEN = 4096                                                     # positions the rotary table covers (prompt + new tokens)

    def __init__(self, llama_model, max_batch, weights="fp16", early_stop=False, grouped_kv=False, activations="fp16", int8_threshold=6.0,
                 outlier_cap=64):
        import ctypes as C
        from . import _lib
        if weights not in _lib.LLM_WEIGHT_FORMATS:
            raise ValueError(f'weights={weights!r}: expected "fp16" or "int8"')
        if activations not in _lib.LLM_ACT_FORMATS:
            raise ValueError(f'activations={activations!r}: expected "fp16" or "int8"')
        if activations == "int8" and weights != "int8":
            raise ValueError('activations="int8" needs weights="int8": int8 activations multiply int8 weights')
        if activations == "int8" and not 1 <= int(outlier_cap) <= 1024:
            raise ValueError(f"outlier_cap={outlier_cap!r}: expected 1..1024")
        self.weights = weights
        self.activations, self.int8_threshold, self.outlier_cap = activations, float(int8_threshold), int(outlier_cap)
        self._act_stats = None
        self.early_stop = bool(early_stop)
        self._greedy_ran = False                                       # live_steps has nothing to report before the first `greedy`
        self.stop_sequences = ()                                       # none is the handle's state at create
        self.grouped_kv = bool(grouped_kv)
        bad = hip_decode_unsupported(llama_model, max_batch, grouped_kv=self.grouped_kv, activations=activations)
        if bad:
            raise ValueError('decode="hip" does not support this decoder -- ' + "; ".join(bad))
        self._C, self._lib_mod, self.L = C, _lib, _lib.lib()
        cfg = llama_model.config
        self.device = next(llama_model.parameters()).device
        self.layers, self.heads, self.vocab = int(cfg.num_hidden_layers), int(cfg.num_attention_heads), int(cfg.vocab_size)
        # K/V heads of the caches every entry works on: the model's own count under grouped_kv, the query heads otherwise
        self.kv_heads = int(getattr(cfg, "num_key_value_heads", None) or self.heads) if self.grouped_kv else self.heads
        self.max_batch = int(max_batch)
        # fp16 handles pass the config up to max_len, which every build of the library accepts (an A/B against an older build loads it
        # through CGPT_LIB_PATH); weight_format travels only when it says something
        # and so does grouped_kv: the extended struct (cgpt_llm_config_gqa) is sent only when the flag is set
        # and so does the activation format (cgpt_llm_config_act)
        size = (C.sizeof(_lib.LlmConfigAct) if activations != "fp16" else C.sizeof(_lib.LlmConfigGqa) if self.grouped_kv else
                C.sizeof(_lib.LlmConfig) if weights != "fp16" else _lib.LLM_CONFIG_SIZE_F16)
        c = _lib.LlmConfig(struct_size=size, weight_format=_lib.LLM_WEIGHT_FORMATS[weights], device=self.device.index or 0, hidden=int(cfg.hidden_size),
                           layers=self.layers, heads=self.heads, kv_heads=self.kv_heads, head_dim=128, mlp=int(cfg.intermediate_size),
                           vocab=self.vocab, rms_eps=float(cfg.rms_norm_eps), rope_theta=_rope_theta(cfg),
                           max_batch=self.max_batch, max_len=self.MAX_LEN)
        self.handle = C.c_void_p()
        ext = _lib.LlmConfigGqa(base=c, grouped_kv=int(self.grouped_kv), reserved=0)     # create reads past `base` only when the size says so
        act = _lib.LlmConfigAct(gqa=ext, act_format=_lib.LLM_ACT_FORMATS[activations], act_threshold=self.int8_threshold,
                                outlier_cap=self.outlier_cap, reserved2=0)
        _lib.check(self.L.cgpt_llm_create(C.byref(act.gqa.base), C.byref(self.handle)))
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        wanted = ["model.embed_tokens.weight", "model.norm.weight", "lm_head.weight"]
        for i in range(self.layers):
            wanted += [f"model.layers.{i}.self_attn.{n}_proj.weight" for n in "qkvo"]
            wanted += [f"model.layers.{i}.mlp.{n}_proj.weight" for n in ("gate", "up", "down")]
            wanted += [f"model.layers.{i}.{n}_layernorm.weight" for n in ("input", "post_attention")]
        sd = llama_model.state_dict()
        for name in wanted:
            w = sd[name].detach()
            assert w.dtype == torch.float16 and w.device == self.device, name
            w = w.contiguous()
            _lib.check(self.L.cgpt_llm_load_weight_f16(self.handle, name.encode(), C.c_void_p(w.data_ptr()), w.numel(), st))
        torch.cuda.current_stream(self.device).synchronize()           # contiguous() temporaries may go once the copies have run
        if self.early_stop:                                            # off is the handle's state at create: nothing is called for it
            _lib.check(self.L.cgpt_llm_set_early_stop(self.handle, 1))

    @property
    def weight_bytes(self):
        """Bytes the handle holds for weight matrices, row scales and the dequantisation scratch (cgpt_llm_weight_bytes: the
        library's own accounting).  None on a build of the library that predates the entry (CGPT_LIB_PATH A/B runs)."""
        C = self._C
        if not hasattr(self.L, "cgpt_llm_weight_bytes"):
            return None
        n = C.c_int64()
        self._lib_mod.check(self.L.cgpt_llm_weight_bytes(self.handle, C.byref(n)))
        return int(n.value)

    def act_stats(self):
        """{rows, outliers, max_outliers_per_row, overflow_rows} of the native calls since the last read (cgpt_llm_act_stats: one
        device sync; the counters are reset).  When nothing ran since, the last non-empty reading is returned again.  RuntimeError when
        a row had more outliers than `outlier_cap`: its result is not the law's."""
        C = self._C
        if self.activations != "int8":
            raise RuntimeError('act_stats: the engine was built with activations="fp16"')
        v = (C.c_int64 * 4)()
        self._lib_mod.check(self.L.cgpt_llm_act_stats(self.handle, v))
        if v[0] > 0 or self._act_stats is None:
            self._act_stats = {"rows": int(v[0]), "outliers": int(v[1]), "max_outliers_per_row": int(v[2]), "overflow_rows": int(v[3])}
        if self._act_stats["overflow_rows"] > 0:
            stats, self._act_stats = self._act_stats, None
            raise RuntimeError(f'activations="int8": {stats["overflow_rows"]} of {stats["rows"]} activation rows had more than '
                               f'outlier_cap={self.outlier_cap} outliers (the largest row: {stats["max_outliers_per_row"]}); their '
                               "results are not the law's -- raise outlier_cap (up to 1024) or int8_threshold")
        return dict(self._act_stats)

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self.L.cgpt_llm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _cache_tables(self, k_bufs, v_bufs, B, need_len):
        """Host tables of the per-layer K / V device pointers, after checking every buffer is what the kernels index:
        [B, heads, len_stride, 128] fp16 ([B, kv_heads, len_stride, 128] under grouped_kv), contiguous, on the handle's device, long
        enough for the last appended row."""
        C = self._C
        assert len(k_bufs) == len(v_bufs) == self.layers, "one K and one V buffer per layer"
        stride = int(k_bufs[0].shape[2])
        assert need_len <= stride and need_len <= self.MAX_LEN, (need_len, stride, self.MAX_LEN)
        for t in list(k_bufs) + list(v_bufs):
            assert (t.dtype == torch.float16 and t.device == self.device and t.is_contiguous()
                    and tuple(t.shape) == (B, self.kv_heads, stride, 128)), (tuple(t.shape), t.dtype, t.device)
        kp = (C.c_void_p * self.layers)(*[t.data_ptr() for t in k_bufs])
        vp = (C.c_void_p * self.layers)(*[t.data_ptr() for t in v_bufs])
        return kp, vp, stride

    def _starts_ptr(self, starts, B):
        """`starts` [B] int32 on the handle's device (pad positions per row of a left-padded batch; the kernels read it when they run,
        so a captured call sees its contents at every replay) -> the pointer the _ragged entries take."""
        assert (starts.dtype == torch.int32 and starts.device == self.device and starts.is_contiguous()
                and tuple(starts.shape) == (B,)), (tuple(starts.shape), starts.dtype, starts.device)
        return self._C.c_void_p(starts.data_ptr())

    def step(self, tokens, pos, k_bufs, v_bufs, starts=None):
        """One teacher-forced step: tokens [B] int64 at position `pos` -> logits [B, vocab] fp32; K / V row `pos` appended in place.
        starts (or None: the plain entry): left-padded rows, `pos` is the position in the padded buffer."""
        C = self._C
        B = int(tokens.shape[0])
        assert tokens.dtype == torch.int64 and tokens.device == self.device and tokens.is_contiguous() and 1 <= B <= self.max_batch
        kp, vp, stride = self._cache_tables(k_bufs, v_bufs, B, int(pos) + 1)
        logits = torch.empty((B, self.vocab), dtype=torch.float32, device=self.device)
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        if starts is None:
            self._lib_mod.check(self.L.cgpt_llm_step(self.handle, C.c_void_p(tokens.data_ptr()), B, int(pos), kp, vp, stride,
                                                     C.c_void_p(logits.data_ptr()), st))
        else:
            self._lib_mod.check(self.L.cgpt_llm_step_ragged(self.handle, C.c_void_p(tokens.data_ptr()), B, int(pos),
                                                            self._starts_ptr(starts, B), kp, vp, stride, C.c_void_p(logits.data_ptr()), st))
        return logits

    def prefill(self, embs, k_bufs, v_bufs, starts=None):
        """The native prefill: embs [B, L, hidden] fp16 -> last-position logits [B, vocab] fp32; rows 0 .. L-1 of every layer's K / V
        buffer filled in place.  The workspace is reserved here, for `max_batch` rows of this prompt length, so that batches of any
        size share one reservation (outside any capture: a captured call must come after an eager one of the same prompt length,
        which `_generate_graph`'s warm-up run is).  A longer prompt later grows it; the library keeps the replaced buffers until the
        handle goes, so graphs captured before keep replaying on valid memory.
        starts (or None: the plain entry): row b is left-padded by starts[b] positions; cache rows starts[b] .. L-1 are filled."""
        C = self._C
        B, L, hidden = embs.shape
        assert (embs.dtype == torch.float16 and embs.device == self.device and embs.is_contiguous() and hidden == self.heads * 128
                and 1 <= B <= self.max_batch and L >= 1)
        kp, vp, stride = self._cache_tables(k_bufs, v_bufs, B, L)
        if not torch.cuda.is_current_stream_capturing():
            self._lib_mod.check(self.L.cgpt_llm_prefill_reserve(self.handle, self.max_batch, L))
        logits = torch.empty((B, self.vocab), dtype=torch.float32, device=self.device)
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        if starts is None:
            self._lib_mod.check(self.L.cgpt_llm_prefill(self.handle, C.c_void_p(embs.data_ptr()), B, int(L), kp, vp, stride,
                                                        C.c_void_p(logits.data_ptr()), st))
        else:
            self._lib_mod.check(self.L.cgpt_llm_prefill_ragged(self.handle, C.c_void_p(embs.data_ptr()), B, int(L),
                                                               self._starts_ptr(starts, B), kp, vp, stride,
                                                               C.c_void_p(logits.data_ptr()), st))
        return logits

    def greedy(self, first_logits, prompt_len, num_new, min_new, eos_ids, pad_id, k_bufs, v_bufs, return_logits=False, starts=None):
        """The loop of `greedy_tokens` after the prefill: tokens [B, num_new] int64 (and the logits each arg-max saw).
        starts (or None: the plain entry): the prefill's left padding; `prompt_len` is then the padded length."""
        C = self._C
        B, V = first_logits.shape
        assert (first_logits.dtype == torch.float32 and first_logits.device == self.device and first_logits.is_contiguous()
                and V == self.vocab and 1 <= B <= self.max_batch and num_new >= 1 and len(eos_ids) <= 8)
        kp, vp, stride = self._cache_tables(k_bufs, v_bufs, B, prompt_len + num_new - 1)
        tokens = torch.empty((B, num_new), dtype=torch.int64, device=self.device)
        steps = torch.empty((B, num_new, V), dtype=torch.float32, device=self.device) if return_logits else None
        eos = (C.c_int64 * max(1, len(eos_ids)))(*[int(e) for e in eos_ids])
        self._greedy_ran = True
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        tail = (int(num_new), int(min_new), eos, len(eos_ids), int(pad_id), kp, vp, stride, C.c_void_p(tokens.data_ptr()),
                C.c_void_p(steps.data_ptr()) if return_logits else None, st)
        if starts is None:
            self._lib_mod.check(self.L.cgpt_llm_greedy(self.handle, C.c_void_p(first_logits.data_ptr()), B, int(prompt_len), *tail))
        else:
            self._lib_mod.check(self.L.cgpt_llm_greedy_ragged(self.handle, C.c_void_p(first_logits.data_ptr()), B, int(prompt_len),
                                                              self._starts_ptr(starts, B), *tail))
        return (tokens, steps) if return_logits else tokens

    def sample(self, first_logits, prompt_len, num_new, min_new, eos_ids, pad_id, k_bufs, v_bufs, settings, draw_ids, seed,
               return_logits=False, starts=None):
        """`greedy` with the sampling law in the place of the arg-max (cgpt_llm_sample / cgpt_llm_sample_ragged; `sample_token_law`).
        settings = (do_sample, temperature, top_k, top_p, repetition_penalty); draw_ids [B] int64 and seed [1] int64 (the 64 bits of
        the seed) live on the device and are read when the kernels run, so a captured call draws whatever they hold at each replay."""
        C = self._C
        B, V = first_logits.shape
        assert (first_logits.dtype == torch.float32 and first_logits.device == self.device and first_logits.is_contiguous()
                and V == self.vocab and 1 <= B <= self.max_batch and num_new >= 1 and len(eos_ids) <= 8)
        assert (draw_ids.dtype == torch.int64 and draw_ids.device == self.device and draw_ids.is_contiguous()
                and tuple(draw_ids.shape) == (B,)), (tuple(draw_ids.shape), draw_ids.dtype, draw_ids.device)
        assert seed.dtype == torch.int64 and seed.device == self.device and seed.numel() == 1, (seed.dtype, seed.device)
        params = self._lib_mod.sample_params(*check_sample_settings(settings))
        kp, vp, stride = self._cache_tables(k_bufs, v_bufs, B, prompt_len + num_new - 1)
        tokens = torch.empty((B, num_new), dtype=torch.int64, device=self.device)
        steps = torch.empty((B, num_new, V), dtype=torch.float32, device=self.device) if return_logits else None
        eos = (C.c_int64 * max(1, len(eos_ids)))(*[int(e) for e in eos_ids])
        self._greedy_ran = True
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        tail = (int(num_new), int(min_new), eos, len(eos_ids), int(pad_id), kp, vp, stride, C.c_void_p(tokens.data_ptr()),
                C.c_void_p(steps.data_ptr()) if return_logits else None, params, C.c_void_p(draw_ids.data_ptr()),
                C.c_void_p(seed.data_ptr()), st)
        if starts is None:
            self._lib_mod.check(self.L.cgpt_llm_sample(self.handle, C.c_void_p(first_logits.data_ptr()), B, int(prompt_len), *tail))
        else:
            self._lib_mod.check(self.L.cgpt_llm_sample_ragged(self.handle, C.c_void_p(first_logits.data_ptr()), B, int(prompt_len),
                                                              self._starts_ptr(starts, B), *tail))
        return (tokens, steps) if return_logits else tokens

    def set_early_stop(self, on):
        """cgpt_llm_set_early_stop: read by the next `greedy` when it enqueues; a captured call keeps what it was captured under."""
        self._lib_mod.check(self.L.cgpt_llm_set_early_stop(self.handle, int(bool(on))))
        self.early_stop = bool(on)

    def set_stop_sequences(self, seqs):
        """cgpt_llm_set_stop_sequences: token-id sequences (`check_stop_words_ids`; () or None clears them) at which a row of the next
        `greedy` finishes besides its EOS ids; read when it enqueues, a captured call keeps what it was captured under."""
        C = self._C
        seqs = check_stop_words_ids(seqs)
        flat = [t for s in seqs for t in s]
        ids = (C.c_int64 * max(1, len(flat)))(*flat)
        lens = (C.c_int32 * max(1, len(seqs)))(*[len(s) for s in seqs])
        self._lib_mod.check(self.L.cgpt_llm_set_stop_sequences(self.handle, ids, lens, len(seqs)))
        self.stop_sequences = seqs

    def live_steps(self):
        """cgpt_llm_live_steps after the last `greedy` (or the last replay of a graph that captured it): the token steps that ran.
        Synchronises the CURRENT stream -- the one the call was enqueued or the graph replayed on; RuntimeError when no greedy has
        been enqueued."""
        C = self._C
        if not self._greedy_ran:
            raise RuntimeError("live_steps: no native greedy decode has run on this engine yet")
        n = C.c_int32(-1)
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        self._lib_mod.check(self.L.cgpt_llm_live_steps(self.handle, C.byref(n), st))
        return int(n.value)

    MAX_CANDS, MAX_TAIL = 64, 64                                       # SCORE_MAX_CANDS, SCORE_MAX_TAIL (csrc/llm.h)

    def score(self, first_logits, prompt_len, cand_tokens, cand_lens, label_smoothing, k_bufs, v_bufs, starts=None, row_lens=None):
        """Every candidate on the prompt cache a prefill left (cgpt_llm_score): first_logits [B, vocab] fp32 = that prefill's result,
        cand_tokens [C, Tmax] int64 on the device, cand_lens = the C token counts (host) -> [B, C] fp32, the SUM over each
        candidate's tokens of the label-smoothed cross-entropy.  Reads cache rows 0 .. prompt_len-1 and writes none.  The workspace is
        reserved here (outside any capture), for `max_batch` rows of this call's tail rows.
        starts and row_lens (both, or both None: the plain entry) -- per-row prompts and candidates (cgpt_llm_score_ragged): starts
        [B] int32 = the ragged prefill's left padding, `prompt_len` the padded length; cand_tokens [B, C, Tmax], row_lens [B, C] int32 on
        the device = each row's real length of each candidate, cand_lens = the longest length of each candidate over the rows
        (`pack_row_candidates`).  Reads cache rows starts[b] .. prompt_len-1 only; sums each row's own tokens."""
        C = self._C
        B, V = first_logits.shape
        assert (starts is None) == (row_lens is None), "starts and row_lens travel together"
        n, tmax = cand_tokens.shape[-2:]
        lens = [int(t) for t in cand_lens]
        assert (first_logits.dtype == torch.float32 and first_logits.device == self.device and first_logits.is_contiguous()
                and V == self.vocab and 1 <= B <= self.max_batch)
        assert (cand_tokens.dtype == torch.int64 and cand_tokens.device == self.device and cand_tokens.is_contiguous()
                and len(lens) == n and tuple(cand_tokens.shape) == ((n, tmax) if starts is None else (B, n, tmax)))
        if row_lens is not None:
            assert (row_lens.dtype == torch.int32 and row_lens.device == self.device and row_lens.is_contiguous()
                    and tuple(row_lens.shape) == (B, n)), (tuple(row_lens.shape), row_lens.dtype, row_lens.device)
        kp, vp, stride = self._cache_tables(k_bufs, v_bufs, B, int(prompt_len))
        if not torch.cuda.is_current_stream_capturing():
            self._lib_mod.check(self.L.cgpt_llm_score_reserve(self.handle, self.max_batch, max(1, sum(t - 1 for t in lens))))
        out = torch.empty((B, n), dtype=torch.float32, device=self.device)
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        tail = ((C.c_int32 * n)(*lens), n, int(tmax), float(label_smoothing), kp, vp, stride, C.c_void_p(out.data_ptr()), st)
        if starts is None:
            self._lib_mod.check(self.L.cgpt_llm_score(self.handle, C.c_void_p(first_logits.data_ptr()), B, int(prompt_len),
                                                      C.c_void_p(cand_tokens.data_ptr()), *tail))
        else:
            self._lib_mod.check(self.L.cgpt_llm_score_ragged(self.handle, C.c_void_p(first_logits.data_ptr()), B, int(prompt_len),
                                                             self._starts_ptr(starts, B), C.c_void_p(cand_tokens.data_ptr()),
                                                             C.c_void_p(row_lens.data_ptr()), *tail))
        return out


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
       :param stop_words_ids: None (default) | up to 8 token-id sequences of 1..8 tokens -- a row finishes when its answer ends in one
       :param stop_text: None (default) | str -- every decoded answer is cut at its first occurrence (the reference's "###")
       :param end_sym: text appended to every candidate answer of `multi_select` ("\n": the reference's default; its VQA configs: "###")
       :param label_smoothing: of the answer loss (0.1: modeling_llama.py:105)
       :param score: "hf" (default) | "hip" -- who computes the answer losses of `multi_select`; see __init__
       :param classify: "generate" (default) | "multi_select" -- what the base classifier of `Smooth` does with a batch; see __init__
       :param candidates: the answers `classify="multi_select"` ranks (default: `label_map.answers`, in class-id order)

    `prompt` is a plain attribute: assigning a new prompt between two images (`clf.prompt = ...`) is the supported way to ask a
    per-image question (VQA: one question per image).  Under decode="graph" / "hip" every new prompt LENGTH captures a graph of its
    own; with ragged="hip", prompt_bucket=k all prompts whose length rounds up to the same multiple of k replay one graph.
    """

    noise_laws = ("gaussian", "uniform")       # passed through to encoder.encode_img_noisy

    def __init__(self, encoder, llama_model, llama_tokenizer, prompt, label_map, max_new_tokens=20, max_batch=None,
                 generate_kwargs=None, decode="hf", prefill_linear="torch", prefill="model", ragged="hf", prompt_bucket=None,
                 weights="fp16", end_sym="\n", label_smoothing=0.1, score="hf", classify="generate", candidates=None,
                 early_stop=False, grouped_kv=False, activations="fp16", int8_threshold=6.0, outlier_cap=64, stop_words_ids=None,
                 stop_text=None, sample="hf"):
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
        #   (csrc/llm.hip: RMSNorm, decode-shape GEMMs, rotary + K/V append + one-query attention, token select) on the K/V the
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
        if classify not in ("generate", "multi_select"):
            raise ValueError(f'classify={classify!r}: expected "generate" or "multi_select"')
        if not 0.0 <= float(label_smoothing) < 1.0:
            raise ValueError(f"label_smoothing={label_smoothing!r}: expected a value in [0, 1)")
        if candidates is not None and classify != "multi_select":
            raise ValueError('candidates need classify="multi_select" (classify="generate" maps free text through label_map)')
        if classify == "multi_select":
            candidates = list(label_map.answers if candidates is None else candidates)
            if not 2 <= len(candidates) <= self.num_classes - 1:
                raise ValueError(f'classify="multi_select" needs at least 2 and at most num_classes - 1 = {self.num_classes - 1} '
                                 f"candidates (got {len(candidates)}): class id num_classes - 1 stays \"other\"")
        self.end_sym = end_sym
        self.label_smoothing = float(label_smoothing)
        self.score = score
        self.classify = classify
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
        self.sample = sample
        self._draw_next, self._draw_seed = 0, 0             # `reset_draws`: the ids and the seed of calls that name no sample index
        self._draw_bufs = None                              # (ids [max_batch] int64, seed [1] int64) on the device, made at first use
        if sample == "hip":
            self._sample_settings()                         # a ValueError for a setting the sampler refuses comes now
        # the keyword reaches the engine only when it is set (as `law` reaches an encoder)
        gqa = {"grouped_kv": True} if grouped_kv else {}
        self.activations, self.int8_threshold, self.outlier_cap = activations, float(int8_threshold), int(outlier_cap)
        if activations == "int8":
            gqa.update(activations="int8", int8_threshold=self.int8_threshold, outlier_cap=self.outlier_cap)
        self._hip = _HipDecoder(llama_model, self.max_batch, weights=weights, early_stop=early_stop, **gqa) if decode == "hip" else None
        if self._hip is not None and stops:                 # none is the handle's state at create: nothing is called for it
            self._hip.set_stop_sequences(stops)
        self.routed_linears = (_LinearRoute.install(llama_model)
                               if (decode in ("graph", "hip") and prefill_linear == "cgpt" and prefill == "model") else 0)
        import collections
        self._graphs = collections.OrderedDict()            # LRU of captured decode graphs, see _generate_graph
        self.max_graphs = 4
        self._eos_mask = None
        self.decode_stats = {"graph_replays": 0, "graph_captures": 0, "graph_evictions": 0, "hf_calls": 0, "hf_fallback_kwargs": 0,
                             "hip_steps": 0,                      # token steps enqueued on the native engine (decode = "hip")
                             "hip_prefills": 0,                   # native prefills enqueued (prefill = "hip"), counted alike
                             "hf_score_forwards": 0,              # model forwards of score = "hf": one per candidate and call
                             "hip_scores": 0,                     # native scoring passes (score = "hip"): one per call
                             "hip_ragged_scores": 0,              # native per-row scoring passes (score = "hip", ragged = "hip")
                             "hf_score_fallbacks": 0,             # score = "hip" calls that took the "hf" path (see __init__)
                             "hip_sampled": 0,                    # decodes of the native sampler (sample = "hip"): one per call
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
    def _segment_embeddings(self, prompt, device):
        segs = prompt.split(IMAGE_PLACEHOLDER)
        toks = [self.llama_tokenizer(seg, return_tensors="pt", add_special_tokens=(i == 0)).input_ids.to(device)
                for i, seg in enumerate(segs)]                         # only add bos to the first seg
        return [self.embed_tokens(t) for t in toks]

    def get_context_emb(self, prompt, img_list):
        seg_embs = self._segment_embeddings(prompt, img_list[0].device)
        assert len(seg_embs) == len(img_list) + 1, "Unmatched numbers of image placeholders and images."
        mixed = [emb for pair in zip(seg_embs[:-1], img_list) for emb in pair] + [seg_embs[-1]]
        return torch.cat(mixed, dim=1)

    # ---- minigpt_base.py:374-448 with encode_img's output given
    @torch.no_grad()
    def generate_from_embeds(self, img_embeds, texts, draws=None):
        """img_embeds [B, queries, hidden] (any float dtype) + one prompt per row (or ONE str shared by all rows) -> list[str].
        draws (sample = "hip" only): (first draw id, seed) -- row r draws stream first + r; None: the running counter (`reset_draws`)."""
        dtype = self.embed_tokens(torch.zeros(1, 1, dtype=torch.long, device=img_embeds.device)).dtype
        img_embeds = img_embeds.to(dtype)
        B = img_embeds.shape[0]
        shared = isinstance(texts, str) or len(set(texts)) == 1
        # the native engine takes left-padded rows only where it would take a shared prompt: on the device, greedy arguments
        native_pad = self.ragged == "hip" and img_embeds.is_cuda and self._greedy_defaults()
        starts = None
        if shared:
            # shared prompt: segments embedded once and broadcast; equal lengths -> no padding, all-ones mask
            prompt = texts if isinstance(texts, str) else texts[0]
            segs = self._segment_embeddings(prompt, img_embeds.device)
            assert len(segs) == 2, "Unmatched numbers of image placeholders and images."
            embs = torch.cat([segs[0].expand(B, -1, -1), img_embeds, segs[1].expand(B, -1, -1)], dim=1)
            if native_pad and self.prompt_bucket:                      # padded up to the bucket: one graph for every length in it
                embs, attn_mask, starts = left_pad_embeds([embs], self.prompt_bucket)
            else:
                attn_mask = torch.ones(embs.shape[:2], dtype=torch.int, device=embs.device)
        else:
            assert len(texts) == B
            batch_embs = [self.get_context_emb(t, [img_embeds[i][None]]) for i, t in enumerate(texts)]
            embs, attn_mask, starts = left_pad_embeds(batch_embs, self.prompt_bucket if native_pad else None)     # minigpt_base.py:407-416
            if not native_pad:
                starts = None
        if self.decode in ("graph", "hip") and (shared or native_pad) and embs.is_cuda and self._greedy_defaults():
            if self._sample_settings() is not None:                     # written before the replay: the kernels read them when they run
                self._write_draws(B, draws, embs.device)
                self.decode_stats["hip_sampled"] += 1
            outputs = self._generate_graph(embs, starts)
            if self.activations == "int8":                              # the tokens are read next: the same sync
                self.last_act_stats()
        else:
            self.decode_stats["hf_calls"] += 1
            if self.decode in ("graph", "hip") and (shared or self.ragged == "hip") and embs.is_cuda:
                self.decode_stats["hf_fallback_kwargs"] += 1            # generation arguments outside the greedy whitelist
            outputs = self.llama_model.generate(inputs_embeds=embs, attention_mask=attn_mask, max_new_tokens=self.max_new_tokens,
                                                **self.hf_generate_kwargs())
        return self._decode_outputs(outputs)

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

    def _greedy_defaults(self):
        """May this call take the fixed-length greedy loop?  Only when every argument of the call AND every field of the model's own
        generation_config (which `generate` applies wherever the call is silent) is one the loop reproduces; otherwise the HF path
        runs, so the same classifier never decodes differently by `decode=`."""
        for key, val in self.generate_kwargs.items():
            if key not in self._GREEDY_NEUTRAL:
                return False
            if self.sample == "hip" and key in SAMPLE_FIELDS:         # the native sampler takes these at any value it accepts
                continue
            want = self._GREEDY_NEUTRAL[key]
            if want is not None and val != want:
                return False
        gen = getattr(self.llama_model, "generation_config", None)
        if gen is not None:
            for key, neutral in self._CONFIG_NEUTRAL.items():
                if key in self.generate_kwargs or (self.sample == "hip" and key in SAMPLE_FIELDS):
                    continue                                           # the call's argument wins over the checkpoint's field
                val = getattr(gen, key, None)
                if isinstance(val, (list, tuple, dict)) and len(val) == 0:
                    val = None
                if val not in neutral:
                    return False
        return True

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

    def _select(self, logits, L, min_new, eos_ids, pad, k_bufs, v_bufs, return_logits, starts=None):
        """The native loop after the prefill: the sampler under sample = "hip" when the settings ask for it, the arg-max otherwise."""
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

    def greedy_tokens(self, embs, return_logits=False, starts=None):
        """What `generate(inputs_embeds=embs, attention_mask=ones, max_new_tokens=n, do_sample=False, min_length=1, ...)` returns for
        prompts without padding, as a straight loop of the model's own forward calls: [B, n] token ids, pad_token_id after a row's
        EOS.  (HF additionally stops, and truncates, at the step where every row has finished; the extra columns here are pad ids,
        which decode to nothing.)  No data-dependent control flow: capturable as one graph.
        starts ([B] int32 on the device, prefill = "hip" only): row b of `embs` is left-padded by starts[b] positions (zeros); the
        result is what each row gives without its padding."""
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
        gen = getattr(llm, "generation_config", None)
        eos = getattr(gen, "eos_token_id", None)
        eos = getattr(llm.config, "eos_token_id", None) if eos is None else eos
        eos_ids = list(eos) if isinstance(eos, (list, tuple)) else ([eos] if eos is not None else [])
        pad = getattr(gen, "pad_token_id", None)
        pad = getattr(llm.config, "pad_token_id", None) if pad is None else pad
        pad = (eos_ids[0] if eos_ids else 0) if pad is None else pad
        B, L, _ = embs.shape
        assert starts is None or self.prefill == "hip", 'left-padded rows need prefill="hip"'
        if self.prefill == "hip":                                      # the whole decode in this library: no HF forward, no DynamicCache
            assert B <= self.max_batch, f"{B} rows > max_batch {self.max_batch} (the native decoder's workspace)"
            shape = (B, self._hip.kv_heads, L + self.max_new_tokens, 128)    # what PreallocLayer allocates on the other path
            k_bufs = [embs.new_empty(shape) for _ in range(self._hip.layers)]
            v_bufs = [embs.new_empty(shape) for _ in range(self._hip.layers)]
            logits = self._hip.prefill(embs.contiguous(), k_bufs, v_bufs, starts=starts)
            self.decode_stats["hip_prefills"] += 1
            self.decode_stats["hip_steps"] += self.max_new_tokens - 1
            return self._select(logits, L, self.min_new_tokens() if eos_ids else 0, eos_ids, pad, k_bufs, v_bufs, return_logits, starts)
        cache = DynamicCache(config=llm.config)
        cache.layers = [PreallocLayer(L + self.max_new_tokens) for _ in cache.layers] or cache.layers
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
            self.decode_stats["hip_steps"] += self.max_new_tokens - 1
            return self._select(logits.contiguous(), L, min_new, eos_ids, pad, [l.buf_k for l in cache.layers],
                                [l.buf_v for l in cache.layers], return_logits)
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

    def _graph_key(self, embs, ragged=False):
        key = (embs.shape[0], embs.shape[1], embs.dtype, embs.device.index, self.max_new_tokens, bool(self.routed_linears), self.decode,
               self.prefill)
        key = key + ("ragged",) if ragged else key                    # a graph of the _ragged entries is never an unpadded one's
        key = key + ("grouped_kv",) if self.grouped_kv else key
        key = key + ("early_stop",) if self.early_stop else key       # nor is one captured with early stop on one captured without
        key = key + ("stop", self.stop_words_ids) if self.stop_words_ids else key      # nor under one set of stop sequences another's
        settings = self._sample_settings()
        return key + ("sample", settings) if settings is not None else key             # nor the sampler under one law another's

    def last_live_steps(self):
        """Token steps of the most recent native greedy decode (eager, or the last graph replay) that actually ran: max_new_tokens - 1
        with early_stop off, min(F, max_new_tokens - 1) with it on, F = the first select at which every row had produced an EOS.
        ONE host sync, which is why it is never read on its own after a replay.  RuntimeError when no native greedy decode has run."""
        if self._hip is None:
            raise RuntimeError('last_live_steps: no native engine (decode="hip") on this classifier')
        return self._hip.live_steps()

    def _generate_graph(self, embs, starts=None):
        """One captured hipGraph per (batch, prompt length, dtype, device, max_new_tokens, routed prefill, engine, prefill engine), kept in an LRU of
        `max_graphs` entries: a graph pins its private pool -- the pre-allocated K / V of every layer plus activations, ~6.7 GB of K / V
        alone at 200 rows x 32 layers x 64 positions -- and ragged last batches or new prompt lengths add entries; the least recently
        used one is dropped (graph and static tensors freed) before a new capture.
        starts (left-padded rows, see greedy_tokens): the graph is captured on a static copy that is refreshed before every replay, like
        the embeds -- the kernels read it when they run, so one graph per (batch, PADDED length) serves every mix of prompt lengths."""
        key = self._graph_key(embs, ragged=starts is not None)
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
            side = torch.cuda.Stream(device=embs.device)
            side.wait_stream(torch.cuda.current_stream())
            import contextlib
            route = _LinearRoute.enabled() if self.routed_linears else contextlib.nullcontext()
            hip_steps = self.decode_stats["hip_steps"]                 # counted per replay below, not for warm-up and capture
            hip_prefills = self.decode_stats["hip_prefills"]
            with route:
                with torch.cuda.stream(side):                          # warm-up outside the capture (lazy initialisations)
                    self.greedy_tokens(static_in, starts=static_starts)
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
                        static_out = self.greedy_tokens(static_in, starts=static_starts)
                finally:
                    if gc_was_on:
                        gc.enable()
            self.decode_stats["hip_steps"] = hip_steps
            self.decode_stats["hip_prefills"] = hip_prefills
            entry = (graph, static_in, static_out, static_starts)
            self._graphs[key] = entry
            self.decode_stats["graph_captures"] += 1
        graph, static_in, static_out, static_starts = entry
        static_in.copy_(embs)
        if static_starts is not None:
            static_starts.copy_(starts)
        graph.replay()
        self.decode_stats["graph_replays"] += 1
        if self._hip is not None:
            self.decode_stats["hip_steps"] += self.max_new_tokens - 1
        if self.prefill == "hip":
            self.decode_stats["hip_prefills"] += 1
        return static_out.clone()

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
        shape = (B, hip.kv_heads, L, 128)                              # the prompt's rows only: scoring appends nothing
        k_bufs = [embs.new_empty(shape) for _ in range(hip.layers)]
        v_bufs = [embs.new_empty(shape) for _ in range(hip.layers)]
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
        shape = (B, hip.kv_heads, L, 128)
        k_bufs = [embs.new_empty(shape) for _ in range(hip.layers)]
        v_bufs = [embs.new_empty(shape) for _ in range(hip.layers)]
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
        -inf in column `other_id` (and in unused columns), so the top class is always a candidate."""
        if self.classify == "generate":
            # the keyword travels only where it says something (sample = "hip"): subclasses that replace generate_from_embeds keep working
            kw = {"draws": draws} if draws is not None and self.sample == "hip" else {}
            answers = self.generate_from_embeds(emb, self.prompt, **kw)
            return self.label_map.one_hot_logits(answers, device), answers
        losses = self.answer_losses_from_embeds(emb, self.prompt, self.candidates)
        logits = torch.full((losses.shape[0], self.num_classes), float("-inf"), dtype=torch.float32, device=losses.device)
        logits[:, :losses.shape[1]] = -losses
        answers = [self.candidates[i] for i in losses.argmin(dim=1).tolist()]
        return logits.to(device), answers

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
        bs = max(1, min(int(batch_size), self.max_batch))
        done = 0
        while done < num:
            nb = min(bs, num - done)
            emb = self._encode_noisy(x, first_sample + done, nb, sigma, seed, law)
            logits, self.last_answers = self._classify_embeds(emb, x.device, draws=(first_sample + done, seed))
            vote(logits, counts)
            done += nb
        return counts
