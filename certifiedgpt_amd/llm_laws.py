"""The arithmetic laws of the LLaMA path, stated once: what the native engine (llm_engine.py, csrc/llm*.hip) and the classifier
(minigpt4.py) are specified to compute, in plain torch.  The tests use them as oracles; the engine and the classifier use the checks.

    the finishing rule of the greedy decode (EOS ids + per-row stop sequences)   stop_finish_columns, apply_stop_sequences, ...
    the sampling law and its Philox uniform                                      sample_uniform, sample_token_law, ...
    the parity rule between two greedy decoders of one fp16 model                greedy_decode_parity, fp16_ulp
    the int8 weight law and the int8 activation law with its outlier split       quantize_rows_int8, llm_int8_linear, act_int8_twin, ...
    the multi-head twin of a grouped-query decoder                               expand_kv_state_dict
    left padding and per-row candidate packing                                   left_pad_embeds, pack_row_candidates
    the trie-constrained select over a vocabulary of candidate answers           build_answer_trie, constrained_select_law, ...
    beam search, HF 5.x `_beam_search` restated                                  beam_step_law, beam_decode_law, check_beam_settings

Nothing here touches the library or a device API: torch and the standard library only (`transformers` lazily, where a law is handed
to HF).  Dependencies point one way: llm_laws <- llm_engine <- minigpt4.
"""
import torch


MAX_STOP_SEQS, MAX_STOP_LEN = 8, 8                                    # MAX_STOP, MAX_STOP_LEN of csrc/llm_select.h


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


def shared_prefix_len(first_segment_ids):
    """shared_prefix=True: the positions every row of a call shares in front of its image tokens.  `first_segment_ids` holds one
    sequence of token ids per row -- the tokens of the prompt's first segment (everything before <ImageHere>: <s>, the template's
    opening, "<Img>", a system text) -- and the result is P, their common length, when every row's ids are equal, and 0 otherwise
    (no row, an empty segment, or rows that differ anywhere: the call then takes the whole-prompt prefill).  Equal TOKENS, not equal
    lengths: under causal attention the hidden states and K/V rows of those positions are then the same in every layer for every row,
    which is what lets one prefill on one row stand for all of them.  Pure: sequences of ints in, an int out."""
    rows = [tuple(int(t) for t in ids) for ids in first_segment_ids]
    if not rows or not rows[0] or any(r != rows[0] for r in rows[1:]):
        return 0
    return len(rows[0])


def left_pad_embeds(batch_embs, bucket=None, prefix=0):
    """Left padding of prompts of different lengths (minigpt_base.py:407-416): `batch_embs` is a list of tensors [n_i, len_i, hidden]
    (n_i rows that share one length; the reference's loop has n_i = 1) -> (embeds [B, L, hidden] with zeros on the pad positions,
    attention mask [B, L] int, starts [B] int32 = pad positions per row), B = sum n_i, L = the longest length, rounded up to a
    multiple of `bucket` when that is set.  Row b's real tokens sit at positions starts[b] .. L-1.  Pure tensor arithmetic on the
    inputs' device (CPU tensors work); a row with no real token is a ValueError.
    prefix = P (shared_prefix=True): the rows are SUFFIXES that follow P positions held elsewhere; it is P + L that is rounded up to
    the bucket, so P + L is the padded length, and starts are the starts, of the same call on the whole prompts."""
    if bucket is not None and (isinstance(bucket, bool) or not isinstance(bucket, int) or bucket < 1):
        raise ValueError(f"bucket={bucket!r}: expected None or an int >= 1")
    if not batch_embs:
        raise ValueError("left_pad_embeds: no rows")
    lens = [int(e.shape[1]) for e in batch_embs]
    if min(lens) < 1:
        raise ValueError(f"left_pad_embeds: row group {lens.index(min(lens))} has no real token (length 0)")
    if isinstance(prefix, bool) or not isinstance(prefix, int) or prefix < 0:
        raise ValueError(f"prefix={prefix!r}: expected an int >= 0")
    L = max(lens)
    if bucket:
        L = (prefix + L + bucket - 1) // bucket * bucket - prefix
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


# ---- the weight law of weights="int8" (csrc/llm_step.hip: llm_quant_rows_kernel; include/cgpt.h: CGPT_LLM_W_INT8), in plain torch
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


# ---- trie-constrained answer decoding (classify="constrained"; csrc/llm_trie.hip; include/cgpt.h), stated once
TRIE_MAX_NODES, TRIE_MAX_DEPTH = 2 ** 20, 32                            # TRIE_MAX_NODES, TRIE_MAX_DEPTH of csrc/llm_select.h


class AnswerTrie:
    """The candidates' token sequences as a CSR trie of int32 CPU tensors (`build_answer_trie`): the edges of node n are
    child_begin[n] .. child_begin[n + 1], edge e carries token child_tok[e] and leads to node child_node[e]; leaf_class[n] is the
    candidate's index at a leaf and -1 on an inner node; `depth` is the longest candidate."""

    def __init__(self, child_begin, child_tok, child_node, leaf_class, depth):
        self.child_begin, self.child_tok, self.child_node, self.leaf_class, self.depth = child_begin, child_tok, child_node, leaf_class, int(depth)

    @property
    def nodes(self):
        return int(self.leaf_class.numel())

    @property
    def edges(self):
        return int(self.child_tok.numel())

    def tables(self):
        return self.child_begin, self.child_tok, self.child_node, self.leaf_class

    def to(self, device):
        return AnswerTrie(*[t.to(device) for t in self.tables()], self.depth)


def build_answer_trie(seqs, vocab_size, names=None):
    """seqs[c] = the token ids of candidate c -> `AnswerTrie`.  Node 0 is the root; nodes are numbered breadth-first (the child of
    edge e is node e + 1, so a child's index is greater than its parent's); the edges of one node ascend strictly by token id, which
    is what makes "first maximum" mean "lowest token id".  The tables depend on the SET of sequences alone (every rank of a
    distributed run builds the same ones); leaf_class follows the input order.
    ValueError naming the candidates (names[c], default: the index) for: an empty sequence, a token outside 0 .. vocab_size-1, two equal
    sequences, a sequence that is a proper prefix of another (a leaf has no children), fewer than 2 candidates, more than 2**20 nodes,
    depth over 32."""
    seqs = [tuple(int(t) for t in (s.tolist() if hasattr(s, "tolist") else s)) for s in seqs]
    name = (lambda c: repr(names[c])) if names is not None else (lambda c: f"#{c}")
    if len(seqs) < 2:
        raise ValueError(f"a constrained decode needs at least 2 candidates (got {len(seqs)})")
    seen = {}
    for c, s in enumerate(seqs):
        if not s:
            raise ValueError(f"candidate {name(c)} has no token")
        bad = [t for t in s if not 0 <= t < int(vocab_size)]
        if bad:
            raise ValueError(f"candidate {name(c)} holds token {bad[0]} outside 0..{int(vocab_size) - 1}")
        if s in seen:
            raise ValueError(f"candidates {name(seen[s])} and {name(c)} have the same tokens {list(s)}")
        seen[s] = c
    depth = max(len(s) for s in seqs)
    if depth > TRIE_MAX_DEPTH:
        c = max(range(len(seqs)), key=lambda i: len(seqs[i]))
        raise ValueError(f"candidate {name(c)} has {depth} tokens (at most {TRIE_MAX_DEPTH})")
    order = sorted(range(len(seqs)), key=lambda c: seqs[c])            # lexicographic: a prefix sorts right before its extensions
    for a, b in zip(order, order[1:]):
        if seqs[b][:len(seqs[a])] == seqs[a]:
            raise ValueError(f"candidate {name(a)} (tokens {list(seqs[a])}) is a prefix of candidate {name(b)} (tokens {list(seqs[b])}): "
                             "a row would end at the shorter one")
    # breadth-first over groups of candidates that share a prefix; within a node the groups come in ascending token order
    child_begin, child_tok, child_node, leaf_class = [0], [], [], [-1]
    queue, head = [(order, 0)], 0                                      # (sorted candidates below the node, the node's depth)
    while head < len(queue):
        members, d = queue[head]
        head += 1
        if len(members) == 1 and len(seqs[members[0]]) == d:           # a leaf
            leaf_class[head - 1] = members[0]
            child_begin.append(len(child_tok))
            continue
        i = 0
        while i < len(members):
            tok = seqs[members[i]][d]
            j = i
            while j < len(members) and seqs[members[j]][d] == tok:
                j += 1
            child_tok.append(tok)
            child_node.append(len(queue))
            queue.append((members[i:j], d + 1))
            leaf_class.append(-1)
            i = j
        child_begin.append(len(child_tok))
        if len(queue) > TRIE_MAX_NODES:
            raise ValueError(f"the candidates' trie has more than {TRIE_MAX_NODES} nodes")
    as_i32 = lambda v: torch.tensor(v, dtype=torch.int32)              # noqa: E731
    return AnswerTrie(as_i32(child_begin), as_i32(child_tok), as_i32(child_node), as_i32(leaf_class), depth)


def constrained_select_law(logits, node, unfinished, trie, pad):
    """One select of the constrained decode over logits [B, V] (fp32, finite by contract), node [B] and unfinished [B] (ints) ->
    (token [B] int64, node' [B] int32, unfinished' [B] int32, label [B] int32).  A finished row gives `pad` and keeps its node; an
    unfinished row takes the FIRST maximum of logits[b, child_tok[e]] over its node's edges (ascending tokens: the lowest token id
    among the maxima) and moves to that child; if the child is a leaf the row finishes with label = leaf_class, else label is -1."""
    cb, ct, cn, lc = [t.tolist() for t in trie.tables()]
    rows = logits.detach().float().cpu()
    token, node2, unf2, label = [], [], [], []
    for b, (n, u) in enumerate(zip([int(v) for v in node.tolist()], [int(v) for v in unfinished.tolist()])):
        if not u:
            token.append(int(pad)); node2.append(n); unf2.append(0); label.append(-1)
            continue
        e0, e1 = cb[n], cb[n + 1]
        vals = rows[b, torch.tensor(ct[e0:e1], dtype=torch.long)]
        e = e0 + int((vals == vals.max()).nonzero()[0])                # the first maximum
        child = cn[e]
        token.append(ct[e]); node2.append(child); unf2.append(0 if lc[child] >= 0 else 1); label.append(lc[child] if lc[child] >= 0 else -1)
    dev = logits.device
    return (torch.tensor(token, dtype=torch.int64, device=dev), torch.tensor(node2, dtype=torch.int32, device=dev),
            torch.tensor(unf2, dtype=torch.int32, device=dev), torch.tensor(label, dtype=torch.int32, device=dev))


def constrained_decode_law(step_logits, trie, pad):
    """`constrained_select_law` over step_logits [B, depth, V], teacher-forced on the given per-step logits: every row starts
    unfinished at the root -> (tokens [B, depth] int64, labels [B] int32).  The test oracle of the native loop and of HF's."""
    B, depth, _ = step_logits.shape
    assert depth == trie.depth, (depth, trie.depth)
    dev = step_logits.device
    node = torch.zeros(B, dtype=torch.int32, device=dev)
    unfinished = torch.ones(B, dtype=torch.int32, device=dev)
    labels = torch.full((B,), -1, dtype=torch.int32, device=dev)
    tokens = []
    for i in range(depth):
        tok, node, unfinished, lab = constrained_select_law(step_logits[:, i], node, unfinished, trie, pad)
        labels = torch.where(lab >= 0, lab, labels)
        tokens.append(tok)
    return torch.stack(tokens, dim=1), labels


def trie_walk(tokens, trie):
    """The leaf class each row of `tokens` [B, n] (tensor or nested lists) spells from the root, reading tokens until a leaf; -1 for
    a row that leaves the trie or ends on an inner node."""
    cb, ct, cn, lc = [t.tolist() for t in trie.tables()]
    out = []
    for row in _as_rows(tokens):
        n = 0
        for t in row:
            if lc[n] >= 0:
                break
            edge = {ct[e]: cn[e] for e in range(cb[n], cb[n + 1])}
            if t not in edge:
                n = -1
                break
            n = edge[t]
        out.append(lc[n] if n >= 0 else -1)
    return out


def allowed_tokens_fn(trie, pad=0):
    """The `prefix_allowed_tokens_fn(batch_id, input_ids)` of HF `generate` for `trie`: walks the GENERATED ids (the prompt is
    embeddings, so `input_ids` holds generated tokens only) from the root and returns the tokens of the node's edges; [pad] after a
    leaf, and for ids that left the trie."""
    cb, ct, cn, lc = [t.tolist() for t in trie.tables()]
    edges = [{ct[e]: cn[e] for e in range(cb[n], cb[n + 1])} for n in range(len(lc))]

    def fn(batch_id, input_ids):
        n = 0
        for t in input_ids.tolist():
            if lc[n] >= 0 or t not in edges[n]:
                return [int(pad)]
            n = edges[n][t]
        return [int(pad)] if lc[n] >= 0 else list(edges[n].keys())
    return fn


# ---- beam search (beams="hip"; csrc/llm_beam.hip; include/cgpt.h: "Beam search"), stated once
BEAM_MIN, BEAM_MAX = 2, 8                                               # num_beams the native engine takes
BEAM_NEG = -1.0e9                                                       # HF's "never chosen" score
BEAM_FIELDS = ("num_beams", "length_penalty")
# the fields that shape a beam search, with GenerationConfig's defaults: what `generate` resolves where call and checkpoint are silent
BEAM_HF_DEFAULTS = {"num_beams": 1, "length_penalty": 1.0, "early_stopping": False, "num_return_sequences": 1, "num_beam_groups": 1}


def check_beam_settings(num_beams, length_penalty=1.0, early_stopping=False, num_return_sequences=1, num_beam_groups=1,
                        do_sample=False, repetition_penalty=1.0):
    """(num_beams, length_penalty) as the native beam search takes them; ValueError naming the field for num_beams outside 2..8, a
    length_penalty that is not finite, early_stopping set (True or "never"), num_return_sequences != 1, num_beam_groups != 1,
    do_sample set or a repetition_penalty other than 1 (beam sampling and penalised beams are HF's)."""
    if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not BEAM_MIN <= num_beams <= BEAM_MAX:
        raise ValueError(f"num_beams={num_beams!r}: expected an int in {BEAM_MIN}..{BEAM_MAX}")
    lp = 1.0 if length_penalty is None else length_penalty
    if isinstance(lp, bool) or not isinstance(lp, (int, float)) or lp != lp or abs(lp) == float("inf"):
        raise ValueError(f"length_penalty={length_penalty!r}: expected a finite number")
    if early_stopping not in (False, None):
        raise ValueError(f"early_stopping={early_stopping!r}: only early_stopping=False is supported")
    if num_return_sequences not in (1, None):
        raise ValueError(f"num_return_sequences={num_return_sequences!r}: only 1 is supported")
    if num_beam_groups not in (1, None):
        raise ValueError(f"num_beam_groups={num_beam_groups!r}: only 1 is supported (no group / diverse beams)")
    if do_sample not in (False, None, 0):
        raise ValueError(f"do_sample={do_sample!r}: beam sampling is not supported")
    if repetition_penalty not in (1, 1.0, None):
        raise ValueError(f"repetition_penalty={repetition_penalty!r}: a penalty cannot be combined with beams")
    return int(num_beams), float(lp)


def beam_keep(num_beams, num_eos):
    """K: the candidates HF keeps per image and step, max(2, 1 + number of EOS ids) * num_beams."""
    return max(2, 1 + int(num_eos)) * int(num_beams)


def beam_length_divisor(i, length_penalty):
    """What a hypothesis of i + 1 generated tokens is divided by: (i + 1) ** length_penalty in float64, rounded ONCE to fp32 -- the
    value HF's fp32 tensor division sees and the one the select kernel is handed."""
    return float(torch.tensor(float(i + 1) ** float(length_penalty), dtype=torch.float64).to(torch.float32))


def _ulp32(x):
    """Spacing of fp32 at magnitude |x| (float64 tensor in, float64 tensor out); the smallest normal spacing below that range."""
    a = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def _near(a, b, ulps):
    """Is the pair (a, b) of float64 scores separated by more than nothing and by at most `ulps` fp32 ulp of the larger magnitude?"""
    if not (torch.isfinite(a) and torch.isfinite(b)) or a == b:
        return False
    return bool((a - b).abs() <= ulps * _ulp32(torch.maximum(a.abs(), b.abs())))


def beam_init_state(B, k, n, pad):
    """The state of B images before select 0: running scores (0, -1e9, ...), per-beam tokens, the finished pool (scores -1e9, flags
    false, sequences of pad ids, lengths 0) and `open`; all CPU tensors."""
    running = torch.full((B, k), BEAM_NEG, dtype=torch.float64)
    running[:, 0] = 0.0
    return {"running": running, "tokens": torch.full((B, k, n), int(pad), dtype=torch.int64),
            "pool_score": torch.full((B, k), BEAM_NEG, dtype=torch.float64), "pool_fin": torch.zeros((B, k), dtype=torch.bool),
            "pool_seq": torch.full((B, k, n), int(pad), dtype=torch.int64), "pool_len": torch.zeros((B, k), dtype=torch.int64),
            "open": torch.ones(B, dtype=torch.bool)}


def beam_step_law(state, logits, i, n, min_new, eos_ids, pad, length_penalty=1.0, ulps=(2.0, 3.0)):
    """One beam-search select, HF 5.x `_beam_search` with do_sample=False, early_stopping=False, num_return_sequences=1 and no prompt
    ids, on the fp32 logits [B, k, V] of the k beams of B images at step i of n, evaluated in float64:
      1. lp = l - logsumexp(l) per beam row; the EOS columns then read -inf while i < min_new (the processor runs after the
         log-softmax, so the normaliser includes the EOS mass);   2. c = running + lp;
      3. the top K = max(2, 1 + E) k of the flat [k V] array by value descending, then by lowest flat index j V + v;
      4. fin_r = (token is an EOS id) or (i == n - 1);
      5. the next running beams are the first k ranks in the order (fin ascending, rank ascending): score, parent's tokens + token;
      6. while `open`, every rank r < k with fin_r enters the pool with score s_r / d, d = `beam_length_divisor(i, length_penalty)`; the
         pool keeps the best k of old slots + entrants, old slots first on ties, then by rank;
      7. open &= running'[0] / d > worst, worst = the smallest pool score when all k slots are finished, else -1e9.
    `state` (`beam_init_state`, or a state this function returned; fp32 scores are read as float64) is not modified.  Returns the new
    state with, besides its fields, parents [B, k] (the beam each new beam continues), next_tokens [B, k], and near [B] bool: some pair of
    scores the select COMPARES (neighbours among the first K + 1 sorted candidates: `ulps[0]` fp32 ulp; an entrant against a pool
    score or another entrant, and step 7: `ulps[1]`) differs by less than what fp32 arithmetic can resolve -- such an image may
    legitimately come out differently from an fp32 evaluation."""
    l = torch.as_tensor(logits).detach().cpu().to(torch.float64)
    B, k, V = l.shape
    eos = [int(e) for e in eos_ids]
    K = beam_keep(k, len(eos))
    # K + E columns: with the EOS columns masked, beam 0 alone still fills select 0's top K, so the -1e9 beams never enter it
    assert V >= K + len(eos), f"vocabulary {V} < K + E = {K + len(eos)}"
    lp = l - torch.logsumexp(l, dim=-1, keepdim=True)
    if i < int(min_new):
        for e in eos:
            if 0 <= e < V:
                lp[:, :, e] = float("-inf")
    run = state["running"].detach().cpu().to(torch.float64)
    c = (run[:, :, None] + lp).reshape(B, k * V)
    d = torch.tensor(beam_length_divisor(i, length_penalty), dtype=torch.float64)
    last = i == n - 1
    out = {key: val.detach().cpu().clone() for key, val in state.items() if key in
           ("running", "tokens", "pool_score", "pool_fin", "pool_seq", "pool_len", "open")}
    out["running"] = out["running"].to(torch.float64)
    out["pool_score"] = out["pool_score"].to(torch.float64)
    out["parents"] = torch.zeros((B, k), dtype=torch.int64)
    out["next_tokens"] = torch.zeros((B, k), dtype=torch.int64)
    out["near"] = torch.zeros(B, dtype=torch.bool)
    for b in range(B):
        vals, idx = torch.sort(c[b], descending=True, stable=True)         # equal values keep ascending flat index
        take = min(K + 1, k * V)
        near = any(_near(vals[r], vals[r + 1], ulps[0]) for r in range(take - 1))
        s, par, tok = vals[:K], (idx[:K] // V).tolist(), (idx[:K] % V).tolist()
        fin = [bool(t in eos or last) for t in tok]
        order = [r for r in range(K) if not fin[r]] + [r for r in range(K) if fin[r]]
        old_tokens = state["tokens"][b]
        for q, r in enumerate(order[:k]):
            out["running"][b, q] = s[r]
            out["tokens"][b, q] = old_tokens[par[r]]
            out["tokens"][b, q, i] = tok[r]
            out["parents"][b, q] = par[r]
            out["next_tokens"][b, q] = tok[r]
        if bool(state["open"][b]):
            old_s = state["pool_score"][b].to(torch.float64)
            merged = [(old_s[j], ("old", j)) for j in range(k)] + [(s[r] / d, ("new", r)) for r in range(k) if fin[r]]
            for a in range(k, len(merged)):
                near = near or any(_near(merged[a][0], merged[o][0], ulps[1]) for o in range(len(merged)) if o != a)
            picked = sorted(range(len(merged)), key=lambda m: (-float(merged[m][0]), m))[:k]     # stable: old first, then by rank
            for q, m in enumerate(picked):
                score, (kind, j) = merged[m]
                out["pool_score"][b, q] = score
                if kind == "old":
                    out["pool_fin"][b, q] = state["pool_fin"][b, j]
                    out["pool_seq"][b, q] = state["pool_seq"][b, j]
                    out["pool_len"][b, q] = state["pool_len"][b, j]
                else:
                    out["pool_fin"][b, q] = True
                    out["pool_seq"][b, q] = old_tokens[par[j]]
                    out["pool_seq"][b, q, i] = tok[j]
                    out["pool_seq"][b, q, i + 1:] = int(pad)
                    out["pool_len"][b, q] = i + 1
        worst = out["pool_score"][b].min() if bool(out["pool_fin"][b].all()) else torch.tensor(BEAM_NEG, dtype=torch.float64)
        best = out["running"][b, 0] / d
        near = near or (bool(state["open"][b]) and _near(best, worst, ulps[1]))
        out["open"][b] = bool(state["open"][b]) and bool(best > worst)
        out["near"][b] = near
    return out


def beam_decode_law(logits_fn, B, k, n, min_new, eos_ids, pad, length_penalty=1.0, ulps=(2.0, 3.0)):
    """The whole beam search of B images: `logits_fn(tokens [B, k, i] int64) -> logits [B, k, V]` gives the next-token logits of
    every beam after its i generated tokens (i = 0: after the prompt alone; every beam of an image then gets the same row, and only
    beam 0 counts).  n selects of `beam_step_law` -> (tokens [B, n] int64: pool slot 0's sequence, EOS included, then pad ids;
    scores [B] float64: its score, HF's `sequences_scores`; near [B] bool: some select of the image compared a near-tied pair; the
    list of the n states).  An image that is no longer `open` keeps its pool, which is why a loop of fixed length gives what HF's loop
    gives, whose exit is global to the batch."""
    state = beam_init_state(B, k, n, pad)
    near = torch.zeros(B, dtype=torch.bool)
    trace = []
    for i in range(n):
        state = beam_step_law(state, logits_fn(state["tokens"][:, :, :i]), i, n, min_new, eos_ids, pad, length_penalty, ulps)
        near |= state["near"]
        trace.append(state)
    return state["pool_seq"][:, 0].clone(), state["pool_score"][:, 0].clone(), near, trace
