"""Per-row stop sequences on the native LLaMA engine (cgpt_llm_set_stop_sequences) and through the classifier.

The oracle, everywhere and without any tolerance: greedy rows are independent, so a decode WITH stop sequences equals
`apply_stop_sequences` (certifiedgpt_amd/llm_laws.py, pinned on the CPU by tests/test_llm_stop_cpu.py) applied to the SAME decode
without them, bit for bit; the step logits of every select up to a row's finishing column are that decode's; and with early stop on,
cgpt_llm_live_steps = min(F, n - 1) with F = the last row's finishing column, the dead part of the call leaving the cache and the
step logits untouched (the sentinel pattern of tests/test_gpu_llm_early_stop.py).

The exact finishing step comes from a synthetic law that needs no trained model: lm_head is zeroed, so every logit is 0 and every
token is 0; with no EOS id and the sequence "k zeros" every row finishes at column k - 1."""
import ctypes as C

import pytest
import torch

from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import (MiniGPT4Classifier, WordHashTokenizer, _HipDecoder, apply_stop_sequences,
                                       stop_finish_columns)
from gpu_util import DEV
import llm_util as lu
from llm_util import LOGIT_SENTINEL, PROMPT

pytestmark = pytest.mark.gpu


def _greedy(dec, on, seqs, first, L, n, eos, pad, kb, vb, logits=False, starts=None, tokens_init=None):
    """One greedy call on clones of the caches, stop sequences `seqs` (None: none) and early stop `on`:
    (tokens, live_steps, K, V, step logits or None).  With `logits` (or `tokens_init`: what the token table holds beforehand) the call
    goes through the C entry on caller-visible buffers, the step logits filled with a sentinel."""
    kb, vb = [t.clone() for t in kb], [t.clone() for t in vb]
    B, V = first.shape
    dec.set_stop_sequences(seqs)
    dec.set_early_stop(on)
    try:
        if logits or tokens_init is not None:
            tokens = torch.full((B, n), -7, dtype=torch.int64, device=DEV) if tokens_init is None else tokens_init.clone()
            buf = torch.full((B, n, V), LOGIT_SENTINEL, dtype=torch.float32, device=DEV) if logits else None
            kp, vp, stride = dec._cache_tables(kb, vb, B, L + n - 1)
            ids = (C.c_int64 * max(1, len(eos)))(*eos)
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            dec._greedy_ran = True
            tail = (n, 0, ids, len(eos), pad, kp, vp, stride, C.c_void_p(tokens.data_ptr()), C.c_void_p(buf.data_ptr()) if logits else None, st)
            if starts is None:
                rc = dec.L.cgpt_llm_greedy(dec.handle, C.c_void_p(first.data_ptr()), B, L, *tail)
            else:
                rc = dec.L.cgpt_llm_greedy_ragged(dec.handle, C.c_void_p(first.data_ptr()), B, L, dec._starts_ptr(starts, B), *tail)
            assert rc == 0, dec.L.cgpt_last_error()
        else:
            buf = None
            tokens = dec.greedy(first, L, n, 0, eos, pad, kb, vb, starts=starts)
        steps = dec.live_steps()
    finally:
        dec.set_early_stop(False)
        dec.set_stop_sequences(None)
    return tokens, steps, kb, vb, buf


@pytest.fixture(scope="module")
def zero_small():
    llm = lu.zero_head(lu.small_decoder())
    dec = _HipDecoder(llm, 64)
    yield llm, dec
    dec.close()


@pytest.fixture(scope="module")
def small():
    llm = lu.small_decoder()
    dec = _HipDecoder(llm, 64)
    yield llm, dec
    dec.close()


@pytest.fixture(scope="module")
def natural(small):
    """B = 37 rows of the small decoder after the native prefill, and T = the engine's own 12 tokens per row without stop sequences
    and without EOS ids: computed once, shared, never changed."""
    llm, dec = small
    B, L, n = 37, 12, 12
    kb, vb = lu.sentinel_cache(dec.layers, dec.heads, B, L + n)
    first = dec.prefill(llm.get_input_embeddings()(lu.ids(llm, B, L, 4)).contiguous(), kb, vb)
    plain = _greedy(dec, False, None, first, L, n, [], 5, kb, vb, logits=True)
    assert plain[1] == n - 1
    return dec, first, L, n, kb, vb, plain


def _natural_seqs(T):
    """One, two, three and eight tokens, each from a different row of T."""
    return [[int(T[0, 3])], T[1, 5:7].tolist(), T[2, 6:9].tolist(), T[3, 2:10].tolist()]


# ------------------------------------------------------------------------------------------ 1. exact finishing step
@pytest.mark.parametrize("k", [1, 3, 8])
def test_exact_finishing_step_on_the_synthetic_law(zero_small, k):
    llm, dec = zero_small
    B, L, n, pad = 37, 12, 10, 5
    first, kb, vb, _ = lu.prefill(llm, llm.get_input_embeddings()(lu.ids(llm, B, L, 3)), n)      # the model's own prefill
    assert bool((first == 0).all())
    seqs = [[0] * k]
    off = _greedy(dec, False, seqs, first, L, n, [], pad, kb, vb, logits=True)
    on = _greedy(dec, True, seqs, first, L, n, [], pad, kb, vb, logits=True)
    want = torch.full((B, n), pad, dtype=torch.int64, device=DEV)
    want[:, :k] = 0
    assert torch.equal(off[0], want)                                   # the law of the module docstring
    assert torch.equal(off[0], apply_stop_sequences(torch.zeros_like(want), [], seqs, pad))
    assert torch.equal(on[0], off[0])
    assert off[1] == n - 1 and on[1] == k - 1
    lu.check_dead_part(L, k - 1, on, off)
    on2 = _greedy(dec, True, seqs, first, L, n, [], pad, kb, vb)        # the same without step logits (the engine's own buffer)
    assert torch.equal(on2[0], off[0]) and on2[1] == k - 1
    lu.check_dead_part(L, k - 1, on2, off[:4] + (None,))
    none = _greedy(dec, True, None, first, L, n, [], pad, kb, vb)       # cleared: nothing ever stops, as before the entry existed
    assert bool((none[0] == 0).all()) and none[1] == n - 1


# ------------------------------------------------------------------------------------------ 2. + 4. natural rows
def _natural_rows(dec, first, L, n, kb, vb, plain, starts=None):
    T, pad, B = plain[0], 5, first.shape[0]
    seqs = _natural_seqs(T)
    cols = stop_finish_columns(T, [], seqs)
    one_token = stop_finish_columns(T, [], seqs[:1])
    print("finishing columns:", cols, "\nby the one-token sequence alone:", one_token)
    finished = [c for c in cols if c < n]
    assert len(set(finished)) >= 3, cols                                # preconditions, from the rule on T
    assert any(c < o for c, o in zip(cols, one_token)), (cols, one_token)     # a row finished by a sequence longer than one token
    assert len(finished) < B, cols                                      # and a row that never finishes
    got = _greedy(dec, False, seqs, first, L, n, [], pad, kb, vb, logits=True, starts=starts)
    assert torch.equal(got[0], apply_stop_sequences(T, [], seqs, pad))
    assert got[1] == n - 1
    for b, c in enumerate(cols):                                       # every select up to the finishing column saw the off run's logits
        assert torch.equal(got[4][b, :c + 1], plain[4][b, :c + 1]), (b, c)
    # with EOS ids on top, staggered as in the early-stop tests -- a later column for a later row -- over the rows after those that
    # supply the sequences, leaving out ids that would finish one of those four before its sequence does
    kept = {int(t) for b in range(4) for t in T[b, :cols[b] + 1].tolist()}
    eos = []
    for j, b in enumerate(range(4, B)):
        t = int(T[b, j % (n - 1) + 1])
        if t not in kept and t not in eos and len(eos) < 5:
            eos.append(t)
    eos.sort()
    assert 1 <= len(eos) <= 8
    T_eos = _greedy(dec, False, None, first, L, n, eos, pad, kb, vb, starts=starts)[0]
    want = apply_stop_sequences(T_eos, eos, seqs, pad)
    assert torch.equal(want, apply_stop_sequences(T, eos, seqs, pad))   # the rule holds the EOS rule: either table gives the same
    cols_eos = stop_finish_columns(T, eos, seqs)
    assert cols_eos != cols and cols_eos != stop_finish_columns(T, eos, [])     # both kinds of finish decide some row
    got_eos = _greedy(dec, False, seqs, first, L, n, eos, pad, kb, vb, starts=starts)
    assert torch.equal(got_eos[0], want)
    return seqs, cols


def test_natural_rows(natural):
    dec, first, L, n, kb, vb, plain = natural
    _natural_rows(dec, first, L, n, kb, vb, plain)


def test_natural_rows_left_padded(small):
    llm, dec = small
    B, L, n = 37, 12, 12
    g = torch.Generator(device="cpu").manual_seed(9)
    starts = torch.randint(0, L, (B,), generator=g).to(torch.int32)
    starts[:4] = torch.tensor([0, 11, 5, 1], dtype=torch.int32)
    starts = starts.to(DEV)
    embs = llm.get_input_embeddings()(lu.ids(llm, B, L, 4)).clone()
    for b, s in enumerate(starts.tolist()):
        embs[b, :s] = 0
    kb, vb = lu.sentinel_cache(dec.layers, dec.heads, B, L + n)
    first = dec.prefill(embs.contiguous(), kb, vb, starts=starts)
    plain = _greedy(dec, False, None, first, L, n, [], 5, kb, vb, logits=True, starts=starts)
    _natural_rows(dec, first, L, n, kb, vb, plain, starts=starts)


# ------------------------------------------------------------------------------------------ 3. no look-back before column 0
def test_no_look_back_before_column_0(natural):
    dec, first, L, n, kb, vb, plain = natural
    T, pad, B = plain[0], 5, first.shape[0]
    # row b - 1's last token followed by row b's first: adjacent in the [B, n] table, and no match at column 0.  The table holds T
    # beforehand, so a select 0 that looked one entry back from row b's column 0 would find exactly that pair and finish row b there.
    # b: a row the rule lets run on past column 1 with a token other than the pad id there, so that such a finish would show.
    pairs = [(b, [int(T[b - 1, n - 1]), int(T[b, 0])]) for b in range(1, B)]
    b, seq = next((b, s) for b, s in pairs if stop_finish_columns(T, [], [s])[b] > 1 and int(T[b, 1]) != pad)
    cols = stop_finish_columns(T, [], [seq])
    want = apply_stop_sequences(T, [], [seq], pad)
    assert cols[b] != 0 and int(want[b, 1]) == int(T[b, 1]) != pad
    got = _greedy(dec, False, [seq], first, L, n, [], pad, kb, vb, tokens_init=T)
    assert torch.equal(got[0], want)
    got = _greedy(dec, True, [seq], first, L, n, [], pad, kb, vb, tokens_init=T)
    assert torch.equal(got[0], want) and got[1] == min(max(cols), n - 1)


# ------------------------------------------------------------------------------------------ 5. early stop on natural rows
def test_early_stop_on_natural_rows(natural):
    dec, first, L, n, kb, vb, plain = natural
    pad = 5
    first4, kb4, vb4 = first[:4].contiguous(), [t[:4].contiguous() for t in kb], [t[:4].contiguous() for t in vb]
    T = _greedy(dec, False, None, first4, L, n, [], pad, kb4, vb4)[0]       # the four-row batch's own tokens without sequences
    seqs = [[int(T[0, 1])], T[1, 2:4].tolist(), T[2, 3:6].tolist(), T[3, 0:8].tolist()]       # every row supplies one: all finish
    cols = stop_finish_columns(T, [], seqs)
    print("finishing columns:", cols)
    F = max(cols)
    assert F <= 7 < n - 1 and len(set(cols)) >= 2, cols
    off = _greedy(dec, False, seqs, first4, L, n, [], pad, kb4, vb4, logits=True)
    on = _greedy(dec, True, seqs, first4, L, n, [], pad, kb4, vb4, logits=True)
    assert torch.equal(off[0], apply_stop_sequences(T, [], seqs, pad)) and torch.equal(on[0], off[0])
    assert off[1] == n - 1 and on[1] == min(F, n - 1)
    lu.check_dead_part(L, F, on, off)


# ------------------------------------------------------------------------------------------ 6. classifier
def test_classifier_graph_replays(small):
    llm, _ = small
    gen = llm.generation_config
    saved = gen.eos_token_id
    try:
        # image embeds with the spread of the embedding table (the tiny encoder's rows all decode alike): rows that differ
        embs = [llm.get_input_embeddings()(lu.ids(llm, 8, 6, seed)) for seed in (21, 22)]
        n, tok, pad = 8, WordHashTokenizer(320), 0
        gen.eos_token_id = []                                              # the natural rows
        kw = dict(max_new_tokens=n, max_batch=8, generate_kwargs=dict(min_length=0))

        def run(**extra):
            clf = MiniGPT4Classifier(None, llm, tok, PROMPT, AnswerLabelMap(4, ()), **kw, **extra)
            seen, inner = [], clf._generate_graph
            clf._generate_graph = lambda e, s=None: seen.append(inner(e, s)) or seen[-1]
            answers = [clf.generate_from_embeds(e, PROMPT) for e in embs]   # one capture, two replays on different embeds
            s = clf.decode_stats
            assert s["hf_calls"] == 0 and s["graph_captures"] == 1 and s["graph_replays"] == 2, s
            return clf, answers, seen

        for engine in (dict(decode="hip", prefill="hip"), dict(decode="graph")):
            early = dict(early_stop=True) if engine["decode"] == "hip" else {}
            off, a_off, T = run(**engine)
            assert not torch.equal(T[0], T[1])
            seqs = [[int(T[0][0, 5])], T[0][1, 2:4].tolist(), [int(T[1][2, 6])], T[1][3, 2:5].tolist()]
            text = "w%d" % int(T[0][4, 2])                                 # WordHashTokenizer decodes id k to the word "w<k>"
            want = [apply_stop_sequences(t, [], seqs, pad) for t in T]
            cols = [stop_finish_columns(t, [], seqs) for t in T]
            print(engine, "finishing columns:", cols)
            assert all(min(c) < n - 1 for c in cols) and any(c == n for c in cols[0] + cols[1]), cols
            on, a_on, got = run(stop_words_ids=seqs, stop_text=text, **engine, **early)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), engine
            assert a_on == [on._decode_outputs(w) for w in want] and a_on != a_off
            assert text in " ".join(a_off[0]) and text not in " ".join(a_on[0])
            if early:                                                      # the last replay: the steps the rule says ran
                assert on.last_live_steps() == min(max(cols[1]), n - 1) and off.last_live_steps() == n - 1
    finally:
        gen.eos_token_id = saved


# ------------------------------------------------------------------------------------------ 7. Vicuna width
def test_vicuna_width():
    llm = lu.vicuna_width_decoder()
    dec = _HipDecoder(llm, 8)
    try:
        B, L, n, pad = 8, 12, 6, 5
        kb, vb = lu.sentinel_cache(dec.layers, dec.heads, B, L + n)
        first = dec.prefill(llm.get_input_embeddings()(lu.ids(llm, B, L, 3)).contiguous(), kb, vb)
        T = _greedy(dec, False, None, first, L, n, [], pad, kb, vb)[0]
        assert int(T.max()) >= 320                                         # the select at vocabulary 32 000: ids beyond the small one's
        seqs = [[int(T[0, 1])], T[1, 1:3].tolist(), T[2, 0:3].tolist()]
        cols = stop_finish_columns(T, [], seqs)
        print("finishing columns:", cols)
        assert min(cols) < n - 1 and len(set(cols)) >= 2, cols
        off = _greedy(dec, False, seqs, first, L, n, [], pad, kb, vb)
        on = _greedy(dec, True, seqs, first, L, n, [], pad, kb, vb)
        assert torch.equal(off[0], apply_stop_sequences(T, [], seqs, pad)) and torch.equal(on[0], off[0])
        assert off[1] == n - 1 and on[1] == min(max(cols), n - 1)
    finally:
        dec.close()
        del llm
        torch.cuda.empty_cache()
