"""early_stop=True on the native LLaMA engine (cgpt_llm_set_early_stop): once every row of a greedy call has
produced an EOS, the remaining token steps do no work.  What is checked, always against the SAME call with early stop off:
tokens bit-equal; cgpt_llm_live_steps = the rule of tests/test_llm_early_stop_cpu.py applied to the off run's tokens; the dead part of
the call left the cache and the step logits untouched (sentinels) and the live part wrote what the off run wrote, bit for bit.

The exact finishing step comes from a synthetic law that needs no trained model: lm_head is zeroed (the layers stay random), so every
logit is 0 and the first-max arg-max is token 0; with eos = [0] and min_new = F the select picks token 1 while EOS is masked and
token 0 -- EOS, for every row -- at select F."""
import ctypes as C
import dataclasses

import pytest
import torch

from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import MiniGPT4Classifier, WordHashTokenizer, _HipDecoder
from oracle import model_oracle as mo
from gpu_util import DEV, make_classifier
import llm_util as lu
from llm_util import LOGIT_SENTINEL, PROMPT
from test_llm_early_stop_cpu import expected_live_steps, finishing_select

pytestmark = pytest.mark.gpu


def _greedy(dec, on, first, L, n, min_new, eos, pad, kb, vb, logits=False, starts=None):
    """One greedy call on clones of the caches, early stop `on`: (tokens, live_steps, K, V, step logits or None).  The step logits
    buffer is the caller-visible one of the C entry, filled with a sentinel beforehand."""
    kb, vb = [t.clone() for t in kb], [t.clone() for t in vb]
    B, V = first.shape
    dec.set_early_stop(on)
    try:
        if logits:                                                     # dec.greedy allocates its own buffer: go through the C entry
            tokens = torch.full((B, n), -7, dtype=torch.int64, device=DEV)
            buf = torch.full((B, n, V), LOGIT_SENTINEL, dtype=torch.float32, device=DEV)
            kp, vp, stride = dec._cache_tables(kb, vb, B, L + n - 1)
            ids = (C.c_int64 * max(1, len(eos)))(*eos)
            st = torch.cuda.current_stream()
            dec._greedy_ran = True
            assert starts is None
            rc = dec.L.cgpt_llm_greedy(dec.handle, C.c_void_p(first.data_ptr()), B, L, n, min_new, ids, len(eos), pad, kp, vp, stride,
                                       C.c_void_p(tokens.data_ptr()), C.c_void_p(buf.data_ptr()), C.c_void_p(st.cuda_stream))
            assert rc == 0, dec.L.cgpt_last_error()
        else:
            buf = None
            tokens = dec.greedy(first, L, n, min_new, eos, pad, kb, vb, starts=starts)
        steps = dec.live_steps()
    finally:
        dec.set_early_stop(False)
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


# ------------------------------------------------------------------------------------------ 1. exact finishing step
@pytest.mark.parametrize("min_new, want", [(0, 0), (3, 3), (7, 7), (8, 7)])
def test_exact_finishing_step_small_decoder(zero_small, min_new, want):
    llm, dec = zero_small
    B, L, n = 37, 12, 8
    first, kb, vb, _ = lu.prefill(llm, llm.get_input_embeddings()(lu.ids(llm, B, L, 3)), n)      # the model's own prefill
    assert bool((first == 0).all())
    off = _greedy(dec, False, first, L, n, min_new, [0], 0, kb, vb, logits=True)
    on = _greedy(dec, True, first, L, n, min_new, [0], 0, kb, vb, logits=True)
    want_tokens = torch.zeros(B, n, dtype=torch.int64, device=DEV)
    want_tokens[:, :min_new] = 1
    assert torch.equal(off[0], want_tokens)                            # the law of the module docstring
    assert torch.equal(on[0], off[0])
    assert off[1] == n - 1 and on[1] == want == expected_live_steps(off[0], [0])
    lu.check_dead_part(L, want, on, off)
    # the same without step logits (the engine's own logits buffer)
    on2 = _greedy(dec, True, first, L, n, min_new, [0], 0, kb, vb)
    assert torch.equal(on2[0], off[0]) and on2[1] == want
    lu.check_dead_part(L, want, on2, off[:4] + (None,))


# ------------------------------------------------------------------------------------------ 2. + 3. staggered finish on natural rows
def _staggered(dec, first, L, n, kb, vb, starts=None):
    B = first.shape[0]
    T = _greedy(dec, False, first, L, n, 0, [], 0, kb, vb, starts=starts)[0]       # no EOS id: the natural rows
    eos = sorted({int(T[b, b + 1]) for b in range(B)})
    assert 1 <= len(eos) <= 8
    off = _greedy(dec, False, first, L, n, 0, eos, 0, kb, vb, starts=starts)
    # rows are independent and deterministic: row b repeats T[b] up to its first EOS, which is at column b + 1 at the latest
    F = finishing_select(off[0], eos)
    assert F <= B < n - 1, (F, off[0].tolist(), eos)
    on = _greedy(dec, True, first, L, n, 0, eos, 0, kb, vb, starts=starts)
    assert torch.equal(on[0], off[0])
    assert off[1] == n - 1 and on[1] == expected_live_steps(off[0], eos) == F
    lu.check_dead_part(L, F, on, off)
    return F


def test_staggered_finish_on_natural_rows(small):
    llm, dec = small
    B, L, n = 5, 12, 8
    kb, vb = lu.sentinel_cache(dec.layers, dec.heads, B, L + n)
    first = dec.prefill(llm.get_input_embeddings()(lu.ids(llm, B, L, 4)).contiguous(), kb, vb)
    _staggered(dec, first, L, n, kb, vb)


def test_staggered_finish_on_left_padded_rows(small):
    llm, dec = small
    B, L, n = 5, 12, 8
    starts = torch.tensor([0, 1, 5, 11, 3], dtype=torch.int32, device=DEV)
    embs = llm.get_input_embeddings()(lu.ids(llm, B, L, 4)).clone()
    for b, s in enumerate(starts.tolist()):
        embs[b, :s] = 0
    kb, vb = lu.sentinel_cache(dec.layers, dec.heads, B, L + n)
    first = dec.prefill(embs.contiguous(), kb, vb, starts=starts)
    _staggered(dec, first, L, n, kb, vb, starts=starts)


# ------------------------------------------------------------------------------------------ 4. int8 handle
def test_int8_handle(zero_small):
    llm, _ = zero_small
    dec = _HipDecoder(llm, 64, weights="int8")
    try:
        B, L, n = 37, 12, 8
        kb, vb = lu.sentinel_cache(dec.layers, dec.heads, B, L + n)
        first = dec.prefill(llm.get_input_embeddings()(lu.ids(llm, B, L, 3)).contiguous(), kb, vb)
        off = _greedy(dec, False, first, L, n, 3, [0], 0, kb, vb)
        on = _greedy(dec, True, first, L, n, 3, [0], 0, kb, vb)
        assert torch.equal(on[0], off[0]) and on[1] == 3 == expected_live_steps(off[0], [0]) and off[1] == n - 1
        lu.check_dead_part(L, 3, on, off)
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------ 5. one capture, several finishing steps
def test_one_capture_serves_every_finishing_step(zero_small):
    llm, dec = zero_small
    B, L, n = 37, 12, 8
    first0, kb, vb, _ = lu.prefill(llm, llm.get_input_embeddings()(lu.ids(llm, B, L, 3)), n)
    late = first0.clone()
    late[:, 5] = 1.0                                                   # select 0 picks token 5, the zero logits of step 1 give EOS: F = 1
    at_once = first0.clone()
    at_once[:, 0] = 1.0e4                                              # the EOS column scaled up: every row finishes at select 0
    eager = {name: (_greedy(dec, False, f, L, n, 0, [0], 0, kb, vb), _greedy(dec, True, f, L, n, 0, [0], 0, kb, vb))
             for name, f in (("late", late), ("at_once", at_once))}
    assert eager["late"][1][1] == 1 and eager["at_once"][1][1] == 0
    static_first = late.clone()
    k2, v2 = [t.clone() for t in kb], [t.clone() for t in vb]
    dec.set_early_stop(True)
    try:
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            t_g = dec.greedy(static_first, L, n, 0, [0], 0, k2, v2)
    finally:
        dec.set_early_stop(False)                                      # the handle says off from here on: the graph keeps what it captured

    def replay(contents):
        static_first.copy_(contents)
        for k, v, k0, v0 in zip(k2, v2, kb, vb):
            k.copy_(k0)
            v.copy_(v0)
        t_g.fill_(-7)
        graph.replay()
        return t_g.clone(), dec.live_steps(), [t.clone() for t in k2], [t.clone() for t in v2], None

    for name in ("late", "at_once", "late"):
        off, on = eager[name]
        got = replay(late if name == "late" else at_once)
        assert torch.equal(got[0], off[0]) and got[1] == on[1] == expected_live_steps(off[0], [0]), name
        lu.check_dead_part(L, on[1], got, off)
    del graph


# ------------------------------------------------------------------------------------------ 6. Vicuna width
def test_vicuna_width():
    llm = lu.zero_head(lu.vicuna_width_decoder())
    dec = _HipDecoder(llm, 200)
    try:
        B, L, n = 200, 44, 6
        kb, vb = lu.sentinel_cache(dec.layers, dec.heads, B, L + n)
        first = dec.prefill(llm.get_input_embeddings()(lu.ids(llm, B, L, 3)).contiguous(), kb, vb)
        off = _greedy(dec, False, first, L, n, 2, [0], 0, kb, vb)
        on = _greedy(dec, True, first, L, n, 2, [0], 0, kb, vb)
        assert torch.equal(on[0], off[0]) and on[1] == 2 == expected_live_steps(off[0], [0]) and off[1] == n - 1
        lu.check_dead_part(L, 2, on, off, layers=(0, 1))
    finally:
        dec.close()
        del llm
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------ 7. classifier
@pytest.mark.parametrize("extra", [dict(), dict(weights="int8", ragged="hip", prompt_bucket=16), dict(prefill="model")],
                         ids=["plain", "int8-bucketed", "model-prefill"])
def test_classifier_answers_and_live_steps(small, extra):
    llm, _ = small
    cfg = dataclasses.replace(mo.tiny_config(mode=mo.MODE_ENCODE_IMG), proj_dim=512)
    enc = make_classifier(cfg, max_batch=8)
    gen = llm.generation_config
    saved = gen.eos_token_id
    try:
        enc.init_synthetic(seed=0)
        x = torch.from_numpy(mo.synthetic_image(cfg, seed=11)).to(DEV)
        emb = enc.encode_img_noisy(x, 0, 8, 0.5, 42).to(torch.float16)
        n, tok = 8, WordHashTokenizer(320)
        kw = dict(max_new_tokens=n, max_batch=8, decode="hip", generate_kwargs=dict(min_length=0))
        kw.update(dict(prefill="hip"), **extra)

        def run(early_stop):
            clf = MiniGPT4Classifier(enc, llm, tok, PROMPT, AnswerLabelMap(4, ()), early_stop=early_stop, **kw)
            seen, inner = [], clf._generate_graph
            clf._generate_graph = lambda e, s=None: seen.append(inner(e, s)) or seen[-1]
            answers = clf.generate_from_embeds(emb, PROMPT)
            again = clf.generate_from_embeds(emb, PROMPT)                  # a replay of the captured graph
            assert again == answers and torch.equal(seen[0], seen[1])
            s = clf.decode_stats
            assert s["hf_calls"] == 0 and s["graph_captures"] == 1 and s["graph_replays"] == 2 and s["hip_steps"] == 2 * (n - 1)
            return answers, seen[1], clf.last_live_steps()

        gen.eos_token_id = []                                              # the natural rows, then a staggered EOS set as in test 2
        T = run(False)[1]
        eos = sorted({int(T[b, b % 4 + 1]) for b in range(8)})
        gen.eos_token_id = eos
        a_off, t_off, live_off = run(False)
        a_on, t_on, live_on = run(True)
        assert finishing_select(t_off, eos) <= 4 < n - 1
        assert a_on == a_off and torch.equal(t_on, t_off)
        assert live_off == n - 1 and live_on == expected_live_steps(t_off, eos)
    finally:
        gen.eos_token_id = saved
        enc.close()
