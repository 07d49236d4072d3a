"""Trie-constrained answer decoding on the native LLaMA engine (classify="constrained", constrain="hip"; csrc/llm_trie.hip; DESIGN.md
4.4.12).  The law is `constrained_select_law` / `constrained_decode_law` (llm_laws.py), and every comparison with it is bit for bit:
the kernel alone on hand-made tries, the loop after both prefills on the logits it read itself, early stop, left padding, the
engine's other modes, the label vote, and the refusals.  Against HF `generate(prefix_allowed_tokens_fn=...)` the classifier is held to
the project's margin rule (`greedy_decode_parity`): the two run different GEMMs, so only rows HF itself decides by more than the
measured logit noise must agree."""
import ctypes as C
import dataclasses
import random

import pytest
import torch

from certifiedgpt_amd import _lib
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.classifier import vote_labels
from certifiedgpt_amd.llm_laws import (act_int8_twin, allowed_tokens_fn, build_answer_trie, constrained_decode_law,
                                       constrained_select_law, expand_kv_state_dict, greedy_decode_parity, trie_walk)
from certifiedgpt_amd.minigpt4 import MiniGPT4Classifier, WordHashTokenizer, _HipDecoder
from oracle import model_oracle as mo
from gpu_util import DEV, make_classifier
import llm_util as lu
from llm_util import K_SENTINEL, LOGIT_SENTINEL, PAD, PROMPT, V_SENTINEL

pytestmark = pytest.mark.gpu


def P(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------ 1. the kernel alone
# the lane (1, 2), wave (63, 64, 65), workgroup-stride (255, 256, 257) and several-strides (1000) boundaries of the 256-thread scan
FANS = (1, 2, 63, 64, 65, 255, 256, 257, 1000)


def fan_trie(vocab, seed):
    """Root edge i + 1 leads to node i + 1, whose fan-out is min(FANS[i], vocab) leaves (a node cannot have more edges than the
    vocabulary has tokens: at vocab 320 the last node carries every token).  Edge tokens are a seeded sample that always holds
    token 0 and token vocab - 1 when the fan-out is 2 or more.  -> (trie, fans)."""
    rng = random.Random(seed)
    seqs, fans = [], []
    for i, f in enumerate(FANS):
        f = min(f, vocab)
        toks = {0, vocab - 1} if f >= 2 else {rng.randrange(vocab)}
        while len(toks) < f:
            toks.add(rng.randrange(vocab))
        seqs += [(i + 1, t) for t in sorted(toks)]
        fans.append(f)
    trie = build_answer_trie(seqs, vocab)
    begin = trie.child_begin.tolist()
    assert [begin[n + 1] - begin[n] for n in range(1, len(FANS) + 1)] == fans and begin[1] == len(FANS)
    return trie, fans


def kernel_select(logits, node, unfinished, trie_dev, nodes, pad):
    """cgpt_llm_trie_select_logits on buffers with a sentinel element on either side of what the kernel may write."""
    B, V = logits.shape
    L = _lib.lib()
    bufs = {"node": torch.full((B + 2,), -77, dtype=torch.int32, device=DEV), "unf": torch.full((B + 2,), -78, dtype=torch.int32, device=DEV),
            "tok": torch.full((B + 2,), -79, dtype=torch.int64, device=DEV), "lab": torch.full((B + 2,), -80, dtype=torch.int32, device=DEV)}
    bufs["node"][1:B + 1] = node
    bufs["unf"][1:B + 1] = unfinished
    view = {k: v[1:B + 1] for k, v in bufs.items()}
    rc = L.cgpt_llm_trie_select_logits(P(logits), V, B, V, *[P(t) for t in trie_dev.tables()], nodes, pad, P(view["node"]), P(view["unf"]),
                                       P(view["tok"]), P(view["lab"]), _stream())
    assert rc == 0, L.cgpt_last_error()
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert v[0] == v[-1] and int(v[0]) in (-77, -78, -79, -80), f"{k}: a neighbouring element was written"
    return view


@pytest.mark.parametrize("B", [1, 37, 256])
@pytest.mark.parametrize("vocab", [320, 32000])
def test_select_kernel_equals_the_law_bit_for_bit(vocab, B):
    trie, fans = fan_trie(vocab, seed=vocab + B)
    begin, tok = trie.child_begin.tolist(), trie.child_tok.tolist()
    g = torch.Generator(device="cpu").manual_seed(7 * vocab + B)
    logits = torch.randn(B, vocab, generator=g)
    # the first rows pin every (boundary, case) pair that matters -- (node, case): 4 = a tie across two strides of one thread (nodes of
    # 257 and more edges), 3 = across two waves, 2 = across two lanes of one wave, 1 = the maximum on the last edge, 0 = random -- and
    # the others are spread over the root and the nine fan-out nodes, some of them finished; B = 1 is the first of them
    special = [(8, 4), (9, 4), (7, 3), (9, 3), (3, 2), (6, 2), (1, 1), (2, 1), (5, 1), (0, 1), (4, 0), (0, 0)]
    node = [special[b][0] if b < len(special) else (b * 7 + 3) % (len(FANS) + 1) for b in range(B)]
    unfinished = [0 if (b >= len(special) and b % 5 == 3) else 1 for b in range(B)]
    cases = []
    for b in range(B):
        e0, e1 = begin[node[b]], begin[node[b] + 1]
        f = e1 - e0
        allowed = torch.tensor(tok[e0:e1])
        # tokens on no edge of the row's node hold huge logits of both signs: they must not matter
        off = torch.ones(vocab, dtype=torch.bool)
        off[allowed] = False
        logits[b, off] = torch.where(torch.arange(int(off.sum())) % 2 == 0, 3.0e38, -3.0e38)
        case = special[b][1] if b < len(special) else (b // 3) % 5
        pair = {2: (3, 40), 3: (10, 200), 4: (0, 256)}.get(case)        # edge offsets: thread = offset % 256, wave = thread // 64
        if case == 1 or (pair is not None and pair[1] >= f):         # the maximum on the last edge (token vocab - 1 when f >= 2)
            logits[b, tok[e1 - 1]] = 50.0
            cases.append("last")
        elif pair is not None:                                         # equal maxima in two lanes / two waves / two strides of one thread
            logits[b, tok[e0 + pair[0]]] = logits[b, tok[e0 + pair[1]]] = 60.0
            cases.append(("lanes", "waves", "strides")[case - 2])
        else:
            cases.append("plain")
    if B > 1:
        assert {"last", "lanes", "waves", "strides", "plain"} <= set(cases) and 0 in unfinished
        assert set(node) == set(range(len(FANS) + 1))
    logits = logits.to(DEV)
    node_t = torch.tensor(node, dtype=torch.int32, device=DEV)
    unf_t = torch.tensor(unfinished, dtype=torch.int32, device=DEV)
    want = constrained_select_law(logits, node_t, unf_t, trie, 99)
    got = kernel_select(logits, node_t, unf_t, trie.to(DEV), trie.nodes, 99)
    assert torch.equal(got["tok"], want[0]) and torch.equal(got["node"], want[1]) and torch.equal(got["unf"], want[2])
    assert torch.equal(got["lab"], torch.where(want[3] >= 0, want[3], torch.full_like(want[3], -80)))     # written at a leaf only
    for b, case in enumerate(cases):                                   # the planted winners, spelled out
        if not unfinished[b]:
            assert int(got["tok"][b]) == 99 and int(got["node"][b]) == node[b]
        elif case == "last":
            assert int(got["tok"][b]) == tok[begin[node[b] + 1] - 1]
        elif case != "plain":
            lo = {"lanes": 3, "waves": 10, "strides": 0}[case]
            assert int(got["tok"][b]) == tok[begin[node[b]] + lo], (b, case)     # the lower token id of the tie


# ------------------------------------------------------------------------------------------ 2. the loop
def answer_trie(seed=5, count=40, vocab=320, alphabet=9):
    """About `count` candidates of 1..4 tokens over a small alphabet (so prefixes are shared), prefix-free, depth 4."""
    rng = random.Random(seed)
    letters = rng.sample(range(3, vocab), alphabet)
    seqs = set()
    while len(seqs) < count * 2:
        seqs.add(tuple(rng.choice(letters) for _ in range(rng.randrange(1, 5))))
    seqs = sorted(s for s in seqs if not any(o != s and o[:len(s)] == s for o in seqs))[:count]
    rng.shuffle(seqs)
    trie = build_answer_trie(seqs, vocab)
    assert trie.depth == 4 and {len(s) for s in seqs} >= {2, 3, 4} and len(seqs) >= 30
    return trie, seqs


@pytest.fixture(scope="module")
def small():
    llm = lu.small_decoder()
    dec = _HipDecoder(llm, 64)
    trie, seqs = answer_trie()
    dec.set_trie(trie)
    yield llm, dec, trie, seqs
    dec.close()


def check_rows(tokens, labels, seqs, depth):
    for row, lab in zip(tokens.tolist(), labels.tolist()):
        n = len(seqs[lab])
        assert tuple(row[:n]) == tuple(seqs[lab]) and row[n:] == [PAD] * (depth - n), (row, lab, seqs[lab])


@pytest.mark.parametrize("prefill", ["model", "hip"])
def test_loop_equals_the_law_on_the_logits_it_read(small, prefill):
    llm, dec, trie, seqs = small
    B, L, depth = 37, 12, trie.depth
    embs = lu.embeds(llm, B, L, seed=3)
    if prefill == "model":
        first, kb, vb, _ = lu.prefill(llm, embs, depth + 2)
        first = first.contiguous()
    else:
        kb, vb = lu.sentinel_cache(dec.layers, dec.kv_heads, B, L + depth + 2)
        first = dec.prefill(embs, kb, vb)
    tokens, labels, steps = dec.constrained(first, L, PAD, kb, vb, return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(steps[:, 0], first) and bool(torch.isfinite(steps).all())
    want_tokens, want_labels = constrained_decode_law(steps, trie, PAD)
    assert torch.equal(tokens, want_tokens) and torch.equal(labels, want_labels)
    check_rows(tokens, labels, seqs, depth)
    assert len(set(labels.tolist())) >= 3
    for l in range(len(kb)):                                           # depth - 1 steps append rows L .. L + depth - 2
        assert not bool((kb[l][:, :, L:L + depth - 1] == K_SENTINEL).all(dim=-1).any())
        assert bool((kb[l][:, :, L + depth - 1:] == K_SENTINEL).all()) and bool((vb[l][:, :, L + depth - 1:] == V_SENTINEL).all())
    # the same call without the step-logits table (the engine's own logits buffer)
    if prefill == "hip":
        kb2, vb2 = lu.sentinel_cache(dec.layers, dec.kv_heads, B, L + depth + 2)
        first2 = dec.prefill(embs, kb2, vb2)
        t2, l2 = dec.constrained(first2, L, PAD, kb2, vb2)
        assert torch.equal(t2, tokens) and torch.equal(l2, labels)


# ------------------------------------------------------------------------------------------ 3. early stop
def _constrained(dec, on, first, L, kb, vb, depth, starts=None):
    """One constrained call through the C entry on clones of the caches, early stop `on`: (tokens, live_steps, K, V, step logits,
    labels); the step logits and the labels are filled with sentinels beforehand."""
    kb, vb = [t.clone() for t in kb], [t.clone() for t in vb]
    B, V = first.shape
    dec.set_early_stop(on)
    try:
        tokens = torch.full((B, depth), -7, dtype=torch.int64, device=DEV)
        labels = torch.full((B,), -9, dtype=torch.int32, device=DEV)
        buf = torch.full((B, depth, V), LOGIT_SENTINEL, dtype=torch.float32, device=DEV)
        kp, vp, stride = dec._cache_tables(kb, vb, B, L + depth - 1)
        dec._greedy_ran = True
        assert starts is None
        rc = dec.L.cgpt_llm_constrained(dec.handle, P(first), B, L, depth, PAD, kp, vp, stride, P(tokens), P(buf), P(labels), _stream())
        assert rc == 0, dec.L.cgpt_last_error()
        steps = dec.live_steps()
    finally:
        dec.set_early_stop(False)
    return tokens, steps, kb, vb, buf, labels


def selects_needed(tokens):
    """The largest number of selects a row needed: its tokens before the pad ids (no candidate holds the pad id)."""
    return int((tokens != PAD).sum(dim=1).max())


def test_early_stop_exact_path_on_a_zeroed_head():
    """lm_head zeroed: every select ties, so every row takes the lowest token id at each node -- the path is known in advance: the
    root's lowest edge, then that node's lowest edge, ... to a leaf after `k` selects; with early stop k - 1 steps run."""
    llm = lu.zero_head(lu.small_decoder())
    dec = _HipDecoder(llm, 64)
    try:
        seqs = [(9, 4), (9, 8, 5, 6), (9, 8, 5, 7), (20, 3), (20, 11, 12), (30,)]     # the all-lowest path: 9 then 4 -> class 0, k = 2
        trie = build_answer_trie(seqs, 320)
        dec.set_trie(trie)
        B, L, depth = 37, 12, trie.depth
        assert depth == 4
        first, kb, vb, _ = lu.prefill(llm, llm.get_input_embeddings()(lu.ids(llm, B, L, 3)), depth)
        assert bool((first == 0).all())
        off = _constrained(dec, False, first, L, kb, vb, depth)
        on = _constrained(dec, True, first, L, kb, vb, depth)
        want = torch.tensor([[9, 4, PAD, PAD]] * B, dtype=torch.int64, device=DEV)
        assert torch.equal(off[0], want) and torch.equal(on[0], want)
        assert bool((off[5] == 0).all()) and bool((on[5] == 0).all())
        assert off[1] == depth - 1 and on[1] == 1 == selects_needed(off[0]) - 1
        lu.check_dead_part(L, 1, on[:5], off[:5])
    finally:
        dec.close()


def test_early_stop_gives_the_same_tokens_and_labels_on_natural_rows(small):
    llm, dec, trie, seqs = small
    depth = trie.depth
    # the candidates cut to 2 tokens, beside one of 4 that keeps the depth: most rows end within 2 selects
    short = build_answer_trie(sorted({s[:2] for s in seqs}) + [(1, 1, 1, 2)], 320)
    assert short.depth == 4
    for t, B in ((trie, 37), (short, 5)):
        dec.set_trie(t)
        try:
            L = 12
            kb, vb = lu.sentinel_cache(dec.layers, dec.kv_heads, B, L + depth)
            first = dec.prefill(lu.embeds(llm, B, L, seed=4), kb, vb)
            off = _constrained(dec, False, first, L, kb, vb, depth)
            on = _constrained(dec, True, first, L, kb, vb, depth)
            assert torch.equal(on[0], off[0]) and torch.equal(on[5], off[5]) and bool((off[5] >= 0).all())
            live = selects_needed(off[0]) - 1
            assert off[1] == depth - 1 and on[1] == live
            assert 0 <= live <= depth - 1
            lu.check_dead_part(L, live, on[:5], off[:5])
        finally:
            dec.set_trie(trie)


# ------------------------------------------------------------------------------------------ 4. left padding
def test_a_left_padded_row_equals_the_row_alone(small):
    llm, dec, trie, seqs = small
    L, lens, depth = 12, [7, 9, 12, 8, 10], trie.depth
    g = torch.Generator(device="cpu").manual_seed(6)
    embs = llm.get_input_embeddings()(torch.randint(3, 320, (len(lens), L), generator=g).to(DEV)).contiguous()
    starts = torch.tensor([L - n for n in lens], dtype=torch.int32, device=DEV)
    embs = (embs * (torch.arange(L, device=DEV)[None, :] >= starts[:, None])[:, :, None].to(embs.dtype)).contiguous()

    def run(e, n, st=None):
        kb, vb = lu.sentinel_cache(dec.layers, dec.kv_heads, e.shape[0], n + depth + 1)
        first = dec.prefill(e, kb, vb, starts=st)
        return dec.constrained(first, n, PAD, kb, vb, return_logits=True, starts=st) + (kb, vb)

    tokens, labels, steps, kb, vb = run(embs, L, starts)
    check_rows(tokens, labels, seqs, depth)
    for b, n in enumerate(lens):
        s_tokens, s_labels, s_steps, s_kb, s_vb = run(embs[b:b + 1, L - n:].contiguous(), n)
        assert torch.equal(tokens[b:b + 1], s_tokens) and torch.equal(labels[b:b + 1], s_labels) and torch.equal(steps[b:b + 1], s_steps), b
        for l in range(len(kb)):
            assert torch.equal(kb[l][b:b + 1, :, L - n:L + depth - 1], s_kb[l][:, :, :n + depth - 1])
            assert bool((kb[l][b, :, :L - n] == K_SENTINEL).all()) and bool((kb[l][b, :, L + depth - 1:] == K_SENTINEL).all())


# ------------------------------------------------------------------------------------------ 5. the engine's other modes
def _run(dec, embs, trie, starts=None):
    B, L = embs.shape[:2]
    kb, vb = lu.sentinel_cache(dec.layers, dec.kv_heads, B, L + trie.depth)
    first = dec.prefill(embs, kb, vb, starts=starts)
    tokens, labels, steps = dec.constrained(first, L, PAD, kb, vb, return_logits=True, starts=starts)
    torch.cuda.synchronize()
    return first, tokens, labels, steps, kb, vb


def test_int8_weights_and_activations():
    """On a W8A8 handle the loop is that handle's own token step around the trie select: tokens and labels are the law of the logits
    the call read, every step's logits are bit for bit `step()` of the same handle teacher-forced on the call's tokens, and against the
    mode's oracle `act_int8_twin` under HF's constrained generate the decisive rows agree (the margin rule, zero violations)."""
    llm = lu.llama_decoder(512, 4, 1408, 320, plant=True)
    dec = _HipDecoder(llm, 64, weights="int8", activations="int8", outlier_cap=1024)
    try:
        trie, seqs = answer_trie()
        dec.set_trie(trie)
        B, L, depth = 37, 12, trie.depth
        embs = lu.embeds(llm, B, L, seed=8)
        first, tokens, labels, steps, kb, vb = _run(dec, embs, trie)
        want_tokens, want_labels = constrained_decode_law(steps, trie, PAD)
        assert torch.equal(tokens, want_tokens) and torch.equal(labels, want_labels)
        check_rows(tokens, labels, seqs, depth)
        kb2, vb2 = lu.sentinel_cache(dec.layers, dec.kv_heads, B, L + depth)
        assert torch.equal(dec.prefill(embs, kb2, vb2), first)
        for i in range(1, depth):                                      # a finished row steps on the pad id, in the loop and here
            assert torch.equal(dec.step(tokens[:, i - 1].contiguous(), L + i - 1, kb2, vb2), steps[:, i]), i
        for a, b in zip(kb + vb, kb2 + vb2):
            assert torch.equal(a, b)
        assert dec.act_stats()["overflow_rows"] == 0
        twin = act_int8_twin(llm)
        with torch.no_grad():
            out = twin.generate(inputs_embeds=embs, attention_mask=torch.ones(embs.shape[:2], dtype=torch.int, device=DEV),
                                max_new_tokens=depth, output_scores=True, return_dict_in_generate=True, do_sample=False, num_beams=1,
                                prefix_allowed_tokens_fn=allowed_tokens_fn(trie, PAD))
        hf_first, _, _ = lu.model_prefill(twin, embs)
        eps = 2.0 * float((first - hf_first).abs().max())
        v = greedy_decode_parity(out.sequences, torch.stack(out.scores, dim=1).float(), tokens, eps)
        print(f"[constrained, W8A8 against act_int8_twin] eps {eps:.4g}: {v['identical']}/{B} rows identical, "
              f"{v['decisive_identical']}/{v['decisive']} decisive rows identical, {len(v['violations'])} violations", flush=True)
        assert v["violations"] == [] and v["decisive_identical"] == v["decisive"]
    finally:
        dec.close()


def test_grouped_kv_equals_the_plain_engine_on_the_expanded_twin():
    llm = lu.llama_decoder(512, 4, 1408, 320, kv_heads=2)
    twin = lu.llama_decoder(512, 4, 1408, 320, kv_heads=4, sd=expand_kv_state_dict(llm))
    gqa, mha = _HipDecoder(llm, 64, grouped_kv=True), _HipDecoder(twin, 64)
    try:
        trie, seqs = answer_trie()
        gqa.set_trie(trie)
        mha.set_trie(trie)
        embs = lu.embeds(llm, 37, 12, seed=9)
        a, b = _run(gqa, embs, trie), _run(mha, embs, trie)
        assert gqa.kv_heads == 2 and mha.kv_heads == 4
        for x, y, name in zip(a[:4], b[:4], ("first logits", "tokens", "labels", "step logits")):
            assert torch.equal(x, y), name
        check_rows(a[1], a[2], seqs, trie.depth)
    finally:
        gqa.close()
        mha.close()


def test_shared_prefix_gives_the_bits_of_the_whole_prompt(small):
    llm, dec, trie, seqs = small
    B, Pn, Ln, depth = 37, 5, 7, trie.depth
    embs = lu.embeds(llm, B, Pn + Ln, seed=10)
    embs[:, :Pn] = embs[:1, :Pn]
    embs = embs.contiguous()
    plain = _run(dec, embs, trie)
    pk, pv = lu.sentinel_cache(dec.layers, dec.kv_heads, 1, Pn)
    dec.prefill(embs[:1, :Pn].contiguous(), pk, pv)
    kb, vb = lu.sentinel_cache(dec.layers, dec.kv_heads, B, Pn + Ln + depth)
    dec.kv_broadcast(pk, pv, Pn, kb, vb)
    first = dec.prefill_from(embs[:, Pn:].contiguous(), Pn, kb, vb)
    tokens, labels, steps = dec.constrained(first, Pn + Ln, PAD, kb, vb, return_logits=True)
    for x, y, name in zip((first, tokens, labels, steps), plain[:4], ("first logits", "tokens", "labels", "step logits")):
        assert torch.equal(x, y), name
    for x, y in zip(kb + vb, plain[4] + plain[5]):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------ 6. the classifier
CANDS = ["red", "red car", "red car door", "blue", "blue sky", "green", "green car", "dark blue sky", "dark red", "white", "white door",
         "black car"]


@pytest.fixture(scope="module")
def clf_setup():
    llm = lu.small_decoder()
    cfg = dataclasses.replace(mo.tiny_config(mode=mo.MODE_ENCODE_IMG, num_classes=10), proj_dim=512)
    enc = make_classifier(cfg, max_batch=50)
    missing, unexpected = enc.load_state_dict(mo.init_params(cfg, 20251121))
    assert not missing and not unexpected
    x = torch.from_numpy(mo.synthetic_image(cfg)).to(DEV)
    yield llm, enc, x
    enc.close()


def make(llm, enc, tok=None, **kw):
    return MiniGPT4Classifier(enc, llm, tok or WordHashTokenizer(320), PROMPT, AnswerLabelMap(len(CANDS) + 1, CANDS), max_batch=50,
                              classify="constrained", end_sym=" ###", **kw)


def test_classifier_follows_hf_constrained_generate_on_decisive_rows(clf_setup):
    """constrain="hip" against constrain="hf" on the same 50 noisy rows by the margin rule: HF's processed scores are -inf off the
    trie, so `greedy_decode_parity`'s top-2 margin is the margin among allowed tokens; eps = 2 x the largest |library - HF| first-token
    logit difference measured here.  Every decisive row must be identical (zero violations), and at least half of the rows must be
    decisive for the rule to bite.  The noisy copies of one image all spell the same answer on this random-init decoder, so half of
    the rows carry token embeddings in the image's place: rows that differ, and several paths through the trie.
    Observed on an MI355X with this seed and these candidates: eps 0.00244, 50 of 50 rows decisive under HF alone, 50 of 50
    identical to HF, no violation, 7 distinct labels."""
    llm, enc, x = clf_setup
    B, sigma, seed = 50, 0.5, 42
    emb = enc.encode_img_noisy(x, 0, B // 2, sigma, seed).to(torch.float16)
    emb = torch.cat([emb, lu.embeds(llm, B - B // 2, emb.shape[1], seed=12)]).contiguous()
    hf = make(llm, enc)
    hip = make(llm, enc, decode="hip", prefill="hip", constrain="hip")
    depth = hf.trie.depth
    assert depth == 4
    embs, mask, *_ = hf._prompt_inputs(emb, PROMPT)
    embs = embs.contiguous()
    kw = hf.hf_generate_kwargs()
    kw.pop("min_new_tokens", None)
    with torch.no_grad():
        out = llm.generate(inputs_embeds=embs, attention_mask=mask, max_new_tokens=depth, output_scores=True, return_dict_in_generate=True,
                           prefix_allowed_tokens_fn=allowed_tokens_fn(hf.trie, PAD), **kw)
    hf_tokens, hf_scores = out.sequences, torch.stack(out.scores, dim=1).float()
    hf_labels, hf_toks2 = hf.constrained_from_embeds(emb, PROMPT)
    assert torch.equal(hf_toks2[:, :hf_tokens.shape[1]], hf_tokens) and hf_labels.tolist() == trie_walk(hf_tokens, hf.trie)
    kb, vb = lu.sentinel_cache(hip._hip.layers, hip._hip.kv_heads, B, embs.shape[1])
    lib_first = hip._hip.prefill(embs, kb, vb)
    hf_first, _, _ = lu.model_prefill(llm, embs)
    eps = 2.0 * float((lib_first - hf_first).abs().max())
    labels, tokens = hip.constrained_from_embeds(emb, PROMPT)
    v = greedy_decode_parity(hf_tokens, hf_scores, tokens, eps)
    same = (tokens == hf_toks2).all(dim=1)
    print(f"[constrained classifier] eps {eps:.4g}: {v['identical']}/{B} rows identical to HF, {v['decisive_identical']}/{v['decisive']} "
          f"decisive rows identical, {len(v['violations'])} violations, {len(set(labels.tolist()))} distinct labels", flush=True)
    assert v["violations"] == [] and v["decisive_identical"] == v["decisive"]
    assert v["decisive"] >= B // 2, v
    assert len(set(labels.tolist())) >= 3
    assert torch.equal(labels[same], hf_labels[same]) and labels.tolist() == trie_walk(tokens, hip.trie)
    s = hip.decode_stats
    assert s["hip_constrained"] == 1 and s["hf_constrained"] == 0 and s["hf_constrained_fallbacks"] == 0 and s["graph_captures"] == 1
    assert hf.decode_stats["hf_constrained"] == 1
    # a call the engine cannot take goes down the "hf" path and is counted
    big = make(llm, enc, decode="hip", prefill="hip", constrain="hip")
    big.max_batch = 4
    lab, lab_tokens = big.constrained_from_embeds(emb[:6], PROMPT)                # more rows than max_batch
    assert big.decode_stats["hf_constrained_fallbacks"] == 1 and big.decode_stats["hf_constrained"] == 1
    assert lab.tolist() == trie_walk(lab_tokens, big.trie) and min(lab.tolist()) >= 0


@pytest.mark.parametrize("constrain", ["hip", "hf"])
def test_classifier_with_shared_prefix_votes_as_without(clf_setup, constrain):
    """shared_prefix=True changes nothing: the native path continues the prefix cache, and every call that goes to HF `generate` --
    constrain="hf", or more rows than the engine takes -- is handed the WHOLE prompt, never the part behind the prefix."""
    llm, enc, x = clf_setup
    emb = enc.encode_img_noisy(x, 0, 6, 0.5, 42).to(torch.float16)
    emb = torch.cat([emb, lu.embeds(llm, 6, emb.shape[1], seed=13)]).contiguous()
    on, off = (make(llm, enc, decode="hip", prefill="hip", constrain=constrain, shared_prefix=flag) for flag in (True, False))
    (l_on, t_on), (l_off, t_off) = on.constrained_from_embeds(emb, PROMPT), off.constrained_from_embeds(emb, PROMPT)
    assert torch.equal(l_on, l_off) and torch.equal(t_on, t_off) and len(set(l_off.tolist())) >= 2
    s = on.decode_stats
    if constrain == "hip":
        assert s["hip_constrained"] == 1 and s["hip_prefix_prefills"] == 1 and s["hf_constrained"] == 0
        on.max_batch = off.max_batch = 8                               # 12 rows > max_batch: the "hf" fallback, on the whole prompt
        (l_on, t_on), (l_off, t_off) = on.constrained_from_embeds(emb, PROMPT), off.constrained_from_embeds(emb, PROMPT)
        assert torch.equal(l_on, l_off) and torch.equal(t_on, t_off)
        assert s["hf_constrained_fallbacks"] == 1 and s["hip_prefix_prefills"] == 1
    else:
        assert s["hf_constrained"] == 1 and s["hip_prefix_prefills"] == 0 and s["hip_prefix_hits"] == 0
    # and with the logits asked for (always HF's): the whole prompt again
    a, b = on.constrained_from_embeds(emb, PROMPT, return_logits=True), off.constrained_from_embeds(emb, PROMPT, return_logits=True)
    assert torch.equal(a[2], b[2]) and torch.equal(a[1], b[1]) and s["hip_prefix_prefills"] == (1 if constrain == "hip" else 0)


def test_classifier_counts_come_from_device_labels(clf_setup):
    llm, enc, x = clf_setup

    class Tok(WordHashTokenizer):
        decodes = 0

        def decode(self, *a, **kw):
            Tok.decodes += 1
            return super().decode(*a, **kw)

    clf = make(llm, enc, tok=Tok(320), decode="hip", prefill="hip", constrain="hip", early_stop=True)
    sigma, seed, other = 0.5, 42, clf.label_map.other_id
    whole = clf.sample_counts(x, 0, 40, 40, sigma, seed)
    answers = list(clf.last_answers)
    assert int(whole.sum()) == 40 and int(whole[other]) == 0 and len(answers) == 40 and set(answers) <= set(CANDS)
    assert whole.tolist() == [answers.count(c) for c in CANDS] + [0]
    captures = clf.decode_stats["graph_captures"]
    for bs in (40, 20, 8):                                             # one graph per batch size; 8 leaves no ragged last batch
        before = dict(clf.decode_stats)
        got = clf.sample_counts(x, 0, 40, bs, sigma, seed)
        assert got.tolist() == whole.tolist() and clf.last_answers == answers, bs
        assert clf.decode_stats["hip_constrained"] == before["hip_constrained"] + 40 // bs
        assert clf.decode_stats["graph_replays"] == before["graph_replays"] + 40 // bs
        if bs == 40:                                                   # a repeated call replays: nothing is captured again
            assert clf.decode_stats["graph_captures"] == captures
    assert clf.decode_stats["graph_captures"] == captures + 2           # 20 and 8: the 40-row graph was there
    before = dict(clf.decode_stats)
    pair = clf.sample_counts_pair(x, 0, 16, 16, 24, 20, sigma, seed)
    both = list(clf.last_answers)
    a = clf.sample_counts(x, 0, 16, 20, sigma, seed)
    b = clf.sample_counts(x, 16, 24, 20, sigma, seed)
    assert pair[0].tolist() == a.tolist() and pair[1].tolist() == b.tolist() and both == answers
    assert (pair[0] + pair[1]).tolist() == whole.tolist()
    assert clf.decode_stats["graph_captures"] == before["graph_captures"] + 2      # 16 rows, then 20 + 4; the pair's two batches of 20 replay
    assert clf.decode_stats["hf_constrained"] == 0 and clf.decode_stats["hf_calls"] == 0 and Tok.decodes == 0
    assert 0 <= clf.last_live_steps() <= clf.trie.depth - 1
    # the nn.Module-shaped surface: one-hot logits of the labels
    imgs = x[None].expand(3, -1, -1, -1).contiguous()
    logits = clf(imgs)
    assert logits.shape == (3, len(CANDS) + 1) and bool((logits.sum(1) == 1).all()) and int(logits[:, other].sum()) == 0
    assert clf.last_answers == [CANDS[i] for i in logits.argmax(1).tolist()]


# ------------------------------------------------------------------------------------------ 7. the label vote
def test_vote_labels_equals_bincount():
    g = torch.Generator(device="cpu").manual_seed(1)
    K = 1000
    labels = torch.randint(0, K, (1000,), generator=g, dtype=torch.int32)
    labels[::37] = -1
    labels[5::41] = K
    labels[7] = 2 ** 31 - 1
    labels[8] = -2 ** 31
    base = torch.randint(0, 2 ** 40, (K,), generator=g, dtype=torch.int64)
    counts = torch.cat([torch.tensor([-5]), base, torch.tensor([-6])]).to(DEV)      # sentinels around the histogram
    view = counts[1:K + 1]
    dev = labels.to(DEV)
    vote_labels(dev, view)
    vote_labels(dev[:0], view)                                         # no label: nothing is launched
    torch.cuda.synchronize()
    valid = labels[(labels >= 0) & (labels < K)].long()
    assert torch.equal(view.cpu(), base + torch.bincount(valid, minlength=K))
    assert int(counts[0]) == -5 and int(counts[-1]) == -6


# ------------------------------------------------------------------------------------------ 8. refusals
def test_entries_refuse_before_any_launch(small):
    llm, dec, trie, _ = small
    L = dec.L
    B, Lp, depth = 2, 4, trie.depth
    fresh = _HipDecoder(llm, 4)
    try:
        kb, vb = lu.sentinel_cache(dec.layers, dec.kv_heads, B, Lp + depth)
        first = torch.zeros(B, 320, dtype=torch.float32, device=DEV)
        tokens = torch.full((B, depth), -7, dtype=torch.int64, device=DEV)
        labels = torch.full((B,), -9, dtype=torch.int32, device=DEV)

        def call(d, n, lab, ragged=False):
            kp, vp, stride = d._cache_tables(kb, vb, B, Lp + depth - 1)
            if ragged:
                return L.cgpt_llm_constrained_ragged(d.handle, P(first), B, Lp, None, n, PAD, kp, vp, stride, P(tokens), None, lab, _stream())
            return L.cgpt_llm_constrained(d.handle, P(first), B, Lp, n, PAD, kp, vp, stride, P(tokens), None, lab, _stream())

        def refused(rc, word):
            msg = L.cgpt_last_error().decode()
            assert rc == 1 and word in msg, (rc, msg)

        refused(call(fresh, depth, P(labels)), "no trie")
        refused(call(dec, depth - 1, P(labels)), "depth")
        refused(call(dec, depth + 1, P(labels)), "depth")
        refused(call(dec, depth, None), "labels_out_dev")
        refused(call(dec, depth, P(labels), ragged=True), "starts_dev")
        tabs = [t.clone() for t in trie.tables()]
        tabs[1][0] = 320                                               # a token >= the handle's vocabulary
        refused(L.cgpt_llm_set_trie(fresh.handle, *[P(t) for t in tabs], trie.nodes, trie.edges), "token 320")
        refused(call(fresh, depth, P(labels)), "no trie")              # a refused set_trie leaves the handle as it was
        with pytest.raises(RuntimeError, match="no trie"):
            fresh.constrained(first, Lp, PAD, kb, vb)
        fresh.set_trie(trie)
        fresh.set_trie(None)                                           # cleared again
        refused(call(fresh, depth, P(labels)), "no trie")
        torch.cuda.synchronize()
        assert bool((tokens == -7).all()) and bool((labels == -9).all())
        for t in kb + vb:
            assert bool(((t == K_SENTINEL) | (t == V_SENTINEL)).all())
    finally:
        fresh.close()
