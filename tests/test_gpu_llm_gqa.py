"""grouped_kv=True: grouped-query attention on the native LLaMA engine (cgpt_llm_config_gqa.grouped_kv).

The central property is EXACT.  A grouped handle loaded from the grouped model W is compared, by `torch.equal` and with no tolerance,
with the plain handle loaded from the multi-head twin `expand_kv_state_dict(W)` (k_proj / v_proj head blocks repeated G times): query
head h of the grouped engine reads K/V head h // G, which holds what twin head h holds, and every query's arithmetic and key order
are the plain kernels'.  Grouped cache head g equals twin heads g G .. g G + G - 1.  The one thing that could break this from
outside is the decode GEMM's K split, which depends on the fused q/k/v width: the step tests first assert, from the rule restated
here, that the grouped and the twin width run the same number of slices at these hidden sizes.

Accuracy against HF's own grouped-query forward is held to the project's yardstick (test_gpu_llm_decode.py / test_gpu_llm_prefill.py:
distance to an fp32 copy, library / HF <= 1.5 in max and rms, layer-0 cache rows >= 98 % bit-equal) at Llama-3-8B's widths."""
import copy
import dataclasses

import pytest
import torch

import certifiedgpt_amd as cg
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import (MiniGPT4Classifier, WordHashTokenizer, _HipDecoder, expand_kv_state_dict, hip_decode_unsupported,
                                       int8_state_dict, left_pad_embeds)
from oracle import model_oracle as mo
from gpu_util import DEV, make_classifier
import llm_util as lu
from llm_util import PAD, EOS, K_SENTINEL, V_SENTINEL, PROMPT

pytestmark = pytest.mark.gpu

GUARD = 5                                                              # sentinel positions behind every cache


class _Pair:
    """The grouped model with the grouped engine, and its multi-head twin with the plain engine."""

    def __init__(self, hidden, heads, kv_heads, mlp=1408, vocab=320):
        self.G = heads // kv_heads
        self.llm = lu.llama_decoder(hidden, heads, mlp, vocab, kv_heads=kv_heads)
        self.twin = lu.llama_decoder(hidden, heads, mlp, vocab, kv_heads=heads, sd=expand_kv_state_dict(self.llm))
        assert hip_decode_unsupported(self.llm, 64, grouped_kv=True) == []
        self.gqa = _HipDecoder(self.llm, 64, grouped_kv=True)
        self.mha = _HipDecoder(self.twin, 64)
        assert self.gqa.kv_heads == kv_heads and self.mha.kv_heads == heads

    def close(self):
        self.gqa.close()
        self.mha.close()


SHAPES = {"g2": (512, 4, 2), "g4": (512, 4, 1), "g8": (1024, 8, 1), "g1": (512, 4, 4)}


@pytest.fixture(scope="module")
def pairs():
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Pair(*SHAPES[name])
        return made[name]
    yield get
    for p in made.values():
        p.close()


def _same_caches(grouped, twin, G, where):
    """Grouped cache head g == twin heads g G .. g G + G - 1, every layer and position (sentinels included: nothing else written)."""
    for l, (x, y) in enumerate(zip(grouped, twin)):
        assert torch.equal(x.repeat_interleave(G, dim=1), y), f"{where}: cache of layer {l} differs"


def _run(dec, embs, n_new, starts=None, min_new=1, eos=(EOS,)):
    B, L = embs.shape[:2]
    kb, vb = lu.sentinel_cache(dec.layers, dec.kv_heads, B, L + n_new - 1 + GUARD)
    first = dec.prefill(embs, kb, vb, starts=starts)
    tokens, steps = dec.greedy(first, L, n_new, min_new, list(eos), PAD, kb, vb, return_logits=True, starts=starts)
    torch.cuda.synchronize()
    return first, tokens, steps, kb, vb


# ------------------------------------------------------------------------------------------ 1. prefill
@pytest.mark.parametrize("L", [1, 12, 44, 70, 300])
@pytest.mark.parametrize("which", ["g2", "g4", "g8"])
def test_prefill_equals_the_plain_engine_on_the_expanded_twin(pairs, which, L):
    p = pairs(which)
    for B in (5, 37):
        embs = lu.embeds(p.llm, B, L, seed=B + L)
        ka, va = lu.sentinel_cache(p.gqa.layers, p.gqa.kv_heads, B, L + GUARD)
        kb, vb = lu.sentinel_cache(p.mha.layers, p.mha.kv_heads, B, L + GUARD)
        a = p.gqa.prefill(embs, ka, va)
        b = p.mha.prefill(embs, kb, vb)
        torch.cuda.synchronize()
        where = f"{which}, {B} rows, L {L}"
        assert bool(torch.isfinite(a).all())
        assert torch.equal(a, b), f"{where}: last-position logits differ, max {float((a - b).abs().max())}"
        _same_caches(ka, kb, p.G, where + " K")
        _same_caches(va, vb, p.G, where + " V")
        assert bool((ka[0][:, :, L:] == K_SENTINEL).all()) and not bool((ka[0][:, :, :L] == K_SENTINEL).all(dim=-1).any())


# ------------------------------------------------------------------------------------------ 2. steps and greedy
def splitk_rule(N, K):
    """decode_gemm_splitk (csrc/llm_gemm.hip) restated: 64-column tiles, 64-deep K tiles; double the slices while the grid stays
    within 256 workgroups and a slice stays at least 4 K tiles deep, below 8 slices."""
    tiles, nkt, s = N // 64, K // 64, 1
    while s < 8 and tiles * s * 2 <= 256 and nkt // (s * 2) >= 4:
        s *= 2
    return s


@pytest.mark.parametrize("which", ["g2", "g4", "g8", "g1"])
def test_steps_and_greedy_equal_the_plain_engine_on_the_expanded_twin(pairs, which):
    p = pairs(which)
    hidden, heads, kv = SHAPES[which]
    n_grouped, n_twin = hidden + 2 * kv * 128, 3 * hidden
    want = {512: 2, 1024: 4}[hidden]
    assert splitk_rule(n_grouped, hidden) == splitk_rule(n_twin, hidden) == want, \
        (f"the decode GEMM's K split differs between the grouped q/k/v width {n_grouped} and the twin's {n_twin} at hidden {hidden}: the "
         "steps below are then two valid summation orders, not bit-equal -- choose shapes with equal slice counts")
    B, L, steps = 37, 12, 4
    embs = lu.embeds(p.llm, B, L, seed=3)
    g = torch.Generator(device="cpu").manual_seed(11)
    forced = torch.randint(3, 320, (steps, B), generator=g).to(DEV)
    got = {}
    for name, dec in (("gqa", p.gqa), ("mha", p.mha)):
        kb, vb = lu.sentinel_cache(dec.layers, dec.kv_heads, B, L + steps + GUARD)
        logits = [dec.prefill(embs, kb, vb)]
        for i in range(steps):
            logits.append(dec.step(forced[i].contiguous(), L + i, kb, vb))
        torch.cuda.synchronize()
        got[name] = (torch.stack(logits), kb, vb)
    for i in range(steps + 1):
        assert torch.equal(got["gqa"][0][i], got["mha"][0][i]), \
            f"{which}: logits of {'the prefill' if i == 0 else f'step {i}'} differ, max {float((got['gqa'][0][i] - got['mha'][0][i]).abs().max())}"
    _same_caches(got["gqa"][1], got["mha"][1], p.G, f"{which} teacher-forced K")
    _same_caches(got["gqa"][2], got["mha"][2], p.G, f"{which} teacher-forced V")
    a, b = _run(p.gqa, embs, 6), _run(p.mha, embs, 6)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), f"{which}: greedy run differs"
    _same_caches(a[3], b[3], p.G, f"{which} greedy K")
    _same_caches(a[4], b[4], p.G, f"{which} greedy V")


def test_a_long_row_crosses_the_step_kernels_staging_chunks(pairs):
    """Prompt 130: the step attention walks three 64-key chunks, the last one partial and holding the new key."""
    p = pairs("g4")
    embs = lu.embeds(p.llm, 5, 130, seed=9)
    a, b = _run(p.gqa, embs, 4), _run(p.mha, embs, 4)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    _same_caches(a[3], b[3], p.G, "long row K")
    _same_caches(a[4], b[4], p.G, "long row V")


# ------------------------------------------------------------------------------------------ 3. ragged
@pytest.mark.parametrize("which", ["g2", "g8"])
def test_a_padded_row_equals_the_row_alone_on_the_same_grouped_handle(pairs, which):
    p = pairs(which)
    L, n_new = 80, 5
    lens = [1, 15, 16, 17, 63, 64, 65, 80]
    embs, _, starts = left_pad_embeds([lu.embeds(p.llm, 1, n, seed=100 + n) for n in lens])
    assert embs.shape[1] == L
    embs, starts = embs.contiguous(), starts.to(DEV)
    a = _run(p.gqa, embs, n_new, starts)
    for b, n in enumerate(lens):
        s = L - n
        solo = _run(p.gqa, embs[b:b + 1, s:].contiguous(), n_new)
        where = f"{which}, row of length {n}"
        assert torch.equal(solo[0], a[0][b:b + 1]) and torch.equal(solo[1], a[1][b:b + 1]) and torch.equal(solo[2], a[2][b:b + 1]), where
        for l in range(len(a[3])):
            for padded, alone, sentinel in ((a[3][l], solo[3][l], K_SENTINEL), (a[4][l], solo[4][l], V_SENTINEL)):
                assert torch.equal(padded[b, :, s:L + n_new - 1], alone[0, :, :n + n_new - 1]), where
                assert bool((padded[b, :, :s] == sentinel).all()), where + ": rows below start[b] were touched"
    # the step entry itself, teacher-forced, against the twin through the same ragged entries
    ka, va = lu.sentinel_cache(p.gqa.layers, p.gqa.kv_heads, len(lens), L + 1 + GUARD)
    kb, vb = lu.sentinel_cache(p.mha.layers, p.mha.kv_heads, len(lens), L + 1 + GUARD)
    p.gqa.prefill(embs, ka, va, starts=starts)
    p.mha.prefill(embs, kb, vb, starts=starts)
    tok = torch.randint(3, 320, (len(lens),), generator=torch.Generator().manual_seed(1)).to(DEV)
    la = p.gqa.step(tok, L, ka, va, starts=starts)
    lb = p.mha.step(tok, L, kb, vb, starts=starts)
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    _same_caches(ka + va, kb + vb, p.G, "ragged step")


# ------------------------------------------------------------------------------------------ 4. bounds
@pytest.mark.parametrize("which", ["g2", "g4", "g8"])
def test_only_the_prompt_and_the_appended_rows_are_written(pairs, which):
    p = pairs(which)
    L, n_new = 21, 6
    _, _, _, kb, vb = _run(p.gqa, lu.embeds(p.llm, 7, L, seed=2), n_new)
    used = L + n_new - 1                                               # positions 0 .. prompt + steps - 1
    for l in range(len(kb)):
        assert tuple(kb[l].shape) == (7, p.gqa.kv_heads, used + GUARD, 128)
        assert bool((kb[l][:, :, used:] == K_SENTINEL).all()) and bool((vb[l][:, :, used:] == V_SENTINEL).all()), "the guard region was written"
        assert not bool((kb[l][:, :, :used] == K_SENTINEL).all(dim=-1).any()) and not bool((vb[l][:, :, :used] == V_SENTINEL).all(dim=-1).any())


# ------------------------------------------------------------------------------------------ 5. determinism
def test_graph_replays_and_row_splits_are_bit_identical(pairs):
    p = pairs("g4")
    L, n_new = 12, 4
    embs = lu.embeds(p.llm, 37, L, seed=3)
    eager = _run(p.gqa, embs, n_new)
    static = embs.clone()
    kb, vb = lu.sentinel_cache(p.gqa.layers, p.gqa.kv_heads, 37, L + n_new - 1 + GUARD)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        first = p.gqa.prefill(static, kb, vb)
        tokens, steps = p.gqa.greedy(first, L, n_new, 1, [EOS], PAD, kb, vb, return_logits=True)
    for _ in range(2):
        for t in kb + vb:
            t.fill_(3.0)
        first.zero_(), tokens.zero_(), steps.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(first, eager[0]) and torch.equal(tokens, eager[1]) and torch.equal(steps, eager[2])
        for l in range(len(kb)):
            assert torch.equal(kb[l][:, :, :L + n_new - 1], eager[3][l][:, :, :L + n_new - 1])
            assert torch.equal(vb[l][:, :, :L + n_new - 1], eager[4][l][:, :, :L + n_new - 1])
    del graph
    for lo, hi in ((0, 20), (20, 37)):
        part = _run(p.gqa, embs[lo:hi].contiguous(), n_new)
        assert torch.equal(part[0], eager[0][lo:hi]) and torch.equal(part[1], eager[1][lo:hi]) and torch.equal(part[2], eager[2][lo:hi])
        for l in range(len(kb)):
            assert torch.equal(part[3][l], eager[3][l][lo:hi]) and torch.equal(part[4][l], eager[4][l][lo:hi])


# ------------------------------------------------------------------------------------------ 6. scoring
@pytest.mark.parametrize("which", ["g2", "g8"])
def test_scores_equal_the_twins_and_leave_the_cache_alone(pairs, which):
    p = pairs(which)
    B, L, n_new = 5, 13, 4
    embs = lu.embeds(p.llm, B, L, seed=4)
    g = torch.Generator(device="cpu").manual_seed(5)
    cands = [torch.randint(3, 320, (n,), generator=g) for n in (1, 2, 5)]
    table = torch.zeros((3, 5), dtype=torch.long)
    for i, c in enumerate(cands):
        table[i, :len(c)] = c
    table, lens = table.to(DEV), [len(c) for c in cands]
    out = {}
    for name, dec in (("gqa", p.gqa), ("mha", p.mha)):
        kb, vb = lu.sentinel_cache(dec.layers, dec.kv_heads, B, L + n_new - 1 + GUARD)
        first = dec.prefill(embs, kb, vb)
        before = [t.clone() for t in kb + vb]
        sums = dec.score(first, L, table, lens, 0.1, kb, vb)
        torch.cuda.synchronize()
        for x, y in zip(kb + vb, before):
            assert torch.equal(x, y), f"{name}: cgpt_llm_score wrote to the cache"
        tokens = dec.greedy(first, L, n_new, 1, [EOS], PAD, kb, vb)
        out[name] = (sums, tokens)
    assert bool(torch.isfinite(out["gqa"][0]).all()) and torch.equal(out["gqa"][0], out["mha"][0]), \
        float((out["gqa"][0] - out["mha"][0]).abs().max())
    assert torch.equal(out["gqa"][1], _run(p.gqa, embs, n_new)[1])     # the greedy after a score call == one without it


# ------------------------------------------------------------------------------------------ 7. int8
def test_a_grouped_int8_handle_equals_a_grouped_fp16_handle_on_the_dequantised_weights(pairs):
    p = pairs("g4")
    twin8 = lu.llama_decoder(512, 4, 1408, 320, kv_heads=1, sd=int8_state_dict(p.llm, device="cpu"))
    q8 = _HipDecoder(p.llm, 64, weights="int8", grouped_kv=True)
    f16 = _HipDecoder(twin8, 64, grouped_kv=True)
    try:
        assert q8.weight_bytes < f16.weight_bytes < p.mha.weight_bytes
        for L in (12, 70):
            embs = lu.embeds(p.llm, 37, L, seed=L)
            a, b = _run(q8, embs, 5), _run(f16, embs, 5)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), L
            for x, y in zip(a[3] + a[4], b[3] + b[4]):
                assert torch.equal(x, y), L
    finally:
        q8.close()
        f16.close()


# ------------------------------------------------------------------------------------------ 8. early stop
@pytest.mark.parametrize("F", [0, 3])
def test_early_stop_tokens_and_live_steps(pairs, F):
    """The synthetic finishing law of test_gpu_llm_early_stop.py: with lm_head = 0 every logit is 0 and the first-max arg-max is
    token 0, which is the EOS and pad id here; it is suppressed on the first F tokens (then token 1 wins), so every row finishes at
    select F."""
    llm = lu.llama_decoder(512, 4, 1408, 320, kv_heads=2)
    with torch.no_grad():
        llm.lm_head.weight.zero_()
    dec = _HipDecoder(llm, 64, grouped_kv=True)
    try:
        B, L, n = 9, 12, 8
        embs = lu.embeds(llm, B, L, seed=3)
        res = {}
        for on in (False, True):
            kb, vb = lu.sentinel_cache(dec.layers, dec.kv_heads, B, L + n - 1 + GUARD)
            first = dec.prefill(embs, kb, vb)
            dec.set_early_stop(on)
            try:
                tokens = dec.greedy(first, L, n, F, [0], 0, kb, vb)
                res[on] = (tokens, dec.live_steps(), kb, vb)
            finally:
                dec.set_early_stop(False)
        want = torch.zeros(B, n, dtype=torch.int64, device=DEV)
        want[:, :F] = 1
        assert torch.equal(res[False][0], want) and torch.equal(res[True][0], res[False][0])
        assert res[False][1] == n - 1 and res[True][1] == F == lu.expected_live_steps(res[False][0], [0])
        for l in range(dec.layers):                                    # the dead steps appended nothing; the live ones what the off run did
            assert bool((res[True][2][l][:, :, L + F:] == K_SENTINEL).all()) and bool((res[True][3][l][:, :, L + F:] == V_SENTINEL).all())
            assert torch.equal(res[True][2][l][:, :, :L + F], res[False][2][l][:, :, :L + F])
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------ 9. accuracy against HF, Llama-3-8B widths
@pytest.fixture(scope="module")
def llama3():
    """Llama-3-8B's widths (hidden 4096, 32 / 8 heads, MLP 14336, rope_theta 500000) with 2 random-init layers and a 32000-token
    vocabulary (the real 128256 adds seconds, not coverage)."""
    llm = lu.llama_decoder(4096, 32, 14336, 32000, kv_heads=8, theta=500000.0)
    dec = _HipDecoder(llm, 200, grouped_kv=True)
    llm32 = copy.deepcopy(llm).float()
    yield llm, dec, llm32
    dec.close()
    del llm, llm32
    torch.cuda.empty_cache()


@pytest.mark.parametrize("B", [200, 37])
def test_teacher_forced_step_error_is_within_hfs_own_fp16_error_llama3_width(llama3, B):
    llm, dec, _ = llama3
    lu.check_ratios(f"Llama-3 width, grouped_kv, {B} rows", lu.teacher_forced(llm, dec, B, L=44, steps=4))


@pytest.mark.parametrize("L", [12, 44])
def test_prefill_error_is_within_hfs_own_fp16_error_llama3_width(llama3, L):
    """The criterion of test_gpu_llm_prefill.py (`_check_against_hf`) on caches of kv_heads heads."""
    llm, dec, llm32 = llama3
    B = 37
    embs = lu.embeds(llm, B, L, seed=3)
    kb, vb = lu.sentinel_cache(dec.layers, dec.kv_heads, B, L + GUARD)
    lib = dec.prefill(embs, kb, vb)
    torch.cuda.synchronize()
    hf, hk, hv = lu.model_prefill(llm, embs)
    ref, rk, rv = lu.model_prefill(llm32, embs.float())
    assert hk[0].shape[1] == 8 and bool(torch.isfinite(lib).all())
    figures = {"logits": lu.err(lib, ref) + lu.err(hf, ref)}
    share = {}
    for l in range(len(kb)):
        for nm, mine, theirs, exact in (("k", kb[l], hk[l], rk[l]), ("v", vb[l], hv[l], rv[l])):
            figures[f"{nm}{l}"] = lu.err(mine[:, :, :L], exact) + lu.err(theirs, exact)
            if l == 0:
                share[nm] = float((mine[:, :, :L] == theirs).float().mean())
    print(f"[prefill Llama-3 width, grouped_kv, {B} rows x {L} positions] (max, rms) error ratio library / HF against the fp32 model: "
          + ", ".join(f"{k} ({v[0] / v[2]:.3f}, {v[1] / v[3]:.3f})" for k, v in figures.items())
          + f"; layer 0 share bit-equal to HF: k {share['k']:.4f}, v {share['v']:.4f}", flush=True)
    for k, v in figures.items():
        assert v[0] <= 1.5 * v[2] and v[1] <= 1.5 * v[3], (k, v)
    assert share["k"] >= 0.98 and share["v"] >= 0.98, share


# ------------------------------------------------------------------------------------------ 10. the classifier
def test_classifier_answers_and_certificate_equal_the_twin_classifiers(pairs):
    p = pairs("g2")
    cfg = dataclasses.replace(mo.tiny_config(mode=mo.MODE_ENCODE_IMG, num_classes=10), proj_dim=512)
    enc = make_classifier(cfg, max_batch=50)
    try:
        missing, unexpected = enc.load_state_dict(mo.init_params(cfg, 20251121))
        assert not missing and not unexpected
        tok = WordHashTokenizer(320)
        x = torch.from_numpy(mo.synthetic_image(cfg)).to(DEV)
        B, n, sigma, seed = 50, 8, 0.5, 42
        emb = enc.encode_img_noisy(x, 0, B, sigma, seed).to(torch.float16)
        kw = dict(max_new_tokens=n, max_batch=B, decode="hip")
        calls = {"n": 0}
        hook = p.llm.register_forward_pre_hook(lambda *_: calls.__setitem__("n", calls["n"] + 1))
        try:
            gqa = MiniGPT4Classifier(enc, p.llm, tok, PROMPT, AnswerLabelMap(4, ()), prefill="hip", grouped_kv=True, **kw)
            ref = MiniGPT4Classifier(enc, p.twin, tok, PROMPT, AnswerLabelMap(4, ()), prefill="hip", **kw)
            pools = []                                                 # the K/V pool, seen where greedy_tokens hands it to the engine
            orig = gqa._hip.prefill
            gqa._hip.prefill = lambda e, kb, vb, starts=None: (pools.append(tuple(kb[0].shape)), orig(e, kb, vb, starts=starts))[1]
            answers, want = gqa.generate_from_embeds(emb, PROMPT), ref.generate_from_embeds(emb, PROMPT)
            assert len(answers) == B
            for i, (a, b) in enumerate(zip(answers, want)):
                assert a == b, f"row {i}: {a!r} != {b!r}"
            assert gqa.decode_stats["hf_calls"] == 0 and gqa.decode_stats["hip_prefills"] == 1 and calls["n"] == 0
            assert pools and all(sh[0] == B and sh[1] == 2 and sh[3] == 128 for sh in pools), pools      # kv_heads, not heads
            assert gqa._hip.kv_heads == 2 and ref._hip.kv_heads == 4
            for extra in (dict(prefill="hip", ragged="hip", prompt_bucket=16, weights="int8"), dict(prefill="model")):
                model, twin = p.llm, p.twin
                if extra.get("weights") == "int8":                     # the twin of an int8 engine: dequantised, then expanded
                    twin = lu.llama_decoder(512, 4, 1408, 320, kv_heads=4, sd=expand_kv_state_dict(
                        lu.llama_decoder(512, 4, 1408, 320, kv_heads=2, sd=int8_state_dict(p.llm, device="cpu"))))
                    extra_ref = dict(prefill="hip", ragged="hip", prompt_bucket=16)
                else:
                    extra_ref = extra
                a = MiniGPT4Classifier(enc, model, tok, PROMPT, AnswerLabelMap(4, ()), grouped_kv=True, **kw, **extra)
                b = MiniGPT4Classifier(enc, twin, tok, PROMPT, AnswerLabelMap(4, ()), **kw, **extra_ref)
                got_a, got_b = a.generate_from_embeds(emb, PROMPT), b.generate_from_embeds(emb, PROMPT)
                assert got_a == got_b, extra
                assert a.decode_stats["hf_calls"] == 0
                del a, b
        finally:
            hook.remove()
        vocab = sorted(set(answers), key=lambda a: (-answers.count(a), a))[:3]
        results = []
        for llm, extra in ((p.llm, dict(grouped_kv=True)), (p.twin, {})):
            clf = MiniGPT4Classifier(enc, llm, tok, PROMPT, AnswerLabelMap(len(vocab) + 1, vocab, frozen=True), prefill="hip", **kw, **extra)
            sm = cg.Smooth(clf, len(vocab) + 1, sigma, seed=seed, non_certifiable=(clf.label_map.other_id,))
            results.append((sm.certify(x, 100, 100, 0.001, 50), list(clf.last_answers)))
            del clf, sm
        assert results[0] == results[1], (results[0][0], results[1][0])
    finally:
        enc.close()
