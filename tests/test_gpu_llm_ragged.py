"""ragged="hip": left-padded prompts on the native LLaMA engine (cgpt_llm_prefill_ragged / _step_ragged / _greedy_ragged: a per-row
start offset in device memory, row-relative coordinates in the rotary and attention kernels).

The central property is EXACT.  The library's documented invariants are that a GEMM element's bits do not depend on the kernel, tile
or batch it was computed in and that a row's result does not depend on the batch around it; with
row-relative coordinates a padded row performs the operations of the unpadded row in the same order.  So a row of a padded batch
must give, bit for bit, the last-position logits, every step's logits, the tokens and the cache rows of the same row run WITHOUT
padding through the plain entries -- `torch.equal`, no tolerance.

Against HF the yardstick and the bounds are those of test_gpu_llm_prefill.py: e = distance to an fp32 copy of the weights,
max e_lib <= 1.5 max e_hf and rms e_lib <= 1.5 rms e_hf, here on the real positions only; trajectories by `greedy_decode_parity`
with eps = 2 x the first-token logit difference measured on the very rows of the test."""
import copy
import dataclasses

import pytest
import torch

import certifiedgpt_amd as cg
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import (MiniGPT4Classifier, WordHashTokenizer, _HipDecoder, greedy_decode_parity, hip_decode_unsupported,
                                       left_pad_embeds, prepare_texts)
from oracle import model_oracle as mo
from gpu_util import DEV, make_classifier
import llm_util as lu
from llm_util import PAD, EOS, K_SENTINEL, V_SENTINEL

pytestmark = pytest.mark.gpu

QUESTIONS = ["what is shown", "what is shown in the picture", "is there a dog or a cat in this picture",
             "how many people are there in the picture and what are they doing now"]
PROMPTS = prepare_texts(["<Img><ImageHere></Img> [vqa] " + q for q in QUESTIONS])


@pytest.fixture(scope="module")
def small():
    """hidden 512 = 4 heads x 128, MLP 1408, vocabulary 320, 2 layers."""
    llm = lu.llama_decoder(512, 4, 1408, 320)
    assert hip_decode_unsupported(llm, 200) == []
    dec = _HipDecoder(llm, 200)
    llm32 = copy.deepcopy(llm).float()
    yield llm, dec, llm32
    dec.close()


@pytest.fixture(scope="module")
def vicuna():
    """Vicuna-7B's widths (hidden 4096, 32 heads, MLP 11008, vocabulary 32000) with 2 random-init layers."""
    llm = lu.llama_decoder(4096, 32, 11008, 32000)
    dec = _HipDecoder(llm, 200)
    llm32 = copy.deepcopy(llm).float()
    yield llm, dec, llm32
    dec.close()
    del llm, llm32
    torch.cuda.empty_cache()


def _padded_batch(llm, L, lens, seed):
    """Row b: lens[b] real positions (embeddings of random tokens) at the END of L buffer positions, zeros before them."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    B = len(lens)
    embs = llm.get_input_embeddings()(torch.randint(3, llm.config.vocab_size, (B, L), generator=g).to(DEV)).contiguous()
    starts = torch.tensor([L - n for n in lens], dtype=torch.int32)
    mask = (torch.arange(L)[None, :] >= starts[:, None])
    embs = embs * mask.to(DEV)[:, :, None].to(embs.dtype)
    return embs.contiguous(), starts.to(DEV), mask.to(DEV)


def _run(llm, dec, embs, prompt_len, n_new, starts=None, extra=2):
    """prefill + greedy with the logits of every step; buffers hold `extra` rows past the last appended one."""
    B = embs.shape[0]
    kb, vb = lu.sentinel_cache(llm.config.num_hidden_layers, llm.config.num_attention_heads, B, prompt_len + n_new - 1 + extra)
    first = dec.prefill(embs, kb, vb, starts=starts)
    tokens, steps = dec.greedy(first, prompt_len, n_new, 1, [EOS], PAD, kb, vb, return_logits=True, starts=starts)
    torch.cuda.synchronize()
    return first, tokens, steps, kb, vb


def _assert_ragged_equals_solo(name, llm, dec, L, lens, n_new, seed):
    embs, starts, _ = _padded_batch(llm, L, lens, seed)
    first, tokens, steps, kb, vb = _run(llm, dec, embs, L, n_new, starts)
    assert bool(torch.isfinite(first).all())
    end = L + n_new - 1                                                # rows start[b] .. end-1 are written, nothing else
    for n in sorted(set(lens)):
        idx = torch.tensor([b for b, m in enumerate(lens) if m == n], device=DEV)
        solo = embs[idx, L - n:].contiguous()                          # the same rows without their padding, through the PLAIN entries
        s_first, s_tokens, s_steps, s_kb, s_vb = _run(llm, dec, solo, n, n_new)
        where = f"{name}: L {L}, length {n}, rows {idx.tolist()[:4]}.."
        assert torch.equal(first[idx], s_first), f"{where}: last-position logits differ, max {float((first[idx] - s_first).abs().max())}"
        assert torch.equal(steps[idx], s_steps), f"{where}: step logits differ"
        assert torch.equal(tokens[idx], s_tokens), f"{where}: tokens differ"
        for l in range(len(kb)):
            for nm, mine, theirs, sentinel in (("k", kb[l], s_kb[l], K_SENTINEL), ("v", vb[l], s_vb[l], V_SENTINEL)):
                rows = mine[idx]
                assert torch.equal(rows[:, :, L - n:end], theirs[:, :, :n + n_new - 1]), f"{where}: layer {l} {nm} cache differs"
                assert bool((rows[:, :, :L - n] == sentinel).all()), f"{where}: layer {l} {nm}: a cache row below start was written"
                assert bool((rows[:, :, end:] == sentinel).all()), f"{where}: layer {l} {nm}: a row past the last appended one was written"
                assert bool((theirs[:, :, n + n_new - 1:] == sentinel).all())
    return tokens


# ------------------------------------------------------------------------------------------ 1. ragged equals solo, bit for bit
# lengths across the attention kernel's 32-key block (31, 32, 33), its 64-key chunk and 64-query block (63, 64, 65), the token
# step's groups of four keys, and the two ends (1 real token; no padding at all)
SMALL_SHAPES = [(80, [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 79, 80]), (300, [1, 37, 236, 299, 300])]


@pytest.mark.parametrize("L, lengths", SMALL_SHAPES)
def test_a_padded_row_equals_the_row_alone_bit_for_bit_small_decoder(small, L, lengths):
    llm, dec, _ = small
    g = torch.Generator(device="cpu").manual_seed(L)
    lens = [lengths[i] for i in torch.randperm(3 * len(lengths), generator=g).remainder(len(lengths)).tolist()]      # 3 rows each, mixed
    assert sorted(set(lens)) == sorted(lengths)
    _assert_ragged_equals_solo("small decoder", llm, dec, L, lens, n_new=6, seed=31 + L)


def test_a_padded_row_equals_the_row_alone_bit_for_bit_vicuna_width(vicuna):
    llm, dec, _ = vicuna
    g = torch.Generator(device="cpu").manual_seed(48)
    lens = torch.randint(33, 49, (200,), generator=g).tolist()         # 200 rows, lengths drawn from 33 .. 48
    assert min(lens) >= 33 and max(lens) <= 48 and len(set(lens)) > 8
    _assert_ragged_equals_solo("Vicuna width", llm, dec, 48, lens, n_new=5, seed=9)      # 5 selects, 4 steps


# ------------------------------------------------------------------------------------------ 2. all starts zero = the plain entries
@pytest.mark.parametrize("which, B, L", [("small", 37, 70), ("vicuna", 200, 44)])
def test_all_starts_zero_gives_the_plain_entries_bits(which, B, L, request):
    llm, dec, _ = request.getfixturevalue(which)
    embs, starts, _ = _padded_batch(llm, L, [L] * B, seed=5)
    assert int(starts.abs().sum()) == 0
    ragged = _run(llm, dec, embs, L, 5, starts)
    plain = _run(llm, dec, embs, L, 5)
    for a, b in zip(ragged[:3], plain[:3]):
        assert torch.equal(a, b)
    assert all(torch.equal(a, b) for a, b in zip(ragged[3] + ragged[4], plain[3] + plain[4]))          # every cache row, sentinels included


def test_starts_outside_the_prompt_are_clamped_and_replays_read_the_current_starts(small):
    """The kernels clamp start[b] into 0 .. L-1 (the host cannot check device contents without a sync); a captured graph reads the
    array when it runs, so new contents take effect at the next replay without a new capture."""
    llm, dec, _ = small
    L, B, n_new = 40, 6, 4
    embs, _, _ = _padded_batch(llm, L, [L] * B, seed=8)
    wild = torch.tensor([-7, 0, L - 1, L, 5000, 3], dtype=torch.int32, device=DEV)
    clamped = wild.clamp(0, L - 1)
    got = _run(llm, dec, embs, L, n_new, wild)
    want = _run(llm, dec, embs, L, n_new, clamped)
    assert bool(torch.isfinite(got[0]).all())
    for a, b in zip(got[:3], want[:3]):
        assert torch.equal(a, b)
    assert all(torch.equal(a, b) for a, b in zip(got[3] + got[4], want[3] + want[4]))
    # one capture, two contents of the same starts tensor
    static = clamped.clone()
    kb, vb = lu.sentinel_cache(llm.config.num_hidden_layers, llm.config.num_attention_heads, B, L + n_new)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        first = dec.prefill(embs, kb, vb, starts=static)
        tokens = dec.greedy(first, L, n_new, 1, [EOS], PAD, kb, vb, starts=static)
    for contents in (torch.tensor([3, 9, 0, 20, 39, 1], dtype=torch.int32, device=DEV), clamped):
        static.copy_(contents)
        graph.replay()
        torch.cuda.synchronize()
        eager = _run(llm, dec, embs, L, n_new, contents)
        assert torch.equal(first, eager[0]) and torch.equal(tokens, eager[1])
    del graph


# ------------------------------------------------------------------------------------------ 3. against HF on real positions
def _model_prefill_padded(model, embs, mask):
    """(last-position logits fp32, per-layer keys, per-layer values) of the model's own forward on left-padded rows: the attention
    mask and the positions HF's `generate` derives from it (the first real token at position 0)."""
    from transformers import DynamicCache
    cache = DynamicCache(config=model.config)
    pos = (mask.long().cumsum(-1) - 1).clamp_min(0)
    with torch.no_grad():
        out = model(inputs_embeds=embs, attention_mask=mask.long(), position_ids=pos, past_key_values=cache, use_cache=True,
                    logits_to_keep=1)
    return out.logits[:, -1].float(), [l.keys for l in cache.layers], [l.values for l in cache.layers]


def _check_against_hf(name, llm, dec, llm32, L, lens, seed):
    embs, starts, mask = _padded_batch(llm, L, lens, seed)
    B = len(lens)
    kb, vb = lu.sentinel_cache(llm.config.num_hidden_layers, llm.config.num_attention_heads, B, L + 3)
    lib = dec.prefill(embs, kb, vb, starts=starts)
    torch.cuda.synchronize()
    hf, hk, hv = _model_prefill_padded(llm, embs, mask)
    ref, rk, rv = _model_prefill_padded(llm32, embs.float(), mask)
    assert bool(torch.isfinite(lib).all()) and bool(torch.isfinite(hf).all()) and bool(torch.isfinite(ref).all())
    figures = {"logits": lu.err(lib, ref) + lu.err(hf, ref)}

    def real(t):                                                       # [B, heads, L, 128] -> the real positions' rows
        return t[:, :, :L].permute(0, 2, 1, 3)[mask]

    for l in range(len(kb)):
        for nm, mine, theirs, exact in (("k", kb[l], hk[l], rk[l]), ("v", vb[l], hv[l], rv[l])):
            assert bool(torch.isfinite(real(mine)).all())
            figures[f"{nm}{l}"] = lu.err(real(mine), real(exact)) + lu.err(real(theirs), real(exact))
    print(f"[ragged prefill {name}, {B} rows padded to {L}, lengths {min(lens)} .. {max(lens)}] (max, rms) error ratio library / HF "
          "against the fp32 model on real positions: " + ", ".join(f"{k} ({v[0] / v[2]:.3f}, {v[1] / v[3]:.3f})" for k, v in figures.items())
          + f"; max |logit lib - hf| {float((lib - hf).abs().max()):.4g} at max |logit| {float(hf.abs().max()):.4g}", flush=True)
    for k, v in figures.items():
        assert v[0] <= 1.5 * v[2] and v[1] <= 1.5 * v[3], (k, v)


def test_ragged_prefill_error_is_within_hfs_own_fp16_error_small_decoder(small):
    llm, dec, llm32 = small
    lengths = SMALL_SHAPES[0][1]
    _check_against_hf("small decoder", llm, dec, llm32, 80, [lengths[i % len(lengths)] for i in range(39)], seed=3)
    _check_against_hf("small decoder", llm, dec, llm32, 300, [SMALL_SHAPES[1][1][i % 5] for i in range(10)], seed=4)


def test_ragged_prefill_error_is_within_hfs_own_fp16_error_vicuna_width(vicuna):
    llm, dec, llm32 = vicuna
    g = torch.Generator(device="cpu").manual_seed(48)
    _check_against_hf("Vicuna width", llm, dec, llm32, 48, torch.randint(33, 49, (200,), generator=g).tolist(), seed=3)


# ------------------------------------------------------------------------------------------ 4. the classifier at Vicuna width
def test_classifier_decodes_distinct_texts_natively_and_follows_hf_generate(vicuna):
    llm, dec, _ = vicuna
    cfg = mo.Config(mode=mo.MODE_ENCODE_IMG, num_classes=10)
    enc = make_classifier(cfg, max_batch=20)
    try:
        enc.init_synthetic(seed=0)
        tok = WordHashTokenizer(32000)
        x = torch.from_numpy(mo.synthetic_image(cfg, seed=11)).to(DEV)
        B, n, sigma, seed = 200, 20, 0.5, 42
        emb = torch.cat([enc.encode_img_noisy(x, lo, min(enc.max_batch, B - lo), sigma, seed) for lo in range(0, B, enc.max_batch)]).to(torch.float16)
        texts = [PROMPTS[i % len(PROMPTS)] for i in range(B)]
        hip = MiniGPT4Classifier(enc, llm, tok, PROMPTS[0], AnswerLabelMap(4, ()), max_new_tokens=n, max_batch=B, decode="hip", prefill="hip",
                                 ragged="hip")
        batch = [hip.get_context_emb(t, [emb[i][None]]) for i, t in enumerate(texts)]
        assert len({e.shape[1] for e in batch}) == len(PROMPTS) >= 4    # four distinct token lengths
        calls = {"n": 0}
        hook = llm.register_forward_pre_hook(lambda *_: calls.__setitem__("n", calls["n"] + 1))
        try:
            answers = hip.generate_from_embeds(emb, texts)
            again = hip.generate_from_embeds(emb, texts)
            assert calls["n"] == 0                                     # no HF forward ran: warm-up, capture and both replays are native
        finally:
            hook.remove()
        s = hip.decode_stats
        assert s["hf_calls"] == 0 and s["graph_captures"] == 1 and s["graph_replays"] == 2
        assert s["hip_prefills"] == 2 and s["hip_steps"] == 2 * (n - 1)          # counted as on the shared path
        assert answers == again and len(answers) == B
        for p in PROMPTS:                                              # the same classifier, once per distinct text, on that text's rows
            idx = [i for i, t in enumerate(texts) if t == p]
            assert hip.generate_from_embeds(emb[idx], p) == [answers[i] for i in idx], p
        assert hip.decode_stats["hf_calls"] == 0
        # against HF's own ragged generate on the same padded embeds
        embs, mask, starts = left_pad_embeds(batch)
        hf = MiniGPT4Classifier(enc, llm, tok, PROMPTS[0], AnswerLabelMap(4, ()), max_new_tokens=n, max_batch=B, decode="hf")
        with torch.no_grad():
            out = llm.generate(inputs_embeds=embs, attention_mask=mask, max_new_tokens=n, output_scores=True, return_dict_in_generate=True,
                               **hf.hf_generate_kwargs())
            hf_tokens, hf_scores = out.sequences, torch.stack(out.scores, dim=1).float()
            hf_first, _, _ = _model_prefill_padded(llm, embs, mask.bool())
            kb, vb = lu.sentinel_cache(llm.config.num_hidden_layers, llm.config.num_attention_heads, B, embs.shape[1] + 1)
            lib_first = dec.prefill(embs.contiguous(), kb, vb, starts=starts)
            del kb, vb
            tokens = hip._generate_graph(embs, starts)
        assert hip._decode_outputs(tokens) == answers
        d_first = float((lib_first - hf_first).abs().max())
        eps = 2.0 * d_first
        v = greedy_decode_parity(hf_tokens, hf_scores, tokens, eps)
        print(f"[ragged classifier, {B} rows, lengths {sorted({e.shape[1] for e in batch})}] largest first-token |lib - hf| {d_first:.4g}, "
              f"eps {eps:.4g}; {v['identical']}/{B} rows identical to HF, {v['decisive_identical']}/{v['decisive']} decisive rows identical, "
              f"largest HF margin at a first divergence {v['max_margin_at_divergence']:.4g}", flush=True)
        assert not v["violations"], v
        assert v["decisive_identical"] == v["decisive"] and v["diverged"] <= B - v["decisive"], v
        assert v["decisive"] >= B // 10, v                             # the rule must bite on a meaningful number of rows
    finally:
        enc.close()


# ------------------------------------------------------------------------------------------ 5. one graph per bucket
def test_prompts_of_one_bucket_share_one_graph(small):
    llm, _, _ = small
    tok = WordHashTokenizer(320)
    prompts = prepare_texts(["<Img><ImageHere></Img> " + " ".join(f"word{i}" for i in range(k)) for k in (3, 5, 9)])
    g = torch.Generator(device="cpu").manual_seed(21)
    emb = (torch.randn(100, 32, 512, generator=g) * 0.02).to(DEV).to(torch.float16)
    bucketed = MiniGPT4Classifier(None, llm, tok, prompts[0], AnswerLabelMap(4, ()), max_new_tokens=6, max_batch=100, decode="hip", prefill="hip",
                                  ragged="hip", prompt_bucket=16)
    plain = MiniGPT4Classifier(None, llm, tok, prompts[0], AnswerLabelMap(4, ()), max_new_tokens=6, max_batch=100, decode="hip", prefill="hip",
                               ragged="hip")
    lengths = [32 + sum(s.shape[1] for s in plain._segment_embeddings(p, emb.device)) for p in prompts]
    assert len(set(lengths)) == 3 and len({(n + 15) // 16 for n in lengths}) == 1 and all(n % 16 for n in lengths), lengths
    got, want = [], []
    for p in prompts:                                                  # a per-image question: assign the prompt, then call
        bucketed.prompt = p
        plain.prompt = p
        got.append(bucketed.generate_from_embeds(emb, bucketed.prompt))
        want.append(plain.generate_from_embeds(emb, plain.prompt))
    sb, sp = bucketed.decode_stats, plain.decode_stats
    assert sb["graph_captures"] == 1 and sb["graph_replays"] == 3 and sb["hf_calls"] == 0 and sb["hip_prefills"] == 3
    assert sp["graph_captures"] == 3 and sp["graph_replays"] == 3 and sp["hf_calls"] == 0
    assert got == want
    assert len({tuple(a) for a in got}) > 1                            # the prompts do change the answers: the starts were refreshed


# ------------------------------------------------------------------------------------------ 6. certify
def test_certify_with_a_prompt_bucket_equals_certify_without(small):
    llm, _, _ = small
    cfg = dataclasses.replace(mo.tiny_config(mode=mo.MODE_ENCODE_IMG, num_classes=10), proj_dim=512)
    enc = make_classifier(cfg, max_batch=100)
    try:
        missing, unexpected = enc.load_state_dict(mo.init_params(cfg, 20251121))
        assert not missing and not unexpected
        tok = WordHashTokenizer(320)
        x = torch.from_numpy(mo.synthetic_image(cfg)).to(DEV)
        prompt, sigma, seed, mnt = PROMPTS[1], 0.5, 7, 5
        probe = MiniGPT4Classifier(enc, llm, tok, prompt, AnswerLabelMap(4, ()), max_new_tokens=mnt, max_batch=100, decode="hip", prefill="hip")
        seen = probe.generate_from_embeds(enc.encode_img_noisy(x, 0, 100, sigma, seed).to(torch.float16), prompt)
        vocab = sorted(set(seen), key=lambda a: (-seen.count(a), a))[:3]
        results = {}
        for bucket in (None, 16):
            kw = dict(ragged="hip", prompt_bucket=bucket)
            clf = MiniGPT4Classifier(enc, llm, tok, prompt, AnswerLabelMap(len(vocab) + 1, vocab, frozen=True), max_new_tokens=mnt, max_batch=100,
                                     decode="hip", prefill="hip", **kw)
            s = cg.Smooth(clf, len(vocab) + 1, sigma, seed=seed, non_certifiable=(clf.label_map.other_id,))
            results[bucket] = (s.certify(x, 100, 100, 0.001, 100), list(clf.last_answers), dict(clf.decode_stats))
        (lab_a, rad_a), ans_a, st_a = results[None]
        (lab_b, rad_b), ans_b, st_b = results[16]
        print(f"[certify with prompt_bucket 16] {(lab_b, rad_b)} against {(lab_a, rad_a)} without; {len(set(ans_a))} distinct answers", flush=True)
        assert (lab_a, rad_a) == (lab_b, rad_b) and ans_a == ans_b and len(ans_a) == 200
        assert st_a["hf_calls"] == st_b["hf_calls"] == 0 and st_b["hip_prefills"] == st_a["hip_prefills"] == 2
    finally:
        enc.close()
