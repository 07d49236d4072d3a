"""Sampled decoding (sample="hip") without a GPU: the stream (`sample_uniform`) against oracle.philox, the law
(`sample_token_law`) against transformers' own logits processors, and the plumbing -- keyword validation, which calls stay on the
native engine, the draw ids `sample_counts` hands over, the running counter, the C declarations, the agent's keys and the graph key.

tests/test_gpu_llm_sample.py holds the kernel to the law stated here."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import certifiedgpt_amd as cg
from certifiedgpt_amd import _lib
from certifiedgpt_amd import minigpt4
from certifiedgpt_amd.agents import minigpt4_certify_agent as agent
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import MiniGPT4Classifier, WordHashTokenizer, check_sample_settings, sample_token_law, sample_uniform
from oracle import philox

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAT_KW = dict(do_sample=True, top_p=0.9, repetition_penalty=1.05, temperature=1.0)
CHAT = (True, 1.0, 50, 0.9, 1.05)


# ------------------------------------------------------------------------------------------ C1. the stream
def test_stream_is_word_0_of_counter_word_3():
    cases = [(0, 0, 0), (1234, 7, 19), (0x9E3779B97F4A7C15, 2 ** 32 - 1, 0), (0x9E3779B97F4A7C15, 2 ** 32, 3), (2 ** 64 - 1, 2 ** 63 + 5, 19)]
    for seed, draw, step in cases:
        words = philox.philox4x32_10(step, 3, draw & 0xFFFFFFFF, draw >> 32, seed & 0xFFFFFFFF, seed >> 32)
        want = (int(words[0]) >> 8) * 2.0 ** -24
        got = sample_uniform(seed, draw, step)
        assert got == want and 0.0 <= got < 1.0
        assert float(np.float32(got)) == got                           # 24 bits: exact in fp32
        noise = philox.philox4x32_10(step, 0, draw & 0xFFFFFFFF, draw >> 32, seed & 0xFFFFFFFF, seed >> 32)
        assert int(noise[0]) != int(words[0])                          # not the noise stream of the same (seed, id)
    assert minigpt4.PHILOX_WORD_SAMPLE == 3
    header = open(os.path.join(ROOT, "certifiedgpt_amd", "csrc", "philox.h")).read()
    assert "PHILOX_WORD_SAMPLE = 3" in header and "PHILOX_WORD_NOISE = 0" in header
    assert len({sample_uniform(5, d, s) for d in range(50) for s in range(20)}) == 1000


# ------------------------------------------------------------------------------------------ C2. the law
def _hf_kept(logits, prev, top_k, top_p, T, pen):
    from transformers import RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    ids, scores = torch.as_tensor(prev)[None], logits[None].clone()
    if pen != 1:
        scores = RepetitionPenaltyLogitsProcessor(pen)(ids, scores)
    scores = TemperatureLogitsWarper(float(T))(ids, scores)
    if top_k:
        scores = TopKLogitsWarper(top_k)(ids, scores)
    if top_p < 1:
        scores = TopPLogitsWarper(top_p)(ids, scores)
    return scores[0] > float("-inf")


@pytest.mark.parametrize("top_k, top_p, T, pen", [(50, 0.9, 1, 1.05), (0, 0.9, 0.7, 1), (5, 1.0, 1, 1.3)])
@pytest.mark.parametrize("V", [64, 320])
def test_kept_set_is_the_one_of_transformers_processors(V, top_k, top_p, T, pen):
    g = torch.Generator().manual_seed(V)
    for row in range(50):
        logits = torch.randn(V, generator=g) * 2
        assert logits.unique().numel() == V                            # tie-free
        prev = torch.randint(0, V, (5,), generator=g)
        prev[4] = prev[3]
        prev[0] = int(logits.argmax())
        token, kept = sample_token_law(logits, prev, 0.5, T, top_k, top_p, pen)
        assert torch.equal(kept, _hf_kept(logits, prev, top_k, top_p, T, pen)), row
        assert bool(kept[token]) and 1 <= int(kept.sum()) <= (top_k or V)


def test_ties_at_the_cuts_keep_the_whole_group_and_the_law_ignores_the_column_order():
    logits = torch.log(torch.tensor([0.5, 0.2, 0.2, 0.1], dtype=torch.float64))
    _, kept = sample_token_law(logits, [], 0.0, top_p=0.6)             # sorted masses 0.5, 0.7: n = 2, and both 0.2s stay
    assert kept.tolist() == [True, True, True, False]
    _, kept = sample_token_law(logits, [], 0.0, top_k=2)
    assert kept.tolist() == [True, True, True, False]
    g = torch.Generator().manual_seed(0)
    row = torch.randn(64, generator=g)
    row[10] = row[20] = row[30]
    perm = torch.randperm(64, generator=g)
    for kw in (dict(top_k=int((row > row[10]).sum()) + 1), dict(top_p=float(torch.softmax(row.double(), 0)[row >= row[10]].sum()) - 1e-3)):
        _, kept = sample_token_law(row, [], 0.3, **kw)
        _, kept_p = sample_token_law(row[perm], [], 0.3, **kw)
        assert bool(kept[10]) and bool(kept[20]) and bool(kept[30]) and torch.equal(kept[perm], kept_p)


def test_dyadic_probabilities():
    logits = torch.log(torch.tensor([2.0 ** -(i + 1) for i in range(63)] + [2.0 ** -63], dtype=torch.float64))
    for u, want in ((4 / 15, 0), (10 / 15, 1), (13 / 15, 2), (14.5 / 15, 3)):      # the midpoints of the four kept intervals
        d = sample_token_law(logits, [], u, top_p=0.9, details=True)
        assert d["token"] == want and int(d["kept"].sum()) == 4 and abs(d["kept_mass"] - 0.9375) < 1e-12 and d["n"] == 4


def test_penalty_mask_and_arg_max():
    logits = torch.tensor([2.0, 1.5, -1.0, -1.4, 0.0])
    assert sample_token_law(logits, [0], 0.0, repetition_penalty=1.5, do_sample=False)[0] == 1       # 2 / 1.5 < 1.5
    assert sample_token_law(logits, [0, 0, 0], 0.0, repetition_penalty=1.2, do_sample=False)[0] == 0  # once: 1.67, not 1.16
    assert sample_token_law(logits[2:4], [0], 0.0, repetition_penalty=1.5, do_sample=False)[0] == 1  # -1 * 1.5 < -1.4
    assert sample_token_law(logits, [], 0.0, mask_eos_ids=[0], do_sample=False)[0] == 1
    assert sample_token_law(torch.zeros(8), [], 0.0, do_sample=False)[0] == 0                         # the first maximum
    token, kept = sample_token_law(logits, [], 0.999, mask_eos_ids=[0, 1])
    assert not bool(kept[0]) and not bool(kept[1]) and token == 4
    for bad in ((True, 0, 0, 0.9, 1), (True, 1, -1, 0.9, 1), (True, 1, 0, 0, 1), (True, 1, 0, 1.1, 1), (True, 1, 0, 0.9, 0)):
        with pytest.raises(ValueError):
            check_sample_settings(bad)
    assert check_sample_settings((1, 1, 50, 0.9, 1.05)) == CHAT


# ------------------------------------------------------------------------------------------ C3. the plumbing
class _Engine:
    """Stand-in for the native engine: what the classifier's constructor touches."""
    weight_bytes = None

    def __init__(self, *a, **kw):
        pass

    def set_stop_sequences(self, seqs):
        pass


def _clf(monkeypatch=None, llm=None, **kw):
    if monkeypatch is not None:
        monkeypatch.setattr(minigpt4, "_HipDecoder", _Engine)
    return MiniGPT4Classifier(None, llm or object(), WordHashTokenizer(96), "<ImageHere>", AnswerLabelMap(4, ()), max_batch=4, **kw)


def test_sample_needs_the_native_decode():
    for decode in ("hf", "graph"):
        with pytest.raises(ValueError) as e:
            _clf(decode=decode, sample="hip")
        assert 'sample="hip"' in str(e.value) and 'decode="hip"' in str(e.value)
    with pytest.raises(ValueError):
        _clf(sample="cuda")
    assert _clf().sample == "hf"


def test_which_calls_stay_on_the_native_engine(monkeypatch):
    clf = _clf(monkeypatch, decode="hip", sample="hip", generate_kwargs=CHAT_KW)
    assert clf._greedy_defaults() and clf._sample_settings() == CHAT
    assert not _clf(monkeypatch, decode="hip", generate_kwargs=CHAT_KW)._greedy_defaults()          # sample = "hf": HF, as before
    assert _clf(monkeypatch, decode="hip", generate_kwargs=CHAT_KW)._sample_settings() is None
    assert not _clf(monkeypatch, decode="hip", sample="hip", generate_kwargs=dict(CHAT_KW, num_beams=2))._greedy_defaults()
    assert not _clf(monkeypatch, decode="hip", sample="hip", generate_kwargs=dict(CHAT_KW, no_repeat_ngram_size=2))._greedy_defaults()
    plain = _clf(monkeypatch, decode="hip", sample="hip")                # the greedy arguments: the arg-max entries, no sampler
    assert plain._greedy_defaults() and plain._sample_settings() is None
    pen = _clf(monkeypatch, decode="hip", sample="hip", generate_kwargs=dict(repetition_penalty=1.2))
    assert pen._greedy_defaults() and pen._sample_settings() == (False, 1.0, 50, 0.9, 1.2)    # top_p 0.9: the class default
    # the checkpoint's own generation_config supplies what the call leaves out: of the five, top_k (the class passes the other four
    # with every call, as the reference does)
    gen = types.SimpleNamespace(top_k=40, do_sample=True, temperature=0.6)
    llm = types.SimpleNamespace(generation_config=gen)
    assert _clf(monkeypatch, llm=llm, decode="hip", sample="hip", generate_kwargs=CHAT_KW)._sample_settings() == (True, 1.0, 40, 0.9, 1.05)
    assert _clf(monkeypatch, llm=llm, decode="hip", sample="hip", generate_kwargs=dict(CHAT_KW, top_k=0))._sample_settings()[2] == 0
    assert _clf(monkeypatch, llm=llm, decode="hip", sample="hip")._sample_settings() is None            # the call says do_sample=False
    gen.no_repeat_ngram_size = 3                                        # a field outside the five: HF
    assert not _clf(monkeypatch, llm=llm, decode="hip", sample="hip", generate_kwargs=CHAT_KW)._greedy_defaults()
    for bad in (dict(temperature=0.0), dict(top_p=1.5), dict(top_k=-1), dict(repetition_penalty=0)):
        with pytest.raises(ValueError):
            _clf(monkeypatch, decode="hip", sample="hip", generate_kwargs=dict(CHAT_KW, **bad))


def test_a_field_outside_the_five_takes_hf_generate():
    from toy_llm import StubEncoder, ToyTokenizer, tiny_llama
    llm = tiny_llama(seed=0)
    clf = MiniGPT4Classifier(StubEncoder(), llm, ToyTokenizer(), "<ImageHere> what is it", AnswerLabelMap(4, ()), max_new_tokens=4,
                             generate_kwargs=dict(num_beams=2))
    img, _ = clf.encoder.encode_img(torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(0)))
    clf.generate_from_embeds(img, clf.prompt)
    assert clf.decode_stats["hf_calls"] == 1 and clf.decode_stats["hip_sampled"] == 0


def test_sample_counts_hands_first_plus_row_and_the_seed_through(monkeypatch):
    clf = _clf(monkeypatch, decode="hip", sample="hip", generate_kwargs=CHAT_KW)
    seen = []

    def fake(emb, texts, draws=None):
        seen.append((emb.shape[0], draws))
        return ["x"] * emb.shape[0]

    clf.generate_from_embeds = fake
    clf.encoder = types.SimpleNamespace(encode_img_noisy=lambda x, first, num, sigma, seed, **kw: torch.zeros(num, 2, 8))
    monkeypatch.setattr(minigpt4, "vote", lambda logits, counts: None)
    x = torch.zeros(3, 8, 8)
    clf.sample_counts(x, 10, 10, 4, 0.25, 77)
    assert seen == [(4, (10, 77)), (4, (14, 77)), (2, (18, 77))]
    del seen[:]
    clf.sample_counts_pair(x, 0, 6, 6, 3, 4, 0.25, 5)
    assert seen == [(4, (0, 5)), (4, (4, 5)), (1, (8, 5))]
    # sample = "hf": the keyword does not travel
    del seen[:]
    hf = _clf(monkeypatch, decode="hip", generate_kwargs=CHAT_KW)
    hf.generate_from_embeds = lambda emb, texts: seen.append(emb.shape[0]) or ["x"] * emb.shape[0]
    hf.encoder = clf.encoder
    hf.sample_counts(x, 0, 5, 4, 0.25, 1)
    assert seen == [4, 1]


def test_draw_buffers_and_the_running_counter(monkeypatch):
    clf = _clf(monkeypatch, decode="hip", sample="hip", generate_kwargs=CHAT_KW)
    cpu = torch.device("cpu")
    ids, seed = clf._write_draws(3, (2 ** 32 - 1, 2 ** 64 - 2), cpu)
    assert ids[:3].tolist() == [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1] and seed.tolist() == [-2] and ids.shape == (4,)
    a = [clf._write_draws(2, None, cpu)[0][:2].tolist() for _ in range(2)]
    assert a == [[0, 1], [2, 3]] and clf._write_draws(1, None, cpu)[1].tolist() == [0]
    clf.reset_draws(0, seed=9)
    assert [clf._write_draws(2, None, cpu)[0][:2].tolist() for _ in range(2)] == a and clf._draw_bufs[1].tolist() == [9]
    clf.reset_draws(100)
    assert clf._write_draws(2, None, cpu)[0][:2].tolist() == [100, 101] and clf._draw_bufs[1].tolist() == [9]
    assert clf._write_draws(2, None, cpu)[0] is ids                    # persistent: a captured graph keeps reading them


def test_graph_key_carries_the_settings(monkeypatch):
    embs = types.SimpleNamespace(shape=(4, 12, 512), dtype=torch.float16, device=types.SimpleNamespace(index=0))
    plain = _clf(monkeypatch, decode="hip")._graph_key(embs)
    assert plain == (4, 12, torch.float16, 0, 20, False, "hip", "model")
    assert _clf(monkeypatch, decode="hip", sample="hip")._graph_key(embs) == plain                 # greedy arguments: the greedy graph
    chat = _clf(monkeypatch, decode="hip", sample="hip", generate_kwargs=CHAT_KW)._graph_key(embs)
    cool = _clf(monkeypatch, decode="hip", sample="hip", generate_kwargs=dict(CHAT_KW, temperature=0.7))._graph_key(embs)
    assert len({plain, chat, cool}) == 3 and chat[-2:] == ("sample", CHAT)


_CTYPES = {"cgpt_llm_handle": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p, "const int64_t*": C.c_void_p,
           "int64_t*": C.c_void_p, "const int32_t*": C.c_void_p, "int32_t*": C.c_void_p, "const uint64_t*": C.c_void_p,
           "void* const*": C.c_void_p, "void*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64,
           "cgpt_llm_sample_params": _lib.LlmSampleParams}


@pytest.mark.parametrize("name", ["cgpt_llm_sample", "cgpt_llm_sample_ragged", "cgpt_llm_sample_logits"])
def test_header_declares_and_binding_matches(name):
    text = open(os.path.join(ROOT, "include", "cgpt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"cgpt_status\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m, f"cgpt.h does not declare {name}"
    assert hasattr(cg.lib(), name), f"libcgpt.so does not export {name}"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    types_ = [re.sub(r"\s*\b[A-Za-z_0-9]+$", "", p).replace(" *", "*") for p in params]
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int32 and [_CTYPES[t] for t in types_] == list(args), types_
    fields = re.search(r"typedef struct cgpt_llm_sample_params \{(.*?)\}", code, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [f for f, _ in _lib.LlmSampleParams._fields_]
    assert C.sizeof(_lib.LlmSampleParams) == 24
    if name != "cgpt_llm_sample_logits":                               # the greedy entry's arguments, then the four new ones
        greedy = re.search(r"cgpt_status\s+" + name.replace("sample", "greedy") + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        gp = [" ".join(p.split()) for p in greedy.split(",")]
        assert params[:len(gp) - 1] == gp[:-1] and params[-1] == gp[-1] and len(params) == len(gp) + 3


def test_entries_refuse_bad_arguments_without_a_device():
    L = cg.lib()
    ok = _lib.sample_params(*CHAT)
    one = C.c_void_p(8)                                                # never dereferenced: every call is refused first

    def refused(params, ids=one, seed=one, uniforms=None, V=64, num_prev=0):
        rc = L.cgpt_llm_sample_logits(one, V, 2, V, one if num_prev else None, num_prev, num_prev, 0, 0, None, 0, 0, one, params, ids, seed,
                                      uniforms, one, None, None, None, None)
        assert rc == 1 and b"cgpt_llm_sample_logits" in L.cgpt_last_error(), L.cgpt_last_error()
        return L.cgpt_last_error()

    assert b"temperature" in refused(_lib.sample_params(True, 0.0, 50, 0.9, 1.05))
    assert b"temperature" in refused(_lib.sample_params(True, float("nan"), 50, 0.9, 1.05))
    assert b"top_p" in refused(_lib.sample_params(True, 1.0, 50, 0.0, 1.05))
    assert b"top_p" in refused(_lib.sample_params(True, 1.0, 50, 1.0001, 1.05))
    assert b"top_k" in refused(_lib.sample_params(True, 1.0, -1, 0.9, 1.05))
    assert b"repetition_penalty" in refused(_lib.sample_params(True, 1.0, 50, 0.9, 0.0))
    short = _lib.sample_params(*CHAT)
    short.struct_size = 20
    assert b"struct_size" in refused(short)
    assert b"draw_ids_dev" in refused(ok, ids=None)
    assert b"seed_dev" in refused(ok, seed=None)
    assert b"vocabulary" in refused(ok, V=131073)
    assert b"1024" in refused(ok, num_prev=1025)
    for name in ("cgpt_llm_sample", "cgpt_llm_sample_ragged"):         # a null handle is refused before anything else
        extra = (one,) if name.endswith("ragged") else ()
        rc = getattr(L, name)(None, one, 2, 4, *extra, 3, 1, None, 0, 0, one, one, 8, one, None, ok, one, one, None)
        assert rc == 1 and name.encode() in L.cgpt_last_error()


def test_agent_passes_the_keys_through(monkeypatch):
    assert "sample" in agent.__doc__ and "repetition_penalty" in agent.__doc__
    seen = {}

    class Spy:
        def __init__(self, *a, **kw):
            seen.update(kw)

    monkeypatch.setattr(minigpt4, "MiniGPT4Classifier", Spy)
    enc = types.SimpleNamespace(max_batch=4, device="cpu")
    llm = types.SimpleNamespace(parameters=lambda: [])
    base = {"prompt": "<ImageHere>", "answers": ["a", "b"], "decode": "hip"}
    agent.build_generating_classifier(enc, dict(base, sample="hip", top_k=40, **CHAT_KW), 4, tokenizer=object(), llama_model=llm)
    assert seen["sample"] == "hip" and seen["generate_kwargs"] == dict(CHAT_KW, top_k=40)
    agent.build_generating_classifier(enc, base, 4, tokenizer=object(), llama_model=llm)
    assert seen["sample"] == "hf" and seen["generate_kwargs"] is None
