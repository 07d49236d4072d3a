"""ragged="hip" / prompt_bucket (left-padded prompts on the native LLaMA engine, cgpt_llm_*_ragged) without a GPU: the three new
entries are declared, exported and bound with the declared signature and refuse null arguments before any device call; the keywords
never select another engine and the defaults build no extra state; the padding arithmetic is one pure function that reproduces
today's left padding; the agent forwards the keywords and assigns a per-image question before that image's call."""
import ctypes as C
import os
import re

import pytest
import torch

import certifiedgpt_amd as cg
from certifiedgpt_amd import _lib
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import MiniGPT4Classifier, left_pad_embeds, prepare_texts
from toy_llm import StubEncoder, ToyTokenizer, tiny_llama

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPT = prepare_texts(["<Img><ImageHere></Img> what is this"])[0]
RAGGED_ENTRIES = {"cgpt_llm_prefill_ragged": "cgpt_llm_prefill", "cgpt_llm_step_ragged": "cgpt_llm_step",
                  "cgpt_llm_greedy_ragged": "cgpt_llm_greedy"}
STARTS_AT = {"cgpt_llm_prefill_ragged": 4, "cgpt_llm_step_ragged": 4, "cgpt_llm_greedy_ragged": 4}     # after the length / position
INVALID = 1

_CTYPES = {"cgpt_llm_handle": C.c_void_p, "const void*": C.c_void_p, "void*": C.c_void_p, "void* const*": C.c_void_p,
           "float*": C.c_void_p, "const float*": C.c_void_p, "const int64_t*": C.c_void_p, "int64_t*": C.c_void_p,
           "const int32_t*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}


def _classifier(llm, **kw):
    return MiniGPT4Classifier(StubEncoder(), llm, ToyTokenizer(), PROMPT, AnswerLabelMap(4, ()), max_new_tokens=3, **kw)


def _declared(code, name):
    m = re.search(r"cgpt_status\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m, f"cgpt.h does not declare {name}"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    names = [re.search(r"([A-Za-z_0-9]+)$", p).group(1) for p in params]
    types = [re.sub(r"\s*\b[A-Za-z_0-9]+$", "", p).replace(" *", "*") for p in params]
    return names, types


# ------------------------------------------------------------------------------------------ the C-ABI
def test_header_declares_and_binding_matches_the_ragged_entries():
    text = open(os.path.join(ROOT, "include", "cgpt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = cg.lib()
    for name, plain in RAGGED_ENTRIES.items():
        names, types = _declared(code, name)
        assert hasattr(L, name), f"libcgpt.so does not export {name}"
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int32
        assert [_CTYPES[t] for t in types] == list(args), (name, types)
        # the plain sibling's arguments in the plain sibling's order, with `const int32_t* starts_dev` after the length / position
        pnames, ptypes = _declared(code, plain)
        at = STARTS_AT[name]
        assert names[at] == "starts_dev" and types[at] == "const int32_t*", (name, names, types)
        assert names[:at] + names[at + 1:] == pnames and types[:at] + types[at + 1:] == ptypes, name
    for word in ("starts_dev", "clamp", "NEVER written", "replay"):     # layout, clamp, rows written, read when the kernels run
        assert word in text, word


def test_ragged_and_plain_entries_take_the_same_cache_arguments():
    for name, plain in RAGGED_ENTRIES.items():
        ragged, base = list(_lib.SIGNATURES[name][1]), list(_lib.SIGNATURES[plain][1])
        at = STARTS_AT[name]
        assert ragged[:at] + ragged[at + 1:] == base, name
    step, prefill = _lib.SIGNATURES["cgpt_llm_step_ragged"][1], _lib.SIGNATURES["cgpt_llm_prefill_ragged"][1]
    assert list(step[4:]) == list(prefill[4:])                         # starts, the two pointer tables, the stride, logits, stream


def test_null_handle_and_null_starts_are_errors_not_crashes():
    L = cg.lib()
    buf = (C.c_uint64 * 64)()
    p = C.cast(buf, C.c_void_p)
    calls = {
        "cgpt_llm_prefill_ragged": lambda h, st: L.cgpt_llm_prefill_ragged(h, p, 1, 4, st, p, p, 8, p, None),
        "cgpt_llm_step_ragged": lambda h, st: L.cgpt_llm_step_ragged(h, p, 1, 4, st, p, p, 8, p, None),
        "cgpt_llm_greedy_ragged": lambda h, st: L.cgpt_llm_greedy_ragged(h, p, 1, 4, st, 2, 0, None, 0, 0, p, p, 8, p, None, None),
    }
    for name, call in calls.items():
        assert call(None, p) == INVALID                                # a null handle
        assert name.encode() in L.cgpt_last_error(), (name, L.cgpt_last_error())
        # a null starts_dev is refused before the handle is looked at (the "handle" here is host memory that is never read)
        assert call(p, None) == INVALID
        msg = L.cgpt_last_error()
        assert name.encode() in msg and b"starts_dev" in msg, (name, msg)
        assert call(None, None) == INVALID


# ------------------------------------------------------------------------------------------ the keywords
@pytest.mark.parametrize("decode, prefill", [("hf", "model"), ("graph", "model"), ("hip", "model")])
def test_ragged_hip_with_another_engine_is_a_value_error_naming_both(decode, prefill):
    with pytest.raises(ValueError) as e:
        _classifier(tiny_llama(), decode=decode, prefill=prefill, ragged="hip")
    msg = str(e.value)
    assert 'decode="hip"' in msg and 'prefill="hip"' in msg and repr(decode) in msg and repr(prefill) in msg


def test_unknown_ragged_values_and_bad_buckets_are_value_errors():
    with pytest.raises(ValueError):
        _classifier(tiny_llama(), ragged="native")
    with pytest.raises(ValueError):
        _classifier(tiny_llama(), ragged=None)
    with pytest.raises(ValueError) as e:                               # a bucket without the native ragged engine
        _classifier(tiny_llama(), prompt_bucket=16)
    assert 'ragged="hip"' in str(e.value)
    with pytest.raises(ValueError):
        _classifier(tiny_llama(), decode="graph", prompt_bucket=16)
    for bad in (0, -16, 2.0, "16", True):
        with pytest.raises(ValueError):
            _classifier(tiny_llama(), decode="hip", prefill="hip", ragged="hip", prompt_bucket=bad)
    with pytest.raises(ValueError):                                    # an unsupported decoder stays a ValueError under the new keywords
        _classifier(tiny_llama(), decode="hip", prefill="hip", ragged="hip", prompt_bucket=16)


@pytest.mark.parametrize("decode", ["hf", "graph"])
def test_defaults_build_no_extra_state(decode):
    plain = _classifier(tiny_llama(), decode=decode)
    named = _classifier(tiny_llama(), decode=decode, ragged="hf", prompt_bucket=None)
    assert plain.ragged == named.ragged == "hf" and plain.prompt_bucket is named.prompt_bucket is None
    assert sorted(vars(plain)) == sorted(vars(named))
    skip = {"encoder", "llama_model", "llama_tokenizer", "label_map"}   # objects built per call; everything else compares by value
    assert {k: v for k, v in vars(plain).items() if k not in skip} == {k: v for k, v in vars(named).items() if k not in skip}
    embs = torch.zeros(2, 4, 64)
    assert plain._graph_key(embs) == named._graph_key(embs) and len(plain._graph_key(embs)) == 8        # the key of today
    assert plain._graph_key(embs, ragged=True) != plain._graph_key(embs)
    assert plain._graph_key(embs, ragged=True)[:8] == plain._graph_key(embs)
    plain.generate_from_embeds(torch.zeros(2, 4, 64), [PROMPT, PROMPT + " now"])      # different texts: the HF call, counted
    assert plain.decode_stats["hf_calls"] == 1 and plain.decode_stats["hip_prefills"] == 0 and plain.decode_stats["graph_captures"] == 0


# ------------------------------------------------------------------------------------------ the padding function
def _todays_left_padding(batch_embs):
    """The padding loop of `generate_from_embeds` before this function existed (minigpt_base.py:407-416), restated."""
    B = len(batch_embs)
    max_len = max(e.shape[1] for e in batch_embs)
    embs = torch.zeros([B, max_len, batch_embs[0].shape[2]], dtype=batch_embs[0].dtype)
    mask = torch.zeros([B, max_len], dtype=torch.int)
    for i, emb in enumerate(batch_embs):
        embs[i, -emb.shape[1]:] = emb[0]
        mask[i, -emb.shape[1]:] = 1
    return embs, mask


@pytest.mark.parametrize("bucket", [None, 1])
def test_padding_without_a_bucket_is_todays_left_padding(bucket, monkeypatch):
    llm = tiny_llama()
    clf = _classifier(llm)
    texts = [PROMPT, PROMPT + " now", prepare_texts(["<Img><ImageHere></Img> a much longer question about the picture"])[0], PROMPT]
    g = torch.Generator().manual_seed(3)
    img = torch.randn(4, 4, 64, generator=g)
    batch = [clf.get_context_emb(t, [img[i][None]]) for i, t in enumerate(texts)]
    assert len({e.shape[1] for e in batch}) == 3
    want_e, want_m = _todays_left_padding(batch)
    embs, mask, starts = left_pad_embeds(batch, bucket)
    assert torch.equal(embs, want_e) and torch.equal(mask, want_m) and mask.dtype == want_m.dtype and embs.dtype == want_e.dtype
    assert starts.dtype == torch.int32 and starts.tolist() == [want_e.shape[1] - e.shape[1] for e in batch]
    # and it is what the classifier hands to HF `generate` for these texts
    seen = {}

    def fake_generate(**kw):
        seen.update(kw)
        return torch.zeros(4, 3, dtype=torch.long)

    monkeypatch.setattr(llm, "generate", fake_generate)
    clf.generate_from_embeds(img, texts)
    assert torch.equal(seen["inputs_embeds"], want_e) and torch.equal(seen["attention_mask"], want_m)


def test_padding_to_a_bucket_of_16():
    g = torch.Generator().manual_seed(4)
    lens = [5, 9, 12, 17]
    batch = [torch.randn(1, n, 8, generator=g) + 3.0 for n in lens]
    embs, mask, starts = left_pad_embeds(batch, 16)
    assert tuple(embs.shape) == (4, 32, 8) and tuple(mask.shape) == (4, 32)
    assert starts.tolist() == [27, 23, 20, 15] and starts.dtype == torch.int32
    for i, (n, e) in enumerate(zip(lens, batch)):
        assert torch.equal(embs[i, 32 - n:], e[0]) and bool((embs[i, :32 - n] == 0).all())      # pads are zeros
        assert mask[i].tolist() == [0] * (32 - n) + [1] * n
    # a length that is a multiple of the bucket is not padded further; groups of rows that share a length
    embs, mask, starts = left_pad_embeds([torch.ones(3, 16, 8), torch.ones(2, 7, 8)], 16)
    assert tuple(embs.shape) == (5, 16, 8) and starts.tolist() == [0, 0, 0, 9, 9] and int(mask.sum()) == 3 * 16 + 2 * 7
    embs, _, starts = left_pad_embeds([torch.ones(3, 44, 8)], 16)      # a shared prompt padded up to its bucket
    assert tuple(embs.shape) == (3, 48, 8) and starts.tolist() == [4, 4, 4] and bool((embs[:, :4] == 0).all())


def test_a_row_with_no_real_token_and_a_bad_bucket_are_value_errors():
    with pytest.raises(ValueError):
        left_pad_embeds([torch.ones(1, 5, 8), torch.ones(1, 0, 8)], 16)
    with pytest.raises(ValueError):
        left_pad_embeds([torch.ones(1, 0, 8)])
    with pytest.raises(ValueError):
        left_pad_embeds([], 16)
    for bad in (0, -1, 1.5, "16", True):
        with pytest.raises(ValueError):
            left_pad_embeds([torch.ones(1, 5, 8)], bad)


# ------------------------------------------------------------------------------------------ the agent
def test_agent_documents_and_forwards_ragged_and_prompt_bucket(monkeypatch):
    import inspect
    from certifiedgpt_amd.agents import minigpt4_certify_agent as agent
    src = inspect.getsource(agent)
    assert 'ragged: "hf" | "hip"' in src and "prompt_bucket" in agent.__doc__ and 'gen_cfg.get("ragged", "hf")' in src
    seen = {}

    class Recorder:
        def __init__(self, *args, **kw):
            seen.update(kw)

    import certifiedgpt_amd.minigpt4 as minigpt4
    monkeypatch.setattr(minigpt4, "MiniGPT4Classifier", Recorder)
    enc = StubEncoder()
    gen = {"prompt": PROMPT, "answers": ["a", "b", "c"], "decode": "hip", "prefill": "hip", "ragged": "hip", "prompt_bucket": 16}
    agent.build_generating_classifier(enc, gen, 4, tokenizer=ToyTokenizer(), llama_model=tiny_llama())
    assert seen["ragged"] == "hip" and seen["prompt_bucket"] == 16 and seen["decode"] == "hip" and seen["prefill"] == "hip"
    seen.clear()
    del gen["ragged"], gen["prompt_bucket"]
    agent.build_generating_classifier(enc, gen, 4, tokenizer=ToyTokenizer(), llama_model=tiny_llama())
    assert seen["ragged"] == "hf" and seen["prompt_bucket"] is None


class _RecordingSmooth:
    """Stands where Smooth stands in CertifyLoop: records the classifier's prompt at the moment of every call."""
    process_group = None

    class _Clf:
        prompt = "the configured prompt"

    def __init__(self):
        self.base_classifier = self._Clf()
        self.calls = []

    def certify(self, x, n0, n, alpha, batch_size):
        self.calls.append(("certify", int(x[0]), self.base_classifier.prompt))
        return 1, 0.5

    def predict(self, x, n, alpha, batch_size):
        self.calls.append(("predict", int(x[0]), self.base_classifier.prompt))
        return 1

    def certify_many(self, xs, n0, n, alpha, batch_size):
        self.calls.append(("certify_many", len(xs), self.base_classifier.prompt))
        return [(1, 0.5)] * len(xs)


SM_CFG = {"n0": 4, "n": 8, "alpha": 0.05, "batch_size": 4}


def test_a_dataset_of_triples_assigns_each_images_prompt_before_its_certify():
    from certifiedgpt_amd.agents import minigpt4_certify_agent as agent
    questions = ["what colour is the bus", "is it raining", "how many people are there in this picture"]
    data = [(torch.full((1,), float(i)), i % 2, q) for i, q in enumerate(questions)]
    for mode in ("certify", "predict"):
        smooth, loop = _RecordingSmooth(), agent.CertifyLoop()
        records = loop.certify_dataset(dict(SM_CFG), data, smooth, mode=mode)
        assert len(records) == 3
        want = [prepare_texts(["<Img><ImageHere></Img> " + q])[0] for q in questions]     # as build_generating_classifier builds it
        assert smooth.calls == [(mode, i, p) for i, p in enumerate(want)]
    # the same prompt the builder gives a configured `question`
    seen = {}

    class Recorder:
        def __init__(self, *args, **kw):
            seen["prompt"] = args[3]

    import certifiedgpt_amd.minigpt4 as minigpt4
    orig = minigpt4.MiniGPT4Classifier
    minigpt4.MiniGPT4Classifier = Recorder
    try:
        agent.build_generating_classifier(StubEncoder(), {"question": questions[0], "answers": ["a"]}, 4, tokenizer=ToyTokenizer(),
                                          llama_model=tiny_llama())
    finally:
        minigpt4.MiniGPT4Classifier = orig
    assert seen["prompt"] == want[0] == agent.question_prompt(questions[0])
    # pairs behave as before: the prompt is never touched
    smooth, loop = _RecordingSmooth(), agent.CertifyLoop()
    loop.certify_dataset(dict(SM_CFG), [(x, lab) for x, lab, _ in data], smooth)
    assert [c[2] for c in smooth.calls] == ["the configured prompt"] * 3


@pytest.mark.parametrize("extra", [{"images_per_pass": 2}, {"shard": "images"}])
def test_triples_under_a_grouping_mode_raise(extra):
    from certifiedgpt_amd.agents import minigpt4_certify_agent as agent
    data = [(torch.zeros(1), 0, "what is this"), (torch.ones(1), 1, "and this")]
    smooth, loop = _RecordingSmooth(), agent.CertifyLoop()
    with pytest.raises(ValueError) as e:
        loop.certify_dataset(dict(SM_CFG, **extra), data, smooth)
    assert "images_per_pass: 1" in str(e.value) and "shard: samples" in str(e.value)
    assert smooth.calls == [] and smooth.base_classifier.prompt == "the configured prompt"
    pairs = [(x, lab) for x, lab, _ in data]                           # pairs keep working under images_per_pass: 2
    if "images_per_pass" in extra:
        loop.certify_dataset(dict(SM_CFG, **extra), pairs, smooth)
        assert smooth.calls == [("certify_many", 2, "the configured prompt")]
