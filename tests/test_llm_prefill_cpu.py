"""prefill="hip" (the native LLaMA prefill, csrc/llm_prefill.hip) without a GPU: the two new cgpt_llm_* entries are declared and bound
with the declared signature and refuse null arguments before any device call; the keyword never selects another engine; the
default builds no extra state; the agent forwards the keyword."""
import ctypes as C
import os
import re

import pytest
import torch

import certifiedgpt_amd as cg
from certifiedgpt_amd import _lib
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import MiniGPT4Classifier, prepare_texts
from toy_llm import StubEncoder, ToyTokenizer, tiny_llama

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPT = prepare_texts(["<Img><ImageHere></Img> what is this"])[0]
PREFILL_ENTRIES = ["cgpt_llm_prefill_reserve", "cgpt_llm_prefill"]

_CTYPES = {"cgpt_llm_handle": C.c_void_p, "const void*": C.c_void_p, "void*": C.c_void_p, "void* const*": C.c_void_p,
           "float*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}


def _classifier(llm, **kw):
    return MiniGPT4Classifier(StubEncoder(), llm, ToyTokenizer(), PROMPT, AnswerLabelMap(4, ()), max_new_tokens=3, **kw)


# ------------------------------------------------------------------------------------------ the C-ABI
def test_header_declares_and_binding_matches_the_prefill_entries():
    text = open(os.path.join(ROOT, "include", "cgpt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = cg.lib()
    for name in PREFILL_ENTRIES:
        m = re.search(r"cgpt_status\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, f"cgpt.h does not declare {name}"
        assert hasattr(L, name), f"libcgpt.so does not export {name}"
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        types = [re.sub(r"\s*\b[A-Za-z_0-9]+$", "", p).replace(" *", "*") for p in params]      # drop the parameter name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int32
        assert [_CTYPES[t] for t in types] == list(args), (name, types)
    assert "The PREFILL stays with the caller" not in text             # the section describes both ways now
    assert "cgpt_llm_prefill:" in text or "or cgpt_llm_prefill" in text


def test_prefill_and_step_take_the_same_cache_arguments():
    """Same pointer tables and stride as cgpt_llm_step: one cache layout for both entries."""
    step, prefill = _lib.SIGNATURES["cgpt_llm_step"][1], _lib.SIGNATURES["cgpt_llm_prefill"][1]
    assert list(step[4:]) == list(prefill[4:])


def test_null_handle_and_null_arguments_are_errors_not_crashes():
    L = cg.lib()
    assert L.cgpt_llm_prefill_reserve(None, 200, 44) == 1              # CGPT_ERR_INVALID
    assert b"cgpt_llm_prefill_reserve" in L.cgpt_last_error()
    assert L.cgpt_llm_prefill(None, None, 1, 4, None, None, 8, None, None) == 1
    assert b"cgpt_llm_prefill" in L.cgpt_last_error()
    buf = (C.c_uint16 * 64)()
    assert L.cgpt_llm_prefill(None, C.cast(buf, C.c_void_p), 1, 4, None, None, 8, C.cast(buf, C.c_void_p), None) == 1


# ------------------------------------------------------------------------------------------ the keyword
@pytest.mark.parametrize("decode", ["hf", "graph"])
def test_prefill_hip_with_another_engine_is_a_value_error(decode):
    with pytest.raises(ValueError) as e:
        _classifier(tiny_llama(), decode=decode, prefill="hip")
    assert 'decode="hip"' in str(e.value) and decode in str(e.value)


def test_prefill_hip_is_a_value_error_by_default_engine_and_unknown_values_are_refused():
    with pytest.raises(ValueError):
        _classifier(tiny_llama(), prefill="hip")                       # decode defaults to "hf"
    with pytest.raises(ValueError):
        _classifier(tiny_llama(), decode="graph", prefill="native")
    with pytest.raises(ValueError):                                    # an unsupported decoder stays a ValueError, whatever the prefill
        _classifier(tiny_llama(), decode="hip", prefill="hip")


@pytest.mark.parametrize("decode", ["hf", "graph"])
def test_prefill_model_is_the_default_and_builds_no_extra_state(decode):
    plain = _classifier(tiny_llama(), decode=decode)
    named = _classifier(tiny_llama(), decode=decode, prefill="model")
    for clf in (plain, named):
        assert clf.prefill == "model" and clf._hip is None and clf.routed_linears == 0
        assert clf.decode_stats["hip_prefills"] == 0 and clf.decode_stats["hip_steps"] == 0
    assert sorted(vars(plain)) == sorted(vars(named))
    llm = tiny_llama()
    before = {n: m.forward for n, m in llm.named_modules() if isinstance(m, torch.nn.Linear)}
    clf = _classifier(llm, decode=decode, prefill="model")
    assert all(m.forward == before[n] for n, m in llm.named_modules() if isinstance(m, torch.nn.Linear))    # nothing patched
    clf.generate_from_embeds(torch.zeros(2, 4, 64), PROMPT)            # CPU tensors: the HF call
    assert clf.decode_stats["hf_calls"] == 1 and clf.decode_stats["hip_prefills"] == 0


def test_graph_cache_key_names_the_prefill_engine():
    clf = _classifier(tiny_llama(), decode="graph")
    embs = torch.zeros(2, 4, 64)
    key_model = clf._graph_key(embs)
    assert key_model == clf._graph_key(embs.clone())
    clf.prefill = "hip"                                                # what a decode="hip", prefill="hip" classifier carries
    key_hip = clf._graph_key(embs)
    assert key_hip != key_model
    assert [a for a, b in zip(key_model, key_hip) if a != b] == ["model"]       # and differs in nothing else
    assert clf._graph_key(torch.zeros(3, 4, 64)) != key_hip and clf._graph_key(torch.zeros(2, 5, 64)) != key_hip


# ------------------------------------------------------------------------------------------ the agent
def test_agent_documents_and_forwards_the_prefill_engine(monkeypatch):
    import inspect
    from certifiedgpt_amd.agents import minigpt4_certify_agent as agent
    src = inspect.getsource(agent)
    assert 'prefill: "model" | "hip"' in src and 'gen_cfg.get("prefill", "model")' in src          # documented; the default stays "model"
    seen = {}

    class Recorder:
        def __init__(self, *args, **kw):
            seen.update(kw)

    import certifiedgpt_amd.minigpt4 as minigpt4                       # the agent imports the class from there when it builds
    monkeypatch.setattr(minigpt4, "MiniGPT4Classifier", Recorder)
    enc = StubEncoder()
    gen = {"prompt": PROMPT, "answers": ["a", "b", "c"], "decode": "hip", "prefill": "hip"}
    agent.build_generating_classifier(enc, gen, 4, tokenizer=ToyTokenizer(), llama_model=tiny_llama())
    assert seen["decode"] == "hip" and seen["prefill"] == "hip"
    seen.clear()
    del gen["prefill"]
    agent.build_generating_classifier(enc, gen, 4, tokenizer=ToyTokenizer(), llama_model=tiny_llama())
    assert seen["prefill"] == "model"
