"""decode="hip" (the native LLaMA token step, csrc/llm.hip and csrc/llm_step.hip) without a GPU: the model check names every unsupported property and
the constructor never builds another engine in its place; the cgpt_llm_* C-ABI is declared, bound with the declared signature
and validates its arguments before any device call."""
import ctypes as C
import os
import re

import pytest
import torch

import certifiedgpt_amd as cg
from certifiedgpt_amd import _lib
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import MiniGPT4Classifier, hip_decode_unsupported, prepare_texts
from toy_llm import StubEncoder, ToyTokenizer, VOCAB, tiny_llama

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPT = prepare_texts(["<Img><ImageHere></Img> what is this"])[0]
LLM_ENTRIES = ["cgpt_llm_create", "cgpt_llm_destroy", "cgpt_llm_load_weight_f16", "cgpt_llm_step", "cgpt_llm_greedy"]


def _tiny(**overrides):
    from transformers import LlamaConfig, LlamaForCausalLM
    kw = dict(vocab_size=VOCAB, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
              num_key_value_heads=4, max_position_embeddings=512, pad_token_id=0, bos_token_id=1, eos_token_id=2)
    kw.update(overrides)
    torch.manual_seed(0)
    return LlamaForCausalLM(LlamaConfig(**kw)).eval()


def _classifier(llm, decode):
    return MiniGPT4Classifier(StubEncoder(), llm, ToyTokenizer(), PROMPT, AnswerLabelMap(4, ()), max_new_tokens=3, decode=decode)


def _has(problems, word):
    return any(p.startswith(word) for p in problems)


# ------------------------------------------------------------------------------------------ the model check
def test_plain_tiny_model_names_device_dtype_and_head_size():
    problems = hip_decode_unsupported(tiny_llama())
    assert _has(problems, "device:") and _has(problems, "dtype:") and _has(problems, "head size:")
    assert not _has(problems, "K/V heads:") and not _has(problems, "biases:") and not _has(problems, "rotary law:")
    with pytest.raises(ValueError) as e:
        _classifier(tiny_llama(), "hip")
    msg = str(e.value)
    for p in problems:                                                  # the message lists every one of them
        assert p in msg
    assert "device" in msg and "dtype" in msg and "head size" in msg


@pytest.mark.parametrize("overrides, word", [
    (dict(num_key_value_heads=2), "K/V heads:"),
    (dict(attention_bias=True), "biases:"),
    (dict(rope_scaling={"rope_type": "linear", "factor": 2.0}), "rotary law:"),
])
def test_each_further_rule_is_named_beside_the_others(overrides, word):
    llm = _tiny(**overrides)
    problems = hip_decode_unsupported(llm)
    assert _has(problems, word), problems
    assert _has(problems, "device:") and _has(problems, "dtype:") and _has(problems, "head size:")     # collected, not first-only
    with pytest.raises(ValueError) as e:
        _classifier(llm, "hip")
    assert word.rstrip(":") in str(e.value) and "head size" in str(e.value)


def test_other_rules_of_the_check():
    assert _has(hip_decode_unsupported(_tiny(mlp_bias=True)), "biases:")
    assert _has(hip_decode_unsupported(_tiny(hidden_act="gelu")), "activation:")
    assert _has(hip_decode_unsupported(_tiny(vocab_size=VOCAB + 1)), "shape:")
    assert _has(hip_decode_unsupported(tiny_llama(), max_batch=300), "batch:")
    assert hip_decode_unsupported(torch.nn.Linear(4, 4))[0].startswith("architecture:")
    many = tiny_llama()
    many.generation_config.eos_token_id = list(range(2, 11))           # 9 ids: known at construction, so refused there
    assert _has(hip_decode_unsupported(many), "EOS ids:")
    many.generation_config.eos_token_id = list(range(2, 10))
    assert not _has(hip_decode_unsupported(many), "EOS ids:")


def test_hip_never_turns_into_another_engine_and_other_engines_carry_no_handle():
    with pytest.raises(ValueError):
        _classifier(tiny_llama(), "hip")                               # no classifier object comes back at all
    with pytest.raises(AssertionError):
        _classifier(tiny_llama(), "native")
    for decode in ("hf", "graph"):
        clf = _classifier(tiny_llama(), decode)
        assert clf.decode == decode and clf._hip is None
        assert clf.decode_stats["hip_steps"] == 0
        clf.generate_from_embeds(torch.zeros(2, 4, 64), PROMPT)        # CPU tensors: both take the HF call
        assert clf.decode_stats["hip_steps"] == 0 and clf.decode_stats["hf_calls"] == 1


def test_agent_documents_and_forwards_the_engine():
    import inspect
    from certifiedgpt_amd.agents import minigpt4_certify_agent as agent
    src = inspect.getsource(agent)
    assert '"hip"' in src and 'gen_cfg.get("decode", "hf")' in src     # documented; the default stays "hf"


# ------------------------------------------------------------------------------------------ the C-ABI
def _header():
    text = open(os.path.join(ROOT, "include", "cgpt.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


_CTYPES = {"cgpt_llm_handle": C.c_void_p, "const cgpt_llm_config*": C.POINTER(_lib.LlmConfig), "cgpt_llm_handle*": C.POINTER(C.c_void_p),
           "const char*": C.c_char_p, "const void*": C.c_void_p, "void*": C.c_void_p, "void* const*": C.c_void_p,
           "const int64_t*": C.c_void_p, "int64_t*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p,
           "int32_t": C.c_int32, "int64_t": C.c_int64}


def test_header_declares_and_binding_matches_every_llm_entry():
    _, code = _header()
    L = cg.lib()
    for name in LLM_ENTRIES:
        m = re.search(r"cgpt_status\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, f"cgpt.h does not declare {name}"
        assert hasattr(L, name), f"libcgpt.so does not export {name}"
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        types = [re.sub(r"\s*\b[A-Za-z_0-9]+$", "", p).replace(" *", "*") for p in params]      # drop the parameter name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int32
        assert [_CTYPES[t] for t in types] == list(args), (name, types)


def test_llm_config_struct_matches_header():
    text, _ = _header()
    body = re.search(r"typedef struct cgpt_llm_config \{(.*?)\} cgpt_llm_config;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int32_t|float)\s+([a-z_0-9]+)\s*;", body)
    assert [f[1] for f in fields] == [f[0] for f in _lib.LlmConfig._fields_]
    assert [{"int32_t": C.c_int32, "float": C.c_float}[f[0]] for f in fields] == [f[1] for f in _lib.LlmConfig._fields_]


def _config(**overrides):
    kw = dict(struct_size=C.sizeof(_lib.LlmConfig), device=0, hidden=512, layers=2, heads=4, kv_heads=4, head_dim=128, mlp=1408,
              vocab=320, rms_eps=1e-6, rope_theta=10000.0, max_batch=200, max_len=128)
    kw.update(overrides)
    return _lib.LlmConfig(**kw)


@pytest.mark.parametrize("overrides", [dict(kv_heads=2), dict(head_dim=64), dict(hidden=520, heads=4), dict(max_batch=257),
                                       dict(max_batch=0), dict(struct_size=8), dict(mlp=1400), dict(vocab=321), dict(layers=0),
                                       dict(hidden=640, heads=4), dict(max_len=0), dict(rms_eps=0.0)])
def test_create_rejects_bad_fields_before_any_device_call(overrides):
    L = cg.lib()
    h = C.c_void_p()
    assert L.cgpt_llm_create(C.byref(_config(**overrides)), C.byref(h)) == 1, overrides           # CGPT_ERR_INVALID
    assert not h.value and L.cgpt_last_error()


def test_create_without_gpu_is_no_device_and_null_handles_are_errors():
    L = cg.lib()
    h = C.c_void_p()
    assert L.cgpt_llm_create(None, C.byref(h)) == 1
    if not torch.cuda.is_available():
        assert L.cgpt_llm_create(C.byref(_config()), C.byref(h)) == 2                             # CGPT_ERR_NO_DEVICE
        assert b"no HIP device" in L.cgpt_last_error()
    assert L.cgpt_llm_step(None, None, 1, 0, None, None, 8, None, None) != 0                      # an error, not a crash
    assert L.cgpt_llm_greedy(None, None, 1, 4, 2, 1, None, 0, 0, None, None, 8, None, None, None) != 0
    assert L.cgpt_llm_load_weight_f16(None, b"lm_head.weight", None, 0, None) != 0
    assert L.cgpt_llm_destroy(None) == 0
