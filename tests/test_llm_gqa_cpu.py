"""grouped_kv without a GPU: what `hip_decode_unsupported` says with and without the flag, cgpt_llm_create's validation of
cgpt_llm_config_gqa.grouped_kv (it runs before any device call, so an accepted config ends in CGPT_ERR_NO_DEVICE here), the three valid
struct sizes, the classifier's keyword validation, the agent's key, and `expand_kv_state_dict` -- the oracle of
tests/test_gpu_llm_gqa.py -- against HF's own grouped-query attention in fp32."""
import ctypes as C
import inspect
import types

import pytest
import torch

import certifiedgpt_amd as cg
from certifiedgpt_amd import _lib
from certifiedgpt_amd.agents import minigpt4_certify_agent as agent
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import MiniGPT4Classifier, WordHashTokenizer, expand_kv_state_dict, hip_decode_unsupported

INVALID, NO_DEVICE = 1, 2


def _hf(heads, kv, hidden=None, dtype=torch.float32, layers=2, vocab=320, mlp=1408, seed=0):
    from transformers import LlamaConfig, LlamaForCausalLM
    lcfg = LlamaConfig(vocab_size=vocab, hidden_size=hidden or heads * 128, intermediate_size=mlp, num_hidden_layers=layers,
                       num_attention_heads=heads, num_key_value_heads=kv, max_position_embeddings=256, pad_token_id=0, bos_token_id=1,
                       eos_token_id=2)
    torch.manual_seed(seed)
    return LlamaForCausalLM(lcfg).to(dtype).eval()


# ------------------------------------------------------------------------------------------ hip_decode_unsupported
def _kv_sentences(bad):
    return [b for b in bad if b.startswith("K/V heads:")]


def test_default_list_is_unchanged_and_the_flag_accepts_grouped_decoders():
    assert inspect.signature(hip_decode_unsupported).parameters["grouped_kv"].default is False
    gqa = _hf(4, 2, dtype=torch.float16)
    plain = hip_decode_unsupported(gqa)
    assert _kv_sentences(plain) == ["K/V heads: num_key_value_heads 2 != num_attention_heads 4 (grouped-query attention is not supported)"]
    assert hip_decode_unsupported(gqa, None, False) == plain
    with_flag = hip_decode_unsupported(gqa, grouped_kv=True)
    assert _kv_sentences(with_flag) == [] and with_flag == [b for b in plain if not b.startswith("K/V heads:")]
    mha = _hf(4, 4, dtype=torch.float16)
    assert hip_decode_unsupported(mha, grouped_kv=True) == hip_decode_unsupported(mha)          # G = 1 under the flag
    assert _kv_sentences(hip_decode_unsupported(_hf(8, 1, dtype=torch.float16, layers=1), grouped_kv=True)) == []


def test_bad_ratios_are_named_under_the_flag():
    llm = _hf(16, 1, hidden=2048, dtype=torch.float16, layers=1, mlp=128, vocab=64)              # ratio 16
    (msg,) = _kv_sentences(hip_decode_unsupported(llm, grouped_kv=True))
    assert "num_key_value_heads 1" in msg and "num_attention_heads 16" in msg and "[1, 2, 4, 8]" in msg
    llm.config.num_key_value_heads = 3                                                          # a count that does not divide (HF refuses to build it)
    (msg,) = _kv_sentences(hip_decode_unsupported(llm, grouped_kv=True))
    assert "num_key_value_heads 3" in msg


# ------------------------------------------------------------------------------------------ cgpt_llm_create
GQA_SIZE = C.sizeof(_lib.LlmConfigGqa)


def _config(grouped_kv=0, reserved=0, **over):
    """A cgpt_llm_config_gqa; struct_size defaults to the extended size, so the switches behind `base` are read."""
    kw = dict(struct_size=GQA_SIZE, device=0, hidden=512, layers=2, heads=4, kv_heads=4, head_dim=128, mlp=1408, vocab=320,
              rms_eps=1e-6, rope_theta=10000.0, max_batch=8, max_len=128, weight_format=0)
    kw.update(over)
    return _lib.LlmConfigGqa(base=_lib.LlmConfig(**kw), grouped_kv=grouped_kv, reserved=reserved)


def _create(cfg):
    L = cg.lib()
    h = C.c_void_p()
    rc = L.cgpt_llm_create(C.byref(cfg.base), C.byref(h))
    msg = L.cgpt_last_error()
    if rc == 0:
        L.cgpt_llm_destroy(h)
    return rc, msg


ACCEPTED = (0, NO_DEVICE)                                          # validation passed: OK with a GPU, NO_DEVICE without


def test_extended_struct_mirrors_the_header_and_the_plain_struct_is_unchanged():
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "cgpt.h")).read()
    body = re.search(r"typedef struct cgpt_llm_config_gqa \{(.*?)\} cgpt_llm_config_gqa;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(cgpt_llm_config|int32_t)\s+([a-z_0-9]+)\s*;", body) == [("cgpt_llm_config", "base"), ("int32_t", "grouped_kv"),
                                                                                ("int32_t", "reserved")]
    assert _lib.LlmConfigGqa._fields_ == [("base", _lib.LlmConfig), ("grouped_kv", C.c_int32), ("reserved", C.c_int32)]
    assert _lib.LlmConfigGqa.grouped_kv.offset == C.sizeof(_lib.LlmConfig) and GQA_SIZE == C.sizeof(_lib.LlmConfig) + 8
    assert _lib.LlmConfig._fields_[-1][0] == "weight_format"           # the plain struct did not grow


def test_grouped_config_passes_validation():
    rc, msg = _create(_config(grouped_kv=1, kv_heads=2))
    assert rc in ACCEPTED, (rc, msg)
    if not torch.cuda.is_available():
        assert rc == NO_DEVICE, (rc, msg)
    for heads, kv in ((4, 4), (4, 1), (8, 1), (32, 8), (64, 8)):
        rc, msg = _create(_config(grouped_kv=1, heads=heads, hidden=heads * 128, kv_heads=kv, layers=1, mlp=128, vocab=64, max_batch=1))
        assert rc in ACCEPTED, (heads, kv, rc, msg)


@pytest.mark.parametrize("over", [dict(grouped_kv=1, kv_heads=3), dict(grouped_kv=2, kv_heads=2), dict(grouped_kv=-1),
                                  dict(grouped_kv=1, heads=16, hidden=2048, kv_heads=1), dict(grouped_kv=1, kv_heads=0),
                                  dict(grouped_kv=1, kv_heads=8), dict(grouped_kv=0, kv_heads=2), dict(grouped_kv=1, kv_heads=2, reserved=1)])
def test_bad_grouped_configs_are_invalid_before_any_device_call(over):
    rc, msg = _create(_config(**over))
    assert rc == INVALID and (b"grouped_kv" in msg or b"kv_heads" in msg or b"reserved" in msg), (over, rc, msg)


def test_all_three_struct_sizes_are_accepted_and_the_plain_sizes_do_not_read_the_switches():
    plain = (C.sizeof(_lib.LlmConfig), _lib.LLM_CONFIG_SIZE_F16)
    for size in (GQA_SIZE,) + plain:
        rc, msg = _create(_config(struct_size=size))
        assert rc in ACCEPTED, (size, rc, msg)
    # a plain size: what lies behind the struct is NOT read (garbage there must not matter), and kv_heads != heads is refused
    for size in plain:
        rc, msg = _create(_config(struct_size=size, grouped_kv=77, reserved=5))
        assert rc in ACCEPTED, (size, rc, msg)
        rc, msg = _create(_config(struct_size=size, grouped_kv=1, kv_heads=2))
        assert rc == INVALID and b"kv_heads" in msg, (size, rc, msg)
    for size in (0, _lib.LLM_CONFIG_SIZE_F16 - 4, C.sizeof(_lib.LlmConfig) + 4, GQA_SIZE + 4):
        rc, msg = _create(_config(struct_size=size))
        assert rc == INVALID and b"struct_size" in msg, (size, rc, msg)


def test_a_group_size_and_length_that_exceed_the_lds_are_refused_with_a_message():
    """G = 8 keeps 8 score arrays of max_len floats in LDS: 8192 positions need 283 KB, a CU has 160 KiB."""
    big = dict(grouped_kv=1, heads=8, hidden=1024, kv_heads=1)
    rc, msg = _create(_config(max_len=8192, **big))
    assert rc == INVALID and b"LDS" in msg and b"max_len" in msg, (rc, msg)
    rc, msg = _create(_config(max_len=4096, **big))                                              # what the Python engine asks for
    assert rc in ACCEPTED, (rc, msg)
    rc, msg = _create(_config(max_len=8192, grouped_kv=1, kv_heads=1))                           # G = 4 fits at the longest max_len
    assert rc in ACCEPTED, (rc, msg)


# ------------------------------------------------------------------------------------------ the classifier and the agent
def _clf(**kw):
    return MiniGPT4Classifier(None, object(), WordHashTokenizer(96), "<ImageHere>", AnswerLabelMap(4, ()), max_batch=4, **kw)


@pytest.mark.parametrize("kw", [dict(decode="hf"), dict(decode="graph"), dict()])
def test_grouped_kv_needs_the_native_engine(kw):
    with pytest.raises(ValueError) as e:
        _clf(grouped_kv=True, **kw)
    assert "grouped_kv" in str(e.value) and "decode" in str(e.value), str(e.value)


def test_grouped_kv_is_a_bool_and_off_by_default():
    for bad in (1, "on", None):
        with pytest.raises(ValueError) as e:
            _clf(grouped_kv=bad, decode="hip")
        assert "grouped_kv" in str(e.value)
    clf = _clf()
    assert clf.grouped_kv is False and inspect.signature(MiniGPT4Classifier.__init__).parameters["grouped_kv"].default is False
    embs = types.SimpleNamespace(shape=(4, 12, 512), dtype=torch.float16, device=types.SimpleNamespace(index=0))
    plain = clf._graph_key(embs)
    assert plain == (4, 12, torch.float16, 0, 20, False, "hf", "model")                          # the key as it was before the keyword
    clf.grouped_kv = True
    assert clf._graph_key(embs) == plain + ("grouped_kv",)


def test_a_grouped_decoder_without_the_flag_is_still_a_value_error():
    gqa = _hf(4, 2, dtype=torch.float16)
    with pytest.raises(ValueError) as e:
        MiniGPT4Classifier(None, gqa, WordHashTokenizer(320), "<ImageHere>", AnswerLabelMap(4, ()), max_batch=4, decode="hip")
    assert "grouped-query attention is not supported" in str(e.value)


def test_agents_pass_the_key_through(monkeypatch):
    src = inspect.getsource(agent)
    assert "grouped_kv: false | true" in agent.__doc__ and 'gen_cfg.get("grouped_kv", False)' in src
    seen = {}

    class Spy:
        def __init__(self, *a, **kw):
            seen.update(kw)

    import certifiedgpt_amd.minigpt4 as m
    monkeypatch.setattr(m, "MiniGPT4Classifier", Spy)
    enc = types.SimpleNamespace(max_batch=4, device="cpu")
    llm = types.SimpleNamespace(parameters=lambda: [])
    base = {"prompt": "<ImageHere>", "answers": ["a", "b"], "decode": "hip"}
    agent.build_generating_classifier(enc, dict(base, grouped_kv=True), 4, tokenizer=object(), llama_model=llm)
    assert seen["grouped_kv"] is True and seen["decode"] == "hip"
    agent.build_generating_classifier(enc, base, 4, tokenizer=object(), llama_model=llm)
    assert seen["grouped_kv"] is False
    from certifiedgpt_amd.agents.minigpt4_predict_agent import MiniGPT4PredictAgent
    assert issubclass(MiniGPT4PredictAgent, agent.MiniGPT4CertifyAgent)


# ------------------------------------------------------------------------------------------ expand_kv_state_dict
@pytest.mark.parametrize("heads, kv", [(4, 2), (4, 1), (8, 1), (4, 4)])
def test_the_expanded_twin_computes_what_the_grouped_model_computes(heads, kv):
    """fp32 on the CPU: HF's grouped-query forward (repeat_kv of kv heads) against HF's multi-head forward on the expanded weights.
    The two differ by fp32 rounding of differently blocked matmuls only -- 1e-5 absolute at logits of order 1; a wrong head
    mapping moves the logits by their own size."""
    from transformers import LlamaForCausalLM
    gqa = _hf(heads, kv)
    sd = expand_kv_state_dict(gqa)
    G = heads // kv
    k0, kx = gqa.state_dict()["model.layers.1.self_attn.k_proj.weight"], sd["model.layers.1.self_attn.k_proj.weight"]
    assert kx.shape == (heads * 128, heads * 128) and k0.shape == (kv * 128, heads * 128)
    for h in range(heads):                                             # twin head h is K/V head h // G: repeat_interleave order
        assert torch.equal(kx[h * 128:(h + 1) * 128], k0[(h // G) * 128:(h // G + 1) * 128])
    assert torch.equal(sd["model.layers.0.self_attn.q_proj.weight"], gqa.state_dict()["model.layers.0.self_attn.q_proj.weight"])
    import copy
    tcfg = copy.deepcopy(gqa.config)
    tcfg.num_key_value_heads = heads
    twin = LlamaForCausalLM(tcfg).eval()
    missing, unexpected = twin.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    ids = torch.randint(3, 320, (3, 17), generator=torch.Generator().manual_seed(heads * 10 + kv))
    with torch.no_grad():
        a, b = gqa(input_ids=ids).logits, twin(input_ids=ids).logits
    scale = float(a.abs().max())
    assert 0.1 < scale < 10.0, scale                                   # logits of order 1: the bound below means something
    assert float((a - b).abs().max()) <= 1e-5, float((a - b).abs().max())
    if G > 1 and kv > 1:                                               # the comparison is not vacuous: the tiled order is a different model
        wrong = dict(sd)
        for name in sd:
            if name.endswith("k_proj.weight") or name.endswith("v_proj.weight"):
                w = gqa.state_dict()[name]
                wrong[name] = w.view(kv, 128, -1).repeat(G, 1, 1).reshape(heads * 128, -1)
        twin.load_state_dict(wrong, strict=True)
        with torch.no_grad():
            c = twin(input_ids=ids).logits
        assert float((a - c).abs().max()) > 1e-3


def test_expand_refuses_a_count_that_does_not_divide():
    llm = _hf(4, 2, layers=1)
    llm.config.num_key_value_heads = 3
    with pytest.raises(ValueError):
        expand_kv_state_dict(llm)
