"""weights="int8" without a GPU: the weight law in plain torch (`quantize_rows_int8` / `dequantize_rows_int8`, the restatement of
csrc/llm_step.hip's llm_quant_rows_kernel), the classifier's keyword validation (it runs before any device work) and the config struct's
two valid sizes (cgpt_llm_create validates the config before it looks for a device).

The law, per output row n of an fp16 nn.Linear.weight [N, K]:  s_n = fp16(absmax / 127) with the division in fp32;
q_nk = clamp(rint(w_nk / s_n), -127, 127) in fp32, round to nearest even, q = 0 where s_n = 0;  W'_nk = fp16(q_nk) * s_n, one fp16
multiply."""
import ctypes as C
import math

import pytest
import torch

import certifiedgpt_amd as cg
from certifiedgpt_amd import _lib
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import (MiniGPT4Classifier, WordHashTokenizer, dequantize_rows_int8, int8_state_dict, quantize_rows_int8)


def _matrices():
    g = torch.Generator().manual_seed(0)
    rnd = (torch.randn(48, 256, generator=g) * 0.02).to(torch.float16)
    wide = (torch.randn(16, 512, generator=g) * 3.0).to(torch.float16)
    special = (torch.randn(6, 128, generator=g) * 0.02).to(torch.float16)
    special[0] = 0                                                     # a zero row
    special[1, 17] = 60000.0                                           # a single huge element: everything else quantises to 0
    special[2] = 0
    special[2, 5] = 2.0 ** -24                                         # the smallest subnormal: absmax / 127 underflows fp16 to 0
    special[2, 9] = -(2.0 ** -24)
    special[3] = (torch.randn(128, generator=g) * 2.0 ** -17).to(torch.float16)   # a row whose scale is an fp16 subnormal, not 0
    special[4] = 60000.0                                               # every element equal and huge (within 2^-11 of fp16's maximum
                                                                       # a scale rounded up makes 127 s overflow: DESIGN.md 4.4.3)
    return {"random": rnd, "wide": wide, "special": special}


def _ulp16(x):
    """Spacing of fp16 at |x| (subnormal spacing below the smallest normal)."""
    x = x.abs().double().clamp_min(2.0 ** -14)
    return torch.pow(2.0, torch.floor(torch.log2(x)) - 10)


@pytest.mark.parametrize("name", ["random", "wide", "special"])
def test_the_law_gives_int8_in_range_fp16_scales_and_the_stated_arithmetic(name):
    w = _matrices()[name]
    q, s = quantize_rows_int8(w)
    assert q.dtype == torch.int8 and s.dtype == torch.float16 and q.shape == w.shape and tuple(s.shape) == (w.shape[0],)
    assert int(q.min()) >= -127 and int(q.max()) <= 127
    # the law element by element in Python floats (fp32 steps made explicit with torch scalars)
    for n in range(w.shape[0]):
        amax = max(abs(float(v)) for v in w[n])
        want_s = (torch.tensor(amax, dtype=torch.float32) / torch.tensor(127.0, dtype=torch.float32)).to(torch.float16)
        assert float(s[n]) == float(want_s), (n, float(s[n]), float(want_s))
        if float(want_s) == 0.0:
            assert int(q[n].abs().max()) == 0
            continue
        for k in range(0, w.shape[1], 7):
            t = float(w[n, k].float() / want_s.float())
            r = math.floor(t)
            d = t - r
            r = r + 1 if d > 0.5 or (d == 0.5 and r % 2) else r        # round half to even
            assert int(q[n, k]) == max(-127, min(127, r)), (n, k, t)
        assert int(q[n].abs().max()) == 127 or float(s[n]) < 2.0 ** -14   # the absmax element sits at +-127 (normal scales)


def test_special_rows():
    w = _matrices()["special"]
    q, s = quantize_rows_int8(w)
    wd = dequantize_rows_int8(q, s)
    assert float(s[0]) == 0.0 and int(q[0].abs().max()) == 0 and bool((wd[0] == 0).all())          # zero row
    assert int(q[1, 17]) == 127 and int(q[1].abs().sum()) == 127                                    # one huge element
    assert abs(float(wd[1, 17]) - 60000.0) <= 0.5 * float(s[1]) + 16.0
    assert float(s[2]) == 0.0 and int(q[2].abs().max()) == 0 and bool((wd[2] == 0).all())          # absmax / 127 underflows: zeros
    assert 0.0 < float(s[3]) < 2.0 ** -14 and int(q[3].abs().max()) > 0                             # a subnormal scale still works
    assert bool(torch.isfinite(wd).all())
    assert bool((q[4] == 127).all()) and bool(torch.isfinite(wd[4]).all())


@pytest.mark.parametrize("name", ["random", "wide", "special"])
def test_dequantised_weights_are_reproducible_close_and_a_fixed_point(name):
    w = _matrices()[name]
    q, s = quantize_rows_int8(w)
    wd = dequantize_rows_int8(q, s)
    assert wd.dtype == torch.float16 and wd.shape == w.shape
    q2, s2 = quantize_rows_int8(w.clone())
    assert torch.equal(q, q2) and torch.equal(s, s2) and torch.equal(wd, dequantize_rows_int8(q2, s2))       # reproducible
    # one fp16 multiply: the exact product of two fp16 values, rounded once
    exact = q.double() * s.double()[:, None]
    assert torch.equal(wd, exact.to(torch.float16))
    # |W - W'| <= s / 2 + half an fp16 ulp of |W'| per element; an element clamped at +-127 (only where the scale is a subnormal
    # or was rounded down) is bounded by its own row's absmax instead
    clamped = (w.float() / torch.where(s == 0, torch.ones_like(s), s).float()[:, None]).abs() > 127.5
    err = (w.double() - wd.double()).abs()
    bound = s.double()[:, None] / 2 + _ulp16(wd) / 2
    live = (s != 0)[:, None] & ~clamped
    assert bool((err[live.expand_as(err)] <= bound[live.expand_as(err)]).all()), float((err - bound)[live.expand_as(err)].max())
    assert not bool(clamped[(s.float() >= 2.0 ** -14)].any())          # with a normal scale nothing is clamped beyond rounding
    # re-quantising W' returns the same q
    q3, _ = quantize_rows_int8(wd)
    normal = s.float() >= 2.0 ** -14
    assert torch.equal(q3[normal], q[normal])


def test_bad_inputs_are_value_errors():
    with pytest.raises(ValueError):
        quantize_rows_int8(torch.zeros(4, 8))                          # fp32
    with pytest.raises(ValueError):
        quantize_rows_int8(torch.zeros(8, dtype=torch.float16))        # not a matrix
    with pytest.raises(ValueError):
        dequantize_rows_int8(torch.zeros(4, 8, dtype=torch.int8), torch.zeros(3, dtype=torch.float16))


def test_int8_state_dict_replaces_the_layer_linears_only():
    from transformers import LlamaConfig, LlamaForCausalLM
    lcfg = LlamaConfig(vocab_size=64, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=1,
                       num_key_value_heads=1, max_position_embeddings=64)
    torch.manual_seed(0)
    llm = LlamaForCausalLM(lcfg).half().eval()
    sd, before = int8_state_dict(llm), llm.state_dict()
    assert sorted(sd) == sorted(before)
    changed = 0
    for name, w in before.items():
        linear = name.startswith("model.layers.") and "_proj." in name
        if linear:
            assert torch.equal(sd[name], dequantize_rows_int8(*quantize_rows_int8(w))), name
            changed += int(not torch.equal(sd[name], w))
        else:
            assert torch.equal(sd[name], w), name                      # embed_tokens, lm_head, RMSNorm weights: untouched
    assert changed == 14
    twin = LlamaForCausalLM(lcfg).half()
    missing, unexpected = twin.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    # rows keep their scales wherever they end up: quantising a row subset is the subset of the quantised rows
    w = before["model.layers.0.mlp.gate_proj.weight"]
    q, s = quantize_rows_int8(w)
    q16, s16 = quantize_rows_int8(w[16:32].contiguous())
    assert torch.equal(q[16:32], q16) and torch.equal(s[16:32], s16)


# ------------------------------------------------------------------------------------------ keyword validation (before any device work)
@pytest.mark.parametrize("kw, words", [
    (dict(weights="int8", decode="graph"), ("weights", "decode", "prefill")),
    (dict(weights="int8", decode="hip", prefill="model"), ("weights", "decode", "prefill")),
    (dict(weights="int8"), ("weights", "decode", "prefill")),
    (dict(weights="int4", decode="hip", prefill="hip"), ("weights", "int4")),
    (dict(weights=None), ("weights",)),
])
def test_weights_keyword_is_validated_at_construction(kw, words):
    with pytest.raises(ValueError) as e:
        MiniGPT4Classifier(None, object(), WordHashTokenizer(96), "<ImageHere>", AnswerLabelMap(4, ()), max_batch=4, **kw)
    for word in words:
        assert word in str(e.value), (word, str(e.value))


def test_default_weights_keyword_is_fp16_and_reported():
    clf = MiniGPT4Classifier(None, object(), WordHashTokenizer(96), "<ImageHere>", AnswerLabelMap(4, ()), max_batch=4)
    assert clf.weights == "fp16" and clf.decode_stats["weight_bytes"] is None       # no native engine, nothing held


# ------------------------------------------------------------------------------------------ the config struct's two sizes
def _config(**over):
    kw = dict(struct_size=C.sizeof(_lib.LlmConfig), device=0, hidden=128, layers=1, heads=1, kv_heads=1, head_dim=128, mlp=128, vocab=64,
              rms_eps=1e-5, rope_theta=10000.0, max_batch=4, max_len=16, weight_format=0)
    kw.update(over)
    return _lib.LlmConfig(**kw)


def _create(cfg):
    L = cg.lib()
    h = C.c_void_p()
    rc = L.cgpt_llm_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        n = C.c_int64(-1)
        assert L.cgpt_llm_weight_bytes(h, C.byref(n)) == 0 and n.value > 0
        L.cgpt_llm_destroy(h)
    return rc, L.cgpt_last_error()


def test_config_struct_matches_header_and_both_sizes_are_accepted():
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "cgpt.h")).read()
    body = re.search(r"typedef struct cgpt_llm_config \{(.*?)\} cgpt_llm_config;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(?:int32_t|float)\s+([a-z_0-9]+)\s*;", body) == [f[0] for f in _lib.LlmConfig._fields_]
    assert _lib.LlmConfig._fields_[-1][0] == "weight_format" and _lib.LLM_CONFIG_SIZE_F16 == C.sizeof(_lib.LlmConfig) - 4
    assert re.search(r"#define\s+CGPT_LLM_W_F16\s+0\b", text) and re.search(r"#define\s+CGPT_LLM_W_INT8\s+1\b", text)
    assert _lib.LLM_WEIGHT_FORMATS == {"fp16": 0, "int8": 1}
    # the config is validated before the device is looked for: an accepted config ends in OK (GPU) or NO_DEVICE (none), never INVALID
    accepted = (0, 2)
    for fmt in (0, 1):
        rc, msg = _create(_config(weight_format=fmt))
        assert rc in accepted, (fmt, rc, msg)
    # the size before weight_format existed: accepted, and the field is NOT read (garbage there must not matter)
    rc, msg = _create(_config(struct_size=_lib.LLM_CONFIG_SIZE_F16, weight_format=77))
    assert rc in accepted, (rc, msg)
    # an unknown format is refused when the size covers the field; any other size is refused as before
    for bad in (2, -1, 77):
        rc, msg = _create(_config(weight_format=bad))
        assert rc == 1 and b"weight_format" in msg, (bad, rc, msg)
    for size in (0, _lib.LLM_CONFIG_SIZE_F16 - 4, C.sizeof(_lib.LlmConfig) + 4):
        rc, msg = _create(_config(struct_size=size))
        assert rc == 1 and b"struct_size" in msg, (size, rc, msg)
    L = cg.lib()
    assert L.cgpt_llm_weight_bytes(None, None) == 1
