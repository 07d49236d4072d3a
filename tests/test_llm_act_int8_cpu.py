"""activations="int8" without a GPU: the law (`quantize_act_rows_int8`, `llm_int8_linear`) against a scalar restatement written out in
Python loops, its properties (row independence, threshold 0, the outlier split's gain, the quantisation error bound), the oracle
`act_int8_twin` on the toy decoder, the classifier's keyword validation, `hip_decode_unsupported(activations=...)`, and the C-ABI
(cgpt_llm_config_act; create's validation runs before any device call, so an accepted config ends in CGPT_ERR_NO_DEVICE here)."""
import copy
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import certifiedgpt_amd as cg
from certifiedgpt_amd import _lib
from certifiedgpt_amd.agents import minigpt4_certify_agent as agent
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import (MiniGPT4Classifier, WordHashTokenizer, act_int8_twin, dequantize_rows_int8, hip_decode_unsupported,
                                       int8_state_dict, llm_int8_linear, quantize_act_rows_int8, quantize_rows_int8)
from toy_llm import tiny_llama

INVALID, NO_DEVICE = 1, 2
ACCEPTED = (0, NO_DEVICE)
T = 6.0


# ------------------------------------------------------------------------------------------ the law
def _planted_input():
    """5 x 256: an outlier column, a lone outlier, +-threshold exactly, an all-outlier row, an all-zero row."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, 256, generator=g)
    x[:, 9] = torch.tensor([25.0, -31.0, 40.0, 12.0, 0.0])             # an outlier column
    x[0, 200] = -7.25                                                  # a lone outlier
    x[1, 3], x[1, 4] = T, -T                                           # exactly +-threshold: both outliers
    x[2, 77] = 5.996                                                   # fp16 rounds it to 5.9961 < 6: not an outlier, and the row's absmax
    x[3] = 6.0 + (torch.arange(256) % 7).float()                       # every element an outlier: s_a = 0
    x[3, ::2] *= -1
    x[4] = 0.0                                                         # an all-zero row
    return x.half()


def _weights(N=64, K=256, seed=1):
    g = torch.Generator().manual_seed(seed)
    return quantize_rows_int8((torch.randn(N, K, generator=g) * 0.05).half())


def _scalar_law(x, q, s_w, t):
    """Steps 1-7 one element at a time, in numpy float32 scalars (every operation rounds to fp32, nothing is fused)."""
    f32 = np.float32
    M, K = x.shape
    N = q.shape[0]
    xs, qs, sw = x.float().numpy(), q.numpy().astype(np.int64), s_w.float().numpy()
    swh, qh = s_w.numpy(), q.numpy().astype(np.float16)
    v = np.zeros((M, N), dtype=np.float32)
    for m in range(M):
        outlier = [t > 0 and abs(xs[m, k]) >= f32(t) for k in range(K)]
        amax = f32(0)
        for k in range(K):
            if not outlier[k]:
                amax = max(amax, abs(xs[m, k]))
        s_a = f32(amax) / f32(127)
        a = [0] * K
        if s_a != 0:
            for k in range(K):
                if not outlier[k]:
                    a[k] = int(min(max(np.rint(f32(xs[m, k]) / s_a), -127), 127))
        for n in range(N):
            acc = sum(a[k] * int(qs[n, k]) for k in range(K))
            y = f32(acc) * (s_a * f32(sw[n]))
            o = f32(0)
            for k in range(K):
                if outlier[k]:
                    wp = np.float16(qh[n, k] * swh[n])                 # one fp16 multiply
                    o = f32(o + f32(xs[m, k]) * f32(wp))
            v[m, n] = f32(y + o)
    return torch.from_numpy(v)


@pytest.mark.parametrize("t", [T, 0.0])
def test_the_law_equals_its_scalar_restatement(t):
    x, (q, s_w) = _planted_input(), _weights()
    a, s_a, out = quantize_act_rows_int8(x, t)
    if t > 0:
        assert out[:4, 9].all() and out[0, 200] and out[1, 3] and out[1, 4] and not out[2, 77] and out[3].all() and not out[4].any()
        assert float(s_a[3]) == 0.0 and not a[3].any() and float(s_a[4]) == 0.0 and not a[4].any()
        assert int(a[2].abs().max()) == 127 and int(a[2, 77]) == 127
    else:
        assert not out.any() and int(a[3].abs().max()) == 127
    v = llm_int8_linear(x, q, s_w, t)
    assert v.dtype == torch.float32 and torch.equal(v, _scalar_law(x, q, s_w, t))


def _outlier_column_input(M=37, K=1024, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    x[:, 17] *= 20.0
    x[5, 300], x[11, 900] = 9.0, -30.0
    return x.half()


def test_a_row_alone_equals_the_row_in_any_batch():
    x, (q, s_w) = _outlier_column_input(), _weights(192, 1024)
    v = llm_int8_linear(x, q, s_w)
    for rows in ([5], [11, 0], [36, 5, 20]):
        assert torch.equal(llm_int8_linear(x[rows], q, s_w), v[rows])
    assert torch.equal(llm_int8_linear(torch.cat([x[30:], x[:30]]), q, s_w), torch.cat([v[30:], v[:30]]))


def test_threshold_zero_equals_threshold_six_when_nothing_reaches_six():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(16, 256, generator=g).clamp_(-5.9, 5.9).half()
    q, s_w = _weights()
    assert not quantize_act_rows_int8(x, T)[2].any()
    assert torch.equal(llm_int8_linear(x, q, s_w, T), llm_int8_linear(x, q, s_w, 0.0))


def test_the_split_lowers_the_error_on_an_outlier_column_and_the_integer_product_is_exact():
    x, (q, s_w) = _outlier_column_input(), _weights(192, 1024)
    ref = x.double() @ dequantize_rows_int8(q, s_w).double().t()
    e6 = float((llm_int8_linear(x, q, s_w, T).double() - ref).abs().max())
    e0 = float((llm_int8_linear(x, q, s_w, 0.0).double() - ref).abs().max())
    assert e6 < e0, (e6, e0)
    a, _, _ = quantize_act_rows_int8(x, T)
    assert torch.equal((a.long() @ q.long().t()).double(), a.double() @ q.double().t())
    assert 127 * 127 * 65536 < 2 ** 31


@pytest.mark.parametrize("t", [T, 0.0])
def test_the_quantisation_error_bound(t):
    """Non-outlier inputs are rounded to a grid of spacing s_a, outliers enter exactly: |v - x W'^T| <= (s_a / 2) sum_k |W'_nk| plus
    fp32 slack -- 2^-22 of the sum of magnitudes covers the roundings of the two scale products, of y + o and of the outlier sum."""
    x, (q, s_w) = _outlier_column_input(), _weights(192, 1024)
    wp = dequantize_rows_int8(q, s_w).double()
    _, s_a, _ = quantize_act_rows_int8(x, t)
    v = llm_int8_linear(x, q, s_w, t).double()
    bound = 0.5 * s_a.double()[:, None] * wp.abs().sum(dim=1)[None, :] + 2.0 ** -22 * (x.double().abs() @ wp.abs().t())
    assert bool(((v - x.double() @ wp.t()).abs() <= bound).all())


def test_bad_arguments_are_refused():
    q, s_w = _weights()
    with pytest.raises(ValueError):
        quantize_act_rows_int8(torch.zeros(2, 8))
    with pytest.raises(ValueError):
        llm_int8_linear(torch.zeros(2, 128, dtype=torch.float16), q, s_w)


# ------------------------------------------------------------------------------------------ the twin
def test_the_twin_on_the_toy_decoder():
    llm = tiny_llama()
    before = {k: v.clone() for k, v in llm.state_dict().items()}
    twin = act_int8_twin(llm)
    sd = twin.state_dict()
    assert list(sd) == list(before) and all(torch.equal(sd[k], before[k]) for k in before)
    assert all(torch.equal(v, before[k]) for k, v in llm.state_dict().items())
    ids = torch.randint(3, 96, (3, 9), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        got = twin(ids).logits
        base = copy_with(llm, int8_state_dict(copy.deepcopy(llm).half()))(ids).logits     # the W' twin: the same weights, fp activations
        # one linear of the twin against the bound, on the activations the twin itself feeds it
        seen = {}
        lin = twin.model.layers[0].mlp.down_proj
        hook = lin.register_forward_hook(lambda m, i, o: seen.update(x=i[0], y=o))
        twin(ids)
        hook.remove()
    assert bool(torch.isfinite(got).all())
    x = seen["x"].reshape(-1, seen["x"].shape[-1]).half()
    wp = dequantize_rows_int8(lin.q, lin.s_w).double()
    _, s_a, _ = quantize_act_rows_int8(x, T)
    bound = 0.5 * s_a.double()[:, None] * wp.abs().sum(dim=1)[None, :] + 2.0 ** -22 * (x.double().abs() @ wp.abs().t())
    v = llm_int8_linear(x, lin.q, lin.s_w, T)
    assert bool(((v.double() - x.double() @ wp.t()).abs() <= bound).all())
    assert torch.equal(seen["y"].reshape(-1, v.shape[1]), v.half().float())         # the module returns fp16 of v in the model's dtype
    # the logits stay near the W' twin's: a code is off by at most half a level of 127, 2^-8 of a row's absmax; the 8 linears a logit
    # passes through add at most 8 x 2^-8 = 3 % of the scale even if every error lined up
    assert float((got - base).abs().max()) < 0.05 * float(base.abs().max())
    with pytest.raises(ValueError):
        act_int8_twin(types.SimpleNamespace(model=types.SimpleNamespace(layers=[_BiasLayer()])))


def copy_with(llm, state):
    twin = copy.deepcopy(llm).float()
    twin.load_state_dict({k: v.float() for k, v in state.items()}, strict=True)
    return twin.eval()


class _BiasLayer(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.self_attn = torch.nn.Module()
        self.mlp = torch.nn.Module()
        for name in ("q_proj", "k_proj", "v_proj", "o_proj"):
            setattr(self.self_attn, name, torch.nn.Linear(8, 8, bias=True))
        for name in ("gate_proj", "up_proj", "down_proj"):
            setattr(self.mlp, name, torch.nn.Linear(8, 8, bias=True))

    def __deepcopy__(self, memo):
        return self


# ------------------------------------------------------------------------------------------ the classifier, the engine check, the agent
def _clf(**kw):
    return MiniGPT4Classifier(None, object(), WordHashTokenizer(96), "<ImageHere>", AnswerLabelMap(4, ()), max_batch=4, **kw)


@pytest.mark.parametrize("kw, missing", [(dict(), ['decode="hip"', 'prefill="hip"', 'weights="int8"']),
                                          (dict(decode="hip"), ['prefill="hip"', 'weights="int8"']),
                                          (dict(decode="hip", prefill="hip"), ['weights="int8"']),
                                          (dict(decode="graph"), ['decode="hip"', 'prefill="hip"', 'weights="int8"'])])
def test_int8_activations_name_every_missing_keyword(kw, missing):
    with pytest.raises(ValueError) as e:
        _clf(activations="int8", **kw)
    head = str(e.value).split("(got")[0]
    assert 'activations="int8"' in head and all(m in head for m in missing), str(e.value)
    assert [m for m in ('decode="hip"', 'prefill="hip"', 'weights="int8"') if m in head] == missing


def test_keyword_values_are_validated_and_the_default_is_fp16():
    p = inspect.signature(MiniGPT4Classifier.__init__).parameters
    assert (p["activations"].default, p["int8_threshold"].default, p["outlier_cap"].default) == ("fp16", 6.0, 64)
    clf = _clf()
    assert clf.activations == "fp16"
    with pytest.raises(RuntimeError):
        clf.last_act_stats()
    with pytest.raises(ValueError) as e:
        _clf(activations="int4")
    assert "activations" in str(e.value)
    full = dict(activations="int8", decode="hip", prefill="hip", weights="int8")
    for bad in (0, 1025, 2.5, True):
        with pytest.raises(ValueError) as e:
            _clf(outlier_cap=bad, **full)
        assert "outlier_cap" in str(e.value)
    for bad in (float("nan"), float("inf"), "6"):
        with pytest.raises(ValueError) as e:
            _clf(int8_threshold=bad, **full)
        assert "int8_threshold" in str(e.value)


def _hf(hidden, heads, mlp):
    from transformers import LlamaConfig, LlamaForCausalLM
    lcfg = LlamaConfig(vocab_size=64, hidden_size=hidden, intermediate_size=mlp, num_hidden_layers=1, num_attention_heads=heads,
                       num_key_value_heads=heads, max_position_embeddings=64, pad_token_id=0, bos_token_id=1, eos_token_id=2)
    return LlamaForCausalLM(lcfg).half().eval()


def test_hip_decode_unsupported_names_the_multiple_of_128():
    assert inspect.signature(hip_decode_unsupported).parameters["activations"].default == "fp16"
    odd = _hf(192, 3, 320)                                             # hidden 192: a multiple of 64, not of 128 (and not heads x 128)
    plain = hip_decode_unsupported(odd)
    extra = [b for b in hip_decode_unsupported(odd, activations="int8") if b not in plain]
    assert len(extra) == 2 and "hidden_size 192" in extra[0] and "intermediate_size 320" in extra[1] and all("128" in b for b in extra)
    good = _hf(256, 2, 384)
    assert hip_decode_unsupported(good, activations="int8") == hip_decode_unsupported(good)


def test_agents_pass_the_keys_through(monkeypatch):
    src = inspect.getsource(agent)
    assert 'gen_cfg.get("activations", "fp16")' in src and "activations:" in agent.build_generating_classifier.__doc__
    seen = {}

    class Spy:
        def __init__(self, *a, **kw):
            seen.update(kw)

    import certifiedgpt_amd.minigpt4 as m
    monkeypatch.setattr(m, "MiniGPT4Classifier", Spy)
    enc = types.SimpleNamespace(max_batch=4, device="cpu")
    llm = types.SimpleNamespace(parameters=lambda: [])
    base = {"prompt": "<ImageHere>", "answers": ["a", "b"], "decode": "hip"}
    agent.build_generating_classifier(enc, dict(base, activations="int8", int8_threshold=5.0, outlier_cap=128), 4, tokenizer=object(),
                                      llama_model=llm)
    assert (seen["activations"], seen["int8_threshold"], seen["outlier_cap"]) == ("int8", 5.0, 128)
    agent.build_generating_classifier(enc, base, 4, tokenizer=object(), llama_model=llm)
    assert (seen["activations"], seen["int8_threshold"], seen["outlier_cap"]) == ("fp16", 6.0, 64)


# ------------------------------------------------------------------------------------------ the C-ABI without a device
ACT_SIZE = C.sizeof(_lib.LlmConfigAct)
GQA_SIZE = C.sizeof(_lib.LlmConfigGqa)


def _config(act_format=1, act_threshold=6.0, outlier_cap=64, reserved2=0, grouped_kv=0, reserved=0, **over):
    kw = dict(struct_size=ACT_SIZE, device=0, hidden=512, layers=2, heads=4, kv_heads=4, head_dim=128, mlp=1408, vocab=320,
              rms_eps=1e-6, rope_theta=10000.0, max_batch=8, max_len=128, weight_format=1)
    kw.update(over)
    return _lib.LlmConfigAct(gqa=_lib.LlmConfigGqa(base=_lib.LlmConfig(**kw), grouped_kv=grouped_kv, reserved=reserved),
                             act_format=act_format, act_threshold=act_threshold, outlier_cap=outlier_cap, reserved2=reserved2)


def _create(cfg):
    L = cg.lib()
    h = C.c_void_p()
    rc = L.cgpt_llm_create(C.byref(cfg.gqa.base), C.byref(h))
    msg = L.cgpt_last_error()
    if rc == 0:
        L.cgpt_llm_destroy(h)
    return rc, msg


def test_the_struct_mirrors_the_header():
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "cgpt.h")).read()
    body = re.search(r"typedef struct cgpt_llm_config_act \{(.*?)\} cgpt_llm_config_act;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(cgpt_llm_config_gqa|int32_t|float)\s+([a-z_0-9]+)\s*;", body) == [
        ("cgpt_llm_config_gqa", "gqa"), ("int32_t", "act_format"), ("float", "act_threshold"), ("int32_t", "outlier_cap"), ("int32_t", "reserved2")]
    assert _lib.LlmConfigAct._fields_ == [("gqa", _lib.LlmConfigGqa), ("act_format", C.c_int32), ("act_threshold", C.c_float),
                                          ("outlier_cap", C.c_int32), ("reserved2", C.c_int32)]
    assert _lib.LlmConfigAct.act_format.offset == GQA_SIZE and ACT_SIZE == GQA_SIZE + 16 and ACT_SIZE % 8 == 0
    assert GQA_SIZE == C.sizeof(_lib.LlmConfig) + 8 and _lib.LlmConfig._fields_[-1][0] == "weight_format"      # the older structs did not grow
    for name in ("cgpt_llm_act_stats", "cgpt_llm_linear_i8", "cgpt_llm_linear_i8_workspace", "cgpt_llm_linear_i8_slices"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\(" % name, text)


def test_good_configs_pass_validation():
    for over in (dict(), dict(act_threshold=0.0), dict(act_threshold=-1.0), dict(outlier_cap=1), dict(outlier_cap=1024),
                 dict(grouped_kv=1, kv_heads=2), dict(act_format=0, weight_format=0), dict(act_format=0, weight_format=1),
                 dict(act_format=0, outlier_cap=-5, act_threshold=float("nan"), mlp=1344)):
        rc, msg = _create(_config(**over))
        assert rc in ACCEPTED, (over, rc, msg)
        if not torch.cuda.is_available():
            assert rc == NO_DEVICE, (over, rc, msg)


@pytest.mark.parametrize("over, word", [(dict(weight_format=0), b"weight_format"), (dict(act_format=2), b"act_format"),
                                        (dict(act_format=-1), b"act_format"), (dict(outlier_cap=0), b"outlier_cap"),
                                        (dict(outlier_cap=1025), b"outlier_cap"), (dict(act_threshold=float("nan")), b"act_threshold"),
                                        (dict(act_threshold=float("inf")), b"act_threshold"), (dict(mlp=1344), b"128"),
                                        (dict(reserved2=1), b"reserved2"), (dict(reserved=1), b"reserved"),
                                        (dict(kv_heads=2), b"kv_heads")])
def test_bad_configs_are_invalid_before_any_device_call(over, word):
    rc, msg = _create(_config(**over))
    assert rc == INVALID and word in msg, (over, rc, msg)


def test_the_older_struct_sizes_behave_as_before():
    older = (GQA_SIZE, C.sizeof(_lib.LlmConfig), _lib.LLM_CONFIG_SIZE_F16)
    for size in older:
        # what lies behind the struct the size names is NOT read: garbage in the activation fields must not matter
        rc, msg = _create(_config(struct_size=size, act_format=7, outlier_cap=-1, reserved2=9, act_threshold=float("nan"), weight_format=0))
        assert rc in ACCEPTED, (size, rc, msg)
    rc, msg = _create(_config(struct_size=GQA_SIZE, reserved=1, weight_format=0))
    assert rc == INVALID and b"reserved" in msg
    for size in (0, _lib.LLM_CONFIG_SIZE_F16 - 4, C.sizeof(_lib.LlmConfig) + 4, GQA_SIZE + 4, GQA_SIZE + 8, ACT_SIZE - 4, ACT_SIZE + 4, ACT_SIZE + 8):
        rc, msg = _create(_config(struct_size=size))
        assert rc == INVALID and b"struct_size" in msg, (size, rc, msg)


def test_raw_entry_helpers_without_a_device():
    L = cg.lib()
    assert [L.cgpt_llm_linear_i8_slices(n, k) for n, k in ((64, 128), (192, 256), (64, 1024), (128, 2048))] == [1, 1, 2, 4]
    assert L.cgpt_llm_linear_i8_slices(12288, 4096) == 1 and L.cgpt_llm_linear_i8_slices(4096, 4096) == 4
    for n, k in ((0, 128), (96, 128), (64, 64), (64, 192), (64, 65536 + 128)):
        assert L.cgpt_llm_linear_i8_slices(n, k) == -1
    off = (C.c_int64 * 5)()
    total = L.cgpt_llm_linear_i8_workspace(37, 64, 1024, 16, off)
    o = list(off)
    assert o[0] == 0 and o[1] >= 32 and o[2] - o[1] >= 256 * 1024 and o[3] - o[2] >= 256 * 4 and o[4] - o[3] >= 256 * 17 * 4
    assert total - o[4] >= 2 * 256 * 64 * 4 and all(v % 256 == 0 for v in o)
    assert L.cgpt_llm_linear_i8_workspace(600, 64, 1024, 16, off) > 0 and list(off)[2] - list(off)[1] >= 768 * 1024
    for bad in ((0, 64, 128, 16), (1, 64, 128, 0), (1, 64, 128, 1025), (1, 64, 100, 16), (2 ** 24 + 1, 64, 128, 16)):
        assert L.cgpt_llm_linear_i8_workspace(*bad, None) == -1
    rc = L.cgpt_llm_linear_i8(None, None, None, 1, 64, 128, 6.0, 16, 0, None, None, 128, None, 0, None)
    assert rc == INVALID and b"null" in L.cgpt_last_error()
    v = (C.c_int64 * 4)()
    assert L.cgpt_llm_act_stats(None, v) == INVALID
