"""shared_prefix=True (cgpt_llm_prefill_from, cgpt_llm_kv_broadcast) without a GPU: the two entries are declared and bound with the
declared signature and refuse a null handle and every bad argument before any device call; `shared_prefix_len` and the suffix padding
rule; the keyword never selects another engine; the graph key, the prefix LRU and its counters; the agent forwards the key."""
import ctypes as C
import os
import re

import pytest
import torch

import certifiedgpt_amd as cg
from certifiedgpt_amd import _lib
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.llm_laws import left_pad_embeds, shared_prefix_len
from certifiedgpt_amd.minigpt4 import MiniGPT4Classifier, prepare_texts
from toy_llm import StubEncoder, ToyTokenizer, tiny_llama

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPT = prepare_texts(["<Img><ImageHere></Img> what is this"])[0]
INVALID = 1                                                            # CGPT_ERR_INVALID

_CTYPES = {"cgpt_llm_handle": C.c_void_p, "const void*": C.c_void_p, "void*": C.c_void_p, "void* const*": C.c_void_p,
           "float*": C.c_void_p, "const int32_t*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}


def _classifier(llm, **kw):
    return MiniGPT4Classifier(StubEncoder(), llm, ToyTokenizer(), PROMPT, AnswerLabelMap(4, ()), max_new_tokens=3, **kw)


# ------------------------------------------------------------------------------------------ the C-ABI
def test_header_declares_and_binding_matches_the_two_entries():
    text = open(os.path.join(ROOT, "include", "cgpt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = cg.lib()
    for name in ("cgpt_llm_prefill_from", "cgpt_llm_kv_broadcast"):
        m = re.search(r"cgpt_status\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, f"cgpt.h does not declare {name}"
        assert hasattr(L, name), f"libcgpt.so does not export {name}"
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        types = [re.sub(r"\s*\b[A-Za-z_0-9]+$", "", p).replace(" *", "*") for p in params]
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int32 and [_CTYPES[t] for t in types] == list(args), (name, types)
    # the header says which rows are written and what must already be there
    assert "rows 0 .. pos0-1 of every layer's K / V buffer MUST ALREADY HOLD" in text and "writes rows pos0 .. pos0+Ln-1" in text
    assert "No other cache row is written" in text


def test_prefill_from_takes_the_ragged_prefill_arguments_plus_pos0():
    ragged, cont = _lib.SIGNATURES["cgpt_llm_prefill_ragged"][1], _lib.SIGNATURES["cgpt_llm_prefill_from"][1]
    assert list(cont[:3]) + list(cont[4:]) == list(ragged) and cont[3] is C.c_int32


def _buf():
    return C.cast((C.c_uint16 * 64)(), C.c_void_p)


def test_prefill_from_refuses_a_null_handle_and_each_bad_argument():
    L = cg.lib()
    b = _buf()
    tables = (C.c_void_p * 2)(b, b)

    def call(B=1, pos0=4, Ln=4, stride=8, h=None, embs=b, logits=b):
        rc = L.cgpt_llm_prefill_from(h, embs, B, pos0, Ln, None, tables, tables, stride, logits, None)
        return rc, L.cgpt_last_error().decode()

    rc, msg = call()
    assert rc == INVALID and "cgpt_llm_prefill_from" in msg and "null" in msg
    for kw, word in ((dict(Ln=0), "Ln"), (dict(Ln=-3), "Ln"), (dict(pos0=-1), "pos0"), (dict(pos0=5, Ln=4, stride=8), "kv_len_stride"),
                     (dict(embs=None), "null"), (dict(logits=None), "null")):
        rc, msg = call(**kw)
        assert rc == INVALID and "cgpt_llm_prefill_from" in msg and word in msg, (kw, msg)
    assert L.cgpt_llm_prefill_from(None, None, 1, 0, 4, None, None, None, 8, None, None) == INVALID


def test_kv_broadcast_refuses_a_null_handle_and_each_bad_argument():
    L = cg.lib()
    b = _buf()
    tables = (C.c_void_p * 2)(b, b)

    def call(P=4, B=2, src=8, dst=8):
        rc = L.cgpt_llm_kv_broadcast(None, tables, tables, src, P, B, None, tables, tables, dst, None)
        return rc, L.cgpt_last_error().decode()

    rc, msg = call()
    assert rc == INVALID and "cgpt_llm_kv_broadcast" in msg and "null handle" in msg
    for kw, word in ((dict(P=0), "P must be at least 1"), (dict(P=-2), "P must be at least 1"), (dict(P=9, src=8, dst=16), "src_len_stride"),
                     (dict(P=9, src=16, dst=8), "dst_len_stride")):
        rc, msg = call(**kw)
        assert rc == INVALID and "cgpt_llm_kv_broadcast" in msg and word in msg, (kw, msg)
    assert L.cgpt_llm_kv_broadcast(None, None, None, 8, 4, 2, None, None, None, 8, None) == INVALID


# ------------------------------------------------------------------------------------------ the laws
def test_shared_prefix_len_equal_unequal_and_empty():
    assert shared_prefix_len([[1, 5, 9]]) == 3
    assert shared_prefix_len([[1, 5, 9], (1, 5, 9), torch.tensor([1, 5, 9]).tolist()]) == 3
    assert shared_prefix_len([[1, 5, 9], [1, 5, 8]]) == 0             # equal lengths, other tokens
    assert shared_prefix_len([[1, 5, 9], [1, 5]]) == 0                # one is a prefix of the other: still not the same segment
    assert shared_prefix_len([[1, 5], [1, 5], [2, 5]]) == 0           # the odd row is not the second one
    assert shared_prefix_len([]) == 0 and shared_prefix_len([[]]) == 0 and shared_prefix_len([[], []]) == 0


@pytest.mark.parametrize("bucket", [None, 1, 8, 16, 64])
@pytest.mark.parametrize("P", [1, 3, 7, 40])
def test_suffix_padding_keeps_the_padded_length_and_the_starts(bucket, P):
    """P + Ls is the padded length of the same rows with their prefix in front, and the starts are the same: the K/V pool and the
    graph's bucket do not move."""
    for lens in ([37], [1, 9, 30], [16 - P % 16, 33], [64, 65, 5]):
        whole = [torch.ones(1, P + n, 4) for n in lens]
        suffix = [torch.ones(1, n, 4) for n in lens]
        w_embs, w_mask, w_starts = left_pad_embeds(whole, bucket)
        s_embs, s_mask, s_starts = left_pad_embeds(suffix, bucket, prefix=P)
        assert P + s_embs.shape[1] == w_embs.shape[1], (lens, bucket, P)
        assert torch.equal(s_starts, w_starts)
        assert torch.equal(s_mask.sum(1) + P, w_mask.sum(1))
        assert all(0 <= int(s) < s_embs.shape[1] for s in s_starts)    # every row keeps a real suffix token
    with pytest.raises(ValueError):
        left_pad_embeds([torch.ones(1, 3, 4)], bucket, prefix=-1)
    a, b = left_pad_embeds([torch.ones(1, 3, 4), torch.ones(2, 5, 4)], bucket), left_pad_embeds([torch.ones(1, 3, 4), torch.ones(2, 5, 4)], bucket, prefix=0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))                # prefix = 0 is the function as it was


# ------------------------------------------------------------------------------------------ the keyword
@pytest.mark.parametrize("kw", [dict(), dict(decode="graph"), dict(decode="hf", prefill="model")])
def test_shared_prefix_with_another_engine_is_a_value_error_naming_both(kw):
    with pytest.raises(ValueError) as e:
        _classifier(tiny_llama(), shared_prefix=True, **kw)
    assert 'decode="hip"' in str(e.value) and 'prefill="hip"' in str(e.value) and "shared_prefix" in str(e.value)


def test_shared_prefix_is_off_by_default_and_refuses_other_values():
    clf = _classifier(tiny_llama())
    assert clf.shared_prefix is False and len(clf._prefixes) == 0 and clf.max_prefixes == 4
    assert clf.decode_stats["hip_prefix_prefills"] == 0 and clf.decode_stats["hip_prefix_hits"] == 0
    clf.generate_from_embeds(torch.zeros(2, 4, 64), PROMPT)            # CPU tensors: the HF call, no prefix work
    assert clf.decode_stats["hf_calls"] == 1 and clf.decode_stats["hip_prefix_prefills"] == 0 and len(clf._prefixes) == 0
    with pytest.raises(ValueError):
        _classifier(tiny_llama(), shared_prefix=1)
    with pytest.raises(ValueError):                                    # an unsupported decoder stays a ValueError, never another engine
        _classifier(tiny_llama(), decode="hip", prefill="hip", shared_prefix=True)


def test_graph_key_gains_its_element_only_under_the_flag():
    clf = _classifier(tiny_llama(), decode="graph")
    embs = torch.zeros(2, 4, 64)
    plain = clf._graph_key(embs)
    assert plain == clf._graph_key(embs, prefix=0) and "prefix" not in plain
    keyed = clf._graph_key(embs, prefix=7)
    assert keyed[:len(plain)] == plain and keyed[len(plain):] == ("prefix", 7)
    assert clf._graph_key(embs, prefix=8) != keyed
    ragged = clf._graph_key(embs, ragged=True, prefix=7)
    assert "ragged" in ragged and ragged[-2:] == ("prefix", 7)


# ------------------------------------------------------------------------------------------ the LRU
class _StubEngine:
    layers, kv_heads = 2, 4

    def __init__(self):
        self.prefills = []

    def prefill(self, embs, k_bufs, v_bufs, starts=None):
        assert starts is None and embs.shape[0] == 1 and len(k_bufs) == len(v_bufs) == self.layers
        assert all(tuple(t.shape) == (1, self.kv_heads, embs.shape[1], 128) for t in k_bufs + v_bufs)
        self.prefills.append(embs.shape[1])
        for t in k_bufs + v_bufs:
            t.fill_(float(len(self.prefills)))


def test_prefix_lru_and_its_counters_with_a_stubbed_engine():
    clf = _classifier(tiny_llama())
    clf._hip = eng = _StubEngine()
    s = clf.decode_stats
    a, b = (1, 10, 11), (1, 10, 12)
    first = clf._prefix_entry(a, "cpu")
    assert first.ids == a and first.P == 3 and len(first.k) == len(first.v) == eng.layers
    assert eng.prefills == [3] and s["hip_prefix_prefills"] == 1 and s["hip_prefix_hits"] == 0
    again = clf._prefix_entry(a, "cpu")
    assert again is first and eng.prefills == [3] and s["hip_prefix_hits"] == 1
    clf._prefix_entry(b, "cpu")                                        # same length, other ids: an entry of its own
    assert eng.prefills == [3, 3] and s["hip_prefix_prefills"] == 2 and float(clf._prefixes[b].k[0].max()) == 2.0
    for i in range(3):                                                 # a, b + three more: one over the 4 entries
        clf._prefix_entry((1, 20 + i), "cpu")
    assert list(clf._prefixes) == [b, (1, 20), (1, 21), (1, 22)] and s["hip_prefix_prefills"] == 5
    clf._prefix_entry(b, "cpu")                                        # a hit moves the entry to the recent end ...
    clf._prefix_entry((1, 30), "cpu")                                  # ... so the next miss drops (1, 20), not b
    assert list(clf._prefixes) == [(1, 21), (1, 22), b, (1, 30)] and s["hip_prefix_hits"] == 2 and s["hip_prefix_prefills"] == 6
    clf._prefix_entry(a, "cpu")                                        # a was evicted: prefilled again
    assert s["hip_prefix_prefills"] == 7 and len(clf._prefixes) == 4


def test_the_static_copy_of_a_graph_is_refreshed_only_for_another_prefix():
    from certifiedgpt_amd.minigpt4 import _Prefix
    a = _Prefix((1, 10, 11), [torch.full((1, 4, 3, 128), 1.0)], [torch.full((1, 4, 3, 128), 2.0)])
    b = _Prefix((1, 10, 12), [torch.full((1, 4, 3, 128), 3.0)], [torch.full((1, 4, 3, 128), 4.0)])
    static = a.clone()
    assert static.ids == a.ids and static.k[0] is not a.k[0] and torch.equal(static.k[0], a.k[0])
    a.k[0].fill_(9.0)                                                  # same ids: nothing is copied, whatever the tensors hold
    static.hold(a)
    assert float(static.k[0].max()) == 1.0
    kept = static.k[0]
    static.hold(b)                                                     # other ids: copied in place, the graph's addresses stay
    assert static.ids == b.ids and static.k[0] is kept and torch.equal(static.k[0], b.k[0]) and torch.equal(static.v[0], b.v[0])


def test_the_prefix_ids_come_from_the_tokenizers_host_output():
    clf = _classifier(tiny_llama())
    ids = clf._segment_ids(PROMPT)
    assert len(ids) == 2 and all(t.device.type == "cpu" for t in ids)
    assert [t.tolist() for t in clf._segment_tokens(PROMPT, "cpu")] == [t.tolist() for t in ids]


# ------------------------------------------------------------------------------------------ the agent
def test_agent_documents_and_forwards_shared_prefix(monkeypatch):
    import inspect
    from certifiedgpt_amd.agents import minigpt4_certify_agent as agent
    src = inspect.getsource(agent)
    assert "shared_prefix: false | true" in src and 'gen_cfg.get("shared_prefix", False)' in src
    seen = {}

    class Recorder:
        def __init__(self, *args, **kw):
            seen.update(kw)

    import certifiedgpt_amd.minigpt4 as minigpt4
    monkeypatch.setattr(minigpt4, "MiniGPT4Classifier", Recorder)
    gen = {"prompt": PROMPT, "answers": ["a", "b", "c"], "decode": "hip", "prefill": "hip", "shared_prefix": True}
    agent.build_generating_classifier(StubEncoder(), gen, 4, tokenizer=ToyTokenizer(), llama_model=tiny_llama())
    assert seen["shared_prefix"] is True and seen["decode"] == "hip" and seen["prefill"] == "hip"
    seen.clear()
    del gen["shared_prefix"]
    agent.build_generating_classifier(StubEncoder(), gen, 4, tokenizer=ToyTokenizer(), llama_model=tiny_llama())
    assert seen["shared_prefix"] is False
