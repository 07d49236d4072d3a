"""Per-row stop sequences of the greedy decode (stop_words_ids / stop_text) without a GPU: the rule itself
(`stop_finish_columns`, `apply_stop_sequences`) on hand-written tables, the keyword validation, the HF path and the eager torch loop on
the toy decoder, the C entry's declaration, binding and argument checks, the agent's pass-through and the graph cache key.

The oracle everywhere: greedy rows are independent, so a decode WITH stop sequences equals `apply_stop_sequences` of the same decode
WITHOUT them, bit for bit.  tests/test_gpu_llm_stop.py holds the native engine to the same identity."""
import ctypes as C
import inspect
import os
import re
import types

import pytest
import torch

import certifiedgpt_amd as cg
from certifiedgpt_amd import _lib
from certifiedgpt_amd.agents import minigpt4_certify_agent as agent
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import (MiniGPT4Classifier, WordHashTokenizer, apply_stop_sequences, check_stop_words_ids,
                                       stop_finish_columns)
from test_llm_early_stop_cpu import finishing_select
from toy_llm import EOS, PAD, StubEncoder, ToyTokenizer, tiny_llama

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ 1. the rule
def test_the_rule_on_hand_written_tables():
    a, b, c, E, P = 7, 8, 9, 2, 0
    assert stop_finish_columns([[c, a, c, c]], [], [[a]]) == [1]                                  # a one-token stop
    assert apply_stop_sequences([[c, a, c, c]], [], [[a]], P) == [[c, a, P, P]]                   # the finishing token stays
    assert stop_finish_columns([[a, a, b, c]], [], [[a, b]]) == [2]                               # [a, b] on a a b
    assert stop_finish_columns([[a, a, a, c]], [], [[a, a]]) == [1]                               # overlap: the first match counts
    assert stop_finish_columns([[a, b, c]], [], [[a, b, c, a]]) == [3]                            # longer than the row: never
    assert apply_stop_sequences([[a, b, c]], [], [[a, b, c, a]], P) == [[a, b, c]]
    for k in (1, 2, 3):                                                                          # the row's first k tokens: column k - 1
        assert stop_finish_columns([[a, b, c, c]], [], [[a, b, c][:k]]) == [k - 1]
    assert stop_finish_columns([[b, a, b, c]], [], [[a, b, c][1:]]) == [3]                        # [b, c] is not matched before column 1
    assert stop_finish_columns([[c, E, a, b]], [E], [[a, b]]) == [1]                              # EOS before a stop match
    assert stop_finish_columns([[a, b, E, c]], [E], [[a, b]]) == [1]                              # a stop match before EOS
    assert apply_stop_sequences([[c, E, a, b], [a, b, E, c]], [E], [[a, b]], P) == [[c, E, P, P], [a, b, P, P]]
    # the stop token equal to the pad id: the row finishes once, at its first pad-valued token, and stays finished
    assert stop_finish_columns([[c, P, c, c]], [], [[P]]) == [1]
    assert apply_stop_sequences([[c, P, c, c]], [], [[P]], P) == [[c, P, P, P]]
    assert apply_stop_sequences(apply_stop_sequences([[c, P, c, c]], [], [[P]], P), [], [[P]], P) == [[c, P, P, P]]
    # several sequences: the earliest finish of any
    assert stop_finish_columns([[a, b, c, a]], [], [[c, a], [b]]) == [1]
    # no sequences: today's EOS rule, the F of the early-stop tests
    tables = ([[5, 6, 7, 8], [9, 9, 9, 9]], [[E, P, P, P], [E, P, P, P]], [[5, E, P, P, P, P], [5, 6, 7, E, P, P], [E, P, P, P, P, P]],
              [[5, 11, P, P], [E, P, P, P]])
    for table in tables:
        for eos in ([E], [E, 11], []):
            for none in ([], None, ()):
                cols = stop_finish_columns(table, eos, none)
                assert max(cols) == finishing_select(table, eos)
                assert cols == [next((i for i, t in enumerate(row) if t in eos), len(row)) for row in table]
    # tensors and nested lists alike
    T = torch.tensor([[a, a, b, c], [c, c, c, c], [b, E, a, b]])
    seqs = [[a, b], [c]]
    assert stop_finish_columns(T, [E], seqs) == stop_finish_columns(T.tolist(), torch.tensor([E]), [torch.tensor(s) for s in seqs]) == [2, 0, 1]
    got = apply_stop_sequences(T, [E], seqs, P)
    assert isinstance(got, torch.Tensor) and got.dtype == T.dtype and got.tolist() == apply_stop_sequences(T.tolist(), [E], seqs, P)
    assert got.tolist() == [[a, a, b, P], [c, P, P, P], [b, E, P, P]] and T[0, 3] == c              # a new table: the input is left alone


# ------------------------------------------------------------------------------------------ 2. the keywords
def _clf(**kw):
    return MiniGPT4Classifier(None, object(), WordHashTokenizer(96), "<ImageHere>", AnswerLabelMap(4, ()), max_batch=4, **kw)


@pytest.mark.parametrize("bad, names", [
    ([[i] for i in range(9)], "9 sequences"),
    ([[5], []], "stop_words_ids[1]"),
    ([list(range(9))], "stop_words_ids[0]"),
    ([[3, 4], [5, -1]], "stop_words_ids[1]"),
    ("###", "stop_words_ids"),
    ([[3], "ab"], "stop_words_ids[1]"),
    ([[3.5]], "stop_words_ids[0]"),
    (7, "stop_words_ids"),
])
def test_stop_words_ids_is_validated(bad, names):
    with pytest.raises(ValueError) as e:
        _clf(stop_words_ids=bad)
    assert "stop_words_ids" in str(e.value) and names in str(e.value), str(e.value)


def test_stop_text_is_a_string():
    for bad in (3, ["###"], b"###", ""):
        with pytest.raises(ValueError) as e:
            _clf(stop_text=bad)
        assert "stop_text" in str(e.value)


def test_defaults_are_none_and_accepted_forms():
    p = inspect.signature(MiniGPT4Classifier.__init__).parameters
    assert p["stop_words_ids"].default is None and p["stop_text"].default is None
    clf = _clf()
    assert clf.stop_words_ids is None and clf.stop_text is None
    assert _clf(stop_words_ids=[]).stop_words_ids is None                                        # an empty list sets nothing
    assert _clf(stop_words_ids=[2]).stop_words_ids == ((2,),)                                    # the reference's [2]: one-token sequences
    assert _clf(stop_words_ids=[[5, 6], (7,), torch.tensor([8, 9, 10])]).stop_words_ids == ((5, 6), (7,), (8, 9, 10))
    assert check_stop_words_ids([list(range(8))] * 8) == (tuple(range(8)),) * 8                  # the limits themselves are fine
    for decode in ("hf", "graph"):                                                               # every engine takes the keyword
        assert _clf(decode=decode, stop_words_ids=[[5, 6]], stop_text="###").stop_text == "###"


# ------------------------------------------------------------------------------------------ 3. the toy decoder, HF path and torch loop
PROMPT = "<ImageHere> what is in the picture"


@pytest.fixture(scope="module")
def toy():
    """The decode without stop sequences, computed once: (llm, image embeds, prompt embeds, T)."""
    llm = tiny_llama(seed=0)
    clf = MiniGPT4Classifier(StubEncoder(), llm, ToyTokenizer(), PROMPT, AnswerLabelMap(4, ()), max_new_tokens=12, max_batch=12)
    g = torch.Generator().manual_seed(0)
    img, _ = clf.encoder.encode_img(torch.randn(12, 3, 8, 8, generator=g))
    segs = clf._segment_embeddings(PROMPT, img.device)
    embs = torch.cat([segs[0].expand(12, -1, -1), img, segs[1].expand(12, -1, -1)], dim=1)
    with torch.no_grad():
        T = clf.greedy_tokens(embs)
    return llm, img, embs, T


def _toy_clf(llm, **kw):
    return MiniGPT4Classifier(StubEncoder(), llm, ToyTokenizer(), PROMPT, AnswerLabelMap(4, ()), max_new_tokens=12, max_batch=12, **kw)


def _toy_seqs(T):
    return [[int(T[0, 1])], [int(T[1, 2]), int(T[1, 3])], [int(T[2, 4]), int(T[2, 5]), int(T[2, 6])]]


def test_preconditions_on_the_toy_decode(toy):
    _, _, _, T = toy
    assert T.shape == (12, 12)
    seqs = _toy_seqs(T)
    cols = stop_finish_columns(T, [EOS], seqs)
    print("finishing columns:", cols, "sequences:", seqs)
    finished = [c for c in cols if c < 12]
    assert len(finished) >= 3 and len(set(finished)) >= 2 and len(finished) < 12, cols
    assert cols != stop_finish_columns(T, [EOS], [])                                             # the sequences change something


def test_hf_path_gives_the_rule(toy):
    llm, img, _, T = toy
    seqs = _toy_seqs(T)
    want_tokens = apply_stop_sequences(T, [EOS], seqs, PAD)
    plain = _toy_clf(llm)
    want = plain._decode_outputs(want_tokens)
    assert want != plain._decode_outputs(T)
    clf = _toy_clf(llm, decode="hf", stop_words_ids=seqs)
    assert clf.generate_from_embeds(img, PROMPT) == want
    assert clf.decode_stats["hf_calls"] == 1
    assert plain.generate_from_embeds(img, PROMPT) == plain._decode_outputs(T)                   # and without them HF gives T


def test_eager_torch_loop_gives_the_rule(toy):
    llm, _, embs, T = toy
    seqs = _toy_seqs(T)
    clf = _toy_clf(llm, decode="graph", stop_words_ids=seqs)
    with torch.no_grad():
        got, logits = clf.greedy_tokens(embs, return_logits=True)
    assert torch.equal(got, apply_stop_sequences(T, [EOS], seqs, PAD))
    assert logits.shape[:2] == (12, 12)
    with torch.no_grad():
        assert torch.equal(_toy_clf(llm, decode="graph").greedy_tokens(embs), T)                  # without them: unchanged


def test_stop_text_cuts_the_decoded_answer(toy):
    llm, _, _, T = toy
    plain = _toy_clf(llm)
    text = plain._decode_outputs(T[3:4])[0]
    words = text.split()
    assert len(words) >= 3, text
    cut = _toy_clf(llm, stop_text=words[2])
    want = text.split(words[2])[0].strip()
    assert cut._decode_outputs(T[3:4]) == [want] and want != text and text.startswith(want)
    assert _toy_clf(llm, stop_text="###")._decode_outputs(T[3:4]) == [text]                      # absent: nothing is cut


# ------------------------------------------------------------------------------------------ 4. the C entry
_CTYPES = {"cgpt_llm_handle": C.c_void_p, "const int64_t*": C.POINTER(C.c_int64), "const int32_t*": C.POINTER(C.c_int32),
           "int32_t": C.c_int32}


def test_header_declares_and_binding_matches():
    text = open(os.path.join(ROOT, "include", "cgpt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    name = "cgpt_llm_set_stop_sequences"
    m = re.search(r"cgpt_status\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m, f"cgpt.h does not declare {name}"
    assert hasattr(cg.lib(), name), f"libcgpt.so does not export {name}"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert [re.search(r"([A-Za-z_0-9]+)$", p).group(1) for p in params] == ["h", "ids_host", "lens_host", "n"]
    types_ = [re.sub(r"\s*\b[A-Za-z_0-9]+$", "", p).replace(" *", "*") for p in params]
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int32 and [_CTYPES[t] for t in types_] == list(args), types_
    assert "Stop sequences" in text and "n = 0 clears" in text


def test_entry_refuses_bad_arguments_without_a_device():
    L = cg.lib()
    name = b"cgpt_llm_set_stop_sequences"
    ids = (C.c_int64 * 80)(*range(80))
    lens = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731

    def refused(*call):
        assert L.cgpt_llm_set_stop_sequences(*call) == 1                                          # CGPT_ERR_INVALID
        msg = L.cgpt_last_error()
        assert name in msg, msg
        return msg

    assert b"null handle" in refused(None, ids, lens(2, 3), 2)
    assert b"null handle" in refused(None, None, None, 0)
    assert b"9 sequences" in refused(None, ids, lens(*[1] * 9), 9)
    assert b"-1 sequences" in refused(None, ids, lens(1), -1)
    assert b"sequence 1" in refused(None, ids, lens(2, 0), 2)
    assert b"sequence 0" in refused(None, ids, lens(9), 1)
    assert b"sequence 2" in refused(None, ids, lens(1, 1, -3), 3)
    neg = (C.c_int64 * 4)(5, 6, -1, 7)
    assert b"negative" in refused(None, neg, lens(2, 2), 2)
    assert b"null" in refused(None, None, lens(1), 1)
    assert b"null" in refused(None, ids, None, 1)


# ------------------------------------------------------------------------------------------ 5. the agent
def test_agent_passes_both_keys_through(monkeypatch):
    assert "stop_words_ids" in agent.__doc__ and "stop_text" in agent.__doc__
    seen = {}

    class Spy:
        def __init__(self, *a, **kw):
            seen.update(kw)

    import certifiedgpt_amd.minigpt4 as m
    monkeypatch.setattr(m, "MiniGPT4Classifier", Spy)
    enc = types.SimpleNamespace(max_batch=4, device="cpu")
    llm = types.SimpleNamespace(parameters=lambda: [])
    base = {"prompt": "<ImageHere>", "answers": ["a", "b"], "decode": "hip", "early_stop": True, "end_sym": "###"}
    agent.build_generating_classifier(enc, dict(base, stop_words_ids=[[5, 6], [7]], stop_text="###"), 4, tokenizer=object(), llama_model=llm)
    assert seen["stop_words_ids"] == [[5, 6], [7]] and seen["stop_text"] == "###" and seen["early_stop"] is True
    agent.build_generating_classifier(enc, base, 4, tokenizer=object(), llama_model=llm)
    assert seen["stop_words_ids"] is None and seen["stop_text"] is None


# ------------------------------------------------------------------------------------------ 6. the graph key
def test_graph_key_carries_the_sequences():
    embs = types.SimpleNamespace(shape=(4, 12, 512), dtype=torch.float16, device=types.SimpleNamespace(index=0))
    plain = _clf()._graph_key(embs)
    assert plain == (4, 12, torch.float16, 0, 20, False, "hf", "model")                          # the key as it was before the keyword
    one, other = _clf(stop_words_ids=[[5, 6]]), _clf(stop_words_ids=[[5], [6]])
    keys = {plain, one._graph_key(embs), other._graph_key(embs), one._graph_key(embs, ragged=True)}
    assert len(keys) == 4
    assert one._graph_key(embs) == _clf(stop_words_ids=[(5, 6)])._graph_key(embs)                # the same set, the same graph
    assert _clf(stop_text="###")._graph_key(embs) == plain                                       # the text cut happens after the graph
