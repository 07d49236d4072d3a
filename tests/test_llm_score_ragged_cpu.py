"""Per-row prompts and per-row candidates on the native scoring pass, without a GPU: `pack_row_candidates` on hand-written cases
and at the engine's limits, the cgpt_llm_score_ragged entry (declared, bound with the declared signature, null arguments refused),
the fall-back of a ragged="hip", score="hip" classifier off the device, and the unchanged constructor rules."""
import ctypes as C
import os
import re

import pytest
import torch

import certifiedgpt_amd as cg
from certifiedgpt_amd import _lib
from certifiedgpt_amd import minigpt4
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import MiniGPT4Classifier, _HipDecoder, pack_row_candidates, prepare_texts
from toy_llm import StubEncoder, ToyTokenizer, tiny_llama

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPT = prepare_texts(["<Img><ImageHere></Img> what is this"])[0]

_CTYPES = {"cgpt_llm_handle": C.c_void_p, "const void*": C.c_void_p, "void*": C.c_void_p, "void* const*": C.c_void_p,
           "float*": C.c_void_p, "const float*": C.c_void_p, "const int64_t*": C.c_void_p, "const int32_t*": C.c_void_p,
           "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}


def _classifier(llm, **kw):
    return MiniGPT4Classifier(StubEncoder(), llm, ToyTokenizer(), PROMPT, AnswerLabelMap(6, ()), max_new_tokens=3, **kw)


# ------------------------------------------------------------------------------------------ pack_row_candidates
def test_pack_row_candidates_on_a_hand_written_case():
    # cand[c][b]: 3 candidates x 2 rows
    cand = [[[5, 6, 7], [8]],
            [[9], [10]],
            [torch.tensor([11, 12]), torch.tensor([13, 14, 15, 16])]]
    table, lens, T, S = pack_row_candidates(cand)
    assert table.dtype == torch.int64 and lens.dtype == torch.int32 and tuple(table.shape) == (2, 3, 4) and tuple(lens.shape) == (2, 3)
    assert table.tolist() == [[[5, 6, 7, 0], [9, 0, 0, 0], [11, 12, 0, 0]],
                              [[8, 0, 0, 0], [10, 0, 0, 0], [13, 14, 15, 16]]]
    assert lens.tolist() == [[3, 1, 2], [1, 1, 4]]
    assert T == [3, 1, 4] and all(isinstance(t, int) for t in T)       # the longest length of each candidate over the rows
    assert S == 2 + 0 + 3
    assert table.is_contiguous() and lens.is_contiguous() and not table.is_cuda


def test_pack_row_candidates_with_one_row_is_the_shared_table():
    table, lens, T, S = pack_row_candidates([[[4, 5]], [[6]], [[7, 8, 9]]])
    assert table.tolist() == [[[4, 5, 0], [6, 0, 0], [7, 8, 9]]] and lens.tolist() == [[2, 1, 3]] and T == [2, 1, 3] and S == 3


def test_one_token_candidates_own_no_slot():
    table, lens, T, S = pack_row_candidates([[[3], [4], [5]], [[6], [7], [8]]])
    assert S == 0 and T == [1, 1] and tuple(table.shape) == (3, 2, 1) and bool((lens == 1).all())
    # one row lengthens one candidate: the slot exists for every row, the other rows' lengths stay 1
    table, lens, T, S = pack_row_candidates([[[3], [4, 9], [5]], [[6], [7], [8]]])
    assert S == 1 and T == [2, 1] and lens.tolist() == [[1, 1], [2, 1], [1, 1]] and table[:, 0].tolist() == [[3, 0], [4, 9], [5, 0]]


def test_the_64_slot_limit_is_reported_not_hidden():
    assert _HipDecoder.MAX_TAIL == 64 and _HipDecoder.MAX_CANDS == 64
    fits = [[list(range(3, 3 + 17)), [3]], [[3, 4], list(range(3, 3 + 49))]]           # T = (17, 49): 16 + 48 slots
    assert pack_row_candidates(fits)[3] == 64
    over = [[list(range(3, 3 + 17)), [3]], [[3, 4], list(range(3, 3 + 50))]]
    _, lens, T, S = pack_row_candidates(over)
    assert S == 65 and T == [17, 50] and lens.tolist() == [[17, 2], [1, 50]]           # the caller compares with MAX_TAIL and declines


def test_pack_row_candidates_refuses_what_has_no_meaning():
    with pytest.raises(ValueError):
        pack_row_candidates([])
    with pytest.raises(ValueError):
        pack_row_candidates([[[3], [4]], [[5]]])                       # rows disagree in number
    with pytest.raises(ValueError):
        pack_row_candidates([[[3], []]])                               # a candidate without a token
    with pytest.raises(ValueError):
        pack_row_candidates([[]])                                      # no row


# ------------------------------------------------------------------------------------------ the C-ABI
def test_header_declares_and_binding_matches_the_ragged_score_entry():
    text = open(os.path.join(ROOT, "include", "cgpt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = cg.lib()
    name = "cgpt_llm_score_ragged"
    m = re.search(r"cgpt_status\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m, f"cgpt.h does not declare {name}"
    assert hasattr(L, name), f"libcgpt.so does not export {name}"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    names = [re.search(r"([A-Za-z_0-9]+)$", p).group(1) for p in params]
    assert names == ["h", "first_logits_dev", "B", "prompt_len", "starts_dev", "cand_tokens_dev", "cand_lens_dev", "cand_lens_host", "C",
                     "Tmax", "label_smoothing", "k_ptrs_host", "v_ptrs_host", "kv_len_stride", "out_dev", "stream"]
    types = [re.sub(r"\s*\b[A-Za-z_0-9]+$", "", p).replace(" *", "*") for p in params]
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int32
    assert [_CTYPES[t] for t in types] == list(args), types
    # the plain entry's arguments with the two device arrays added: everything else travels as it does there
    plain = list(_lib.SIGNATURES["cgpt_llm_score"][1])
    assert list(args[:4]) == plain[:4] and list(args[5:6]) + list(args[7:]) == plain[4:]
    assert "rows below start[b] are NEVER read" in text and "read when the kernels RUN" in text


def test_null_handle_and_null_arrays_are_errors_not_crashes():
    L = cg.lib()
    assert L.cgpt_llm_score_ragged(None, None, 1, 4, None, None, None, None, 2, 3, 0.1, None, None, 8, None, None) == 1     # CGPT_ERR_INVALID
    assert b"cgpt_llm_score_ragged" in L.cgpt_last_error()
    buf = (C.c_int64 * 64)()
    lens = (C.c_int32 * 2)(2, 3)
    p, lp = C.cast(buf, C.c_void_p), C.cast(lens, C.c_void_p)
    assert L.cgpt_llm_score_ragged(None, p, 1, 4, p, p, p, lp, 2, 3, 0.1, None, None, 8, p, None) == 1                     # null handle
    assert b"cgpt_llm_score_ragged" in L.cgpt_last_error()
    assert L.cgpt_llm_score_ragged(None, p, 1, 4, None, p, p, lp, 2, 3, 0.1, None, None, 8, p, None) == 1                  # null starts_dev
    assert b"starts_dev" in L.cgpt_last_error()
    assert L.cgpt_llm_score_ragged(None, p, 1, 4, p, p, None, lp, 2, 3, 0.1, None, None, 8, p, None) == 1                  # null cand_lens_dev
    assert b"cand_lens_dev" in L.cgpt_last_error()


# ------------------------------------------------------------------------------------------ the classifier off the device
class _NoEngine:
    """Stands where the native engine would: the toy decoder is not one it takes, and there is no device here.  Any use fails."""
    weight_bytes = None
    MAX_CANDS, MAX_TAIL, MAX_LEN = _HipDecoder.MAX_CANDS, _HipDecoder.MAX_TAIL, 512

    def __init__(self, *args, **kw):
        pass

    def __getattr__(self, name):
        raise AssertionError(f"the native engine was asked for {name} off the device")


def test_off_the_device_the_per_row_call_is_the_models_forward_and_is_counted(monkeypatch):
    monkeypatch.setattr(minigpt4, "_HipDecoder", _NoEngine)
    llm = tiny_llama()
    native = _classifier(llm, decode="hip", prefill="hip", ragged="hip", score="hip")
    plain = _classifier(llm)
    x = torch.randn(3, 3, 8, 8, generator=torch.Generator().manual_seed(5))
    emb, _ = plain.encoder.encode_img(x)
    texts = [PROMPT, PROMPT + " now", PROMPT]
    answers = [["red", "dark blue", "a very light grey"], ["pale green", "red", "dark blue"]]          # answers[c][b]
    want = plain.answer_losses_from_embeds(emb, texts, answers)
    got = native.answer_losses_from_embeds(emb, texts, answers)
    assert torch.equal(got, want)
    s = native.decode_stats
    assert s["hf_score_fallbacks"] == 1 and s["hf_score_forwards"] == 2 and s["hip_ragged_scores"] == 0 and s["hip_scores"] == 0
    assert native.multi_select(x, texts, answers, num_cand=[2, 1, 2]) == plain.multi_select(x, texts, answers, num_cand=[2, 1, 2])
    assert native.decode_stats["hf_score_fallbacks"] == 2
    assert plain.decode_stats["hip_ragged_scores"] == 0 and plain.decode_stats["hf_score_fallbacks"] == 0


# ------------------------------------------------------------------------------------------ the constructor's rules
@pytest.mark.parametrize("kw", [dict(ragged="hip"), dict(ragged="hip", decode="graph"), dict(ragged="hip", decode="hip", prefill="model")])
def test_ragged_scoring_needs_the_native_engine_as_before(kw):
    with pytest.raises(ValueError) as e:
        _classifier(tiny_llama(), score="hip", **kw)
    assert 'decode="hip"' in str(e.value) and 'prefill="hip"' in str(e.value)


def test_an_unsupported_decoder_stays_a_value_error_and_defaults_are_unchanged():
    with pytest.raises(ValueError):
        _classifier(tiny_llama(), decode="hip", prefill="hip", ragged="hip", score="hip")
    with pytest.raises(ValueError):
        _classifier(tiny_llama(), score="hip", prompt_bucket=16)
    clf = _classifier(tiny_llama())
    assert (clf.score, clf.ragged, clf.prompt_bucket) == ("hf", "hf", None) and clf.decode_stats["hip_ragged_scores"] == 0
