"""`multi_select` answer scoring without a GPU: the loss law against a restatement of the reference's `forward(..., reduction='none')`
written out here (minigpt_base.py:320-363, :451-467; modeling_llama.py:101-123), the keyword rules, classify="multi_select" on the
CPU, the two cgpt_llm_score* entries (declared, bound with the declared signature, null arguments refused), the agent keys."""
import ctypes as C
import os
import re

import pytest
import torch

import certifiedgpt_amd as cg
from certifiedgpt_amd import _lib
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import IMAGE_PLACEHOLDER, MiniGPT4Classifier, prepare_texts
from toy_llm import BOS, StubEncoder, ToyTokenizer, tiny_llama

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPT = prepare_texts(["<Img><ImageHere></Img> what is this"])[0]
SCORE_ENTRIES = ["cgpt_llm_score_reserve", "cgpt_llm_score"]
CANDS = ["red", "dark blue", "pale green", "a very light grey"]        # 1, 2, 2 and 4 words = tokens (the toy tokenizer splits on blanks)

_CTYPES = {"cgpt_llm_handle": C.c_void_p, "const void*": C.c_void_p, "void*": C.c_void_p, "void* const*": C.c_void_p,
           "float*": C.c_void_p, "const float*": C.c_void_p, "const int64_t*": C.c_void_p, "const int32_t*": C.c_void_p,
           "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}


def _classifier(llm, classes=6, vocabulary=(), **kw):
    return MiniGPT4Classifier(StubEncoder(), llm, ToyTokenizer(), PROMPT, AnswerLabelMap(classes, vocabulary), max_new_tokens=3, **kw)


def _images(rows=3, seed=5):
    return torch.randn(rows, 3, 8, 8, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------ the reference's law, restated
def _reference_losses(llm, tok, img_embeds, prompt, answers, end_sym="\n"):
    """`multi_select`'s all_losses for a shared prompt and ONE answer per candidate: a full-sequence forward per candidate."""
    B = img_embeds.shape[0]
    emb = llm.get_input_embeddings()
    before, after = prompt.split(IMAGE_PLACEHOLDER)
    ids = lambda text: tok(text, return_tensors="pt", add_special_tokens=False).input_ids      # noqa: E731
    cond = torch.cat([emb(torch.tensor([[BOS]])).expand(B, -1, -1), emb(ids(before)).expand(B, -1, -1), img_embeds,
                      emb(ids(after)).expand(B, -1, -1)], dim=1)
    out = []
    for a in answers:
        regress = ids(a + end_sym)
        inputs = torch.cat([cond, emb(regress).expand(B, -1, -1)], dim=1)
        targets = torch.full(inputs.shape[:2], -100, dtype=torch.long)
        targets[:, cond.shape[1]:] = regress
        with torch.no_grad():
            logits = llm(inputs_embeds=inputs, attention_mask=torch.ones(inputs.shape[:2], dtype=torch.int)).logits.float()
        shift_logits, shift_labels = logits[..., :-1, :].contiguous(), targets[..., 1:].contiguous()
        loss = torch.nn.CrossEntropyLoss(reduction="none", label_smoothing=0.1)(shift_logits.view(-1, logits.shape[-1]), shift_labels.view(-1))
        out.append(loss.view(B, -1).mean(1).reshape(-1, 1))
    return torch.cat(out, dim=-1)


@pytest.fixture(scope="module")
def law():
    llm = tiny_llama()
    clf = _classifier(llm)
    x = _images()
    emb, _ = clf.encoder.encode_img(x)
    return llm, clf, x, emb, _reference_losses(llm, ToyTokenizer(), emb, PROMPT, CANDS)


def test_losses_and_ranks_are_the_references(law):
    _, clf, x, emb, want = law
    assert [len(c.split()) for c in CANDS] == [1, 2, 2, 4]
    got = clf.answer_losses_from_embeds(emb, PROMPT, CANDS)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 4)
    torch.testing.assert_close(got, want)
    per_row = clf.answer_losses_from_embeds(emb, [PROMPT] * 3, [[c] * 3 for c in CANDS])    # the reference's own argument shapes
    torch.testing.assert_close(per_row, want)
    assert clf.multi_select(x, [PROMPT] * 3, [[c] * 3 for c in CANDS]) == torch.argsort(want, dim=-1).tolist()


def test_num_cand_puts_9999_where_the_reference_does(law):
    _, clf, x, _, want = law
    num_cand = [4, 2, 1]
    masked = want.clone()
    for i in range(3):
        masked[i, num_cand[i]:] = 9999
    ranks = clf.multi_select(x, PROMPT, CANDS, num_cand=num_cand)
    assert ranks == torch.argsort(masked, dim=-1).tolist()
    assert ranks[2][0] == 0 and set(ranks[1][:2]) == {0, 1}            # the live candidates come first


def test_answers_of_different_lengths_in_one_call_share_the_longest_answers_divisor(law):
    llm, clf, _, emb, _ = law
    tok = ToyTokenizer()
    mixed = [["red", "dark blue", "a very light grey"], ["pale green", "red", "dark blue"]]      # answers[c][b]
    got = clf.answer_losses_from_embeds(emb, PROMPT, mixed)
    for c, cand in enumerate(mixed):
        Tmax = max(len(a.split()) for a in cand)
        for b, a in enumerate(cand):
            alone = _reference_losses(llm, tok, emb[b:b + 1], PROMPT, [a])[0, 0]     # divided by L + T - 1
            L = 1 + len(PROMPT.replace(IMAGE_PLACEHOLDER, " ").split()) + emb.shape[1]
            T = len(a.split())
            torch.testing.assert_close(got[b, c], alone * (L + T - 1) / (L + Tmax - 1))


def test_rows_with_different_texts_are_scored_as_each_row_alone_up_to_the_divisor(law):
    llm, clf, _, emb, _ = law
    tok = ToyTokenizer()
    texts = [PROMPT, PROMPT + " now", PROMPT + " right now please"]
    got = clf.answer_losses_from_embeds(emb, texts, CANDS[:2])
    lens = [1 + len(t.replace(IMAGE_PLACEHOLDER, " ").split()) + emb.shape[1] for t in texts]
    for b, t in enumerate(texts):
        alone = _reference_losses(llm, tok, emb[b:b + 1], t, CANDS[:2])[0]
        for c, a in enumerate(CANDS[:2]):
            T = len(a.split())
            torch.testing.assert_close(got[b, c], alone[c] * (lens[b] + T - 1) / (max(lens) + T - 1))


def test_end_sym_is_part_of_the_answer(law):
    llm, _, _, emb, _ = law
    clf = _classifier(llm, end_sym=" ###")
    want = _reference_losses(llm, ToyTokenizer(), emb, PROMPT, CANDS, end_sym=" ###")
    torch.testing.assert_close(clf.answer_losses_from_embeds(emb, PROMPT, CANDS), want)


# ------------------------------------------------------------------------------------------ the keywords
@pytest.mark.parametrize("kw", [dict(), dict(decode="graph"), dict(decode="hf", prefill="model")])
def test_score_hip_without_the_native_engine_is_a_value_error(kw):
    with pytest.raises(ValueError) as e:
        _classifier(tiny_llama(), score="hip", **kw)
    assert 'decode="hip"' in str(e.value) and 'prefill="hip"' in str(e.value)


def test_score_hip_on_an_unsupported_decoder_is_a_value_error_never_another_engine():
    with pytest.raises(ValueError):
        _classifier(tiny_llama(), decode="hip", prefill="hip", score="hip")


def test_unknown_values_are_refused():
    with pytest.raises(ValueError):
        _classifier(tiny_llama(), score="native")
    with pytest.raises(ValueError):
        _classifier(tiny_llama(), classify="rank")
    with pytest.raises(ValueError):
        _classifier(tiny_llama(), label_smoothing=1.0)
    with pytest.raises(ValueError):
        _classifier(tiny_llama(), candidates=["a", "b"])               # candidates without classify="multi_select"


@pytest.mark.parametrize("cands", [[], ["red"], ["c%d" % i for i in range(6)]])
def test_multi_select_needs_two_to_num_classes_minus_one_candidates(cands):
    with pytest.raises(ValueError) as e:
        _classifier(tiny_llama(), classes=6, classify="multi_select", candidates=cands)
    assert "num_classes - 1" in str(e.value)
    if len(cands) < 2:                                                 # the label map's answers by default (it never holds too many)
        with pytest.raises(ValueError):
            _classifier(tiny_llama(), classes=6, vocabulary=cands, classify="multi_select")


def test_defaults_keep_the_generating_classifier():
    clf = _classifier(tiny_llama())
    assert (clf.score, clf.classify, clf.candidates, clf.end_sym, clf.label_smoothing) == ("hf", "generate", None, "\n", 0.1)
    s = clf.decode_stats
    assert s["hf_score_forwards"] == 0 and s["hip_scores"] == 0 and s["hf_score_fallbacks"] == 0
    logits = clf(_images())
    assert clf.decode_stats["hf_calls"] == 1 and clf.decode_stats["hf_score_forwards"] == 0
    assert bool(((logits == 0) | (logits == 1)).all()) and bool((logits.sum(dim=1) == 1).all())      # one-hot, as before


# ------------------------------------------------------------------------------------------ classify="multi_select" on the CPU
def test_classify_multi_select_returns_minus_loss_columns_and_never_the_other_class(law):
    llm, _, x, emb, want = law
    clf = _classifier(llm, classes=6, classify="multi_select", candidates=CANDS)
    logits = clf(x)
    assert tuple(logits.shape) == (3, 6) and clf.decode_stats["hf_score_forwards"] == 4 and clf.decode_stats["hf_calls"] == 0
    torch.testing.assert_close(logits[:, :4], -want)
    assert bool(torch.isneginf(logits[:, 4:]).all()) and clf.label_map.other_id == 5
    ranks = clf.multi_select(x, PROMPT, CANDS)
    assert logits.argmax(dim=1).tolist() == [r[0] for r in ranks]
    assert clf.last_answers == [CANDS[r[0]] for r in ranks]
    assert clf.decode_stats["hf_score_forwards"] == 8
    by_vocab = _classifier(llm, classes=5, vocabulary=CANDS, classify="multi_select")       # candidates default to the label map's answers
    assert by_vocab.candidates == by_vocab.label_map.answers and len(by_vocab.candidates) == 4
    assert tuple(by_vocab(x).shape) == (3, 5)


# ------------------------------------------------------------------------------------------ the C-ABI
def test_header_declares_and_binding_matches_the_score_entries():
    text = open(os.path.join(ROOT, "include", "cgpt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = cg.lib()
    for name in SCORE_ENTRIES:
        m = re.search(r"cgpt_status\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, f"cgpt.h does not declare {name}"
        assert hasattr(L, name), f"libcgpt.so does not export {name}"
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        types = [re.sub(r"\s*\b[A-Za-z_0-9]+$", "", p).replace(" *", "*") for p in params]      # drop the parameter name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int32
        assert [_CTYPES[t] for t in types] == list(args), (name, types)
    assert "WRITES NO CACHE ROW" in text and "minigpt_base.py:451-467" in text


def test_score_takes_the_cache_arguments_of_the_step_entry():
    step, score = _lib.SIGNATURES["cgpt_llm_step"][1], _lib.SIGNATURES["cgpt_llm_score"][1]
    assert list(step[4:7]) == list(score[9:12])                        # K table, V table, stride


def test_null_handle_and_null_arguments_are_errors_not_crashes():
    L = cg.lib()
    assert L.cgpt_llm_score_reserve(None, 200, 16) == 1                # CGPT_ERR_INVALID
    assert b"cgpt_llm_score_reserve" in L.cgpt_last_error()
    assert L.cgpt_llm_score(None, None, 1, 4, None, None, 2, 3, 0.1, None, None, 8, None, None) == 1
    assert b"cgpt_llm_score" in L.cgpt_last_error()
    buf = (C.c_int64 * 64)()
    lens = (C.c_int32 * 2)(2, 3)
    p = C.cast(buf, C.c_void_p)
    assert L.cgpt_llm_score(None, p, 1, 4, p, C.cast(lens, C.c_void_p), 2, 3, 0.1, None, None, 8, p, None) == 1


# ------------------------------------------------------------------------------------------ the agent
def test_agent_documents_and_forwards_the_scoring_keys(monkeypatch):
    import inspect
    from certifiedgpt_amd.agents import minigpt4_certify_agent as agent
    src = inspect.getsource(agent)
    assert 'classify: "generate" | "multi_select"' in src and 'score: "hf" | "hip"' in src and "end_sym:" in src
    assert 'gen_cfg.get("classify", "generate")' in src and 'gen_cfg.get("score", "hf")' in src and 'gen_cfg.get("end_sym", "\\n")' in src
    seen = {}

    class Recorder:
        def __init__(self, *args, **kw):
            seen.update(kw)

    import certifiedgpt_amd.minigpt4 as minigpt4
    monkeypatch.setattr(minigpt4, "MiniGPT4Classifier", Recorder)
    gen = {"prompt": PROMPT, "answers": ["a", "b", "c"], "decode": "hip", "prefill": "hip", "classify": "multi_select", "score": "hip",
           "end_sym": "###"}
    agent.build_generating_classifier(StubEncoder(), gen, 4, tokenizer=ToyTokenizer(), llama_model=tiny_llama())
    assert (seen["classify"], seen["score"], seen["end_sym"]) == ("multi_select", "hip", "###")
    seen.clear()
    for key in ("classify", "score", "end_sym"):
        del gen[key]
    agent.build_generating_classifier(StubEncoder(), gen, 4, tokenizer=ToyTokenizer(), llama_model=tiny_llama())
    assert (seen["classify"], seen["score"], seen["end_sym"]) == ("generate", "hf", "\n")
