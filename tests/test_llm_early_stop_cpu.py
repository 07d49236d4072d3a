"""early_stop without a GPU: the classifier's keyword validation (it runs before any device work), the graph cache key, the agent's
pass-through, the C-ABI's argument checks, and the rule that says how many token steps of a greedy call run -- stated here in plain
Python and used by tests/test_gpu_llm_early_stop.py as the expectation for cgpt_llm_live_steps.

The rule: a greedy call of n selects runs step i + 1 after select i while some row is unfinished.  Row b finishes at the first column
of its token row that holds an EOS id.  With F = max over rows of that column (n for a row without an EOS), the steps that run are
min(F, n - 1): select F is the first at which no row is left, and the last select is followed by no step anyway."""
import inspect
import types

import pytest
import torch

import certifiedgpt_amd as cg
from certifiedgpt_amd.agents import minigpt4_certify_agent as agent
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import MiniGPT4Classifier, WordHashTokenizer


def finishing_select(tokens, eos_ids):
    """F of the module docstring for a [B, n] token table (tensor or nested lists)."""
    rows = tokens.tolist() if hasattr(tokens, "tolist") else tokens
    eos = set(int(e) for e in eos_ids)
    F = 0
    for row in rows:
        first = next((i for i, t in enumerate(row) if int(t) in eos), len(row))
        F = max(F, first)
    return F


def expected_live_steps(tokens, eos_ids):
    rows = tokens.tolist() if hasattr(tokens, "tolist") else tokens
    return min(finishing_select(rows, eos_ids), len(rows[0]) - 1)


def test_the_rule_on_hand_written_tables():
    E, P = 2, 0
    no_eos = [[5, 6, 7, 8], [9, 9, 9, 9]]
    assert finishing_select(no_eos, [E]) == 4 and expected_live_steps(no_eos, [E]) == 3          # every step runs
    at_once = [[E, P, P, P], [E, P, P, P], [E, P, P, P]]
    assert finishing_select(at_once, [E]) == 0 and expected_live_steps(at_once, [E]) == 0        # no step runs
    staggered = [[5, E, P, P, P, P], [5, 6, 7, E, P, P], [E, P, P, P, P, P]]
    assert finishing_select(staggered, [E]) == 3 and expected_live_steps(staggered, [E]) == 3    # the slowest row decides
    one_left = [[E, P, P, P], [5, 6, 7, 8]]
    assert expected_live_steps(one_left, [E]) == 3                                               # one unfinished row keeps all alive
    last_col = [[5, 6, 7, E]]
    assert finishing_select(last_col, [E]) == 3 and expected_live_steps(last_col, [E]) == 3      # EOS at the last select: nothing to skip
    two_ids = [[5, 11, P, P], [E, P, P, P]]
    assert expected_live_steps(two_ids, [E, 11]) == 1 and expected_live_steps(two_ids, [E]) == 3
    assert expected_live_steps(two_ids, []) == 3                                                 # no EOS id: nothing ever stops
    assert expected_live_steps(torch.tensor(staggered), [E]) == 3                                # tensors as well
    assert expected_live_steps([[E]], [E]) == 0                                                  # one select, no step at all


def _clf(**kw):
    return MiniGPT4Classifier(None, object(), WordHashTokenizer(96), "<ImageHere>", AnswerLabelMap(4, ()), max_batch=4, **kw)


@pytest.mark.parametrize("kw", [dict(decode="hf"), dict(decode="graph"), dict()])
def test_early_stop_needs_the_native_engine(kw):
    with pytest.raises(ValueError) as e:
        _clf(early_stop=True, **kw)
    assert "early_stop" in str(e.value) and "decode" in str(e.value), str(e.value)


def test_early_stop_is_a_bool():
    for bad in (1, "on", None):
        with pytest.raises(ValueError) as e:
            _clf(early_stop=bad, decode="hip")
        assert "early_stop" in str(e.value)


def test_default_is_off_and_last_live_steps_raises_without_a_native_decode():
    clf = _clf()
    assert clf.early_stop is False
    assert inspect.signature(MiniGPT4Classifier.__init__).parameters["early_stop"].default is False
    with pytest.raises(RuntimeError):
        clf.last_live_steps()


def test_graph_key_is_unchanged_when_off_and_differs_when_on():
    clf = _clf()
    embs = types.SimpleNamespace(shape=(4, 12, 512), dtype=torch.float16, device=types.SimpleNamespace(index=0))
    plain, ragged = clf._graph_key(embs), clf._graph_key(embs, ragged=True)
    assert plain == (4, 12, torch.float16, 0, 20, False, "hf", "model")                          # the key as it was before the keyword
    assert ragged == plain + ("ragged",)
    clf.early_stop = True                                                                        # what the constructor sets with decode="hip"
    assert clf._graph_key(embs) == plain + ("early_stop",) and clf._graph_key(embs, ragged=True) == ragged + ("early_stop",)
    assert len({plain, ragged, clf._graph_key(embs), clf._graph_key(embs, ragged=True)}) == 4


def test_agents_pass_the_key_through(monkeypatch):
    src = inspect.getsource(agent)
    assert "early_stop: false | true" in agent.__doc__ and 'gen_cfg.get("early_stop", False)' in src
    seen = {}

    class Spy:
        def __init__(self, *a, **kw):
            seen.update(kw)

    import certifiedgpt_amd.minigpt4 as m
    monkeypatch.setattr(m, "MiniGPT4Classifier", Spy)
    enc = types.SimpleNamespace(max_batch=4, device="cpu")
    llm = types.SimpleNamespace(parameters=lambda: [])
    base = {"prompt": "<ImageHere>", "answers": ["a", "b"], "decode": "hip"}
    agent.build_generating_classifier(enc, dict(base, early_stop=True), 4, tokenizer=object(), llama_model=llm)
    assert seen["early_stop"] is True and seen["decode"] == "hip"
    agent.build_generating_classifier(enc, base, 4, tokenizer=object(), llama_model=llm)
    assert seen["early_stop"] is False
    from certifiedgpt_amd.agents.minigpt4_predict_agent import MiniGPT4PredictAgent
    assert issubclass(MiniGPT4PredictAgent, agent.MiniGPT4CertifyAgent)                          # the predict agent builds through the same code


def test_entries_refuse_bad_arguments_without_a_device():
    import ctypes as C
    L = cg.lib()
    assert L.cgpt_llm_set_early_stop(None, 1) == 1 and b"cgpt_llm_set_early_stop" in L.cgpt_last_error()
    n = C.c_int32(7)
    assert L.cgpt_llm_live_steps(None, C.byref(n), None) == 1 and b"cgpt_llm_live_steps" in L.cgpt_last_error()
    assert n.value == 7
