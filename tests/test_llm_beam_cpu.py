"""Beam search on the native LLaMA engine (beams="hip"), the parts that need no GPU: the law against HF
`generate(num_beams=k)` on a CPU fp32 toy decoder, hand-written selects, the settings check, the classifier's refusals and the
argument checks of the C entries.

The parity chain is law = HF here (CPU, fp32 model) and engine = law in tests/test_gpu_llm_beam.py.

Near-tie exclusion.  `beam_decode_law` evaluates a select in float64 on the model's fp32 logits; HF evaluates it in fp32 (an fp32
log-softmax over 96 columns: about 2 ulp of the log-probability; one more rounding per step for the running sum; the division) on
logits of its cached forward, which differ from the law's cache-free forward by the fp32 model's own summation noise.  Over 6 steps a
score of either side is within about 8 fp32 ulp of the exact one, a compared pair within 16: an image one of whose selects compares
two scores closer than NEAR_ULPS = 16 ulp (`beam_step_law`'s `near`) may legitimately come out differently and is excluded.  That is a
condition: at most 10 % of the images of a case (the seeds below were picked so that the law alone stays within it)."""
import ctypes as C

import pytest
import torch

from certifiedgpt_amd import _lib
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.llm_laws import (BEAM_NEG, _ulp32, beam_decode_law, beam_init_state, beam_keep, beam_length_divisor, beam_step_law,
                                       check_beam_settings)
from certifiedgpt_amd.minigpt4 import MiniGPT4Classifier, prepare_texts
from toy_llm import EOS, PAD, StubEncoder, ToyTokenizer, VOCAB, tiny_llama

NEAR_ULPS = (16.0, 16.0)
PROMPT = prepare_texts(["<Img><ImageHere></Img> what colour is it"])[0]
B, LP, N, HID = 8, 5, 6, 64


def biased_llama(seed, eos_bias):
    """The toy decoder with `eos_bias` added to the EOS logit: > 0 ends hypotheses early, << 0 never."""
    llm = tiny_llama(hidden=HID, seed=seed)
    if eos_bias:
        inner = llm.lm_head.forward

        def fwd(x):
            y = inner(x).clone()
            y[..., EOS] += eos_bias
            return y
        llm.lm_head.forward = fwd
    return llm


def law_and_hf(seed, eos_bias, k, lp, min_new=1):
    llm = biased_llama(seed, eos_bias)
    g = torch.Generator().manual_seed(100 + seed)
    embs = torch.randn(B, LP, HID, generator=g) * 0.5
    table = llm.get_input_embeddings()

    def logits_fn(tokens):                                             # [B, k, i] -> [B, k, V]: the model itself, without a cache
        x = embs[:, None].expand(B, k, LP, HID).reshape(B * k, LP, HID)
        if tokens.shape[2]:
            x = torch.cat([x, table(tokens.reshape(B * k, -1))], dim=1)
        with torch.no_grad():
            return llm(inputs_embeds=x).logits[:, -1].float().view(B, k, -1)

    law = beam_decode_law(logits_fn, B, k, N, min_new, [EOS], PAD, lp, ulps=NEAR_ULPS)
    with torch.no_grad():                                              # min_length as the project passes it (hf_generate_kwargs)
        out = llm.generate(inputs_embeds=embs, attention_mask=torch.ones(B, LP, dtype=torch.long), max_new_tokens=N, num_beams=k,
                           length_penalty=lp, do_sample=False, min_new_tokens=min_new, min_length=0, return_dict_in_generate=True,
                           output_scores=True)
    return law, out


def compare(law, out):
    tokens, scores, near, trace = law
    assert int(near.sum()) <= 0.1 * B, f"{int(near.sum())} of {B} images are near-tied: pick another seed"
    fill = PAD or EOS                                                  # HF: `pad_token_id or eos_token_id[0]`
    for b in range(B):
        if bool(near[b]):
            continue
        row = tokens[b].tolist()
        ln = next((j + 1 for j, t in enumerate(row) if t == EOS), N)   # the hypothesis: through its EOS, or all n tokens
        assert row[ln:] == [PAD] * (N - ln)
        assert out.sequences[b, :ln].tolist() == row[:ln], (b, row, out.sequences[b].tolist())
        assert all(t == fill for t in out.sequences[b, ln:].tolist()), (b, out.sequences[b].tolist())
        d = abs(float(out.sequences_scores[b]) - float(scores[b]))
        assert d <= NEAR_ULPS[0] * float(_ulp32(scores[b])), (b, d, float(scores[b]))
    return trace


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("lp", [1.0, 0.0, 2.0])
def test_law_is_hf_beam_search(k, lp):
    compare(*law_and_hf(0, 0.0, k, lp))


@pytest.mark.parametrize("k", [2, 4])
def test_law_is_hf_when_eos_wins_early_and_the_pool_closes(k):
    law, out = law_and_hf(3, 6.0, k, 1.0)
    trace = compare(law, out)
    assert out.sequences.shape[1] < N                                  # HF left its loop before max_new_tokens ...
    assert not bool(trace[out.sequences.shape[1] - 1]["open"].any())   # ... at the select after which no image of the law is open
    assert bool(trace[-1]["pool_fin"].all())


def test_law_is_hf_when_some_hypotheses_end_and_others_run_on():
    law, out = law_and_hf(5, 2.5, 4, 1.0)
    trace = compare(law, out)
    lens = trace[-1]["pool_len"][:, 0]
    assert int(lens.min()) < N                                         # a winner that ended on an EOS


def test_law_is_hf_when_eos_never_appears():
    law, out = law_and_hf(2, -30.0, 4, 1.0)
    trace = compare(law, out)
    assert out.sequences.shape[1] == N and not bool((law[0] == EOS).any())
    for t in trace[:-1]:                                               # nothing finishes before the max-length select
        assert not bool(t["pool_fin"].any()) and bool(t["open"].all())
    assert bool(trace[-1]["pool_fin"].all()) and bool((trace[-1]["pool_len"] == N).all())


# ---- hand-written selects
def state(running, n=4, **kw):
    k = len(running)
    s = beam_init_state(1, k, n, PAD)
    s["running"] = torch.tensor([running], dtype=torch.float64)
    for key, val in kw.items():
        s[key] = val
    return s


def test_ties_go_to_the_lowest_flat_index():
    row = [0.0, 0.0, 3.0, 3.0, 1.0, 3.0, 0.0, 0.0]                     # three equal maxima in every beam
    out = beam_step_law(state([-1.0, -1.0]), torch.tensor([[row, row]]), 1, 4, 0, [7], PAD)
    # K = 4: beam 0's columns 2, 3, 5 come before beam 1's column 2 (flat indices 2, 3, 5, 10)
    assert out["parents"][0].tolist() == [0, 0] and out["next_tokens"][0].tolist() == [2, 3]
    assert not bool(out["near"][0])                                    # exact ties are decided by the index, not by rounding
    flipped = beam_step_law(state([-1.0, -0.5]), torch.tensor([[row, row]]), 1, 4, 0, [7], PAD)
    assert flipped["parents"][0].tolist() == [1, 1] and flipped["next_tokens"][0].tolist() == [2, 3]


def test_step_0_reads_beam_0_alone():
    rows = torch.tensor([[[0.0, 1.0, 2.0, 3.0, 4.0, 5.0], [50.0, 40.0, 0.0, 0.0, 0.0, 0.0]]])
    s = beam_init_state(1, 2, 3, PAD)
    assert s["running"].tolist() == [[0.0, BEAM_NEG]]
    out = beam_step_law(s, rows, 0, 3, 0, [0], PAD)
    assert out["parents"][0].tolist() == [0, 0] and out["next_tokens"][0].tolist() == [5, 4]
    lse = torch.logsumexp(rows[0, 0].double(), 0)
    assert out["running"][0].tolist() == [float(5.0 - lse), float(4.0 - lse)]
    assert out["tokens"][0, :, 0].tolist() == [5, 4] and bool(out["open"][0]) and not bool(out["pool_fin"].any())


def test_eos_is_suppressed_below_min_new_and_enters_the_pool_after_it():
    rows = torch.tensor([[[9.0, 1.0, 2.0, 3.0, 0.0, 0.0], [0.0] * 6]])
    masked = beam_step_law(beam_init_state(1, 2, 3, PAD), rows, 0, 3, 1, [0], PAD)
    assert masked["next_tokens"][0].tolist() == [3, 2] and not bool(masked["pool_fin"].any())
    lse = torch.logsumexp(rows[0, 0].double(), 0)                      # the normaliser keeps the EOS mass
    assert masked["running"][0, 0] == 3.0 - lse
    free = beam_step_law(beam_init_state(1, 2, 3, PAD), rows, 0, 3, 0, [0], PAD, length_penalty=2.0)
    assert free["next_tokens"][0].tolist() == [3, 2]                   # rank 0 is the EOS: it finishes, the next two run on
    assert free["pool_fin"][0].tolist() == [True, False] and free["pool_len"][0].tolist() == [1, 0]
    assert free["pool_seq"][0, 0].tolist() == [0, PAD, PAD]
    assert free["pool_score"][0, 0] == (9.0 - lse) / beam_length_divisor(0, 2.0)
    assert bool(free["open"][0])                                       # one of two slots finished: worst = -1e9
    # the last select finishes everything
    last = beam_step_law(state([-1.0, -2.0], n=2), rows.expand(1, 2, 6).clone(), 1, 2, 0, [0], PAD)
    assert last["pool_fin"][0].tolist() == [True, True] and last["pool_len"][0].tolist() == [2, 2]


def test_pool_takes_an_entrant_and_freezes_once_closed():
    rows = torch.zeros(1, 2, 6)
    rows[0, :, 0] = 20.0                                               # both beams put (almost) all mass on the EOS, id 0
    s = state([-1.0, -1.5], pool_score=torch.tensor([[-0.25, BEAM_NEG]], dtype=torch.float64),
              pool_fin=torch.tensor([[True, False]]), pool_len=torch.tensor([[1, 0]]))
    out = beam_step_law(s, rows, 1, 4, 0, [0], PAD)
    assert out["pool_score"][0, 0] == -0.25 and out["pool_len"][0].tolist() == [1, 2]      # the entrant (-0.5) takes the free slot
    assert not bool(out["open"][0])                                    # running'[0] / 2 is far below the worst finished score
    frozen = beam_step_law(out, rows, 2, 4, 0, [0], PAD)
    for key in ("pool_score", "pool_fin", "pool_len", "pool_seq"):
        assert torch.equal(frozen[key], out[key])
    assert not bool(frozen["open"][0])


def test_keep_and_divisor():
    assert [beam_keep(4, e) for e in (0, 1, 2, 8)] == [8, 8, 12, 36] and beam_keep(8, 8) == 72
    assert beam_length_divisor(2, 1.0) == 3.0 and beam_length_divisor(5, 0.0) == 1.0
    assert beam_length_divisor(2, 0.5) == float(torch.tensor(3.0 ** 0.5, dtype=torch.float64).float())


@pytest.mark.parametrize("kw, field", [
    ({"num_beams": 1}, "num_beams"), ({"num_beams": 9}, "num_beams"), ({"num_beams": 2.0}, "num_beams"), ({"num_beams": True}, "num_beams"),
    ({"length_penalty": float("inf")}, "length_penalty"), ({"length_penalty": float("nan")}, "length_penalty"),
    ({"early_stopping": True}, "early_stopping"), ({"early_stopping": "never"}, "early_stopping"),
    ({"num_return_sequences": 2}, "num_return_sequences"), ({"num_beam_groups": 2}, "num_beam_groups"), ({"do_sample": True}, "do_sample"),
    ({"repetition_penalty": 1.05}, "repetition_penalty")])
def test_settings_check_names_the_field(kw, field):
    args = {"num_beams": 4, **kw}
    with pytest.raises(ValueError, match=field + "="):
        check_beam_settings(**args)


def test_settings_check_accepts_the_supported_range():
    assert check_beam_settings(2) == (2, 1.0) and check_beam_settings(8, 0) == (8, 0.0) and check_beam_settings(4, -0.5) == (4, -0.5)
    assert check_beam_settings(4, None, False, 1, 1, False, 1) == (4, 1.0)


# ---- the classifier
def toy(**kw):
    return MiniGPT4Classifier(StubEncoder(hidden=HID), tiny_llama(hidden=HID), ToyTokenizer(), PROMPT, AnswerLabelMap(4, ["red", "blue"]), **kw)


NATIVE = {"beams": "hip", "decode": "hip", "prefill": "hip"}


@pytest.mark.parametrize("kw, word", [
    ({"beams": "hip"}, 'decode="hip"'), ({"beams": "hip", "decode": "graph"}, 'decode="hip"'),
    ({"beams": "hip", "decode": "hip"}, 'prefill="hip"'),
    ({**NATIVE, "grouped_kv": True}, "grouped_kv"), ({**NATIVE, "ragged": "hip"}, "ragged"),
    ({**NATIVE, "ragged": "hip", "prompt_bucket": 8}, "prompt_bucket"), ({**NATIVE, "early_stop": True}, "early_stop"),
    ({**NATIVE, "stop_words_ids": [[5, 6]]}, "stop_words_ids"),
    ({**NATIVE, "sample": "hip", "generate_kwargs": {"do_sample": True}}, "do_sample")])
def test_classifier_refuses_what_is_out_of_scope(kw, word):
    with pytest.raises(ValueError, match="beams=\"hip\" needs") as e:
        toy(**kw)
    assert word in str(e.value)


def test_classifier_names_all_failing_combinations_together():
    with pytest.raises(ValueError) as e:
        toy(beams="hip", decode="hip", prefill="hip", grouped_kv=True, ragged="hip", prompt_bucket=4, early_stop=True, stop_words_ids=[[5]],
            sample="hip", generate_kwargs={"do_sample": True, "num_beams": 4})
    for word in ("grouped_kv", "ragged", "prompt_bucket", "early_stop", "stop_words_ids", "do_sample"):
        assert word in str(e.value), word
    with pytest.raises(ValueError, match="beams="):
        toy(beams="native")


def test_default_switch_leaves_beam_calls_with_hf():
    clf = toy(generate_kwargs={"num_beams": 4, "length_penalty": 2.0})
    assert clf.beams == "hf" and clf.decode_stats["hip_beam"] == 0 and clf._beam_settings() is None and not clf._greedy_defaults()
    answers = clf.generate(torch.rand(2, 3, 8, 8), PROMPT)
    assert len(answers) == 2 and clf.decode_stats["hf_calls"] == 1
    with pytest.raises(RuntimeError, match="last_beam_scores"):
        clf.last_beam_scores()


def native_stub(gen_fields, **generate_kwargs):
    """A classifier as beams="hip" leaves it, without an engine (none can be created off the device): the two methods under test read
    the switch, the call's arguments and the checkpoint's generation_config, nothing else."""
    clf = toy(generate_kwargs=generate_kwargs)
    clf.beams = "hip"
    for key, val in gen_fields.items():
        setattr(clf.llama_model.generation_config, key, val)
    return clf


def test_beam_fields_resolve_as_generate_resolves_them():
    """The call's argument, else the checkpoint's generation_config, else the default: what the checkpoint sets and the call leaves
    open either reaches the engine (length_penalty, num_beams) or sends the call to HF generate (everything else)."""
    assert native_stub({}, num_beams=4)._beam_settings() == (4, 1.0)                     # the reference's own length_penalty=1
    assert native_stub({"length_penalty": 2.0}, num_beams=4)._beam_settings() == (4, 1.0)   # ... is an argument of the call: it wins
    clf = native_stub({"length_penalty": 2.0}, num_beams=4, length_penalty=None)          # a call that is silent on it
    assert clf._beam_settings() == (4, 2.0) and clf._greedy_defaults()
    clf = native_stub({"num_beams": 3, "length_penalty": 0.5}, num_beams=None, length_penalty=None)
    assert clf._beam_settings() == (3, 0.5) and clf._greedy_defaults()
    for fields in ({"early_stopping": True}, {"early_stopping": "never"}, {"num_return_sequences": 2}, {"num_beam_groups": 2},
                   {"length_penalty": 2.0, "early_stopping": True, "num_return_sequences": 2}):
        clf = native_stub(fields, num_beams=4)
        assert clf._beam_settings() is None and not clf._greedy_defaults(), fields
    for kw in ({"early_stopping": True}, {"num_return_sequences": 2}):                    # set by the call: not a greedy argument either
        clf = native_stub({}, num_beams=4, **kw)
        assert clf._beam_settings() is None and not clf._greedy_defaults(), kw
    one = native_stub({"early_stopping": True}, num_beams=1)                              # one beam: HF ignores the field, the greedy loop runs
    assert one._beam_settings() is None and one._greedy_defaults()


def test_agent_passes_the_beam_keys_through(monkeypatch):
    import certifiedgpt_amd.minigpt4 as m
    from certifiedgpt_amd.agents import minigpt4_certify_agent as agent
    seen = {}

    class Probe:
        def __init__(self, *a, **kw):
            seen.update(kw)

    monkeypatch.setattr(m, "MiniGPT4Classifier", Probe)

    class E:
        max_batch, device = 4, torch.device("cpu")

    agent.build_generating_classifier(E(), {"answers": ["red", "blue"], "beams": "hip", "num_beams": 4, "length_penalty": 0.5,
                                            "decode": "hip", "prefill": "hip"}, 3, ToyTokenizer(), tiny_llama())
    assert seen["beams"] == "hip" and seen["generate_kwargs"] == {"num_beams": 4, "length_penalty": 0.5}
    agent.build_generating_classifier(E(), {"answers": ["red", "blue"]}, 3, ToyTokenizer(), tiny_llama())
    assert seen["beams"] == "hf"


# ---- the C entries, without a device: every refusal comes before the first launch
def test_entries_refuse_null_and_out_of_range_arguments():
    L = _lib.lib()
    one = C.c_void_p(8)
    st = [one] * 8
    assert L.cgpt_llm_beam_reserve(None, 4, 4, 6) == 1 and b"cgpt_llm_beam_reserve" in L.cgpt_last_error()
    assert L.cgpt_llm_beam_step(None, one, 1, 4, 7, 0, one, 6, one, one, 8, one, one, 8, one, None) == 1
    assert b"cgpt_llm_beam_step" in L.cgpt_last_error()
    assert L.cgpt_llm_beam(None, one, 1, 4, 7, 6, 1, None, 0, 0, 1.0, one, one, 8, one, one, 8, one, None, None, None, None) == 1
    assert b"cgpt_llm_beam" in L.cgpt_last_error()
    eos = (C.c_int64 * 1)(2)

    def select(logits=one, ld=320, B=1, k=4, V=320, step=0, n=6, min_new=1, num_eos=1, lp=1.0, last=one):
        return L.cgpt_llm_beam_select_logits(logits, ld, B, k, V, step, n, min_new, eos, num_eos, 0, lp, *st, *st, one, last, None)

    for kw, word in (({"logits": None}, b"null"), ({"last": None}, b"null"), ({"k": 1}, b"num_beams 1"), ({"k": 9}, b"num_beams 9"),
                     ({"V": 8, "ld": 8}, b"K + num_eos <= V"), ({"ld": 300}, b"ld >= V"), ({"V": 131073, "ld": 131073}, b"131072"),
                     ({"step": 6}, b"step < num_new"), ({"step": -1}, b"step"), ({"B": 0}, b"B >= 1"), ({"num_eos": 9}, b"8 EOS"),
                     ({"lp": float("nan")}, b"length_penalty"), ({"lp": float("inf")}, b"length_penalty")):
        assert select(**kw) == 1, kw
        msg = L.cgpt_last_error()
        assert b"cgpt_llm_beam_select_logits" in msg and word in msg, (kw, msg)
