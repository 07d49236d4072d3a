"""Trie-constrained answer decoding (classify="constrained") without a GPU: the trie builder, the library's host
validator (cgpt_llm_trie_check needs no device), the select law against a brute-force loop, and constrain="hf" end to end on the toy
decoder."""
import ctypes as C
import random

import pytest
import torch

import certifiedgpt_amd.minigpt4 as m
from certifiedgpt_amd import _lib
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.llm_laws import (allowed_tokens_fn, build_answer_trie, constrained_decode_law, constrained_select_law,
                                       trie_walk)
from certifiedgpt_amd.minigpt4 import MiniGPT4Classifier, prepare_texts
from toy_llm import PAD, StubEncoder, ToyTokenizer, VOCAB, tiny_llama

PROMPT = prepare_texts(["<Img><ImageHere></Img> what is this"])[0]
# prefixes of length 0, 1 and 2 are shared: (5 7) | (5 3 9) | (2) | (5 3 4) | (8 1)
FIVE = [(5, 7), (5, 3, 9), (2,), (5, 3, 4), (8, 1)]
# by hand: root -2-> n1 (class 2), -5-> n2, -8-> n3;  n2 -3-> n4, -7-> n5 (class 0);  n3 -1-> n6 (class 4);  n4 -4-> n7 (class 3), -9-> n8 (class 1)
FIVE_TABLES = ([0, 3, 3, 5, 6, 8, 8, 8, 8, 8], [2, 5, 8, 3, 7, 1, 4, 9], [1, 2, 3, 4, 5, 6, 7, 8], [-1, 2, -1, -1, -1, 0, 4, 3, 1])


def tables(trie):
    return [t.tolist() for t in trie.tables()]


def test_trie_of_five_candidates_is_the_hand_written_csr():
    trie = build_answer_trie(FIVE, 16)
    assert tables(trie) == [list(t) for t in FIVE_TABLES] and trie.depth == 3
    assert all(t.dtype == torch.int32 and t.device.type == "cpu" for t in trie.tables())
    assert trie.nodes == 9 and trie.edges == 8
    assert trie_walk([list(s) + [0] * (3 - len(s)) for s in FIVE], trie) == [0, 1, 2, 3, 4]
    assert trie_walk([[5, 3, 0], [7, 0, 0], [5, 0, 0]], trie) == [-1, -1, -1]


def test_trie_tables_follow_the_tokens_and_classes_follow_the_input_order():
    rng = random.Random(3)
    want = tables(build_answer_trie(FIVE, 16))
    for _ in range(6):
        perm = list(range(5))
        rng.shuffle(perm)
        got = tables(build_answer_trie([FIVE[p] for p in perm], 16))
        assert got[:3] == want[:3]
        # leaf n holds candidate FIVE[want] = the permuted list's entry at position got
        assert [perm[c] if c >= 0 else -1 for c in got[3]] == want[3]
    assert tables(build_answer_trie([torch.tensor(s) for s in FIVE], 16)) == want


@pytest.mark.parametrize("seqs, vocab, names, word", [
    ([(1, 2), ()], 8, None, "#1"),                                     # an empty sequence
    ([(1, 2), (1, 8)], 8, None, "#1"),                                 # a token outside the vocabulary
    ([(1, 2), (-1,)], 8, None, "#1"),
    ([(1, 2), (3,), (1, 2)], 8, ["a", "b", "c"], "'c'"),               # two equal sequences
    ([(1, 2, 3), (4,), (1, 2)], 8, ["long", "x", "short"], "'short'"), # a proper prefix of another
    ([(1, 2)], 8, None, "2 candidates"),                               # fewer than 2 candidates
    ([tuple(range(33)), (40,)], 64, None, "#0"),                       # depth over 32
])
def test_trie_builder_refusals_name_the_candidates(seqs, vocab, names, word):
    with pytest.raises(ValueError) as e:
        build_answer_trie(seqs, vocab, names=names)
    assert word in str(e.value), str(e.value)


def test_trie_builder_refuses_more_than_2_to_the_20_nodes(monkeypatch):
    import certifiedgpt_amd.llm_laws as laws
    assert laws.TRIE_MAX_NODES == 2 ** 20 and laws.TRIE_MAX_DEPTH == 32
    monkeypatch.setattr(laws, "TRIE_MAX_NODES", 8)                     # the rule itself, at a size a test can build
    with pytest.raises(ValueError, match="more than 8 nodes"):
        build_answer_trie(FIVE, 16)


# ---- cgpt_llm_trie_check: the library loads without a GPU
def trie_check(tabs, vocab, nodes=None, edges=None):
    L = _lib.lib()
    ts = [torch.tensor(t, dtype=torch.int32) for t in tabs]
    depth = C.c_int32(-1)
    rc = L.cgpt_llm_trie_check(*[C.c_void_p(t.data_ptr()) for t in ts], len(tabs[3]) if nodes is None else nodes,
                               len(tabs[1]) if edges is None else edges, vocab, C.byref(depth))
    return rc, depth.value, L.cgpt_last_error().decode()


def test_library_validator_accepts_what_the_builder_makes():
    assert trie_check(FIVE_TABLES, 16)[:2] == (0, 3)
    assert trie_check(FIVE_TABLES, 10)[:2] == (0, 3)                   # token 9 is the last id of a vocabulary of 10
    rng = random.Random(5)
    seqs = {tuple(rng.randrange(3, 40) for _ in range(4))[:rng.randrange(1, 5)] for _ in range(60)}
    seqs = [s for s in seqs if not any(o != s and o[:len(s)] == s for o in seqs)]
    trie = build_answer_trie(seqs, 40)
    assert trie_check(tables(trie), 40)[:2] == (0, trie.depth)
    L = _lib.lib()
    ts = [torch.tensor(t, dtype=torch.int32) for t in FIVE_TABLES]
    assert L.cgpt_llm_trie_check(*[C.c_void_p(t.data_ptr()) for t in ts], 9, 8, 16, None) == 0    # depth_out is optional


def broken(table, index, value):
    tabs = [list(t) for t in FIVE_TABLES]
    tabs[table][index] = value
    return tabs


@pytest.mark.parametrize("name, tabs, vocab, node", [
    ("unsorted edges", broken(1, 0, 6), 16, "node 0"),                 # root: 6 5 8
    ("a duplicate token under one node", broken(1, 1, 2), 16, "node 0"),           # root: 2 2 8
    ("a child index <= its parent's", broken(2, 3, 2), 16, "node 2"),              # node 2 -> node 2
    ("a child index below its parent's", broken(2, 6, 1), 16, "node 4"),           # node 4 -> node 1
    ("a leaf with class -1", broken(3, 1, -1), 16, "node 1"),
    ("an inner node with a class", broken(3, 2, 7), 16, "node 2"),
    ("a token >= vocab", [list(t) for t in FIVE_TABLES], 9, "node 4"),             # token 9 under node 4
    ("child_begin[nodes] != edges", broken(0, 9, 7), 16, "node"),
    ("an unreachable node", broken(2, 7, 7), 16, "node"),                          # nothing leads to node 8, two edges to node 7
])
def test_library_validator_refuses_each_broken_property(name, tabs, vocab, node):
    rc, _, msg = trie_check(tabs, vocab)
    assert rc == 1 and "cgpt_llm_trie_check" in msg and node in msg, (name, rc, msg)


def test_library_validator_refuses_bad_sizes_and_null_tables():
    L = _lib.lib()
    assert trie_check(FIVE_TABLES, 16, edges=7)[0] == 1                # edges != nodes - 1
    assert trie_check(FIVE_TABLES, 16, nodes=2 ** 20 + 1, edges=2 ** 20)[0] == 1
    assert trie_check(([0, 1, 1], [3], [1], [-1, 0]), 16)[0] == 1      # one candidate
    chain = 34                                                         # one candidate of 33 tokens beside a short one: depth 33
    begin = [0, 2, 2] + list(range(3, chain + 1)) + [chain]
    assert len(begin) == chain + 2
    rc, _, msg = trie_check((begin, [1, 2] + [3] * (chain - 2), list(range(1, chain + 1)), [-1, 0] + [-1] * (chain - 2) + [1]), 16)
    assert rc == 1 and "depth" in msg, msg
    assert L.cgpt_llm_trie_check(None, None, None, None, 9, 8, 16, None) == 1
    # cgpt_llm_set_trie needs a handle before it needs a device
    assert L.cgpt_llm_set_trie(None, None, None, None, None, 0, 0) == 1 and b"cgpt_llm_set_trie" in L.cgpt_last_error()


def test_new_entries_are_bound_like_their_greedy_twins():
    sig = _lib.SIGNATURES
    greedy, ragged = list(sig["cgpt_llm_greedy"][1]), list(sig["cgpt_llm_greedy_ragged"][1])
    # without min_new and the EOS ids (three arguments), with the labels pointer in front of the stream
    assert sig["cgpt_llm_constrained"][1] == greedy[:5] + greedy[8:-1] + [C.c_void_p, C.c_void_p]
    assert sig["cgpt_llm_constrained_ragged"][1] == ragged[:6] + ragged[9:-1] + [C.c_void_p, C.c_void_p]
    assert sig["cgpt_vote_labels"] == sig["cgpt_vote"]
    L = _lib.lib()
    one = C.c_void_p(8)
    assert L.cgpt_llm_constrained(None, one, 1, 4, 3, 0, None, None, 8, one, None, one, None) == 1
    assert L.cgpt_vote_labels(None, 4, 3, one, None) == 1 and b"cgpt_vote_labels" in L.cgpt_last_error()
    assert L.cgpt_llm_trie_select_logits(None, 8, 1, 8, one, one, one, one, 9, 0, one, one, one, one, None) == 1
    assert b"cgpt_llm_trie_select_logits" in L.cgpt_last_error()


# ---- the select law against a brute-force loop
def brute_select(logits, node, unfinished, tabs, pad):
    begin, tok, child, leaf = tabs
    out = []
    for b in range(len(node)):
        if not unfinished[b]:
            out.append((pad, node[b], 0, -1))
            continue
        best, at = None, None
        for e in range(begin[node[b]], begin[node[b] + 1]):           # ascending tokens: strictly greater keeps the lowest id
            v = float(logits[b][tok[e]])
            if best is None or v > best:
                best, at = v, e
        c = child[at]
        out.append((tok[at], c, 0 if leaf[c] >= 0 else 1, leaf[c] if leaf[c] >= 0 else -1))
    return [list(col) for col in zip(*out)]


def test_select_law_equals_the_brute_force_loop_ties_and_finished_rows_included():
    trie = build_answer_trie(FIVE, 16)
    g = torch.Generator().manual_seed(11)
    B = 64
    logits = torch.randn(B, 16, generator=g)
    node = torch.tensor([0, 2, 3, 4] * (B // 4), dtype=torch.int32)
    unfinished = torch.ones(B, dtype=torch.int32)
    unfinished[5::7] = 0
    logits[0, 2] = logits[0, 5] = logits[0, 8] = 3.5                   # a three-way tie at the root: token 2
    logits[1, 3] = logits[1, 7] = -0.25                                # a tie at node 2: token 3
    logits[3, 4] = logits[3, 9] = 9.0                                  # a tie at node 4: token 4
    logits[4, 8] = logits[4, 5] = 50.0                                 # root: 5 before 8
    logits[:, [0, 6, 10, 15]] = 1e30                                   # tokens on no edge never matter
    got = constrained_select_law(logits, node, unfinished, trie, 99)
    want = brute_select(logits.tolist(), node.tolist(), unfinished.tolist(), tables(trie), 99)
    assert [t.tolist() for t in got] == want
    assert [t.dtype for t in got] == [torch.int64, torch.int32, torch.int32, torch.int32]
    tok, node2, unf2, lab = got
    assert (tok[0], node2[0], unf2[0], lab[0]) == (2, 1, 0, 2) and (tok[1], node2[1]) == (3, 4) and (tok[3], lab[3]) == (4, 3)
    assert (tok[4], node2[4], unf2[4], lab[4]) == (5, 2, 1, -1)
    assert tok[5] == 99 and node2[5] == node[5] and unf2[5] == 0 and lab[5] == -1     # a finished row emits pad and stays put
    again = constrained_select_law(logits, node2, unf2, trie, 99)                    # and stays finished
    assert bool((again[2][unf2 == 0] == 0).all()) and bool((again[0][unf2 == 0] == 99).all())


def test_decode_law_spells_one_candidate_per_row_and_allowed_tokens_walk_the_same_trie():
    trie = build_answer_trie(FIVE, 16)
    g = torch.Generator().manual_seed(2)
    tokens, labels = constrained_decode_law(torch.randn(40, 3, 16, generator=g), trie, 0)
    assert labels.dtype == torch.int32 and bool((labels >= 0).all()) and len(set(labels.tolist())) >= 4
    for row, lab in zip(tokens.tolist(), labels.tolist()):
        n = len(FIVE[lab])
        assert tuple(row[:n]) == FIVE[lab] and row[n:] == [0] * (3 - n)
    assert trie_walk(tokens, trie) == labels.tolist()
    fn = allowed_tokens_fn(trie, 77)
    ids = lambda *t: torch.tensor(t, dtype=torch.long)                 # noqa: E731
    assert fn(0, ids()) == [2, 5, 8] and fn(3, ids(5)) == [3, 7] and fn(0, ids(5, 3)) == [4, 9]
    assert fn(0, ids(2)) == [77] and fn(0, ids(5, 7)) == [77] and fn(0, ids(5, 7, 77)) == [77] and fn(0, ids(8, 1, 77, 77)) == [77]


# ---- constrain="hf" end to end on the toy decoder
CANDS = ["red", "red car", "red car door", "blue", "blue sky", "green", "green car", "dark blue sky"]


class Enc(StubEncoder):
    max_batch = 8

    def encode_img_noisy(self, x, first, num, sigma, seed):
        g = torch.Generator().manual_seed(1000)
        table = torch.randn(64, 3, generator=g)
        return self.encode_img(x[None] + sigma * table[first:first + num, :, None, None])[0]


def cpu_vote(logits, counts):
    counts += torch.bincount(logits.argmax(1), minlength=counts.numel())


def toy_classifier(classify="constrained", **kw):
    return MiniGPT4Classifier(Enc(), tiny_llama(), ToyTokenizer(), PROMPT, AnswerLabelMap(len(CANDS) + 1, CANDS), max_new_tokens=4,
                              classify=classify, end_sym=" ###", **kw)


def test_hf_constrained_decode_end_to_end(monkeypatch):
    """Every row spells exactly one candidate; the labels are `constrained_decode_law` of HF's own logits of the same run; the
    histogram has no "other" vote -- while free-text generation of the same toy decoder on the same noisy copies votes "other" (seed
    fixed: all 40 rows do, a random-init decoder emits no vocabulary answer)."""
    monkeypatch.setattr(m, "vote", cpu_vote)
    clf = toy_classifier()
    tok = ToyTokenizer()
    seqs = [tuple(tok(c + " ###", add_special_tokens=False).input_ids[0].tolist()) for c in CANDS]
    assert clf.trie.depth == 4 == max(len(s) for s in seqs) and tables(clf.trie) == tables(build_answer_trie(seqs, VOCAB))
    x = torch.randn(3, 8, 8, generator=torch.Generator().manual_seed(4))
    emb = clf.encoder.encode_img_noisy(x, 0, 40, 2.0, 0)
    labels, tokens, logits = clf.constrained_from_embeds(emb, PROMPT, return_logits=True)
    assert tuple(tokens.shape) == (40, 4) and tuple(logits.shape) == (40, 4, VOCAB) and labels.dtype == torch.int32
    for row, lab in zip(tokens.tolist(), labels.tolist()):
        n = len(seqs[lab])
        assert tuple(row[:n]) == seqs[lab] and row[n:] == [PAD] * (4 - n)
    law_tokens, law_labels = constrained_decode_law(logits, clf.trie, PAD)
    assert torch.equal(law_tokens, tokens) and torch.equal(law_labels, labels)
    assert len(set(labels.tolist())) >= 3                              # the noisy copies do not all agree
    # the classifier surface: one-hot logits of the labels, the candidates' texts, the histogram
    out, answers = clf._classify_embeds(emb[:8], torch.device("cpu"))
    assert out.argmax(1).tolist() == labels[:8].tolist() and bool((out.sum(1) == 1).all()) and out.shape == (8, len(CANDS) + 1)
    assert answers == [CANDS[i] for i in labels[:8].tolist()]
    counts = clf.sample_counts(x, 0, 40, 7, 2.0, 0)
    other = clf.label_map.other_id
    assert int(counts.sum()) == 40 and int(counts[other]) == 0
    assert counts.tolist() == torch.bincount(labels.long(), minlength=len(CANDS) + 1).tolist()
    assert clf.last_answers[-5:] == [CANDS[i] for i in labels[-5:].tolist()]
    pair = clf.sample_counts_pair(x, 0, 16, 16, 24, 5, 2.0, 0)
    assert pair[0].tolist() == clf.sample_counts(x, 0, 16, 8, 2.0, 0).tolist()
    assert pair[1].tolist() == clf.sample_counts(x, 16, 24, 8, 2.0, 0).tolist()
    assert clf.decode_stats["hf_constrained"] > 0 and clf.decode_stats["hip_constrained"] == 0
    assert clf.decode_stats["hf_constrained_fallbacks"] == 0
    free = toy_classifier("generate")
    free_counts = free.sample_counts(x, 0, 40, 7, 2.0, 0)
    assert int(free_counts[other]) > 0, free_counts.tolist()           # what the feature buys: these rows are lost votes


def test_stop_sequences_belong_to_generate_and_do_not_touch_the_constrained_call(monkeypatch):
    plain = toy_classifier()
    tok = ToyTokenizer()
    first = int(tok("red", add_special_tokens=False).input_ids[0, 0])
    stopped = toy_classifier(stop_words_ids=[[first]], stop_text="red")
    emb = plain.encoder.encode_img_noisy(torch.randn(3, 8, 8, generator=torch.Generator().manual_seed(4)), 0, 16, 2.0, 0)
    a, b = plain.constrained_from_embeds(emb, PROMPT), stopped.constrained_from_embeds(emb, PROMPT)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_construction_refusals():
    with pytest.raises(ValueError, match='constrain="hip" needs decode="hip"'):
        toy_classifier(constrain="hip")
    with pytest.raises(ValueError, match="constrain="):
        toy_classifier(constrain="native")
    with pytest.raises(ValueError, match='needs classify="constrained"'):
        toy_classifier("generate", constrain="hip", decode="hip")
    for kw in ({"do_sample": True}, {"repetition_penalty": 1.05}, {"num_beams": 2}, {"no_repeat_ngram_size": 2}):
        with pytest.raises(ValueError, match="arg-max"):
            toy_classifier(generate_kwargs=kw)
    with pytest.raises(ValueError) as e:                               # "red" is a prefix of "red car" once nothing ends an answer
        MiniGPT4Classifier(Enc(), tiny_llama(), ToyTokenizer(), PROMPT, AnswerLabelMap(len(CANDS) + 1, CANDS), classify="constrained",
                           candidates=["blue", "red car", "red"])
    assert "'red'" in str(e.value) and "'red car'" in str(e.value) and "prefix" in str(e.value)
    with pytest.raises(ValueError, match="at least 2"):
        MiniGPT4Classifier(Enc(), tiny_llama(), ToyTokenizer(), PROMPT, AnswerLabelMap(4, ["red"]), classify="constrained")
    with pytest.raises(ValueError, match="candidates need"):
        toy_classifier("generate", candidates=["red", "blue"])


def test_agent_passes_classify_and_constrain_through(monkeypatch):
    from certifiedgpt_amd.agents import minigpt4_certify_agent as agent
    seen = {}

    class Probe:
        def __init__(self, *a, **kw):
            seen.update(kw)

    monkeypatch.setattr(m, "MiniGPT4Classifier", Probe)

    class E:
        max_batch, device = 4, torch.device("cpu")

    agent.build_generating_classifier(E(), {"answers": ["red", "blue"], "classify": "constrained", "constrain": "hip", "decode": "hip"}, 3,
                                      ToyTokenizer(), tiny_llama())
    assert seen["classify"] == "constrained" and seen["constrain"] == "hip"
    agent.build_generating_classifier(E(), {"answers": ["red", "blue"]}, 3, ToyTokenizer(), tiny_llama())
    assert seen["classify"] == "generate" and seen["constrain"] == "hf"
