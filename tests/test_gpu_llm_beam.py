"""Beam search on the native LLaMA engine (beams="hip"; csrc/llm_beam.hip) on the device.

The parity chain is law = HF on the CPU (tests/test_llm_beam_cpu.py) and engine = law here: the ancestry attention is the plain step
attention bit for bit, one select is `beam_step_law`, the whole loop is the law applied to the engine's own previous state and logits,
and the classifier returns what the loop returns.

The margin of a select against the float64 law, from the kernel's stated rounding sequence (header of csrc/llm_beam.hip).  The
normaliser is float64 on both sides (about 1e-15 relative between the two summation orders: nothing).  A candidate score then takes
TWO fp32 roundings, lp = fp32(l - lse) and c = fp32(running + lp), each at most half an ulp of its result, and |lp| <= |c| because both
terms are <= 0: the kernel's c is within 1 fp32 ulp (taken at |c|) of the law's, so two candidates the select compares are ordered
alike unless they differ by at most 2 ulp of the larger magnitude -- ULPS[0].  A pool entrant's score and step 7's left side take a
THIRD rounding, the IEEE division by the fp32 divisor both sides share: 1.5 ulp per value, 3 ulp per compared pair -- ULPS[1] (an old
pool score is an input, exact on both sides, which only makes the pair tighter).  Scores are asserted within the same bounds: running
within 2 ulp, pool scores within 3.  A case (an image of one select) whose law margin falls inside these bounds may legitimately come
out differently and is skipped; that is a condition: at most 5 % of the cases of a test."""
import ctypes as C

import pytest
import torch

from certifiedgpt_amd import _lib
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.llm_laws import BEAM_NEG, _ulp32, beam_init_state, beam_keep, beam_step_law, int8_state_dict
from certifiedgpt_amd.minigpt4 import MiniGPT4Classifier, WordHashTokenizer, _HipDecoder
from gpu_util import DEV
import llm_util as lu
from llm_util import EOS, K_SENTINEL, PAD, PROMPT, V_SENTINEL

pytestmark = pytest.mark.gpu
ULPS = (2.0, 3.0)


def P(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def within(a, ref, ulps):
    """|a - ref| <= ulps fp32 ulp of |ref|, elementwise on CPU tensors (equal infinities and the exact -1e9 pass)."""
    a, ref = a.double(), ref.double()
    return bool(((a == ref) | ((a - ref).abs() <= ulps * _ulp32(ref))).all())


@pytest.fixture(scope="module")
def small():
    llm = lu.small_decoder()
    dec = _HipDecoder(llm, 32)
    yield llm, dec
    dec.close()


# ------------------------------------------------------------------------------------------ 1. the ancestry attention
def random_ancestry(B, k, n, t, seed):
    """anc [B k, n] int32: column s < t of row r names a row of r's image.  Row 0 of every image descends from other rows only, rows
    k - 2 and k - 1 share every ancestor; columns >= t hold the row itself, as the select leaves them."""
    g = torch.Generator().manual_seed(seed)
    anc = torch.empty((B * k, n), dtype=torch.int32)
    for b in range(B):
        for j in range(k):
            anc[b * k + j] = b * k + j
            anc[b * k + j, :t] = b * k + torch.randint(0, k, (t,), generator=g).int()
        if t:
            anc[b * k, :t] = b * k + 1 + torch.randint(0, k - 1, (t,), generator=g).int()
            anc[b * k + k - 1, :t] = anc[b * k + k - 2, :t]
    return anc.to(DEV)


@pytest.mark.parametrize("k, t", [(4, 5), (4, 0), (2, 5)])
def test_ancestry_attention_is_the_plain_attention(small, k, t):
    llm, dec = small
    B, L, n = 3, 9, 8
    rows, heads, layers = B * k, dec.heads, dec.layers
    g = torch.Generator().manual_seed(40 + t + k)

    def fill(bufs, upto):
        for buf in bufs:
            buf[:, :, :upto] = (torch.randn(buf[:, :, :upto].shape, generator=g) * 0.5).to(torch.float16).to(DEV)

    pk, pv = lu.sentinel_cache(layers, heads, B, L + 3)               # rows L .. keep their sentinel
    bk, bv = lu.sentinel_cache(layers, heads, rows, n - 1)
    fill(pk + pv, L)
    fill(bk + bv, t)
    anc = random_ancestry(B, k, n, t, seed=7)
    if t:
        assert bool((anc[0, :t] != 0).all()) and torch.equal(anc[k - 1, :t], anc[k - 2, :t])
    tokens = torch.randint(3, 320, (rows,), generator=g).to(DEV)
    before = [x.clone() for x in pk + pv + bk + bv]
    got = dec.beam_step(tokens, k, L, t, anc, pk, pv, bk, bv)
    # the same hypotheses as physically gathered caches [rows, heads, L + t + 1, 128] under the plain step
    gk, gv = lu.sentinel_cache(layers, heads, rows, L + t + 1)
    img = torch.arange(rows, device=DEV) // k
    for l in range(layers):
        for dst, prompt, beam in ((gk[l], pk[l], bk[l]), (gv[l], pv[l], bv[l])):
            dst[:, :, :L] = prompt[img, :, :L]
            for s in range(t):
                dst[:, :, L + s] = beam[anc[:, s].long(), :, s]
    want = dec.step(tokens, L + t, gk, gv)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    for l in range(layers):
        assert torch.equal(bk[l][:, :, t], gk[l][:, :, L + t]) and torch.equal(bv[l][:, :, t], gv[l][:, :, L + t])
        assert not bool((bk[l][:, :, t] == K_SENTINEL).all(dim=-1).any())
        assert bool((bk[l][:, :, t + 1:] == K_SENTINEL).all()) and bool((bv[l][:, :, t + 1:] == V_SENTINEL).all())
        assert bool((pk[l][:, :, L:] == K_SENTINEL).all()) and bool((pv[l][:, :, L:] == V_SENTINEL).all())
    keep = torch.ones(n - 1, dtype=torch.bool, device=DEV)
    keep[t] = False
    for x, was, is_beam in zip(pk + pv + bk + bv, before, [False] * (2 * layers) + [True] * (2 * layers)):
        assert torch.equal(x[:, :, keep], was[:, :, keep]) if is_beam else torch.equal(x, was)


# ------------------------------------------------------------------------------------------ 2. one select against the law
FIELDS = ("running", "tokens", "anc", "pool_score", "pool_fin", "pool_len", "pool_seq", "open")
DTYPES = {"running": torch.float32, "tokens": torch.int64, "anc": torch.int32, "pool_score": torch.float32, "pool_fin": torch.int32,
          "pool_len": torch.int32, "pool_seq": torch.int64, "open": torch.int32}


def kernel_select(logits, state, i, n, min_new, eos, lp):
    """cgpt_llm_beam_select_logits on logits [B, k, V] and a law-shaped `state` (CPU) -> the state after, parents, next tokens (CPU)."""
    B, k, V = logits.shape
    dev_in = {f: state[f].reshape(-1, *state[f].shape[2:]).to(DTYPES[f]).contiguous().to(DEV) if f != "open"
              else state[f].to(torch.int32).to(DEV) for f in FIELDS}
    dev_out = {f: torch.full_like(v, -7) for f, v in dev_in.items()}
    nxt = torch.full((B * k,), -7, dtype=torch.int64, device=DEV)
    par = torch.full((B * k,), -7, dtype=torch.int32, device=DEV)
    lg = logits.reshape(B * k, V).float().contiguous().to(DEV)
    ids = (C.c_int64 * max(1, len(eos)))(*eos)
    _lib.check(_lib.lib().cgpt_llm_beam_select_logits(P(lg), V, B, k, V, i, n, min_new, ids, len(eos), PAD, lp,
                                                      *[P(dev_in[f]) for f in FIELDS], *[P(dev_out[f]) for f in FIELDS], P(nxt), P(par),
                                                      _stream()))
    torch.cuda.synchronize()
    out = {f: v.cpu().view(B, k, *v.shape[1:]) if f != "open" else v.cpu() for f, v in dev_out.items()}
    return out, par.cpu().view(B, k), nxt.cpu().view(B, k)


def with_anc(state, B, k, n, i, seed):
    """`state` plus an ancestry table whose columns < i are random rows of the image."""
    g = torch.Generator().manual_seed(seed)
    anc = (torch.arange(B * k).view(B, k, 1).expand(B, k, n)).clone().int()
    if i:
        anc[:, :, :i] = (torch.arange(B).view(B, 1, 1) * k + torch.randint(0, k, (B, k, i), generator=g)).int()
    return {**state, "anc": anc}


def check_select(got, par, nxt, law, state, i, skip):
    """Discrete outputs identical, scores within the margin, for the images the law does not call near-tied."""
    B, k = par.shape
    for b in range(B):
        if skip[b]:
            continue
        assert par[b].tolist() == law["parents"][b].tolist() and nxt[b].tolist() == law["next_tokens"][b].tolist(), (b, i)
        assert torch.equal(got["tokens"][b], law["tokens"][b]), (b, i)
        assert got["pool_fin"][b].bool().tolist() == law["pool_fin"][b].tolist(), (b, i)
        assert got["pool_len"][b].tolist() == law["pool_len"][b].tolist() and torch.equal(got["pool_seq"][b], law["pool_seq"][b]), (b, i)
        assert bool(got["open"][b]) == bool(law["open"][b]), (b, i)
        assert within(got["running"][b], law["running"][b], ULPS[0]), (b, i, got["running"][b], law["running"][b])
        assert within(got["pool_score"][b], law["pool_score"][b], ULPS[1]), (b, i, got["pool_score"][b], law["pool_score"][b])
        want_anc = state["anc"][b][law["parents"][b]].clone()          # columns < i from the parent, column i the row itself
        want_anc[:, i] = b * k + torch.arange(k, dtype=torch.int32)
        assert torch.equal(got["anc"][b][:, :i + 1], want_anc[:, :i + 1]), (b, i)


def mid_state(B, k, n, i, g, pool):
    """A state before select i >= 1: descending running scores, random tokens, a pool with `pool` finished slots per image (their
    scores near the running scores over the length, so that entrants compete), open unless the pool says otherwise."""
    s = beam_init_state(B, k, n, PAD)
    run = -(torch.rand(B, k, generator=g).double() * 3 + 0.5 * i).sort(dim=1).values
    s["running"] = run.float().double()
    s["tokens"][:, :, :i] = torch.randint(3, 300, (B, k, i), generator=g)
    for b in range(B):
        m = pool[b % len(pool)]
        sc = (run[b, :m] / i + torch.randn(m, generator=g).double() * 0.3).sort(descending=True).values
        s["pool_score"][b, :m] = sc.float().double()
        s["pool_fin"][b, :m] = True
        s["pool_len"][b, :m] = torch.randint(1, i + 1, (m,), generator=g)
        for q in range(m):
            ln = int(s["pool_len"][b, q])
            s["pool_seq"][b, q, :ln] = torch.randint(3, 300, (ln,), generator=g)
    return s


@pytest.mark.parametrize("V, k, eos", [(320, 2, [EOS]), (320, 4, [EOS]), (320, 8, [EOS]), (320, 2, [EOS, 5]), (320, 4, [EOS, 5]),
                                        (320, 8, [EOS, 5]), (32000, 4, [EOS])])
def test_select_equals_the_law(V, k, eos):
    n, B = 6, 8
    g = torch.Generator().manual_seed(V + 10 * k + len(eos))
    cases = near = 0

    def logits(boost):
        lg = torch.randn(B, k, V, generator=g) * 2
        lg[::2, :, eos[0]] += boost                                   # every other image: an EOS that competes
        return lg

    runs = []
    # fresh: select 0 on the initial state, below min_new (EOS masked) and at min_new = 0 (an EOS can win and enter the pool)
    for min_new in (1, 0):
        runs.append((with_anc(beam_init_state(B, k, n, PAD), B, k, n, 0, 1), logits(8.0), 0, min_new, 1.0))
    # mid-run: an empty pool, a partly and a fully finished one; i < min_new once; three length penalties; a closed image
    for i, min_new, lp, pool in ((2, 0, 1.0, (0, 1, k)), (3, 4, 1.0, (0, k - 1)), (2, 0, 0.0, (1, k)), (4, 0, 2.0, (k, k - 1)),
                                 (n - 1, 0, 1.0, (0, 1, k)), (n - 1, 0, 0.7, (k,))):
        s = mid_state(B, k, n, i, g, pool)
        s["open"][B - 1] = False
        lg = logits(6.0)
        lg[1, k - 1] = lg[1, 0]                                        # exact ties: two beams of image 1 with one logits row ...
        s["running"][1, k - 1] = s["running"][1, 0]                    # ... and one running score
        runs.append((with_anc(s, B, k, n, i, 2 + i), lg, i, min_new, lp))
    for state, lg, i, min_new, lp in runs:
        law = beam_step_law(state, lg, i, n, min_new, eos, PAD, lp, ulps=ULPS)
        got, par, nxt = kernel_select(lg, state, i, n, min_new, eos, lp)
        cases += B
        near += int(law["near"].sum())
        check_select(got, par, nxt, law, state, i, law["near"].tolist())
        if not bool(state["open"][B - 1]):                             # a closed image keeps its pool
            assert torch.equal(got["pool_seq"][B - 1], state["pool_seq"][B - 1]) and not bool(got["open"][B - 1])
    print(f"[beam select V={V} k={k} E={len(eos)}] {near} of {cases} cases inside the margin (skipped)", flush=True)
    assert near <= 0.05 * cases


# ------------------------------------------------------------------------------------------ 3. the whole loop
def run_loop(dec, llm, B, k, L, n, eos, lp, seed, min_new=1):
    embs = lu.embeds(llm, B, L, seed=seed)
    pk, pv = lu.sentinel_cache(dec.layers, dec.heads, B, L)
    bk, bv = lu.sentinel_cache(dec.layers, dec.heads, B * k, max(1, n - 1))
    first = dec.prefill(embs, pk, pv)
    out = dec.beam(first, k, L, n, min_new, eos, PAD, lp, pk, pv, bk, bv, return_logits=True)
    torch.cuda.synchronize()
    return first, out, (pk, pv, bk, bv)


def replay(first, out, B, k, n, eos, lp, min_new=1):
    """Every (image, select): the engine's state after equals `beam_step_law` of the engine's own state before and the logits it read.
    Returns (cases, skipped): an image is followed until one of its selects is inside the margin."""
    tokens, scores, steps, trace = [t.cpu() for t in out]
    V = steps.shape[-1]
    assert torch.equal(steps[:, 0].view(B, k, V), first.cpu()[:, None].expand(B, k, V))
    state = beam_init_state(B, k, n, PAD)
    alive = [True] * B
    cases = skipped = 0
    for i in range(n):
        law = beam_step_law(state, steps[:, i].view(B, k, V), i, n, min_new, eos, PAD, lp, ulps=ULPS)
        t = trace[i]
        run, par, tok = t[:, :k], t[:, k:2 * k].long(), t[:, 2 * k:3 * k].long()
        ps, pf, op = t[:, 3 * k:4 * k], t[:, 4 * k:5 * k] != 0, t[:, 5 * k] != 0
        for b in range(B):
            if not alive[b]:
                continue
            cases += 1
            if bool(law["near"][b]):
                alive[b] = False
                skipped += 1
                continue
            assert par[b].tolist() == law["parents"][b].tolist() and tok[b].tolist() == law["next_tokens"][b].tolist(), (b, i)
            assert pf[b].tolist() == law["pool_fin"][b].tolist() and bool(op[b]) == bool(law["open"][b]), (b, i)
            assert within(run[b], law["running"][b], ULPS[0]) and within(ps[b], law["pool_score"][b], ULPS[1]), (b, i)
        state = law                                                   # discrete fields: the law's (equal to the engine's, asserted) ...
        state["running"] = run.double()                               # ... scores: the engine's own fp32 values
        state["pool_score"] = ps.double()
    for b in range(B):
        if alive[b]:
            assert tokens[b].tolist() == state["pool_seq"][b, 0].tolist(), b
            assert float(scores[b]) == float(state["pool_score"][b, 0]), b
            ln = int(state["pool_len"][b, 0])
            assert tokens[b, ln:].tolist() == [PAD] * (n - ln)
    return cases, skipped, state


def test_whole_loop_replays_under_the_law_and_under_a_graph(small):
    llm, dec = small
    B, k, L, n = 5, 4, 7, 6
    first, out, _ = run_loop(dec, llm, B, k, L, n, [EOS], 1.0, seed=21)
    cases, skipped, _ = replay(first, out, B, k, n, [EOS], 1.0)
    # a second EOS id that image 0's winner emits at its third token: hypotheses finish early, the pool fills before the last select
    eos = [EOS, int(out[0][0, 2])]
    # (no length normalisation, so that a short finished hypothesis keeps its place against the longer ones)
    first2, out2, bufs = run_loop(dec, llm, B, k, L, n, eos, 0.0, seed=21)
    c2, s2, state = replay(first2, out2, B, k, n, eos, 0.0)
    assert int(state["pool_len"].min()) < n
    print(f"[beam loop] {skipped + s2} of {cases + c2} (image, select) cases inside the margin (skipped)", flush=True)
    assert skipped + s2 <= 0.05 * (cases + c2)
    # captured and replayed twice: identical bits
    pk, pv, bk, bv = bufs
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        dec.beam(first2, k, L, n, 1, eos, PAD, 0.0, pk, pv, bk, bv, return_logits=True)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        static = dec.beam(first2, k, L, n, 1, eos, PAD, 0.0, pk, pv, bk, bv, return_logits=True)
    for _ in range(2):
        for t in static:
            t.fill_(-3)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(static, out2):
            assert torch.equal(a, b)


def test_entries_refuse_before_any_launch(small):
    llm, dec = small
    L_ = _lib.lib()
    B, k, L, n = 2, 4, 7, 6
    pk, pv = lu.sentinel_cache(dec.layers, dec.heads, B, L)
    bk, bv = lu.sentinel_cache(dec.layers, dec.heads, B * k, n - 1)
    first = torch.zeros(B, 320, device=DEV)
    with pytest.raises(_lib.CgptError, match="outside 1..max_batch = 32") as e:
        _lib.check(dec.L.cgpt_llm_beam_reserve(dec.handle, 9, 4, n))
    assert "9 images x 4 beams" in str(e.value)
    dec.set_early_stop(True)
    try:
        with pytest.raises(_lib.CgptError, match="CGPT_ERR_STATE.*early stop"):
            dec.beam(first, k, L, n, 1, [EOS], PAD, 1.0, pk, pv, bk, bv)
    finally:
        dec.set_early_stop(False)
    dec.set_stop_sequences([[5, 6]])
    try:
        with pytest.raises(_lib.CgptError, match="CGPT_ERR_STATE.*stop sequences"):
            dec.beam(first, k, L, n, 1, [EOS], PAD, 1.0, pk, pv, bk, bv)
    finally:
        dec.set_stop_sequences(None)
    for x in pk + pv + bk + bv:                                        # nothing was launched
        assert bool((x.float().abs() > 50).all())
    assert L_.cgpt_llm_beam_step(dec.handle, P(first), B, 9, L, 0, P(first), 6, None, None, L, None, None, 5, P(first), None) == 1
    gqa_llm = lu.llama_decoder(512, 4, 1408, 320, kv_heads=2)
    gqa = _HipDecoder(gqa_llm, 32, grouped_kv=True)
    try:
        one = C.c_void_p(8)
        tab = (C.c_void_p * gqa.layers)(*[8] * gqa.layers)
        assert L_.cgpt_llm_beam(gqa.handle, P(first), B, k, L, n, 1, None, 0, PAD, 1.0, tab, tab, L, tab, tab, n - 1, one, None, None, None,
                                None) == 1
        assert b"grouped_kv" in L_.cgpt_last_error()
    finally:
        gqa.close()


# ------------------------------------------------------------------------------------------ 4. the classifier
class Enc:
    """Stands where the encoder stands: the tests hand image embeddings to `generate_from_embeds` themselves."""
    max_batch = 16


def make(llm, **kw):
    kw.setdefault("generate_kwargs", {"num_beams": 4})
    return MiniGPT4Classifier(Enc(), llm, WordHashTokenizer(320), PROMPT, AnswerLabelMap(4, ["red", "blue"]), max_batch=16, max_new_tokens=6,
                              decode="hip", prefill="hip", **kw)


def image_embeds(B, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 4, 512, generator=g) * 0.3).to(torch.float16).to(DEV)


def eager(clf, img):
    embs, _, _, prefix, _, _ = clf._prompt_inputs(img, PROMPT)
    return clf.greedy_tokens(embs, return_logits=True, **({"prefix": prefix} if prefix else {}))


@pytest.fixture(scope="module")
def llm_small():
    return lu.small_decoder()


def test_classifier_answers_are_the_replayed_law(llm_small):
    clf = make(llm_small, beams="hip")
    img = image_embeds(3, 1)
    answers = clf.generate_from_embeds(img, PROMPT)
    assert clf.decode_stats["hip_beam"] == 1 and clf.decode_stats["hf_calls"] == 0 and clf.decode_stats["graph_replays"] == 1
    scores = clf.last_beam_scores().clone()
    out = eager(clf, img)
    embs = clf._prompt_inputs(img, PROMPT)[0]
    first = clf._hip.prefill(embs.contiguous(), *clf._kv_buffers(embs, 3, embs.shape[1]))
    torch.cuda.synchronize()
    cases, skipped, _ = replay(first, out, 3, 4, 6, [EOS], 1.0)
    assert skipped == 0, "pick another seed: an image of this call is inside the margin"
    assert clf._decode_outputs(out[0]) == answers and torch.equal(out[1], scores)
    assert clf.generate_from_embeds(img, PROMPT) == answers and clf.decode_stats["hip_beam"] == 2
    assert clf.decode_stats["graph_captures"] == 1


def test_classifier_chunks_equal_the_images_one_by_one(llm_small):
    clf = make(llm_small, beams="hip", generate_kwargs={"num_beams": 4, "length_penalty": 0.5})
    img = image_embeds(10, 2)                                          # max_batch 16 at 4 beams: chunks of 4, 4 and 2 images
    tokens, scores = eager(clf, img)[:2]
    for b in range(10):
        t1, s1 = eager(clf, img[b:b + 1])[:2]
        assert torch.equal(t1[0], tokens[b]) and torch.equal(s1[0], scores[b]), b
    answers = clf.generate_from_embeds(img, PROMPT)
    assert answers == clf._decode_outputs(tokens) and torch.equal(clf.last_beam_scores(), scores)


def test_classifier_int8_weights_equal_the_fp16_engine_on_the_int8_twin(llm_small):
    twin = lu.llama_decoder(512, 4, 1408, 320, sd=int8_state_dict(llm_small))
    a, b = make(llm_small, beams="hip", weights="int8"), make(twin, beams="hip")
    img = image_embeds(5, 3)
    for x, y in zip(eager(a, img), eager(b, img)):
        assert torch.equal(x, y)
    assert a.generate_from_embeds(img, PROMPT) == b.generate_from_embeds(img, PROMPT)


def test_classifier_shared_prefix_equals_it_off(llm_small):
    on, off = make(llm_small, beams="hip", shared_prefix=True), make(llm_small, beams="hip")
    img = image_embeds(5, 4)
    assert on._prompt_inputs(img, PROMPT)[3] is not None
    for x, y in zip(eager(on, img), eager(off, img)):
        assert torch.equal(x, y)
    assert on.generate_from_embeds(img, PROMPT) == off.generate_from_embeds(img, PROMPT)
    assert on.decode_stats["hip_prefix_prefills"] == 1 and on.decode_stats["hip_beam"] == 1


def test_default_switch_still_goes_to_hf_and_hf_agreement_is_reported(llm_small):
    hf, hip = make(llm_small), make(llm_small, beams="hip")
    img = image_embeds(16, 5)
    a = hf.generate_from_embeds(img, PROMPT)
    assert hf.decode_stats["hf_calls"] == 1 and hf.decode_stats["hf_fallback_kwargs"] == 1 and hf.decode_stats["hip_beam"] == 0
    b = hip.generate_from_embeds(img, PROMPT)
    same = sum(x == y for x, y in zip(a, b))
    # not asserted: fp16 rounding separates the two engines' logits; the parity chain is law = HF (CPU) and engine = law (above)
    print(f"[beam search, 4 beams, 6 tokens] {same} of 16 answers equal HF fp16 generate(num_beams=4) on the device", flush=True)
    one = make(llm_small, beams="hip", generate_kwargs={"num_beams": 1})      # one beam: the greedy entries, as before
    one.generate_from_embeds(img, PROMPT)
    assert one.decode_stats["hip_beam"] == 0 and one.decode_stats["graph_replays"] == 1 and one.decode_stats["hf_calls"] == 0
