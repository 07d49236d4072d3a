"""shared_prefix=True and the two entries under it (cgpt_llm_prefill_from: a prefill whose positions follow positions already in the
cache; cgpt_llm_kv_broadcast: a one-row prefix cache copied into every row).

Every comparison is EXACT.  The engine's invariant is that an element's bits do not depend on the kernel, the tiling or the batch it was
computed in, and the continuation attention tiles its queries by absolute position, so a
query meets the key chunks and the reduction order of the plain kernel.  A prefix prefilled once on one row, broadcast, and a suffix
prefilled on B x Ln rows must therefore give the logits, tokens and cache of the plain prefill of the whole prompt: `torch.equal`
against the plain entries on the same handle, no tolerance.  The shapes sit on both sides of the 16-query wave tile, the 64-query
block and the 64-key chunk of llm_prefill_attn_kernel."""
import pytest
import torch

from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import MiniGPT4Classifier, WordHashTokenizer, _HipDecoder, prepare_texts
from gpu_util import DEV
import llm_util as lu
from llm_util import PAD, EOS

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7E77                                                      # an fp16 quiet NaN with a payload: "never written, never read"


def _layers(llm):
    return llm.config.num_hidden_layers


def _kvh(dec):
    return dec.kv_heads


@pytest.fixture(scope="module")
def small():
    llm = lu.small_decoder()
    dec = _HipDecoder(llm, 64)
    yield llm, dec
    dec.close()


def _shared(llm, B, P, Ln, seed):
    """[B, P + Ln, hidden] whose first P positions are row 0's in every row."""
    e = lu.embeds(llm, B, P + Ln, seed)
    e[:, :P] = e[:1, :P]
    return e.contiguous()


def _plain(dec, llm, embs, extra=0, starts=None):
    B, L, _ = embs.shape
    kb, vb = lu.sentinel_cache(_layers(llm), _kvh(dec), B, L + extra)
    return dec.prefill(embs, kb, vb, starts=starts), kb, vb


def _prefix_cache(dec, llm, prefix):
    """One-row caches of `prefix` [1, P, hidden], by the plain prefill."""
    pk, pv = lu.sentinel_cache(_layers(llm), _kvh(dec), 1, prefix.shape[1])
    dec.prefill(prefix.contiguous(), pk, pv)
    return pk, pv


def _prefixed(dec, llm, prefix, suffix, extra=0, starts=None):
    """prefill(1, P) into a one-row cache -> kv_broadcast -> prefill_from(B, P, Ln)."""
    P, (B, Ln, _) = prefix.shape[1], suffix.shape
    pk, pv = _prefix_cache(dec, llm, prefix)
    kb, vb = lu.sentinel_cache(_layers(llm), _kvh(dec), B, P + Ln + extra)
    dec.kv_broadcast(pk, pv, P, kb, vb, starts=starts)
    return dec.prefill_from(suffix.contiguous(), P, kb, vb, starts=starts), kb, vb


def _same_caches(a, b, what):
    for l, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what}: layer {l} differs in {int((x != y).any(-1).sum())} cache rows"


def _assert_identity(dec, llm, B, P, Ln, seed=5):
    embs = _shared(llm, B, P, Ln, seed)
    want, wk, wv = _plain(dec, llm, embs, extra=2)
    got, gk, gv = _prefixed(dec, llm, embs[:1, :P], embs[:, P:], extra=2)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want).all())
    assert torch.equal(got, want), f"B {B}, P {P}, Ln {Ln}: logits differ, max {float((got - want).abs().max())}"
    _same_caches(gk, wk, f"B {B}, P {P}, Ln {Ln}: K")
    _same_caches(gv, wv, f"B {B}, P {P}, Ln {Ln}: V")


# ------------------------------------------------------------------------------------------ 0. refusals that need a handle
def test_both_entries_refuse_before_the_first_launch(small):
    """B outside 1..max_batch, pos0 + Ln > max_len, a reservation that is too small and missing weights: an error code, and the caches
    as they were -- every check runs before the first launch."""
    import ctypes as C
    from certifiedgpt_amd import _lib
    llm, dec = small
    L, P, Ln = dec.L, 4, 6
    INVALID, STATE = 1, 5                                              # CGPT_ERR_INVALID, CGPT_ERR_STATE

    def tables(B, length):
        kb, vb = lu.sentinel_cache(_layers(llm), _kvh(dec), B, length)
        kp = (C.c_void_p * dec.layers)(*[t.data_ptr() for t in kb])
        vp = (C.c_void_p * dec.layers)(*[t.data_ptr() for t in vb])
        return kb, vb, kp, vp

    def untouched(kb, vb):
        torch.cuda.synchronize()
        return all(bool((t == lu.K_SENTINEL).all()) for t in kb) and all(bool((t == lu.V_SENTINEL).all()) for t in vb)

    def prefill_from(h, B, pos0, n, kp, vp, stride, embs, out):
        return L.cgpt_llm_prefill_from(h, C.c_void_p(embs.data_ptr()), B, pos0, n, None, kp, vp, stride, C.c_void_p(out.data_ptr()),
                                       dec._stream())

    assert _lib.ERR_NAMES[INVALID] == "CGPT_ERR_INVALID" and _lib.ERR_NAMES[STATE] == "CGPT_ERR_STATE"
    out = torch.zeros(65, 320, dtype=torch.float32, device=DEV)
    embs = lu.embeds(llm, 65, Ln, 3)
    kb, vb, kp, vp = tables(65, P + Ln)
    skb, svb, skp, svp = tables(1, P)
    dec.prefill_from(embs[:2].contiguous(), P, [t[:2].clone() for t in kb], [t[:2].clone() for t in vb])    # reserves 64 x Ln rows, on copies
    for B in (0, -1, 65):                                              # max_batch = 64
        assert prefill_from(dec.handle, B, P, Ln, kp, vp, P + Ln, embs, out) == INVALID and b"max_batch" in L.cgpt_last_error()
        assert L.cgpt_llm_kv_broadcast(dec.handle, skp, svp, P, P, B, None, kp, vp, P + Ln, dec._stream()) == INVALID
        assert b"cgpt_llm_kv_broadcast" in L.cgpt_last_error()
    assert untouched(kb, vb)
    # pos0 + Ln > max_len, inside a cache that is long enough
    big_kb, big_vb, big_kp, big_vp = tables(1, dec.MAX_LEN + 8)
    assert prefill_from(dec.handle, 1, dec.MAX_LEN - 2, 3, big_kp, big_vp, dec.MAX_LEN + 8, embs, out) == INVALID
    assert b"max_len" in L.cgpt_last_error() and untouched(big_kb, big_vb)
    del big_kb, big_vb
    # a reservation that is too small: a fresh handle has none
    fresh = _HipDecoder(llm, 4)
    try:
        assert prefill_from(fresh.handle, 2, P, Ln, kp, vp, P + Ln, embs, out) == STATE and b"cgpt_llm_prefill_reserve" in L.cgpt_last_error()
        assert untouched(kb, vb)
    finally:
        fresh.close()
    # missing weights: a handle created from the same config, nothing loaded
    cfg = llm.config
    c = _lib.LlmConfig(struct_size=_lib.LLM_CONFIG_SIZE_F16, weight_format=0, device=0, hidden=cfg.hidden_size, layers=cfg.num_hidden_layers,
                       heads=cfg.num_attention_heads, kv_heads=cfg.num_attention_heads, head_dim=128, mlp=cfg.intermediate_size,
                       vocab=cfg.vocab_size, rms_eps=float(cfg.rms_norm_eps), rope_theta=10000.0, max_batch=4, max_len=256)
    empty = C.c_void_p()
    _lib.check(L.cgpt_llm_create(C.byref(c), C.byref(empty)))
    try:
        assert prefill_from(empty, 2, P, Ln, kp, vp, P + Ln, embs, out) == STATE and b"weights" in L.cgpt_last_error()
        assert untouched(kb, vb)
    finally:
        L.cgpt_llm_destroy(empty)


# ------------------------------------------------------------------------------------------ 1. identity
SHAPES = [(1, 1), (7, 37), (15, 1), (16, 16), (17, 47), (63, 1), (64, 1), (65, 20), (70, 230)]


@pytest.mark.parametrize("B", [3, 37])
@pytest.mark.parametrize("P, Ln", SHAPES)
def test_prefix_once_plus_suffix_equals_the_plain_prefill(small, B, P, Ln):
    llm, dec = small
    _assert_identity(dec, llm, B, P, Ln)


# ------------------------------------------------------------------------------------------ 2. continuation alone
@pytest.mark.parametrize("chunks", [(5, 60, 70), (64, 64, 1)])
def test_a_prompt_prefilled_in_chunks_equals_the_prompt_prefilled_at_once(small, chunks):
    llm, dec = small
    B, L = 5, sum(chunks)
    embs = lu.embeds(llm, B, L, 11)                                    # rows that differ everywhere
    want, wk, wv = _plain(dec, llm, embs, extra=1)
    kb, vb = lu.sentinel_cache(_layers(llm), _kvh(dec), B, L + 1)
    got = dec.prefill(embs[:, :chunks[0]].contiguous(), kb, vb)
    pos = chunks[0]
    for n in chunks[1:]:
        got = dec.prefill_from(embs[:, pos:pos + n].contiguous(), pos, kb, vb)
        pos += n
    torch.cuda.synchronize()
    assert torch.equal(got, want), float((got - want).abs().max())
    _same_caches(kb, wk, f"{chunks}: K")
    _same_caches(vb, wv, f"{chunks}: V")


# ------------------------------------------------------------------------------------------ 3. written rows only
def _nan_caches(layers, kvh, B, length):
    """Caches of NaN_BITS inside flat allocations with one guard row of B on either side: (k views, v views, flat buffers)."""
    flat = [torch.full((B + 2, kvh, length, 128), NAN_BITS, dtype=torch.int16, device=DEV).view(torch.float16) for _ in range(2 * layers)]
    views = [f[1:B + 1] for f in flat]
    return views[:layers], views[layers:], flat


def _untouched(t):
    return (t.view(torch.int16) == NAN_BITS).all(-1)                   # [.., rows]: the row still holds the pattern


def test_prefill_from_and_broadcast_write_their_rows_and_no_other(small):
    llm, dec = small
    B, P, Ln, length = 3, 7, 37, 50
    embs = _shared(llm, B, P, Ln, 9)
    pk, pv = _prefix_cache(dec, llm, embs[:1, :P])
    starts = torch.tensor([0, 2, 5], dtype=torch.int32, device=DEV)
    for st in (None, starts):
        off = [0] * B if st is None else st.tolist()
        kb, vb, flat = _nan_caches(_layers(llm), _kvh(dec), B, length)
        dec.kv_broadcast(pk, pv, P, kb, vb, starts=st)
        torch.cuda.synchronize()
        for t, src in zip(kb + vb, pk + pv):
            for b in range(B):
                clean = _untouched(t[b])
                assert not bool(clean[:, off[b]:off[b] + P].any()) and torch.equal(t[b, :, off[b]:off[b] + P], src[0, :, :P])
                assert bool(clean[:, :off[b]].all()) and bool(clean[:, off[b] + P:].all()), "kv_broadcast wrote outside its rows"
        before = [t.clone() for t in kb + vb]
        suffix = embs[:, P:].clone()
        for b in range(B):
            suffix[b, :off[b]] = 0
        logits = dec.prefill_from(suffix.contiguous(), P, kb, vb, starts=st)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(logits).all())                      # no NaN row of the cache was read
        for t, was in zip(kb + vb, before):
            for b in range(B):
                lo = P + off[b]
                assert torch.equal(t[b, :, :lo].view(torch.int16), was[b, :, :lo].view(torch.int16)), "prefill_from wrote below pos0"
                assert not bool(_untouched(t[b, :, lo:P + Ln]).any())
                assert bool(_untouched(t[b, :, P + Ln:]).all()), "prefill_from wrote past pos0 + Ln - 1"
        for f in flat:
            assert bool(_untouched(f[0]).all()) and bool(_untouched(f[-1]).all()), "a guard region was written"


# ------------------------------------------------------------------------------------------ 4. ragged
def _ragged_case(llm, P, Ls, starts, seed):
    """(prefix [1, P], suffix buffer [B, Ls] left-padded by starts, whole prompt [B, P + Ls] left-padded by the same starts)."""
    B = len(starts)
    prefix = lu.embeds(llm, 1, P, seed)
    real = lu.embeds(llm, B, Ls, seed + 1)
    suffix, whole = torch.zeros_like(real), torch.zeros((B, P + Ls, real.shape[2]), dtype=real.dtype, device=DEV)
    for b, s in enumerate(starts):
        suffix[b, s:] = real[b, s:]
        whole[b, s:s + P] = prefix[0]
        whole[b, s + P:] = real[b, s:]
    return prefix, suffix.contiguous(), whole.contiguous()


def test_ragged_suffix_on_a_shared_prefix_equals_the_ragged_prefill(small):
    llm, dec = small
    P, Ls, starts = 7, 73, [0, 1, 8, 9, 56, 72]                        # real suffix lengths 73, 72, 65, 64, 17, 1
    prefix, suffix, whole = _ragged_case(llm, P, Ls, starts, 21)
    st = torch.tensor(starts, dtype=torch.int32, device=DEV)
    want, wk, wv = _plain(dec, llm, whole, extra=1, starts=st)
    got, gk, gv = _prefixed(dec, llm, prefix, suffix, extra=1, starts=st)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want).all())
    assert torch.equal(got, want), float((got - want).abs().max())
    for l in range(_layers(llm)):
        for b, s in enumerate(starts):
            assert torch.equal(gk[l][b, :, s:], wk[l][b, :, s:]) and torch.equal(gv[l][b, :, s:], wv[l][b, :, s:]), (l, b)
            assert bool((gk[l][b, :, :s] == lu.K_SENTINEL).all()) and bool((gv[l][b, :, :s] == lu.V_SENTINEL).all()), (l, b)


def test_out_of_range_starts_behave_as_their_clamped_values(small):
    """prefill_from clamps into 0 .. Ln-1 (as the ragged prefill clamps into 0 .. L-1); the broadcast, which is not told Ln, into
    0 .. dst_len_stride - P.  Each is compared with itself on the clamped values."""
    llm, dec = small
    P, Ls = 7, 20
    prefix, suffix, _ = _ragged_case(llm, P, Ls, [0, Ls - 1, 3], 23)
    pk, pv = _prefix_cache(dec, llm, prefix)

    def i32(v):
        return torch.tensor(v, dtype=torch.int32, device=DEV)

    def broadcast(starts):
        kb, vb = lu.sentinel_cache(_layers(llm), _kvh(dec), 3, P + Ls)
        dec.kv_broadcast(pk, pv, P, kb, vb, starts=i32(starts))
        return kb, vb

    wild, clamped = broadcast([-5, 1000, 3]), broadcast([0, Ls, 3])    # dst_len_stride - P = Ls
    torch.cuda.synchronize()
    _same_caches(wild[0] + wild[1], clamped[0] + clamped[1], "kv_broadcast")
    runs = []
    for starts in ([-5, 1000, 3], [0, Ls - 1, 3]):
        kb, vb = broadcast([0, Ls - 1, 3])                             # the prefix where the continuation's clamped starts look for it
        runs.append((dec.prefill_from(suffix, P, kb, vb, starts=i32(starts)), kb, vb))
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0], runs[1][0]) and bool(torch.isfinite(runs[0][0]).all())
    _same_caches(runs[0][1] + runs[0][2], runs[1][1] + runs[1][2], "prefill_from")


# ------------------------------------------------------------------------------------------ 5. downstream
def test_greedy_and_sample_after_the_prefix_path_give_the_plain_tokens(small):
    llm, dec = small
    B, P, Ln, n = 6, 7, 37, 8
    embs = _shared(llm, B, P, Ln, 13)
    settings = (True, 1.0, 50, 0.9, 1.05)
    draw = torch.arange(B, dtype=torch.int64, device=DEV)
    seed = torch.tensor([1234567], dtype=torch.int64, device=DEV)

    def run(path, decode):
        first, kb, vb = (_plain(dec, llm, embs, extra=n) if path == "plain" else _prefixed(dec, llm, embs[:1, :P], embs[:, P:], extra=n))
        if decode == "greedy":
            return dec.greedy(first, P + Ln, n, 1, [EOS], PAD, kb, vb), kb, vb
        return dec.sample(first, P + Ln, n, 1, [EOS], PAD, kb, vb, settings, draw, seed), kb, vb

    free, _, _ = run("plain", "greedy")
    stop = [free[0, 2:4].tolist()]                                     # a sequence row 0 emits: it finishes there
    dec.set_stop_sequences(stop)
    dec.set_early_stop(True)
    try:
        want, wk, wv = run("plain", "greedy")
        got, gk, gv = run("prefix", "greedy")
        torch.cuda.synchronize()
        assert bool((want[0, 4:] == PAD).all()), "the stop sequence did not fire: the case shows nothing"
        assert torch.equal(got, want)
        _same_caches(gk, wk, "greedy K")
        _same_caches(gv, wv, "greedy V")
    finally:
        dec.set_early_stop(False)
        dec.set_stop_sequences(None)
    want, _, _ = run("plain", "sample")
    got, _, _ = run("prefix", "sample")
    torch.cuda.synchronize()
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------ 6. other handles
@pytest.mark.parametrize("kind", ["grouped_kv G=2", "grouped_kv G=4", "weights int8", "activations int8"])
def test_identity_on_grouped_and_int8_handles(kind):
    if kind.startswith("grouped_kv"):
        llm = lu.llama_decoder(512, 4, 1408, 320, kv_heads=4 // int(kind[-1]))
        dec = _HipDecoder(llm, 8, grouped_kv=True)
    elif kind == "weights int8":
        llm = lu.small_decoder()
        dec = _HipDecoder(llm, 8, weights="int8")
    else:
        llm = lu.small_decoder()
        dec = _HipDecoder(llm, 8, weights="int8", activations="int8", outlier_cap=1024)
    try:
        _assert_identity(dec, llm, 5, 7, 37)
        if kind == "activations int8":
            assert dec.act_stats()["overflow_rows"] == 0
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------ 7. graphs
def test_a_captured_prefix_path_replays_and_follows_the_prefix_it_is_given(small):
    llm, dec = small
    B, P, Ln = 4, 7, 37
    embs = _shared(llm, B, P, Ln, 17)
    other = lu.embeds(llm, 1, P, 18)                                   # another prefix of the same length
    suffix = embs[:, P:].contiguous()
    caches = {"a": _prefix_cache(dec, llm, embs[:1, :P]), "b": _prefix_cache(dec, llm, other)}

    def eager(name):
        kb, vb = lu.sentinel_cache(_layers(llm), _kvh(dec), B, P + Ln)
        dec.kv_broadcast(*caches[name], P, kb, vb)
        return dec.prefill_from(suffix, P, kb, vb), kb, vb

    want = {name: eager(name) for name in caches}                      # also the eager run that reserves the workspace
    sk, sv = [t.clone() for t in caches["a"][0]], [t.clone() for t in caches["a"][1]]       # the static tensors the graph reads
    kb, vb = lu.sentinel_cache(_layers(llm), _kvh(dec), B, P + Ln)
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            dec.kv_broadcast(sk, sv, P, kb, vb)
            out = dec.prefill_from(suffix, P, kb, vb)
    seen = []
    for name in ("a", "a", "b", "a"):
        for dst, src in zip(sk + sv, caches[name][0] + caches[name][1]):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        seen.append((out.clone(), [t.clone() for t in kb], [t.clone() for t in vb]))
        assert torch.equal(out, want[name][0]), name
        _same_caches(kb, want[name][1], f"replay {name}: K")
        _same_caches(vb, want[name][2], f"replay {name}: V")
    assert torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][0], seen[3][0])
    assert not torch.equal(seen[0][0], seen[2][0])


# ------------------------------------------------------------------------------------------ 8. Vicuna width
def test_identity_at_vicuna_width_200_rows():
    """The prefix (7 token rows) goes through the small-shape GEMM kernel, the suffix (7 400 rows) through the large-shape one."""
    llm = lu.vicuna_width_decoder()
    dec = _HipDecoder(llm, 200)
    try:
        _assert_identity(dec, llm, 200, 7, 37)
    finally:
        dec.close()
        del llm
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------ 9. classifier
QUESTIONS = ["what is shown", "what is shown in the picture", "is there a dog or a cat in this picture",
             "how many people are there in the picture and what are they doing now"]
PROMPTS = prepare_texts(["<Img><ImageHere></Img> [vqa] " + q for q in QUESTIONS])      # one first segment: "<s>[INST] <Img>"
OTHER = "<s>[INST] look here <Img><ImageHere></Img> [vqa] what is shown [/INST]"        # another first segment


def _img_embeds(B, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(B, 32, 512, generator=g) * 0.02).to(DEV).to(torch.float16)


def _pair(llm, **kw):
    """The same classifier without and with the flag, and the token tables their graphs returned."""
    out = []
    for flag in (False, True):
        clf = MiniGPT4Classifier(None, llm, WordHashTokenizer(320), PROMPTS[1], AnswerLabelMap(4, ()), max_new_tokens=8, max_batch=8,
                                 decode="hip", prefill="hip", shared_prefix=flag, **kw)
        seen, inner = [], clf._generate_graph
        clf._generate_graph = lambda *a, seen=seen, inner=inner: seen.append(inner(*a)) or seen[-1]
        out.append((clf, seen))
    return out


@pytest.mark.parametrize("kw", [dict(), dict(ragged="hip"), dict(ragged="hip", prompt_bucket=16)], ids=["plain", "ragged", "bucket16"])
def test_classifier_with_the_flag_returns_the_tokens_without_it(small, kw):
    llm, _ = small
    (off, off_seen), (on, on_seen) = _pair(llm, **kw)
    emb = _img_embeds(4, 3)
    calls = [PROMPTS[1], PROMPTS[2]]                                   # shared prompts (two lengths: one bucket under prompt_bucket=16)
    if kw:
        calls.append(list(PROMPTS))                                    # four per-row texts with one first segment
    for texts in calls:
        assert on.generate_from_embeds(emb, texts) == off.generate_from_embeds(emb, texts)
    assert len(on_seen) == len(off_seen) == len(calls)
    for a, b in zip(on_seen, off_seen):
        assert torch.equal(a, b)
    s = on.decode_stats
    assert s["hf_calls"] == 0 and s["hip_prefix_prefills"] == 1 and s["hip_prefix_hits"] == len(calls) - 1, s
    assert off.decode_stats["hip_prefix_prefills"] == 0 and off.decode_stats["hip_prefix_hits"] == 0
    assert s["graph_captures"] == off.decode_stats["graph_captures"]  # the flag adds no graph: one per bucket stays one per bucket
    if kw:                                                             # rows with different first segments take the old path
        mixed = [PROMPTS[0], OTHER, PROMPTS[2], PROMPTS[3]]
        before = dict(s)
        assert on.generate_from_embeds(emb, mixed) == off.generate_from_embeds(emb, mixed)
        assert torch.equal(on_seen[-1], off_seen[-1])
        assert s["hip_prefix_prefills"] == before["hip_prefix_prefills"] and s["hip_prefix_hits"] == before["hip_prefix_hits"]
        assert not any("prefix" in key for key in list(on._graphs)[-1:])


def test_one_template_is_prefilled_once_and_another_prefix_refreshes_the_graph(small):
    llm, _ = small
    (off, _), (on, _) = _pair(llm)
    embs = [_img_embeds(4, s) for s in (5, 6, 7)]
    want = [off.generate_from_embeds(e, PROMPTS[1]) for e in embs]
    assert [on.generate_from_embeds(e, PROMPTS[1]) for e in embs] == want
    s = on.decode_stats
    assert s["hip_prefix_prefills"] == 1 and s["hip_prefix_hits"] == 2 and s["graph_captures"] == 1 and s["graph_replays"] == 3, s
    # another first segment of the same token count: the same graph, its static prefix refreshed; then back
    a = "<s>[INST] <Img><ImageHere></Img> [vqa] what is shown in the picture [/INST]"
    b = "<s>[USER] <Img><ImageHere></Img> [vqa] what is shown in the picture [/INST]"
    for text in (a, b, a):
        assert on.generate_from_embeds(embs[0], text) == off.generate_from_embeds(embs[0], text), text
    assert s["graph_captures"] == 1 and s["hip_prefix_prefills"] == 2, s


def test_certify_gives_the_same_label_and_radius_with_the_flag(small):
    import dataclasses
    import certifiedgpt_amd as cg
    from oracle import model_oracle as mo
    from gpu_util import make_classifier
    llm, _ = small
    cfg = dataclasses.replace(mo.tiny_config(mode=mo.MODE_ENCODE_IMG), proj_dim=512)
    enc = make_classifier(cfg, max_batch=100)
    try:
        enc.init_synthetic(seed=0)
        x = torch.from_numpy(mo.synthetic_image(cfg, seed=11)).to(DEV)
        tok = WordHashTokenizer(320)
        kw = dict(max_new_tokens=4, max_batch=100, decode="hip", prefill="hip")
        probe = MiniGPT4Classifier(enc, llm, tok, PROMPTS[1], AnswerLabelMap(6, ()), **kw)
        import collections
        answers = probe.generate_from_embeds(enc.encode_img_noisy(x, 0, 100, 0.25, 7).to(torch.float16), PROMPTS[1])
        words = [w for w, _ in collections.Counter(answers).most_common(5)]
        got = []
        for flag in (False, True):
            clf = MiniGPT4Classifier(enc, llm, tok, PROMPTS[1], AnswerLabelMap(6, words), shared_prefix=flag, **kw)
            s = cg.Smooth(clf, 6, 0.25, seed=7, non_certifiable=(clf.label_map.other_id,))
            got.append(s.certify(x, 100, 100, 0.05, 100))
            assert clf.decode_stats["hip_prefix_prefills"] == int(flag) and clf.decode_stats["hf_calls"] == 0
        assert got[0] == got[1], got
    finally:
        enc.close()
