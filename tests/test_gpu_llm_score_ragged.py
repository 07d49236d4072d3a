"""score="hip" with per-row prompts and per-row candidates (cgpt_llm_score_ragged: the RAGGED instantiations of csrc/llm_score.hip on
the cache of cgpt_llm_prefill_ragged).  The yardstick is the plain path itself: a padded row of a padded batch must give, bit for
bit, what cgpt_llm_prefill + cgpt_llm_score give for that row run alone and unpadded with its own tokens and lengths -- so the
accuracy tests of the plain entry (tests/test_gpu_llm_score.py) cover this one and no tolerance is introduced here.

Shapes: L = 70 with starts (0, 5, 6, 57, 69) -- real lengths 70, 65, 64, 13 and 1: two 64-key chunks, one key into the second chunk,
exactly one chunk, a short row, a single real token; candidate geometry T = (3, 1, 5, 2) with rows at full length, at length 1 on the
5-token candidate (four dead tail slots), and at T_c - 1."""
import copy
import ctypes as C
import dataclasses

import pytest
import torch

import certifiedgpt_amd as cg
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import (MiniGPT4Classifier, WordHashTokenizer, _HipDecoder, hip_decode_unsupported, int8_state_dict,
                                       pack_row_candidates, prepare_texts)
from oracle import model_oracle as mo
from gpu_util import DEV, make_classifier
import llm_util as lu
from llm_util import K_SENTINEL, V_SENTINEL

pytestmark = pytest.mark.gpu

EPS = 0.1
L_PAD = 70
STARTS = (0, 5, 6, 57, 69)
# LENS[b][c]: row 0 at full length everywhere (every T_c is reached), row 1 with one token of the 5-token candidate and T_c - 1 = 2 of
# the 3-token one, row 2 with T_c - 1 = 4 of the 5-token one
LENS = ((3, 1, 5, 2), (2, 1, 1, 2), (3, 1, 4, 1), (1, 1, 5, 2), (3, 1, 3, 1))
GEOMETRY = (3, 1, 5, 2)
INVALID, STATE = 1, 5


@pytest.fixture(scope="module")
def small():
    """hidden 512 = 4 heads x 128, MLP 1408, vocabulary 320, 2 layers."""
    llm = lu.llama_decoder(512, 4, 1408, 320, kv_heads=4)
    assert hip_decode_unsupported(llm, 200) == []
    dec = _HipDecoder(llm, 200)
    yield llm, dec
    dec.close()


def _padded_embeds(llm, starts, L, seed):
    """[B, L, hidden] with zeros on row b's pad positions 0 .. starts[b]-1, and the starts on the device."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    embs = llm.get_input_embeddings()(torch.randint(3, llm.config.vocab_size, (len(starts), L), generator=g).to(DEV)).contiguous()
    for b, s in enumerate(starts):
        embs[b, :s] = 0
    return embs, torch.tensor(starts, dtype=torch.int32, device=DEV)


def _row_candidates(vocab, lens, seed):
    """cand[c][b] = random tokens of lens[b][c]."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [[torch.randint(3, vocab, (lens[b][c],), generator=g) for b in range(len(lens))] for c in range(len(lens[0]))]


def _ragged_sums(dec, embs, starts, cand, extra=3, keep=False, table=None):
    B, L, _ = embs.shape
    kb, vb = lu.sentinel_cache(dec.layers, dec.kv_heads, B, L + extra)
    first = dec.prefill(embs, kb, vb, starts=starts)
    packed, lens, T, _ = pack_row_candidates(cand)
    table = (packed if table is None else table).to(DEV)
    lens = lens.to(DEV)
    sums = dec.score(first, L, table, T, EPS, kb, vb, starts=starts, row_lens=lens)
    torch.cuda.synchronize()
    return (sums, first, kb, vb, table, lens, T) if keep else sums


def _alone_sums(dec, embs, start, row_cands):
    """The existing plain path on ONE row, unpadded: cgpt_llm_prefill + cgpt_llm_score with the row's own tokens and lengths."""
    row = embs[:, start:].contiguous()
    L = row.shape[1]
    kb, vb = lu.sentinel_cache(dec.layers, dec.kv_heads, 1, L + 3)
    first = dec.prefill(row, kb, vb)
    lens = [len(t) for t in row_cands]
    table = torch.zeros((len(lens), max(lens)), dtype=torch.long)
    for c, t in enumerate(row_cands):
        table[c, :lens[c]] = t
    sums = dec.score(first, L, table.to(DEV), lens, EPS, kb, vb)
    torch.cuda.synchronize()
    return sums[0]


def _check_rows_alone(llm, dec, starts, lens, seed):
    embs, sdev = _padded_embeds(llm, starts, L_PAD, seed)
    cand = _row_candidates(320, lens, seed + 100)
    got = _ragged_sums(dec, embs, sdev, cand)
    assert tuple(got.shape) == (len(starts), len(lens[0])) and bool(torch.isfinite(got).all())
    for b, s in enumerate(starts):
        want = _alone_sums(dec, embs[b:b + 1], s, [cand[c][b] for c in range(len(cand))])
        assert torch.equal(got[b], want), (b, s, got[b].tolist(), want.tolist())
    return got


# ------------------------------------------------------------------------------------------ 1. a padded row is the row alone
def test_a_padded_row_is_the_row_alone_bit_for_bit(small):
    llm, dec = small
    assert [max(LENS[b][c] for b in range(5)) for c in range(4)] == list(GEOMETRY)
    got = _check_rows_alone(llm, dec, STARTS, LENS, 3)
    assert len({float(v) for v in got.flatten()}) == got.numel()       # and the sums are not one value


# ------------------------------------------------------------------------------------------ 2. no padding, uniform lengths
def test_zero_padding_and_uniform_lengths_equal_the_plain_entry_on_the_batch(small):
    llm, dec = small
    B = 5
    embs, sdev = _padded_embeds(llm, (0,) * B, L_PAD, 4)
    g = torch.Generator(device="cpu").manual_seed(18)
    shared = [torch.randint(3, 320, (n,), generator=g) for n in GEOMETRY]
    ragged = _ragged_sums(dec, embs, sdev, [[t] * B for t in shared])
    kb, vb = lu.sentinel_cache(dec.layers, dec.kv_heads, B, L_PAD + 3)
    first = dec.prefill(embs, kb, vb)
    table = torch.zeros((4, max(GEOMETRY)), dtype=torch.long)
    for c, t in enumerate(shared):
        table[c, :len(t)] = t
    plain = dec.score(first, L_PAD, table.to(DEV), list(GEOMETRY), EPS, kb, vb)
    torch.cuda.synchronize()
    assert torch.equal(ragged, plain) and bool(torch.isfinite(plain).all())


# ------------------------------------------------------------------------------------------ 3. grouped-query attention
def test_a_padded_row_is_the_row_alone_on_a_grouped_kv_handle():
    llm = lu.llama_decoder(512, 4, 1408, 320, kv_heads=2)
    assert hip_decode_unsupported(llm, 64, grouped_kv=True) == []
    dec = _HipDecoder(llm, 64, grouped_kv=True)
    try:
        assert dec.kv_heads == 2
        _check_rows_alone(llm, dec, (0, 6, 57), LENS[:3], 5)
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------ 4. the cache
def _bits(t):
    return t.view(torch.int16)


def test_nothing_below_start_is_read_and_nothing_is_written(small):
    llm, dec = small
    extra = 3
    embs, sdev = _padded_embeds(llm, STARTS, L_PAD, 6)
    cand = _row_candidates(320, LENS, 106)
    sums, first, kb, vb, table, lens, T = _ragged_sums(dec, embs, sdev, cand, extra=extra, keep=True)
    for t, sentinel in zip(kb + vb, [K_SENTINEL] * len(kb) + [V_SENTINEL] * len(vb)):
        assert bool((t[:, :, L_PAD:] == sentinel).all())               # rows behind the prompt: still the sentinel
        for b, s in enumerate(STARTS):
            t[b, :, :s] = float("nan")                                 # rows below start[b]: a NaN pattern
    torch.cuda.synchronize()
    before = [t.clone() for t in kb + vb]
    again = dec.score(first, L_PAD, table, T, EPS, kb, vb, starts=sdev, row_lens=lens)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(again).all()) and torch.equal(again, sums)
    assert all(torch.equal(_bits(t), _bits(was)) for t, was in zip(kb + vb, before))   # bitwise unchanged, sentinels and NaNs included
    for t, sentinel in zip(kb + vb, [K_SENTINEL] * len(kb) + [V_SENTINEL] * len(vb)):
        assert bool((t[:, :, L_PAD:] == sentinel).all())


# ------------------------------------------------------------------------------------------ 5. independence
def test_other_rows_their_candidates_and_dead_table_entries_do_not_change_a_single_bit(small):
    llm, dec = small
    embs, sdev = _padded_embeds(llm, STARTS, L_PAD, 7)
    cand = _row_candidates(320, LENS, 107)
    full = _ragged_sums(dec, embs, sdev, cand)
    assert torch.equal(full, _ragged_sums(dec, embs, sdev, cand))      # scoring twice
    # the rows permuted, with their starts, tokens and lengths
    perm = [3, 0, 4, 2, 1]
    idx = torch.tensor(perm, device=DEV)
    permuted = _ragged_sums(dec, embs[idx].contiguous(), sdev[idx].contiguous(), [[col[b] for b in perm] for col in cand])
    assert torch.equal(permuted, full[idx])
    # another row's candidate tokens
    g = torch.Generator(device="cpu").manual_seed(207)
    other = [[t.clone() for t in col] for col in cand]
    for c in range(4):
        other[c][1] = torch.randint(3, 320, (LENS[1][c],), generator=g)
    changed = _ragged_sums(dec, embs, sdev, other)
    keep = [0, 2, 3, 4]
    assert torch.equal(changed[keep], full[keep]) and not torch.equal(changed[1], full[1])
    # T_c raised by one other row: the one-token candidate of row 4 becomes three tokens, every row gains two tail slots
    longer = [[t.clone() for t in col] for col in cand]
    longer[1][4] = torch.cat([cand[1][4], torch.randint(3, 320, (2,), generator=g)])
    _, _, T, S = pack_row_candidates(longer)
    assert T == [3, 3, 5, 2] and S == sum(GEOMETRY) - 4 + 2
    raised = _ragged_sums(dec, embs, sdev, longer)
    assert torch.equal(raised[:4], full[:4]) and torch.equal(raised[4, [0, 2, 3]], full[4, [0, 2, 3]])
    assert not torch.equal(raised[4, 1], full[4, 1])
    # table entries past a row's real length: any ids, ids outside the vocabulary included
    table, lens, _, _ = pack_row_candidates(cand)
    noise = torch.randint(-5, 400, table.shape, generator=g)
    dead = torch.arange(table.shape[2])[None, None, :] >= lens[:, :, None]
    assert bool(dead.any())
    assert torch.equal(_ragged_sums(dec, embs, sdev, cand, table=torch.where(dead, noise, table)), full)


# ------------------------------------------------------------------------------------------ 6. int8
def test_int8_ragged_scoring_is_bit_for_bit_the_fp16_engine_on_the_dequantised_weights(small):
    llm, _ = small
    twin = copy.deepcopy(llm)
    twin.load_state_dict(int8_state_dict(llm))
    dec8, dec16 = _HipDecoder(llm, 200, weights="int8"), _HipDecoder(twin, 200)
    try:
        starts = (0, 6, 57)
        embs, sdev = _padded_embeds(llm, starts, L_PAD, 9)
        cand = _row_candidates(320, LENS[:3], 109)
        a, b = _ragged_sums(dec8, embs, sdev, cand), _ragged_sums(dec16, embs, sdev, cand)
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    finally:
        dec8.close()
        dec16.close()


# ------------------------------------------------------------------------------------------ 7. refusals
def test_the_ragged_entry_refuses_before_any_launch(small):
    llm, dec = small
    L = cg.lib()
    B, Lp = 4, 8
    embs, sdev = _padded_embeds(llm, (0, 2, 5, 7), Lp, 10)
    kb, vb = lu.sentinel_cache(dec.layers, dec.kv_heads, B, Lp)
    first = dec.prefill(embs, kb, vb, starts=sdev)
    cand = _row_candidates(320, ((2, 3), (1, 3), (2, 1), (2, 2)), 110)
    table, lens, T, _ = pack_row_candidates(cand)
    table, lens = table.to(DEV), lens.to(DEV)
    big = torch.zeros((B, 2, 40), dtype=torch.long, device=DEV)        # a table wide enough for the 68-tail-row geometry below
    out = torch.full((B, 2), 3.0, device=DEV)
    kp = (C.c_void_p * 2)(*[t.data_ptr() for t in kb])
    vp = (C.c_void_p * 2)(*[t.data_ptr() for t in vb])

    def score(h=None, B=B, Lp=Lp, starts=sdev, tab=table, dlens=lens, T=T, Tmax=3, k=kp, stride=Lp):
        h = dec.handle if h is None else h
        return L.cgpt_llm_score_ragged(h, C.c_void_p(first.data_ptr()), B, Lp, None if starts is None else C.c_void_p(starts.data_ptr()),
                                       C.c_void_p(tab.data_ptr()), None if dlens is None else C.c_void_p(dlens.data_ptr()),
                                       (C.c_int32 * len(T))(*T), len(T), Tmax, EPS, k, vp, stride, C.c_void_p(out.data_ptr()), None)

    assert L.cgpt_llm_score_reserve(dec.handle, 200, 8) == 0
    for status in (score(starts=None), score(dlens=None), score(tab=big, T=[40, 30], Tmax=40), score(T=[0, 3]), score(T=[2, 4]),
                   score(Lp=Lp + 1), score(B=201), score(B=0), score(k=None)):
        assert status == INVALID and L.cgpt_last_error()
    fresh = _HipDecoder(llm, 200)                                      # nothing reserved on this handle
    try:
        assert score(h=fresh.handle) == STATE and b"cgpt_llm_score_reserve" in L.cgpt_last_error()
        torch.cuda.synchronize()
    finally:
        fresh.close()
    assert bool((out == 3.0).all())                                    # nothing was launched
    assert score() == 0                                                # and a call inside every bound runs
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 3.0).any())


# ------------------------------------------------------------------------------------------ 8. the classifier
def test_per_row_prompts_and_candidates_stay_on_the_engine_and_match_the_models_forward(small):
    llm, _ = small
    cfg = dataclasses.replace(mo.tiny_config(mode=mo.MODE_ENCODE_IMG), proj_dim=512)
    enc = make_classifier(cfg, max_batch=16)
    enc.init_synthetic(seed=0)
    tok = WordHashTokenizer(320)
    short = prepare_texts(["<Img><ImageHere></Img> [vqa] what is shown in the picture"])[0]
    long_ = prepare_texts(["<Img><ImageHere></Img> [vqa] which of these animals is shown in the middle of the picture"])[0]
    texts = [short, long_, short, long_]
    # answers[c][b]: per-row texts and token counts; row 3's answer 0 is three tokens longer than the other rows' -- the divisor of
    # candidate 0 is Lmax + 5 - 1 for EVERY row (the reference pads on the right), which a per-row divisor misses by 3 / 25 of a loss
    answers = [["w5 w11", "w6 w12", "w7 w13", "w5 w11 w30 w31 w32"],
               ["w7", "w9 w8", "w7", "w21"],
               ["w9 w21 w33", "w9 w21", "w40", "w9 w21 w33"]]
    x = torch.from_numpy(mo.synthetic_image(cfg, seed=11)).to(DEV)
    images = cg.noise_batch(x, 0, 4, 0.5, 42)
    num_cand = [2, 3, 3, 1]

    def make(score):
        return MiniGPT4Classifier(enc, llm, tok, short, AnswerLabelMap(4, ["a", "b", "c"], frozen=True), max_batch=16, decode="hip",
                                  prefill="hip", ragged="hip", classify="multi_select", score=score)

    try:
        hip, hf = make("hip"), make("hf")
        emb, _ = enc.encode_img(images)
        lens = [len(tok(t.replace("<ImageHere>", " "), add_special_tokens=True).input_ids[0]) + emb.shape[1] for t in texts]
        assert lens[0] != lens[1] and max(lens) > 20                   # two prompt lengths; every divisor is Lmax + T_c - 1 > 20
        a = hip.answer_losses_from_embeds(emb, texts, answers)
        s = hip.decode_stats
        assert s["hip_ragged_scores"] == 1 and s["hf_score_fallbacks"] == 0 and s["hf_score_forwards"] == 0 and s["hip_scores"] == 0
        assert s["hip_prefills"] == 1
        b = hf.answer_losses_from_embeds(emb, texts, answers)
        assert hf.decode_stats["hf_score_forwards"] == 3 and hf.decode_stats["hip_ragged_scores"] == 0
        assert tuple(a.shape) == tuple(b.shape) == (4, 3) and bool(torch.isfinite(a).all())
        d = float((a - b).abs().max())
        top2 = (-b).topk(2, dim=1).values
        decisive = (top2[:, 0] - top2[:, 1]) > 2.0 * d
        same = a.argmin(dim=1) == b.argmin(dim=1)
        print(f"[ragged score classifier] prompt lengths {lens}, max |loss hip - hf| {d:.4g}, decisive rows {int(decisive.sum())}/4, same "
              f"top candidate on {int(same.sum())}/4; hf losses {b.tolist()}", flush=True)
        # the bound of tests/test_gpu_llm_score.py's classifier test: both engines' sums are within 1e-2 of the fp32 model at this size
        # and the divisor exceeds 20
        assert d < 2e-3, d
        assert int(decisive.sum()) >= 2 and bool(same[decisive].all())
        # multi_select with num_cand: the first num_cand[i] ranks are the model's own on rows whose live candidates are all 2 d apart
        ranks_hip = hip.multi_select(images, texts, answers, num_cand=num_cand)
        ranks_hf = hf.multi_select(images, texts, answers, num_cand=num_cand)
        assert hip.decode_stats["hip_ragged_scores"] == 2 and hip.decode_stats["hf_score_fallbacks"] == 0
        for i, n in enumerate(num_cand):
            assert sorted(ranks_hip[i][:n]) == list(range(n))          # the 9999 entries come last
            live = b[i, :n].sort().values
            if n == 1 or float((live[1:] - live[:-1]).min()) > 2.0 * d:
                assert ranks_hip[i][:n] == ranks_hf[i][:n], (i, ranks_hip[i], ranks_hf[i])
        # shared prompt and candidates without a bucket: the plain entry, whatever ragged says
        hip.answer_losses_from_embeds(emb, short, ["w5 w11", "w7"])
        assert hip.decode_stats["hip_scores"] == 1 and hip.decode_stats["hip_ragged_scores"] == 2
    finally:
        enc.close()
