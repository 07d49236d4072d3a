"""Sampled decoding on the native LLaMA engine (sample="hip"; cgpt_llm_sample*, csrc/llm_sample.hip).

The oracle is `sample_token_law` / `sample_uniform` (certifiedgpt_amd/llm_laws.py, pinned to transformers' own processors and to
oracle.philox on the CPU by tests/test_llm_sample_cpu.py):
  * the uniforms are bit-equal to `sample_uniform` (24 bits, exact in fp32);
  * cases whose every decision has a margin >= 0.02 give the law's token exactly;
  * in general a row passes the MARGIN RULE (`_margin_rule`): with the float64 kept set, u * kept_mass lies inside its token's float64
    CDF interval widened by EPS on both sides; where a float64 cumulative mass at the top-p cut lies within EPS of top_p either
    neighbouring kept set may be used.  Every row must pass; rows whose float64 margin is below EPS ("indecisive") are counted and
    must stay rare, and every decisive row's kept count is the float64 one.
  * EPS = 4 x MASS_ERR, MASS_ERR = the largest relative error of the kernel's kept mass against float64 measured over the inputs
    of test 3 on an MI355X (the figure is asserted there; DESIGN.md 4.4.10 records it).  The kernel's weights and
    sums are float64 (llm_sample.hip states why, and the order), so the figure is the fp32 rounding of the reported mass; the factor 4
    covers the kept mass, the CDF partials and the product u * mass.  EPS <= 1e-5 whatever is measured.
  * on the engine: tokens are a function of (row, draw id, seed) -- partitions, graph replays, padding and twins are compared bit
    for bit -- and every token passes the margin rule on the logits its select saw and on the row's own earlier tokens."""
import collections
import copy
import ctypes as C
import dataclasses

import pytest
import torch

from certifiedgpt_amd import _lib
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import (MiniGPT4Classifier, WordHashTokenizer, _HipDecoder, apply_stop_sequences, expand_kv_state_dict,
                                       int8_state_dict, sample_token_law, sample_uniform, stop_finish_columns)
from gpu_util import DEV, make_classifier
import llm_util as lu
from llm_util import PROMPT
from oracle import model_oracle as mo

pytestmark = pytest.mark.gpu

CHAT = (True, 1.0, 50, 0.9, 1.05)            # Chat.answer_prepare's settings with HF's default top_k
COOL = (True, 0.7, 0, 0.9, 1.0)
CHAT_KW = dict(do_sample=True, top_p=0.9, repetition_penalty=1.05, temperature=1.0)
MASS_ERR = 5e-8                              # measured on an MI355X over test 3's inputs: 4.9e-8, at V 32000 / sigma 2 / "chat"
EPS = 4 * MASS_ERR
SEED = 0x9E3779B97F4A7C15                    # a seed with both key words in use


def _i64(seed):
    seed &= 0xFFFFFFFFFFFFFFFF
    return seed - (1 << 64) if seed >= 1 << 63 else seed


def _seed_dev(seed):
    return torch.tensor([_i64(seed)], dtype=torch.int64, device=DEV)


def _raw(logits, settings, prev=None, step=0, eos=(), mask_eos=False, pad=0, unfinished=None, ids=None, seed=0, uniforms=None):
    """cgpt_llm_sample_logits on logits [B, V] fp32 (device) -> dict(tokens, u, kept, mass, unfinished)."""
    L = _lib.lib()
    B, V = logits.shape
    assert logits.dtype == torch.float32 and logits.is_cuda and logits.is_contiguous()
    tokens = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    u_out = torch.full((B,), -1.0, dtype=torch.float32, device=DEV)
    kept = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    mass = torch.full((B,), -1.0, dtype=torch.float32, device=DEV)
    unf = torch.ones(B, dtype=torch.int32, device=DEV) if unfinished is None else unfinished.to(DEV, torch.int32).contiguous()
    prev = None if prev is None else prev.to(DEV, torch.int64).contiguous()
    ids = torch.arange(B, dtype=torch.int64, device=DEV) if ids is None else ids.to(DEV, torch.int64).contiguous()
    sd = _seed_dev(seed)
    uin = None if uniforms is None else torch.as_tensor(uniforms, dtype=torch.float32).to(DEV).contiguous()
    eos_arr = (C.c_int64 * max(1, len(eos)))(*eos)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.cgpt_llm_sample_logits(ptr(logits), V, B, V, ptr(prev), 0 if prev is None else prev.shape[1], 0 if prev is None else prev.shape[1],
                                  int(step), int(mask_eos), eos_arr, len(eos), int(pad), ptr(unf), _lib.sample_params(*settings), ptr(ids),
                                  ptr(sd), ptr(uin), ptr(tokens), ptr(u_out), ptr(kept), ptr(mass),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.cgpt_last_error()
    torch.cuda.synchronize()
    return dict(tokens=tokens.cpu(), u=u_out.cpu(), kept=kept.cpu(), mass=mass.cpu(), unfinished=unf.cpu())


def _margin_rule(logits, prev, u, token, settings, eps, mask_eos_ids=()):
    """The margin rule of the module docstring for one row: (passes, decisive, float64 kept count, float64 kept mass)."""
    _, T, top_k, top_p, pen = settings
    d = sample_token_law(logits, prev, u, T, top_k, top_p, pen, mask_eos_ids=mask_eos_ids, details=True)
    p, n, srt, cum = d["p"], d["n"], d["sorted_p"], d["cum"]
    cut_margin = float("inf")
    sets = [d["kept"]]
    if n is not None:
        # the cut falls in the group of values equal to p_(n), sorted places lo .. hi: the law keeps the whole group, so the masses
        # that decide are the cumulative ones at the group's two ends.  Where one is within eps of top_p the neighbouring set counts too.
        group = torch.nonzero(srt == srt[n - 1])
        lo, hi = int(group[0]), int(group[-1])
        reach, before = float(cum[hi]) - top_p, top_p - (float(cum[lo - 1]) if lo else 0.0)
        cut_margin = min(reach, before)
        if reach < eps and hi + 1 < srt.numel() and float(srt[hi + 1]) > 0:
            sets.append(p >= srt[hi + 1])
        if before < eps and lo:
            sets.append(p >= srt[lo - 1])
    ok, cdf_margin = False, None
    for k, kept in enumerate(sets):
        if not bool(kept[token]):
            continue
        pk = torch.where(kept, p, torch.zeros((), dtype=p.dtype))
        cdf = torch.cumsum(pk, 0)
        target = u * float(pk.sum())
        lo, hi = (float(cdf[token - 1]) if token else 0.0), float(cdf[token])
        ok = ok or lo - eps <= target < hi + eps
        if k == 0:
            cdf_margin = min(target - lo, hi - target)
    if cdf_margin is None:                                             # the token is outside the float64 kept set
        cdf_margin = -1.0
    return ok, min(cdf_margin, cut_margin) >= eps, int(d["kept"].sum()), d["kept_mass"]


# ------------------------------------------------------------------------------------------ 1. the stream
@pytest.mark.parametrize("B", [3, 200])
def test_uniforms_are_bit_equal_to_the_law(B):
    logits = torch.zeros((B, 64), dtype=torch.float32, device=DEV)
    for first in (0, 2 ** 32 - 1):                                     # the second range carries into the high id word
        ids = torch.arange(first, first + B, dtype=torch.int64)
        for step in (0, 19):
            got = _raw(logits, (True, 1.0, 0, 1.0, 1.0), step=step, ids=ids, seed=SEED)["u"]
            want = torch.tensor([sample_uniform(SEED, first + b, step) for b in range(B)], dtype=torch.float64)
            assert torch.equal(got.to(torch.float64), want), (first, step)
            assert bool(((want >= 0) & (want < 1)).all()) and want.unique().numel() == B


# ------------------------------------------------------------------------------------------ 2. exact cases
def _dyadic(V):
    return torch.log(torch.tensor([2.0 ** -(i + 1) for i in range(V - 1)] + [2.0 ** -(V - 1)], dtype=torch.float64)).float()


@pytest.mark.parametrize("V", [64, 320])
def test_dyadic_probabilities_keep_four_and_invert_the_cdf(V):
    row = _dyadic(V)
    # top_p = 0.9: 1/2 + 1/4 + 1/8 = 0.875 < 0.9 <= 0.9375: four kept, of masses 8, 4, 2, 1 sixteenths; u at each kept interval's midpoint
    for perm_seed in (None, 5):                                        # in index order, and with the columns scattered over the row
        perm = torch.arange(V) if perm_seed is None else torch.randperm(V, generator=torch.Generator().manual_seed(perm_seed))
        logits = torch.empty(V)
        logits[perm] = row
        weight = {int(perm[i]): 2.0 ** -(i + 1) for i in range(4)}
        want = sorted(weight)                                          # the walk is in index order
        mids, acc = [], 0.0
        for j in want:
            mids.append((acc + weight[j] / 2) / 0.9375)
            acc += weight[j]
        assert min(weight.values()) / 2 / 0.9375 >= 0.02               # every u is that far from an interval's end
        got = _raw(logits.repeat(4, 1).to(DEV).contiguous(), (True, 1.0, 0, 0.9, 1.0), uniforms=mids)
        assert got["kept"].tolist() == [4] * 4
        assert torch.allclose(got["mass"], torch.full((4,), 0.9375), rtol=1e-6, atol=0)
        assert got["tokens"].tolist() == want
        assert got["tokens"].tolist() == [sample_token_law(logits, [], m, 1.0, 0, 0.9)[0] for m in mids]


def test_dominant_token_top_k_1_finished_rows_and_the_eos_mask():
    V = 320
    g = torch.Generator().manual_seed(1)
    base = torch.randn(6, V, generator=g).to(torch.float16).float()
    base[:, 17] = 30.0                                                 # dominant: everything else has mass < 1e-10
    got = _raw(base.to(DEV), (True, 1.0, 0, 0.9, 1.0), uniforms=[0.0, 0.3, 0.5, 0.7, 0.99, 0.999])
    assert got["tokens"].tolist() == [17] * 6 and got["kept"].tolist() == [1] * 6
    rows = torch.randn(6, V, generator=g).to(torch.float16).float()
    for b in range(6):
        rows[b, 50 * b + 7] = 6.0                                      # top_k = 1: the maximum, whatever u
    top = rows.argmax(1)
    assert top.tolist() == [50 * b + 7 for b in range(6)]
    assert bool((rows.sort(1).values[:, -1] - rows.sort(1).values[:, -2] >= 0.02).all())
    got = _raw(rows.to(DEV), (True, 1.0, 1, 1.0, 1.0), uniforms=[0.0, 0.2, 0.4, 0.6, 0.8, 0.999])
    assert got["tokens"].tolist() == top.tolist() and got["kept"].tolist() == [1] * 6
    # finished rows get the pad id and stay finished; a row that draws an EOS id finishes
    unf = torch.tensor([1, 0, 1, 0, 1, 1])
    got = _raw(base.to(DEV), (True, 1.0, 0, 0.9, 1.0), uniforms=[0.5] * 6, unfinished=unf, pad=7, eos=(17,))
    assert got["tokens"].tolist() == [17, 7, 17, 7, 17, 17] and got["unfinished"].tolist() == [0] * 6
    # the EOS columns read as -inf while the mask holds: the runner-up is drawn, and the row stays unfinished
    two = base.clone()
    two[:, 40] = 20.0
    got = _raw(two.to(DEV), (True, 1.0, 0, 0.9, 1.0), uniforms=[0.5] * 6, eos=(17, 3), mask_eos=True, pad=7)
    assert got["tokens"].tolist() == [40] * 6 and got["unfinished"].tolist() == [1] * 6 and got["kept"].tolist() == [1] * 6
    got = _raw(two.to(DEV), (True, 1.0, 0, 0.9, 1.0), uniforms=[0.5] * 6, eos=(17, 3), mask_eos=False, pad=7)
    assert got["tokens"].tolist() == [17] * 6 and got["unfinished"].tolist() == [0] * 6


def test_repetition_penalty_flips_the_arg_max_without_sampling():
    V, pen = 320, 1.5
    rows = torch.full((4, V), -3.0)
    rows[0, 5], rows[0, 9] = 2.0, 1.5          # positive: 2.0 / 1.5 = 1.33 < 1.5 -> 9
    rows[1, 5], rows[1, 9] = -1.0, -1.4        # negative: -1.0 * 1.5 = -1.5 < -1.4 -> 9
    rows[2, 5], rows[2, 9] = 2.0, 1.0          # a repeated id is penalised ONCE: 1.33 > 1.0 -> 5 (twice would be 0.89 -> 9)
    rows[3, 5], rows[3, 9] = 2.0, 1.5          # no earlier token is the leader: 5 stays
    prev = torch.tensor([[5, 7, 7], [5, 5, 300], [5, 5, 5], [7, 8, 300]])
    got = _raw(rows.to(DEV), (False, 1.0, 50, 0.9, pen), prev=prev)
    assert got["tokens"].tolist() == [9, 9, 5, 5]
    want = [sample_token_law(rows[b], prev[b], 0.0, repetition_penalty=pen, do_sample=False, dtype=torch.float32)[0] for b in range(4)]
    assert got["tokens"].tolist() == want
    # bit-equal to the fp32 torch law on natural rows, ties included (first maximum)
    g = torch.Generator().manual_seed(2)
    nat = torch.randn(37, V, generator=g).to(torch.float16).float()
    pv = torch.stack([nat[b].topk(3).indices for b in range(37)])       # the leaders themselves are penalised
    got = _raw(nat.to(DEV), (False, 1.0, 0, 1.0, 1.3), prev=pv)
    want = [sample_token_law(nat[b], pv[b], 0.0, repetition_penalty=1.3, do_sample=False, dtype=torch.float32)[0] for b in range(37)]
    assert got["tokens"].tolist() == want and want != nat.argmax(1).tolist()


def test_llama3_vocabulary_does_not_fit_in_lds():
    V = 128256
    g = torch.Generator().manual_seed(3)
    rows = (torch.randn(2, V, generator=g) * 0.5).to(torch.float16).float()
    rows[0, 128255] = 12.0                                             # the last column of the last chunk
    rows[1, 70000], rows[1, 128000] = 11.0, 11.0 + 0.6931471805599453     # masses 1/3 and 2/3 of what matters
    got = _raw(rows.to(DEV), (True, 1.0, 50, 0.9, 1.0), uniforms=[0.5, 0.2])
    assert got["tokens"].tolist() == [128255, 70000]
    got = _raw(rows.to(DEV), (True, 1.0, 50, 0.9, 1.0), uniforms=[0.5, 0.6])
    assert got["tokens"].tolist() == [128255, 128000]
    for b, u in ((0, 0.5), (1, 0.6)):
        tok, kept = sample_token_law(rows[b], [], u, 1.0, 50, 0.9)
        assert tok == got["tokens"][b] and int(kept.sum()) == int(got["kept"][b])


# ------------------------------------------------------------------------------------------ 3. the margin rule
@pytest.fixture(scope="module")
def mass_errors():
    return {}


@pytest.mark.parametrize("settings", [CHAT, COOL], ids=["chat", "cool"])
@pytest.mark.parametrize("V, B, sigma", [(32000, 200, 0.5), (32000, 200, 2.0), (320, 37, 1.0)])
def test_margin_rule(V, B, sigma, settings, mass_errors):
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(B, V, generator=g) * sigma).to(torch.float16).float()
    prev = torch.randint(0, V, (B, 5), generator=g)
    prev[:, 4] = prev[:, 3]                                            # a repeated id in every row
    prev[:, 0] = logits.argmax(1)                                      # and the leader among them
    got = _raw(logits.to(DEV), settings, prev=prev, step=3, seed=1234)
    us = [sample_uniform(1234, b, 3) for b in range(B)]
    assert got["u"].to(torch.float64).tolist() == us
    failed, indecisive, worst = [], 0, 0.0
    for b in range(B):
        ok, decisive, count, mass = _margin_rule(logits[b], prev[b], us[b], int(got["tokens"][b]), settings, EPS)
        worst = max(worst, abs(float(got["mass"][b]) - mass) / mass)
        indecisive += not decisive
        if not ok or (decisive and count != int(got["kept"][b])):
            failed.append((b, ok, decisive, count, int(got["kept"][b])))
    mass_errors[(V, B, sigma, settings)] = worst
    print(f"V {V} rows {B} sigma {sigma} {settings}: max relative kept-mass error {worst:.3e}, indecisive rows {indecisive}, "
          f"kept min / max {int(got['kept'].min())} / {int(got['kept'].max())}")
    assert EPS <= 1e-5
    assert worst <= MASS_ERR, worst
    assert not failed, failed
    assert indecisive <= (10 if B == 200 else 2), indecisive              # 10 of 200; 37 rows: the same share, rounded up


# ------------------------------------------------------------------------------------------ 4. the distribution
def test_distribution_chi_square():
    from scipy.stats import chi2
    V, B, seeds = 64, 200, 50
    g = torch.Generator().manual_seed(4)
    row = (torch.randn(V, generator=g) * 0.7).float()
    p = torch.softmax(row.double(), 0)
    assert float(p.min()) * B * seeds >= 5
    logits = row.repeat(B, 1).to(DEV).contiguous()
    hist = torch.zeros(V, dtype=torch.float64)
    for s in range(seeds):
        hist += torch.bincount(_raw(logits, (True, 1.0, 0, 1.0, 1.0), seed=1000 + s)["tokens"], minlength=V).double()
    assert hist.sum() == B * seeds
    expect = p * B * seeds
    stat = float(((hist - expect) ** 2 / expect).sum())
    bound = float(chi2.ppf(1 - 1e-6, V - 1))
    print(f"chi-square {stat:.1f} (63 degrees of freedom; the 1 - 1e-6 quantile is {bound:.1f})")
    assert stat < bound


def test_entry_refuses_bad_settings_before_any_launch():
    logits = torch.zeros((2, 64), dtype=torch.float32, device=DEV)
    L = _lib.lib()
    for bad in ((True, 0.0, 0, 0.9, 1.0), (True, 1.0, -1, 0.9, 1.0), (True, 1.0, 0, 0.0, 1.0), (True, 1.0, 0, 1.5, 1.0),
                (True, 1.0, 0, 0.9, 0.0), (True, -1.0, 0, 0.9, 1.0)):
        tokens = torch.full((2,), -7, dtype=torch.int64, device=DEV)
        unf = torch.ones(2, dtype=torch.int32, device=DEV)
        u = torch.zeros(2, dtype=torch.float32, device=DEV)
        rc = L.cgpt_llm_sample_logits(C.c_void_p(logits.data_ptr()), 64, 2, 64, None, 0, 0, 0, 0, None, 0, 0, C.c_void_p(unf.data_ptr()),
                                      _lib.sample_params(*bad), None, None, C.c_void_p(u.data_ptr()), C.c_void_p(tokens.data_ptr()),
                                      None, None, None, None)
        torch.cuda.synchronize()
        assert rc == 1 and b"cgpt_llm_sample_logits" in L.cgpt_last_error(), bad
        assert tokens.tolist() == [-7, -7]


# ------------------------------------------------------------------------------------------ 5.-7. the engine
EOS_ID, PAD_ID = 2, 0


def _buffers(dec, B, length):
    shape = (B, dec.kv_heads, length, 128)
    return ([torch.zeros(shape, dtype=torch.float16, device=DEV) for _ in range(dec.layers)],
            [torch.zeros(shape, dtype=torch.float16, device=DEV) for _ in range(dec.layers)])


def _sample(dec, embs, n, ids, seed, settings=CHAT, eos=(EOS_ID,), min_new=1, starts=None, return_logits=False):
    """Native prefill + sampled decode of embs [B, L, hidden]: tokens [B, n] (and the logits every select saw)."""
    B, L, _ = embs.shape
    kb, vb = _buffers(dec, B, L + n)
    first = dec.prefill(embs.contiguous(), kb, vb, starts=starts)
    return dec.sample(first, L, n, min_new if eos else 0, list(eos), PAD_ID, kb, vb, settings, ids.to(DEV), _seed_dev(seed),
                      return_logits=return_logits, starts=starts)


@pytest.fixture(scope="module")
def small():
    llm = lu.small_decoder()
    dec = _HipDecoder(llm, 200)
    yield llm, dec
    dec.close()


def test_every_token_passes_the_margin_rule_and_replays_are_bit_identical(small):
    llm, dec = small
    B, L, n = 37, 12, 8
    embs = llm.get_input_embeddings()(lu.ids(llm, B, L, 4)).contiguous()
    ids = torch.arange(1000, 1000 + B, dtype=torch.int64)
    T, logits = _sample(dec, embs, n, ids, SEED, return_logits=True)
    T2 = _sample(dec, embs, n, ids, SEED)
    assert torch.equal(T, T2)
    Tc, lg = T.cpu(), logits.cpu()
    assert bool(torch.isinf(lg[:, 0, EOS_ID]).all()) and not bool(torch.isinf(lg[:, 1:]).any())     # min_new = 1
    checked, indecisive = 0, 0
    for b in range(B):
        for i in range(n):
            if i and (EOS_ID in Tc[b, :i].tolist()):
                assert Tc[b, i:].tolist() == [PAD_ID] * (n - i)
                break
            ok, decisive, _, _ = _margin_rule(lg[b, i], Tc[b, :i], sample_uniform(SEED, 1000 + b, i), int(Tc[b, i]), CHAT, EPS)
            assert ok, (b, i)
            checked += 1
            indecisive += not decisive
    print(f"{checked} selects checked, {indecisive} indecisive; distinct tokens {Tc.unique().numel()}")
    assert checked >= B * n // 2 and indecisive <= checked // 20
    assert Tc.unique().numel() > 20 and not torch.equal(T, _sample(dec, embs, n, ids, SEED + 1))
    # one capture, two replays: bit-identical to each other and to the eager call
    kb, vb = _buffers(dec, B, L + n)
    ids_dev, seed_dev = ids.to(DEV), _seed_dev(SEED)
    static = embs.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dec.prefill(static, kb, vb)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        first = dec.prefill(static, kb, vb)
        out = dec.sample(first, L, n, 1, [EOS_ID], PAD_ID, kb, vb, CHAT, ids_dev, seed_dev)
    graph.replay()
    r1 = out.clone()
    graph.replay()
    assert torch.equal(out, r1) and torch.equal(r1, T)
    # rewritten ids and seed: the replay draws the new stream
    ids_dev.copy_(torch.arange(5, 5 + B))
    seed_dev.fill_(77)
    graph.replay()
    r2 = out.clone()
    assert torch.equal(r2, _sample(dec, embs, n, torch.arange(5, 5 + B), 77)) and not torch.equal(r2, r1)


def test_partition_invariance(small):
    llm, dec = small
    B, L, n = 200, 12, 8
    embs = llm.get_input_embeddings()(lu.ids(llm, B, L, 6)).contiguous()
    ids = torch.arange(B, dtype=torch.int64)
    whole = _sample(dec, embs, n, ids, 42)
    parts = torch.cat([_sample(dec, embs[:128], n, ids[:128], 42), _sample(dec, embs[128:], n, ids[128:], 42)])
    assert torch.equal(whole, parts)
    assert not torch.equal(whole[:72], _sample(dec, embs[:72], n, ids[128:], 42))          # the ids, not the rows' places, pick the stream


def test_early_stop_and_stop_sequences_compose(small):
    llm, dec = small
    B, L, n = 37, 12, 10
    embs = llm.get_input_embeddings()(lu.ids(llm, B, L, 7)).contiguous()
    ids = torch.arange(B, dtype=torch.int64)
    T = _sample(dec, embs, n, ids, 9, eos=())
    assert dec.live_steps() == n - 1
    seqs = [[int(T[0, 2])], T[1, 3:5].tolist(), T[2, 1:4].tolist()]
    cols = stop_finish_columns(T, [], seqs)
    assert min(cols) < n - 1 and max(cols) == n, cols
    dec.set_stop_sequences(seqs)
    dec.set_early_stop(True)
    try:
        got = _sample(dec, embs, n, ids, 9, eos=())
        assert torch.equal(got, apply_stop_sequences(T, [], seqs, PAD_ID))
        assert dec.live_steps() == n - 1
        four = _sample(dec, embs[:3], n, ids[:3], 9, eos=())               # the three rows that finish: the steps after the last one are dead
        assert torch.equal(four, apply_stop_sequences(T[:3], [], seqs, PAD_ID))
        assert dec.live_steps() == min(max(cols[:3]), n - 1) < n - 1
    finally:
        dec.set_early_stop(False)
        dec.set_stop_sequences(None)


def test_live_steps_on_a_zeroed_lm_head():
    llm = lu.small_decoder()
    with torch.no_grad():
        llm.lm_head.weight.zero_()
    dec = _HipDecoder(llm, 8, early_stop=True)
    try:
        B, L, n, V = 4, 12, 10, 320
        embs = llm.get_input_embeddings()(lu.ids(llm, B, L, 8)).contiguous()
        ids = torch.arange(B, dtype=torch.int64)
        # every logit is 0: all 320 columns tie, both cuts keep the whole group, and the token is floor(320 u) up to the CDF's rounding
        T = _sample(dec, embs, n, ids, 5, eos=()).cpu()
        for b in range(B):
            for i in range(n):
                assert abs(int(T[b, i]) - int(V * sample_uniform(5, b, i))) <= 1, (b, i)
        assert dec.live_steps() == n - 1
        eos = sorted({int(T[b, b + 1]) for b in range(B)})              # staggered: row b finishes at column <= b + 1
        cols = stop_finish_columns(T, eos, [])
        got = _sample(dec, embs, n, ids, 5, eos=eos, min_new=0).cpu()
        assert torch.equal(got, apply_stop_sequences(T, eos, [], PAD_ID))
        assert dec.live_steps() == min(max(cols), n - 1) <= B
    finally:
        dec.close()


def test_a_padded_row_equals_the_row_alone(small):
    llm, dec = small
    B, L, n = 5, 12, 8
    starts = torch.tensor([0, 11, 5, 1, 7], dtype=torch.int32)
    embs = llm.get_input_embeddings()(lu.ids(llm, B, L, 10)).clone()
    for b, s in enumerate(starts.tolist()):
        embs[b, :s] = 0
    ids = torch.tensor([3, 2 ** 32 + 1, 9, 0, 12345], dtype=torch.int64)
    padded = _sample(dec, embs, n, ids, 11, starts=starts.to(DEV))
    for b, s in enumerate(starts.tolist()):
        alone = _sample(dec, embs[b:b + 1, s:].contiguous(), n, ids[b:b + 1], 11)
        assert torch.equal(alone[0], padded[b]), b


def test_int8_and_grouped_twins():
    llm = lu.small_decoder()
    B, L, n = 8, 12, 6
    ids = torch.arange(50, 50 + B, dtype=torch.int64)
    twin = copy.deepcopy(llm)
    twin.load_state_dict(int8_state_dict(llm, device="cpu"), strict=True)
    a, b = _HipDecoder(llm, 8, weights="int8"), _HipDecoder(twin, 8)
    try:
        embs = llm.get_input_embeddings()(lu.ids(llm, B, L, 12)).contiguous()
        assert torch.equal(_sample(a, embs, n, ids, 3), _sample(b, embs, n, ids, 3))
    finally:
        a.close()
        b.close()
    grouped = lu.llama_decoder(512, 4, 1408, 320, kv_heads=2)
    expanded = lu.llama_decoder(512, 4, 1408, 320, kv_heads=4, sd=expand_kv_state_dict(grouped))
    a, b = _HipDecoder(grouped, 8, grouped_kv=True), _HipDecoder(expanded, 8)
    try:
        embs = grouped.get_input_embeddings()(lu.ids(grouped, B, L, 13)).contiguous()
        assert torch.equal(_sample(a, embs, n, ids, 3), _sample(b, embs, n, ids, 3))
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------ 8. the classifier
def test_classifier_counts_do_not_depend_on_the_partition(small):
    llm, _ = small
    cfg = dataclasses.replace(mo.tiny_config(mode=mo.MODE_ENCODE_IMG), proj_dim=512)
    enc = make_classifier(cfg, max_batch=200)
    try:
        enc.init_synthetic(seed=0)
        x = torch.from_numpy(mo.synthetic_image(cfg, seed=11)).to(DEV)
        tok = WordHashTokenizer(320)
        kw = dict(max_new_tokens=4, max_batch=200, decode="hip", prefill="hip", generate_kwargs=dict(CHAT_KW, min_length=1))
        clf = MiniGPT4Classifier(enc, llm, tok, PROMPT, AnswerLabelMap(6, ()), sample="hip", **kw)
        assert clf._sample_settings() == CHAT
        # the answer vocabulary: the five most frequent answers of the 200 rows themselves
        answers = clf.generate_from_embeds(enc.encode_img_noisy(x, 0, 200, 0.5, 7).to(torch.float16), PROMPT, draws=(0, 7))
        words = [w for w, _ in collections.Counter(answers).most_common(5)]
        clf = MiniGPT4Classifier(enc, llm, tok, PROMPT, AnswerLabelMap(6, words), sample="hip", **kw)
        whole = clf.sample_counts(x, 0, 200, 200, 0.5, 7)
        assert clf.decode_stats["hip_sampled"] == 1 and clf.decode_stats["hf_calls"] == 0
        halves = clf.sample_counts(x, 0, 100, 200, 0.5, 7) + clf.sample_counts(x, 100, 100, 200, 0.5, 7)
        by64 = clf.sample_counts(x, 0, 200, 64, 0.5, 7)
        assert clf.decode_stats["hip_sampled"] == 1 + 2 + 4 and clf.decode_stats["hf_calls"] == 0
        print("counts:", whole.tolist())
        assert int(whole.sum()) == 200 and int((whole > 0).sum()) >= 2
        assert torch.equal(whole, halves) and torch.equal(whole, by64)
        pair = clf.sample_counts_pair(x, 0, 100, 100, 100, 200, 0.5, 7)
        assert torch.equal(pair.sum(0), whole)
        # the running counter: two calls differ, a reset reproduces them
        emb = enc.encode_img_noisy(x, 0, 8, 0.5, 7).to(torch.float16)
        clf.reset_draws(0, seed=3)
        a1, a2 = clf.generate_from_embeds(emb, PROMPT), clf.generate_from_embeds(emb, PROMPT)
        clf.reset_draws(0)
        assert [clf.generate_from_embeds(emb, PROMPT), clf.generate_from_embeds(emb, PROMPT)] == [a1, a2] and a1 != a2
        # sample = "hf": the same call still takes HF generate
        hf = MiniGPT4Classifier(enc, llm, tok, PROMPT, AnswerLabelMap(6, words), **kw)
        torch.manual_seed(0)
        hf.generate_from_embeds(emb, PROMPT)
        assert hf.decode_stats["hf_calls"] == 1 and hf.decode_stats["hip_sampled"] == 0 and hf.decode_stats["graph_replays"] == 0
    finally:
        enc.close()
