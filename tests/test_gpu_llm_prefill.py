"""prefill="hip": the native LLaMA prefill (cgpt_llm_prefill: csrc/llm_prefill.hip + the large-shape GEMM) against the installed HF
LlamaForCausalLM.

Accuracy yardstick, the one of test_gpu_llm_decode.py with the same bounds and the same derivation: the same embeds go into the
library, into HF's fp16 forward and into an fp32 copy of the weights; with e = distance to the fp32 model, the engine passes when
max e_lib <= 1.5 max e_hf and rms e_lib <= 1.5 rms e_hf for the last-position logits and for every layer's K and V over ALL
positions; for layer 0 (whose input is identical in both engines) at least 98 % of the elements are bit-equal to HF's and the
largest difference is <= 1 (values) / <= 2 (keys) ulp taken at the head's largest element.  Trajectories are judged by
`greedy_decode_parity`.

One documented difference of rounding: the attention probabilities are rounded to fp16 as the matrix-core operand of P.V
(DESIGN.md 4.4), as the fused attention kernels HF dispatches to do; layer 0's K / V do not depend on it."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import certifiedgpt_amd as cg
from certifiedgpt_amd import _lib
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import (MiniGPT4Classifier, WordHashTokenizer, _HipDecoder, greedy_decode_parity,
                                       hip_decode_unsupported, prepare_texts)
from oracle import model_oracle as mo, smooth_oracle as so
from gpu_util import DEV, make_classifier
import llm_util as lu
from llm_util import K_SENTINEL, V_SENTINEL, PROMPT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small():
    """hidden 512 = 4 heads x 128, MLP 1408, vocabulary 320, 2 layers."""
    llm = lu.llama_decoder(512, 4, 1408, 320)
    assert hip_decode_unsupported(llm, 200) == []
    dec = _HipDecoder(llm, 200)
    llm32 = copy.deepcopy(llm).float()
    yield llm, dec, llm32
    dec.close()


@pytest.fixture(scope="module")
def vicuna():
    """Vicuna-7B's widths (hidden 4096, 32 heads, MLP 11008, vocabulary 32000) with 2 random-init layers."""
    llm = lu.llama_decoder(4096, 32, 11008, 32000)
    dec = _HipDecoder(llm, 200)
    llm32 = copy.deepcopy(llm).float()
    yield llm, dec, llm32
    dec.close()
    del llm, llm32
    torch.cuda.empty_cache()


def _lib_prefill(llm, dec, embs, extra=3):
    B, L, _ = embs.shape
    kb, vb = lu.sentinel_cache(llm.config.num_hidden_layers, llm.config.num_attention_heads, B, L + extra)
    logits = dec.prefill(embs, kb, vb)
    torch.cuda.synchronize()
    return logits, kb, vb


def _check_against_hf(name, llm, dec, llm32, B, L, seed=3):
    embs = lu.embeds(llm, B, L, seed)
    lib, kb, vb = _lib_prefill(llm, dec, embs)
    hf, hk, hv = lu.model_prefill(llm, embs)
    ref, rk, rv = lu.model_prefill(llm32, embs.float())
    assert bool(torch.isfinite(lib).all()) and bool(torch.isfinite(hf).all()) and bool(torch.isfinite(ref).all())
    figures = {"logits": lu.err(lib, ref) + lu.err(hf, ref)}
    layer0 = {}
    for l in range(len(kb)):
        for nm, mine, theirs, exact, sentinel in (("k", kb[l], hk[l], rk[l], K_SENTINEL), ("v", vb[l], hv[l], rv[l], V_SENTINEL)):
            new = mine[:, :, :L]
            assert bool(torch.isfinite(new).all())
            assert bool((mine[:, :, L:] == sentinel).all())            # no cache row outside 0 .. L-1 is written
            figures[f"{nm}{l}"] = lu.err(new, exact) + lu.err(theirs, exact)
            if l == 0:
                want = theirs.float()
                ulp = want.abs().amax(dim=-1, keepdim=True).clamp_min(2.0 ** -14).log2().floor().sub(10).exp2()
                layer0[nm] = (float((new == theirs).float().mean()), float(((new.float() - want).abs() / ulp).max()))
    print(f"[prefill {name}, {B} rows x {L} positions] (max, rms) error ratio library / HF against the fp32 model: "
          + ", ".join(f"{k} ({v[0] / v[2]:.3f}, {v[1] / v[3]:.3f})" for k, v in figures.items())
          + f"; max |logit lib - hf| {float((lib - hf).abs().max()):.4g} at max |logit| {float(hf.abs().max()):.4g}"
          + f"; layer 0 share bit-equal to HF / largest difference in head-max ulp: k {layer0['k'][0]:.4f} / {layer0['k'][1]:.2f}, "
          f"v {layer0['v'][0]:.4f} / {layer0['v'][1]:.2f}", flush=True)
    for k, v in figures.items():
        assert v[0] <= 1.5 * v[2] and v[1] <= 1.5 * v[3], (k, v)
    assert layer0["v"][1] <= 1.0 and layer0["k"][1] <= 2.0, layer0     # head-max ulp
    assert layer0["v"][0] >= 0.98 and layer0["k"][0] >= 0.98, layer0   # bit-equal share
    return float((lib - hf).abs().max())


# ------------------------------------------------------------------------------------------ 1. logits and cache against HF
# L: 1 and 12 (inside one 16-query tile), 44 and 45 (the bench shape and its odd neighbour: two 32-key blocks, three query tiles),
# 70 (across the attention kernel's 64-key chunk and 64-query block), 300 (above 288: five chunks staged one after the other)
@pytest.mark.parametrize("L", [1, 12, 44, 45, 70, 300])
@pytest.mark.parametrize("B", [200, 37])
def test_prefill_error_is_within_hfs_own_fp16_error_small_decoder(small, B, L):
    llm, dec, llm32 = small
    _check_against_hf("small decoder", llm, dec, llm32, B, L)


@pytest.mark.parametrize("L", [12, 44])
@pytest.mark.parametrize("B", [200, 37])
def test_prefill_error_is_within_hfs_own_fp16_error_vicuna_width(vicuna, B, L):
    llm, dec, llm32 = vicuna
    _check_against_hf("Vicuna width", llm, dec, llm32, B, L)


# ------------------------------------------------------------------------------------------ 2. rows outside 0 .. L-1
def test_cache_rows_outside_the_prompt_are_bit_unchanged(small):
    llm, dec, _ = small
    B, L, extra = 37, 21, 20
    kb, vb = lu.sentinel_cache(llm.config.num_hidden_layers, llm.config.num_attention_heads, B, L + extra)
    for i, t in enumerate(kb + vb):                                    # a pattern of its own per buffer, not one constant
        t[:, :, L:] = torch.arange(extra * 128, device=DEV, dtype=torch.float16).view(extra, 128) * 0.25 + i
    before = [t.clone() for t in kb + vb]
    dec.prefill(lu.embeds(llm, B, L, 4), kb, vb)
    torch.cuda.synchronize()
    for t, was in zip(kb + vb, before):
        assert torch.equal(t[:, :, L:], was[:, :, L:])
        assert not torch.equal(t[:, :, :L], was[:, :, :L])


# ------------------------------------------------------------------------------------------ 3. causality
@pytest.mark.parametrize("L, p", [(44, 17), (70, 64), (150, 33)])
def test_positions_at_or_after_p_do_not_reach_cache_rows_before_p(small, L, p):
    llm, dec, _ = small
    B = 9
    embs = lu.embeds(llm, B, L, 6)
    other = embs.clone()
    other[:, p:] = lu.embeds(llm, B, L, 7)[:, p:]
    _, k1, v1 = _lib_prefill(llm, dec, embs)
    _, k2, v2 = _lib_prefill(llm, dec, other)
    for a, b in zip(k1 + v1, k2 + v2):
        assert torch.equal(a[:, :, :p], b[:, :, :p])
    assert not torch.equal(k1[-1][:, :, p:L], k2[-1][:, :, p:L])         # and the change is seen from p on


# ------------------------------------------------------------------------------------------ 4. determinism, batch independence
@pytest.mark.parametrize("which", ["small", "vicuna"])
def test_prefills_are_bit_identical_and_rows_do_not_depend_on_the_batch(which, request):
    llm, dec, _ = request.getfixturevalue(which)
    B, L = 200, 44
    embs = lu.embeds(llm, B, L, 5)
    first = _lib_prefill(llm, dec, embs)
    again = _lib_prefill(llm, dec, embs)
    assert torch.equal(first[0], again[0])
    assert all(torch.equal(a, b) for a, b in zip(first[1] + first[2], again[1] + again[2]))
    for lo, hi in ((0, 128), (128, 200)):                              # the same rows as 128 + 72
        lg, kb, vb = _lib_prefill(llm, dec, embs[lo:hi].contiguous())
        assert torch.equal(lg, first[0][lo:hi])
        assert all(torch.equal(a, b[lo:hi]) for a, b in zip(kb + vb, first[1] + first[2]))
    # captured into a graph: two replays give the eager call's logits and cache, bit for bit
    kb, vb = lu.sentinel_cache(llm.config.num_hidden_layers, llm.config.num_attention_heads, B, L + 3)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lg = dec.prefill(embs, kb, vb)
    for _ in range(2):
        lg.zero_()
        for t in kb + vb:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(lg, first[0])
        assert all(torch.equal(a[:, :, :L], b[:, :, :L]) for a, b in zip(kb + vb, first[1] + first[2]))
    del graph


# ------------------------------------------------------------------------------------------ 5. refusals
def test_prefill_entries_refuse_before_any_launch(small):
    llm, _, _ = small
    L = cg.lib()
    STATE, INVALID = 5, 1

    def config(**kw):
        base = dict(struct_size=C.sizeof(_lib.LlmConfig), device=0, hidden=512, layers=2, heads=4, kv_heads=4, head_dim=128, mlp=1408,
                    vocab=320, rms_eps=1e-6, rope_theta=10000.0, max_batch=8, max_len=64)
        base.update(kw)
        return _lib.LlmConfig(**base)

    emb = torch.zeros(8, 16, 512, dtype=torch.float16, device=DEV)
    out = torch.full((8, 320), 3.0, device=DEV)
    kv = [torch.full((8, 4, 16, 128), 9.0, dtype=torch.float16, device=DEV) for _ in range(2)]
    ptrs = (C.c_void_p * 2)(kv[0].data_ptr(), kv[1].data_ptr())

    def prefill(h, B, Lp, stride=16, k=ptrs, v=ptrs):
        return L.cgpt_llm_prefill(h, C.c_void_p(emb.data_ptr()), B, Lp, k, v, stride, C.c_void_p(out.data_ptr()), None)

    def refused(status, want):
        assert status == want, (status, want)
        assert L.cgpt_last_error()
        torch.cuda.synchronize()
        assert bool((out == 3.0).all()) and all(bool((t == 9.0).all()) for t in kv)        # nothing was launched

    h = C.c_void_p()
    assert L.cgpt_llm_create(C.byref(config()), C.byref(h)) == 0
    try:
        w = llm.state_dict()["model.norm.weight"]
        assert L.cgpt_llm_load_weight_f16(h, b"model.norm.weight", C.c_void_p(w.data_ptr()), w.numel(), None) == 0
        assert L.cgpt_llm_prefill_reserve(h, 8, 16) == 0
        refused(prefill(h, 2, 4), STATE)                               # a half-loaded handle
        assert b"weights" in L.cgpt_last_error()
        assert L.cgpt_llm_prefill_reserve(h, 9, 16) == INVALID and L.cgpt_llm_prefill_reserve(h, 0, 16) == INVALID
        assert L.cgpt_llm_prefill_reserve(h, 8, 65) == INVALID and L.cgpt_llm_prefill_reserve(h, 8, 0) == INVALID
    finally:
        L.cgpt_llm_destroy(h)
    h = C.c_void_p()
    assert L.cgpt_llm_create(C.byref(config()), C.byref(h)) == 0
    try:
        sd = llm.state_dict()
        for name, w in sd.items():
            if name.endswith("weight") and "rotary" not in name:
                assert L.cgpt_llm_load_weight_f16(h, name.encode(), C.c_void_p(w.data_ptr()), w.numel(), None) == 0, name
        torch.cuda.synchronize()
        refused(prefill(h, 2, 4), STATE)                               # before any reserve
        assert b"reserve" in L.cgpt_last_error()
        assert L.cgpt_llm_prefill_reserve(h, 2, 16) == 0               # 32 token rows -> one 256-row tile
        assert L.cgpt_llm_prefill_reserve(h, 2, 16) == 0               # idempotent
        refused(prefill(h, 8, 40, stride=64), STATE)                   # 320 token rows > the reserved 256
        refused(prefill(h, 2, 17, stride=16), INVALID)                 # L > kv_len_stride
        refused(prefill(h, 2, 65, stride=128), INVALID)                # L > max_len
        refused(prefill(h, 2, 0), INVALID)
        refused(prefill(h, 0, 4), INVALID)
        refused(prefill(h, 9, 4), INVALID)                             # B > max_batch
        refused(prefill(h, 2, 4, k=None), INVALID)
        refused(prefill(h, 2, 4, v=(C.c_void_p * 2)(kv[0].data_ptr(), None)), INVALID)
        assert L.cgpt_llm_prefill(h, None, 2, 4, ptrs, ptrs, 16, C.c_void_p(out.data_ptr()), None) == INVALID
        assert prefill(h, 2, 16) == 0                                  # and a call inside every bound runs
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out[:2]).all()) and not bool((out[:2] == 3.0).all())
        assert bool((out[2:] == 3.0).all())
    finally:
        L.cgpt_llm_destroy(h)


# ------------------------------------------------------------------------------------------ 6. + 7. configs[2] at Vicuna width
@pytest.fixture(scope="module")
def configs2(vicuna):
    """200 noisy rows of a full-size encode_img, HF `generate` with scores run eagerly, and eps = 2 x the largest |library - HF|
    first-token logit difference measured on these very rows."""
    llm, dec, _ = vicuna
    cfg = mo.Config(mode=mo.MODE_ENCODE_IMG, num_classes=10)
    enc = make_classifier(cfg, max_batch=20)
    enc.init_synthetic(seed=0)
    tok = WordHashTokenizer(32000)
    x = torch.from_numpy(mo.synthetic_image(cfg, seed=11)).to(DEV)
    B, n, sigma, seed = 200, 20, 0.5, 42
    emb = torch.cat([enc.encode_img_noisy(x, lo, min(enc.max_batch, B - lo), sigma, seed) for lo in range(0, B, enc.max_batch)]).to(torch.float16)
    hf = MiniGPT4Classifier(enc, llm, tok, PROMPT, AnswerLabelMap(4, ()), max_new_tokens=n, max_batch=B, decode="hf")
    segs = hf._segment_embeddings(PROMPT, emb.device)
    embs = torch.cat([segs[0].expand(B, -1, -1), emb, segs[1].expand(B, -1, -1)], dim=1).contiguous()
    with torch.no_grad():
        out = llm.generate(inputs_embeds=embs, attention_mask=torch.ones(embs.shape[:2], dtype=torch.int, device=DEV), max_new_tokens=n,
                           output_scores=True, return_dict_in_generate=True, **hf.hf_generate_kwargs())
    hf_tokens, hf_scores = out.sequences, torch.stack(out.scores, dim=1).float()
    lib_first, _, _ = _lib_prefill(llm, dec, embs)
    hf_first, _, _ = lu.model_prefill(llm, embs)
    d_first = float((lib_first - hf_first).abs().max())
    eps = 2.0 * d_first
    yield {"enc": enc, "cfg": cfg, "tok": tok, "x": x, "emb": emb, "embs": embs, "hf_tokens": hf_tokens, "hf_scores": hf_scores,
           "eps": eps, "d_first": d_first, "B": B, "n": n, "sigma": sigma, "seed": seed}
    enc.close()


def test_configs2_native_prefill_and_steps_follow_hf_generate_at_vicuna_width(vicuna, configs2):
    llm, _, _ = vicuna
    c = configs2
    B, n = c["B"], c["n"]
    hip = MiniGPT4Classifier(c["enc"], llm, c["tok"], PROMPT, AnswerLabelMap(4, ()), max_new_tokens=n, max_batch=B, decode="hip",
                             prefill="hip", prefill_linear="cgpt")
    assert hip.routed_linears == 0 and hip._hip is not None and hip.prefill == "hip"     # prefill_linear is ignored, nothing is routed
    model = MiniGPT4Classifier(c["enc"], llm, c["tok"], PROMPT, AnswerLabelMap(4, ()), max_new_tokens=n, max_batch=B, decode="hip",
                               prefill="model")
    calls = {"n": 0}
    hook = llm.register_forward_pre_hook(lambda *_: calls.__setitem__("n", calls["n"] + 1))
    try:
        with torch.no_grad():
            t_eager = hip.greedy_tokens(c["embs"])
            t_graph = hip._generate_graph(c["embs"])
            again = hip._generate_graph(c["embs"])
        assert calls["n"] == 0                                         # no HF forward ran, eagerly, in the warm-up or under capture
    finally:
        hook.remove()
    assert torch.equal(t_graph, again)
    with torch.no_grad():
        t_model = model._generate_graph(c["embs"])
    report = {"eager": greedy_decode_parity(c["hf_tokens"], c["hf_scores"], t_eager, c["eps"]),
              "graph": greedy_decode_parity(c["hf_tokens"], c["hf_scores"], t_graph, c["eps"])}
    top2 = c["hf_scores"].topk(2, dim=-1).values
    decisive = (torch.nan_to_num(top2[..., 0] - top2[..., 1], nan=float("inf")) > c["eps"]).all(dim=1)
    same_as_model = {"eager": (t_eager == t_model).all(dim=1), "graph": (t_graph == t_model).all(dim=1)}
    print(f"[configs2 native prefill] largest first-token |lib - hf| {c['d_first']:.4g}, eps {c['eps']:.4g}; "
          + "; ".join(f"{k}: {v['identical']}/{B} rows identical to HF, {v['decisive_identical']}/{v['decisive']} decisive rows identical, "
                      f"largest HF margin at a first divergence {v['max_margin_at_divergence']:.4g}, "
                      f"{int(same_as_model[k].sum())}/{B} rows identical to prefill=\"model\"" for k, v in report.items()), flush=True)
    for name, v in report.items():
        assert not v["violations"], (name, v)
        assert v["decisive_identical"] == v["decisive"] and v["diverged"] <= B - v["decisive"], (name, v)
        assert v["decisive"] >= B // 10, (name, v)                     # the rule must bite on a meaningful number of rows
        assert bool(same_as_model[name][decisive].all()), name
    s = hip.decode_stats
    assert s["hf_calls"] == 0 and s["graph_replays"] == 2
    assert s["hip_prefills"] == s["graph_replays"] + 1                  # the replays and the one eager call
    assert s["hip_steps"] == (s["graph_replays"] + 1) * (n - 1)
    assert model.decode_stats["hip_prefills"] == 0
    # ragged prompts keep taking the HF call, and are counted
    hip.generate_from_embeds(c["emb"][:2], [PROMPT, PROMPT + " now"])
    assert hip.decode_stats["hf_calls"] == 1 and hip.decode_stats["hip_prefills"] == 3


@pytest.mark.parametrize("mnt", [1, 20])
def test_configs2_certify_on_native_prefill_matches_model_prefill_on_decisive_rows(vicuna, configs2, mnt):
    llm, _, _ = vicuna
    c = configs2
    n0 = n = 100
    alpha, bs = 0.001, 100
    top2 = c["hf_scores"][:, :mnt].topk(2, dim=-1).values
    decisive = (torch.nan_to_num(top2[..., 0] - top2[..., 1], nan=float("inf")) > c["eps"]).all(dim=1).cpu().numpy()
    answers = {}
    for engine in ("model", "hip"):
        clf = MiniGPT4Classifier(c["enc"], llm, c["tok"], PROMPT, AnswerLabelMap(4, ()), max_new_tokens=mnt, max_batch=bs, decode="hip",
                                 prefill=engine)
        answers[engine] = sum((clf.generate_from_embeds(c["emb"][lo:lo + bs], PROMPT) for lo in range(0, n0 + n, bs)), [])
        assert clf.decode_stats["hf_calls"] == 0 and clf.decode_stats["hip_prefills"] == (2 if engine == "hip" else 0)
        del clf
    freq = sorted(set(answers["model"]), key=lambda a: (-answers["model"].count(a), a))
    vocab = freq[:9]
    K2 = len(vocab) + 1
    lab = {e: np.array([vocab.index(a) if a in vocab else K2 - 1 for a in answers[e]]) for e in answers}
    same = lab["hip"] == lab["model"]
    print(f"[configs2 certify on the native prefill, {mnt} new tokens] decisive rows {int(decisive.sum())}/200, labels equal on "
          f"{int(same.sum())}/200", flush=True)
    assert bool(same[decisive].all())
    assert all(a == b for a, b, d in zip(answers["hip"], answers["model"], decisive) if d)
    hip = MiniGPT4Classifier(c["enc"], llm, c["tok"], PROMPT, AnswerLabelMap(K2, vocab, frozen=True), max_new_tokens=mnt, max_batch=bs,
                             decode="hip", prefill="hip")
    s = cg.Smooth(hip, K2, c["sigma"], seed=c["seed"], non_certifiable=(hip.label_map.other_id,))
    got = s.certify(c["x"], n0, n, alpha, bs)
    assert list(hip.last_answers) == answers["hip"]                    # the certify ran the same rows through the same engine
    sel, est = np.bincount(lab["hip"][:n0], minlength=K2), np.bincount(lab["hip"][n0:], minlength=K2)
    want = so.certify_from_counts(sel, est, n, alpha, c["sigma"])
    if want[0] == hip.label_map.other_id:
        want = (cg.Smooth.ABSTAIN, 0.0)
    print(f"[configs2 certify on the native prefill, {mnt} new tokens] hip {got} oracle-statistics on its counts {want}", flush=True)
    assert got[0] == want[0] and abs(got[1] - want[1]) <= 1e-9
    assert hip.decode_stats["hf_calls"] == 0 and hip.decode_stats["hip_prefills"] == 2 and hip.decode_stats["hip_steps"] == 2 * (mnt - 1)


# ------------------------------------------------------------------------------------------ 8. graphs survive a growing workspace
def test_a_graph_captured_before_the_workspace_grew_replays_bit_for_bit(small):
    """A captured graph holds the workspace addresses of its capture.  A later, larger reservation must not free them: capture
    100 rows, then grow (a longer prompt, 200 rows, its own graph), then replay the first graph."""
    llm, _, _ = small
    dec = _HipDecoder(llm, 200)                                        # a handle of its own: nothing is reserved yet
    try:
        def captured(B, L, seed):
            embs = lu.embeds(llm, B, L, seed)
            eager = _lib_prefill(llm, dec, embs)                       # reserves (and may grow) outside the capture
            kb, vb = lu.sentinel_cache(llm.config.num_hidden_layers, llm.config.num_attention_heads, B, L + 3)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                lg = dec.prefill(embs, kb, vb)
            return graph, lg, kb, vb, eager, embs                   # embs: the graph reads this very tensor at every replay

        def replay(entry):
            graph, lg, kb, vb = entry[:4]
            lg.zero_()
            for t in kb + vb:
                t.zero_()
            graph.replay()
            torch.cuda.synchronize()
            return [lg.clone()] + [t.clone() for t in kb + vb]

        def same_as_eager(got, entry, L):
            eager = entry[4]
            return torch.equal(got[0], eager[0]) and all(torch.equal(a[:, :, :L], b[:, :, :L]) for a, b in zip(got[1:], eager[1] + eager[2]))

        first = captured(100, 20, 11)
        before = replay(first)
        assert same_as_eager(before, first, 20)
        second = captured(200, 60, 12)                                 # 12 000 token rows > the 4 096 reserved for 200 x 20: grows
        assert same_as_eager(replay(second), second, 60)
        after = replay(first)
        assert all(torch.equal(a, b) for a, b in zip(before, after))
        third = captured(37, 150, 13)                                  # 200 x 150 rows: grows again, two superseded workspaces now
        assert same_as_eager(replay(third), third, 150)
        assert all(torch.equal(a, b) for a, b in zip(before, replay(first)))
        assert same_as_eager(replay(second), second, 60)
        del first, second, third
    finally:
        torch.cuda.synchronize()
        dec.close()


def test_classifier_graphs_of_several_shapes_stay_valid_as_prompts_grow(small):
    """`_generate_graph` keeps graphs of different (rows, prompt length) alive; each must give the same tokens after the others
    were captured, larger ones included, as it gave before -- and as the eager loop gives."""
    llm, _, _ = small
    tok = WordHashTokenizer(320)
    short = prepare_texts(["<Img><ImageHere></Img> what"])[0]
    long_ = prepare_texts(["<Img><ImageHere></Img> " + " ".join(f"word{i}" for i in range(40))])[0]
    clf = MiniGPT4Classifier(None, llm, tok, short, AnswerLabelMap(4, ()), max_new_tokens=6, max_batch=200, decode="hip", prefill="hip")
    g = torch.Generator(device="cpu").manual_seed(21)
    emb = (torch.randn(200, 32, 512, generator=g) * 0.02).to(DEV).to(torch.float16)

    def embeds(rows, prompt):
        segs = clf._segment_embeddings(prompt, emb.device)
        return torch.cat([segs[0].expand(rows, -1, -1), emb[:rows], segs[1].expand(rows, -1, -1)], dim=1).contiguous()

    shapes = [(100, short), (200, short), (100, long_), (200, long_)]  # rows grow, then the prompt grows: four live graphs
    with torch.no_grad():
        first = [clf._generate_graph(embeds(r, p)) for r, p in shapes]
        assert clf.decode_stats["graph_captures"] == 4 and clf.decode_stats["graph_evictions"] == 0
        for _ in range(2):
            for (r, p), want in zip(shapes, first):
                assert torch.equal(clf._generate_graph(embeds(r, p)), want), (r, len(p))
        assert clf.decode_stats["graph_captures"] == 4
        for (r, p), want in zip(shapes, first):
            assert torch.equal(clf.greedy_tokens(embeds(r, p)), want)
    assert clf.decode_stats["hf_calls"] == 0


def test_certify_with_selection_smaller_than_the_batch_smaller_than_estimation_twice(small, tmp_path):
    """n0 < batch < n: graphs of several batch sizes are captured within one certify (full batches and a ragged last one); the
    next image replays every graph after the others' captures.  (This classifier draws selection and estimation as one index range,
    so the shapes are the full batch and the ragged last one.)  Two images twice over, and a fresh classifier: same records."""
    import dataclasses
    from certifiedgpt_amd.agents import registry, setup_agent
    from certifiedgpt_amd.agents import minigpt4_certify_agent  # noqa: F401
    llm, _, _ = small
    cfg = dataclasses.replace(mo.tiny_config(mode=mo.MODE_ENCODE_IMG), proj_dim=512)
    dims = {k: getattr(cfg, k) for k in ("img_size", "patch_size", "vit_dim", "vit_depth", "vit_heads", "vit_mlp", "qf_layers",
                                         "qf_dim", "qf_heads", "qf_ffn", "qf_queries", "qf_xattn_freq", "proj_dim")}
    torch.save({"model": dict(mo.init_params(cfg, 20251121))}, tmp_path / "ckpt.pth")

    def run(prefill):
        conf = {"run": {"agent": "image_text_certify", "output_dir": str(tmp_path), "seed": 0,
                        "smoothing": {"sigma": 2.0, "n0": 6, "n": 40, "alpha": 0.05, "batch_size": 16, "num_classes": 4, "radii": [0.0, 0.1]}},
                "model": {"dims": dims, "weights": str(tmp_path / "ckpt.pth"),
                          "generate": {"prompt": PROMPT, "answers": ["w5", "w7", "w9"], "max_new_tokens": 5, "decode": "hip",
                                       "prefill": prefill}},
                "data": {"num_images": 2, "seed": 3}}
        registry.register("configuration", conf)
        agent = setup_agent(conf)
        agent.tokenizer, agent.llama_model = WordHashTokenizer(320), llm
        agent.run()
        agent.finalize()
        return agent

    a = run("hip")
    assert isinstance(a.model, MiniGPT4Classifier) and a.model.prefill == "hip"
    s = a.model.decode_stats
    assert s["hf_calls"] == 0 and s["hip_prefills"] == s["graph_replays"] > 0 and s["graph_captures"] >= 2      # several shapes
    def outcome(agent):
        return [{k: v for k, v in r.items() if k != "time"} for r in agent.records]

    records, answers, captures = outcome(a), list(a.model.last_answers), s["graph_captures"]
    assert len(records) == 2
    a.classifier = a.model                                             # the same classifier, its graphs kept
    a.run()                                                            # every graph is replayed again, each after the others' captures
    assert outcome(a) == records and list(a.model.last_answers) == answers
    assert a.model.decode_stats["graph_captures"] == captures and a.model.decode_stats["hf_calls"] == 0
    b = run("hip")                                                     # a fresh classifier sees the same shapes from scratch
    assert outcome(b) == records and list(b.model.last_answers) == answers
