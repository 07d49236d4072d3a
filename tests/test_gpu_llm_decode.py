"""decode="hip": the native LLaMA token step (csrc/llm.hip, csrc/llm_step.hip, csrc/llm_gemm.hip) against the installed HF LlamaForCausalLM.

Accuracy yardstick (teacher-forced): at every step the library, HF's fp16 forward and an fp32 copy of the same weights get HF's
own token and HF's own cache; with e_hf = |HF fp16 - fp32| and e_lib = |library - fp32| over the logits of the step, the engine
passes when max e_lib <= 1.5 max e_hf and rms e_lib <= 1.5 rms e_hf: the reference engine's own rounding error is the bound, and
1.5 is room for two independent rounding noises whose maxima over B x V values differ by chance.  Trajectories are judged by the
project's rule (`greedy_decode_parity`): a row may leave HF's trajectory only where HF's own top-2 margin is within the logit noise."""
import dataclasses

import numpy as np
import pytest
import torch

import certifiedgpt_amd as cg
from certifiedgpt_amd.agents import registry, setup_agent
from certifiedgpt_amd.agents import minigpt4_certify_agent  # noqa: F401
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import (MiniGPT4Classifier, WordHashTokenizer, _HipDecoder, fp16_ulp, greedy_decode_parity,
                                       hip_decode_unsupported)
from oracle import model_oracle as mo, smooth_oracle as so
from gpu_util import DEV, make_classifier
import llm_util as lu
from llm_util import PAD, EOS, PROMPT

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def small():
    llm = lu.small_decoder()
    assert hip_decode_unsupported(llm, 200) == []
    dec = _HipDecoder(llm, 200)
    yield llm, dec
    dec.close()


@pytest.fixture(scope="module")
def vicuna():
    llm = lu.vicuna_width_decoder()
    dec = _HipDecoder(llm, 200)
    yield llm, dec
    dec.close()
    del llm
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def vicuna_teacher_forced(vicuna):
    llm, dec = vicuna
    return {B: lu.teacher_forced(llm, dec, B, L=44, steps=4) for B in (200, 37)}


# ------------------------------------------------------------------------------------------ 4. teacher-forced step parity
@pytest.mark.parametrize("B", [200, 37])
def test_teacher_forced_step_error_is_within_hfs_own_fp16_error_small_decoder(small, B):
    llm, dec = small
    lu.check_ratios(f"small decoder, {B} rows", lu.teacher_forced(llm, dec, B))


@pytest.mark.parametrize("B", [200, 37])
def test_teacher_forced_step_error_is_within_hfs_own_fp16_error_vicuna_width(vicuna_teacher_forced, B):
    lu.check_ratios(f"Vicuna width, {B} rows", vicuna_teacher_forced[B])


def test_step_entries_refuse_a_half_loaded_handle_and_a_position_outside_the_cache(small):
    import ctypes as C
    from certifiedgpt_amd import _lib
    llm, dec = small
    L = cg.lib()
    c = _lib.LlmConfig(struct_size=C.sizeof(_lib.LlmConfig), device=0, hidden=512, layers=2, heads=4, kv_heads=4, head_dim=128, mlp=1408,
                       vocab=320, rms_eps=1e-6, rope_theta=10000.0, max_batch=8, max_len=64)
    h = C.c_void_p()
    assert L.cgpt_llm_create(C.byref(c), C.byref(h)) == 0
    try:
        w = llm.state_dict()["model.norm.weight"]
        assert L.cgpt_llm_load_weight_f16(h, b"model.norm.weight", C.c_void_p(w.data_ptr()), w.numel(), None) == 0
        assert L.cgpt_llm_load_weight_f16(h, b"model.norm.weight", C.c_void_p(w.data_ptr()), w.numel() - 1, None) == 1
        assert L.cgpt_llm_load_weight_f16(h, b"model.layers.9.mlp.up_proj.weight", C.c_void_p(w.data_ptr()), w.numel(), None) == 4
        tok = torch.zeros(2, dtype=torch.int64, device=DEV)
        out = torch.empty(2, 320, device=DEV)
        kv = torch.zeros(2, 4, 16, 128, dtype=torch.float16, device=DEV)
        ptrs = (C.c_void_p * 2)(kv.data_ptr(), kv.data_ptr())
        assert L.cgpt_llm_step(h, C.c_void_p(tok.data_ptr()), 2, 3, ptrs, ptrs, 16, C.c_void_p(out.data_ptr()), None) == 5   # CGPT_ERR_STATE
    finally:
        L.cgpt_llm_destroy(h)
    tok = torch.zeros(2, dtype=torch.int64, device=DEV)
    kv = [torch.zeros(2, 4, 16, 128, dtype=torch.float16, device=DEV) for _ in range(2)]
    with pytest.raises(AssertionError):
        dec.step(tok, 16, kv, kv)                                      # row 16 of a 16-row cache
    out = torch.empty(2, 320, device=DEV)
    ptrs = (C.c_void_p * 2)(kv[0].data_ptr(), kv[1].data_ptr())
    assert L.cgpt_llm_step(dec.handle, C.c_void_p(tok.data_ptr()), 2, 16, ptrs, ptrs, 16, C.c_void_p(out.data_ptr()), None) == 1
    assert L.cgpt_llm_step(dec.handle, C.c_void_p(tok.data_ptr()), 201, 3, ptrs, ptrs, 16, C.c_void_p(out.data_ptr()), None) == 1


# ------------------------------------------------------------------------------------------ 6. determinism and invariance
def _greedy_rule(step_logits, eos_ids, pad):
    """`greedy_tokens`' bookkeeping on given per-step logits."""
    B, n, _ = step_logits.shape
    unfinished = torch.ones(B, dtype=torch.long, device=step_logits.device)
    cols = []
    for i in range(n):
        nxt = step_logits[:, i].argmax(-1)
        nxt = nxt * unfinished + pad * (1 - unfinished)
        cols.append(nxt)
        for e in eos_ids:
            unfinished = unfinished * (nxt != e).long()
    return torch.stack(cols, dim=1)


@pytest.mark.parametrize("which", ["small", "vicuna"])
def test_replays_are_bit_identical_and_rows_do_not_depend_on_the_batch(which, request):
    llm, dec = request.getfixturevalue(which)
    B, L, n = 200, 16, 6
    g = torch.Generator(device="cpu").manual_seed(5)
    embs = llm.get_input_embeddings()(torch.randint(3, llm.config.vocab_size, (B, L), generator=g).to(DEV))
    first, kb, vb, _ = lu.prefill(llm, embs, n)
    runs = []
    for _ in range(2):
        k2, v2 = [t.clone() for t in kb], [t.clone() for t in vb]
        runs.append(dec.greedy(first, L, n, 1, [EOS], PAD, k2, v2, return_logits=True) + (k2, v2))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])          # tokens and step logits
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2] + runs[0][3], runs[1][2] + runs[1][3]))   # and the caches they left
    assert bool(torch.isfinite(runs[0][1][:, 1:]).all())
    assert torch.equal(runs[0][0], _greedy_rule(runs[0][1], [EOS], PAD))
    # the same rows as 128 + 72: logits row by row
    for lo, hi in ((0, 128), (128, 200)):
        k2, v2 = [t[lo:hi].clone() for t in kb], [t[lo:hi].clone() for t in vb]
        t_part, l_part = dec.greedy(first[lo:hi].contiguous(), L, n, 1, [EOS], PAD, k2, v2, return_logits=True)
        assert torch.equal(l_part, runs[0][1][lo:hi]) and torch.equal(t_part, runs[0][0][lo:hi])
    # without step logits: same tokens
    k2, v2 = [t.clone() for t in kb], [t.clone() for t in vb]
    assert torch.equal(dec.greedy(first, L, n, 1, [EOS], PAD, k2, v2), runs[0][0])
    # captured into a graph: two replays give the eager run's tokens AND step logits, bit for bit
    k2, v2 = [t.clone() for t in kb], [t.clone() for t in vb]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        t_g, l_g = dec.greedy(first, L, n, 1, [EOS], PAD, k2, v2, return_logits=True)
    replays = []
    for _ in range(2):
        t_g.zero_()
        l_g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        replays.append((t_g.clone(), l_g.clone()))
    for t_r, l_r in replays:
        assert torch.equal(t_r, runs[0][0]) and torch.equal(l_r, runs[0][1])
    del graph


@pytest.mark.parametrize("min_new", [0, 1, 3])
def test_min_new_tokens_and_pad_after_eos_follow_greedy_tokens_rule(small, min_new):
    llm, dec = small
    B, L, n = 37, 10, 6
    g = torch.Generator(device="cpu").manual_seed(9)
    embs = llm.get_input_embeddings()(torch.randint(3, 320, (B, L), generator=g).to(DEV))
    first, kb, vb, _ = lu.prefill(llm, embs, n)
    forced = torch.arange(B, device=DEV) % 3 == 0
    first = first.clone()
    first[forced, EOS] = 1.0e4                                         # EOS wins the first arg-max in these rows unless suppressed
    given = first.clone()
    tokens, steps = dec.greedy(first, L, n, min_new, [EOS], PAD, kb, vb, return_logits=True)
    assert torch.equal(first, given)                                   # the caller's logits are not modified
    assert torch.equal(tokens, _greedy_rule(steps, [EOS], PAD))
    assert bool(torch.isinf(steps[:, :min_new, EOS]).all()) and bool(torch.isfinite(steps[:, min_new:, EOS]).all())
    if min_new == 0:
        assert bool((tokens[forced, 0] == EOS).all()) and bool((tokens[forced, 1:] == PAD).all())
        assert torch.equal(steps[:, 0], given)
    else:
        assert bool((tokens[:, :min_new] != EOS).all())
    # the torch loop of the "graph" engine applies the same rule: identical columns wherever its arg-max agrees
    after = (tokens == EOS).long().cumsum(1) - (tokens == EOS).long()
    assert bool((tokens[after > 0] == PAD).all())


# ------------------------------------------------------------------------------------------ 5. + 7. configs[2] at Vicuna width
@pytest.fixture(scope="module")
def configs2(vicuna, vicuna_teacher_forced):
    """200 noisy rows of a full-size encode_img, HF `generate` with scores, and eps from the teacher-forced measurement."""
    llm, _ = vicuna
    cfg = mo.Config(mode=mo.MODE_ENCODE_IMG, num_classes=10)
    enc = make_classifier(cfg, max_batch=20)
    enc.init_synthetic(seed=0)
    tok = WordHashTokenizer(32000)
    x = torch.from_numpy(mo.synthetic_image(cfg, seed=11)).to(DEV)
    B, n, sigma, seed = 200, 20, 0.5, 42
    emb = torch.cat([enc.encode_img_noisy(x, lo, min(enc.max_batch, B - lo), sigma, seed) for lo in range(0, B, enc.max_batch)]).to(torch.float16)
    hf = MiniGPT4Classifier(enc, llm, tok, PROMPT, AnswerLabelMap(4, ()), max_new_tokens=n, max_batch=B, decode="hf")
    segs = hf._segment_embeddings(PROMPT, emb.device)
    embs = torch.cat([segs[0].expand(B, -1, -1), emb, segs[1].expand(B, -1, -1)], dim=1)
    with torch.no_grad():
        out = llm.generate(inputs_embeds=embs, attention_mask=torch.ones(embs.shape[:2], dtype=torch.int, device=DEV), max_new_tokens=n,
                           output_scores=True, return_dict_in_generate=True, **hf.hf_generate_kwargs())
    hf_tokens, hf_scores = out.sequences, torch.stack(out.scores, dim=1).float()
    ulp = fp16_ulp(float(hf_scores[torch.isfinite(hf_scores)].abs().max()))
    d_tf = max(r["max_lib_vs_hf"] for rows in vicuna_teacher_forced.values() for r in rows)
    eps = max(2.0 * d_tf, 2.0 * ulp)
    yield {"enc": enc, "cfg": cfg, "tok": tok, "x": x, "emb": emb, "embs": embs, "hf_tokens": hf_tokens, "hf_scores": hf_scores,
           "eps": eps, "ulp": ulp, "d_tf": d_tf, "B": B, "n": n, "sigma": sigma, "seed": seed}
    enc.close()


def test_configs2_hip_decode_follows_hf_generate_at_vicuna_width(vicuna, configs2):
    llm, _ = vicuna
    c = configs2
    B, n = c["B"], c["n"]
    hip = MiniGPT4Classifier(c["enc"], llm, c["tok"], PROMPT, AnswerLabelMap(4, ()), max_new_tokens=n, max_batch=B, decode="hip",
                             prefill_linear="cgpt")
    assert hip.routed_linears > 0 and hip._hip is not None
    from certifiedgpt_amd.minigpt4 import _LinearRoute
    with torch.no_grad(), _LinearRoute.enabled():
        t_eager = hip.greedy_tokens(c["embs"])
    report = {"hip eager": greedy_decode_parity(c["hf_tokens"], c["hf_scores"], t_eager, c["eps"])}
    with torch.no_grad():
        report["hip graph"] = greedy_decode_parity(c["hf_tokens"], c["hf_scores"], hip._generate_graph(c["embs"]), c["eps"])
        again = hip._generate_graph(c["embs"])
    assert torch.equal(again, hip._generate_graph(c["embs"]))
    print(f"[configs2 hip] fp16 ulp at the largest logit {c['ulp']:.4g}, teacher-forced max |lib - hf| {c['d_tf']:.4g}, eps {c['eps']:.4g}; "
          + "; ".join(f"{k}: {v['identical']}/{B} rows identical, {v['decisive_identical']}/{v['decisive']} decisive rows identical, largest "
                      f"HF margin at a first divergence {v['max_margin_at_divergence']:.4g}" for k, v in report.items()), flush=True)
    for name, v in report.items():
        assert not v["violations"], (name, v)
        assert v["decisive_identical"] == v["decisive"] and v["diverged"] <= B - v["decisive"], (name, v)
        assert v["decisive"] >= B // 10, (name, v)                     # the rule must bite on a meaningful number of rows
    assert hip.decode_stats["graph_replays"] >= 2 and hip.decode_stats["hf_calls"] == 0
    assert hip.decode_stats["hip_steps"] == (hip.decode_stats["graph_replays"] + 1) * (n - 1)      # the replays and the one eager call
    # ragged prompts keep taking the HF call, and are counted
    hip.generate_from_embeds(c["emb"][:2], [PROMPT, PROMPT + " now"])
    assert hip.decode_stats["hf_calls"] == 1


@pytest.mark.parametrize("mnt", [1, 20])
def test_configs2_certify_on_hip_decode_matches_graph_decode_on_decisive_rows(vicuna, configs2, mnt):
    llm, _ = vicuna
    c = configs2
    n0 = n = 100
    alpha, bs = 0.001, 100
    top2 = c["hf_scores"][:, :mnt].topk(2, dim=-1).values
    decisive = (torch.nan_to_num(top2[..., 0] - top2[..., 1], nan=float("inf")) > c["eps"]).all(dim=1).cpu().numpy()
    answers = {}
    for engine in ("graph", "hip"):
        clf = MiniGPT4Classifier(c["enc"], llm, c["tok"], PROMPT, AnswerLabelMap(4, ()), max_new_tokens=mnt, max_batch=bs, decode=engine,
                                 prefill_linear="cgpt")
        answers[engine] = sum((clf.generate_from_embeds(c["emb"][lo:lo + bs], PROMPT) for lo in range(0, n0 + n, bs)), [])
        assert clf.decode_stats["hf_calls"] == 0
    freq = sorted(set(answers["graph"]), key=lambda a: (-answers["graph"].count(a), a))
    vocab = freq[:9]
    K2 = len(vocab) + 1
    lab = {e: np.array([vocab.index(a) if a in vocab else K2 - 1 for a in answers[e]]) for e in answers}
    same = lab["hip"] == lab["graph"]
    print(f"[configs2 certify, {mnt} new tokens] decisive rows {int(decisive.sum())}/200, labels equal on {int(same.sum())}/200", flush=True)
    assert bool(same[decisive].all())
    assert all(a == b for a, b, d in zip(answers["hip"], answers["graph"], decisive) if d)
    hip = MiniGPT4Classifier(c["enc"], llm, c["tok"], PROMPT, AnswerLabelMap(K2, vocab, frozen=True), max_new_tokens=mnt, max_batch=bs,
                             decode="hip", prefill_linear="cgpt")
    s = cg.Smooth(hip, K2, c["sigma"], seed=c["seed"], non_certifiable=(hip.label_map.other_id,))
    got = s.certify(c["x"], n0, n, alpha, bs)
    assert list(hip.last_answers) == answers["hip"]                    # the certify ran the same rows through the same engine
    sel, est = np.bincount(lab["hip"][:n0], minlength=K2), np.bincount(lab["hip"][n0:], minlength=K2)
    want = so.certify_from_counts(sel, est, n, alpha, c["sigma"])
    if want[0] == hip.label_map.other_id:
        want = (cg.Smooth.ABSTAIN, 0.0)
    print(f"[configs2 certify, {mnt} new tokens] hip {got} oracle-statistics on its counts {want}", flush=True)
    assert got[0] == want[0] and abs(got[1] - want[1]) <= 1e-9
    assert hip.decode_stats["hf_calls"] == 0 and hip.decode_stats["hip_steps"] == 2 * (mnt - 1)


def test_certify_agent_runs_with_decode_hip(small, tmp_path):
    llm, _ = small
    cfg = dataclasses.replace(mo.tiny_config(mode=mo.MODE_ENCODE_IMG), proj_dim=512)
    dims = {k: getattr(cfg, k) for k in ("img_size", "patch_size", "vit_dim", "vit_depth", "vit_heads", "vit_mlp", "qf_layers",
                                         "qf_dim", "qf_heads", "qf_ffn", "qf_queries", "qf_xattn_freq", "proj_dim")}
    torch.save({"model": dict(mo.init_params(cfg, 20251121))}, tmp_path / "ckpt.pth")
    conf = {"run": {"agent": "image_text_certify", "output_dir": str(tmp_path), "seed": 0,
                    "smoothing": {"sigma": 2.0, "n0": 8, "n": 16, "alpha": 0.05, "batch_size": 8, "num_classes": 4, "radii": [0.0, 0.1]}},
            "model": {"dims": dims, "weights": str(tmp_path / "ckpt.pth"),
                      "generate": {"prompt": PROMPT, "answers": ["w5", "w7", "w9"], "max_new_tokens": 5, "decode": "hip"}},
            "data": {"num_images": 2, "seed": 3}}
    registry.register("configuration", conf)
    agent = setup_agent(conf)
    agent.tokenizer, agent.llama_model = WordHashTokenizer(320), llm
    agent.run()
    res = agent.finalize()
    assert res["images"] == 2 and len(agent.records) == 2
    assert isinstance(agent.model, MiniGPT4Classifier) and agent.model.decode == "hip"
    assert agent.model.decode_stats["hip_steps"] > 0 and agent.model.decode_stats["hf_calls"] == 0
