"""weights="int8": row-wise absmax int8 layer linears on the native LLaMA engine (cgpt_llm_config.weight_format = CGPT_LLM_W_INT8).

The central property is EXACT.  By definition every result of an int8 handle is the result of the existing fp16 engine whose layer
linears were loaded with W' = fp16(q) * s (`int8_state_dict`, evaluated here on the CPU): the quantising kernel implements the law
of `quantize_rows_int8`, and both readers of q (the int8-weight decode GEMM, the prefill's expansion into the fp16 scratch) form W'
with one fp16 multiply and then run the fp16 kernels' arithmetic.  So an int8 handle loaded from the model W is compared with an
fp16 handle loaded from the W' twin by `torch.equal` -- logits, tokens, every cache row -- with no tolerance.

What the quantisation itself costs is MEASURED, not bounded: the last test prints, against an fp32 copy of the original W
(e = distance to the fp32 model, the yardstick of test_gpu_llm_prefill.py), max e_int8 / max e_hf_fp16 and the rms ratio for the
last-position logits and K/V, and how many of 200 rows keep the fp16 engine's greedy trajectory (`greedy_decode_parity`); it asserts
only that everything is finite.  Figures of the run that produced DESIGN.md 4.4.3 are recorded there."""
import copy

import pytest
import torch

import certifiedgpt_amd as cg
from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap
from certifiedgpt_amd.minigpt4 import (MiniGPT4Classifier, WordHashTokenizer, _HipDecoder, greedy_decode_parity, int8_state_dict,
                                       left_pad_embeds)
from oracle import model_oracle as mo
from gpu_util import DEV, make_classifier
import llm_util as lu
from llm_util import PAD, EOS, K_SENTINEL, PROMPT

pytestmark = pytest.mark.gpu


def _twin(llm):
    """The HF twin whose layer linears are W', the law evaluated on the CPU (the reference evaluation)."""
    twin = copy.deepcopy(llm)
    missing, unexpected = twin.load_state_dict(int8_state_dict(llm, device="cpu"), strict=True)
    assert not missing and not unexpected
    return twin


class _Pair:
    def __init__(self, hidden, heads, mlp, vocab):
        self.llm = lu.llama_decoder(hidden, heads, mlp, vocab)
        self.twin = _twin(self.llm)
        self.int8 = _HipDecoder(self.llm, 200, weights="int8")         # quantised by the library from W
        self.fp16 = _HipDecoder(self.twin, 200)                        # the existing fp16 engine on W'

    def close(self):
        self.int8.close()
        self.fp16.close()


@pytest.fixture(scope="module")
def small():
    """hidden 512 = 4 heads x 128, MLP 1408, vocabulary 320, 2 layers."""
    p = _Pair(512, 4, 1408, 320)
    yield p
    p.close()


@pytest.fixture(scope="module")
def vicuna():
    """Vicuna-7B's widths (hidden 4096, 32 heads, MLP 11008, vocabulary 32000) with 2 random-init layers."""
    p = _Pair(4096, 32, 11008, 32000)
    yield p
    p.close()
    del p
    torch.cuda.empty_cache()


def _same_caches(a, b, where):
    for l, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{where}: cache of layer {l} differs"


def test_the_quantised_model_differs_from_the_model(small):
    """The comparison below is not vacuous: W' is not W, and the two engines of the pair hold different things."""
    sd, sd_t = small.llm.state_dict(), small.twin.state_dict()
    name = "model.layers.1.mlp.down_proj.weight"
    assert not torch.equal(sd[name], sd_t[name]) and torch.equal(sd["lm_head.weight"], sd_t["lm_head.weight"])
    assert small.int8.weights == "int8" and small.fp16.weights == "fp16"


# ------------------------------------------------------------------------------------------ 1. teacher-forced steps
@pytest.mark.parametrize("which", ["small", "vicuna"])
@pytest.mark.parametrize("B", [200, 37])
def test_teacher_forced_steps_equal_the_fp16_engine_on_the_dequantised_weights(which, B, request):
    p = request.getfixturevalue(which)
    L, steps = 44, 4
    embs = lu.embeds(p.llm, B, L, seed=B)
    g = torch.Generator(device="cpu").manual_seed(7 + B)
    forced = torch.randint(3, p.llm.config.vocab_size, (steps, B), generator=g).to(DEV)
    got = {}
    for name, dec in (("int8", p.int8), ("fp16", p.fp16)):
        kb, vb = lu.sentinel_cache(p.llm.config.num_hidden_layers, p.llm.config.num_attention_heads, B, L + steps + 2)
        logits = [dec.prefill(embs, kb, vb)]
        for i in range(steps):
            logits.append(dec.step(forced[i].contiguous(), L + i, kb, vb))
        torch.cuda.synchronize()
        got[name] = (torch.stack(logits), kb, vb)
    assert bool(torch.isfinite(got["int8"][0]).all())
    for i in range(steps + 1):
        assert torch.equal(got["int8"][0][i], got["fp16"][0][i]), \
            f"{which}, {B} rows: logits of {'the prefill' if i == 0 else f'step {i}'} differ, max " \
            f"{float((got['int8'][0][i] - got['fp16'][0][i]).abs().max())}"
    _same_caches(got["int8"][1], got["fp16"][1], f"{which}, {B} rows: K")           # appended rows AND sentinels: nothing else written
    _same_caches(got["int8"][2], got["fp16"][2], f"{which}, {B} rows: V")
    assert bool((got["int8"][1][0][:, :, L + steps:] == K_SENTINEL).all())


# ------------------------------------------------------------------------------------------ 2. prefill and greedy
def _run(dec, llm, embs, n_new, starts=None):
    B, L = embs.shape[:2]
    kb, vb = lu.sentinel_cache(llm.config.num_hidden_layers, llm.config.num_attention_heads, B, L + n_new + 1)
    first = dec.prefill(embs, kb, vb, starts=starts)
    tokens, steps = dec.greedy(first, L, n_new, 1, [EOS], PAD, kb, vb, return_logits=True, starts=starts)
    torch.cuda.synchronize()
    return first, tokens, steps, kb, vb


def _assert_same_run(a, b, where):
    assert bool(torch.isfinite(a[0]).all())
    assert torch.equal(a[0], b[0]), f"{where}: last-position logits differ, max {float((a[0] - b[0]).abs().max())}"
    assert torch.equal(a[1], b[1]), f"{where}: tokens differ"
    assert torch.equal(a[2], b[2]), f"{where}: step logits differ"
    _same_caches(a[3], b[3], where + " K")
    _same_caches(a[4], b[4], where + " V")


@pytest.mark.parametrize("L", [1, 12, 44, 70, 300])
def test_prefill_and_greedy_equal_the_fp16_engine_small_decoder(small, L):
    embs = lu.embeds(small.llm, 37, L, seed=L)
    _assert_same_run(_run(small.int8, small.llm, embs, 5), _run(small.fp16, small.twin, embs, 5), f"small decoder, 37 rows, L {L}")


@pytest.mark.parametrize("B, L", [(200, 12), (200, 44), (37, 12), (37, 44)])
def test_prefill_and_greedy_equal_the_fp16_engine_vicuna_width(vicuna, B, L):
    embs = lu.embeds(vicuna.llm, B, L, seed=B + L)
    _assert_same_run(_run(vicuna.int8, vicuna.llm, embs, 5), _run(vicuna.fp16, vicuna.twin, embs, 5), f"Vicuna width, {B} rows, L {L}")


def test_left_padded_rows_through_the_ragged_entries(small):
    L, n_new = 48, 5
    g = torch.Generator(device="cpu").manual_seed(48)
    lens = torch.randint(1, L + 1, (60,), generator=g).tolist()
    embs, _, starts = left_pad_embeds([lu.embeds(small.llm, 1, n, seed=100 + i) for i, n in enumerate(lens)])
    assert embs.shape[1] == max(lens) and len(set(lens)) > 10
    embs, starts = embs.contiguous(), starts.to(DEV)
    a = _run(small.int8, small.llm, embs, n_new, starts)               # cgpt_llm_prefill_ragged, _greedy_ragged (-> _step_ragged's kernels)
    b = _run(small.fp16, small.twin, embs, n_new, starts)
    _assert_same_run(a, b, "ragged, small decoder")
    cfg = small.llm.config                                             # and the step entry itself, teacher-forced
    kb, vb = lu.sentinel_cache(cfg.num_hidden_layers, cfg.num_attention_heads, 60, embs.shape[1] + 2)
    kb2, vb2 = lu.sentinel_cache(cfg.num_hidden_layers, cfg.num_attention_heads, 60, embs.shape[1] + 2)
    small.int8.prefill(embs, kb, vb, starts=starts)
    small.fp16.prefill(embs, kb2, vb2, starts=starts)
    tok = torch.randint(3, 320, (60,), generator=g).to(DEV)
    la = small.int8.step(tok, embs.shape[1], kb, vb, starts=starts)
    lb = small.fp16.step(tok, embs.shape[1], kb2, vb2, starts=starts)
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    _same_caches(kb + vb, kb2 + vb2, "ragged step")
    # a padded row on the int8 engine is still the row alone
    n = lens[0]
    solo = _run(small.int8, small.llm, embs[:1, embs.shape[1] - n:].contiguous(), n_new)
    assert torch.equal(solo[0], a[0][:1]) and torch.equal(solo[1], a[1][:1]) and torch.equal(solo[2], a[2][:1])


# ------------------------------------------------------------------------------------------ 3. graphs and batch independence
def test_graph_replays_and_row_splits_are_bit_identical(vicuna):
    """One capture of prefill + greedy replayed twice gives the eager bits (the scratch is reused by every layer: stream order inside
    the graph must hold), and 200 rows equal the same rows run as 128 + 72: 2400 / 1536 token rows take the large-shape kernel,
    864 take the 128 x 128 kernel, all of them reading the scratch."""
    L, n_new = 12, 4
    embs = lu.embeds(vicuna.llm, 200, L, seed=3)
    eager = _run(vicuna.int8, vicuna.llm, embs, n_new)
    static = embs.clone()
    kb, vb = lu.sentinel_cache(vicuna.llm.config.num_hidden_layers, vicuna.llm.config.num_attention_heads, 200, L + n_new + 1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        first = vicuna.int8.prefill(static, kb, vb)
        tokens, steps = vicuna.int8.greedy(first, L, n_new, 1, [EOS], PAD, kb, vb, return_logits=True)
    for _ in range(2):
        for t in kb + vb:
            t.fill_(3.0)
        first.zero_(), tokens.zero_(), steps.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(first, eager[0]) and torch.equal(tokens, eager[1]) and torch.equal(steps, eager[2])
        for l in range(len(kb)):
            assert torch.equal(kb[l][:, :, :L + n_new - 1], eager[3][l][:, :, :L + n_new - 1])
            assert torch.equal(vb[l][:, :, :L + n_new - 1], eager[4][l][:, :, :L + n_new - 1])
    del graph
    for lo, hi in ((0, 128), (128, 200)):
        part = _run(vicuna.int8, vicuna.llm, embs[lo:hi].contiguous(), n_new)
        where = f"rows {lo}..{hi} alone"
        assert torch.equal(part[0], eager[0][lo:hi]), where
        assert torch.equal(part[1], eager[1][lo:hi]) and torch.equal(part[2], eager[2][lo:hi]), where
        for l in range(len(kb)):
            assert torch.equal(part[3][l], eager[3][l][lo:hi]) and torch.equal(part[4][l], eager[4][l][lo:hi]), where


# ------------------------------------------------------------------------------------------ 4. the bytes
@pytest.mark.parametrize("which", ["small", "vicuna"])
def test_weight_bytes_is_the_formula(which, request):
    p = request.getfixturevalue(which)
    c = p.llm.config
    H, F, V, layers = c.hidden_size, c.intermediate_size, c.vocab_size, c.num_hidden_layers
    mats = [(3 * H, H), (H, H), (2 * F, H), (H, F)]                    # fused q/k/v, o, fused gate/up, down: [N, K]
    table = 2 * V * H * 2                                              # embed_tokens and lm_head, fp16
    scratch = max(lu.up256(n) * k for n, k in mats) * 2                  # one fp16 matrix, the largest: up256(2 mlp) x hidden
    assert scratch == lu.up256(2 * F) * H * 2
    int8 = layers * sum(lu.up256(n) * k + lu.up256(n) * 2 for n, k in mats) + table + scratch     # int8 rows + fp16 scales, padded alike
    fp16 = layers * sum(lu.up256(n) * k * 2 for n, k in mats) + table
    assert p.int8.weight_bytes == int8, (p.int8.weight_bytes, int8)
    assert p.fp16.weight_bytes == fp16, (p.fp16.weight_bytes, fp16)
    assert p.int8.weight_bytes < p.fp16.weight_bytes
    if which == "vicuna":                                              # the 7B figure of DESIGN.md 4.4.3, from the same formula
        full = lambda per_layer, extra: 32 * per_layer + table + extra  # noqa: E731
        i32 = full(sum(lu.up256(n) * k + lu.up256(n) * 2 for n, k in mats), scratch)
        f32 = full(sum(lu.up256(n) * k * 2 for n, k in mats), 0)
        print(f"[weight_bytes, 7B widths x 32 layers, derived] int8 {i32 / 1e9:.3f} GB, fp16 {f32 / 1e9:.3f} GB, ratio {i32 / f32:.3f}", flush=True)


# ------------------------------------------------------------------------------------------ 5. the classifier at Vicuna width
def test_classifier_answers_and_certificate_equal_the_fp16_engine_on_the_dequantised_model(vicuna):
    cfg = mo.Config(mode=mo.MODE_ENCODE_IMG, num_classes=10)
    enc = make_classifier(cfg, max_batch=100)
    try:
        enc.init_synthetic(seed=0)
        tok = WordHashTokenizer(32000)
        x = torch.from_numpy(mo.synthetic_image(cfg, seed=11)).to(DEV)
        B, n, sigma, seed = 200, 20, 0.5, 42
        emb = torch.cat([enc.encode_img_noisy(x, lo, 100, sigma, seed) for lo in (0, 100)]).to(torch.float16)
        kw = dict(max_new_tokens=n, max_batch=B, decode="hip", prefill="hip")
        calls = {"n": 0}
        hooks = [m.register_forward_pre_hook(lambda *_: calls.__setitem__("n", calls["n"] + 1)) for m in (vicuna.llm, vicuna.twin)]
        try:
            q8 = MiniGPT4Classifier(enc, vicuna.llm, tok, PROMPT, AnswerLabelMap(4, ()), weights="int8", **kw)
            ref = MiniGPT4Classifier(enc, vicuna.twin, tok, PROMPT, AnswerLabelMap(4, ()), **kw)
            answers = q8.generate_from_embeds(emb, PROMPT)
            want = ref.generate_from_embeds(emb, PROMPT)
            assert len(answers) == B
            for i, (a, b) in enumerate(zip(answers, want)):
                assert a == b, f"row {i}: {a!r} != {b!r}"
            assert q8.generate_from_embeds(emb, PROMPT) == answers
            s = q8.decode_stats
            assert s["hf_calls"] == 0 and s["hip_prefills"] == 2 and s["hip_steps"] == 2 * (n - 1) and s["graph_captures"] == 1
            assert s["weight_bytes"] == vicuna.int8.weight_bytes and ref.decode_stats["weight_bytes"] == vicuna.fp16.weight_bytes
            # ragged="hip" with a bucket: the same answers from the padded path
            pad = MiniGPT4Classifier(enc, vicuna.llm, tok, PROMPT, AnswerLabelMap(4, ()), weights="int8", ragged="hip", prompt_bucket=16, **kw)
            assert pad.generate_from_embeds(emb, PROMPT) == answers and pad.decode_stats["hf_calls"] == 0
            del pad
            # certify: same label, radius and answers
            vocab = sorted(set(answers), key=lambda a: (-answers.count(a), a))[:3]
            results = []
            for llm, extra in ((vicuna.llm, dict(weights="int8")), (vicuna.twin, {})):
                clf = MiniGPT4Classifier(enc, llm, tok, PROMPT, AnswerLabelMap(len(vocab) + 1, vocab, frozen=True), **kw, **extra)
                sm = cg.Smooth(clf, len(vocab) + 1, sigma, seed=seed, non_certifiable=(clf.label_map.other_id,))
                results.append((sm.certify(x, 100, 100, 0.001, 100), list(clf.last_answers), dict(clf.decode_stats)))
                del clf, sm
            assert calls["n"] == 0                                     # no HF forward ran on either model
        finally:
            for h in hooks:
                h.remove()
        (lab_a, rad_a), ans_a, st_a = results[0]
        (lab_b, rad_b), ans_b, st_b = results[1]
        print(f"[certify, weights=int8] {(lab_a, rad_a)} against {(lab_b, rad_b)} on the dequantised model; {len(set(ans_a))} distinct answers",
              flush=True)
        assert (lab_a, rad_a) == (lab_b, rad_b) and ans_a == ans_b and len(ans_a) == 200
        assert st_a["hf_calls"] == st_b["hf_calls"] == 0
    finally:
        enc.close()


# ------------------------------------------------------------------------------------------ 6. what the quantisation costs (measured)
def _cost(name, llm, B, L, n_new):
    """Figures of one model: error ratios int8 engine / HF fp16 against the fp32 model, and the trajectories against the fp16 ENGINE
    on the same (unquantised) weights."""
    d8, d16 = _HipDecoder(llm, B, weights="int8"), _HipDecoder(llm, B)
    try:
        embs = lu.embeds(llm, B, L, seed=5)
        q = _run(d8, llm, embs, n_new)
        f = _run(d16, llm, embs, n_new)
        hf, hk, hv = lu.model_prefill(llm, embs)
        llm32 = copy.deepcopy(llm).float()
        ref, rk, rv = lu.model_prefill(llm32, embs.float())
        del llm32
        figures = {"logits": lu.err(q[0], ref) + lu.err(hf, ref)}
        for l in range(len(hk)):
            figures[f"k{l}"] = lu.err(q[3][l][:, :, :L], rk[l]) + lu.err(hk[l], rk[l])
            figures[f"v{l}"] = lu.err(q[4][l][:, :, :L], rv[l]) + lu.err(hv[l], rv[l])
        # step 0 of the greedy loop reads -inf in the EOS column (min_new = 1): every later step's logits must be finite
        finite = all(bool(torch.isfinite(t).all()) for t in (q[0], q[2][:, 1:], f[0], hf, ref, q[3][0][:, :, :L], q[4][0][:, :, :L]))
        d_first = float((q[0] - f[0]).abs().max())
        v = greedy_decode_parity(f[1], f[2], q[1], 2.0 * d_first)
        print(f"[int8 cost, {name}, {B} rows x {L} positions, {n_new} tokens] (max, rms) error ratio int8 engine / HF fp16 against the fp32 "
              "model: " + ", ".join(f"{k} ({x[0] / x[2]:.2f}, {x[1] / x[3]:.2f})" for k, x in figures.items())
              + f"; first-token max |int8 - fp16 engine| {d_first:.4g} at max |logit| {float(f[0].abs().max()):.4g}; "
              f"{v['identical']}/{B} rows keep the fp16 engine's trajectory, {v['decisive_identical']}/{v['decisive']} decisive rows "
              f"(eps {2.0 * d_first:.4g}), {len(v['violations'])} rows leave it at a decisive step", flush=True)
        return finite
    finally:
        d8.close()
        d16.close()


def test_quantisation_cost_is_measured_and_finite(small, vicuna):
    """Measured, not bounded (see the module docstring).  Random-init weights are near-Gaussian rows without outlier elements and
    quantise more kindly than trained ones; the third leg rescales rows 3, 61, 97, 170 of every o_proj / down_proj by the stress
    law's outlier factor (oracle.model_oracle.stress_params: outlier / 4 = 8), which puts outlier channels into the residual
    stream the next layer's quantised linears read."""
    assert _cost("small decoder", small.llm, 200, 44, 20)
    assert _cost("Vicuna width, 2 layers", vicuna.llm, 200, 44, 20)
    stressed = copy.deepcopy(vicuna.llm)
    sd = stressed.state_dict()
    for name, w in sd.items():
        if name.endswith("o_proj.weight") or name.endswith("down_proj.weight"):
            w[list(mo.STRESS_OUTLIER_CHANNELS)] *= 32.0 / 4.0
    assert _cost("Vicuna width, 2 layers, outlier rows x 8", stressed, 200, 44, 20)
