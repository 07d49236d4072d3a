"""Helpers of the LLaMA GPU tests (tests/test_gpu_llm_*.py), one copy: the random-init decoders, sentinel-filled caches, seeded
inputs, the model's own prefill, and the teacher-forced accuracy criterion of test_gpu_llm_decode.py.  Fixtures stay in their files."""
import copy

import torch

from certifiedgpt_amd.minigpt4 import prepare_texts
from gpu_util import DEV
from test_llm_early_stop_cpu import expected_live_steps  # noqa: F401  (re-exported)

PAD, BOS, EOS = 0, 1, 2
K_SENTINEL, V_SENTINEL, LOGIT_SENTINEL = 77.0, -55.0, 123.0          # what untouched cache rows / step logits hold
PROMPT = prepare_texts(["<Img><ImageHere></Img> [vqa] what is shown in the picture"])[0]


def llama_decoder(hidden, heads, mlp, vocab, layers=2, kv_heads=None, theta=None, sd=None, plant=False):
    """A frozen random-init fp16 LlamaForCausalLM on the device (no checkpoint is in the container; nothing is downloaded).
    kv_heads: fewer K/V heads than query heads (None: as many); theta: rope_theta (None: the config's default); sd: a state dict loaded
    over the random weights; plant: one input_layernorm and one post_attention_layernorm channel of every layer x 50, so that every
    row the q/k/v and gate/up linears read has outliers."""
    from transformers import LlamaConfig, LlamaForCausalLM
    rope = {} if theta is None else {"rope_theta": theta}
    lcfg = LlamaConfig(vocab_size=vocab, hidden_size=hidden, intermediate_size=mlp, num_hidden_layers=layers, num_attention_heads=heads,
                       num_key_value_heads=kv_heads or heads, max_position_embeddings=2048, pad_token_id=PAD, bos_token_id=BOS,
                       eos_token_id=EOS, **rope)
    torch.manual_seed(0)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    try:
        with torch.device(DEV):
            llm = LlamaForCausalLM(lcfg).eval()
    finally:
        torch.set_default_dtype(prev)
    if sd is not None:
        missing, unexpected = llm.load_state_dict(sd, strict=True)
        assert not missing and not unexpected
    for prm in llm.parameters():
        prm.requires_grad = False
    if plant:
        for layer in llm.model.layers:
            layer.input_layernorm.weight[11] *= 50.0
            layer.post_attention_layernorm.weight[301] *= 50.0
    return llm


def small_decoder():
    """Small enough that every weight and logit can be compared: hidden 512 = 4 heads x 128, MLP 1408, vocabulary 320, 2 layers."""
    return llama_decoder(512, 4, 1408, 320)


def vicuna_width_decoder():
    """Vicuna-7B's widths (hidden 4096, 32 heads, MLP 11008, vocabulary 32000) with 2 random-init layers."""
    return llama_decoder(4096, 32, 11008, 32000)


def sentinel_cache(layers, kv_heads, B, length):
    """Per-layer K / V buffers [B, kv_heads, length, 128] fp16, filled with K_SENTINEL / V_SENTINEL."""
    shape = (B, kv_heads, length, 128)
    kb = [torch.full(shape, K_SENTINEL, dtype=torch.float16, device=DEV) for _ in range(layers)]
    vb = [torch.full(shape, V_SENTINEL, dtype=torch.float16, device=DEV) for _ in range(layers)]
    return kb, vb


def ids(llm, B, L, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(3, llm.config.vocab_size, (B, L), generator=g).to(DEV)


def embeds(llm, B, L, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return llm.get_input_embeddings()(torch.randint(3, llm.config.vocab_size, (B, L), generator=g).to(DEV)).contiguous()


def model_prefill(model, embs):
    """(last-position logits fp32, per-layer keys, per-layer values) of the model's own forward."""
    from transformers import DynamicCache
    cache = DynamicCache(config=model.config)
    pos = torch.arange(embs.shape[1], device=embs.device).unsqueeze(0)
    with torch.no_grad():
        out = model(inputs_embeds=embs, position_ids=pos, past_key_values=cache, use_cache=True, logits_to_keep=1)
    return out.logits[:, -1].float(), [l.keys for l in cache.layers], [l.values for l in cache.layers]


def err(a, ref):
    d = (a.float() - ref.float()).abs()
    return float(d.max()), float(d.pow(2).mean().sqrt())


def up256(n):
    return (n + 255) // 256 * 256


def zero_head(llm):
    with torch.no_grad():
        llm.lm_head.weight.zero_()
    return llm


def check_dead_part(L, live, on, off, layers=None):
    """The contract of include/cgpt.h: cache rows L + live .. keep their sentinel on the `on` run, rows L .. L + live - 1 are the off
    run's bit for bit (as are the prompt rows, which no step writes); step logits rows 0 .. live are the off run's, later rows keep
    their sentinel.  `on` / `off`: (tokens, live_steps, K, V, step logits or None) of two runs on `sentinel_cache` buffers."""
    _, _, k_on, v_on, lg_on = on
    _, _, k_off, v_off, lg_off = off
    for l in (range(len(k_on)) if layers is None else layers):
        assert bool((k_on[l][:, :, L + live:] == K_SENTINEL).all()) and bool((v_on[l][:, :, L + live:] == V_SENTINEL).all()), (l, live)
        assert torch.equal(k_on[l][:, :, :L + live], k_off[l][:, :, :L + live]), (l, live)
        assert torch.equal(v_on[l][:, :, :L + live], v_off[l][:, :, :L + live]), (l, live)
        n_off = k_off[l].shape[2] - 1                                  # the off run appended every row but the last (n - 1 steps)
        assert not bool((k_off[l][:, :, L:n_off] == K_SENTINEL).all(dim=-1).any())  # so the sentinel check above says something
    if lg_on is not None:
        assert torch.equal(lg_on[:, :live + 1], lg_off[:, :live + 1])
        assert bool((lg_on[:, live + 1:] == LOGIT_SENTINEL).all())
        assert not bool((lg_off == LOGIT_SENTINEL).all(dim=-1).any())


def cache_from(cfg, keys, values, dtype):
    from transformers import DynamicCache
    c = DynamicCache(config=cfg)
    for l, (k, v) in enumerate(zip(keys, values)):
        c.update(k.to(dtype).clone(), v.to(dtype).clone(), l)
    return c


def prefill(llm, embs, extra):
    """HF prefill of embs [B, L, hidden] -> (last-position logits fp32, per-layer K / V buffers [B, heads, L + extra, 128] whose first
    L rows are HF's cache and whose other rows hold a sentinel)."""
    from transformers import DynamicCache
    B, L, _ = embs.shape
    cache = DynamicCache(config=llm.config)
    with torch.no_grad():
        out = llm(inputs_embeds=embs, position_ids=torch.arange(L, device=DEV)[None], past_key_values=cache, use_cache=True,
                  logits_to_keep=1)
    kb, vb = [], []
    for layer in cache.layers:
        k = torch.full((B, layer.keys.shape[1], L + extra, 128), K_SENTINEL, dtype=torch.float16, device=DEV)
        v = torch.full_like(k, V_SENTINEL)
        k[:, :, :L] = layer.keys
        v[:, :, :L] = layer.values
        kb.append(k)
        vb.append(v)
    return out.logits[:, -1].float(), kb, vb, cache


def teacher_forced(llm, dec, B, L=12, steps=6, seed=3):
    """The accuracy criterion of test_gpu_llm_decode.py's module docstring; returns the per-step figures."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    ids = torch.randint(3, llm.config.vocab_size, (B, L), generator=g).to(DEV)
    embs = llm.get_input_embeddings()(ids)
    llm32 = copy.deepcopy(llm).float()
    logits, kb, vb, cache = prefill(llm, embs, steps)
    tok = logits.argmax(-1)
    rows = []
    for s in range(steps):
        pos = L + s
        keys = [l.keys.clone() for l in cache.layers]
        vals = [l.values.clone() for l in cache.layers]
        for l in range(len(kb)):                                       # HF's own cache, every step
            kb[l][:, :, :pos] = keys[l]
            vb[l][:, :, :pos] = vals[l]
        before = [t.clone() for t in kb + vb]
        lib = dec.step(tok, pos, kb, vb)
        pid = torch.full((1, 1), pos, device=DEV, dtype=torch.long)
        with torch.no_grad():
            hf = llm(input_ids=tok[:, None], position_ids=pid, past_key_values=cache, use_cache=True).logits[:, -1].float()
            c32 = cache_from(llm.config, keys, vals, torch.float32)
            ref = llm32(input_ids=tok[:, None], position_ids=pid, past_key_values=c32, use_cache=True).logits[:, -1].float()
        fin = torch.isfinite(ref) & torch.isfinite(hf) & torch.isfinite(lib)
        assert bool(fin.all())
        e_hf, e_lib = (hf - ref).abs(), (lib - ref).abs()
        # the appended rows.  "Within 1 fp16 ulp of HF's row" needs a magnitude to measure the ulp at.  Measured at each element's own
        # magnitude it is not a property any engine with its own GEMM can have: an element of a key or value row is a dot product (and a
        # rotated key a sum of two rounded products) that may cancel to far below its terms, while one fp16 rounding tipped upstream by
        # another summation order moves it by an ulp of the TERMS (measured: up to 44 own-magnitude ulp in a layer-0 value element, 1536
        # in a rotated key element near zero).  What is asserted instead, for layer 0, whose input teacher forcing makes identical in
        # both engines:
        #   (a) the value row within 1 ulp, the key row within 2 ulp, the ulp taken at the largest element of the head's 128-vector
        #       in HF's row.  2 for keys: a rotation can shrink a pair's larger element by up to sqrt(2), i.e. one binade, so one ulp
        #       of the un-rotated terms reads up to 2 there;
        #   (b) at least 98 % of the row's elements bit-equal to HF's.  An element can differ only where another summation order tips
        #       an fp16 rounding: fp32 accumulation noise of ~sqrt(K) 2^-24 relative against an fp16 spacing of 2^-11..2^-10 is a share
        #       of 0.1 - 0.8 % at K = 512..4096 for the projection, about as much again from the RMSNorm in front of it, and a rotated
        #       key takes two inputs: 1 - 2 % at the very most.  Rounding anywhere ELSE than HF does (a product of the rotary kept
        #       unrounded inside a fused multiply-add, another cos / sin) moves an order of magnitude more: this is the assertion
        #       that guards the rotary rounding contract.
        # Every row of every layer is also held to the yardstick of the logits (from layer 1 on the input carries layer 0's rounding
        # noise, so HF's row is no closer to the fp32 model's than ours): distance to the fp32 row against HF's own.  Every other
        # cache row: bit-unchanged.
        kv = {}
        for l in range(len(kb)):
            for name, mine, theirs, exact, was in (("k", kb[l], cache.layers[l].keys, c32.layers[l].keys, before[l]),
                                                   ("v", vb[l], cache.layers[l].values, c32.layers[l].values, before[len(kb) + l])):
                new, want, ref32 = mine[:, :, pos].float(), theirs[:, :, pos].float(), exact[:, :, pos].float()
                assert bool(torch.isfinite(new).all())
                d_hf, d_lib = (want - ref32).abs(), (new - ref32).abs()
                kv[f"{name}{l}"] = (float(d_lib.max()), float(d_hf.max()), float(d_lib.pow(2).mean().sqrt()), float(d_hf.pow(2).mean().sqrt()),
                                    float((new == want).float().mean()))
                if l == 0:
                    ulp = want.abs().amax(dim=-1, keepdim=True).clamp_min(2.0 ** -14).log2().floor().sub(10).exp2()
                    kv[f"{name}{l}"] += (float(((new - want).abs() / ulp).max()),)
                keep = torch.ones(mine.shape[2], dtype=torch.bool, device=DEV)
                keep[pos] = False
                assert torch.equal(mine[:, :, keep], was[:, :, keep])
        rows.append({"step": s, "max_hf": float(e_hf.max()), "max_lib": float(e_lib.max()),
                     "rms_hf": float(e_hf.pow(2).mean().sqrt()), "rms_lib": float(e_lib.pow(2).mean().sqrt()),
                     "max_lib_vs_hf": float((lib - hf).abs().max()), "max_logit": float(hf.abs().max()), "kv": kv})
        tok = hf.argmax(-1)                                            # HF's own token
    del llm32
    return rows


def check_ratios(name, rows):
    for r in rows:
        print(f"[teacher-forced {name}] step {r['step']}: max e_lib / max e_hf = {r['max_lib'] / r['max_hf']:.3f} "
              f"({r['max_lib']:.4g} / {r['max_hf']:.4g}), rms ratio {r['rms_lib'] / r['rms_hf']:.3f} "
              f"({r['rms_lib']:.4g} / {r['rms_hf']:.4g}), max |lib - hf| {r['max_lib_vs_hf']:.4g}, max |logit| {r['max_logit']:.4g}", flush=True)
        print("    appended rows, (max, rms) error ratio library / HF against the fp32 model, share of elements equal to HF's: "
              + ", ".join(f"{k} ({v[0] / v[1]:.2f}, {v[2] / v[3]:.2f}, {v[4]:.4f})" for k, v in r["kv"].items())
              + f"; layer 0 largest difference in head-max ulp: k {r['kv']['k0'][5]:.2f}, v {r['kv']['v0'][5]:.2f}", flush=True)
    for r in rows:
        assert r["max_lib"] <= 1.5 * r["max_hf"], r
        assert r["rms_lib"] <= 1.5 * r["rms_hf"], r
        for k, v in r["kv"].items():
            assert v[0] <= 1.5 * v[1] and v[2] <= 1.5 * v[3], (r["step"], k, v)
        assert r["kv"]["v0"][5] <= 1.0 and r["kv"]["k0"][5] <= 2.0, (r["step"], r["kv"]["v0"], r["kv"]["k0"])     # head-max ulp
        assert r["kv"]["v0"][4] >= 0.98 and r["kv"]["k0"][4] >= 0.98, (r["step"], r["kv"]["v0"], r["kv"]["k0"])   # bit-equal share
