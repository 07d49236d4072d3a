"""Device time of the greedy decode of BASELINE configs[2] on the "graph" engine (PyTorch-ROCm steps, cgpt prefill), on the "hip"
engine (this library's token steps after the model's own prefill, its linears routed through this library's GEMM) and on
"hip_native" (decode="hip", prefill="hip": prefill and steps in this library), interleaved in one process.

Vicuna-7B-shaped random-init decoder (no checkpoint exists here; nothing is downloaded), 200 rows, a prompt of 44 positions, 20 new
tokens.  Per repetition and engine, by HIP events around graph replays:
    generate_ms  = one whole `generate_from_embeds`-shaped replay (prefill + 20 selects + 19 steps)
    prefill_ms   = the same classifier with max_new_tokens = 1 (prefill + 1 select, no step)
    steps_ms     = generate_ms - prefill_ms  (the 19 steps and their selects), step_ms = steps_ms / 19
Prints ONE JSON line.  The floor quoted beside it is bytes / copy rate: the decoder's weight bytes plus the mean K / V bytes a step
reads, over 6.3 TB/s (the copy rate the box reaches).

--ragged runs the left-padding leg instead (ragged="hip"), same protocol, every engine decode="hip", prefill="hip":
    plain       the shared prompt of --prompt positions on the plain entries (today's path)
    bucketed    the same prompt left-padded to --bucket-len positions (one common start): the cost of the pad rows
    ragged      rows of lengths --ragged-min .. --bucket-len (fixed seed), left-padded to --bucket-len -- the SAME captured graph as
                `bucketed`, other contents of the starts tensor
    hf_ragged   today's fallback for those rows: eager HF `generate` with the attention mask (generate_ms only)
    parent      `plain` on another build of the library (--parent-lib PATH, e.g. the parent commit's libcgpt.so), loaded beside
                the product in this process: the claim to check is that the plain path's time is unchanged

--act-int8 adds a third engine to the weight-format leg below: weights="int8" with activations="int8" (quantise +
int8-MFMA GEMM per layer linear, per-row outlier split), reported against both other engines.
--int8 runs the weight-format leg instead (weights="int8"), same protocol, every engine decode="hip", prefill="hip":
    fp16        the engine's own fp16 copies (today's path)
    int8        row-wise absmax int8 layer linears: the int8-weight decode GEMM in the steps, a dequant pass before each prefill GEMM
    parent      `fp16` on another build of the library (--parent-lib PATH), as under --ragged
and reports the handles' weight_bytes beside the times.

--early-stop runs the early-stop leg instead (early_stop=True), same protocol, every engine decode="hip", prefill="hip".
The finishing step is set exactly, without a trained model: lm_head is zeroed (the layers stay random) and eos_token_id = 0, so every
logit is 0, the select picks token 1 while EOS is masked (min_length = F generated tokens) and token 0 = EOS for every row at select F:
    off         early stop off, the law that never finishes (today's path: every step runs whatever the law)
    on_never    early stop on, min_length = --new: no row ever finishes -- what the guards and the reduction cost a batch that runs on
    on_f1/on_f3 early stop on, every row finishes at select 1 / 3: 18 / 16 of the 19 steps are dead
    parent      `off` on another build of the library (--parent-lib PATH), as under --ragged
The order of the legs is rotated from one repetition to the next.  dead_step_ms = the live step minus the saving per skipped step,
(generate(on_never) - generate(on_fF)) / (19 - F).

--stop runs the stop-sequence leg instead (stop_words_ids), same protocol with the rotated leg order, every engine
decode="hip", prefill="hip".  lm_head is zeroed and there is no EOS id, so every logit is 0 and every token is 0:
    off         no stop sequences, early stop off (today's path)
    never       8 sequences of 8 ids beyond the vocabulary, which no row can produce: what the comparisons in the select cost
    on_k1/on_k3 early stop on and the sequence "k zeros": every row finishes at select k - 1, 19 / 17 of the 19 steps are dead
    parent      `off` on another build of the library (--parent-lib PATH), as under --ragged

--gqa runs the grouped-query leg instead (grouped_kv=True), same protocol with the rotated leg order, on a
Llama-3-8B-shaped random-init decoder (hidden 4096, 32 query / 8 K/V heads, MLP 14336, rope_theta 500000, --gqa-vocab tokens):
    gqa         decode="hip", prefill="hip", grouped_kv=True: prefill and steps in this library, caches of 8 heads
    graph       decode="graph" on the same model (PyTorch-ROCm steps replayed from one graph)
    plain       with --parent-lib: the DEFAULT path (no keyword) on the Vicuna-7B-shaped decoder of the other legs, this build
    parent      the same on another build of the library (--parent-lib PATH): the claim to check is that the default path is unchanged
and reports the grouped engine's K/V pool bytes and weight_bytes beside the times.

--sample runs the sampled-decode leg instead (sample="hip"), same protocol with the rotated leg order, every engine
decode="hip", prefill="hip", no EOS id (every row runs every step):
    greedy      the arg-max select (today's path)
    sampled     `Chat.answer`'s settings on the native sampler: do_sample, top_p 0.9, repetition_penalty 1.05, temperature 1.0 and
                HF's default top_k 50; draw ids 0 .. rows - 1, seed 0
    parent      `greedy` on another build of the library (--parent-lib PATH), as under --ragged
sampler_ms_per_select = (generate(sampled) - generate(greedy)) / --new, from the medians: what the sampler costs beyond the arg-max.

--shared-prefix runs the shared-prefix leg instead (shared_prefix=True), same protocol with the rotated leg order,
every engine decode="hip", prefill="hip".  A prompt is P positions every row shares (random tokens, one row's) + L - P positions of
the row's own, at two shapes: (--prefix-len, --prompt), default (7, 44), and (--prefix-len2, --prompt2), default (40, 80):
    plain_L     the whole prompt of L positions on the plain entries, flag off (today's path)
    prefix_L    flag on: the graph copies the one-row prefix cache into every row (cgpt_llm_kv_broadcast) and prefills the L - P
                other positions on top of it (cgpt_llm_prefill_from); the one-row prefill of the prefix ran once, before the timing
    parent      `plain` at the first shape on another build of the library (--parent-lib PATH), as under --ragged
A speed-up is stated only where the slowest flagged repetition beats the fastest plain one (`slowest_prefix_beats_fastest_plain`).
broadcast_ms is the broadcast alone, eagerly (one launch per layer) on caches of the call's shape, by HIP events; prefix_miss_ms the
one-row prefill of the prefix, alike."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap  # noqa: E402
from certifiedgpt_amd.minigpt4 import MiniGPT4Classifier, WordHashTokenizer  # noqa: E402

COPY_RATE = 6.3e12


class _Rows:
    """Stands where the encoder stands: only `max_batch` is read on this path."""
    def __init__(self, n):
        self.max_batch = n


def _decoder(layers, dev, kv_heads=32, mlp=11008, vocab=32000, theta=10000.0):
    from transformers import LlamaConfig, LlamaForCausalLM
    lcfg = LlamaConfig(vocab_size=vocab, hidden_size=4096, intermediate_size=mlp, num_hidden_layers=layers, num_attention_heads=32,
                       num_key_value_heads=kv_heads, max_position_embeddings=2048, pad_token_id=0, bos_token_id=1, eos_token_id=2,
                       rope_theta=theta)
    torch.manual_seed(0)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    try:
        with torch.device(dev):
            llm = LlamaForCausalLM(lcfg).eval()
    finally:
        torch.set_default_dtype(prev)
    for prm in llm.parameters():
        prm.requires_grad = False
    return llm


def _clock():
    try:
        return int(torch.cuda.clock_rate())
    except Exception as e:  # noqa: BLE001 -- the figure is a note beside the result, never an input to it
        return f"unavailable ({type(e).__name__})"


def _other_library(path):
    """Context: `_lib.lib()` answers with the build at `path` (entries it lacks stay unbound), so a decoder created inside binds it."""
    import contextlib
    import ctypes as C
    from certifiedgpt_amd import _lib

    @contextlib.contextmanager
    def ctx():
        _lib.lib()
        other = C.CDLL(path)
        for name, (res, argtypes) in _lib.SIGNATURES.items():
            if hasattr(other, name):
                fn = getattr(other, name)
                fn.restype, fn.argtypes = res, argtypes
        saved, _lib._lib = _lib._lib, other
        try:
            yield
        finally:
            _lib._lib = saved
    return ctx()


def ragged_leg(args, llm, embs, tok, lm):
    from certifiedgpt_amd.minigpt4 import left_pad_embeds
    dev, Lb, rows = embs.device, args.bucket_len, args.rows
    assert args.prompt <= Lb and 1 <= args.ragged_min <= Lb

    def build(n, **kw):
        return MiniGPT4Classifier(_Rows(rows), llm, tok, "<ImageHere>", lm, max_new_tokens=n, max_batch=rows, decode="hip", prefill="hip", **kw)

    clfs = {("plain", n): build(n) for n in (args.new, 1)}
    clfs.update({("padded", n): build(n, ragged="hip", prompt_bucket=Lb) for n in (args.new, 1)})
    legs = ["plain", "bucketed", "ragged", "hf_ragged"]
    if args.parent_lib:
        with _other_library(args.parent_lib):
            clfs.update({("parent", n): build(n) for n in (args.new, 1)})
        legs.append("parent")
    g = torch.Generator(device="cpu").manual_seed(2)
    lens = torch.randint(args.ragged_min, Lb + 1, (rows,), generator=g).tolist()
    wide = llm.get_input_embeddings()(torch.randint(3, 32000, (rows, Lb), generator=g).to(dev))
    b_embs, _, b_starts = left_pad_embeds([embs], Lb)
    r_embs, r_mask, r_starts = left_pad_embeds([wide[i:i + 1, Lb - n:] for i, n in enumerate(lens)], Lb)
    hf_kw = clfs[("plain", args.new)].hf_generate_kwargs()
    inputs = {"plain": (embs, None), "parent": (embs, None), "bucketed": (b_embs, b_starts), "ragged": (r_embs, r_starts)}
    which = {"plain": "plain", "parent": "parent", "bucketed": "padded", "ragged": "padded"}

    def timed(leg, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if leg == "hf_ragged":
            out = llm.generate(inputs_embeds=r_embs, attention_mask=r_mask, max_new_tokens=n, **hf_kw)
        else:
            out = clfs[(which[leg], n)]._generate_graph(*inputs[leg])
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    clock_before = _clock()
    res = {e: {"generate_ms": [], "prefill_ms": []} for e in legs}
    tokens = {}
    with torch.no_grad():
        for rep_i in range(args.warmup + args.reps):                   # interleaved: leg by leg inside every repetition
            for e in legs:
                t, out = timed(e, args.new)
                tp = timed(e, 1)[0]
                print(f"decode_step_bench: repetition {rep_i} {e} generate {t:.1f} ms prefill {tp:.1f} ms", file=sys.stderr, flush=True)
                if rep_i >= args.warmup:
                    res[e]["generate_ms"].append(t)
                    res[e]["prefill_ms"].append(tp)
                    tokens[e] = out
    clock_after = _clock()
    steps = args.new - 1
    for r in res.values():
        r["step_ms"] = [(gm - pm) / steps for gm, pm in zip(r["generate_ms"], r["prefill_ms"])]
        for k in ("generate_ms", "prefill_ms", "step_ms"):
            r[k + "_min_max"] = [min(r[k]), max(r[k])]
    padded = clfs[("padded", args.new)].decode_stats

    def overlap(a, b, k):
        (a0, a1), (b0, b1) = res[a][k + "_min_max"], res[b][k + "_min_max"]
        return a0 <= b1 and b0 <= a1

    def med(e, k):
        return sorted(res[e][k])[len(res[e][k]) // 2]

    line = {"tool": "decode_step_bench", "leg": "ragged", "rows": rows, "prompt": args.prompt, "bucket_len": Lb,
            "ragged_lengths_min_max_mean": [min(lens), max(lens), sum(lens) / len(lens)], "new_tokens": args.new, "layers": args.layers,
            "reps": args.reps, "warmup": args.warmup, "engines": res,
            "bucketed_over_plain_median": {k: med("bucketed", k) / med("plain", k) for k in ("prefill_ms", "step_ms", "generate_ms")},
            "token_rows_ratio": Lb / args.prompt,
            "ragged_over_hf_ragged_generate_median": med("ragged", "generate_ms") / med("hf_ragged", "generate_ms"),
            "padded_graph_captures_replays": [padded["graph_captures"], padded["graph_replays"]],      # bucketed and ragged share ONE graph
            "bucketed_rows_with_plain_tokens": int((tokens["bucketed"] == tokens["plain"]).all(dim=1).sum()),
            "shader_clock_mhz_before_after": [clock_before, clock_after], "device": torch.cuda.get_device_name(0)}
    if "parent" in res:
        line["parent_lib"] = os.path.basename(args.parent_lib)
        line["plain_and_parent_ranges_overlap"] = {k: overlap("plain", "parent", k) for k in ("prefill_ms", "step_ms", "generate_ms")}
        line["plain_rows_with_parent_tokens"] = int((tokens["plain"] == tokens["parent"]).all(dim=1).sum())
    print(json.dumps(line))


def int8_leg(args, llm, embs, tok, lm):
    rows = args.rows

    def build(n, **kw):
        return MiniGPT4Classifier(_Rows(rows), llm, tok, "<ImageHere>", lm, max_new_tokens=n, max_batch=rows, decode="hip", prefill="hip", **kw)

    legs = ["fp16", "int8"]
    clfs = {("fp16", n): build(n) for n in (args.new, 1)}
    clfs.update({("int8", n): build(n, weights="int8") for n in (args.new, 1)})
    if args.act_int8:                                                  # W8A8 with the outlier split beside W8A16 and fp16
        clfs.update({("act_int8", n): build(n, weights="int8", activations="int8") for n in (args.new, 1)})
        legs.append("act_int8")
    if args.parent_lib:
        with _other_library(args.parent_lib):
            clfs.update({("parent", n): build(n) for n in (args.new, 1)})
        legs.append("parent")

    def timed(leg, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = clfs[(leg, n)]._generate_graph(embs)
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    clock_before = _clock()
    res = {e: {"generate_ms": [], "prefill_ms": []} for e in legs}
    tokens = {}
    with torch.no_grad():
        for rep_i in range(args.warmup + args.reps):                   # interleaved: leg by leg inside every repetition
            for e in legs:
                t, out = timed(e, args.new)
                tp = timed(e, 1)[0]
                print(f"decode_step_bench: repetition {rep_i} {e} generate {t:.1f} ms prefill {tp:.1f} ms", file=sys.stderr, flush=True)
                if rep_i >= args.warmup:
                    res[e]["generate_ms"].append(t)
                    res[e]["prefill_ms"].append(tp)
                    tokens[e] = out
    clock_after = _clock()
    steps = args.new - 1
    for r in res.values():
        r["step_ms"] = [(gm - pm) / steps for gm, pm in zip(r["generate_ms"], r["prefill_ms"])]
        for k in ("generate_ms", "prefill_ms", "step_ms"):
            r[k + "_min_max"] = [min(r[k]), max(r[k])]

    def overlap(a, b, k):
        (a0, a1), (b0, b1) = res[a][k + "_min_max"], res[b][k + "_min_max"]
        return a0 <= b1 and b0 <= a1

    def med(e, k):
        return sorted(res[e][k])[len(res[e][k]) // 2]

    keys = ("prefill_ms", "step_ms", "generate_ms")
    wb = {e: clfs[(e, args.new)].decode_stats["weight_bytes"] for e in legs}
    layer_bytes = sum(p.numel() for n, p in llm.named_parameters() if "_proj." in n)
    kv_mean = 2 * 2 * rows * args.layers * 4096 * (args.prompt + (steps + 1) / 2.0)
    lm_head = 2 * 32000 * 4096
    line = {"tool": "decode_step_bench", "leg": "int8", "rows": rows, "prompt": args.prompt, "new_tokens": args.new, "layers": args.layers,
            "reps": args.reps, "warmup": args.warmup, "engines": res, "weight_bytes": wb,
            "int8_over_fp16_weight_bytes": wb["int8"] / wb["fp16"],
            "int8_over_fp16_median": {k: med("int8", k) / med("fp16", k) for k in keys},
            "int8_and_fp16_ranges_overlap": {k: overlap("int8", "fp16", k) for k in keys},
            "floor_ms_per_step": {"fp16": (2 * layer_bytes + lm_head + kv_mean) / COPY_RATE * 1e3,
                                  "int8": (layer_bytes + lm_head + kv_mean) / COPY_RATE * 1e3},
            "copy_rate_bytes_per_s": COPY_RATE,
            "int8_rows_with_fp16_tokens": int((tokens["int8"] == tokens["fp16"]).all(dim=1).sum()),
            "shader_clock_mhz_before_after": [clock_before, clock_after], "device": torch.cuda.get_device_name(0)}
    if "act_int8" in res:
        line["leg"] = "act_int8"
        line["act_int8_over_fp16_median"] = {k: med("act_int8", k) / med("fp16", k) for k in keys}
        line["act_int8_over_int8_median"] = {k: med("act_int8", k) / med("int8", k) for k in keys}
        line["act_int8_and_int8_ranges_overlap"] = {k: overlap("act_int8", "int8", k) for k in keys}
        line["act_int8_rows_with_int8_tokens"] = int((tokens["act_int8"] == tokens["int8"]).all(dim=1).sum())
        line["act_stats_last_call"] = clfs[("act_int8", args.new)].last_act_stats()
    if "parent" in res:
        line["parent_lib"] = os.path.basename(args.parent_lib)
        line["fp16_and_parent_ranges_overlap"] = {k: overlap("fp16", "parent", k) for k in keys}
        line["fp16_over_parent_median"] = {k: med("fp16", k) / med("parent", k) for k in keys}
        line["fp16_rows_with_parent_tokens"] = int((tokens["fp16"] == tokens["parent"]).all(dim=1).sum())
    print(json.dumps(line))


def early_stop_leg(args, llm, embs, tok, lm):
    rows, new = args.rows, args.new
    with torch.no_grad():
        llm.lm_head.weight.zero_()
    llm.config.eos_token_id = llm.generation_config.eos_token_id = 0
    llm.config.pad_token_id = llm.generation_config.pad_token_id = 0

    def build(n, min_length, **kw):
        return MiniGPT4Classifier(_Rows(rows), llm, tok, "<ImageHere>", lm, max_new_tokens=n, max_batch=rows, decode="hip", prefill="hip",
                                  generate_kwargs=dict(min_length=min_length), **kw)

    finish = {"off": new, "on_never": new, "on_f1": 1, "on_f3": 3, "parent": new}
    legs = ["off", "on_never", "on_f1", "on_f3"]
    clfs = {(e, new): build(new, finish[e], early_stop=e != "off") for e in legs}
    prefill = build(1, 1)                                                # one select, no step: the same call on every leg of this build
    for e in legs:
        clfs[(e, 1)] = prefill
    if args.parent_lib:
        with _other_library(args.parent_lib):
            clfs.update({("parent", n): build(n, new) for n in (new, 1)})
        legs.append("parent")

    def timed(leg, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = clfs[(leg, n)]._generate_graph(embs)
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    clock_before = _clock()
    res = {e: {"generate_ms": [], "prefill_ms": [], "order": []} for e in legs}
    tokens, live = {}, {}
    with torch.no_grad():
        for rep_i in range(args.warmup + args.reps):                   # interleaved, and rotated: every leg takes every place in turn
            k = rep_i % len(legs)
            for place, e in enumerate(legs[k:] + legs[:k]):
                t, out = timed(e, new)
                if e != "parent":
                    live[e] = clfs[(e, new)].last_live_steps()         # after the timed region: it synchronises
                tp = timed(e, 1)[0]
                print(f"decode_step_bench: repetition {rep_i} {e} generate {t:.1f} ms prefill {tp:.1f} ms", file=sys.stderr, flush=True)
                if rep_i >= args.warmup:
                    res[e]["generate_ms"].append(t)
                    res[e]["prefill_ms"].append(tp)
                    res[e]["order"].append(place)
                    tokens[e] = out
        # the off engine on the two finishing laws, eagerly and untimed: the tokens the on legs must give
        off = clfs[("off", new)]
        for f in (1, 3):
            off.generate_kwargs["min_length"] = f
            tokens[f"off_f{f}"] = off.greedy_tokens(embs)
        off.generate_kwargs["min_length"] = new
    clock_after = _clock()
    steps = new - 1
    for r in res.values():
        r["step_ms"] = [(gm - pm) / steps for gm, pm in zip(r["generate_ms"], r["prefill_ms"])]
        for k in ("generate_ms", "prefill_ms", "step_ms"):
            r[k + "_min_max"] = [min(r[k]), max(r[k])]

    def overlap(a, b, k):
        (a0, a1), (b0, b1) = res[a][k + "_min_max"], res[b][k + "_min_max"]
        return a0 <= b1 and b0 <= a1

    def med(e, k):
        return sorted(res[e][k])[len(res[e][k]) // 2]

    keys = ("prefill_ms", "step_ms", "generate_ms")
    live_step = med("on_never", "step_ms")
    dead = {}
    for f in (1, 3):
        saving = (med("on_never", "generate_ms") - med(f"on_f{f}", "generate_ms")) / (steps - f)
        dead[f"f{f}"] = {"saving_per_skipped_step_ms": saving, "dead_step_ms": live_step - saving,
                         "dead_step_over_live_step": (live_step - saving) / live_step}
    same = lambda a, b: int((tokens[a] == tokens[b]).all(dim=1).sum())  # noqa: E731
    line = {"tool": "decode_step_bench", "leg": "early_stop", "rows": rows, "prompt": args.prompt, "new_tokens": new, "layers": args.layers,
            "reps": args.reps, "warmup": args.warmup, "leg_order": "rotated by one place per repetition", "engines": res,
            "live_steps": live,
            "on_never_over_off_median": {k: med("on_never", k) / med("off", k) for k in keys},
            "on_never_and_off_ranges_overlap": {k: overlap("on_never", "off", k) for k in keys},
            "on_over_off_generate_median": {e: med(e, "generate_ms") / med("off", "generate_ms") for e in ("on_f1", "on_f3")},
            "on_and_off_generate_ranges_overlap": {e: overlap(e, "off", "generate_ms") for e in ("on_f1", "on_f3")},
            "live_step_ms": live_step, "dead_step": dead,
            "rows_with_off_tokens": {"on_never": same("on_never", "off"), "on_f1": same("on_f1", "off_f1"), "on_f3": same("on_f3", "off_f3")},
            "shader_clock_mhz_before_after": [clock_before, clock_after], "device": torch.cuda.get_device_name(0)}
    if "parent" in res:
        line["parent_lib"] = os.path.basename(args.parent_lib)
        line["off_and_parent_ranges_overlap"] = {k: overlap("off", "parent", k) for k in keys}
        line["off_over_parent_median"] = {k: med("off", k) / med("parent", k) for k in keys}
        line["off_rows_with_parent_tokens"] = same("off", "parent")
    print(json.dumps(line))


def stop_leg(args, llm, embs, tok, lm):
    from certifiedgpt_amd.minigpt4 import apply_stop_sequences
    rows, new = args.rows, args.new
    with torch.no_grad():
        llm.lm_head.weight.zero_()
    llm.config.eos_token_id = llm.generation_config.eos_token_id = []
    llm.config.pad_token_id = llm.generation_config.pad_token_id = 0

    def build(n, **kw):
        return MiniGPT4Classifier(_Rows(rows), llm, tok, "<ImageHere>", lm, max_new_tokens=n, max_batch=rows, decode="hip", prefill="hip",
                                  generate_kwargs=dict(min_length=0), **kw)

    never = [[32000 + 8 * q + j for j in range(8)] for q in range(8)]
    how = {"off": {}, "never": dict(stop_words_ids=never), "on_k1": dict(early_stop=True, stop_words_ids=[[0]]),
           "on_k3": dict(early_stop=True, stop_words_ids=[[0] * 3])}
    legs = list(how)
    clfs = {(e, new): build(new, **how[e]) for e in legs}
    prefill = build(1)                                                   # one select, no step: the same call on every leg of this build
    for e in legs:
        clfs[(e, 1)] = prefill
    if args.parent_lib:
        with _other_library(args.parent_lib):
            clfs.update({("parent", n): build(n) for n in (new, 1)})
        legs.append("parent")

    def timed(leg, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = clfs[(leg, n)]._generate_graph(embs)
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    clock_before = _clock()
    res = {e: {"generate_ms": [], "prefill_ms": [], "order": []} for e in legs}
    tokens, live = {}, {}
    with torch.no_grad():
        for rep_i in range(args.warmup + args.reps):                   # interleaved, and rotated: every leg takes every place in turn
            k = rep_i % len(legs)
            for place, e in enumerate(legs[k:] + legs[:k]):
                t, out = timed(e, new)
                if e != "parent":
                    live[e] = clfs[(e, new)].last_live_steps()         # after the timed region: it synchronises
                tp = timed(e, 1)[0]
                print(f"decode_step_bench: repetition {rep_i} {e} generate {t:.1f} ms prefill {tp:.1f} ms", file=sys.stderr, flush=True)
                if rep_i >= args.warmup:
                    res[e]["generate_ms"].append(t)
                    res[e]["prefill_ms"].append(tp)
                    res[e]["order"].append(place)
                    tokens[e] = out
    clock_after = _clock()
    steps = new - 1
    for r in res.values():
        r["step_ms"] = [(gm - pm) / steps for gm, pm in zip(r["generate_ms"], r["prefill_ms"])]
        for k in ("generate_ms", "prefill_ms", "step_ms"):
            r[k + "_min_max"] = [min(r[k]), max(r[k])]

    def overlap(a, b, k):
        (a0, a1), (b0, b1) = res[a][k + "_min_max"], res[b][k + "_min_max"]
        return a0 <= b1 and b0 <= a1

    def med(e, k):
        return sorted(res[e][k])[len(res[e][k]) // 2]

    keys = ("prefill_ms", "step_ms", "generate_ms")
    rule = lambda e: apply_stop_sequences(tokens["off"], [], how[e]["stop_words_ids"], 0)  # noqa: E731
    line = {"tool": "decode_step_bench", "leg": "stop", "rows": rows, "prompt": args.prompt, "new_tokens": new, "layers": args.layers,
            "reps": args.reps, "warmup": args.warmup, "leg_order": "rotated by one place per repetition", "engines": res,
            "live_steps": live,
            "never_over_off_median": {k: med("never", k) / med("off", k) for k in keys},
            "never_and_off_ranges_overlap": {k: overlap("never", "off", k) for k in keys},
            "on_over_off_generate_median": {e: med(e, "generate_ms") / med("off", "generate_ms") for e in ("on_k1", "on_k3")},
            "rows_with_the_rule_on_off_tokens": {e: int((tokens[e] == rule(e)).all(dim=1).sum()) for e in ("never", "on_k1", "on_k3")},
            "shader_clock_mhz_before_after": [clock_before, clock_after], "device": torch.cuda.get_device_name(0)}
    if "parent" in res:
        line["parent_lib"] = os.path.basename(args.parent_lib)
        line["off_and_parent_ranges_overlap"] = {k: overlap("off", "parent", k) for k in keys}
        line["never_and_parent_ranges_overlap"] = {k: overlap("never", "parent", k) for k in keys}
        line["off_over_parent_median"] = {k: med("off", k) / med("parent", k) for k in keys}
        line["never_over_parent_median"] = {k: med("never", k) / med("parent", k) for k in keys}
        line["off_rows_with_parent_tokens"] = int((tokens["off"] == tokens["parent"]).all(dim=1).sum())
    print(json.dumps(line))


def sample_leg(args, llm, embs, tok, lm):
    rows, new = args.rows, args.new
    llm.config.eos_token_id = llm.generation_config.eos_token_id = []
    llm.config.pad_token_id = llm.generation_config.pad_token_id = 0
    chat = dict(do_sample=True, top_p=0.9, repetition_penalty=1.05, temperature=1.0, min_length=0)

    def build(n, **kw):
        return MiniGPT4Classifier(_Rows(rows), llm, tok, "<ImageHere>", lm, max_new_tokens=n, max_batch=rows, decode="hip", prefill="hip",
                                  **kw)

    how = {"greedy": dict(generate_kwargs=dict(min_length=0)), "sampled": dict(sample="hip", generate_kwargs=chat)}
    legs = list(how)
    clfs = {(e, n): build(n, **how[e]) for e in legs for n in (new, 1)}
    if args.parent_lib:
        with _other_library(args.parent_lib):
            clfs.update({("parent", n): build(n, **how["greedy"]) for n in (new, 1)})
        legs.append("parent")

    def timed(leg, n):
        clf = clfs[(leg, n)]
        if leg == "sampled":                                           # the ids and the seed, written before the timed region
            clf._write_draws(rows, (0, 0), embs.device)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = clf._generate_graph(embs)
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    clock_before = _clock()
    res = {e: {"generate_ms": [], "prefill_ms": [], "order": []} for e in legs}
    tokens = {}
    with torch.no_grad():
        for rep_i in range(args.warmup + args.reps):                   # interleaved, and rotated: every leg takes every place in turn
            k = rep_i % len(legs)
            for place, e in enumerate(legs[k:] + legs[:k]):
                t, out = timed(e, new)
                tp = timed(e, 1)[0]
                print(f"decode_step_bench: repetition {rep_i} {e} generate {t:.1f} ms prefill+select {tp:.1f} ms", file=sys.stderr, flush=True)
                if rep_i >= args.warmup:
                    res[e]["generate_ms"].append(t)
                    res[e]["prefill_ms"].append(tp)
                    res[e]["order"].append(place)
                    assert e not in tokens or torch.equal(tokens[e], out), f"{e}: a replay gave other tokens"
                    tokens[e] = out
    clock_after = _clock()
    steps = new - 1
    for r in res.values():
        r["step_ms"] = [(gm - pm) / steps for gm, pm in zip(r["generate_ms"], r["prefill_ms"])]
        for k in ("generate_ms", "prefill_ms", "step_ms"):
            r[k + "_min_max"] = [min(r[k]), max(r[k])]

    def overlap(a, b, k):
        (a0, a1), (b0, b1) = res[a][k + "_min_max"], res[b][k + "_min_max"]
        return a0 <= b1 and b0 <= a1

    def med(e, k):
        return sorted(res[e][k])[len(res[e][k]) // 2]

    keys = ("prefill_ms", "step_ms", "generate_ms")
    line = {"tool": "decode_step_bench", "leg": "sample", "rows": rows, "prompt": args.prompt, "new_tokens": new, "layers": args.layers,
            "reps": args.reps, "warmup": args.warmup, "leg_order": "rotated by one place per repetition", "engines": res,
            "settings": {k: v for k, v in chat.items() if k != "min_length"}, "top_k": 50,
            "sampled_over_greedy_median": {k: med("sampled", k) / med("greedy", k) for k in keys},
            "sampler_ms_per_select": (med("sampled", "generate_ms") - med("greedy", "generate_ms")) / new,
            "sampler_ms_per_step": med("sampled", "step_ms") - med("greedy", "step_ms"),
            "distinct_sampled_tokens": int(tokens["sampled"].unique().numel()),
            "rows_where_sampled_differs_from_greedy": int((tokens["sampled"] != tokens["greedy"]).any(dim=1).sum()),
            "shader_clock_mhz_before_after": [clock_before, clock_after], "device": torch.cuda.get_device_name(0)}
    if "parent" in res:
        line["parent_lib"] = os.path.basename(args.parent_lib)
        line["greedy_and_parent_ranges_overlap"] = {k: overlap("greedy", "parent", k) for k in keys}
        line["greedy_over_parent_median"] = {k: med("greedy", k) / med("parent", k) for k in keys}
        line["greedy_rows_with_parent_tokens"] = int((tokens["greedy"] == tokens["parent"]).all(dim=1).sum())
    print(json.dumps(line))


def shared_prefix_leg(args, llm, tok, lm):
    rows, new, dev = args.rows, args.new, "cuda:0"
    shapes = [(args.prefix_len, args.prompt), (args.prefix_len2, args.prompt2)]
    assert all(1 <= P < L for P, L in shapes)

    def build(n, **kw):
        return MiniGPT4Classifier(_Rows(rows), llm, tok, "<ImageHere>", lm, max_new_tokens=n, max_batch=rows, decode="hip", prefill="hip", **kw)

    clfs = {("plain", n): build(n) for n in (new, 1)}
    clfs.update({("prefix", n): build(n, shared_prefix=True) for n in (new, 1)})
    legs, inputs, which = [], {}, {}
    g = torch.Generator(device="cpu").manual_seed(1)
    embed = llm.get_input_embeddings()
    with torch.no_grad():
        for P, L in shapes:
            ids = tuple(torch.randint(3, 32000, (P,), generator=g).tolist())
            suffix = embed(torch.randint(3, 32000, (rows, L - P), generator=g).to(dev)).contiguous()
            whole = torch.cat([embed(torch.tensor([ids], device=dev)).expand(rows, -1, -1), suffix], dim=1).contiguous()
            legs += [f"plain_{L}", f"prefix_{L}"]
            inputs[f"plain_{L}"], which[f"plain_{L}"] = (lambda clf, whole=whole: (whole,)), "plain"
            inputs[f"prefix_{L}"] = lambda clf, suffix=suffix, ids=ids, P=P: (suffix, None, clf._prefix_entry(ids, dev))
            which[f"prefix_{L}"] = "prefix"
    if args.parent_lib:
        with _other_library(args.parent_lib):
            clfs.update({("parent", n): build(n) for n in (new, 1)})
        legs.append("parent")
        inputs["parent"], which["parent"] = inputs[f"plain_{shapes[0][1]}"], "parent"

    def timed(leg, n):
        clf = clfs[(which[leg], n)]
        call = inputs[leg](clf)                                        # a prefix miss (the one-row prefill) happens here, untimed
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = clf._generate_graph(*call)
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    def eager_ms(fn, reps=5):
        out = []
        for _ in range(2 + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return out[2:]

    clock_before = _clock()
    res = {e: {"generate_ms": [], "prefill_ms": [], "order": []} for e in legs}
    tokens = {}
    with torch.no_grad():
        for rep_i in range(args.warmup + args.reps):                   # interleaved, and rotated: every leg takes every place in turn
            k = rep_i % len(legs)
            for place, e in enumerate(legs[k:] + legs[:k]):
                t, out = timed(e, new)
                tp = timed(e, 1)[0]
                print(f"decode_step_bench: repetition {rep_i} {e} generate {t:.1f} ms prefill {tp:.1f} ms", file=sys.stderr, flush=True)
                if rep_i >= args.warmup:
                    res[e]["generate_ms"].append(t)
                    res[e]["prefill_ms"].append(tp)
                    res[e]["order"].append(place)
                    tokens[e] = out
        # the two costs the flag adds, alone: the broadcast on caches of the call's shape, and the one-row prefill of a miss
        clf = clfs[("prefix", new)]
        alone = {}
        for P, L in shapes:
            ids = next(i for i in clf._prefixes if len(i) == P)
            pk, pv = clf._prefixes[ids].k, clf._prefixes[ids].v
            kb, vb = clf._kv_buffers(pk[0], rows, L + new)
            embs1 = embed(torch.tensor([ids], device=dev)).contiguous()
            alone[str(L)] = {"broadcast_ms": eager_ms(lambda: clf._hip.kv_broadcast(pk, pv, P, kb, vb)),
                             "broadcast_bytes_written": 2 * 2 * rows * len(pk) * clf._hip.kv_heads * 128 * P,
                             "prefix_miss_ms": eager_ms(lambda: clf._hip.prefill(embs1, pk, pv))}
            del kb, vb
    clock_after = _clock()
    steps = new - 1
    for r in res.values():
        r["step_ms"] = [(gm - pm) / steps for gm, pm in zip(r["generate_ms"], r["prefill_ms"])]
        for k in ("generate_ms", "prefill_ms", "step_ms"):
            r[k + "_min_max"] = [min(r[k]), max(r[k])]

    def overlap(a, b, k):
        (a0, a1), (b0, b1) = res[a][k + "_min_max"], res[b][k + "_min_max"]
        return a0 <= b1 and b0 <= a1

    def med(e, k):
        return sorted(res[e][k])[len(res[e][k]) // 2]

    keys = ("prefill_ms", "step_ms", "generate_ms")
    line = {"tool": "decode_step_bench", "leg": "shared_prefix", "rows": rows, "shapes_prefix_prompt": shapes, "new_tokens": new,
            "layers": args.layers, "reps": args.reps, "warmup": args.warmup, "leg_order": "rotated by one place per repetition",
            "engines": res, "alone": alone, "shader_clock_mhz_before_after": [clock_before, clock_after],
            "device": torch.cuda.get_device_name(0)}
    for P, L in shapes:
        a, b = f"prefix_{L}", f"plain_{L}"
        bc = sorted(alone[str(L)]["broadcast_ms"])[len(alone[str(L)]["broadcast_ms"]) // 2]
        line[f"shape_{P}_{L}"] = {
            "prefix_over_plain_median": {k: med(a, k) / med(b, k) for k in keys},
            "slowest_prefix_beats_fastest_plain": {k: max(res[a][k]) < min(res[b][k]) for k in ("prefill_ms", "generate_ms")},
            "prefix_share_of_positions": P / L,
            "broadcast_ms_median": bc, "broadcast_share_of_flagged_prefill": bc / med(a, "prefill_ms"),
            "rows_with_plain_tokens": int((tokens[a] == tokens[b]).all(dim=1).sum())}
    stats = clfs[("prefix", new)].decode_stats
    line["prefix_prefills_hits_captures_replays"] = [stats["hip_prefix_prefills"], stats["hip_prefix_hits"], stats["graph_captures"],
                                                     stats["graph_replays"]]
    if "parent" in res:
        first = f"plain_{shapes[0][1]}"
        line["parent_lib"] = os.path.basename(args.parent_lib)
        line["plain_and_parent_ranges_overlap"] = {k: overlap(first, "parent", k) for k in keys}
        line["plain_over_parent_median"] = {k: med(first, k) / med("parent", k) for k in keys}
        line["plain_rows_with_parent_tokens"] = int((tokens[first] == tokens["parent"]).all(dim=1).sum())
    print(json.dumps(line))


def gqa_leg(args, dev):
    rows, new = args.rows, args.new
    lm = AnswerLabelMap(4, ())
    llm = _decoder(args.layers, dev, kv_heads=8, mlp=14336, vocab=args.gqa_vocab, theta=500000.0)
    g = torch.Generator(device="cpu").manual_seed(1)
    embs = {"gqa": llm.get_input_embeddings()(torch.randint(3, args.gqa_vocab, (rows, args.prompt), generator=g).to(dev))}
    embs["graph"] = embs["gqa"]
    tok = WordHashTokenizer(args.gqa_vocab)

    def build(model, t, n, **kw):
        return MiniGPT4Classifier(_Rows(rows), model, t, "<ImageHere>", lm, max_new_tokens=n, max_batch=rows, **kw)

    legs = ["gqa", "graph"]
    clfs = {("gqa", n): build(llm, tok, n, decode="hip", prefill="hip", grouped_kv=True) for n in (new, 1)}
    clfs.update({("graph", n): build(llm, tok, n, decode="graph") for n in (new, 1)})
    if args.parent_lib:
        mha = _decoder(args.layers, dev)
        g = torch.Generator(device="cpu").manual_seed(1)
        embs["plain"] = embs["parent"] = mha.get_input_embeddings()(torch.randint(3, 32000, (rows, args.prompt), generator=g).to(dev))
        tok7 = WordHashTokenizer(32000)
        clfs.update({("plain", n): build(mha, tok7, n, decode="hip", prefill="hip") for n in (new, 1)})
        with _other_library(args.parent_lib):
            clfs.update({("parent", n): build(mha, tok7, n, decode="hip", prefill="hip") for n in (new, 1)})
        legs += ["plain", "parent"]

    def timed(leg, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = clfs[(leg, n)]._generate_graph(embs[leg])
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    clock_before = _clock()
    res = {e: {"generate_ms": [], "prefill_ms": []} for e in legs}
    tokens = {}
    with torch.no_grad():
        for rep_i in range(args.warmup + args.reps):                   # interleaved, and the order rotated by one place per repetition
            k = rep_i % len(legs)
            for e in legs[k:] + legs[:k]:
                t, out = timed(e, new)
                tp = timed(e, 1)[0]
                print(f"decode_step_bench: repetition {rep_i} {e} generate {t:.1f} ms prefill {tp:.1f} ms", file=sys.stderr, flush=True)
                if rep_i >= args.warmup:
                    res[e]["generate_ms"].append(t)
                    res[e]["prefill_ms"].append(tp)
                    tokens[e] = out
    clock_after = _clock()
    steps = new - 1
    for r in res.values():
        r["step_ms"] = [(gm - pm) / steps for gm, pm in zip(r["generate_ms"], r["prefill_ms"])]
        for k in ("generate_ms", "prefill_ms", "step_ms"):
            r[k + "_min_max"] = [min(r[k]), max(r[k])]

    def overlap(a, b, k):
        (a0, a1), (b0, b1) = res[a][k + "_min_max"], res[b][k + "_min_max"]
        return a0 <= b1 and b0 <= a1

    def med(e, k):
        return sorted(res[e][k])[len(res[e][k]) // 2]

    keys = ("prefill_ms", "step_ms", "generate_ms")
    hip = clfs[("gqa", new)]._hip
    pool = 2 * 2 * rows * args.layers * hip.kv_heads * 128 * (args.prompt + new)
    layer_bytes = 2 * sum(p.numel() for n, p in llm.named_parameters() if "_proj." in n)
    kv_mean = 2 * 2 * rows * args.layers * hip.kv_heads * 128 * (args.prompt + (steps + 1) / 2.0)
    line = {"tool": "decode_step_bench", "leg": "gqa", "rows": rows, "prompt": args.prompt, "new_tokens": new, "layers": args.layers,
            "heads_kv_heads": [hip.heads, hip.kv_heads], "vocab": args.gqa_vocab, "reps": args.reps, "warmup": args.warmup, "engines": res,
            "kv_pool_bytes": pool, "kv_pool_bytes_at_32_kv_heads": pool * hip.heads // hip.kv_heads, "weight_bytes": hip.weight_bytes,
            "gqa_over_graph_median": {k: med("gqa", k) / med("graph", k) for k in keys},
            "gqa_and_graph_ranges_overlap": {k: overlap("gqa", "graph", k) for k in keys},
            "gqa_rows_with_graph_tokens": int((tokens["gqa"] == tokens["graph"]).all(dim=1).sum()),
            "floor_ms_per_step": (layer_bytes + 2 * args.gqa_vocab * 4096 + kv_mean) / COPY_RATE * 1e3, "copy_rate_bytes_per_s": COPY_RATE,
            "shader_clock_mhz_before_after": [clock_before, clock_after], "device": torch.cuda.get_device_name(0)}
    if "parent" in res:
        line["parent_lib"] = os.path.basename(args.parent_lib)
        line["plain_and_parent_ranges_overlap"] = {k: overlap("plain", "parent", k) for k in keys}
        line["plain_over_parent_median"] = {k: med("plain", k) / med("parent", k) for k in keys}
        line["plain_rows_with_parent_tokens"] = int((tokens["plain"] == tokens["parent"]).all(dim=1).sum())
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--prompt", type=int, default=44)
    ap.add_argument("--new", type=int, default=20)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--engines", default="graph,hip,hip_native")
    ap.add_argument("--ragged", action="store_true", help="the left-padding leg (see the module docstring)")
    ap.add_argument("--bucket-len", type=int, default=48)
    ap.add_argument("--ragged-min", type=int, default=38)
    ap.add_argument("--int8", action="store_true", help="the weight-format leg (see the module docstring)")
    ap.add_argument("--act-int8", action="store_true",
                    help='with the weight-format leg: a third engine, weights="int8" + activations="int8" (DESIGN.md 4.4.7)')
    ap.add_argument("--early-stop", action="store_true", help="the early-stop leg (see the module docstring)")
    ap.add_argument("--stop", action="store_true", help="the stop-sequence leg (see the module docstring)")
    ap.add_argument("--gqa", action="store_true", help="the grouped-query leg (see the module docstring)")
    ap.add_argument("--sample", action="store_true", help="the sampled-decode leg (see the module docstring)")
    ap.add_argument("--shared-prefix", action="store_true", help="the shared-prefix leg (see the module docstring)")
    ap.add_argument("--prefix-len", type=int, default=7, help="P of the first shape (with --prompt)")
    ap.add_argument("--prefix-len2", type=int, default=40, help="P of the second shape (with --prompt2)")
    ap.add_argument("--prompt2", type=int, default=80)
    ap.add_argument("--gqa-vocab", type=int, default=128256)
    ap.add_argument("--parent-lib", default=None,
                    help="another build of libcgpt.so for the plain-path A/B of --ragged / --int8 / --early-stop / --stop / --gqa / --sample / --shared-prefix")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures device time: it needs the GPU"
    assert 1 <= args.rows <= 256 and args.new >= 2 and args.prompt >= 1
    dev = "cuda:0"
    if args.gqa:
        return gqa_leg(args, dev)
    engines = args.engines.split(",")
    llm = _decoder(args.layers, dev)
    g = torch.Generator(device="cpu").manual_seed(1)
    embs = llm.get_input_embeddings()(torch.randint(3, 32000, (args.rows, args.prompt), generator=g).to(dev))
    tok, lm = WordHashTokenizer(32000), AnswerLabelMap(4, ())
    if args.ragged:
        return ragged_leg(args, llm, embs, tok, lm)
    if args.int8 or args.act_int8:
        return int8_leg(args, llm, embs, tok, lm)
    if args.early_stop:
        return early_stop_leg(args, llm, embs, tok, lm)
    if args.stop:
        return stop_leg(args, llm, embs, tok, lm)
    if args.sample:
        return sample_leg(args, llm, embs, tok, lm)
    if args.shared_prefix:
        return shared_prefix_leg(args, llm, tok, lm)
    how = {"graph": dict(decode="graph"), "hip": dict(decode="hip", prefill="model"), "hip_native": dict(decode="hip", prefill="hip")}
    clfs = {(e, n): MiniGPT4Classifier(_Rows(args.rows), llm, tok, "<ImageHere>", lm, max_new_tokens=n, max_batch=args.rows,
                                       prefill_linear="cgpt", **how[e]) for e in engines for n in (args.new, 1)}

    def timed(clf):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = clf._generate_graph(embs)
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    clock_before = _clock()
    with torch.no_grad():
        for _ in range(args.warmup):                                   # capture + warm replays of every graph
            for clf in clfs.values():
                timed(clf)
        res = {e: {"generate_ms": [], "prefill_ms": []} for e in engines}
        tokens = {}
        for _ in range(args.reps):                                     # interleaved: engine by engine inside every repetition
            for e in engines:
                t, out = timed(clfs[(e, args.new)])
                res[e]["generate_ms"].append(t)
                tokens[e] = out
                res[e]["prefill_ms"].append(timed(clfs[(e, 1)])[0])
    clock_after = _clock()
    steps = args.new - 1
    for e in engines:
        r = res[e]
        r["steps_ms"] = [gm - pm for gm, pm in zip(r["generate_ms"], r["prefill_ms"])]
        r["step_ms"] = [s / steps for s in r["steps_ms"]]
        r["step_ms_min_max"] = [min(r["step_ms"]), max(r["step_ms"])]
        r["generate_ms_min_max"] = [min(r["generate_ms"]), max(r["generate_ms"])]
    weight_bytes = 2 * sum(p.numel() for n, p in llm.named_parameters() if "embed_tokens" not in n)
    kv_mean = 2 * 2 * args.rows * args.layers * 4096 * (args.prompt + (steps + 1) / 2.0)
    line = {"tool": "decode_step_bench", "rows": args.rows, "prompt": args.prompt, "new_tokens": args.new, "layers": args.layers,
            "reps": args.reps, "warmup": args.warmup, "engines": res,
            "floor_ms_per_step": (weight_bytes + kv_mean) / COPY_RATE * 1e3, "weight_bytes": weight_bytes, "kv_bytes_mean_step": kv_mean,
            "copy_rate_bytes_per_s": COPY_RATE, "shader_clock_mhz_before_after": [clock_before, clock_after],
            "device": torch.cuda.get_device_name(0)}
    if "graph" in res and "hip" in res:
        line["slowest_hip_beats_fastest_graph"] = {
            "step": max(res["hip"]["step_ms"]) < min(res["graph"]["step_ms"]),
            "generate": max(res["hip"]["generate_ms"]) < min(res["graph"]["generate_ms"])}
        line["rows_with_identical_tokens"] = int((tokens["hip"] == tokens["graph"]).all(dim=1).sum())
    if "hip" in res and "hip_native" in res:                           # the native prefill against the model's own, same steps after it
        line["slowest_native_prefill_beats_fastest_model_prefill"] = {
            "prefill": max(res["hip_native"]["prefill_ms"]) < min(res["hip"]["prefill_ms"]),
            "generate": max(res["hip_native"]["generate_ms"]) < min(res["hip"]["generate_ms"])}
        line["rows_with_identical_tokens_native_vs_model_prefill"] = int((tokens["hip_native"] == tokens["hip"]).all(dim=1).sum())
    line["native_prefills_enqueued"] = sum(c.decode_stats["hip_prefills"] for c in clfs.values())
    print(json.dumps(line))


if __name__ == "__main__":
    main()
