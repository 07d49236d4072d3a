"""What one classifier batch costs under the three ways MiniGPT4Classifier turns noisy rows into votes, on a
Vicuna-7B-shaped random-init decoder (no checkpoint is needed; nothing is downloaded), native prefill, fp16:

    generate        classify="generate": 20 greedy tokens, the tokens read back, decoded and mapped on the host, cgpt_vote
    generate_es     the same with early_stop=True
    constrained     classify="constrained", constrain="hip": `depth` tokens over a trie of --cands synthetic candidates of 1..4 tokens
                    (words of the hash tokenizer, no end symbol), labels voted on the device (cgpt_vote_labels), nothing read back
    constrained_es  the same with early_stop=True
    multi_select    classify="multi_select", score="hip", at its limit of 64 candidates (the first 64 two-token ones: 64 tail rows), cgpt_vote
    parent          `generate` on another build of the library (--parent-lib PATH, e.g. the parent commit's libcgpt.so), loaded beside
                    this one: the default path must be unchanged (ranges that do not overlap are a regression to explain);
                    --parent-after LEG moves it in the rotation (a leg's time depends a little on which leg ran before it)

A batch is timed from the image embeds (the encoder is not part of it) to the histogram, host work included, with the wall clock
around a device sync (`batch_ms`); the captured graph alone is also timed with HIP events (`graph_ms`, generate legs and constrained
legs).  Legs are interleaved and rotated by one place per repetition; min-max over --reps repetitions after --warmup.

    select          the trie select alone (cgpt_llm_trie_select_logits, every row at the root: the trie's largest fan-out) against the
                    arg-max select of the same library (cgpt_llm_greedy with num_new = 1: one select, no step), each launch between
                    two HIP events, the mean of --select-launches launches per repetition

Prints ONE JSON line; --out PATH also writes it to a file.
"""
import argparse
import json
import os
import random
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap  # noqa: E402
from certifiedgpt_amd.classifier import vote, vote_labels  # noqa: E402
from certifiedgpt_amd.minigpt4 import MiniGPT4Classifier, WordHashTokenizer  # noqa: E402
from decode_step_bench import _Rows, _clock, _decoder, _other_library  # noqa: E402

PROMPT = "<s>[INST] <Img><ImageHere></Img> [vqa] what is shown in the picture [/INST]"
END = ""


def synthetic_candidates(tok, count, seed=0):
    """`count` distinct texts of 1..4 words (= tokens: no end symbol) from a pool of 200 words with distinct token ids.  The first
    word says how long a candidate is -- pool words 0..99 are the one-word candidates, 100..129 open the two-word ones, 130..164 the
    three-word ones, 165..199 the four-word ones -- so no candidate is a prefix of another and the root has 200 edges."""
    rng = random.Random(seed)
    pool, ids = [], set()
    i = 0
    while len(pool) < 200:
        w = f"q{i}x"
        i += 1
        if tok._word_id(w) not in ids:
            ids.add(tok._word_id(w))
            pool.append(w)
    out = list(pool[:100])
    seen = set(out)
    heads = {2: pool[100:130], 3: pool[130:165], 4: pool[165:200]}
    while len(out) < count:
        n = 2 if len(out) < count // 3 else 3 if len(out) < 2 * count // 3 else 4
        text = " ".join([rng.choice(heads[n])] + [rng.choice(pool) for _ in range(n - 1)])
        if text not in seen:
            seen.add(text)
            out.append(text)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--new", type=int, default=20)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--cands", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--select-launches", type=int, default=50)
    ap.add_argument("--parent-lib", default=None, help="another build of libcgpt.so for the `parent` leg")
    ap.add_argument("--parent-after", default=None, help="the leg the `parent` leg follows in the rotation (default: the last one)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = args.rows
    llm = _decoder(args.layers, dev)
    tok = WordHashTokenizer(32000)
    cands = synthetic_candidates(tok, args.cands)
    g = torch.Generator(device="cpu").manual_seed(1)
    emb = (torch.randn(rows, 32, 4096, generator=g) * 0.02).to(dev).to(torch.float16)

    def build(**kw):
        kw.setdefault("label_map", AnswerLabelMap(len(cands) + 1, cands, frozen=True))     # free text outside them votes "other"
        lm = kw.pop("label_map")
        return MiniGPT4Classifier(_Rows(rows), llm, tok, PROMPT, lm, max_new_tokens=args.new, max_batch=rows, decode="hip", prefill="hip",
                                  end_sym=END, **kw)

    clfs = {"generate": build(), "generate_es": build(early_stop=True),
            "constrained": build(classify="constrained", constrain="hip", candidates=cands),
            "constrained_es": build(classify="constrained", constrain="hip", candidates=cands, early_stop=True),
            "multi_select": build(classify="multi_select", score="hip", candidates=cands[100:164], label_map=AnswerLabelMap(65, ()))}
    legs = list(clfs)
    if args.parent_lib:
        with _other_library(args.parent_lib):
            clfs["parent"] = build()
        legs.insert(legs.index(args.parent_after) + 1 if args.parent_after else len(legs), "parent")
    counts = {e: torch.zeros(c.num_classes, dtype=torch.int64, device=dev) for e, c in clfs.items()}

    def batch(e):
        """One classifier batch, embeds -> histogram, host work included."""
        clf = clfs[e]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if clf.classify == "constrained":
            labels, _ = clf.constrained_from_embeds(emb, PROMPT)
            vote_labels(labels, counts[e])
        else:
            logits, _ = clf._classify_embeds(emb, dev)
            vote(logits, counts[e])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def graph(e):
        clf = clfs[e]
        embs, _, starts, prefix, _, _ = clf._prompt_inputs(emb, PROMPT)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if clf.classify == "constrained":
            clf._generate_graph(embs, starts, prefix, constrained=True)
        else:
            clf._generate_graph(embs, starts)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    clock_before = _clock()
    res = {e: {"batch_ms": [], "graph_ms": [], "order": []} for e in legs}
    with torch.no_grad():
        for rep_i in range(args.warmup + args.reps):
            k = rep_i % len(legs)
            for place, e in enumerate(legs[k:] + legs[:k]):
                t = batch(e)
                tg = graph(e) if clfs[e].classify != "multi_select" else None
                print(f"constrained_bench: repetition {rep_i} {e} batch {t:.1f} ms graph {tg if tg is None else round(tg, 1)} ms",
                      file=sys.stderr, flush=True)
                if rep_i >= args.warmup:
                    res[e]["batch_ms"].append(t)
                    res[e]["order"].append(place)
                    if tg is not None:
                        res[e]["graph_ms"].append(tg)
    live = {e: clfs[e].last_live_steps() for e in legs if clfs[e].classify != "multi_select"}

    # the selects alone
    trie = clfs["constrained"].trie
    begin = trie.child_begin.tolist()
    fan = begin[1] - begin[0]
    hip = clfs["constrained"]._hip
    tdev = trie.to(dev)
    logits = torch.randn(rows, 32000, generator=g).to(dev)
    node = torch.zeros(rows, dtype=torch.int32, device=dev)
    unf = torch.ones(rows, dtype=torch.int32, device=dev)
    toks = torch.zeros(rows, dtype=torch.int64, device=dev)
    labs = torch.zeros(rows, dtype=torch.int32, device=dev)
    kb, vb = clfs["constrained"]._kv_buffers(emb, rows, 1)
    import ctypes as C
    from certifiedgpt_amd import _lib
    L = _lib.lib()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def one_select(which):
        """Mean HIP-event time of one launch; the trie rows are put back on the root before every launch, outside the timed span."""
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        pairs = []
        for _ in range(args.select_launches):
            if which == "trie":
                node.zero_()
                unf.fill_(1)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if which == "trie":
                _lib.check(L.cgpt_llm_trie_select_logits(P(logits), 32000, rows, 32000, *[P(t) for t in tdev.tables()], trie.nodes, 0,
                                                         P(node), P(unf), P(toks), P(labs), st))
            else:
                hip.greedy(logits, 1, 1, 0, [], 0, kb, vb)
            b.record()
            pairs.append((a, b))
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in pairs) / len(pairs)

    sel = {"trie": [], "argmax": []}
    for rep_i in range(args.warmup + args.reps):
        for which in (("trie", "argmax") if rep_i % 2 == 0 else ("argmax", "trie")):
            t = one_select(which)
            if rep_i >= args.warmup:
                sel[which].append(t)
    clock_after = _clock()

    def mm(v):
        return [min(v), max(v)] if v else None

    def med(v):
        return sorted(v)[len(v) // 2]

    for r in res.values():
        r["batch_ms_min_max"], r["graph_ms_min_max"] = mm(r["batch_ms"]), mm(r["graph_ms"])
    line = {"tool": "constrained_bench", "rows": rows, "new_tokens": args.new, "layers": args.layers, "candidates": len(cands),
            "trie": {"nodes": trie.nodes, "depth": trie.depth, "root_fan_out": fan}, "reps": args.reps, "warmup": args.warmup,
            "leg_order": "rotated by one place per repetition", "leg_cycle": legs, "legs": res, "live_steps_of_the_last_batch": live,
            "constrained_over_generate_median": {k: med(res["constrained"][k]) / med(res["generate"][k]) for k in ("batch_ms", "graph_ms")},
            "constrained_votes_other": int(counts["constrained"][-1]), "generate_votes_other": int(counts["generate"][-1]),
            "votes_per_leg": {e: int(c.sum()) for e, c in counts.items()},
            "select_us": {k: [1e3 * x for x in mm(v)] for k, v in sel.items()}, "select_launches": args.select_launches,
            "note": "select_us: one eager launch between two HIP events, so the figure includes what the events see of the launch itself",
            "shader_clock_mhz_before_after": [clock_before, clock_after], "device": torch.cuda.get_device_name(0)}
    if "parent" in res:
        def overlap(k):
            (a0, a1), (b0, b1) = res["generate"][k + "_min_max"], res["parent"][k + "_min_max"]
            return a0 <= b1 and b0 <= a1
        line["parent_lib"] = os.path.basename(args.parent_lib)
        line["generate_and_parent_ranges_overlap"] = {k: overlap(k) for k in ("batch_ms", "graph_ms")}
        line["generate_over_parent_median"] = {k: med(res["generate"][k]) / med(res["parent"][k]) for k in ("batch_ms", "graph_ms")}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
