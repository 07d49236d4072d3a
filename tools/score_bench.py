"""Device time of `multi_select` answer scoring against greedy generation, legs interleaved in one process.

Vicuna-7B-shaped random-init decoder (no checkpoint exists here; nothing is downloaded), 200 rows, a prompt of 44 positions (bos + 43
image positions), candidates of 3 tokens.  Per repetition, by HIP events around each call:
    score_hip_C   (a) score="hip": ONE native prefill + the native scoring pass over C candidates (C = 2, 4, 8)
    score_hf_C    (b) score="hf": the model's own forward over prompt + answer once per candidate, as the reference does
    generate_hip  (c) decode="hip", prefill="hip": native prefill + 20 greedy tokens, one graph replay (the existing figure)
    prefill_hip       the same with 1 new token: the prefill both (a) and (c) contain
Prints ONE JSON line.  The expectation to confirm or refute: (a) grows by the tail rows only -- rows x sum(T_c - 1) token rows against
rows x 44 prefill rows -- while (b) grows by C whole prefills."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap  # noqa: E402
from certifiedgpt_amd.minigpt4 import MiniGPT4Classifier, WordHashTokenizer  # noqa: E402
from tools.decode_step_bench import _Rows, _clock, _decoder  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--prompt", type=int, default=44)
    ap.add_argument("--new", type=int, default=20)
    ap.add_argument("--answer-tokens", type=int, default=3)
    ap.add_argument("--cands", default="2,4,8")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-hf", action="store_true", help="leave out the score_hf legs (a profiling run of the native pass)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures device time: it needs the GPU"
    assert 1 <= args.rows <= 256 and args.prompt >= 2 and args.answer_tokens >= 1
    dev = "cuda:0"
    counts = [int(c) for c in args.cands.split(",")]
    llm = _decoder(args.layers, dev)
    tok, lm = WordHashTokenizer(32000), AnswerLabelMap(4, ())
    g = torch.Generator(device="cpu").manual_seed(1)
    # "<ImageHere>" alone: the scored prompt is bos + the image positions, the generated one the same number of positions
    img = llm.get_input_embeddings()(torch.randint(3, 32000, (args.rows, args.prompt - 1), generator=g).to(dev))
    embs = llm.get_input_embeddings()(torch.randint(3, 32000, (args.rows, args.prompt), generator=g).to(dev))
    cands = [" ".join(f"answer{c}word{j}" for j in range(args.answer_tokens)) for c in range(max(counts))]

    def build(n=1, **kw):
        return MiniGPT4Classifier(_Rows(args.rows), llm, tok, "<ImageHere>", lm, max_new_tokens=n, max_batch=args.rows, decode="hip",
                                  prefill="hip", **kw)

    hip, hf, gen, pre = build(score="hip"), build(score="hf"), build(args.new), build(1)
    legs = {f"score_hip_{c}": (lambda c=c: hip.answer_losses_from_embeds(img, "<ImageHere>", cands[:c])) for c in counts}
    if not args.skip_hf:
        legs.update({f"score_hf_{c}": (lambda c=c: hf.answer_losses_from_embeds(img, "<ImageHere>", cands[:c])) for c in counts})
    legs["generate_hip"] = lambda: gen._generate_graph(embs)
    legs["prefill_hip"] = lambda: pre._generate_graph(embs)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    clock_before = _clock()
    res = {k: [] for k in legs}
    outs = {}
    with torch.no_grad():
        for rep in range(args.warmup + args.reps):                     # interleaved: leg by leg inside every repetition
            for k, fn in legs.items():
                t, out = timed(fn)
                print(f"score_bench: repetition {rep} {k} {t:.1f} ms", file=sys.stderr, flush=True)
                if rep >= args.warmup:
                    res[k].append(t)
                    outs[k] = out
    clock_after = _clock()

    def med(k):
        return sorted(res[k])[len(res[k]) // 2]

    tail_rows = {c: args.rows * c * (args.answer_tokens - 1) for c in counts}
    line = {"tool": "score_bench", "rows": args.rows, "prompt": args.prompt, "answer_tokens": args.answer_tokens, "candidates": counts,
            "new_tokens": args.new, "layers": args.layers, "reps": args.reps, "warmup": args.warmup,
            "ms": res, "ms_min_max": {k: [min(v), max(v)] for k, v in res.items()},
            "prefill_token_rows": args.rows * args.prompt, "tail_token_rows": tail_rows,
            "score_hip_minus_prefill_median_ms": {c: med(f"score_hip_{c}") - med("prefill_hip") for c in counts},
            "slowest_score_hip_beats_fastest_generate": {c: max(res[f"score_hip_{c}"]) < min(res["generate_hip"]) for c in counts},
            "hip_scores_prefills": [hip.decode_stats["hip_scores"], hip.decode_stats["hip_prefills"]],
            "shader_clock_mhz_before_after": [clock_before, clock_after], "device": torch.cuda.get_device_name(0)}
    if not args.skip_hf:
        line["slowest_score_hip_beats_fastest_score_hf"] = {c: max(res[f"score_hip_{c}"]) < min(res[f"score_hf_{c}"]) for c in counts}
        line["score_hf_over_score_hip_median"] = {c: med(f"score_hf_{c}") / med(f"score_hip_{c}") for c in counts}
        line["max_abs_loss_difference_hip_hf"] = {c: float((outs[f"score_hip_{c}"] - outs[f"score_hf_{c}"]).abs().max()) for c in counts}
        line["rows_with_the_same_top_candidate"] = {c: int((outs[f"score_hip_{c}"].argmin(1) == outs[f"score_hf_{c}"].argmin(1)).sum()) for c in counts}
        line["hf_score_forwards"] = hf.decode_stats["hf_score_forwards"]
    print(json.dumps(line))


if __name__ == "__main__":
    main()
