"""Device time of `multi_select` answer scoring with per-row prompts and per-row candidates, legs interleaved in
one process.

Vicuna-7B-shaped random-init decoder (no checkpoint exists here; nothing is downloaded), 200 rows, prompts of two lengths inside one
prompt bucket (bos + 43 image positions, and two words more), 4 candidates whose answers differ per row in text and have 2 - 4
tokens.  Per repetition, by HIP events around each call:
    ragged_hip    (a) ragged="hip", score="hip": ONE ragged prefill + the ragged scoring pass (cgpt_llm_score_ragged)
    ragged_hf     (a) the same call on the model's own forward, once per candidate over the right-padded prompt + answer: what a
                      score="hip" classifier did with this call before the ragged entry existed (its counted fall-back)
    plain_hip     (b) score="hip" with ONE prompt and ONE candidate list for all rows: the plain entry, this build
    plain_other   (b) the same on the build given by --other-lib (the parent commit's), when it is given
Prints ONE JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap  # noqa: E402
from certifiedgpt_amd.minigpt4 import MiniGPT4Classifier, WordHashTokenizer  # noqa: E402
from tools.decode_step_bench import _Rows, _clock, _decoder, _other_library  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--prompt", type=int, default=44)
    ap.add_argument("--bucket", type=int, default=16)
    ap.add_argument("--cands", type=int, default=4)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--other-lib", default=None, help="another build of libcgpt.so for the plain_other leg")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures device time: it needs the GPU"
    assert 1 <= args.rows <= 256 and args.prompt >= 2 and 2 <= args.cands <= 16
    dev = "cuda:0"
    llm = _decoder(args.layers, dev)
    tok, lm = WordHashTokenizer(32000), AnswerLabelMap(4, ())
    g = torch.Generator(device="cpu").manual_seed(1)
    img = llm.get_input_embeddings()(torch.randint(3, 32000, (args.rows, args.prompt - 1), generator=g).to(dev))
    texts = ["<ImageHere>" if b % 2 == 0 else "<ImageHere> tell me" for b in range(args.rows)]
    # answers[c][b]: 2 - 4 words, another text in every row
    answers = [[" ".join(f"a{c}r{b}w{j}" for j in range(2 + (b + c) % 3)) for b in range(args.rows)] for c in range(args.cands)]
    shared = [" ".join(f"answer{c}word{j}" for j in range(3)) for c in range(args.cands)]

    def build(**kw):
        return MiniGPT4Classifier(_Rows(args.rows), llm, tok, "<ImageHere>", lm, max_new_tokens=1, max_batch=args.rows, decode="hip",
                                  prefill="hip", **kw)

    hip = build(ragged="hip", prompt_bucket=args.bucket, score="hip")
    hf = build(ragged="hip", prompt_bucket=args.bucket, score="hf")
    plain = build(score="hip")
    legs = {"ragged_hip": lambda: hip.answer_losses_from_embeds(img, texts, answers),
            "ragged_hf": lambda: hf.answer_losses_from_embeds(img, texts, answers),
            "plain_hip": lambda: plain.answer_losses_from_embeds(img, "<ImageHere>", shared)}
    if args.other_lib:
        with _other_library(args.other_lib):
            other = build(score="hip")
        legs["plain_other"] = lambda: other.answer_losses_from_embeds(img, "<ImageHere>", shared)

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
                print(f"score_ragged_bench: repetition {rep} {k} {t:.1f} ms", file=sys.stderr, flush=True)
                if rep >= args.warmup:
                    res[k].append(t)
                    outs[k] = out
    clock_after = _clock()

    def med(k):
        return sorted(res[k])[len(res[k]) // 2]

    d = float((outs["ragged_hip"] - outs["ragged_hf"]).abs().max())
    line = {"tool": "score_ragged_bench", "rows": args.rows, "prompt_lengths": [args.prompt, args.prompt + 2], "bucket": args.bucket,
            "candidates": args.cands, "answer_tokens": [2, 4], "layers": args.layers, "reps": args.reps, "warmup": args.warmup,
            "ms": res, "ms_median": {k: med(k) for k in res}, "ms_min_max": {k: [min(v), max(v)] for k, v in res.items()},
            "ragged_hf_over_ragged_hip_median": med("ragged_hf") / med("ragged_hip"),
            "slowest_ragged_hip_beats_fastest_ragged_hf": max(res["ragged_hip"]) < min(res["ragged_hf"]),
            "max_abs_loss_difference_hip_hf": d,
            "rows_with_the_same_top_candidate": int((outs["ragged_hip"].argmin(1) == outs["ragged_hf"].argmin(1)).sum()),
            "hip_ragged_scores_fallbacks": [hip.decode_stats["hip_ragged_scores"], hip.decode_stats["hf_score_fallbacks"]],
            "hf_score_forwards": hf.decode_stats["hf_score_forwards"],
            "shader_clock_mhz_before_after": [clock_before, clock_after], "device": torch.cuda.get_device_name(0)}
    if args.other_lib:
        line["plain_hip_minus_plain_other_median_ms"] = med("plain_hip") - med("plain_other")
        line["plain_spread_ms"] = {k: max(res[k]) - min(res[k]) for k in ("plain_hip", "plain_other")}
        line["plain_results_equal_bit_for_bit"] = bool(torch.equal(outs["plain_hip"], outs["plain_other"]))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
