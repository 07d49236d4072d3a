"""What a beam-search generate costs on the native LLaMA engine (beams="hip"), on a Vicuna-7B-shaped random-init
decoder (no checkpoint is needed; nothing is downloaded), native prefill, fp16, --images images x --beams beams, --new tokens:

    beam        beams="hip": one prefill of the images, the beam loop in chunks of max_batch // beams images, one captured graph
    beam_hf     the same classifier with beams="hf": today's fallback, HF `generate(num_beams=...)` on PyTorch-ROCm
    greedy_rows the native greedy generate of images x beams ROWS (num_beams=1): what the same number of token-step rows costs
                without the beam select and the ancestry attention -- it prefills every row, the beam leg one row per image
    greedy      the default path: the native greedy generate of --rows rows, nothing of this feature switched on
    parent      `greedy` on another build of the library (--parent-lib PATH, e.g. the parent commit's libcgpt.so), loaded beside
                this one: the default path must be unchanged (ranges that do not overlap are a difference to explain)

A generate is `generate_from_embeds`: from the image embeds to the decoded answer texts, host work included, with the wall clock
around a device sync.
Legs are interleaved and rotated by one place per repetition; min-max over --reps repetitions after --warmup.

    select      one beam select alone (cgpt_llm_beam_select_logits, mid-run state, vocabulary 32000) at the bench's shape (--beams
                beams, 1 EOS id, --images images) and at the largest K the entries take (8 beams, 8 EOS ids: K = 72, 32 images), each
                launch between two HIP events, the mean of --select-launches launches per repetition; --select-only runs nothing else
Prints ONE JSON line; --out PATH also writes it to a file.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from certifiedgpt_amd.agents.label_adapter import AnswerLabelMap  # noqa: E402
from certifiedgpt_amd.minigpt4 import MiniGPT4Classifier, WordHashTokenizer  # noqa: E402
from decode_step_bench import _Rows, _clock, _decoder, _other_library  # noqa: E402

PROMPT = "<s>[INST] <Img><ImageHere></Img> [vqa] what is shown in the picture [/INST]"


def emit(args, line):
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


def select_times(args, dev, vocab=32000, n=20, step=10):
    """{name: [min, max] us} of one cgpt_llm_beam_select_logits launch on a mid-run state: every image open, an empty pool."""
    import ctypes as C
    from certifiedgpt_amd import _lib
    L = _lib.lib()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = {}
    for name, images, k, num_eos in ((f"k{args.beams}_e1", args.images, args.beams, 1), ("k8_e8", 32, 8, 8)):
        rows = images * k
        g = torch.Generator(device="cpu").manual_seed(2)
        logits = (torch.randn(rows, vocab, generator=g) * 2).to(dev)
        state = [(-torch.rand(rows, generator=g) * 3 - 5).to(dev), torch.zeros(rows, n, dtype=torch.int64, device=dev),
                 torch.arange(rows, dtype=torch.int32, device=dev)[:, None].repeat(1, n).contiguous(),
                 torch.full((rows,), -1.0e9, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev),
                 torch.zeros(rows, dtype=torch.int32, device=dev), torch.zeros(rows, n, dtype=torch.int64, device=dev),
                 torch.ones(images, dtype=torch.int32, device=dev)]
        after = [torch.empty_like(t) for t in state]
        nxt, par = torch.empty(rows, dtype=torch.int64, device=dev), torch.empty(rows, dtype=torch.int32, device=dev)
        eos = (C.c_int64 * 8)(*range(2, 10))
        times = []
        for rep_i in range(args.warmup + args.reps):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            pairs = []
            for _ in range(args.select_launches):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                _lib.check(L.cgpt_llm_beam_select_logits(P(logits), vocab, images, k, vocab, step, n, 0, eos, num_eos, 0, 1.0,
                                                         *[P(t) for t in state], *[P(t) for t in after], P(nxt), P(par), st))
                b.record()
                pairs.append((a, b))
            torch.cuda.synchronize()
            if rep_i >= args.warmup:
                times.append(1e3 * sum(a.elapsed_time(b) for a, b in pairs) / len(pairs))
        out[name] = {"images": images, "beams": k, "eos_ids": num_eos, "keep": max(2, 1 + num_eos) * k, "vocab": vocab,
                     "us_min_max": [min(times), max(times)]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--rows", type=int, default=200, help="rows of the default-path legs (greedy, parent)")
    ap.add_argument("--new", type=int, default=20)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None, help="another build of libcgpt.so for the `parent` leg")
    ap.add_argument("--select-launches", type=int, default=20)
    ap.add_argument("--select-only", action="store_true", help="only the `select` measurement (no decoder is built)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    beam_rows = args.images * args.beams
    if args.select_only:
        return emit(args, {"tool": "beam_bench", "select_us": select_times(args, dev), "select_launches": args.select_launches,
                           "note": "select_us: one eager launch between two HIP events, so the figure includes what the events see of the "
                                   "launch itself", "device": torch.cuda.get_device_name(0)})
    llm = _decoder(args.layers, dev)
    tok = WordHashTokenizer(32000)
    lm = AnswerLabelMap(3, ["red", "blue"], frozen=True)
    g = torch.Generator(device="cpu").manual_seed(1)
    emb = (torch.randn(max(beam_rows, args.rows), 32, 4096, generator=g) * 0.02).to(dev).to(torch.float16)

    def build(max_batch, **kw):
        return MiniGPT4Classifier(_Rows(max_batch), llm, tok, PROMPT, lm, max_new_tokens=args.new, max_batch=max_batch, decode="hip",
                                  prefill="hip", **kw)

    beams = {"num_beams": args.beams}
    clfs = {"beam": (build(beam_rows, beams="hip", generate_kwargs=beams), args.images),
            "beam_hf": (build(beam_rows, generate_kwargs=beams), args.images),
            "greedy_rows": (build(beam_rows), beam_rows),
            "greedy": (build(args.rows), args.rows)}
    if args.parent_lib:
        with _other_library(args.parent_lib):
            clfs["parent"] = (build(args.rows), args.rows)
    legs = list(clfs)

    def generate(e):
        clf, n = clfs[e]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        clf.generate_from_embeds(emb[:n], PROMPT)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    clock_before = _clock()
    res = {e: {"ms": [], "order": []} for e in legs}
    with torch.no_grad():
        for rep_i in range(args.warmup + args.reps):
            k = rep_i % len(legs)
            for place, e in enumerate(legs[k:] + legs[:k]):
                t = generate(e)
                print(f"beam_bench: repetition {rep_i} {e} {t:.1f} ms", file=sys.stderr, flush=True)
                if rep_i >= args.warmup:
                    res[e]["ms"].append(t)
                    res[e]["order"].append(place)
    clock_after = _clock()

    def med(v):
        return sorted(v)[len(v) // 2]

    for r in res.values():
        r["ms_min_max"] = [min(r["ms"]), max(r["ms"])]
    line = {"tool": "beam_bench", "images": args.images, "beams": args.beams, "beam_rows": beam_rows, "default_path_rows": args.rows,
            "new_tokens": args.new, "layers": args.layers, "reps": args.reps, "warmup": args.warmup,
            "leg_order": "rotated by one place per repetition", "leg_cycle": legs, "legs": res,
            "beam_over_beam_hf_median": med(res["beam"]["ms"]) / med(res["beam_hf"]["ms"]),
            "beam_over_greedy_rows_median": med(res["beam"]["ms"]) / med(res["greedy_rows"]["ms"]),
            "hip_beam_calls": clfs["beam"][0].decode_stats["hip_beam"], "hf_calls_of_beam_hf": clfs["beam_hf"][0].decode_stats["hf_calls"],
            "select_us": select_times(args, dev), "select_launches": args.select_launches,
            "shader_clock_mhz_before_after": [clock_before, clock_after], "device": torch.cuda.get_device_name(0)}
    if "parent" in res:
        (a0, a1), (b0, b1) = res["greedy"]["ms_min_max"], res["parent"]["ms_min_max"]
        line["parent_lib"] = os.path.basename(args.parent_lib)
        line["greedy_and_parent_ranges_overlap"] = bool(a0 <= b1 and b0 <= a1)
        line["greedy_over_parent_median"] = med(res["greedy"]["ms"]) / med(res["parent"]["ms"])
    emit(args, line)


if __name__ == "__main__":
    main()
