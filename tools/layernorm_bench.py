"""Raw timing of the ViT-block LayerNorm launches: both kernels of the 16-byte path (cgpt_set_option "ln_kernel": 0 = chunk-at-a-time body,
1 = loads-first rows kernel; a lab build of the library also takes the schedules 10..15, see --variants) and two copy yardsticks with the same
per-element byte mix (tools/layernorm_copy.hip), interleaved in ONE process and timed by HIP events: us per launch and TB/s per case and round.

Forms (through cgpt_layernorm_resid): LN1 = delta + keep_x (8 B per element), LN2 = delta + delta2 + store (14 B), block-0 LN1 = no update (6 B),
and the Q-Former's post-LN (768 wide, fp16 + fp32 out, 10 B).  Shapes: the bench's batch, M = 255 x 257 rows of D = 1408, and 8 x 257 rows.
A LayerNorm form is judged against the copy of ITS mix (the rate this device grants that access pattern), not against the HBM data-sheet peak.

  timeout -k 10 600 python3 tools/layernorm_bench.py [--rounds 5] [--launches 20] [--variants 10,11,...] [--out FILE]
The copy kernels are built on first use (hipcc, gfx950) into tools/liblayernorm_copy.so."""
import argparse, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctypes as C, torch
import certifiedgpt_amd as cg
from certifiedgpt_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--variants", default="", help="further ln_kernel values to time (lab builds: 10..15 = 10 + 3 * SPLIT + (WAVES - 4))")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.rounds >= 3, "at least three interleaved rounds"

HERE = os.path.dirname(os.path.abspath(__file__))
COPY_SO = os.path.join(HERE, "liblayernorm_copy.so")
if not os.path.exists(COPY_SO):
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "--offload-arch=gfx950", "-shared", "-fPIC",
                    os.path.join(HERE, "layernorm_copy.hip"), "-o", COPY_SO], check=True, timeout=300)
CP = C.CDLL(COPY_SO)
CP.ln_copy.restype = C.c_int
CP.ln_copy.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]

L = cg.lib(); DEV = "cuda:0"
def P(t): return C.c_void_p(t.data_ptr()) if t is not None else None
def st(): return C.c_void_p(torch.cuda.current_stream().cuda_stream)
KERNELS = [0, 1] + [int(v) for v in args.variants.split(",") if v]
for k in KERNELS:
    _lib.check(L.cgpt_set_option(b"ln_kernel", k))          # a value this build does not have fails here, before anything is timed
_lib.check(L.cgpt_set_option(b"ln_kernel", 1))

# form: (delta, delta2, keep_x, y32, bytes per element)
FORMS = {"LN1 (delta, keep_x)": (1, 0, 1, 0, 8), "LN2 (delta, delta2, store)": (1, 1, 0, 0, 14), "block-0 LN1 (no update)": (0, 0, 1, 0, 6),
         "Q-Former post-LN (y16 + y32)": (0, 0, 0, 1, 10)}
SHAPES = [(255 * 257, 1408), (8 * 257, 1408)]
QF_SHAPE = (255 * 32, 768)
g = torch.Generator(device=DEV).manual_seed(7)
bufs = {}
for M, D in SHAPES + [QF_SHAPE]:
    bufs[(M, D)] = dict(x=torch.randn(M, D, device=DEV, generator=g), d=(torch.randn(M, D, device=DEV, generator=g) * 1e-3).half(),
                        d2=(torch.randn(M, D, device=DEV, generator=g) * 1e-3).half(), y16=torch.zeros(M, D, device=DEV, dtype=torch.float16),
                        y32=torch.zeros(M, D, device=DEV), w=torch.randn(D, device=DEV, generator=g), b=torch.randn(D, device=DEV, generator=g))

def ln(shape, form, kern):
    M, D = shape; t = bufs[shape]; hd, hd2, keep, y32, _ = FORMS[form]
    _lib.check(L.cgpt_set_option(b"ln_kernel", kern))
    _lib.check(L.cgpt_layernorm_resid(P(t["x"]), D, P(t["d"]) if hd else None, D if hd else 0, P(t["d2"]) if hd2 else None, D if hd2 else 0, keep,
                                      P(t["w"]), P(t["b"]), 1e-6, P(t["y16"]), D, P(t["y32"]) if y32 else None, D if y32 else 0, M, D, st()))

def copy(shape, mix, unroll):
    M, D = shape; t = bufs[shape]
    e = CP.ln_copy(mix, unroll, P(t["xc"]), P(t["d"]), P(t["d2"]), P(t["y16"]), M * D, st())
    assert e == 0, f"ln_copy: hipError {e}"

cases = {}    # name -> (callable, bytes)
for shape in SHAPES:
    M, D = shape
    for form in list(FORMS)[:3]:
        for k in KERNELS:
            cases[f"{M}x{D} {form} ln_kernel={k}"] = (lambda s=shape, f=form, k=k: ln(s, f, k), M * D * FORMS[form][4])
    for u in (1, 2, 4):                                   # groups of 4 elements per thread: the fastest is the yardstick
        cases[f"{M}x{D} copy, LN1 mix, {u} per thread"] = (lambda s=shape, u=u: copy(s, 1, u), M * D * 8)
        cases[f"{M}x{D} copy, LN2 mix, {u} per thread"] = (lambda s=shape, u=u: copy(s, 2, u), M * D * 14)
for shape in SHAPES:
    bufs[shape]["xc"] = bufs[shape]["x"].clone()          # the copies write bit mixes: keep them out of the LayerNorms' input
for k in (0, 1):
    M, D = QF_SHAPE
    cases[f"{M}x{D} Q-Former post-LN (y16 + y32) ln_kernel={k}"] = (lambda k=k: ln(QF_SHAPE, "Q-Former post-LN (y16 + y32)", k), M * D * 10)

res = {n: [] for n in cases}
for n, (fn, _) in cases.items():
    for _ in range(3): fn()
torch.cuda.synchronize()
for r in range(args.rounds):
    for n, (fn, _) in cases.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches): fn()
        e1.record(); torch.cuda.synchronize()
        res[n].append(e0.elapsed_time(e1) * 1000.0 / args.launches)
_lib.check(L.cgpt_set_option(b"ln_kernel", 1))

lines = [f"# {torch.cuda.get_device_name(0)}; {args.rounds} interleaved rounds x {args.launches} launches; us per launch per round | median us | median TB/s"]
for n, (_, nbytes) in cases.items():
    med = statistics.median(res[n])
    lines.append(f"{n:62s} " + " ".join(f"{v:7.1f}" for v in res[n]) + f" | {med:7.1f} us | {nbytes / med / 1e6:5.2f} TB/s")
text = "\n".join(lines)
print(text, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text + "\n")
