"""The LayerNorm kernels in every form the forward launches them in, through the raw entry cgpt_layernorm_resid: the deferred residual
adds (delta, delta2), keep_x, the fp32 stream store and both outputs -- which cgpt_layernorm cannot reach.  Two kernels serve the
16-byte path (cgpt_set_option "ln_kernel": 0 = chunk-at-a-time body, 1 = loads-first rows kernel with gamma / beta in LDS and a
grid-stride loop over row groups); they must agree bit for bit, the stored stream must be the exact fp32 sum, and nothing outside
the rows may be written (a workgroup holds 8 rows: a dead half-wave reads a clamped row and must not store).

Tolerances: those of test_gpu_kernels.py's cgpt_layernorm tests against a float64 LayerNorm of the kernel's own fp32 sum: 2e-5 (fp32
out) and 2e-3 (fp16 out) x max(1, max|ref|)."""
import ctypes as C
import functools

import pytest
import torch

import certifiedgpt_amd as cg
from certifiedgpt_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-6
ROWS = (1, 7, 8, 9, 17, 2 * 257 + 1)
# more row groups than any resident grid of the rows kernel (CUs x 6 workgroups of 8 rows on a 256-CU device = 12 288 rows): some workgroups walk
# two groups, the others one, and the last group is partly dead
ROWS_STRIDE_LOOP = 8 * 256 * 7 + 5
CANARY_ROWS = 2
# (delta, delta2, keep_x): none | LN1 | LN2 | block-0 LN2 | ln_vision
UPDATE_FORMS = {"none": (False, False, 0), "delta_keep_x": (True, False, 1), "delta_delta2_store": (True, True, 0),
                "delta2_store": (False, True, 0), "delta_store": (True, False, 0)}


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def inputs(rows, D):
    """x with row means ~ 3 sigma and four channels 50 x the rest; updates whose magnitudes run over the fp16 range; gamma, beta."""
    g = torch.Generator(device="cpu").manual_seed(1000 * D + rows)
    sig = torch.exp(torch.randn(rows, 1, generator=g))
    x = sig * (torch.randn(rows, D, generator=g) + 3.0 * torch.sign(torch.randn(rows, 1, generator=g)))
    x[:, [1, D // 3, D // 2 + 5, D - 2]] *= 50.0

    def update():
        mag = torch.exp2(torch.rand(rows, D, generator=g) * 29.0 - 14.0)          # 2^-14 .. 2^15
        return (torch.randn(rows, D, generator=g) * mag).clamp(-6e4, 6e4).half()

    return x, update(), update(), 1.0 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)


@functools.lru_cache(maxsize=None)
def reference(rows, D, has_d, has_d2):
    """(the fp32 sum (x + delta) + delta2 computed on the host, its float64 LayerNorm)"""
    x, d, d2, w, b = inputs(rows, D)
    v = x.clone()
    if has_d:
        v = v + d.float()
    if has_d2:
        v = v + d2.float()
    ref = torch.nn.functional.layer_norm(v.to(DEV).double(), (D,), w.to(DEV).double(), b.to(DEV).double(), EPS).cpu()
    return v, ref


def run_form(kernel, rows, D, form, with_y32, pad):
    """One launch on fresh buffers with canary rows behind the last row; returns the host copies (x, y16, y32)."""
    L = cg.lib()
    has_d, has_d2, keep_x = UPDATE_FORMS[form]
    x, d, d2, w, b = inputs(rows, D)
    ld16, ld32 = D + pad, D + (pad and 4)
    tot = rows + CANARY_ROWS
    xd = torch.full((tot, D), 77.0, device=DEV)
    xd[:rows] = x.to(DEV)
    dd = d.to(DEV) if has_d else None
    d2d = d2.to(DEV) if has_d2 else None
    y16 = torch.full((tot, ld16), -7.0, dtype=torch.float16, device=DEV)
    y32 = torch.full((tot, ld32), -7.0, device=DEV) if with_y32 else None
    wd, bd = w.to(DEV), b.to(DEV)
    _lib.check(L.cgpt_set_option(b"ln_kernel", kernel))
    try:
        _lib.check(L.cgpt_layernorm_resid(P(xd), D, P(dd), D if has_d else 0, P(d2d), D if has_d2 else 0, keep_x, P(wd), P(bd), EPS, P(y16), ld16,
                                          P(y32), ld32 if with_y32 else 0, rows, D, stream()))
        torch.cuda.synchronize()
    finally:
        _lib.check(L.cgpt_set_option(b"ln_kernel", 1))
    return xd.cpu(), y16.cpu(), y32.cpu() if with_y32 else None


def check_form(rows, D, form, with_y32, pad):
    has_d, has_d2, keep_x = UPDATE_FORMS[form]
    x = inputs(rows, D)[0]
    v, ref = reference(rows, D, has_d, has_d2)
    tag = f"{form} rows={rows} D={D} y32={with_y32} pad={pad}"
    old = run_form(0, rows, D, form, with_y32, pad)
    new = run_form(1, rows, D, form, with_y32, pad)
    for name, a, b in zip(("x", "y16", "y32"), old, new):
        if a is not None:
            assert torch.equal(a, b), f"ln_kernel 1 and 0 differ in {name} ({tag})"
    xs, y16, y32 = new
    stores = (has_d or has_d2) and not keep_x
    assert torch.equal(xs[:rows], v if stores else x), f"x after the launch is not {'the exact fp32 sum' if stores else 'untouched'} ({tag})"
    assert bool((xs[rows:] == 77.0).all()), f"canary rows of x were written ({tag})"
    assert bool((y16[rows:] == -7.0).all()) and bool((y16[:, D:] == -7.0).all()), f"y16 written outside the rows / columns ({tag})"
    scale = max(1.0, float(ref.abs().max()))
    err16 = float((y16[:rows, :D].double() - ref).abs().max())
    print(f"{tag}: max abs err fp16 {err16:.3e} (bound {2e-3 * scale:.3e})", end="")
    assert err16 <= 2e-3 * scale, f"y16 off the float64 LayerNorm by {err16} ({tag})"
    if with_y32:
        assert bool((y32[rows:] == -7.0).all()) and bool((y32[:, D:] == -7.0).all()), f"y32 written outside the rows / columns ({tag})"
        err32 = float((y32[:rows, :D].double() - ref).abs().max())
        print(f", fp32 {err32:.3e} (bound {2e-5 * scale:.3e})", end="")
        assert err32 <= 2e-5 * scale, f"y32 off the float64 LayerNorm by {err32} ({tag})"
    print()


@pytest.mark.parametrize("form", list(UPDATE_FORMS))
@pytest.mark.parametrize("D", [1408, 768, 128])
def test_forms_agree_store_exactly_and_stay_inside_the_rows(D, form):
    for rows in ROWS:
        check_form(rows, D, form, with_y32=False, pad=0)
        check_form(rows, D, form, with_y32=True, pad=64 if rows % 2 else 0)      # padded leading dimensions on the odd row counts
    check_form(9, D, form, with_y32=False, pad=64)


@pytest.mark.parametrize("form", list(UPDATE_FORMS))
def test_grid_stride_loop_ends_at_the_last_row(form):
    """More row groups than resident workgroups at the ViT-G width: the loop's later rounds and its end, canaries behind the last row."""
    check_form(ROWS_STRIDE_LOOP, 1408, form, with_y32=False, pad=0)


def test_strided_rows_like_the_cls_call():
    """ln_vision on the CLS rows: 5 rows, one per image, ldx = ldd = 257 D; the other 256 rows of every image are canaries."""
    L = cg.lib()
    D, T, nb = 1408, 257, 5
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randn(nb * T, D, generator=g) * 2.0 + 6.0
    d = (torch.randn(nb * T, D, generator=g) * 30.0).half()
    w, b = 1.0 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    v = x[::T] + d[::T].float()
    ref = torch.nn.functional.layer_norm(v.double(), (D,), w.double(), b.double(), EPS)
    outs = []
    for kernel in (0, 1):
        xd, dd, wd, bd = x.to(DEV), d.to(DEV), w.to(DEV), b.to(DEV)
        y16 = torch.full((nb + CANARY_ROWS, D), -7.0, dtype=torch.float16, device=DEV)
        _lib.check(L.cgpt_set_option(b"ln_kernel", kernel))
        try:
            _lib.check(L.cgpt_layernorm_resid(P(xd), T * D, P(dd), T * D, None, 0, 0, P(wd), P(bd), EPS, P(y16), D, None, 0, nb, D, stream()))
            torch.cuda.synchronize()
        finally:
            _lib.check(L.cgpt_set_option(b"ln_kernel", 1))
        outs.append((xd.cpu(), y16.cpu()))
    (x0, y0), (x1, y1) = outs
    assert torch.equal(x0, x1) and torch.equal(y0, y1)
    want = x.clone()
    want[::T] = v
    assert torch.equal(x1, want), "the CLS rows are not the exact sum, or another row of an image was written"
    assert bool((y1[nb:] == -7.0).all())
    err = float((y1[:nb].double() - ref).abs().max())
    print(f"strided CLS rows: max abs err fp16 {err:.3e}")
    assert err <= 2e-3 * max(1.0, float(ref.abs().max()))


def test_refusals():
    L = cg.lib()
    D, rows = 1408, 4
    x = torch.zeros(rows, D + 2, device=DEV)
    d = torch.zeros(rows, D + 2, dtype=torch.float16, device=DEV)
    w, b = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    y16 = torch.zeros(rows, D + 2, dtype=torch.float16, device=DEV)
    y32 = torch.zeros(rows, D + 2, device=DEV)

    def call(xp=x, ldx=D, dp=d, ldd=D, d2p=None, ldd2=0, wp=w, bp=b, y16p=y16, ldy16=D, y32p=y32, ldy32=D, dim=D):
        return L.cgpt_layernorm_resid(P(xp), ldx, P(dp), ldd, P(d2p), ldd2, 1, P(wp), P(bp), EPS, P(y16p), ldy16, P(y32p), ldy32, rows, dim, stream())

    assert call() == 0
    bad = {"null x": dict(xp=None), "null gamma": dict(wp=None), "null beta": dict(bp=None), "no output": dict(y16p=None, y32p=None),
           "odd ldx": dict(ldx=D + 1), "odd ldd": dict(ldd=D + 1), "odd ldd2": dict(d2p=d, ldd2=D + 1), "odd ldy16": dict(ldy16=D + 1),
           "odd ldy32": dict(ldy32=D + 1), "D = 0": dict(dim=0), "odd D": dict(dim=127, ldx=128, ldd=128, ldy16=128, ldy32=128),
           "D above 4096": dict(dim=4098, ldx=4098, ldd=4098, ldy16=4098, ldy32=4098), "ldx below D": dict(ldx=D - 2)}
    for name, kw in bad.items():
        assert call(**kw) == 1, f"{name}: expected CGPT_ERR_INVALID"
        assert b"cgpt_layernorm_resid" in L.cgpt_last_error()
    torch.cuda.synchronize()
