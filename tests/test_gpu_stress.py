"""The device forward on trained-like weights (oracle/model_oracle.py: stress_params -- peaked attention, residual outlier
channels ~1e2, token rows whose mean is >= 3 sigma) against the fp32 oracle, stage by stage, at per-stage tolerances
(mo.STRESS_TOL).  Under the plain init law every softmax is almost uniform and a wrong K pointer, scale or K/V slice moves no
stage past the tiny tests' 1e-2; here each such bug moves its stage by >= 10x the tolerance (tests/test_oracle_stress.py
measures that on the CPU, together with the error the fp16 stores alone cause).  Every measured error is printed."""
import os

import numpy as np
import pytest
import torch

import certifiedgpt_amd as cg
from oracle import model_oracle as mo, smooth_oracle as so
from gpu_util import DEV, make_classifier

pytestmark = pytest.mark.gpu
SEED = 20251121
FULL_WIDTH = dict(img_size=224, vit_dim=1408, vit_heads=16, vit_mlp=6144, vit_depth=2)


def stress_pair(mode, max_batch, num_classes=10, **over):
    cfg = mo.stress_config(mode, num_classes=num_classes, **over)
    params = mo.stress_params(mo.init_params(cfg, SEED), cfg)
    clf = make_classifier(cfg, max_batch)
    missing, unexpected = clf.load_state_dict(params)
    assert not missing and not unexpected
    return clf, mo.round_fp16_weights(params), cfg


def check_stages(clf, p16, cfg, nb, label, tol=mo.STRESS_TOL):
    """Noisy batch of the synthetic image through classify / forward_logits vs the oracle: every stage, finiteness, decisive
    argmax, and the fused noise path bit-identical to classify on the same noisy batch."""
    x0 = torch.from_numpy(mo.synthetic_image(cfg)).to(DEV)
    noisy = cg.noise_batch(x0, 0, nb, 0.5, 42)
    logits = clf(noisy)
    got = {"logits": logits}
    for what in ["vit_out"] + (["ln_vision", "qformer", "llama"] if cfg.mode == mo.MODE_ENCODE_IMG else []):
        got[what] = clf.activation(what, nb)
    torch.set_num_threads(min(os.cpu_count() or 1, int(os.environ.get("CGPT_CPU_THREADS", "16"))))   # the box's CPU share
    ref = mo.forward_all(p16, noisy.cpu(), cfg)
    errs = mo.stress_errors(got, ref)
    print(f"\n[{label}] T={cfg.tokens} width={cfg.vit_dim} nb={nb}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (label, k)
    bad = {k: (v, tol[k]) for k, v in errs.items() if not v <= tol[k]}
    assert not bad, (label, bad)
    r = ref["logits"]
    top2 = r.topk(2, dim=1).values
    decisive = (top2[:, 0] - top2[:, 1]) > 2e-2 * r.abs().max()
    agree = logits.cpu().argmax(1) == r.argmax(1)
    assert bool(agree[decisive].all()), (label, int((~agree).sum()), int(decisive.sum()))
    fused = clf.forward_logits(x0, 0, nb, 0.5, 42)
    assert torch.equal(fused, logits), label
    return errs


@pytest.mark.parametrize("mode", [mo.MODE_VIT_HEAD, mo.MODE_ENCODE_IMG])
def test_stress_model_matches_oracle_all_stages(mode):
    clf, p16, cfg = stress_pair(mode, max_batch=8)
    try:
        check_stages(clf, p16, cfg, 8, f"stress mode {mode}")
    finally:
        clf.close()


@pytest.mark.parametrize("img_size", [280, 448])
def test_stress_streaming_attention_inside_the_model(img_size):
    """T = 401 (streaming kernel) and T = 1025 (streaming kernel with the lone 1025th query split by keys) with peaked scores."""
    clf, p16, cfg = stress_pair(mo.MODE_ENCODE_IMG, max_batch=2, img_size=img_size)
    try:
        check_stages(clf, p16, cfg, 2, f"stress {img_size}^2")
    finally:
        clf.close()


def test_stress_full_vit_width():
    """vit_dim 1408 / 16 heads of 88 / mlp 6144 at 224^2 (T = 257): layernorm4_vitg_kernel, the resident attention kernel at
    hd = 88 and the large-shape GEMMs, under the stress law; Q-Former at the tiny widths."""
    clf, p16, cfg = stress_pair(mo.MODE_ENCODE_IMG, max_batch=2, **FULL_WIDTH)
    try:
        check_stages(clf, p16, cfg, 2, "stress full ViT width", mo.STRESS_TOL_FULL_WIDTH)
    finally:
        clf.close()


def test_stress_smooth_matches_oracle_on_identical_noise():
    """Smooth.certify on the stress weights vs SmoothOracle fed the GPU's own noise: votes agree on every decisive sample,
    and (label, radius) equal the oracle statistics of the GPU counts."""
    K = 10
    clf, p16, cfg = stress_pair(mo.MODE_ENCODE_IMG, max_batch=16, num_classes=K)
    try:
        x0 = torch.from_numpy(mo.synthetic_image(cfg)).to(DEV)
        sigma, seed, n0, n, alpha, bs = 0.25, 5, 24, 40, 0.05, 16

        def gpu_noise(first, num, shape):
            return cg.noise_batch(torch.zeros(shape, device=DEV), first, num, 1.0, seed).cpu().numpy()

        oracle = so.SmoothOracle(mo.make_classifier(p16, cfg), K, sigma, gpu_noise)
        noisy = cg.noise_batch(x0, 0, n0 + n, sigma, seed)
        ref_logits = mo.forward_all(p16, noisy.cpu(), cfg)["logits"]
        got_logits = torch.cat([clf(noisy[i:i + 16]) for i in range(0, n0 + n, 16)]).cpu()
        top2 = ref_logits.topk(2, dim=1).values
        decisive = (top2[:, 0] - top2[:, 1]) > 2e-2 * ref_logits.abs().max()
        agree = got_logits.argmax(1) == ref_logits.argmax(1)
        print(f"\n[stress smooth] decisive {int(decisive.sum())}/{n0 + n}, agree {int(agree.sum())}/{n0 + n}")
        assert bool(agree[decisive].all()), (int((~agree).sum()), int(decisive.sum()))
        s = cg.Smooth(clf, K, sigma, seed=seed)
        c_sel = s._sample_noise(x0, n0, bs)
        c_est = s._sample_noise(x0, n, bs)
        oracle._cursor = 0
        o_sel = oracle._sample_noise(x0.cpu().numpy(), n0, bs)
        o_est = oracle._sample_noise(x0.cpu().numpy(), n, bs)
        flips = int(np.abs(c_sel - o_sel).sum() + np.abs(c_est - o_est).sum()) // 2
        assert flips <= int((~decisive).sum()), (c_sel, o_sel, c_est, o_est)
        lab, rad = s.certify_from_counts(c_sel, c_est, n, alpha)
        olab, orad = so.certify_from_counts(c_sel, c_est, n, alpha, sigma)
        assert lab == olab and abs(rad - orad) <= 1e-9
        s.reset()
        assert s.certify(x0, n0, n, alpha, bs) == (lab, rad)
    finally:
        clf.close()
