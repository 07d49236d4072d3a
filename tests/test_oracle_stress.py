"""The stress weight law of the oracle (oracle/model_oracle.py: stress_config / stress_params) on the CPU: it has the
statistics it claims (peaked attention, outlier channels, rows far off zero, nothing near the fp16 range), every wiring
bug the GPU stress tests (tests/test_gpu_stress.py) are meant to catch moves its stage by >= 10x the tolerance that test
uses, and the error the device's fp16 stores alone cause (forward_all(fp16_contract=True)) stays <= 1/3 of it.  So if
someone edits the law later, this file says whether the GPU tests still mean anything."""
import numpy as np
import pytest
import torch

from oracle import model_oracle as mo, philox

SEED = 20251121
TOL = mo.STRESS_TOL


def stress_setup(mode=mo.MODE_ENCODE_IMG, batch=8, **over):
    cfg = mo.stress_config(mode, **over)
    p16 = mo.round_fp16_weights(mo.stress_params(mo.init_params(cfg, SEED), cfg))
    x0 = torch.from_numpy(mo.synthetic_image(cfg))
    x = x0 + 0.5 * torch.from_numpy(philox.noise_batch(42, 0, batch, tuple(x0.shape)))
    return cfg, p16, x


def test_stress_law_has_the_statistics_it_claims():
    cfg, p16, x = stress_setup()
    probe = {}
    ref = mo.forward_all(p16, x, cfg, probe=probe)
    for kind, a in probe["attn"].items():
        std, mp = float(np.median(a["logit_std"])), float(np.median(a["max_prob"]))
        print(f"attention {kind:9s}: logit std {np.round(a['logit_std'], 2)} median max-prob {np.round(a['max_prob'], 2)}")
        assert 1.5 <= std <= 6.0, (kind, std)
        assert 0.2 <= mp <= 0.8, (kind, mp)
    assert set(probe["attn"]) == {"vit", "qf_self", "qf_cross"}
    vit = ref["vit_out"]
    chans = list(mo.STRESS_OUTLIER_CHANNELS)
    rest = [c for c in range(cfg.vit_dim) if c not in chans]
    outl = vit[..., chans].abs().amax(dim=(0, 1))
    centred_rest = (vit[..., rest] - vit[..., rest].mean(dim=-1, keepdim=True)).abs().max()
    print(f"vit_out: outlier channels max |x| {outl.tolist()}, other channels max |x - row mean| {float(centred_rest):.2f}")
    assert float(outl.max()) >= 100.0 and float(outl.min()) >= 16.0
    assert float(centred_rest) <= 8.0 and float(outl.max()) >= 10.0 * float(centred_rest)
    ratio = vit.mean(dim=-1).abs() / vit.std(dim=-1)
    print(f"vit_out: row mean / row sigma min {float(ratio.min()):.2f} median {float(ratio.median()):.2f}")
    assert float(ratio.min()) >= 3.0
    for k, v in ref.items():
        assert bool(torch.isfinite(v).all()), k
    fmax = probe["fp16_max"]
    print("largest value through each fp16 store:", {k: round(v, 1) for k, v in fmax.items()})
    assert max(fmax.values()) <= 65504.0 / 8
    assert {"im2col", "xn", "qkv", "attn_p", "attn_o", "proj", "gelu_hidden", "fc2", "emb", "kv_all", "qqkv", "qq", "qctx",
            "qff", "qh16", "pooled"} <= set(fmax)


def test_stress_law_leaves_the_plain_law_alone():
    cfg = mo.stress_config(mo.MODE_ENCODE_IMG)
    plain = mo.init_params(cfg, SEED)
    before = {k: v.clone() for k, v in plain.items()}
    mo.stress_params(plain, cfg)
    assert all(torch.equal(before[k], plain[k]) for k in plain)                      # a new dict; the input is untouched
    tiny = mo.tiny_config(mo.MODE_ENCODE_IMG)
    assert (tiny.vit_depth, tiny.qf_layers, tiny.img_size) == (2, 2, 56)             # pinned by model_golden.npz
    assert (cfg.vit_depth, cfg.qf_layers, cfg.vit_dim, cfg.qf_dim) == (3, 4, 176, 128)


def _vit_blocks(cfg):
    return [f"visual_encoder.blocks.{i}." for i in range(cfg.vit_depth)]


def perturb(p, cfg, name):
    """The parameter change that computes what a named wiring bug of the device forward computes."""
    q = {k: v.clone() for k, v in p.items()}
    D, hd = cfg.vit_dim, cfg.vit_dim // cfg.vit_heads
    if name == "vit q x2 (attention scale x2)":
        for b in _vit_blocks(cfg):
            q[b + "attn.qkv.weight"][:D] *= 2
            q[b + "attn.q_bias"] *= 2
    elif name == "vit q x0 (keys ignored)":
        for b in _vit_blocks(cfg):
            q[b + "attn.qkv.weight"][:D] *= 0
            q[b + "attn.q_bias"] *= 0
    elif name == "vit K<->V rows swapped":
        for b in _vit_blocks(cfg):
            w = q[b + "attn.qkv.weight"]
            k = w[D:2 * D].clone()
            w[D:2 * D] = w[2 * D:]
            w[2 * D:] = k
    elif name == "vit proj input permuted by head":
        for b in _vit_blocks(cfg):
            w = q[b + "attn.proj.weight"]
            w[:] = torch.cat([w[:, hd:], w[:, :hd]], dim=1)
    elif name in ("qformer self-attention scale x2", "qformer cross-attention scale x2"):
        att = ".attention." if "self" in name else ".crossattention."
        for k in q:
            if att + "self.query." in k:
                q[k] *= 2
    elif name == "qformer cross layer 2 reads layer 0's K/V":
        for s in ("key", "value"):
            for t in ("weight", "bias"):
                q[f"Qformer.bert.encoder.layer.2.crossattention.self.{s}.{t}"] = \
                    q[f"Qformer.bert.encoder.layer.0.crossattention.self.{s}.{t}"].clone()
    else:
        raise KeyError(name)
    return q


PERTURBATIONS = [("vit q x2 (attention scale x2)", "vit_out_chan"), ("vit q x0 (keys ignored)", "vit_out_chan"),
                 ("vit K<->V rows swapped", "vit_out_chan"), ("vit proj input permuted by head", "vit_out_chan"),
                 ("qformer self-attention scale x2", "qformer"), ("qformer cross-attention scale x2", "qformer"),
                 ("qformer cross layer 2 reads layer 0's K/V", "qformer")]


def test_each_wiring_perturbation_moves_its_stage_by_10x_the_gpu_tolerance():
    cfg, p16, x = stress_setup()
    base = mo.forward_all(p16, x, cfg)
    no_vbias = {k: (v * 0 if k.endswith("attn.v_bias") else v) for k, v in p16.items()}   # K has no bias on the device
    base_nv = mo.forward_all(no_vbias, x, cfg)
    print(f"\n{'perturbation':44s} {'stage':13s} {'moved':>9s} {'gpu tol':>9s} {'ratio':>8s}")
    worst = np.inf
    for name, stage in PERTURBATIONS:
        src, ref = (no_vbias, base_nv) if "K<->V" in name else (p16, base)
        moved = mo.stress_errors(mo.forward_all(perturb(src, cfg, name), x, cfg), ref)[stage]
        ratio = moved / TOL[stage]
        worst = min(worst, ratio)
        print(f"{name:44s} {stage:13s} {moved:9.2e} {TOL[stage]:9.1e} {ratio:8.1f}")
    assert worst >= 10.0, worst


@pytest.mark.parametrize("mode,over,batch", [(mo.MODE_VIT_HEAD, {}, 8), (mo.MODE_ENCODE_IMG, {}, 8),
                                             (mo.MODE_ENCODE_IMG, {"img_size": 280}, 2),
                                             (mo.MODE_ENCODE_IMG, {"img_size": 448}, 2),
                                             (mo.MODE_ENCODE_IMG, dict(img_size=224, vit_dim=1408, vit_heads=16, vit_mlp=6144,
                                                                       vit_depth=2), 2)])
def test_emulated_fp16_contract_error_is_a_third_of_the_tolerance(mode, over, batch):
    cfg, p16, x = stress_setup(mode, batch, **over)
    ref = mo.forward_all(p16, x, cfg)
    emu = mo.forward_all(p16, x, cfg, fp16_contract=True)
    errs = mo.stress_errors(emu, ref)
    print(f"\nemulated fp16 contract, mode {mode} {cfg.img_size}^2:", {k: f"{v:.2e}" for k, v in errs.items()})
    tol = mo.STRESS_TOL_FULL_WIDTH if cfg.vit_dim == 1408 else TOL
    for k, e in errs.items():
        assert e <= tol[k] / 3, (k, e, tol[k])


def test_emulated_fp16_contract_of_the_plain_law_is_small():
    cfg = mo.tiny_config(mo.MODE_ENCODE_IMG)
    p16 = mo.round_fp16_weights(mo.init_params(cfg, SEED))
    x0 = torch.from_numpy(mo.synthetic_image(cfg))
    x = x0 + 0.5 * torch.from_numpy(philox.noise_batch(42, 0, 4, tuple(x0.shape)))
    errs = mo.stress_errors(mo.forward_all(p16, x, cfg, fp16_contract=True), mo.forward_all(p16, x, cfg))
    print("\nemulated fp16 contract, plain law:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["vit_out"] <= 1e-3 and errs["logits"] <= 1e-2
