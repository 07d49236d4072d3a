"""ORACLE (test infrastructure) -- fp32 PyTorch-CPU restatement of the base classifier the reference's
`Smooth` would wrap: EVA-ViT-G forward_features, ln_vision, Q-Former query path, llama_proj
(MiniGPT4.encode_img, graphs/models/minigpt4/models/minigpt4.py:121-149) plus the build-side label head.

Parameters are a flat dict {reference state_dict name: torch.float32 tensor}.  Pinned against the reference's
own classes by tests/golden/model_golden.npz (oracle/gen_golden_model.py; tests/test_oracle_model.py).

CPU semantics: on a CPU device the reference runs without autocast (base_model.py:135-136), i.e. fp32
arithmetic; the HIP path uses fp16 operands with fp32 accumulation (the reference's `cuda` autocast
contract, base_model.py:141-142, eva_vit.py:407-414), so GPU-vs-oracle comparisons carry a tolerance.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from . import philox

MODE_VIT_HEAD = 0
MODE_ENCODE_IMG = 1


@dataclass
class Config:
    """Mirror of cgpt_config (include/cgpt.h).  Defaults = create_eva_vit_g (eva_vit.py:425-438) and
    init_Qformer (minigpt4.py:90-119, BERT-base)."""
    mode: int = MODE_VIT_HEAD
    num_classes: int = 1000
    img_size: int = 224
    patch_size: int = 14
    vit_dim: int = 1408
    vit_depth: int = 39
    vit_heads: int = 16
    vit_mlp: int = 6144            # int(1408 * 4.3637)
    vit_ln_eps: float = 1e-6
    ln_vision_eps: float = 1e-5
    qf_layers: int = 12
    qf_dim: int = 768
    qf_heads: int = 12
    qf_ffn: int = 3072
    qf_queries: int = 32
    qf_xattn_freq: int = 2
    qf_ln_eps: float = 1e-12
    proj_dim: int = 4096

    @property
    def tokens(self):
        return (self.img_size // self.patch_size) ** 2 + 1


def tiny_config(mode=MODE_VIT_HEAD, num_classes=10):
    """Small shape used by fixtures/tests: 2 ViT heads of 88, 2 Q-Former heads of 64."""
    return Config(mode=mode, num_classes=num_classes, img_size=56, patch_size=14, vit_dim=176, vit_depth=2,
                  vit_heads=2, vit_mlp=int(176 * 4.3637), qf_layers=2, qf_dim=128, qf_heads=2, qf_ffn=256,
                  qf_queries=8, qf_xattn_freq=2, proj_dim=192)


# --------------------------------------------------------------------------------------- parameters
def param_shapes(cfg: Config):
    """Ordered {name: shape} of every tensor the classifier uses (reference state_dict names)."""
    D, P = cfg.vit_dim, cfg.patch_size
    s = {}
    s["visual_encoder.cls_token"] = (1, 1, D)                                   # eva_vit.py:270
    s["visual_encoder.pos_embed"] = (1, cfg.tokens, D)                          # :272
    s["visual_encoder.patch_embed.proj.weight"] = (D, 3, P, P)                  # :202
    s["visual_encoder.patch_embed.proj.bias"] = (D,)
    for i in range(cfg.vit_depth):
        b = f"visual_encoder.blocks.{i}."
        s[b + "norm1.weight"] = (D,); s[b + "norm1.bias"] = (D,)                # :162
        s[b + "attn.q_bias"] = (D,); s[b + "attn.v_bias"] = (D,)                # :83-84
        s[b + "attn.qkv.weight"] = (3 * D, D)                                   # :81
        s[b + "attn.proj.weight"] = (D, D); s[b + "attn.proj.bias"] = (D,)      # :120
        s[b + "norm2.weight"] = (D,); s[b + "norm2.bias"] = (D,)                # :168
        s[b + "mlp.fc1.weight"] = (cfg.vit_mlp, D); s[b + "mlp.fc1.bias"] = (cfg.vit_mlp,)   # :54
        s[b + "mlp.fc2.weight"] = (D, cfg.vit_mlp); s[b + "mlp.fc2.bias"] = (D,)             # :56
    s["ln_vision.weight"] = (D,); s["ln_vision.bias"] = (D,)                    # base_model.py:281
    if cfg.mode == MODE_ENCODE_IMG:
        H = cfg.qf_dim
        s["query_tokens"] = (1, cfg.qf_queries, H)                              # minigpt4.py:99
        s["Qformer.bert.embeddings.LayerNorm.weight"] = (H,)                    # Qformer.py:65
        s["Qformer.bert.embeddings.LayerNorm.bias"] = (H,)
        for i in range(cfg.qf_layers):
            L = f"Qformer.bert.encoder.layer.{i}."
            atts = ["attention"] + (["crossattention"] if i % cfg.qf_xattn_freq == 0 else [])
            for att in atts:
                kv_in = cfg.vit_dim if att == "crossattention" else H           # Qformer.py:127-129
                s[L + att + ".self.query.weight"] = (H, H); s[L + att + ".self.query.bias"] = (H,)
                s[L + att + ".self.key.weight"] = (H, kv_in); s[L + att + ".self.key.bias"] = (H,)
                s[L + att + ".self.value.weight"] = (H, kv_in); s[L + att + ".self.value.bias"] = (H,)
                s[L + att + ".output.dense.weight"] = (H, H); s[L + att + ".output.dense.bias"] = (H,)
                s[L + att + ".output.LayerNorm.weight"] = (H,); s[L + att + ".output.LayerNorm.bias"] = (H,)
            s[L + "intermediate_query.dense.weight"] = (cfg.qf_ffn, H)          # Qformer.py:399
            s[L + "intermediate_query.dense.bias"] = (cfg.qf_ffn,)
            s[L + "output_query.dense.weight"] = (H, cfg.qf_ffn)                # :400
            s[L + "output_query.dense.bias"] = (H,)
            s[L + "output_query.LayerNorm.weight"] = (H,); s[L + "output_query.LayerNorm.bias"] = (H,)
        s["llama_proj.weight"] = (cfg.proj_dim, H); s["llama_proj.bias"] = (cfg.proj_dim,)   # minigpt4.py:76
        s["head.weight"] = (cfg.num_classes, cfg.proj_dim)
    else:
        s["head.weight"] = (cfg.num_classes, D)
    s["head.bias"] = (cfg.num_classes,)
    return s


def init_params(cfg: Config, seed: int, randomize_affine: bool = True):
    """Seeded parameters following the reference init law: Linear/Conv weights ~ N(0, .02) (trunc at +-2
    never binds: eva_vit.py:316-318, Qformer.py:664-674), proj/fc2 weights / sqrt(2*layer_id)
    (eva_vit.py:308-314), query_tokens ~ N(0,.02) (minigpt4.py:99-102).  With randomize_affine the
    biases / LayerNorm affine parameters get small random values instead of the (0 / 1) init so that every
    term of the forward is exercised by parity tests.  Draws come from the counter-based stream
    (oracle/philox.py) with stream id = index of the tensor, so the table is stable forever."""
    out = {}
    for tid, (name, shape) in enumerate(param_shapes(cfg).items()):
        n = int(np.prod(shape))
        z = philox.normal_stream(seed, tid, n, hi_word=1).reshape(shape)
        if name.endswith("norm1.weight") or name.endswith("norm2.weight") or name.endswith("LayerNorm.weight") \
                or name == "ln_vision.weight":
            w = 1.0 + (0.1 * z if randomize_affine else 0.0 * z)
        elif name.endswith("bias") or name.endswith("q_bias") or name.endswith("v_bias"):
            w = (0.02 * z) if randomize_affine else 0.0 * z
        else:
            w = 0.02 * z
            if name.startswith("head."):
                w = 0.05 * z   # build-side head: spread the logits so that argmax is not a near-tie
            for key in ("attn.proj.weight", "mlp.fc2.weight"):
                if name.endswith(key):
                    layer_id = int(name.split(".")[2]) + 1
                    w = w / math.sqrt(2.0 * layer_id)
        out[name] = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32))
    return out


def round_fp16_weights(params):
    """What the device computes with: matrices (GEMM operands) rounded through fp16
    (convert_weights_to_fp16, eva_vit.py:407-414); 1-D parameters (biases, LayerNorm affine) and
    cls_token / pos_embed / query_tokens stay fp32.  Mirrors cgpt_load_weight (include/cgpt.h)."""
    out = {}
    for k, v in params.items():
        is_mat = v.dim() >= 2 and not (k.endswith("cls_token") or k.endswith("pos_embed") or k == "query_tokens")
        out[k] = v.half().float() if is_mat else v.clone()
    return out


# ----------------------------------------------------------------------------- stress law (trained-like)
STRESS_OUTLIER_CHANNELS = (3, 61, 97, 170)      # fixed residual channels made 10-100x the rest (all < the tiny width 176)
STRESS_ROW_OFFSET = 64.0                        # added to patch_embed.proj.bias: every token row's mean sits >= 3 sigma off zero


def stress_config(mode=MODE_VIT_HEAD, img_size=56, num_classes=10, **over):
    """The tiny widths of tiny_config with three ViT blocks and four Q-Former layers, so that the two cross-attention
    layers (0 and 2) read different K/V slices of the device's shared kv_all buffer.  `over` replaces fields (e.g. the
    full ViT-G width)."""
    import dataclasses
    cfg = dataclasses.replace(tiny_config(mode=mode, num_classes=num_classes), img_size=img_size, vit_depth=3, qf_layers=4)
    return dataclasses.replace(cfg, **over)


# logit gain g = g_q * g_k per attention kind at the tiny widths (vit_dim 176, qf_dim 128), and the power of 176 / vit_dim
# it scales with; ViT blocks after the first see the outlier channels, which inflate the row's sigma and so shrink every other
# channel of the LayerNorm output (logit std ~ width^2 / outlier^2 there instead of ~ width)
STRESS_LOGIT_GAIN = {"vit_first": (32.0, 1), "vit_later": (512.0, 2), "qf_self": (64.0, 0), "qf_cross": (64.0, 1)}


def _split_gain(g):
    e = round(math.log2(g))
    return 2.0 ** ((e + 1) // 2), 2.0 ** (e // 2)          # (g_q, g_k), g_q * g_k = g


def stress_params(params, cfg: Config, outlier=32.0, row_offset=STRESS_ROW_OFFSET):
    """Trained-like statistics (peaked attention, outlier channels, rows far off zero) from init_params output, by a fixed
    transform with power-of-two factors (the fp16 rounding of a scaled matrix is the scaled rounding).  Returns a new dict.

    Peaked attention: random-init attention logits have std ~ 0.0004 * width (0.07 at width 176: every softmax is almost
      uniform).  The q rows and k rows of every ViT `attn.qkv.weight` (+ `q_bias`) and the `query` / `key` weights and biases
      of every Q-Former self- and cross-attention are multiplied by g_q and g_k, g_q * g_k = STRESS_LOGIT_GAIN[kind] scaled
      by (176 / vit_dim)^power and rounded to a power of two, g_q = g_k or 2 g_k.  At the stress config that puts the logit
      std at ~1.5-6 and the median max probability of every attention kind at ~0.2-0.8 (tests/test_oracle_stress.py):
      peaked, not one-hot.
    Outlier channels: output channels STRESS_OUTLIER_CHANNELS of every `attn.proj` / `mlp.fc2` get their weight row scaled by
      outlier / 4 and their bias set to sign * outlier / 2 (signs +, -, +, +): the residual stream grows by ~outlier per
      block in those channels (|x| ~ 1e2 after three blocks at outlier = 32) while the other channels stay O(1) about the
      row offset.
    LayerNorm compensation: `ln_vision.weight` x 2^round(log2(outlier / 2)) outside the outlier channels, / 4 on them, so that
      image_embeds is O(1) in every channel (trained weights compensate their outliers the same way); without it every
      cross-attention V row would be the same outlier vector and the cross-attention would not matter.
    Row offset: `patch_embed.proj.bias` and `cls_token` += row_offset: with the outliers, every token row's mean is
      >= 3 times its standard deviation -- the cancellation each LayerNorm has to survive."""
    out = {k: v.clone() for k, v in params.items()}
    D = cfg.vit_dim

    def gains(kind):
        g, power = STRESS_LOGIT_GAIN[kind]
        return _split_gain(g * (176.0 / D) ** power)

    for i in range(cfg.vit_depth):
        gq, gk = gains("vit_first" if i == 0 else "vit_later")
        b = f"visual_encoder.blocks.{i}."
        w = out[b + "attn.qkv.weight"]
        w[:D] *= gq
        w[D:2 * D] *= gk
        out[b + "attn.q_bias"] *= gq
    if cfg.mode == MODE_ENCODE_IMG:
        for i in range(cfg.qf_layers):
            L = f"Qformer.bert.encoder.layer.{i}."
            atts = ["attention"] + (["crossattention"] if i % cfg.qf_xattn_freq == 0 else [])
            for att in atts:
                gq, gk = gains("qf_cross" if att == "crossattention" else "qf_self")
                for name, g in (("query", gq), ("key", gk)):
                    out[f"{L}{att}.self.{name}.weight"] *= g
                    out[f"{L}{att}.self.{name}.bias"] *= g
    chans = [c for c in STRESS_OUTLIER_CHANNELS if c < D]
    signs = [1.0, -1.0, 1.0, 1.0]
    for i in range(cfg.vit_depth):
        b = f"visual_encoder.blocks.{i}."
        for key in ("attn.proj", "mlp.fc2"):
            for c, s in zip(chans, signs):
                out[b + key + ".weight"][c] *= outlier / 4.0
                out[b + key + ".bias"][c] = s * outlier / 2.0
    # ln_vision's affine weight compensates the outliers the way trained weights do: other channels x outlier / 2, outlier channels
    # / 4, so image_embeds (the cross-attention K/V input) is O(1) in every channel instead of ~0.07 beside ~6
    lnv = out["ln_vision.weight"]
    keep = lnv[chans].clone()
    lnv *= 2.0 ** round(math.log2(outlier / 2.0))
    lnv[chans] = keep / 4.0
    out["visual_encoder.patch_embed.proj.bias"] += row_offset
    out["visual_encoder.cls_token"] += row_offset
    return out


# Stage tolerances of the GPU stress tests (tests/test_gpu_stress.py): max |device - fp32 oracle| / max |oracle| per stage;
# "vit_out_chan" is the per-channel metric stress_errors computes.  tests/test_oracle_stress.py holds them to >= 3x the
# emulated fp16-contract error and to <= 1/10 of what each named wiring perturbation moves its stage by.
STRESS_TOL = {"vit_out": 2e-3, "vit_out_chan": 3e-3, "ln_vision": 3e-3, "qformer": 1e-3, "llama": 3e-3, "logits": 3e-3}
# at the full ViT width (1408) the Q-Former reads a 1408-wide fp16 kv_all: its emulated contract error is ~1e-3
STRESS_TOL_FULL_WIDTH = dict(STRESS_TOL, qformer=3e-3, llama=4e-3)


def channel_err(got, ref, skip=()):
    """max over channels (except `skip`) of (column max |got - ref|) / (column max |ref - column mean|): the row offset
    dominates every column's max|ref|, so each channel is judged against its own spread.  The stress tests skip the outlier
    channels: they dominate max|ref| of the whole tensor, which is what the plain metric judges them by."""
    got = torch.as_tensor(got).float().cpu().reshape(-1, ref.shape[-1])
    ref = torch.as_tensor(ref).float().cpu().reshape(-1, ref.shape[-1])
    keep = [c for c in range(ref.shape[-1]) if c not in set(skip)]
    got, ref = got[:, keep], ref[:, keep]
    spread = (ref - ref.mean(dim=0)).abs().amax(dim=0).clamp_min(1e-6)
    return float(((got - ref).abs().amax(dim=0) / spread).max())


def stress_errors(got, ref):
    """{stage: error} for every stage both dicts hold, in the metric of STRESS_TOL (+ "vit_out_chan")."""
    out = {}
    for k in ("vit_out", "ln_vision", "qformer", "llama", "logits"):
        if k in got and k in ref:
            g, r = torch.as_tensor(got[k]).float().cpu(), torch.as_tensor(ref[k]).float().cpu()
            out[k] = float((g - r).abs().max() / r.abs().max().clamp_min(1e-6))
    if "vit_out" in got and "vit_out" in ref:
        out["vit_out_chan"] = channel_err(got["vit_out"], ref["vit_out"], STRESS_OUTLIER_CHANNELS)
    return out


# ------------------------------------------------------------------------------------------ forward
def _identity(t, name=None):
    return t


def _fp16_store(probe):
    """r(t, name): t rounded through fp16 (an fp16 store of the device path); records max|t| per store in probe["fp16_max"]."""
    def r(t, name):
        if probe is not None:
            d = probe.setdefault("fp16_max", {})
            d[name] = max(d.get(name, 0.0), float(t.abs().max()))
        return t.half().float()
    return r


def _softmax_attention(q, k, v, scale, r, probe, kind):
    """softmax(q k^T * scale) v over the last two dims (kind "vit": q is scaled first; Q-Former kinds: the scores are divided by
    `scale` = sqrt(head_dim)).  Under the fp16 contract (r != _identity) the probabilities enter the
    PV product as fp16 values and the output is stored as fp16 (the device's P and O); the normaliser stays fp32."""
    s = (q * scale) @ k.transpose(-2, -1) if kind == "vit" else (q @ k.transpose(-2, -1)) / scale   # eva_vit.py:131 / Qformer.py:244
    if probe is not None:
        a = probe.setdefault("attn", {}).setdefault(kind, {"logit_std": [], "max_prob": []})
        sd = s.double()
        a["logit_std"].append(float(sd.std(dim=-1).median()))
        a["max_prob"].append(float(sd.softmax(dim=-1).max(dim=-1).values.median()))
    if r is _identity:
        return s.softmax(dim=-1) @ v
    e = (s - s.amax(dim=-1, keepdim=True)).exp()
    return r((r(e, "attn_p") @ v) / e.sum(dim=-1, keepdim=True), "attn_o")


def vit_forward(p, x, cfg: Config, r=_identity, probe=None):
    """VisionTransformer.forward_features (eva_vit.py:332-349): [B,3,H,W] -> [B,T,D]; no final norm.
    r = _identity: fp32 throughout; otherwise the fp16 stores of the device path (forward_all(fp16_contract=True))."""
    pre = "visual_encoder."
    B = x.shape[0]
    D, Hh = cfg.vit_dim, cfg.vit_heads
    if r is not _identity:
        x = r(x, "im2col")
    h = F.conv2d(x, p[pre + "patch_embed.proj.weight"], p[pre + "patch_embed.proj.bias"], stride=cfg.patch_size)
    h = h.flatten(2).transpose(1, 2)                                            # :209
    h = torch.cat((p[pre + "cls_token"].expand(B, -1, -1), h), dim=1)           # :337-338
    h = h + p[pre + "pos_embed"]                                                # :340
    scale = (D // Hh) ** -0.5                                                   # :79
    for i in range(cfg.vit_depth):
        b = f"{pre}blocks.{i}."
        y = r(F.layer_norm(h, (D,), p[b + "norm1.weight"], p[b + "norm1.bias"], cfg.vit_ln_eps), "xn")
        qkv_bias = torch.cat((p[b + "attn.q_bias"], torch.zeros_like(p[b + "attn.v_bias"]), p[b + "attn.v_bias"]))  # :127
        qkv = r(F.linear(y, p[b + "attn.qkv.weight"], qkv_bias), "qkv")         # :129
        qkv = qkv.reshape(B, -1, 3, Hh, D // Hh).permute(2, 0, 3, 1, 4)         # :130
        q, k, v = qkv[0], qkv[1], qkv[2]                                        # :131-133
        y = _softmax_attention(q, k, v, scale, r, probe, "vit")                 # :134,147
        y = y.transpose(1, 2).reshape(B, -1, D)                                 # :150
        h = h + r(F.linear(y, p[b + "attn.proj.weight"], p[b + "attn.proj.bias"]), "proj")   # :151,180
        y = r(F.layer_norm(h, (D,), p[b + "norm2.weight"], p[b + "norm2.bias"], cfg.vit_ln_eps), "xn")
        y = r(F.gelu(F.linear(y, p[b + "mlp.fc1.weight"], p[b + "mlp.fc1.bias"])), "gelu_hidden")  # :60-61 exact-erf GELU
        h = h + r(F.linear(y, p[b + "mlp.fc2.weight"], p[b + "mlp.fc2.bias"]), "fc2")           # :64,181
    return h


def _bert_attention(p, prefix, hidden, kv_src, cfg: Config, r=_identity, probe=None, kind="qf_self", name="qqkv"):
    """BertAttention = BertSelfAttention (Qformer.py:169-275) + BertSelfOutput (:278-289); all masks are 0.
    Under the fp16 contract the GEMMs read the fp16 copy of `hidden` while the residual add reads the fp32 one."""
    B, Tq, H = hidden.shape
    nh, hd = cfg.qf_heads, cfg.qf_dim // cfg.qf_heads
    h16 = hidden if r is _identity else r(hidden, "qh16")
    if kind == "qf_self":
        kv_src = h16
    q = r(F.linear(h16, p[prefix + ".self.query.weight"], p[prefix + ".self.query.bias"]), name)
    k = r(F.linear(kv_src, p[prefix + ".self.key.weight"], p[prefix + ".self.key.bias"]), "kv_all" if kind == "qf_cross" else name)
    v = r(F.linear(kv_src, p[prefix + ".self.value.weight"], p[prefix + ".self.value.bias"]), "kv_all" if kind == "qf_cross" else name)
    q = q.view(B, Tq, nh, hd).permute(0, 2, 1, 3)
    k = k.view(B, -1, nh, hd).permute(0, 2, 1, 3)
    v = v.view(B, -1, nh, hd).permute(0, 2, 1, 3)
    ctx = _softmax_attention(q, k, v, math.sqrt(hd), r, probe, kind)           # :244,250-266
    ctx = ctx.permute(0, 2, 1, 3).reshape(B, Tq, H)
    if r is not _identity:
        ctx = r(ctx, "qctx")
    o = F.linear(ctx, p[prefix + ".output.dense.weight"], p[prefix + ".output.dense.bias"])
    return F.layer_norm(o + hidden, (H,), p[prefix + ".output.LayerNorm.weight"],
                        p[prefix + ".output.LayerNorm.bias"], cfg.qf_ln_eps)    # :288


def qformer_forward(p, image_embeds, cfg: Config, r=_identity, probe=None):
    """Qformer.bert(query_embeds=query_tokens, encoder_hidden_states=image_embeds) query path
    (minigpt4.py:132-139; Qformer.py:78-108 embeddings, :402-484 layers) -> last_hidden_state [B,Q,H]."""
    B = image_embeds.shape[0]
    H = cfg.qf_dim
    h = p["query_tokens"].expand(B, -1, -1)
    h = F.layer_norm(h, (H,), p["Qformer.bert.embeddings.LayerNorm.weight"],
                     p["Qformer.bert.embeddings.LayerNorm.bias"], cfg.qf_ln_eps)  # :106
    for i in range(cfg.qf_layers):
        L = f"Qformer.bert.encoder.layer.{i}."
        h = _bert_attention(p, L + "attention", h, h, cfg, r, probe, "qf_self", "qqkv")               # :415-421
        if i % cfg.qf_xattn_freq == 0:                                          # :386-395,432-441
            h = _bert_attention(p, L + "crossattention", h, image_embeds, cfg, r, probe, "qf_cross", "qq")
        h16 = h if r is _identity else r(h, "qh16")
        y = r(F.gelu(F.linear(h16, p[L + "intermediate_query.dense.weight"], p[L + "intermediate_query.dense.bias"])), "qff")  # :481
        y = F.linear(y, p[L + "output_query.dense.weight"], p[L + "output_query.dense.bias"])
        h = F.layer_norm(y + h, (H,), p[L + "output_query.LayerNorm.weight"],
                         p[L + "output_query.LayerNorm.bias"], cfg.qf_ln_eps)   # :483, :372
    return h


def forward_all(p, x, cfg: Config, fp16_contract=False, probe=None):
    """Returns dict of stages: vit_out, ln_vision (CLS row only in MODE_VIT_HEAD), qformer, llama, logits.

    fp16_contract=True rounds to fp16 wherever the device path stores fp16 (certifiedgpt_amd/csrc/model.hip `forward`):
    the im2col operand, LayerNorm outputs, qkv, attention P and O, the proj / fc2 outputs, the GELU hidden, the Q-Former
    qqkv / qq / qctx / qff, kv_all, the pooled head input; the residual streams stay fp32.  CPU tests use it to predict
    the device's error before a GPU run (tests/test_oracle_stress.py).  probe (a dict) collects the largest value passing
    through each fp16 store (probe["fp16_max"], recorded with or without the rounding) and per attention kind the median
    logit std / max probability of every launch (probe["attn"])."""
    if fp16_contract:
        r = _fp16_store(probe)
    elif probe is not None:
        rec = _fp16_store(probe)

        def r(t, name):
            rec(t, name)
            return t
    else:
        r = _identity
    with torch.no_grad():
        x = torch.as_tensor(x, dtype=torch.float32)
        out = {}
        vit = vit_forward(p, x, cfg, r, probe)
        out["vit_out"] = vit
        D = cfg.vit_dim
        if cfg.mode == MODE_VIT_HEAD:
            cls = r(F.layer_norm(vit[:, 0], (D,), p["ln_vision.weight"], p["ln_vision.bias"], cfg.ln_vision_eps), "emb")
            out["logits"] = F.linear(cls, p["head.weight"], p["head.bias"])
            return out
        emb = r(F.layer_norm(vit, (D,), p["ln_vision.weight"], p["ln_vision.bias"], cfg.ln_vision_eps), "emb")  # minigpt4.py:129
        out["ln_vision"] = emb
        qf = qformer_forward(p, emb, cfg, r, probe)
        out["qformer"] = qf
        llama = F.linear(r(qf, "qh16"), p["llama_proj.weight"], p["llama_proj.bias"])      # minigpt4.py:141
        out["llama"] = llama
        out["logits"] = F.linear(r(llama.mean(dim=1), "pooled"), p["head.weight"], p["head.bias"])
        return out


def interpolate_pos_embed(pos_embed_checkpoint, num_patches):
    """eva_vit.py:383-404 restated: keep the extra (class) token, bicubic-resize the square grid of patch tokens."""
    pe = torch.as_tensor(pos_embed_checkpoint, dtype=torch.float32)
    embedding_size = pe.shape[-1]
    num_extra_tokens = 1                                               # model.pos_embed.shape[-2] - num_patches (:388)
    orig_size = int((pe.shape[-2] - num_extra_tokens) ** 0.5)          # :390
    new_size = int(num_patches ** 0.5)                                 # :392
    if orig_size == new_size:
        return pe
    extra_tokens = pe[:, :num_extra_tokens]
    pos_tokens = pe[:, num_extra_tokens:]
    pos_tokens = pos_tokens.reshape(-1, orig_size, orig_size, embedding_size).permute(0, 3, 1, 2)
    pos_tokens = F.interpolate(pos_tokens, size=(new_size, new_size), mode="bicubic", align_corners=False)   # :400-401
    pos_tokens = pos_tokens.permute(0, 2, 3, 1).flatten(1, 2)
    return torch.cat((extra_tokens, pos_tokens), dim=1)                # :403


def make_classifier(p, cfg: Config):
    """base_classifier([B,C,H,W] float32) -> logits [B,num_classes] numpy, for SmoothOracle."""
    def f(batch):
        return forward_all(p, batch, cfg)["logits"].numpy()
    return f


def synthetic_image(cfg: Config, seed: int = 1234):
    """x = (u - mean)/std, u ~ U[0,1)^{3xHxW}, CLIP statistics
    (processors/base_processor.py:18-20).  u comes from the Philox words (24-bit uniforms)."""
    n = 3 * cfg.img_size * cfg.img_size
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    r = philox.philox4x32_10(g, np.uint64(2), np.uint64(0), np.uint64(0), seed & 0xFFFFFFFF, seed >> 32)
    u = (np.stack(r, axis=1).reshape(-1)[:n] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    u = u.reshape(3, cfg.img_size, cfg.img_size)
    mean = np.array([0.48145466, 0.4578275, 0.40821073], dtype=np.float32)[:, None, None]
    std = np.array([0.26862954, 0.26130258, 0.27577711], dtype=np.float32)[:, None, None]
    return ((u - mean) / std).astype(np.float32)
