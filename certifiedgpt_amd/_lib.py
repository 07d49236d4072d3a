"""ctypes binding of libcgpt.so (include/cgpt.h).  This is the stub a certifiedGPT maintainer would add
(INTEGRATION.md); there is no CPU fallback: a missing library is an ImportError, a missing GPU is a
CGPT_ERR_NO_DEVICE from cgpt_create."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CGPT_LIB_PATH") or os.path.join(_HERE, "libcgpt.so")   # CGPT_LIB_PATH: another build of the same ABI (A/B measurements)

CGPT_OK = 0
ERR_NAMES = {1: "CGPT_ERR_INVALID", 2: "CGPT_ERR_NO_DEVICE", 3: "CGPT_ERR_HIP", 4: "CGPT_ERR_NOT_FOUND", 5: "CGPT_ERR_STATE"}
MODE_VIT_HEAD = 0
MODE_ENCODE_IMG = 1
ABSTAIN = -1
NOISE_LAWS = {"gaussian": 0, "uniform": 1}   # CGPT_NOISE_GAUSSIAN, CGPT_NOISE_UNIFORM


class CgptError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


class Config(C.Structure):
    """struct cgpt_config (include/cgpt.h) -- field order is ABI."""
    _fields_ = [
        ("struct_size", C.c_int32), ("mode", C.c_int32), ("device", C.c_int32), ("num_classes", C.c_int32),
        ("max_batch", C.c_int32),
        ("img_size", C.c_int32), ("patch_size", C.c_int32), ("vit_dim", C.c_int32), ("vit_depth", C.c_int32),
        ("vit_heads", C.c_int32), ("vit_mlp", C.c_int32), ("vit_ln_eps", C.c_float), ("ln_vision_eps", C.c_float),
        ("qf_layers", C.c_int32), ("qf_dim", C.c_int32), ("qf_heads", C.c_int32), ("qf_ffn", C.c_int32),
        ("qf_queries", C.c_int32), ("qf_xattn_freq", C.c_int32), ("qf_ln_eps", C.c_float), ("proj_dim", C.c_int32),
    ]


class LlmConfig(C.Structure):
    """struct cgpt_llm_config (include/cgpt.h) -- field order is ABI."""
    _fields_ = [
        ("struct_size", C.c_int32), ("device", C.c_int32), ("hidden", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32),
        ("kv_heads", C.c_int32), ("head_dim", C.c_int32), ("mlp", C.c_int32), ("vocab", C.c_int32), ("rms_eps", C.c_float),
        ("rope_theta", C.c_float), ("max_batch", C.c_int32), ("max_len", C.c_int32), ("weight_format", C.c_int32),
    ]


class LlmConfigGqa(C.Structure):
    """struct cgpt_llm_config_gqa (include/cgpt.h): the config followed by the later switches.  base.struct_size = sizeof(this);
    cgpt_llm_create takes a pointer to `base`."""
    _fields_ = [("base", LlmConfig), ("grouped_kv", C.c_int32), ("reserved", C.c_int32)]


class LlmConfigAct(C.Structure):
    """struct cgpt_llm_config_act (include/cgpt.h): cgpt_llm_config_gqa followed by the activation format.  gqa.base.struct_size =
    sizeof(this); cgpt_llm_create takes a pointer to `gqa.base`."""
    _fields_ = [("gqa", LlmConfigGqa), ("act_format", C.c_int32), ("act_threshold", C.c_float), ("outlier_cap", C.c_int32),
                ("reserved2", C.c_int32)]


class LlmSampleParams(C.Structure):
    """struct cgpt_llm_sample_params (include/cgpt.h), passed BY VALUE to the sampling entries -- field order is ABI."""
    _fields_ = [("struct_size", C.c_int32), ("do_sample", C.c_int32), ("temperature", C.c_float), ("top_k", C.c_int32),
                ("top_p", C.c_float), ("repetition_penalty", C.c_float)]


def sample_params(do_sample, temperature, top_k, top_p, repetition_penalty):
    return LlmSampleParams(struct_size=C.sizeof(LlmSampleParams), do_sample=int(bool(do_sample)), temperature=float(temperature),
                           top_k=int(top_k), top_p=float(top_p), repetition_penalty=float(repetition_penalty))


LLM_ACT_FORMATS = {"fp16": 0, "int8": 1}      # CGPT_LLM_A_F16, CGPT_LLM_A_INT8
LLM_WEIGHT_FORMATS = {"fp16": 0, "int8": 1}   # CGPT_LLM_W_F16, CGPT_LLM_W_INT8
# sizeof(cgpt_llm_config) before weight_format existed: still accepted by cgpt_llm_create (fp16), and what older builds expect
LLM_CONFIG_SIZE_F16 = LlmConfig.weight_format.offset


# (name, restype, argtypes) of every symbol include/cgpt.h declares
_P, _I64, _I32, _F, _D, _U64 = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_double, C.c_uint64
SIGNATURES = {
    "cgpt_create": (_I32, [C.POINTER(Config), C.POINTER(_P)]),
    "cgpt_destroy": (_I32, [_P]),
    "cgpt_last_error": (C.c_char_p, []),
    "cgpt_version": (C.c_char_p, []),
    "cgpt_load_weight": (_I32, [_P, C.c_char_p, _P, _I64]),
    "cgpt_get_weight": (_I32, [_P, C.c_char_p, _P, _I64]),
    "cgpt_weight_numel": (_I64, [_P, C.c_char_p]),
    "cgpt_weight_name": (C.c_char_p, [_P, _I32]),
    "cgpt_init_synthetic_weights": (_I32, [_P, _U64, _P]),
    "cgpt_set_noise_law": (_I32, [_P, _I32]),
    "cgpt_sample_counts": (_I32, [_P, _P, _I64, _I64, _I64, _F, _U64, _P, _P]),
    "cgpt_sample_counts2": (_I32, [_P, _P, _I64, _I64, _P, _I64, _I64, _P, _I64, _F, _U64, _P]),
    "cgpt_sample_counts_images": (_I32, [_P, _P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _F, _U64, _P]),
    "cgpt_forward_logits": (_I32, [_P, _P, _I64, _I64, _F, _U64, _P, _P]),
    "cgpt_classify": (_I32, [_P, _P, _I64, _P, _P]),
    "cgpt_encode_img": (_I32, [_P, _P, _I64, _P, _P]),
    "cgpt_encode_img_noisy": (_I32, [_P, _P, _I64, _I64, _F, _U64, _P, _P]),
    "cgpt_get_activation": (_I32, [_P, C.c_char_p, _P, _I64, _P]),
    "cgpt_noise_batch": (_I32, [_P, _I64, _I64, _I64, _F, _U64, _P, _P]),
    "cgpt_noise_batch_law": (_I32, [_P, _I64, _I64, _I64, _F, _I32, _U64, _P, _P]),
    "cgpt_rgf_step": (_I32, [_P, _P, _I64, _I64, _I32, _P, _F, _F, _U64, _P, _P]),
    "cgpt_vote": (_I32, [_P, _I64, _I32, _P, _P]),
    "cgpt_vote_labels": (_I32, [_P, _I64, _I32, _P, _P]),
    "cgpt_allreduce_counts": (_I32, [_P, _P, _I64, _P]),
    "cgpt_allreduce_counts_fn": (_I32, [_P, _P, _P, _I64, _P]),
    "cgpt_certify_from_counts": (_I32, [_P, _P, _I32, _I64, _D, _D, C.POINTER(_I32), C.POINTER(_D)]),
    "cgpt_certify_many_from_counts": (_I32, [_P, _I64, _I32, _I64, _D, _D, _P, _P]),
    "cgpt_certify_many_from_counts_law": (_I32, [_P, _I64, _I32, _I64, _D, _D, _I32, _P, _P]),
    "cgpt_predict_from_counts": (_I32, [_P, _I32, _D, C.POINTER(_I32)]),
    "cgpt_certify_device": (_I32, [_P, _P, _I32, _I64, _D, _D, _P, _P]),
    "cgpt_certify_device_law": (_I32, [_P, _P, _I32, _I64, _D, _D, _I32, _P, _P]),
    "cgpt_predict_device": (_I32, [_P, _I32, _D, _P, _P]),
    "cgpt_lower_confidence_bound": (_D, [_I64, _I64, _D]),
    "cgpt_binom_test": (_D, [_I64, _I64, _D]),
    "cgpt_norm_ppf": (_D, [_D]),
    "cgpt_set_option": (_I32, [C.c_char_p, _I32]),
    "cgpt_mfma_sustained": (_I32, [_D, C.POINTER(_D), C.POINTER(_D)]),
    "cgpt_profile_enable": (_I32, [_P, _I32]),
    "cgpt_profile_read": (_I32, [_P, _I32, C.POINTER(_D), C.POINTER(_D), C.POINTER(_I64)]),
    "cgpt_profile_clock": (_I32, [_P, _I32, C.POINTER(_D)]),
    "cgpt_profile_batches": (_I32, [_P, C.POINTER(_I32), _I64, C.POINTER(_I64)]),
    "cgpt_gemm_f16": (_I32, [_P, _I64, _P, _I64, _P, _P, _I64, _I64, _I64, _I64, _P]),
    "cgpt_linear_f16": (_I32, [_P, _I64, _P, _I64, _P, _P, _I64, _P, _I64, _I64, _I64, _I64, _I32, _P]),
    "cgpt_attention_f16": (_I32, [_P, _I64, _P, _P, _I64, _P, _I64, _I32, _I32, _I32, _I32, _I32, _F, _P]),
    "cgpt_layernorm": (_I32, [_P, _I64, _P, _P, _F, _P, _I64, _P, _I64, _I64, _I32, _P]),
    "cgpt_layernorm_resid": (_I32, [_P, _I64, _P, _I64, _P, _I64, _I32, _P, _P, _F, _P, _I64, _P, _I64, _I64, _I32, _P]),
    "cgpt_llm_create": (_I32, [C.POINTER(LlmConfig), C.POINTER(_P)]),
    "cgpt_llm_destroy": (_I32, [_P]),
    "cgpt_llm_load_weight_f16": (_I32, [_P, C.c_char_p, _P, _I64, _P]),
    "cgpt_llm_weight_bytes": (_I32, [_P, C.POINTER(_I64)]),
    "cgpt_llm_step": (_I32, [_P, _P, _I32, _I32, _P, _P, _I64, _P, _P]),
    "cgpt_llm_greedy": (_I32, [_P, _P, _I32, _I32, _I32, _I32, _P, _I32, _I64, _P, _P, _I64, _P, _P, _P]),
    "cgpt_llm_prefill_reserve": (_I32, [_P, _I32, _I32]),
    "cgpt_llm_prefill": (_I32, [_P, _P, _I32, _I32, _P, _P, _I64, _P, _P]),
    "cgpt_llm_prefill_ragged": (_I32, [_P, _P, _I32, _I32, _P, _P, _P, _I64, _P, _P]),
    "cgpt_llm_prefill_from": (_I32, [_P, _P, _I32, _I32, _I32, _P, _P, _P, _I64, _P, _P]),
    "cgpt_llm_kv_broadcast": (_I32, [_P, _P, _P, _I64, _I32, _I32, _P, _P, _P, _I64, _P]),
    "cgpt_llm_step_ragged": (_I32, [_P, _P, _I32, _I32, _P, _P, _P, _I64, _P, _P]),
    "cgpt_llm_greedy_ragged": (_I32, [_P, _P, _I32, _I32, _P, _I32, _I32, _P, _I32, _I64, _P, _P, _I64, _P, _P, _P]),
    "cgpt_llm_set_early_stop": (_I32, [_P, _I32]),
    "cgpt_llm_live_steps": (_I32, [_P, C.POINTER(_I32), _P]),
    "cgpt_llm_set_stop_sequences": (_I32, [_P, C.POINTER(_I64), C.POINTER(_I32), _I32]),
    "cgpt_llm_score_reserve": (_I32, [_P, _I32, _I32]),
    "cgpt_llm_act_stats": (_I32, [_P, C.POINTER(_I64)]),
    "cgpt_llm_linear_i8": (_I32, [_P, _P, _P, _I64, _I64, _I64, _F, _I32, _I32, _P, _P, _I64, _P, _I64, _P]),
    "cgpt_llm_linear_i8_workspace": (_I64, [_I64, _I64, _I64, _I32, C.POINTER(_I64)]),
    "cgpt_llm_linear_i8_slices": (_I32, [_I64, _I64]),
    "cgpt_llm_score": (_I32, [_P, _P, _I32, _I32, _P, _P, _I32, _I32, _F, _P, _P, _I64, _P, _P]),
    "cgpt_llm_score_ragged": (_I32, [_P, _P, _I32, _I32, _P, _P, _P, _P, _I32, _I32, _F, _P, _P, _I64, _P, _P]),
    "cgpt_llm_sample": (_I32, [_P, _P, _I32, _I32, _I32, _I32, _P, _I32, _I64, _P, _P, _I64, _P, _P, LlmSampleParams, _P, _P, _P]),
    "cgpt_llm_sample_ragged": (_I32, [_P, _P, _I32, _I32, _P, _I32, _I32, _P, _I32, _I64, _P, _P, _I64, _P, _P, LlmSampleParams, _P, _P,
                                      _P]),
    "cgpt_llm_sample_logits": (_I32, [_P, _I64, _I32, _I32, _P, _I64, _I32, _I32, _I32, _P, _I32, _I64, _P, LlmSampleParams, _P, _P, _P,
                                      _P, _P, _P, _P, _P]),
    "cgpt_llm_trie_check": (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, C.POINTER(_I32)]),
    "cgpt_llm_set_trie": (_I32, [_P, _P, _P, _P, _P, _I32, _I32]),
    "cgpt_llm_constrained": (_I32, [_P, _P, _I32, _I32, _I32, _I64, _P, _P, _I64, _P, _P, _P, _P]),
    "cgpt_llm_constrained_ragged": (_I32, [_P, _P, _I32, _I32, _P, _I32, _I64, _P, _P, _I64, _P, _P, _P, _P]),
    "cgpt_llm_trie_select_logits": (_I32, [_P, _I64, _I32, _I32, _P, _P, _P, _P, _I32, _I64, _P, _P, _P, _P, _P]),
    "cgpt_llm_beam_reserve": (_I32, [_P, _I32, _I32, _I32]),
    "cgpt_llm_beam_step": (_I32, [_P, _P, _I32, _I32, _I32, _I32, _P, _I64, _P, _P, _I64, _P, _P, _I64, _P, _P]),
    "cgpt_llm_beam_select_logits": (_I32, [_P, _I64, _I32, _I32, _I32, _I32, _I32, _I32, _P, _I32, _I64, _F] + [_P] * 18 + [_P]),
    "cgpt_llm_beam": (_I32, [_P, _P, _I32, _I32, _I32, _I32, _I32, _P, _I32, _I64, _F, _P, _P, _I64, _P, _P, _I64, _P, _P, _P, _P, _P]),
}

_lib = None


def lib():
    """Load libcgpt.so once.  Raises ImportError (loudly) when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()' or make -C certifiedgpt_amd/csrc). "
                "certifiedgpt_amd has no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def noise_law(law):
    """"gaussian" | "uniform" -> CGPT_NOISE_* (ValueError for anything else)."""
    if law not in NOISE_LAWS:
        raise ValueError(f"unknown noise law {law!r}: expected one of {sorted(NOISE_LAWS)}")
    return NOISE_LAWS[law]


def check(status):
    if status != CGPT_OK:
        raise CgptError(status, lib().cgpt_last_error().decode())
