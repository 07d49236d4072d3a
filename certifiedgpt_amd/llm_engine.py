"""The ctypes binding of the native LLaMA engine (`cgpt_llm_*`, include/cgpt.h; csrc/llm*.hip): which decoders it takes
(`hip_decode_unsupported`), the handle with its entries (`_HipDecoder`), and the route of a decoder's own linears through the
library's GEMM (`_LinearRoute`).  What the entries are specified to compute is stated in llm_laws.py; who calls them, and when, is
minigpt4.py's `MiniGPT4Classifier`.
"""
import torch

from .llm_laws import GQA_RATIOS, check_sample_settings, check_stop_words_ids


class _LinearRoute:
    """Routes the bias-free fp16 `nn.Linear` layers of a frozen decoder through libcgpt's MFMA GEMM (`cgpt_linear_f16`, the kernel
    of the ViT's qkv / proj / MLP) for calls with at least `min_rows` rows, i.e. the PREFILL of a Monte-Carlo batch (200 rows x 44
    tokens = 8 800 rows); decode steps (one row per copy) stay with the vendor library.  One patch per module; the patch is inert
    outside `enabled()`, and the switch is a context variable (per thread / per task), so another thread or another classifier that
    calls the same shared decoder meanwhile is not routed.  Eligibility (fp16, contiguous, on the device, no bias, K in 64s, N in 256s)
    is re-checked at every call: after a `.to()`, a dtype change or a weight swap (a LoRA merge) the original forward runs."""
    import contextvars as _cv
    _active = _cv.ContextVar("cgpt_linear_route", default=False)

    @staticmethod
    def _eligible(m):
        w = m.weight
        return (m.bias is None and w.dtype == torch.float16 and w.is_cuda and w.is_contiguous()
                and w.shape == (m.out_features, m.in_features) and m.in_features % 64 == 0 and m.out_features % 256 == 0)

    @classmethod
    def install(cls, model, min_rows=1024):
        import ctypes as C
        from . import _lib
        L = _lib.lib()
        n = 0
        for m in model.modules():
            if not isinstance(m, torch.nn.Linear):
                continue
            if getattr(m, "_cgpt_routed", False):                       # patched by an earlier classifier on the same module
                n += 1
                continue
            if not cls._eligible(m):                                    # W must be readable for whole 256-row tiles, K in 64s
                continue
            orig = m.forward

            def fwd(x, m=m, orig=orig):
                rows = x.numel() // x.shape[-1] if x.shape[-1] else 0
                if (not cls._active.get() or rows < min_rows or x.dtype != torch.float16 or not x.is_cuda
                        or x.device != m.weight.device or not cls._eligible(m)):
                    return orig(x)
                K, N = m.in_features, m.out_features
                a = x.reshape(rows, K)
                if rows % 256 or not a.is_contiguous():                 # the kernel reads whole 256-row tiles: pad rows exist but are
                    pad = x.new_empty(((rows + 255) // 256 * 256, K))   # never stored from (their garbage stays in their own outputs)
                    pad[:rows].copy_(a)
                    a = pad
                out = x.new_empty((rows, N))
                st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                _lib.check(L.cgpt_linear_f16(C.c_void_p(a.data_ptr()), K, C.c_void_p(m.weight.data_ptr()), K, None,
                                             C.c_void_p(out.data_ptr()), N, None, N, rows, N, K, 0, st))
                return out.view(*x.shape[:-1], N)
            m.forward = fwd
            m._cgpt_routed = True
            n += 1
        return n

    @classmethod
    def enabled(cls):
        import contextlib

        @contextlib.contextmanager
        def ctx():
            token = cls._active.set(True)
            try:
                yield
            finally:
                cls._active.reset(token)
        return ctx()


def hip_decode_unsupported(llama_model, max_batch=None, grouped_kv=False, activations="fp16"):
    """Every property of `llama_model` (and of the classifier batch) that keeps it off the native token step (`decode="hip"`,
    csrc/llm.hip, csrc/llm_step.hip), as a list of sentences; empty = supported.  The step kernels are written for HF `LlamaForCausalLM` in fp16 on
    a HIP device: bias-free linears, RMSNorm, `rotate_half` rotary with the default (unscaled) rope_theta law, as many K/V heads
    as query heads, head size 128, SwiGLU, no sliding window -- Vicuna-7B / 13B.  ALL failing properties are collected, so one
    message names them all.
    grouped_kv=True (the engine's grouped-query mode): fewer K/V heads than query heads are accepted when they
    divide them and heads / kv_heads is 1, 2, 4 or 8 -- Llama-3-8B (32 / 8), Llama-2-70B's shape (64 / 8).
    activations="int8" (DESIGN.md 4.4.7): hidden_size and intermediate_size must be multiples of 128, because one K-tile of the int8
    kernel is 128 bytes -- 7B, 13B, Llama-3-8B and 70B all are."""
    cfg = getattr(llama_model, "config", None)
    bad = []
    if type(llama_model).__name__ != "LlamaForCausalLM" or cfg is None:
        return [f"architecture: {type(llama_model).__name__} (HF LlamaForCausalLM required)"]
    prm = next(llama_model.parameters())
    if not (prm.is_cuda and getattr(torch.version, "hip", None)):
        bad.append(f"device: {prm.device} (a HIP device is required)")
    dtypes = sorted({str(q.dtype) for q in llama_model.parameters()})
    if dtypes != ["torch.float16"]:
        bad.append(f"dtype: {', '.join(dtypes)} (torch.float16 required)")
    heads, hidden = int(cfg.num_attention_heads), int(cfg.hidden_size)
    head_dim = int(getattr(cfg, "head_dim", None) or hidden // heads)
    if head_dim != 128 or hidden != heads * 128:
        bad.append(f"head size: head_dim {head_dim} with hidden_size {hidden} / {heads} heads (head_dim 128 and hidden = heads x 128 required)")
    kv = int(getattr(cfg, "num_key_value_heads", None) or heads)
    if grouped_kv:
        if kv < 1 or heads % kv or heads // kv not in GQA_RATIOS:
            bad.append(f"K/V heads: num_key_value_heads {kv} with num_attention_heads {heads} (grouped_kv takes a count that divides "
                       f"the query heads with a ratio in {list(GQA_RATIOS)})")
    elif kv != heads:
        bad.append(f"K/V heads: num_key_value_heads {kv} != num_attention_heads {heads} (grouped-query attention is not supported)")
    with_bias = [n for n, m in llama_model.named_modules() if isinstance(m, torch.nn.Linear) and m.bias is not None]
    if getattr(cfg, "attention_bias", False) or getattr(cfg, "mlp_bias", False) or with_bias:
        bad.append(f"biases: {len(with_bias)} linear layers carry a bias (bias-free linears required)")
    rope = getattr(cfg, "rope_parameters", None) or getattr(cfg, "rope_scaling", None) or {}
    rope_type = rope.get("rope_type", rope.get("type", "default")) if isinstance(rope, dict) else str(rope)
    if rope_type != "default":
        bad.append(f"rotary law: rope type {rope_type!r} (only the default, unscaled rope_theta law is supported)")
    if getattr(cfg, "sliding_window", None):
        bad.append(f"sliding window: {cfg.sliding_window} (full attention required)")
    if getattr(cfg, "hidden_act", "silu") != "silu":
        bad.append(f"activation: {cfg.hidden_act} (SwiGLU with silu required)")
    for name, val in (("hidden_size", hidden), ("intermediate_size", int(cfg.intermediate_size)), ("vocab_size", int(cfg.vocab_size))):
        if val % 64:
            bad.append(f"shape: {name} {val} is not a multiple of 64")
    if activations == "int8":
        for name, val in (("hidden_size", hidden), ("intermediate_size", int(cfg.intermediate_size))):
            if val % 128:
                bad.append(f'shape: {name} {val} is not a multiple of 128 (activations="int8": one K-tile of the int8 kernel is 128 bytes)')
    if max_batch is not None and int(max_batch) > 256:
        bad.append(f"batch: max_batch {int(max_batch)} > 256 rows (one GEMM row tile)")
    eos = getattr(getattr(llama_model, "generation_config", None), "eos_token_id", None)      # as greedy_tokens resolves it
    eos = getattr(cfg, "eos_token_id", None) if eos is None else eos
    if isinstance(eos, (list, tuple)) and len(eos) > 8:
        bad.append(f"EOS ids: {len(eos)} end-of-sequence ids (the token select takes at most 8)")
    return bad


def _rope_theta(cfg):
    rope = getattr(cfg, "rope_parameters", None) or getattr(cfg, "rope_scaling", None) or {}
    theta = rope.get("rope_theta") if isinstance(rope, dict) else None
    return float(theta or getattr(cfg, "rope_theta", None) or 10000.0)


class _HipDecoder:
    """The native token step of a frozen LlamaForCausalLM (`cgpt_llm_*`, include/cgpt.h): validates the model, creates the handle
    and hands it the module's own fp16 parameters ONCE (the library keeps fused copies: 2 bytes per parameter more HBM, 13.5 GB at
    7B; a later change of the module's weights is not seen; with weights="int8" the seven linears of every layer are held as row-wise
    absmax int8 instead, quantised on the device at load, 7.2 GB at 7B -- see `quantize_rows_int8`).  `greedy` enqueues the whole loop after the prefill on the current
    stream -- no host sync, capturable -- on the K/V buffers the prefill filled, in place."""
    MAX_LEN = 4096                                                     # positions the rotary table covers (prompt + new tokens)

    def __init__(self, llama_model, max_batch, weights="fp16", early_stop=False, grouped_kv=False, activations="fp16", int8_threshold=6.0,
                 outlier_cap=64):
        import ctypes as C
        from . import _lib
        if weights not in _lib.LLM_WEIGHT_FORMATS:
            raise ValueError(f'weights={weights!r}: expected "fp16" or "int8"')
        if activations not in _lib.LLM_ACT_FORMATS:
            raise ValueError(f'activations={activations!r}: expected "fp16" or "int8"')
        if activations == "int8" and weights != "int8":
            raise ValueError('activations="int8" needs weights="int8": int8 activations multiply int8 weights')
        if activations == "int8" and not 1 <= int(outlier_cap) <= 1024:
            raise ValueError(f"outlier_cap={outlier_cap!r}: expected 1..1024")
        self.weights = weights
        self.activations, self.int8_threshold, self.outlier_cap = activations, float(int8_threshold), int(outlier_cap)
        self._act_stats = None
        self.early_stop = bool(early_stop)
        self._greedy_ran = False                                       # live_steps has nothing to report before the first `greedy`
        self.stop_sequences = ()                                       # none is the handle's state at create
        self.trie = None                                               # likewise (set_trie)
        self.grouped_kv = bool(grouped_kv)
        bad = hip_decode_unsupported(llama_model, max_batch, grouped_kv=self.grouped_kv, activations=activations)
        if bad:
            raise ValueError('decode="hip" does not support this decoder -- ' + "; ".join(bad))
        self._C, self._lib_mod, self.L = C, _lib, _lib.lib()
        cfg = llama_model.config
        self.device = next(llama_model.parameters()).device
        self.layers, self.heads, self.vocab = int(cfg.num_hidden_layers), int(cfg.num_attention_heads), int(cfg.vocab_size)
        # K/V heads of the caches every entry works on: the model's own count under grouped_kv, the query heads otherwise
        self.kv_heads = int(getattr(cfg, "num_key_value_heads", None) or self.heads) if self.grouped_kv else self.heads
        self.max_batch = int(max_batch)
        # fp16 handles pass the config up to max_len, which every build of the library accepts (an A/B against an older build loads it
        # through CGPT_LIB_PATH); weight_format travels only when it says something
        # and so does grouped_kv: the extended struct (cgpt_llm_config_gqa) is sent only when the flag is set
        # and so does the activation format (cgpt_llm_config_act)
        size = (C.sizeof(_lib.LlmConfigAct) if activations != "fp16" else C.sizeof(_lib.LlmConfigGqa) if self.grouped_kv else
                C.sizeof(_lib.LlmConfig) if weights != "fp16" else _lib.LLM_CONFIG_SIZE_F16)
        c = _lib.LlmConfig(struct_size=size, weight_format=_lib.LLM_WEIGHT_FORMATS[weights], device=self.device.index or 0, hidden=int(cfg.hidden_size),
                           layers=self.layers, heads=self.heads, kv_heads=self.kv_heads, head_dim=128, mlp=int(cfg.intermediate_size),
                           vocab=self.vocab, rms_eps=float(cfg.rms_norm_eps), rope_theta=_rope_theta(cfg),
                           max_batch=self.max_batch, max_len=self.MAX_LEN)
        self.handle = C.c_void_p()
        ext = _lib.LlmConfigGqa(base=c, grouped_kv=int(self.grouped_kv), reserved=0)     # create reads past `base` only when the size says so
        act = _lib.LlmConfigAct(gqa=ext, act_format=_lib.LLM_ACT_FORMATS[activations], act_threshold=self.int8_threshold,
                                outlier_cap=self.outlier_cap, reserved2=0)
        _lib.check(self.L.cgpt_llm_create(C.byref(act.gqa.base), C.byref(self.handle)))
        st = self._stream()
        wanted = ["model.embed_tokens.weight", "model.norm.weight", "lm_head.weight"]
        for i in range(self.layers):
            wanted += [f"model.layers.{i}.self_attn.{n}_proj.weight" for n in "qkvo"]
            wanted += [f"model.layers.{i}.mlp.{n}_proj.weight" for n in ("gate", "up", "down")]
            wanted += [f"model.layers.{i}.{n}_layernorm.weight" for n in ("input", "post_attention")]
        sd = llama_model.state_dict()
        for name in wanted:
            w = sd[name].detach()
            assert w.dtype == torch.float16 and w.device == self.device, name
            w = w.contiguous()
            _lib.check(self.L.cgpt_llm_load_weight_f16(self.handle, name.encode(), C.c_void_p(w.data_ptr()), w.numel(), st))
        torch.cuda.current_stream(self.device).synchronize()           # contiguous() temporaries may go once the copies have run
        if self.early_stop:                                            # off is the handle's state at create: nothing is called for it
            _lib.check(self.L.cgpt_llm_set_early_stop(self.handle, 1))

    @property
    def weight_bytes(self):
        """Bytes the handle holds for weight matrices, row scales and the dequantisation scratch (cgpt_llm_weight_bytes: the
        library's own accounting).  None on a build of the library that predates the entry (CGPT_LIB_PATH A/B runs)."""
        C = self._C
        if not hasattr(self.L, "cgpt_llm_weight_bytes"):
            return None
        n = C.c_int64()
        self._lib_mod.check(self.L.cgpt_llm_weight_bytes(self.handle, C.byref(n)))
        return int(n.value)

    def act_stats(self):
        """{rows, outliers, max_outliers_per_row, overflow_rows} of the native calls since the last read (cgpt_llm_act_stats: one
        device sync; the counters are reset).  When nothing ran since, the last non-empty reading is returned again.  RuntimeError when
        a row had more outliers than `outlier_cap`: its result is not the law's."""
        C = self._C
        if self.activations != "int8":
            raise RuntimeError('act_stats: the engine was built with activations="fp16"')
        v = (C.c_int64 * 4)()
        self._lib_mod.check(self.L.cgpt_llm_act_stats(self.handle, v))
        if v[0] > 0 or self._act_stats is None:
            self._act_stats = {"rows": int(v[0]), "outliers": int(v[1]), "max_outliers_per_row": int(v[2]), "overflow_rows": int(v[3])}
        if self._act_stats["overflow_rows"] > 0:
            stats, self._act_stats = self._act_stats, None
            raise RuntimeError(f'activations="int8": {stats["overflow_rows"]} of {stats["rows"]} activation rows had more than '
                               f'outlier_cap={self.outlier_cap} outliers (the largest row: {stats["max_outliers_per_row"]}); their '
                               "results are not the law's -- raise outlier_cap (up to 1024) or int8_threshold")
        return dict(self._act_stats)

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self.L.cgpt_llm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _cache_tables(self, k_bufs, v_bufs, B, need_len):
        """Host tables of the per-layer K / V device pointers, after checking every buffer is what the kernels index:
        [B, heads, len_stride, 128] fp16 ([B, kv_heads, len_stride, 128] under grouped_kv), contiguous, on the handle's device, long
        enough for the last appended row."""
        C = self._C
        assert len(k_bufs) == len(v_bufs) == self.layers, "one K and one V buffer per layer"
        stride = int(k_bufs[0].shape[2])
        assert need_len <= stride and need_len <= self.MAX_LEN, (need_len, stride, self.MAX_LEN)
        for t in list(k_bufs) + list(v_bufs):
            assert (t.dtype == torch.float16 and t.device == self.device and t.is_contiguous()
                    and tuple(t.shape) == (B, self.kv_heads, stride, 128)), (tuple(t.shape), t.dtype, t.device)
        kp = (C.c_void_p * self.layers)(*[t.data_ptr() for t in k_bufs])
        vp = (C.c_void_p * self.layers)(*[t.data_ptr() for t in v_bufs])
        return kp, vp, stride

    def _stream(self):
        """The current stream of the handle's device, as the entries take it."""
        return self._C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check_first_logits(self, first_logits):
        """first_logits [B, vocab] fp32 as a prefill leaves them -> (B, vocab)."""
        B, V = first_logits.shape
        assert (first_logits.dtype == torch.float32 and first_logits.device == self.device and first_logits.is_contiguous()
                and V == self.vocab and 1 <= B <= self.max_batch)
        return B, V

    def _starts_ptr(self, starts, B):
        """`starts` [B] int32 on the handle's device (pad positions per row of a left-padded batch; the kernels read it when they run,
        so a captured call sees its contents at every replay) -> the pointer the _ragged entries take."""
        assert (starts.dtype == torch.int32 and starts.device == self.device and starts.is_contiguous()
                and tuple(starts.shape) == (B,)), (tuple(starts.shape), starts.dtype, starts.device)
        return self._C.c_void_p(starts.data_ptr())

    def _call(self, entry, starts, src, B, n, *rest):
        """cgpt_llm_<entry>(handle, src, B, n, *rest), or with `starts` its _ragged twin, whose signature is the plain one with the
        starts pointer after those four."""
        if starts is None:
            rc = getattr(self.L, "cgpt_llm_" + entry)(self.handle, src, B, n, *rest)
        else:
            rc = getattr(self.L, "cgpt_llm_" + entry + "_ragged")(self.handle, src, B, n, self._starts_ptr(starts, B), *rest)
        self._lib_mod.check(rc)

    def step(self, tokens, pos, k_bufs, v_bufs, starts=None):
        """One teacher-forced step: tokens [B] int64 at position `pos` -> logits [B, vocab] fp32; K / V row `pos` appended in place.
        starts (or None: the plain entry): left-padded rows, `pos` is the position in the padded buffer."""
        C = self._C
        B = int(tokens.shape[0])
        assert tokens.dtype == torch.int64 and tokens.device == self.device and tokens.is_contiguous() and 1 <= B <= self.max_batch
        kp, vp, stride = self._cache_tables(k_bufs, v_bufs, B, int(pos) + 1)
        logits = torch.empty((B, self.vocab), dtype=torch.float32, device=self.device)
        self._call("step", starts, C.c_void_p(tokens.data_ptr()), B, int(pos), kp, vp, stride, C.c_void_p(logits.data_ptr()), self._stream())
        return logits

    def prefill(self, embs, k_bufs, v_bufs, starts=None):
        """The native prefill: embs [B, L, hidden] fp16 -> last-position logits [B, vocab] fp32; rows 0 .. L-1 of every layer's K / V
        buffer filled in place.  The workspace is reserved here, for `max_batch` rows of this prompt length, so that batches of any
        size share one reservation (outside any capture: a captured call must come after an eager one of the same prompt length,
        which `_generate_graph`'s warm-up run is).  A longer prompt later grows it; the library keeps the replaced buffers until the
        handle goes, so graphs captured before keep replaying on valid memory.
        starts (or None: the plain entry): row b is left-padded by starts[b] positions; cache rows starts[b] .. L-1 are filled."""
        C = self._C
        B, L, hidden = embs.shape
        assert (embs.dtype == torch.float16 and embs.device == self.device and embs.is_contiguous() and hidden == self.heads * 128
                and 1 <= B <= self.max_batch and L >= 1)
        kp, vp, stride = self._cache_tables(k_bufs, v_bufs, B, L)
        if not torch.cuda.is_current_stream_capturing():
            self._lib_mod.check(self.L.cgpt_llm_prefill_reserve(self.handle, self.max_batch, L))
        logits = torch.empty((B, self.vocab), dtype=torch.float32, device=self.device)
        self._call("prefill", starts, C.c_void_p(embs.data_ptr()), B, int(L), kp, vp, stride, C.c_void_p(logits.data_ptr()), self._stream())
        return logits

    def prefill_from(self, embs, pos0, k_bufs, v_bufs, starts=None):
        """The continuation prefill (cgpt_llm_prefill_from): embs [B, Ln, hidden] fp16 are positions pos0 .. pos0+Ln-1 of rows whose
        cache rows 0 .. pos0-1 exist (an earlier `prefill` / `prefill_from`, steps, or `kv_broadcast`) -> the logits of position
        pos0+Ln-1, [B, vocab] fp32; cache rows pos0 .. pos0+Ln-1 of every layer filled in place, bit for bit what `prefill` leaves for
        the whole prompt.  The workspace is reserved as in `prefill`, for `max_batch` rows of Ln positions.
        starts (or None): the left padding of the Ln-position buffer; the cache layout is then the ragged prefill's of pos0+Ln buffer
        positions under the same starts (the earlier rows of row b sit at starts[b] .. starts[b]+pos0-1)."""
        C = self._C
        B, Ln, hidden = embs.shape
        pos0 = int(pos0)
        assert (embs.dtype == torch.float16 and embs.device == self.device and embs.is_contiguous() and hidden == self.heads * 128
                and 1 <= B <= self.max_batch and Ln >= 1 and pos0 >= 0)
        kp, vp, stride = self._cache_tables(k_bufs, v_bufs, B, pos0 + Ln)
        if not torch.cuda.is_current_stream_capturing():
            self._lib_mod.check(self.L.cgpt_llm_prefill_reserve(self.handle, self.max_batch, Ln))
        logits = torch.empty((B, self.vocab), dtype=torch.float32, device=self.device)
        self._lib_mod.check(self.L.cgpt_llm_prefill_from(self.handle, C.c_void_p(embs.data_ptr()), B, pos0, int(Ln),
                                                         None if starts is None else self._starts_ptr(starts, B), kp, vp, stride,
                                                         C.c_void_p(logits.data_ptr()), self._stream()))
        return logits

    def kv_broadcast(self, src_k, src_v, P, k_bufs, v_bufs, starts=None):
        """cgpt_llm_kv_broadcast: rows 0 .. P-1 of the one-row caches src_k / src_v (per layer, [1, kv_heads, src_stride, 128]) into rows
        starts[b] .. starts[b]+P-1 (0 .. P-1 without starts) of every row of k_bufs / v_bufs; no other row is written."""
        B = int(k_bufs[0].shape[0])
        skp, svp, sstride = self._cache_tables(src_k, src_v, 1, int(P))
        kp, vp, stride = self._cache_tables(k_bufs, v_bufs, B, int(P))
        self._lib_mod.check(self.L.cgpt_llm_kv_broadcast(self.handle, skp, svp, sstride, int(P), B,
                                                         None if starts is None else self._starts_ptr(starts, B), kp, vp, stride,
                                                         self._stream()))

    def _decode(self, entry, first_logits, prompt_len, num_new, min_new, eos_ids, pad_id, k_bufs, v_bufs, return_logits, starts, extra=()):
        """The one body of `greedy`, `sample` and `constrained`: cgpt_llm_<entry>, whose arguments between the step-logits pointer and
        the stream are `extra`."""
        C = self._C
        B, V = self._check_first_logits(first_logits)
        assert num_new >= 1 and (eos_ids is None or len(eos_ids) <= 8)
        kp, vp, stride = self._cache_tables(k_bufs, v_bufs, B, prompt_len + num_new - 1)
        tokens = torch.empty((B, num_new), dtype=torch.int64, device=self.device)
        steps = torch.empty((B, num_new, V), dtype=torch.float32, device=self.device) if return_logits else None
        # the constrained entries (eos_ids None) take neither min_new nor EOS ids: the trie ends the rows
        stop = () if eos_ids is None else (int(min_new), (C.c_int64 * max(1, len(eos_ids)))(*[int(e) for e in eos_ids]), len(eos_ids))
        self._greedy_ran = True
        self._call(entry, starts, C.c_void_p(first_logits.data_ptr()), B, int(prompt_len), int(num_new), *stop,
                   int(pad_id), kp, vp, stride, C.c_void_p(tokens.data_ptr()), C.c_void_p(steps.data_ptr()) if return_logits else None,
                   *extra, self._stream())
        return (tokens, steps) if return_logits else tokens

    def greedy(self, first_logits, prompt_len, num_new, min_new, eos_ids, pad_id, k_bufs, v_bufs, return_logits=False, starts=None):
        """The loop of `greedy_tokens` after the prefill: tokens [B, num_new] int64 (and the logits each arg-max saw).
        starts (or None: the plain entry): the prefill's left padding; `prompt_len` is then the padded length."""
        return self._decode("greedy", first_logits, prompt_len, num_new, min_new, eos_ids, pad_id, k_bufs, v_bufs, return_logits, starts)

    def sample(self, first_logits, prompt_len, num_new, min_new, eos_ids, pad_id, k_bufs, v_bufs, settings, draw_ids, seed,
               return_logits=False, starts=None):
        """`greedy` with the sampling law in the place of the arg-max (cgpt_llm_sample / cgpt_llm_sample_ragged; `sample_token_law`).
        settings = (do_sample, temperature, top_k, top_p, repetition_penalty); draw_ids [B] int64 and seed [1] int64 (the 64 bits of
        the seed) live on the device and are read when the kernels run, so a captured call draws whatever they hold at each replay."""
        C = self._C
        B = int(first_logits.shape[0])                                 # `_decode` checks first_logits itself
        assert (draw_ids.dtype == torch.int64 and draw_ids.device == self.device and draw_ids.is_contiguous()
                and tuple(draw_ids.shape) == (B,)), (tuple(draw_ids.shape), draw_ids.dtype, draw_ids.device)
        assert seed.dtype == torch.int64 and seed.device == self.device and seed.numel() == 1, (seed.dtype, seed.device)
        params = self._lib_mod.sample_params(*check_sample_settings(settings))
        return self._decode("sample", first_logits, prompt_len, num_new, min_new, eos_ids, pad_id, k_bufs, v_bufs, return_logits, starts,
                            extra=(params, C.c_void_p(draw_ids.data_ptr()), C.c_void_p(seed.data_ptr())))

    def set_trie(self, trie):
        """cgpt_llm_set_trie: the candidate trie (`build_answer_trie`; None clears it) of the next `constrained`; validated by the
        library, copied to the device, read when a constrained call enqueues -- a captured call keeps what it was captured under.
        Synchronises and allocates: outside any capture."""
        C = self._C
        if trie is None:
            self._lib_mod.check(self.L.cgpt_llm_set_trie(self.handle, None, None, None, None, 0, 0))
        else:
            tabs = [t.to(dtype=torch.int32, device="cpu").contiguous() for t in trie.tables()]
            self._lib_mod.check(self.L.cgpt_llm_set_trie(self.handle, *[C.c_void_p(t.data_ptr()) for t in tabs], trie.nodes, trie.edges))
        self.trie = trie

    def constrained(self, first_logits, prompt_len, pad_id, k_bufs, v_bufs, return_logits=False, starts=None):
        """The constrained loop after the prefill (cgpt_llm_constrained / _ragged; `constrained_decode_law`): `depth` selects over the
        trie `set_trie` handed over -> (tokens [B, depth] int64, labels [B] int32[, the raw logits each select read])."""
        C = self._C
        if self.trie is None:
            raise RuntimeError("constrained: no trie is set on this engine (set_trie)")
        B = int(first_logits.shape[0])
        labels = torch.empty((B,), dtype=torch.int32, device=self.device)
        out = self._decode("constrained", first_logits, prompt_len, self.trie.depth, None, None, pad_id, k_bufs, v_bufs, return_logits,
                           starts, extra=(C.c_void_p(labels.data_ptr()),))
        return (out[0], labels, out[1]) if return_logits else (out, labels)

    def _beam_tables(self, B, k, prompt_k, prompt_v, beam_k, beam_v, prompt_len, beam_len):
        """The four host pointer tables of a beam entry: prompt caches of B image rows, beam caches of B * k beam rows."""
        assert not self.grouped_kv, "beam search runs on plain handles"
        pk, pv, pstride = self._cache_tables(prompt_k, prompt_v, B, int(prompt_len))
        bk, bv, bstride = self._cache_tables(beam_k, beam_v, B * k, max(1, int(beam_len)))
        return pk, pv, pstride, bk, bv, bstride

    def beam_step(self, tokens, k, prompt_len, t, anc, prompt_k, prompt_v, beam_k, beam_v):
        """One teacher-forced beam step (cgpt_llm_beam_step): tokens [B * k] int64 at generated position t of beam rows whose image
        prompts (prompt_len positions) sit in prompt_k / prompt_v [B, heads, ., 128] and whose generated positions sit in beam_k /
        beam_v [B * k, heads, ., 128] under the ancestry table anc [B * k, >= t] int32 -> logits [B * k, vocab] fp32; row t of every
        beam row's own cache appended in place."""
        C = self._C
        rows = int(tokens.shape[0])
        B = rows // int(k)
        assert rows == B * k and tokens.dtype == torch.int64 and tokens.device == self.device and tokens.is_contiguous()
        assert (anc.dtype == torch.int32 and anc.device == self.device and anc.is_contiguous() and anc.dim() == 2
                and anc.shape[0] == rows and anc.shape[1] >= t), (tuple(anc.shape), anc.dtype)
        pk, pv, pstride, bk, bv, bstride = self._beam_tables(B, k, prompt_k, prompt_v, beam_k, beam_v, prompt_len, t + 1)
        logits = torch.empty((rows, self.vocab), dtype=torch.float32, device=self.device)
        self._lib_mod.check(self.L.cgpt_llm_beam_step(self.handle, C.c_void_p(tokens.data_ptr()), B, int(k), int(prompt_len), int(t),
                                                      C.c_void_p(anc.data_ptr()), int(anc.shape[1]), pk, pv, pstride, bk, bv, bstride,
                                                      C.c_void_p(logits.data_ptr()), self._stream()))
        return logits

    def beam_reserve(self, k, num_new):
        """cgpt_llm_beam_reserve for as many images as the handle's rows hold at k beams; outside any capture, grows only."""
        self._lib_mod.check(self.L.cgpt_llm_beam_reserve(self.handle, max(1, self.max_batch // int(k)), int(k), int(num_new)))

    def beam(self, first_logits, k, prompt_len, num_new, min_new, eos_ids, pad_id, length_penalty, prompt_k, prompt_v, beam_k, beam_v,
             return_logits=False):
        """The beam search after the prefill (cgpt_llm_beam; `beam_decode_law`): first_logits [B, vocab] fp32 = the prefill's logits
        of B images, prompt_k / prompt_v the caches it filled, beam_k / beam_v [B * k, heads, >= num_new - 1, 128] the beams' own ->
        (tokens [B, num_new] int64: the best finished hypothesis, then pad ids; scores [B] fp32: its `sequences_scores`) and, with
        return_logits, the raw logits every select read [B * k, num_new, vocab] and the state after every select [num_new, B, 5 k + 1]
        (running, parents, tokens, pool scores, pool flags, open).  The state is reserved here (outside a capture only)."""
        C = self._C
        B, V = first_logits.shape
        assert (first_logits.dtype == torch.float32 and first_logits.device == self.device and first_logits.is_contiguous()
                and V == self.vocab and 1 <= B * k <= self.max_batch), (tuple(first_logits.shape), k, self.max_batch)
        assert num_new >= 1 and len(eos_ids) <= 8
        pk, pv, pstride, bk, bv, bstride = self._beam_tables(B, k, prompt_k, prompt_v, beam_k, beam_v, prompt_len, num_new - 1)
        if not torch.cuda.is_current_stream_capturing():
            self.beam_reserve(k, num_new)
        tokens = torch.empty((B, num_new), dtype=torch.int64, device=self.device)
        scores = torch.empty((B,), dtype=torch.float32, device=self.device)
        steps = torch.empty((B * k, num_new, V), dtype=torch.float32, device=self.device) if return_logits else None
        trace = torch.empty((num_new, B, 5 * k + 1), dtype=torch.float32, device=self.device) if return_logits else None
        self._greedy_ran = True
        self._lib_mod.check(self.L.cgpt_llm_beam(
            self.handle, C.c_void_p(first_logits.data_ptr()), B, int(k), int(prompt_len), int(num_new), int(min_new),
            (C.c_int64 * max(1, len(eos_ids)))(*[int(e) for e in eos_ids]), len(eos_ids), int(pad_id), float(length_penalty), pk, pv, pstride,
            bk, bv, bstride, C.c_void_p(tokens.data_ptr()), C.c_void_p(scores.data_ptr()),
            C.c_void_p(steps.data_ptr()) if return_logits else None, C.c_void_p(trace.data_ptr()) if return_logits else None, self._stream()))
        return (tokens, scores, steps, trace) if return_logits else (tokens, scores)

    def set_early_stop(self, on):
        """cgpt_llm_set_early_stop: read by the next `greedy` when it enqueues; a captured call keeps what it was captured under."""
        self._lib_mod.check(self.L.cgpt_llm_set_early_stop(self.handle, int(bool(on))))
        self.early_stop = bool(on)

    def set_stop_sequences(self, seqs):
        """cgpt_llm_set_stop_sequences: token-id sequences (`check_stop_words_ids`; () or None clears them) at which a row of the next
        `greedy` finishes besides its EOS ids; read when it enqueues, a captured call keeps what it was captured under."""
        C = self._C
        seqs = check_stop_words_ids(seqs)
        flat = [t for s in seqs for t in s]
        ids = (C.c_int64 * max(1, len(flat)))(*flat)
        lens = (C.c_int32 * max(1, len(seqs)))(*[len(s) for s in seqs])
        self._lib_mod.check(self.L.cgpt_llm_set_stop_sequences(self.handle, ids, lens, len(seqs)))
        self.stop_sequences = seqs

    def live_steps(self):
        """cgpt_llm_live_steps after the last `greedy` (or the last replay of a graph that captured it): the token steps that ran.
        Synchronises the CURRENT stream -- the one the call was enqueued or the graph replayed on; RuntimeError when no greedy has
        been enqueued."""
        C = self._C
        if not self._greedy_ran:
            raise RuntimeError("live_steps: no native greedy decode has run on this engine yet")
        n = C.c_int32(-1)
        self._lib_mod.check(self.L.cgpt_llm_live_steps(self.handle, C.byref(n), self._stream()))
        return int(n.value)

    MAX_CANDS, MAX_TAIL = 64, 64                                       # SCORE_MAX_CANDS, SCORE_MAX_TAIL (csrc/llm.h)

    def score(self, first_logits, prompt_len, cand_tokens, cand_lens, label_smoothing, k_bufs, v_bufs, starts=None, row_lens=None):
        """Every candidate on the prompt cache a prefill left (cgpt_llm_score): first_logits [B, vocab] fp32 = that prefill's result,
        cand_tokens [C, Tmax] int64 on the device, cand_lens = the C token counts (host) -> [B, C] fp32, the SUM over each
        candidate's tokens of the label-smoothed cross-entropy.  Reads cache rows 0 .. prompt_len-1 and writes none.  The workspace is
        reserved here (outside any capture), for `max_batch` rows of this call's tail rows.
        starts and row_lens (both, or both None: the plain entry) -- per-row prompts and candidates (cgpt_llm_score_ragged): starts
        [B] int32 = the ragged prefill's left padding, `prompt_len` the padded length; cand_tokens [B, C, Tmax], row_lens [B, C] int32 on
        the device = each row's real length of each candidate, cand_lens = the longest length of each candidate over the rows
        (`pack_row_candidates`).  Reads cache rows starts[b] .. prompt_len-1 only; sums each row's own tokens."""
        C = self._C
        assert (starts is None) == (row_lens is None), "starts and row_lens travel together"
        n, tmax = cand_tokens.shape[-2:]
        lens = [int(t) for t in cand_lens]
        B, _ = self._check_first_logits(first_logits)
        assert (cand_tokens.dtype == torch.int64 and cand_tokens.device == self.device and cand_tokens.is_contiguous()
                and len(lens) == n and tuple(cand_tokens.shape) == ((n, tmax) if starts is None else (B, n, tmax)))
        if row_lens is not None:
            assert (row_lens.dtype == torch.int32 and row_lens.device == self.device and row_lens.is_contiguous()
                    and tuple(row_lens.shape) == (B, n)), (tuple(row_lens.shape), row_lens.dtype, row_lens.device)
        kp, vp, stride = self._cache_tables(k_bufs, v_bufs, B, int(prompt_len))
        if not torch.cuda.is_current_stream_capturing():
            self._lib_mod.check(self.L.cgpt_llm_score_reserve(self.handle, self.max_batch, max(1, sum(t - 1 for t in lens))))
        out = torch.empty((B, n), dtype=torch.float32, device=self.device)
        table = (C.c_void_p(cand_tokens.data_ptr()),) + (() if row_lens is None else (C.c_void_p(row_lens.data_ptr()),))
        self._call("score", starts, C.c_void_p(first_logits.data_ptr()), B, int(prompt_len), *table, (C.c_int32 * n)(*lens), n, int(tmax),
                   float(label_smoothing), kp, vp, stride, C.c_void_p(out.data_ptr()), self._stream())
        return out
