/*
 * cgpt.h -- C-ABI of libcgpt.so: the MI355X-native randomized-smoothing certify/predict hot path.
 *
 * The reference (leodesouza/certifiedGPT) has no FFI: its hot path is the Python class
 * `Smooth` (randomized_smoothing/smoothing.py:13-117) calling a PyTorch base classifier
 * (MiniGPT4.encode_img, graphs/models/minigpt4/models/minigpt4.py:121-149, built from
 * eva_vit.py / Qformer.py).  Each entry point below names the reference interface it replaces.
 * A maintainer binds them with ctypes; certifiedgpt_amd/_lib.py is that binding.
 *
 * Conventions
 *   - plain C types only; no torch / HIP types in signatures (streams are passed as void* = hipStream_t,
 *     0 = the null stream; PyTorch-ROCm's torch.cuda.current_stream().cuda_stream is accepted as is).
 *   - every function returns cgpt_status (0 = ok).  Nothing throws across the ABI;
 *     cgpt_last_error() returns a thread-local message for the last failing call.
 *   - the caller owns every buffer it passes.  `*_dev` pointers are device (HBM) pointers,
 *     `*_host` pointers are host pointers.
 *   - a handle is bound to one device and is NOT thread-safe: one handle per process per GPU.
 *     All device work is enqueued on the caller's stream; the only host syncs are inside
 *     cgpt_load_weight/cgpt_get_weight (host<->device copies) and where documented.
 *   - there is no CPU fallback: device entry points fail with CGPT_ERR_NO_DEVICE without a GPU.
 */
#ifndef CGPT_H
#define CGPT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int cgpt_status;
enum {
    CGPT_OK = 0,
    CGPT_ERR_INVALID = 1,     /* bad argument / shape mismatch                         */
    CGPT_ERR_NO_DEVICE = 2,   /* no HIP device visible                                 */
    CGPT_ERR_HIP = 3,         /* a HIP runtime call failed (message in cgpt_last_error) */
    CGPT_ERR_NOT_FOUND = 4,   /* unknown weight name                                   */
    CGPT_ERR_STATE = 5        /* weights not loaded / wrong mode                       */
};

#define CGPT_ABSTAIN (-1)     /* Smooth.ABSTAIN, smoothing.py:17 */

/* Noise law of the Monte-Carlo draws (cgpt_set_noise_law, cgpt_noise_batch_law) and of the certificate (*_law statistics).
 * GAUSSIAN: x + sigma * eps, eps ~ N(0,1)^d (smoothing.py:96); certified L2 radius sigma * Phi^-1(pA_lower).
 * UNIFORM:  x + level * u, u ~ U[0,1)^d per coordinate (the fine-tuning noise `image + torch.rand_like(image) * noise_level`,
 *           agents/minigpt4_finetune_agent.py:142-147); certified L1 radius level * (pA_lower - 1/2).
 * Both laws draw from the same counter-based Philox stream, keyed (noise_seed, sample index, element): counts stay invariant
 * under any batching or sharding.  The `sigma` argument of every noisy entry point is the scale: sigma or level. */
enum { CGPT_NOISE_GAUSSIAN = 0, CGPT_NOISE_UNIFORM = 1 };

/* What the base classifier computes after the noise is added (smoothing.py:97 `base_classifier(batch + noise)`). */
enum {
    CGPT_MODE_VIT_HEAD = 0,   /* EVA-ViT-G forward_features (eva_vit.py:332-349) -> ln_vision (base_model.py:281-287)
                                 on the CLS token -> build-side Linear(vit_dim -> num_classes) head.  BASELINE config 2. */
    CGPT_MODE_ENCODE_IMG = 1  /* full MiniGPT4.encode_img (minigpt4.py:121-149): ViT -> ln_vision -> Q-Former
                                 (Qformer.py:78-108,169-289,349-484) -> llama_proj, then a build-side head
                                 Linear(proj_dim -> num_classes) on the mean of the query tokens.             */
};

typedef struct cgpt_config {
    int32_t struct_size;      /* = sizeof(cgpt_config); guards ABI drift */
    int32_t mode;             /* CGPT_MODE_*                                                       */
    int32_t device;           /* HIP device ordinal                                                */
    int32_t num_classes;      /* Smooth.num_classes, smoothing.py:19                               */
    int32_t max_batch;        /* largest batch_size a call may use (sizes the HBM workspace)       */
    /* EVA-ViT (create_eva_vit_g, eva_vit.py:425-438) */
    int32_t img_size;         /* 224  */
    int32_t patch_size;       /* 14   */
    int32_t vit_dim;          /* 1408 */
    int32_t vit_depth;        /* 39   */
    int32_t vit_heads;        /* 16 (head_dim must be 88 or 64)                                    */
    int32_t vit_mlp;          /* 6144 = int(1408 * 4.3637)                                         */
    float   vit_ln_eps;       /* 1e-6 (eva_vit.py:436)                                             */
    float   ln_vision_eps;    /* 1e-5 (nn.LayerNorm default, base_model.py:281)                    */
    /* Q-Former (MiniGPT4.init_Qformer, minigpt4.py:90-119; BERT-base) -- ignored in CGPT_MODE_VIT_HEAD */
    int32_t qf_layers;        /* 12   */
    int32_t qf_dim;           /* 768  */
    int32_t qf_heads;         /* 12 (head_dim must be 64)                                          */
    int32_t qf_ffn;           /* 3072 */
    int32_t qf_queries;       /* 32   */
    int32_t qf_xattn_freq;    /* 2: cross-attention in layers 0,2,4,... (Qformer.py:386-395)       */
    float   qf_ln_eps;        /* 1e-12 */
    int32_t proj_dim;         /* 4096: llama_proj out features (minigpt4.py:76-78)                 */
} cgpt_config;

typedef struct cgpt_model* cgpt_handle;

/* ---- life cycle (replaces: MiniGPT4.__init__/from_config device placement, minigpt4.py:29-199) ---- */
cgpt_status cgpt_create(const cgpt_config* cfg, cgpt_handle* out);
cgpt_status cgpt_destroy(cgpt_handle h);
const char* cgpt_last_error(void);
const char* cgpt_version(void);

/* ---- weights (replaces: load_state_dict + convert_weights_to_fp16, eva_vit.py:407-422,454) ----
 * Names follow the reference state_dict:  "visual_encoder.patch_embed.proj.weight", "visual_encoder.cls_token",
 * "visual_encoder.pos_embed", "visual_encoder.blocks.<i>.{norm1,norm2}.{weight,bias}",
 * "visual_encoder.blocks.<i>.attn.{qkv.weight,q_bias,v_bias,proj.weight,proj.bias}",
 * "visual_encoder.blocks.<i>.mlp.{fc1,fc2}.{weight,bias}", "ln_vision.{weight,bias}", "query_tokens",
 * "Qformer.bert.embeddings.LayerNorm.{weight,bias}",
 * "Qformer.bert.encoder.layer.<i>.{attention,crossattention}.self.{query,key,value}.{weight,bias}",
 * "Qformer.bert.encoder.layer.<i>.{attention,crossattention}.output.{dense,LayerNorm}.{weight,bias}",
 * "Qformer.bert.encoder.layer.<i>.{intermediate_query,output_query}.dense.{weight,bias}",
 * "Qformer.bert.encoder.layer.<i>.output_query.LayerNorm.{weight,bias}", "llama_proj.{weight,bias}",
 * and the build-side "head.{weight,bias}".
 * `data_host` is float32, contiguous, in the PyTorch shape; `numel` must match.  GEMM weights are stored
 * in HBM as fp16 (the reference's precision contract on HIP: fp16 weights + fp16 autocast,
 * eva_vit.py:407-414, base_model.py:132-142); LayerNorm / bias / pos_embed parameters stay fp32. */
cgpt_status cgpt_load_weight(cgpt_handle h, const char* name, const float* data_host, int64_t numel);
/* Copy a weight back as float32 (exactly the values the device computes with, i.e. after fp16 rounding). */
cgpt_status cgpt_get_weight(cgpt_handle h, const char* name, float* out_host, int64_t numel);
/* Number of elements of a named weight (for sizing cgpt_get_weight buffers); <0 if unknown. */
int64_t     cgpt_weight_numel(cgpt_handle h, const char* name);
/* Name of the i-th weight (NULL past the end) -- lets a binding enumerate the state_dict. */
const char* cgpt_weight_name(cgpt_handle h, int32_t index);
/* Fill every weight on the device following the reference's init law (eva_vit.py:295-323:
 * trunc_normal(.02) Linear weights, zero biases, LN (1,0), proj/fc2 / sqrt(2*layer_id); Qformer.py:664-674:
 * normal(0,.02); minigpt4.py:99-102) from a counter-based generator.  There is no checkpoint in the container. */
cgpt_status cgpt_init_synthetic_weights(cgpt_handle h, uint64_t seed, void* stream);
/* Noise law (CGPT_NOISE_*) of every later noisy call of the handle: cgpt_sample_counts, cgpt_sample_counts2,
 * cgpt_sample_counts_images, cgpt_forward_logits and cgpt_encode_img_noisy.  Default CGPT_NOISE_GAUSSIAN; any other value
 * is CGPT_ERR_INVALID.  The law is read when a call ENQUEUES its kernels: a graph captured under one law keeps that law. */
cgpt_status cgpt_set_noise_law(cgpt_handle h, int32_t law);

/* ---- the hot loop: Smooth._sample_noise (smoothing.py:81-99) ----
 * For global sample indices s in [first_sample, first_sample + num): draw eps_s ~ N(0,1)^{3xHxW} from the
 * counter-based stream keyed (noise_seed, s, element), run the base classifier on x + sigma*eps_s in
 * batches of at most batch_size, take argmax(1) and ADD the votes into counts_dev[num_classes] (int64).
 * counts_dev is NOT zeroed here (callers accumulate shards); no host sync.
 * Sharding-aware through first_sample: counts are bit-identical for any partition of the index range. */
cgpt_status cgpt_sample_counts(cgpt_handle h, const float* x_dev, int64_t first_sample, int64_t num,
                               int64_t batch_size, float sigma, uint64_t noise_seed,
                               int64_t* counts_dev, void* stream);
/* Two sample-index ranges in ONE pass: Smooth.certify draws n0 selection samples and n estimation samples
 * (smoothing.py:44,48); they are independent, so both can ride in the same classifier batches.  Samples
 * [first_a, first_a+num_a) vote into counts_a_dev, samples [first_b, first_b+num_b) into counts_b_dev; batches of up to
 * batch_size samples may span the two ranges.  Results are identical to two cgpt_sample_counts calls. */
cgpt_status cgpt_sample_counts2(cgpt_handle h, const float* x_dev, int64_t first_a, int64_t num_a, int64_t* counts_a_dev,
                                int64_t first_b, int64_t num_b, int64_t* counts_b_dev, int64_t batch_size, float sigma,
                                uint64_t noise_seed, void* stream);
/* The same pass for SEVERAL images at once: image i (x_dev + i*3*H*W) draws samples first_a + i*image_stride + [0, num_a)
 * and first_b + i*image_stride + [0, num_b), exactly what num_images consecutive Smooth.certify calls would use with
 * image_stride = n0 + n.  counts_dev is int64 [num_images, 2, num_classes] (selection row, estimation row), ADDED into.
 * The (image, sample) rows of all images form one sequence that is cut into classifier batches of max_batch rows, NOT aligned
 * to image boundaries: a rank that owns only a thin slice of every image's samples (N/8 on 8 GPUs) still runs full batches,
 * and max_batch can be chosen for the GEMMs' tile quantisation (255 samples = 65 535 token rows = exactly 256 tile rows)
 * rather than for n0 + n.  Counts are bit-identical to the per-image calls. */
cgpt_status cgpt_sample_counts_images(cgpt_handle h, const float* x_dev, int64_t num_images, int64_t first_a, int64_t num_a,
                                      int64_t first_b, int64_t num_b, int64_t image_stride, int64_t* counts_dev, float sigma,
                                      uint64_t noise_seed, void* stream);
/* Same batches, but return the logits [num, num_classes] float32 instead of voting (parity tests; num <= max_batch). */
cgpt_status cgpt_forward_logits(cgpt_handle h, const float* x_dev, int64_t first_sample, int64_t num,
                                float sigma, uint64_t noise_seed, float* logits_dev, void* stream);
/* Run the classifier on caller-supplied images [num,3,H,W] float32 (no noise) -> logits [num,num_classes]. */
cgpt_status cgpt_classify(cgpt_handle h, const float* images_dev, int64_t num, float* logits_dev, void* stream);
/* MiniGPT4.encode_img (minigpt4.py:121-149) as a first-class product: ViT -> ln_vision -> Q-Former -> llama_proj for
 * `num` caller-supplied images [num,3,H,W] float32, written to inputs_llama_dev [num, qf_queries, proj_dim] float32 -- the
 * tensor MiniGPTBase.generate splices into the LLM prompt (minigpt_base.py:401-405; `atts_llama` is all ones, minigpt4.py:148,
 * and is not materialised).  Any num >= 0 (internally cut into batches of max_batch); CGPT_MODE_ENCODE_IMG handles only
 * (CGPT_ERR_STATE otherwise); no host sync.  The build-side label head is not evaluated. */
cgpt_status cgpt_encode_img(cgpt_handle h, const float* images_dev, int64_t num, float* inputs_llama_dev, void* stream);
/* The same for the Monte-Carlo draws of Smooth._sample_noise (smoothing.py:95-97 with a generating base classifier):
 * row b of inputs_llama_dev is encode_img(x + sigma * eps_{first_sample + b}); the noise is generated inside the patch-embed
 * operand as in cgpt_sample_counts, so the noisy images never exist in HBM. */
cgpt_status cgpt_encode_img_noisy(cgpt_handle h, const float* x_dev, int64_t first_sample, int64_t num, float sigma,
                                  uint64_t noise_seed, float* inputs_llama_dev, void* stream);
/* Intermediate activations of the last cgpt_forward_logits / cgpt_classify call, as float32, for parity tests:
 * what = "vit_out"   [num, T, vit_dim]   (VisionTransformer.forward_features output, eva_vit.py:349)
 *        "ln_vision" [num, T, vit_dim]   (CGPT_MODE_ENCODE_IMG only; minigpt4.py:129)
 *        "qformer"   [num, Q, qf_dim]    (query_output.last_hidden_state, minigpt4.py:134-139)
 *        "llama"     [num, Q, proj_dim]  (inputs_llama, minigpt4.py:141)                                      */
cgpt_status cgpt_get_activation(cgpt_handle h, const char* what, float* out_dev, int64_t numel, void* stream);

/* ---- pieces of the loop, for callers whose base classifier is not this library's
 *      (e.g. full MiniGPT-4 with a Vicuna decode on PyTorch-ROCm, minigpt_base.py:374-448) ---- */
/* smoothing.py:95-96: out[b] = x + sigma * eps_{first_sample+b}; out_dev is [num,3,H,W] float32.  Handle-free. */
cgpt_status cgpt_noise_batch(const float* x_dev, int64_t chw, int64_t first_sample, int64_t num, float sigma,
                             uint64_t noise_seed, float* out_dev, void* stream);
/* The same under noise law `law` (CGPT_NOISE_*): out[b] = x + scale * eps_{first_sample+b}, rounded exactly as the noisy
 * classifier calls round it (one fma in fp32).  cgpt_noise_batch is this call with CGPT_NOISE_GAUSSIAN.  Handle-free. */
cgpt_status cgpt_noise_batch_law(const float* x_dev, int64_t chw, int64_t first_sample, int64_t num, float scale, int32_t law,
                                 uint64_t noise_seed, float* out_dev, void* stream);
/* One step of the random-gradient-free black-box attack of BASELINE configs[4] (the reference has no code for it, only prose:
 * README.md:62-64,108-120; the rule is this library's): with u_s the N(0,1) image of sample index s of the noise stream (the
 * direction cgpt_noise_batch(x, s, 1, delta, seed) adds),
 *   out = clamp(x_adv + lr * sign(sum_{i<num_dirs} coeffs_host[i] * u_{first_dir+i}), x_clean - eps, x_clean + eps).
 * coeffs_host: num_dirs (1..32) finite-difference coefficients on the HOST; the three images are [chw] float32 on the device
 * (out_dev may alias x_adv_dev).  Handle-free. */
cgpt_status cgpt_rgf_step(const float* x_adv_dev, const float* x_clean_dev, int64_t chw, int64_t first_dir, int32_t num_dirs,
                          const float* coeffs_host, float lr, float eps, uint64_t noise_seed, float* out_dev, void* stream);
/* smoothing.py:97-98,101-105: counts_dev[argmax(logits[b,:])] += 1 for b < num (first max index on ties). */
cgpt_status cgpt_vote(const float* logits_dev, int64_t num, int32_t num_classes, int64_t* counts_dev, void* stream);
/* counts_dev[labels_dev[i]] += 1 for i < num: the vote of rows whose class is already known on the device (int32 labels, the
 * labels_out_dev of cgpt_llm_constrained), into the int64 histogram cgpt_vote fills, with 64-bit atomics.  A label outside
 * 0 .. num_classes-1 is not counted.  Enqueues only. */
cgpt_status cgpt_vote_labels(const int32_t* labels_dev, int64_t num, int32_t num_classes, int64_t* counts_dev, void* stream);

/* ---- the one collective of the path, for callers that are not Python (Python callers use torch.distributed, whose "nccl"
 *      backend IS RCCL on ROCm): in-place sum over all ranks of the int64 vote histograms a cgpt_sample_counts* call produced
 *      on each rank's shard of the sample range -- ncclAllReduce(counts, counts, count, ncclInt64, ncclSum, comm, stream) over
 *      xGMI.  rccl_comm is the caller's ncclComm_t (one process per GPU); count = num_classes for one histogram, or
 *      num_images * 2 * num_classes for the table of cgpt_sample_counts_images.  Enqueued on `stream`, no host sync.
 *      (The reference has no call site: its collectives are torch_xla's)
 *      SAME-INSTANCE REQUIREMENT: a communicator lives inside the RCCL library instance that created it.  libcgpt.so does not
 *      link RCCL and never loads one: cgpt_allreduce_counts binds to the ONE librccl already mapped in the process (whatever its
 *      dlopen flags) and returns CGPT_ERR_STATE when none or more than one is mapped (e.g. torch's bundled copy next to
 *      /opt/rocm's); in that case, or whenever you hold the pointer anyway, pass the ncclAllReduce of the library that created
 *      rccl_comm to cgpt_allreduce_counts_fn.  Stateless and callable from any thread. ---- */
cgpt_status cgpt_allreduce_counts(void* rccl_comm, int64_t* counts_dev, int64_t count, void* stream);
cgpt_status cgpt_allreduce_counts_fn(void* nccl_allreduce, void* rccl_comm, int64_t* counts_dev, int64_t count, void* stream);

/* ---- statistics: pure host functions, float64, no device needed ----
 * Smooth.certify lines 46-56 given the two histograms (smoothing.py:44,48). */
cgpt_status cgpt_certify_from_counts(const int64_t* counts_selection, const int64_t* counts_estimation,
                                     int32_t num_classes, int64_t n, double alpha, double sigma,
                                     int32_t* label_out, double* radius_out);
/* The same for a table of histograms counts[num_images][2][num_classes] (selection then estimation per image: what
 * cgpt_sample_counts_images fills), one call for the group of images of Smooth.certify_many: image i gets exactly what
 * cgpt_certify_from_counts gives for its two rows (the per-image Python round trips were 70 us per image of host time in which the
 * GPU idles: 3 % of a rank's time at 8 GPUs). */
cgpt_status cgpt_certify_many_from_counts(const int64_t* counts, int64_t num_images, int32_t num_classes, int64_t n, double alpha,
                                          double sigma, int32_t* labels_out, double* radii_out);
/* The same under noise law `law` (CGPT_NOISE_*) with noise scale `scale`: the radius is scale * Phi^-1(pA_lower) (L2, Gaussian)
 * or scale * (pA_lower - 1/2) (L1, uniform); labels and the abstain rule (pA_lower < 1/2) do not depend on the law.  One image is
 * num_images = 1.  cgpt_certify_from_counts and cgpt_certify_many_from_counts are this function with CGPT_NOISE_GAUSSIAN. */
cgpt_status cgpt_certify_many_from_counts_law(const int64_t* counts, int64_t num_images, int32_t num_classes, int64_t n, double alpha,
                                              double scale, int32_t law, int32_t* labels_out, double* radii_out);
/* Smooth.predict lines 73-79 given the histogram (smoothing.py:72). */
cgpt_status cgpt_predict_from_counts(const int64_t* counts, int32_t num_classes, double alpha, int32_t* label_out);
/* The same two decisions computed ON THE DEVICE from device histograms (no histogram copy, no host sync): one wavefront,
 * arg-max / top-2 by xor-shuffles, Clopper-Pearson bound, binomial test and Phi^-1 in float64 with the same code as the
 * host functions.  out2_dev[0] = label (-1 = abstain) as a double, out2_dev[1] = radius (certify) or p-value (predict). */
cgpt_status cgpt_certify_device(const int64_t* counts_selection_dev, const int64_t* counts_estimation_dev, int32_t num_classes,
                                int64_t n, double alpha, double sigma, double* out2_dev, void* stream);
/* cgpt_certify_device under noise law `law` (CGPT_NOISE_*), radius as in cgpt_certify_many_from_counts_law. */
cgpt_status cgpt_certify_device_law(const int64_t* counts_selection_dev, const int64_t* counts_estimation_dev, int32_t num_classes,
                                    int64_t n, double alpha, double scale, int32_t law, double* out2_dev, void* stream);
cgpt_status cgpt_predict_device(const int64_t* counts_dev, int32_t num_classes, double alpha, double* out2_dev, void* stream);
/* Smooth._lower_confidence_bound (smoothing.py:107-117) == statsmodels proportion_confint(NA,N,2*alpha,"beta")[0]. */
double cgpt_lower_confidence_bound(int64_t NA, int64_t N, double alpha);
/* scipy.stats.binom_test(x, n, p) two-sided (scipy 1.7 algorithm; call site smoothing.py:76). */
double cgpt_binom_test(int64_t x, int64_t n, double p);
/* scipy.stats.norm.ppf (call site smoothing.py:55). */
double cgpt_norm_ppf(double p);

/* ---- measurement hooks (bench.py roofline) ----
 * When enabled, every GEMM launch is bracketed by HIP events on the launch stream; totals are read back with
 * cgpt_profile_read (which synchronises those events).  kind: 0 = all GEMMs (reading it drains the log), 1 = the ViT MLP fc1
 * (GELU epilogue) GEMMs only, 2 = ViT qkv, 3 = ViT attention proj, 4 = ViT MLP fc2. */
cgpt_status cgpt_profile_enable(cgpt_handle h, int32_t on);
cgpt_status cgpt_profile_read(cgpt_handle h, int32_t kind, double* total_ms, double* total_flops, int64_t* launches);
/* The shader clock the profiled GEMMs of `kind` (as above; 0 = all) actually ran at: every workgroup of the 256-row kernels reads
 * s_memtime and s_memrealtime at its first and last instruction while profiling is on; clock_ghz = sum of cycles / sum of 100-MHz
 * ticks x 0.1 (0 when nothing was profiled).  Synchronises the device.  Read it BEFORE cgpt_profile_read(kind 0), which resets
 * the sums with the log.  For ONE run, frac = (share of cycles in which the matrix pipes issue) x this clock / 2.4 GHz, so a clock
 * give-back shows up here; bench.py prints that share as roofline.implied_mfma_busy_frac.  (roofline.pmc.mfma_busy_frac and .clock_ghz
 * come from a separate rocprofv3 --pmc run, which holds other clocks: never multiply numbers of the two runs.) */
cgpt_status cgpt_profile_clock(cgpt_handle h, int32_t kind, double* clock_ghz);
/* The classifier batches the handle ran since profiling was last switched on, in order: samples (rows of smoothing.py:93-97's `batch`)
 * of every base-classifier forward, i.e. how cgpt_sample_counts* cut their sample ranges (smoothing.py:91-98: `this_batch_size`).
 * *count_out = number of forwards; the first min(count, capacity) sizes are written to samples_out (capacity 0: count only).  Host
 * bookkeeping only, nothing is synchronised.  bench.py prints it per rank, so that a multi-GPU line shows the GEMM shapes it ran. */
cgpt_status cgpt_profile_batches(cgpt_handle h, int32_t* samples_out, int64_t capacity, int64_t* count_out);

/* Process-wide SPEED knobs.  No option changes a result: every accepted value gives bit-identical outputs (tested).
 * THREADING OF THE LIBRARY (not only of a handle): these options AND the per-device first-launch caches of the kernel launchers (LDS
 * attribute + CU count, set on a device's first launch of each kernel) are process-global and unsynchronised.  One thread drives the
 * library until every device in use has run its first forward; afterwards handles on DIFFERENT devices may be driven from different
 * threads (one thread per handle), and options are set only while no launch is in flight.  The supported deployment is the reference's:
 * one process per GPU (launch.py:110-120).
 *   "gemm_kernel": 0 = automatic choice (default); 1 = 128x128 register-staged tile, 3 = 256x128 direct-to-LDS tile,
 *                  4 = 256x256 phase-alternating tile, 14 = 256x256 two-phase quadrant tile with a 1.5-K-tile LDS-DMA run-ahead (the
 *                  automatic choice for M >= 1024 when the shape has more than 128 tiles of 256x256).
 *   "ln_kernel":   MEASUREMENT aid; 1 (default) = the LayerNorm forms the ViT launches (D = 1408, fp16 out, any of the deferred residual adds)
 *                  run the kernel that issues a row's loads before its first use and reads gamma / beta from LDS; 0 = the earlier
 *                  chunk-at-a-time kernel for every form.  Same bits (tests/test_gpu_layernorm_forms.py); tools/layernorm_bench.py
 *                  times both in one process.
 *   "gemm_ablate": TEST-ONLY bit mask; each bit turns ONE optimisation of the 256x256 kernels off without changing a result, so that
 *                  the test suite can check that the bits do not depend on it: 512 = LDS-transposed fp16 epilogue, 16384 = 192-column
 *                  last tiles for N = 256k+128.  Any other bit is rejected with CGPT_ERR_INVALID.  Process-global and unsynchronised: set it only while no launch is in flight.
 *   "gemm_grid":   0 (default) = one workgroup of the persistent 256x256 GEMM per CU; n > 0 (a multiple of 8) = at most n workgroups, i.e.
 *                  CUs left free for kernels of another stream (tools/two_stream_probe.py; measured: no split beats the default).
 *   "sync_batches": MEASUREMENT aid; 1 = cgpt_sample_counts* wait for the stream after every classifier batch (a --pmc profiler keeps a
 *                  record per in-flight dispatch and one call can enqueue tens of thousands: profiles/r06/pmc_sigsegv.txt); 0 (default) =
 *                  nothing is synchronised.  It stays in the shipped library on purpose: counters must be taken on the binary that ships.
 *   "trace_batches": MEASUREMENT aid; 1 = one stderr line per classifier batch the cgpt_sample_counts* entry points enqueue; 0 (default).
 * (A lab build of the library -- make LAB=1, never shipped -- additionally accepts the experimental schedules 2, 5..11, 15 and
 * timing-study switches that skip work; profiles/r01/gemm_variants.txt.) */
cgpt_status cgpt_set_option(const char* key, int32_t value);

/* Measurement aid (no counterpart in the reference): the dense fp16 MFMA rate THIS device sustains on random operands when it does nothing
 * else -- v_mfma_f32_16x16x32_f16 back to back from registers for `seconds` (clock settled first), in TFLOP/s, and the in-kernel shader
 * clock in GHz.  The data sheet's 2.5 PFLOP/s assumes 2.4 GHz; under an MFMA-dense load an MI355X holds 1.8-1.95 GHz, so bench.py reports
 * a kernel's fraction of the data-sheet peak AND of this rate (profiles/r04/mfma_sustained.txt).  Synchronous; runs on the null stream of
 * the CURRENT device: select the device first (hipSetDevice / torch.cuda.set_device).  Every HIP call inside is checked: a failed launch,
 * a zero elapsed time or an unwritten clock buffer returns an error (outputs 0), never a number. */
cgpt_status cgpt_mfma_sustained(double seconds, double* tflops_out, double* clock_ghz_out);

/* ---- raw kernels exported for unit tests and reuse (all fp16 operands are IEEE binary16) ----
 * C[M,N] = A[M,K] * W[N,K]^T (+ bias[N]) ; A row stride lda, W row stride ldw (elements), fp32 accumulate.
 * Requirements: A must be readable for ceil(M/256)*256 rows and W for ceil(N/256)*256 rows (zero padded; the
 * library's own buffers always are); K%64==0.  out is fp32 [M,ldc]. */
cgpt_status cgpt_gemm_f16(const void* A_dev, int64_t lda, const void* W_dev, int64_t ldw, const float* bias_dev,
                          float* C_dev, int64_t ldc, int64_t M, int64_t N, int64_t K, void* stream);
/* nn.Linear with a fused epilogue: 0 = fp16 out (acc + bias), 1 = fp16 out gelu_erf(acc + bias), 2 = fp32 out,
 * 3 = fp32 out = aux + acc + bias (aux may alias out: the residual add x = x + f(x), eva_vit.py:180-181). */
cgpt_status cgpt_linear_f16(const void* A_dev, int64_t lda, const void* W_dev, int64_t ldw, const float* bias_dev,
                            void* out_dev, int64_t ldo, const float* aux_dev, int64_t ldaux, int64_t M, int64_t N, int64_t K,
                            int32_t epilogue, void* stream);
/* softmax(scale * Q K^T) V per (batch, head): Q [B,Tq,ldq] K,V [B,Tk,ldkv] fp16 with head h at column h*head_dim;
 * O [B,Tq,ldo] fp16.  head_dim in {64, 88}.  (eva_vit.py:133-150; Qformer.py:244-264 with zero masks)
 * Tk <= 288: K/V of a head resident in LDS; Tk > 288 (448^2 images): K/V streamed in 288-key chunks, online softmax. */
cgpt_status cgpt_attention_f16(const void* Q_dev, int64_t ldq, const void* K_dev, const void* V_dev, int64_t ldkv,
                               void* O_dev, int64_t ldo, int32_t B, int32_t heads, int32_t head_dim,
                               int32_t Tq, int32_t Tk, float scale, void* stream);
/* y = LayerNorm(x) * gamma + beta over the last dim D (fp32 statistics), x fp32 [rows, ldx] -> y fp16 [rows, ldy]
 * (and optionally y32 fp32 [rows, ldy32] when y32_dev != NULL).  (eva_vit.py:162,168; base_model.py:281-287) */
cgpt_status cgpt_layernorm(const float* x_dev, int64_t ldx, const float* gamma_dev, const float* beta_dev, float eps,
                           void* y_dev, int64_t ldy, float* y32_dev, int64_t ldy32, int64_t rows, int32_t D,
                           void* stream);
/* The same LayerNorm with the ViT blocks' deferred residual adds (eva_vit.py:180-181), as the forward launches it:
 * v = (x + delta) + delta2 in fp32 (delta_dev / delta2_dev: fp16 [rows, ldd] / [rows, ldd2], either may be NULL), y = LayerNorm(v);
 * unless keep_x != 0, v is written back to x when at least one update is given.  y16_dev (fp16) and y32_dev (fp32): at least one.
 * CGPT_ERR_INVALID: null x / gamma / beta, both outputs null, rows < 0, D <= 0, odd or above 4096, an odd leading dimension, or a
 * leading dimension of a given operand below D.  Rows of x / delta / delta2 must be 4-byte aligned (even strides); the 16-byte
 * kernels run when D % 128 == 0 and every stride is a multiple of 4. */
cgpt_status cgpt_layernorm_resid(float* x_dev, int64_t ldx, const void* delta_dev, int64_t ldd, const void* delta2_dev, int64_t ldd2,
                                 int32_t keep_x, const float* gamma_dev, const float* beta_dev, float eps, void* y16_dev, int64_t ldy16,
                                 float* y32_dev, int64_t ldy32, int64_t rows, int32_t D, void* stream);

/* ---- LLaMA decode steps and prefill (replaces: the forwards inside `self.llama_model.generate(...)`,
 *      minigpt_base.py:418-431 -- greedy, one new token per row, K/V cache) ----
 * A decoder is not a cgpt_model: it has its own handle.  Supported architecture (checked by cgpt_llm_create BEFORE any device
 * call): HF LlamaForCausalLM in fp16 -- bias-free linears, RMSNorm, rotate_half rotary with the default (unscaled) rope_theta
 * law, kv_heads == heads (with cgpt_llm_config_gqa.grouped_kv = 1: grouped-query attention, heads / kv_heads in {1, 2, 4, 8}, see
 * below), head_dim == 128, hidden == heads * 128, SwiGLU MLP; hidden, mlp and vocab multiples of 64; max_batch <= 256 (one GEMM
 * row tile); max_len <= 8192 (positions the rotary table covers).  That is Vicuna-7B / 13B, and with grouped_kv = 1 the
 * Llama-3-8B (32 / 8 heads) and Llama-2-70B (64 / 8) shapes.  The step entries work on the caller's K/V buffers in place, layout
 * [B, heads, kv_len_stride, 128] fp16 per layer ([B, kv_heads, kv_len_stride, 128] on a grouped_kv = 1 handle), rows 0 .. pos-1
 * filled by the prefill.  The prefill is either the caller's (the model's own forward writes
 * those rows) or cgpt_llm_prefill: the same layers on B x L token rows in this library's kernels, filling the same buffers.
 * Rounding: where HF's fp16 eager model rounds ("LLaMA decode steps"); split-K partial sums are combined in slice
 * order, so results are bit-identical from launch to launch and a row's result does not depend on the batch around it.
 * All work is enqueued on `stream`; no host sync, no allocation and no host->device copy after create: capturable in a graph
 * without a warm-up call (kernel attributes are set by create).  The step entries select the handle's device.  A handle owns ONE
 * step workspace: one stream at a time per handle -- calls on two streams must be ordered by the caller. */
typedef struct cgpt_llm_config {
    int32_t struct_size;      /* = sizeof(cgpt_llm_config)                                         */
    int32_t device;           /* HIP device ordinal                                                */
    int32_t hidden;           /* 4096 (Vicuna-7B)                                                  */
    int32_t layers;           /* 32                                                                */
    int32_t heads;            /* 32                                                                */
    int32_t kv_heads;         /* must equal heads unless grouped_kv = 1                            */
    int32_t head_dim;         /* must be 128                                                       */
    int32_t mlp;              /* 11008 (intermediate_size)                                         */
    int32_t vocab;            /* 32000                                                             */
    float   rms_eps;          /* 1e-5 / 1e-6 (config.rms_norm_eps)                                 */
    float   rope_theta;       /* 10000                                                             */
    int32_t max_batch;        /* rows of a step, <= 256                                            */
    int32_t max_len;          /* positions (prompt + new tokens) the rotary table covers           */
    int32_t weight_format;    /* CGPT_LLM_W_F16 (0) | CGPT_LLM_W_INT8 (1): how the layer linears are held; read only when
                                 struct_size covers it -- a caller that passes the size up to max_len gets fp16 */
} cgpt_llm_config;

/* The extended config: a cgpt_llm_config followed by the switches added after weight_format.  A caller that wants one of them fills
 * this struct, sets base.struct_size = sizeof(cgpt_llm_config_gqa) and passes &cfg.base to cgpt_llm_create, which tells the two
 * apart by struct_size alone.  cgpt_llm_config itself keeps its fields and its two sizes (the whole struct, the struct up to
 * max_len), so sizeof(cgpt_llm_config) + 4 stays what it has always been: header / library drift, refused.  That is why the
 * extension is 8 bytes: `reserved` must be 0 (anything else is CGPT_ERR_INVALID) and is room for the next switch. */
typedef struct cgpt_llm_config_gqa {
    cgpt_llm_config base;     /* base.struct_size = sizeof(cgpt_llm_config_gqa)                    */
    int32_t grouped_kv;       /* 0 | 1: grouped-query attention (below)                            */
    int32_t reserved;         /* must be 0                                                         */
} cgpt_llm_config_gqa;

/* cgpt_llm_config_gqa.grouped_kv = 1: grouped-query attention.  Requires 1 <= kv_heads <= heads, heads % kv_heads == 0 and
 * G = heads / kv_heads in {1, 2, 4, 8}; query head h reads K/V head h / G (HF's repeat_kv).  The switch is explicit because the
 * caller owns the K/V buffers: on such a handle EVERY entry that takes k_ptrs_host / v_ptrs_host reads and writes caches laid out
 * [B, kv_heads, kv_len_stride, 128] -- 1 / G of the bytes -- and a caller that sized or indexed them by `heads` must say that it
 * knows.  k_proj / v_proj are loaded as [kv_heads * 128, hidden] (HF's shapes).  The token step's attention keeps G score arrays of
 * max_len floats in LDS: a (G, max_len) pair that does not fit the CU's 160 KiB (G = 8 with max_len > 4464) is CGPT_ERR_INVALID
 * at create.  grouped_kv = 0 (or a plain cgpt_llm_config, which has no such field) is the handle as it was, CGPT_ERR_INVALID for
 * kv_heads != heads included; any other value of the field is CGPT_ERR_INVALID.
 * Rounding and summation orders per query head are those of the plain handle, with one consequence of the narrower fused q/k/v
 * projection: the decode GEMM's K split depends on N, so at hidden 4096 the grouped N = 6144 runs 2 K slices where the expanded
 * (repeat_interleave'd) twin's N = 12288 runs 1 -- two valid summation orders, not bit-equal. */

/* cgpt_llm_config.weight_format.
 * CGPT_LLM_W_INT8 (W8A16): the seven linears of every layer are held as row-wise absmax int8, one fp16 scale per output row
 * (the weight law of bitsandbytes' load_in_8bit; activations stay fp16 and there is no outlier decomposition unless
 * cgpt_llm_config_act.act_format = 1, below -- parity with LLM.int8()'s forward is NOT pinned).  For row n of an nn.Linear.weight [N, K]:  s_n = fp16(absmax_k |w_nk| / 127), the division in fp32;
 * q_nk = clamp(rint(fp32(w_nk) / fp32(s_n)), -127, 127), round to nearest even, q = 0 where s_n = 0;  W'_nk = fp16(q_nk) * s_n,
 * ONE fp16 multiply.  Every result of an int8 handle is bit for bit the result of an fp16 handle whose layer linears were loaded
 * with W'.  lm_head, embed_tokens and the RMSNorm weights stay fp16. */
#define CGPT_LLM_W_F16 0
#define CGPT_LLM_W_INT8 1

typedef struct cgpt_llm* cgpt_llm_handle;

/* Allocates the library's own weight copies (fused q/k/v and gate/up, 2 bytes per parameter: 13.5 GB MORE HBM at 7B, beside the
 * HF module's; CGPT_LLM_W_INT8: 1 byte per layer-linear parameter, the row scales and ONE fp16 scratch matrix of the largest fused
 * layer matrix for the prefill, 7.2 GB at 7B) and the step workspace.  CGPT_ERR_INVALID for an unsupported config, a struct_size
 * that is none of the valid ones (cgpt_llm_config_act, cgpt_llm_config_gqa, the whole cgpt_llm_config, cgpt_llm_config up to max_len),
 * or an unknown weight_format / grouped_kv / act_format; CGPT_ERR_NO_DEVICE without a GPU. */
cgpt_status cgpt_llm_create(const cgpt_llm_config* cfg, cgpt_llm_handle* out);
cgpt_status cgpt_llm_destroy(cgpt_llm_handle h);
/* Device-to-device copy of one fp16 parameter of the HF module under its state_dict name: "model.embed_tokens.weight",
 * "model.layers.<i>.self_attn.{q,k,v,o}_proj.weight", "model.layers.<i>.mlp.{gate,up,down}_proj.weight",
 * "model.layers.<i>.{input,post_attention}_layernorm.weight", "model.norm.weight", "lm_head.weight" (contiguous, PyTorch shape:
 * k_proj / v_proj are [kv_heads * 128, hidden]; numel must match).  Enqueued on `stream`.  The step entries return CGPT_ERR_STATE until every name has been loaded. */
cgpt_status cgpt_llm_load_weight_f16(cgpt_llm_handle h, const char* name, const void* data_dev, int64_t numel, void* stream);
/* On a CGPT_LLM_W_INT8 handle cgpt_llm_load_weight_f16 of a layer linear is a quantising kernel instead of a copy: it reads the
 * caller's fp16 rows and writes int8 rows and their scales into the fused matrix (rows keep their scales through the q/k/v fusion
 * and the gate/up interleave); no fp16 copy of the layer survives the call.  The other names are copied as above.
 * cgpt_llm_weight_bytes: *out = the bytes this handle holds for weight matrices (embed_tokens, lm_head and the layer linears with
 * their padding to 256-row tiles), row scales and the dequantisation scratch (none with act_format = 1), as allocated -- the
 * library's own accounting: embed + lm_head (2 V H bytes) + per layer, for each fused matrix [N, K], up256(N) K (int8) + 2 up256(N)
 * (scales), or 2 up256(N) K (fp16); + the scratch, 2 max(up256(N) K) bytes, on an int8 handle with act_format = 0 only.  The
 * RMSNorm vectors, the rotary table and the step / prefill workspaces are not counted. */
cgpt_status cgpt_llm_weight_bytes(cgpt_llm_handle h, int64_t* out);
/* One token step: row b feeds token tokens_dev[b] (int64) at position `pos`; layer l appends its rotated key and its value to
 * row `pos` of k_ptrs_host[l] / v_ptrs_host[l] (device buffers [B, heads, kv_len_stride, 128] fp16, [B, kv_heads, kv_len_stride, 128]
 * on a grouped_kv = 1 handle -- at this and every other entry that takes the tables; the two tables are HOST
 * arrays of `layers` device pointers, read when the call enqueues) and attends over rows 0 .. pos.  No other cache row is
 * written.  logits_dev: [B, vocab] fp32 (fp16-rounded values, as HF's `.float()` of fp16 logits).  Tests drive this entry
 * teacher-forced. */
cgpt_status cgpt_llm_step(cgpt_llm_handle h, const int64_t* tokens_dev, int32_t B, int32_t pos, void* const* k_ptrs_host,
                          void* const* v_ptrs_host, int64_t kv_len_stride, float* logits_dev, void* stream);
/* The greedy loop after a prefill of prompt_len positions whose last-position logits are first_logits_dev [B, vocab] fp32 (not
 * modified): num_new x select, with num_new - 1 steps between them, all enqueued by this one call.  Select = HF greedy search:
 * the num_eos ids of eos_ids_host (<= 8) read as -inf on the first min_new tokens, first-max arg-max, pad_id for a row that has
 * produced an EOS.  tokens_out_dev: [B, num_new] int64.  step_logits_out_dev (or NULL): [B, num_new, vocab] fp32, the logits each
 * arg-max was taken on (EOS columns at -inf where suppressed).  K/V layout as cgpt_llm_step (grouped_kv = 1: kv_heads heads). */
cgpt_status cgpt_llm_greedy(cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t prompt_len, int32_t num_new,
                            int32_t min_new, const int64_t* eos_ids_host, int32_t num_eos, int64_t pad_id, void* const* k_ptrs_host,
                            void* const* v_ptrs_host, int64_t kv_len_stride, int64_t* tokens_out_dev, float* step_logits_out_dev,
                            void* stream);

/* Workspace of cgpt_llm_prefill for up to max_rows prompts of up to max_prompt_len positions: max_rows x max_prompt_len token rows,
 * padded to whole 256-row GEMM tiles and zeroed -- residual stream, normalised rows, fused q/k/v, attention output, projection
 * output, gate/up product, SwiGLU output: (8 hidden + 3 mlp) x 2 bytes per token row, 1.2 GB at 200 x 44 rows of a 7B decoder.
 * Synchronises and allocates: call it OUTSIDE any stream capture.  Idempotent; grows only (a smaller request changes nothing).
 * Growth never invalidates an earlier capture: a graph captured on the smaller workspace keeps replaying on it, because replaced
 * buffers stay allocated until cgpt_llm_destroy (their bytes are the price: reserve once for the largest shape to avoid it).  A
 * failed growth (CGPT_ERR_HIP) leaves the workspace the handle had.
 * CGPT_ERR_INVALID for max_rows outside 1..max_batch or max_prompt_len outside 1..max_len. */
cgpt_status cgpt_llm_prefill_reserve(cgpt_llm_handle h, int32_t max_rows, int32_t max_prompt_len);
/* The prefill of B prompts of L positions each (no padding, positions 0 .. L-1, causal): embeds_dev is [B, L, hidden] fp16,
 * contiguous.  Layer l writes its rotated keys and its values to rows 0 .. L-1 of k_ptrs_host[l] / v_ptrs_host[l] (layout and
 * tables as cgpt_llm_step, [B, kv_heads, kv_len_stride, 128] on a grouped_kv = 1 handle; no other cache row is written); logits_dev receives the LAST position's logits, [B, vocab] fp32
 * (fp16-rounded values).  Rounding as the step entries, except that the attention probabilities are rounded to fp16 as the
 * matrix-core operand of P.V.  Enqueues only: no host sync, no allocation, no host->device copy -- capturable.
 * CGPT_ERR_STATE while weights are missing or when B x L exceeds the reserved workspace; CGPT_ERR_INVALID for B outside
 * 1..max_batch, L < 1, L > kv_len_stride, L > max_len or a null table / buffer; all checked before the first launch. */
cgpt_status cgpt_llm_prefill(cgpt_llm_handle h, const void* embeds_dev, int32_t B, int32_t L, void* const* k_ptrs_host,
                             void* const* v_ptrs_host, int64_t kv_len_stride, float* logits_dev, void* stream);

/* ---- Left-padded prompts: the three entries above with a per-row start offset ----
 * starts_dev is a DEVICE array of B int32.  Row b of a batch padded to L positions has start[b] pad positions at buffer positions
 * 0 .. start[b]-1 and its len[b] = L - start[b] >= 1 real tokens at start[b] .. L-1 (HF's left padding: the first real token sits at
 * rotary position 0).  The kernels clamp start[b] into 0 .. L-1 (cgpt_llm_step_ragged, which is not told L: 0 .. pos): the host cannot check device
 * contents without a sync.  They work in row-relative coordinates -- the row's q / k / v, cache and output pointers moved by
 * start[b], the plain entries' arithmetic on len[b] positions -- so a padded row's logits, tokens and cache rows
 * start[b] .. are bit for bit those of the same row run unpadded through the plain entries (cache rows 0 ..).
 * Cache rows written: the prefill writes rows start[b] .. L-1 of row b, a step at `pos` writes row `pos`; rows below start[b] are
 * NEVER written or read.  embeds_dev holds all B x L rows; pad rows go through the row-independent kernels and GEMMs like any other
 * row (the price of left padding), so their embeds must be finite (zeros stay zeros); pad rows of the attention output are zeros.
 * starts_dev is read when the kernels RUN, not when the call enqueues: a captured graph sees the array's current contents at each
 * replay, so one graph per (B, L) serves every mix of prompt lengths.  All three calls of one decode must see the same contents.
 * Same contracts as the plain entries (enqueue only, capturable, CGPT_ERR_STATE / CGPT_ERR_INVALID rules, all checks before the
 * first launch; the workspace is cgpt_llm_prefill_reserve's, for B x L rows), plus CGPT_ERR_INVALID for a null starts_dev.
 * K/V layout as the plain entries: [B, heads, kv_len_stride, 128], [B, kv_heads, kv_len_stride, 128] on a grouped_kv = 1 handle.
 * cgpt_llm_greedy_ragged: prompt_len is the PADDED length L; its steps run at buffer positions L, L + 1, ... */
cgpt_status cgpt_llm_prefill_ragged(cgpt_llm_handle h, const void* embeds_dev, int32_t B, int32_t L, const int32_t* starts_dev,
                                    void* const* k_ptrs_host, void* const* v_ptrs_host, int64_t kv_len_stride, float* logits_dev,
                                    void* stream);
cgpt_status cgpt_llm_step_ragged(cgpt_llm_handle h, const int64_t* tokens_dev, int32_t B, int32_t pos, const int32_t* starts_dev,
                                 void* const* k_ptrs_host, void* const* v_ptrs_host, int64_t kv_len_stride, float* logits_dev,
                                 void* stream);
cgpt_status cgpt_llm_greedy_ragged(cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t prompt_len,
                                   const int32_t* starts_dev, int32_t num_new, int32_t min_new, const int64_t* eos_ids_host,
                                   int32_t num_eos, int64_t pad_id, void* const* k_ptrs_host, void* const* v_ptrs_host,
                                   int64_t kv_len_stride, int64_t* tokens_out_dev, float* step_logits_out_dev, void* stream);

/* ---- Continuation prefill: Ln positions on top of a cache that already holds the pos0 positions before them ----
 * cgpt_llm_prefill_from is cgpt_llm_prefill for positions pos0 .. pos0+Ln-1 of every row: embeds_dev is [B, Ln, hidden] fp16 (the NEW
 * positions only), rows 0 .. pos0-1 of every layer's K / V buffer MUST ALREADY HOLD the row's keys and values (an earlier
 * cgpt_llm_prefill / cgpt_llm_prefill_from / steps, or cgpt_llm_kv_broadcast below); layer l writes rows pos0 .. pos0+Ln-1 and no
 * other cache row; logits_dev receives the logits of position pos0+Ln-1, [B, vocab] fp32.  The attention tiles the queries by their
 * absolute position, so logits and cache rows are bit for bit those of cgpt_llm_prefill on the whole prompt of pos0+Ln positions
 * (DESIGN.md 4.4.11): a prompt may be prefilled in chunks with a workspace reserved for B x Ln rows, or a turn appended to an
 * earlier turn's cache.  pos0 = 0 is cgpt_llm_prefill (cgpt_llm_prefill_ragged with starts_dev).
 * starts_dev (or NULL: no padding) is the left padding of the Ln-position buffer, clamped into 0 .. Ln-1: row b's pad positions
 * 0 .. start[b]-1 are left alone (not rotated, not written to the cache, attention output zeros), its real position j >= start[b] is
 * rotated at pos0 + (j - start[b]) and written to cache row pos0 + j.  The row's cache is then [start[b] rows never touched]
 * [pos0 earlier rows at start[b] .. start[b]+pos0-1][its real new rows]: the layout cgpt_llm_prefill_ragged gives the whole prompt
 * of pos0+Ln buffer positions under the same starts, so the _ragged step / greedy / sample / score entries follow with
 * prompt_len = pos0+Ln and the same starts_dev.  Read when the kernels run.
 * Contracts of cgpt_llm_prefill: enqueues only, no allocation, no host sync, capturable; the workspace is
 * cgpt_llm_prefill_reserve's, for B x Ln rows.  CGPT_ERR_INVALID for a null handle, table or buffer, B outside 1..max_batch, Ln < 1,
 * pos0 < 0, pos0+Ln > kv_len_stride or pos0+Ln > max_len; CGPT_ERR_STATE while weights are missing or the reservation is too small;
 * all checked before the first launch. */
cgpt_status cgpt_llm_prefill_from(cgpt_llm_handle h, const void* embeds_dev, int32_t B, int32_t pos0, int32_t Ln, const int32_t* starts_dev,
                                  void* const* k_ptrs_host, void* const* v_ptrs_host, int64_t kv_len_stride, float* logits_dev,
                                  void* stream);
/* Copies a prefix that B rows share into each of them: rows 0 .. P-1 of every head of the ONE-row caches src_k_ptrs_host[l] /
 * src_v_ptrs_host[l] ([1, kv_heads, src_len_stride, 128], e.g. what cgpt_llm_prefill with B = 1 left) go to rows s_b .. s_b+P-1 of
 * every row b of dst_k_ptrs_host[l] / dst_v_ptrs_host[l] ([B, kv_heads, dst_len_stride, 128]), for every layer; s_b = 0 with a NULL
 * starts_dev, otherwise start[b] clamped into 0 .. dst_len_stride-P (read when the kernels run).  No other cache row is written.
 * One launch per layer, 16-byte loads and stores.  Followed by cgpt_llm_prefill_from(pos0 = P) with the same starts_dev it gives
 * the cache of the whole prompt.  Enqueues only, capturable, needs no workspace and no weights.  CGPT_ERR_INVALID for a null handle,
 * table or buffer, B outside 1..max_batch, P < 1, P > src_len_stride, P > dst_len_stride or P > max_len. */
cgpt_status cgpt_llm_kv_broadcast(cgpt_llm_handle h, void* const* src_k_ptrs_host, void* const* src_v_ptrs_host, int64_t src_len_stride,
                                  int32_t P, int32_t B, const int32_t* starts_dev, void* const* dst_k_ptrs_host,
                                  void* const* dst_v_ptrs_host, int64_t dst_len_stride, void* stream);

/* ---- Early stop: the greedy entries do no work once every row has produced an EOS ----
 * cgpt_llm_set_early_stop(h, 1): handle state, read when cgpt_llm_greedy / cgpt_llm_greedy_ragged ENQUEUE (as cgpt_set_noise_law is):
 * a captured graph keeps the setting it was captured under, whatever the handle says at replay.  Off (0) is the state after
 * cgpt_llm_create, and with it both entries are exactly what they were.  CGPT_ERR_INVALID for a null handle or a value other than 0 / 1.
 * With early stop on, a one-workgroup reduction after every select writes `live` = "some row is unfinished" to the handle, and
 * every kernel of the token steps that follow reads it first and returns when it is 0: after the select at which the last unfinished
 * row produces an EOS, the remaining steps of the call stream no weight byte, read and append no K / V row and write no logits; the
 * remaining selects write pad_id without looking at any logits.  The call still enqueues every launch (a dead step costs its
 * launches and nothing else), so it has no host sync, no allocation and no host->device copy, stays capturable, and ONE capture
 * serves every finishing step.  The tokens are, bit for bit, those of the same call with early stop off.
 * live_steps = the number of token steps of the call that ran = min(F, num_new - 1), F = the first select at which no row is left
 * unfinished (num_new if there is none; with num_eos == 0 nothing ever stops).  The dead part of a call, with early stop on:
 *   - cache rows prompt_len + live_steps .. of k_ptrs_host[l] / v_ptrs_host[l] are NOT written (rows below are, as without it);
 *   - rows [.., i, ..] of step_logits_out_dev for selects i > live_steps are NOT written (rows i <= live_steps are, as without it);
 *   - tokens_out_dev is fully written.
 * cgpt_llm_step, cgpt_llm_step_ragged, the prefill entries and cgpt_llm_score never look at the setting.
 * cgpt_llm_live_steps: SYNCHRONISES `stream`, then *out_host = live_steps of the greedy call this handle enqueued last (on that
 * stream).  Not capturable: call it outside any capture.  After a call with early stop on the value is read from the device, so after
 * replays of a graph that captured such a call it is the last replay's; after a call with early stop off it is num_new - 1 (every
 * step runs), kept on the host when the call enqueues.  0 before any greedy call.  CGPT_ERR_INVALID for a null argument. */
cgpt_status cgpt_llm_set_early_stop(cgpt_llm_handle h, int32_t on);
cgpt_status cgpt_llm_live_steps(cgpt_llm_handle h, int32_t* out_host, void* stream);

/* ---- Stop sequences: a row of the greedy entries also finishes when its generated tokens end in one of them ----
 * Replaces: `StoppingCriteriaSub` (conversation.py:96-107) behind `MiniGPTBase.generate(..., stop_words_ids=...)`
 * (minigpt_base.py:387-394), with one deviation: the reference's criterion fires only when ALL rows end in a sequence at the same
 * step; here every row finishes on its own, as it does on an EOS id.
 * cgpt_llm_set_stop_sequences(h, ids_host, lens_host, n): n sequences, sequence s of lens_host[s] token ids, the ids of all
 * sequences one after the other in ids_host (sum of lens_host entries).  Handle state, read when cgpt_llm_greedy /
 * cgpt_llm_greedy_ragged ENQUEUE (as cgpt_llm_set_early_stop is): the arrays are copied by this call, the sequences travel to the
 * select kernel by value, and a captured graph keeps the set it was captured under.  n = 0 clears the set, which is the state after
 * cgpt_llm_create; with it both entries launch exactly what they launched before this entry existed.
 * The rule: row b finishes at select i when token i is an EOS id (as before) or when, for a sequence s of length len <= i + 1,
 * tokens i-len+1 .. i of the row equal s.  Only tokens the call generated are compared (the prompt is embeddings), so a sequence
 * longer than i + 1 cannot match at select i.  min_new masks the EOS logits only: it never suppresses a match.  The finishing
 * tokens stay in tokens_out_dev; later columns hold pad_id.  The tokens are, bit for bit, those of the same call without sequences
 * with everything after each row's finishing column replaced by pad_id, and the step logits of every select up to a row's
 * finishing column are that call's.  A finished row counts as finished for early stop and cgpt_llm_live_steps.
 * cgpt_llm_step, cgpt_llm_step_ragged, the prefill entries and the scoring entries never see the sequences.
 * CGPT_ERR_INVALID, before any device call and leaving the handle's set as it was: a null handle, n outside 0..8, a length outside
 * 1..8, a negative id, null arrays with n > 0. */
cgpt_status cgpt_llm_set_stop_sequences(cgpt_llm_handle h, const int64_t* ids_host, const int32_t* lens_host, int32_t n);

/* ---- Answer scoring: all candidates of a multiple-choice question on ONE prefilled prompt ----
 * Replaces: `MiniGPTBase.multi_select` (minigpt_base.py:451-467), i.e. `forward(..., reduction='none')` (minigpt_base.py:320-363;
 * modeling_llama.py:101-123) once per candidate: a whole forward over prompt + answer and
 * CrossEntropyLoss(label_smoothing) on `logits.float()`.  Here cgpt_llm_prefill runs once and every candidate is scored on the
 * cache rows it left: candidate c of T_c tokens adds T_c - 1 "tail rows" per prompt row (its tokens 0 .. T_c - 2 at rotary
 * positions prompt_len ..), which run the layers like prefill rows but attend over the prompt's cache rows 0 .. prompt_len-1 and
 * over the rotated keys / values of their own candidate's earlier tail rows.  Those exist in the workspace and on chip only.
 *
 * cgpt_llm_score_reserve: workspace for max_rows prompt rows with up to max_tail_rows tail rows each (sum over the candidates of
 * T_c - 1; at most 64): the prefill workspace grown to max_rows x max_tail_rows token rows where it is smaller, fp16 logits of up
 * to 4096 tail rows (more rows run lm_head and the cross-entropy in chunks) and the per-token losses.  Same rules as
 * cgpt_llm_prefill_reserve: synchronises and allocates, so call it OUTSIDE any capture; idempotent; grows only; replaced buffers
 * stay allocated until cgpt_llm_destroy; a failed growth leaves the handle as it was.  CGPT_ERR_INVALID for max_rows outside
 * 1..max_batch or max_tail_rows outside 1..64. */
cgpt_status cgpt_llm_score_reserve(cgpt_llm_handle h, int32_t max_rows, int32_t max_tail_rows);
/* first_logits_dev: [B, vocab] fp32, the prefill's last-position logits (not modified).  cand_tokens_dev: DEVICE int64 [C, Tmax],
 * row c holding the T_c = cand_lens_host[c] tokens of candidate c (the rest of the row is not read); cand_lens_host: HOST int32 [C],
 * read when the call enqueues.  out_dev[b, c] (fp32 [B, C]) receives the SUM over candidate c's tokens of
 *     ce = lse(z) - (1 - label_smoothing) z[token] - label_smoothing mean(z)
 * with z the fp16 logits widened to fp32 (HF's `logits.float()`), all statistics in fp32: token 0 on first_logits_dev, token j >= 1
 * on the logits of tail row j - 1.  The caller divides (the reference's `.view(B, -1).mean(1)` divides by sequence length - 1).
 * A token id outside 0 .. vocab-1 reads as 0 (the host cannot check device contents without a sync).
 * Reads cache rows 0 .. prompt_len-1 of k_ptrs_host[l] / v_ptrs_host[l] (layout and tables as cgpt_llm_step; kv_heads heads on a
 * grouped_kv = 1 handle) and WRITES NO CACHE ROW:
 * after the call the same cache serves cgpt_llm_greedy or another cgpt_llm_score.  A (row, candidate) result depends on that row's
 * cache and that candidate's tokens only -- not on B, C, the other candidates or their order; fixed summation orders, no atomics.
 * Enqueues only: no host sync, no allocation, no host->device copy (the lengths travel as kernel arguments).
 * CGPT_ERR_INVALID, before any device call: a null handle or pointer, C outside 1..64, Tmax < 1, a length outside 1..Tmax, more than
 * 64 tail rows per prompt row, label_smoothing outside [0, 1), prompt_len < 1, prompt_len + Tmax - 1 > max_len, prompt_len >
 * kv_len_stride, B outside 1..max_batch, a null table / buffer.  CGPT_ERR_STATE while weights are missing or when the call exceeds
 * what cgpt_llm_score_reserve reserved. */
cgpt_status cgpt_llm_score(cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t prompt_len,
                           const int64_t* cand_tokens_dev, const int32_t* cand_lens_host, int32_t C, int32_t Tmax, float label_smoothing,
                           void* const* k_ptrs_host, void* const* v_ptrs_host, int64_t kv_len_stride, float* out_dev, void* stream);

/* ---- Answer scoring with per-row prompts and per-row candidates: cgpt_llm_score on left-padded rows ----
 * The reference's `multi_select` gives every row its own question and its own candidate answers (`answers[c][b]`).  This entry scores
 * them on the cache cgpt_llm_prefill_ragged left: prompt_len is the PADDED length L and starts_dev the DEVICE array of B int32 that
 * prefill saw -- row b has start[b] pad positions and len[b] = L - start[b] >= 1 real ones.  The kernels clamp start[b] into
 * 0 .. L-1 (the host cannot check device contents without a sync) and work in row-relative coordinates: the row's K / V pointers moved
 * by start[b], the walk over the prompt's keys on len[b] keys from the row's first real one, tail row j rotated at len[b] + j.
 * cand_tokens_dev: DEVICE int64 [B, C, Tmax], row (b, c) holding row b's tokens of candidate c.  cand_lens_dev: DEVICE int32 [B, C],
 * row b's real length of candidate c.  cand_lens_host: HOST int32 [C], read when the call enqueues: T_c = the LONGEST length of
 * candidate c over the rows.  The T_c define the tail rows, which are the same for every row (sum over c of T_c - 1, at most 64);
 * a device length is clamped into 1 .. T_c.  A row whose candidate is shorter than T_c still runs its surplus tail rows: they read
 * the table entries behind the real length like any other token (an id outside 0 .. vocab-1 reads as 0; keep them finite ids, e.g.
 * 0), nothing of them reaches a result: a token j >= the row's length is left out of out_dev[b, c].
 * out_dev[b, c] (fp32 [B, C]): the SUM over row b's own tokens of candidate c, the law of cgpt_llm_score.  It is bit for bit what
 * cgpt_llm_prefill + cgpt_llm_score give for row b run alone and unpadded with its own tokens and lengths, and depends on nothing but
 * that row's cache rows start[b] .., its tokens of that candidate and its length -- not on B, C, L, the padding, the other rows'
 * candidates, or T_c beyond the row's own length; fixed summation orders, no atomics.
 * Reads cache rows start[b] .. L-1 of row b of k_ptrs_host[l] / v_ptrs_host[l]; rows below start[b] are NEVER read, and NO cache
 * row is written.  Layouts as cgpt_llm_score ([B, kv_heads, kv_len_stride, 128] on a grouped_kv = 1 handle); works with
 * CGPT_LLM_W_INT8 and act_format = 1 like it.
 * starts_dev, cand_tokens_dev and cand_lens_dev are read when the kernels RUN, not when the call enqueues.
 * Same contracts as cgpt_llm_score (enqueues only: no host sync, no allocation, no host->device copy; the workspace is
 * cgpt_llm_score_reserve's, for B x sum (T_c - 1) tail rows; its CGPT_ERR_INVALID / CGPT_ERR_STATE rules, all checked before the
 * first launch), plus CGPT_ERR_INVALID for a null starts_dev or cand_lens_dev. */
cgpt_status cgpt_llm_score_ragged(cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t prompt_len,
                                  const int32_t* starts_dev, const int64_t* cand_tokens_dev /* [B, C, Tmax] */,
                                  const int32_t* cand_lens_dev /* [B, C] */, const int32_t* cand_lens_host /* [C] = T_c */,
                                  int32_t C, int32_t Tmax, float label_smoothing, void* const* k_ptrs_host,
                                  void* const* v_ptrs_host, int64_t kv_len_stride, float* out_dev, void* stream);

/* ---- int8 activations: the LLM.int8() forward on the native engine (W8A8 with a per-row outlier split) ----
 * Replaces: the `load_in_8bit=True` decoder the reference's configs select (`low_resource: true`, base_model.py:196-213): row-wise
 * int8 weights, row-wise int8 activations, int32 accumulation, outlier features above a threshold multiplied in higher precision.
 * One more extended config: a cgpt_llm_config_gqa followed by three fields, recognised by gqa.base.struct_size =
 * sizeof(cgpt_llm_config_act) alone; pass &cfg.gqa.base to cgpt_llm_create.  The older structs, their sizes and their `reserved must
 * be 0` rule are unchanged.  act_format = 1 needs weight_format = CGPT_LLM_W_INT8, hidden and mlp multiples of 128 (one K-tile of the
 * int8 kernel is 128 bytes), a finite act_threshold and outlier_cap in 1..1024; each violation is CGPT_ERR_INVALID with a message,
 * before any device call.  act_format = 0 ignores the other two fields and is the handle as it was.
 * The law of a layer linear on such a handle, per input row x[K] (fp16), with q / s_w the weight law above and t = act_threshold:
 *   k is an outlier iff t > 0 and |x_k| >= t;   s_a = max over non-outliers |x_k| / 127 (fp32, correctly rounded, kept in fp32);
 *   a_k = clamp(rint(fp32(x_k) / s_a), -127, 127) (nearest even), 0 for outliers, the whole row 0 when s_a == 0;
 *   acc_n = sum_k a_k q_nk in int32 (exact);   y_n = fp32(acc_n) * (s_a * fp32(s_w[n])), two fp32 multiplies, the inner first;
 *   o_n = sum over outliers in ascending k of fp32(x_k) * fp32(W'_nk), sequential fp32 from 0;   v_n = y_n + o_n;
 *   then the epilogue rounds where the fp16 engine's does.  lm_head, embed_tokens and the RMSNorm weights stay fp16.
 * The outlier set is PER ROW (bitsandbytes takes outlier columns over the whole batch): a row's result is a function of that row
 * alone, as every batch-independence identity of this engine requires.  Parity with bitsandbytes is NOT pinned.
 * A row with more than outlier_cap outliers keeps its first outlier_cap (ascending k), is counted in overflow_rows, and its result is
 * finite but not the law's: read cgpt_llm_act_stats and treat overflow_rows > 0 as an error (raise outlier_cap).
 * Such a handle allocates no fp16 dequantisation scratch (the prefill runs the same int8 kernel), and cgpt_llm_weight_bytes says so. */
typedef struct cgpt_llm_config_act {
    cgpt_llm_config_gqa gqa;  /* gqa.base.struct_size = sizeof(cgpt_llm_config_act); gqa.reserved must be 0 */
    int32_t act_format;       /* CGPT_LLM_A_F16 (0) | CGPT_LLM_A_INT8 (1)                          */
    float   act_threshold;    /* 6.0 = HF's llm_int8_threshold default; <= 0: no outlier split     */
    int32_t outlier_cap;      /* 1 .. 1024 outliers kept per row                                   */
    int32_t reserved2;        /* must be 0                                                         */
} cgpt_llm_config_act;
#define CGPT_LLM_A_F16 0
#define CGPT_LLM_A_INT8 1
/* SYNCHRONISES the handle's device, then out_host[0..3] = rows quantised, outliers found, the largest outlier count of one row and
 * overflow_rows, over every native call since the last read (or create); the counters are then reset.  All zeros on a handle with
 * act_format = 0.  Not capturable (call it outside a capture; captured work counts when it replays). */
cgpt_status cgpt_llm_act_stats(cgpt_llm_handle h, int64_t* out_host);

/* The raw linear of the law above, without a handle: out = epilogue(law(A, q, s_w)) for A [M, K] fp16 (rows K apart), q [N, K] int8,
 * s_w [N] fp16, on `stream`.  epilogue: 0 = fp16(v) -> out [M, N];  1 = fp16(fp16(v) + resid) -> out [M, N], resid [M, N] fp16 (may be
 * out);  2 = SwiGLU -> out [M, N / 2], q / s_w holding gate / up rows interleaved in blocks of 16 as the engine's fused matrix does.
 * out_bytes is the size of the buffer at out_dev and must cover the result; workspace_dev must be 256-byte aligned and hold
 * cgpt_llm_linear_i8_workspace(M, N, K, outlier_cap, NULL) bytes.  CGPT_ERR_INVALID before any launch for: a null pointer, M < 1 or
 * M > 2^24, N or K < 1, N % 64, K % 128, K > 65536, a cap outside 1..1024, an unknown epilogue, epilogue 1 without resid, a short
 * out_bytes or workspace_bytes, a misaligned workspace.  Sets kernel attributes on the current device: call it outside a capture.
 * cgpt_llm_linear_i8_workspace: the bytes needed (-1 for bad sizes); offsets_out (or NULL) receives the byte offsets of the five
 * regions: [0] counters (4 x int64: rows, outliers, max per row, overflow rows -- zeroed by the call, then written by it),
 * [1] int8 codes [round_up(M, 256)][K] (rows >= M are read by the GEMM, never written), [2] s_a fp32 [round_up(M, 256)],
 * [3] outlier lists uint32 [round_up(M, 256)][cap + 1], [4] int32 slabs.
 * cgpt_llm_linear_i8_slices: K slices a call of M <= 256 runs with (a function of N and K only; 1 for M > 256); -1 for bad sizes. */
cgpt_status cgpt_llm_linear_i8(const void* A_dev, const void* q_dev, const void* sw_dev, int64_t M, int64_t N, int64_t K,
                               float threshold, int32_t outlier_cap, int32_t epilogue, const void* resid_dev, void* out_dev,
                               int64_t out_bytes, void* workspace_dev, int64_t workspace_bytes, void* stream);
int64_t cgpt_llm_linear_i8_workspace(int64_t M, int64_t N, int64_t K, int32_t outlier_cap, int64_t* offsets_out);
int32_t cgpt_llm_linear_i8_slices(int64_t N, int64_t K);

/* ---- Sampled decoding: the greedy entries with a sampling law in the place of the arg-max ----
 * Replaces: HF `generate(do_sample=True, temperature, top_k, top_p, repetition_penalty)` as `Chat.answer_prepare` calls it
 * (do_sample=True, top_p=0.9, repetition_penalty=1.05, temperature=1.0, and HF's default top_k=50), whose draws come from torch's
 * device-global generator.  Here the uniform of row b at select i is word 0 of
 *   Philox4x32-10(counter = (i, 3, id_lo, id_hi), key = (seed_lo, seed_hi)),  u = (word >> 8) * 2^-24,
 * id = draw_ids_dev[b], seed = *seed_dev: a function of (seed, draw id, select) alone, so a row's tokens do not depend on the batch it
 * runs in.  Both are DEVICE memory read when the kernels RUN (as starts_dev is): a captured graph replayed after
 * the buffers were rewritten draws the new stream.
 * The law of one select on one fp32 logits row, in HF's processor order (`sample_token_law` in minigpt4.py is the float64 oracle):
 *   1. the EOS columns read as -inf on the first min_new tokens (as in the greedy select);
 *   2. every DISTINCT id among the row's tokens generated so far is penalised once: l > 0 ? l / pen : l * pen (the prompt is embeddings
 *      and has no ids);                       3. l / temperature;
 *   4. top_k: keep l >= the k-th largest value (0 or >= vocab: off);        5. softmax over what is kept;
 *   6. top_p: n = the smallest count whose descending cumulative mass is >= top_p, keep p >= p_(n) (1: off);
 *   7. the token is the first kept column, in vocabulary order, whose cumulative kept mass exceeds u * kept_mass.
 * Both cuts keep a whole group of equal values at their boundary, where HF splits it by torch.sort's unspecified tie order.
 * do_sample = 0: steps 1-2, then the first-max arg-max (greedy with a repetition penalty); no draw is made.
 * Finished rows, EOS, stop sequences, early stop, pad_id, tokens_out_dev, step_logits_out_dev (the EOS-masked logits each select saw)
 * and every contract of cgpt_llm_greedy / cgpt_llm_greedy_ragged hold unchanged; cgpt_llm_live_steps reports these calls too.  The
 * greedy entries themselves launch exactly what they launched before these existed.
 * CGPT_ERR_INVALID before any launch, besides the greedy entries' rules: a wrong struct_size, do_sample not 0 / 1, temperature <= 0,
 * top_p outside (0, 1], top_k < 0, repetition_penalty <= 0, a null draw_ids_dev or seed_dev, vocab > 131072, num_new + num_eos > 1024. */
typedef struct cgpt_llm_sample_params {
    int32_t struct_size;              /* = sizeof(cgpt_llm_sample_params) */
    int32_t do_sample;
    float temperature;
    int32_t top_k;
    float top_p;
    float repetition_penalty;
} cgpt_llm_sample_params;
cgpt_status cgpt_llm_sample(cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t prompt_len, int32_t num_new,
                            int32_t min_new, const int64_t* eos_ids_host, int32_t num_eos, int64_t pad_id, void* const* k_ptrs_host,
                            void* const* v_ptrs_host, int64_t kv_len_stride, int64_t* tokens_out_dev, float* step_logits_out_dev,
                            cgpt_llm_sample_params params, const int64_t* draw_ids_dev, const uint64_t* seed_dev, void* stream);
cgpt_status cgpt_llm_sample_ragged(cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t prompt_len,
                                   const int32_t* starts_dev, int32_t num_new, int32_t min_new, const int64_t* eos_ids_host,
                                   int32_t num_eos, int64_t pad_id, void* const* k_ptrs_host, void* const* v_ptrs_host,
                                   int64_t kv_len_stride, int64_t* tokens_out_dev, float* step_logits_out_dev,
                                   cgpt_llm_sample_params params, const int64_t* draw_ids_dev, const uint64_t* seed_dev, void* stream);
/* One sampled select alone, without a handle, on the current device: logits_dev [B, V] fp32 (rows ld apart; not modified), row b's
 * earlier tokens prev_tokens_dev[b * ld_prev + 0 .. num_prev) (NULL with num_prev = 0), `step` = Philox counter word 0.  mask_eos != 0
 * applies step 1 to the num_eos ids of eos_ids_host.  unfinished_dev: [B] int32, read and written as the engine's own flags are -- a row
 * holding 0 gets pad_id; a row that draws an EOS id is set to 0.  uniforms_in_dev (or NULL): [B] fp32 taken in the place of the Philox
 * draw, so that the law can be tested apart from the stream; draw_ids_dev / seed_dev may then be NULL.  tokens_out_dev: [B] int64.
 * uniforms_out_dev, kept_count_out_dev, kept_mass_out_dev (each [B], or NULL): the uniform used, the number of kept columns and the
 * kept probability mass (kept weight sum / softmax denominator).  CGPT_ERR_INVALID before the launch as above, and for B < 1, V outside
 * 1..131072, ld < V, ld_prev < num_prev, num_prev + num_eos > 1024 or a null logits / tokens / unfinished pointer. */
cgpt_status cgpt_llm_sample_logits(const float* logits_dev, int64_t ld, int32_t B, int32_t V, const int64_t* prev_tokens_dev,
                                   int64_t ld_prev, int32_t num_prev, int32_t step, int32_t mask_eos, const int64_t* eos_ids_host,
                                   int32_t num_eos, int64_t pad_id, int32_t* unfinished_dev, cgpt_llm_sample_params params,
                                   const int64_t* draw_ids_dev, const uint64_t* seed_dev, const float* uniforms_in_dev,
                                   int64_t* tokens_out_dev, float* uniforms_out_dev, int32_t* kept_count_out_dev,
                                   float* kept_mass_out_dev, void* stream);

/* ---- Trie-constrained answer decoding: the greedy entries with the arg-max restricted to a vocabulary of candidate answers ----
 * Replaces: HF `generate(..., prefix_allowed_tokens_fn=...)`, greedy, over the token sequences of C candidate answers: at every select
 * the arg-max runs over the tokens that continue some candidate, a row finishes when it has spelled a whole candidate, and its class
 * id is then known on the device (`constrained_select_law` in llm_laws.py is the law).
 * The candidates are a CSR trie of int32 tables: node 0 is the root; the edges of node n are child_begin[n] .. child_begin[n + 1];
 * edge e carries token child_tok[e] and leads to node child_node[e]; leaf_class[n] is the class id (>= 0) of a leaf and -1 on an
 * inner node.  Nodes are numbered breadth-first (child_node[e] == e + 1, so a child's index is greater than its parent's) and the
 * edges of one node ascend STRICTLY by token id: "the first maximum over the edges" is "the lowest token id among the maxima".
 * cgpt_llm_trie_check: host only, no handle, no GPU.  CGPT_OK and *depth_out (may be NULL) = the longest candidate, or
 * CGPT_ERR_INVALID with a message naming the first offending node for: a null table, nodes outside 3 .. 2^20, edges != nodes - 1,
 * child_begin not monotone from 0 to child_begin[nodes] == edges, a token outside 0 .. vocab-1, edge tokens not strictly ascending, a
 * child index not above its parent's or out of range or not breadth-first, a node with two parents or none, a leaf with a class < 0,
 * an inner node with a class other than -1 (a candidate that is a prefix of another), fewer than 2 leaves, depth > 32.
 * cgpt_llm_set_trie: validates the host tables with that check (vocab = the handle's) and copies them to the device.  Handle state,
 * read when a constrained call ENQUEUES (as cgpt_llm_set_stop_sequences is): a captured call keeps the tables it was captured under,
 * so replaced tables stay allocated until cgpt_llm_destroy.  SYNCHRONISES and allocates: call it outside any capture.  nodes = 0
 * clears it (the table pointers are then ignored).  A refused call leaves the handle as it was.
 * cgpt_llm_constrained / cgpt_llm_constrained_ragged: cgpt_llm_greedy / cgpt_llm_greedy_ragged without min_new and the EOS ids, the
 * select replaced: num_new selects with num_new - 1 token steps between them, num_new == the trie's depth, so every row reaches a
 * leaf.  tokens_out_dev [B, num_new] int64: the row's candidate, then pad_id.  labels_out_dev [B] int32: leaf_class of the leaf each
 * row reached (every entry is written).  step_logits_out_dev (or NULL) [B, num_new, vocab] fp32: row i = the RAW logits select i
 * read.  Logits are finite by contract.  Early stop (a row is finished at its leaf), grouped K/V, int8 weights and activations and
 * left padding are the token step's and hold unchanged; cgpt_llm_live_steps reports these calls too.  The greedy and sampling entries
 * launch exactly what they launched before these existed.  CGPT_ERR_INVALID before any launch, besides the greedy entries' rules:
 * no trie set on the handle, num_new != the trie's depth, a null labels_out_dev.
 * cgpt_llm_trie_select_logits: one select alone, without a handle, on the current device: logits_dev [B, V] fp32 (rows ld apart),
 * the four tables as DEVICE pointers (trusted: pass tables cgpt_llm_trie_check accepted), node_dev / unfinished_dev [B] int32 read and
 * written as the engine's own are (a row holding unfinished 0, or standing on a leaf, gets pad_id and nothing else is written for it;
 * a node outside 0 .. nodes-1 reads as the root), tokens_out_dev [B] int64, labels_out_dev [B] int32 written for the rows that reach
 * a leaf in this select. */
cgpt_status cgpt_llm_trie_check(const int32_t* child_begin, const int32_t* child_tok, const int32_t* child_node,
                                const int32_t* leaf_class, int32_t nodes, int32_t edges, int32_t vocab, int32_t* depth_out);
cgpt_status cgpt_llm_set_trie(cgpt_llm_handle h, const int32_t* child_begin, const int32_t* child_tok, const int32_t* child_node,
                              const int32_t* leaf_class, int32_t nodes, int32_t edges);
cgpt_status cgpt_llm_constrained(cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t prompt_len, int32_t num_new,
                                 int64_t pad_id, void* const* k_ptrs_host, void* const* v_ptrs_host, int64_t kv_len_stride,
                                 int64_t* tokens_out_dev, float* step_logits_out_dev, int32_t* labels_out_dev, void* stream);
cgpt_status cgpt_llm_constrained_ragged(cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t prompt_len,
                                        const int32_t* starts_dev, int32_t num_new, int64_t pad_id, void* const* k_ptrs_host,
                                        void* const* v_ptrs_host, int64_t kv_len_stride, int64_t* tokens_out_dev,
                                        float* step_logits_out_dev, int32_t* labels_out_dev, void* stream);
cgpt_status cgpt_llm_trie_select_logits(const float* logits_dev, int64_t ld, int32_t B, int32_t V, const int32_t* child_begin_dev,
                                        const int32_t* child_tok_dev, const int32_t* child_node_dev, const int32_t* leaf_class_dev,
                                        int32_t nodes, int64_t pad_id, int32_t* node_dev, int32_t* unfinished_dev,
                                        int64_t* tokens_out_dev, int32_t* labels_out_dev, void* stream);

/* ---- Beam search: the decode loop with HF's beam search in the place of the arg-max ----
 * Replaces: HF `generate(num_beams=k, length_penalty=..., do_sample=False, early_stopping=False, num_return_sequences=1)` on
 * `inputs_embeds` (transformers 5.x `_beam_search`), the first slider of MiniGPT-4's demo (`beam_step_law` /
 * `beam_decode_law` in llm_laws.py are the law).  An image has k beams (2..8), E EOS ids and n = num_new; every select keeps
 * K = max(2, 1 + E) * k candidates; vocab >= K + E is required (with the EOS columns masked, beam 0 alone fills select 0's top K, so
 * the -1e9 beams never enter it).  Per image: running[k] scores (0, -1e9, ...), the beams' tokens, a pool
 * of k finished hypotheses (score -1e9, flag 0) and `open` = 1.  Select i on the k beams' fp32 logits:
 *   1. lp = l - logsumexp(l) per row (float64 normaliser, ONE fp32 rounding); EOS columns then read -inf while i < min_new;
 *   2. c = running + lp (fp32);   3. the top K of the flat [k * vocab] array, by value descending, then lowest flat index;
 *   4. fin = the token is an EOS id, or i == n - 1;   5. the next beams: the first k ranks in (fin ascending, rank ascending);
 *   6. while open: every rank < k with fin enters the pool with c / fp32((i + 1) ** length_penalty) and its tokens; the pool keeps
 *      the best k, old slots first on ties, then by rank;
 *   7. open &= running'[0] / fp32((i + 1) ** length_penalty) > (all k slots finished ? the smallest pool score : -1e9).
 * The result of an image is pool slot 0's tokens, EOS included, then pad_id, and its score (HF's sequences_scores).
 * Rows: beam row r = b * k + j of image b.  Two cache sets per layer: the PROMPT cache [B, heads, prompt_stride, 128], rows
 * 0 .. prompt_len-1 as a prefill of the B images left them (read, never written), and a BEAM cache [B * k, heads, beam_stride, 128]
 * of generated positions only: generated step t of row r rotates at prompt_len + t, writes beam row r's cache row t (the only row
 * written) and attends over the image's prompt rows, then cache row s of beam row anc[r][s] for s < t, then its own new key.  No K/V
 * byte moves between beams.  A row's logits and its appended cache row are bit for bit what cgpt_llm_step gives on the physically
 * gathered cache.  int8 weights and activations are the token step's and hold unchanged.
 * cgpt_llm_beam_reserve: the beam state of max_images x k beam rows and num_new tokens (two sets a select alternates between).  Outside
 * any capture; idempotent, grows only (replaced buffers stay allocated until cgpt_llm_destroy), like cgpt_llm_prefill_reserve.
 * cgpt_llm_beam_step: ONE teacher-forced beam step (the twin of cgpt_llm_step): tokens_dev [B * k], anc_dev [B * k, anc_ld] int32
 * (columns 0 .. t-1 read; a value outside 0 .. B*k-1 is clamped into it), logits_dev [B * k, vocab] fp32.
 * cgpt_llm_beam_select_logits: ONE select alone, without a handle, on the current device, on the caller's logits [B * k, V] (rows ld
 * apart) and the caller's state before (running [B k] fp32, tokens [B k, num_new] int64, anc [B k, num_new] int32, pool score [B k]
 * fp32 / finished [B k] int32 / length [B k] int32 / tokens [B k, num_new] int64, open [B] int32); writes the state after into the
 * second set (never in place), the next tokens [B k] int64 and the parents [B k] int32 (0 .. k-1 within the image).
 * cgpt_llm_beam: the whole loop after the prefill: num_new selects with num_new - 1 beam steps between them.  first_logits_dev
 * [B, vocab] = the prefill's logits, one row per image, read by select 0 for every beam (only beam 0 counts there).  tokens_out_dev
 * [B, num_new] int64, scores_out_dev [B] fp32 (or NULL).  step_logits_out_dev (or NULL) [B * k, num_new, vocab] fp32: row (r, i) =
 * the raw logits select i read for beam row r.  trace_out_dev (or NULL) [num_new, B, 5 k + 1] fp32: the state after select i of image
 * b: running[k], parents[k], tokens[k], pool scores[k], pool finished flags[k], open.
 * Enqueue only: no host sync, allocation or copy after the reserve call; capturable.  CGPT_ERR_INVALID before any launch for: a null
 * pointer, num_beams outside 2..8, B * num_beams outside 1..max_batch (the message names both), a grouped_kv handle, vocab < K + E or
 * > 131072, more than 8 EOS ids, a length_penalty that is not finite, positions outside either cache or max_len.  CGPT_ERR_STATE for:
 * early stop or stop sequences set on the handle, weights not loaded, a beam state not reserved for the call. */
cgpt_status cgpt_llm_beam_reserve(cgpt_llm_handle h, int32_t max_images, int32_t num_beams, int32_t num_new);
cgpt_status cgpt_llm_beam_step(cgpt_llm_handle h, const int64_t* tokens_dev, int32_t B, int32_t num_beams, int32_t prompt_len, int32_t t,
                               const int32_t* anc_dev, int64_t anc_ld, void* const* prompt_k_ptrs_host, void* const* prompt_v_ptrs_host,
                               int64_t prompt_stride, void* const* beam_k_ptrs_host, void* const* beam_v_ptrs_host, int64_t beam_stride,
                               float* logits_dev, void* stream);
cgpt_status cgpt_llm_beam_select_logits(const float* logits_dev, int64_t ld, int32_t B, int32_t num_beams, int32_t V, int32_t step,
                                        int32_t num_new, int32_t min_new, const int64_t* eos_ids_host, int32_t num_eos, int64_t pad_id,
                                        float length_penalty, const float* running_in_dev, const int64_t* tokens_in_dev,
                                        const int32_t* anc_in_dev, const float* pool_score_in_dev, const int32_t* pool_fin_in_dev,
                                        const int32_t* pool_len_in_dev, const int64_t* pool_seq_in_dev, const int32_t* open_in_dev,
                                        float* running_out_dev, int64_t* tokens_out_dev, int32_t* anc_out_dev, float* pool_score_out_dev,
                                        int32_t* pool_fin_out_dev, int32_t* pool_len_out_dev, int64_t* pool_seq_out_dev,
                                        int32_t* open_out_dev, int64_t* next_tokens_dev, int32_t* parents_dev, void* stream);
cgpt_status cgpt_llm_beam(cgpt_llm_handle h, const float* first_logits_dev, int32_t B, int32_t num_beams, int32_t prompt_len,
                          int32_t num_new, int32_t min_new, const int64_t* eos_ids_host, int32_t num_eos, int64_t pad_id,
                          float length_penalty, void* const* prompt_k_ptrs_host, void* const* prompt_v_ptrs_host, int64_t prompt_stride,
                          void* const* beam_k_ptrs_host, void* const* beam_v_ptrs_host, int64_t beam_stride, int64_t* tokens_out_dev,
                          float* scores_out_dev, float* step_logits_out_dev, float* trace_out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CGPT_H */
