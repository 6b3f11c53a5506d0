/* awt.h -- C-ABI of libawt.so: the MI355X-native (gfx950) log-mel front-end + Whisper-style audio encoder.
 *
 * The reference (AdamBeedell/MLX8-WS-Audio-Transformer) has no FFI / plugin interface for this path: it is
 * reached through ordinary Python call sites into `transformers`.  Each entry point below
 * names the reference call it stands behind; the Python modules under mlx8-ws-audio-transformer_amd/ wrap them so that those
 * call sites keep their names, argument meaning and error behaviour (INTEGRATION.md shows the ctypes stub).
 *
 * Conventions
 *  - every function returns AWT_OK (0) or a negative awt_status; nothing throws across the ABI;
 *    awt_last_error() returns a thread-local message owned by the library;
 *  - all data pointers are CALLER-OWNED DEVICE pointers (e.g. torch tensors' data_ptr()); the library never
 *    frees caller memory and never allocates inside a compute call (tables and converted weights are
 *    allocated in *_create / *_set_weight / awt_*_prepare; only a front-end configuration that was never prepared is
 *    built at its first use);
 *  - all work is enqueued on the caller's hipStream_t (passed as void*; NULL = default stream);
 *    no hidden synchronisation except where a function says so (awt_prof_collect; the creation and upload calls awt_weight_create and
 *    awt_encoder_set_weight; awt_op_linear / awt_op_linear_fused with terms 4 and 5 outside a stream capture).  Every other function with a
 *    stream parameter can be recorded into a HIP graph (hipStreamBeginCapture on that stream) and replayed on new contents of the same buffers
 *    bit-identically, once the tables and weights it uses exist, i.e. after one ordinary call; the communicator's calls, which use a second
 *    stream, are the exception.  tests/graph_capture.py lists both groups and tests/test_gpu_graph_capture.py holds every operator to it;
 *  - a handle is not thread-safe; distinct handles are independent; one awt_ctx per (process, device).
 */
#ifndef AWT_H_
#define AWT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum awt_status {
  AWT_OK = 0,
  AWT_ERR_INVALID = -1,      /* bad argument (shape, alignment, NULL, unsupported config)            */
  AWT_ERR_HIP = -2,          /* a HIP runtime call failed; message carries hipGetErrorString          */
  AWT_ERR_WORKSPACE = -3,    /* caller's workspace is smaller than *_workspace_bytes()                */
  AWT_ERR_STATE = -4,        /* weights missing / handle misuse                                       */
  AWT_ERR_VALUE = -5         /* value error the reference raises too (e.g. mel length != 2*S)         */
} awt_status;

typedef struct awt_ctx awt_ctx;
typedef struct awt_encoder awt_encoder;

const char* awt_last_error(void);
const char* awt_version(void);

int awt_ctx_create(int device, awt_ctx** out);
void awt_ctx_destroy(awt_ctx* c);

/* ------------------------------------------------------------------------------------------------------
 * Whisper log-mel (K1-K4).  Stands behind `processor(audio, sampling_rate=16000)` /
 * `WhisperFeatureExtractor.__call__`:
 *   /root/reference/AB/fineTune.py:88, AB/wavToWhisper.py:55, AB/fineTuneMidiTester.py:33,
 *   .charles/music2midi/model.py:100-104 -> HF:models/whisper/feature_extraction_whisper.py:105-168,193-346.
 * pcm        [B] clips, `pcm_stride` elements apart; int16 (decoded as x/32768, the reference loaders'
 *            convention) when pcm_is_i16 != 0, else float32.
 * n_valid    device int32[B] = samples of each clip that are real (rest is zero padding), or NULL = max_valid
 *            for every clip.  Samples at index >= n_valid[b] are never read.
 * max_valid  host-side upper bound of n_valid (sizes the grid); clips longer than 160*n_frames_out samples
 *            are truncated like the reference does (feature_extraction_whisper.py:300-305).
 * n_frames_out  3000 = the reference's behaviour (clip zero-padded to 30 s); 400 = trimmed 4 s mode.
 * out        float32 [B, 80, n_frames_out].
 * workspace  >= awt_logmel_workspace_bytes(B) bytes, 16-byte aligned.
 */
size_t awt_logmel_workspace_bytes(int B);
int awt_logmel_whisper(awt_ctx* c, const void* pcm, int pcm_is_i16, int64_t pcm_stride, const int32_t* n_valid,
                       int max_valid, int B, int n_frames_out, float* out, void* workspace, size_t ws_bytes,
                       void* stream);
/* Same with the number of mel bins explicit: 80 (`WhisperFeatureExtractor()` defaults, tiny .. large-v2) or 128
 * (`feature_size=128`, large-v3); out is [B, n_mels, n_frames_out]. */
int awt_logmel_whisper_mels(awt_ctx* c, const void* pcm, int pcm_is_i16, int64_t pcm_stride, const int32_t* n_valid,
                            int max_valid, int B, int n_frames_out, int n_mels, float* out, void* workspace, size_t ws_bytes,
                            void* stream);
/* Long-form input (`processor(audio, truncation=False, padding="longest")`): the clips zero-padded to n_signal samples (the longest
 * clip), reflect padding only beyond n_signal, the last STFT frame dropped, each clip's max over all its frames.  out is
 * [B, n_mels, n_signal / 160] (any frame count, 4-byte aligned); n_signal > 200. */
int awt_logmel_whisper_signal(awt_ctx* c, const void* pcm, int pcm_is_i16, int64_t pcm_stride, const int32_t* n_valid,
                              int max_valid, int B, int n_signal, int n_mels, float* out, void* workspace, size_t ws_bytes,
                              void* stream);

/* UrbanSound log-mel (K15).  Stands behind `torch.log(mel_spectrogram(waveform) + 1e-6)`:
 *   /root/reference/.charles/spectrogram.py:79-87,160-162 (torchaudio MelSpectrogram: periodic Hann(n_fft),
 *   center/reflect, power 2, HTK mel, no norm).
 * pcm float32 [B] clips of n_samples (already mono / padded / trimmed: spectrogram.py:145-157),
 * out float32 [B, n_mels, 1 + n_samples / hop].  Supported: n_fft in {400, 512, 1024}, n_mels <= 128. */
int awt_logmel_generic(awt_ctx* c, const float* pcm, int64_t pcm_stride, int B, int n_samples, int sample_rate,
                       int n_fft, int hop, int n_mels, float f_min, float f_max, float log_eps, float* out,
                       void* stream);

/* Mono mix + sample-rate conversion + pad / trim (K16).  Stands behind /root/reference/.charles/spectrogram.py:146-157:
 *   `torch.mean(waveform, dim=0, keepdim=True)` when there is more than one channel, then
 *   `torchaudio.transforms.Resample(orig_freq=sr, new_freq=SAMPLE_RATE)(waveform)` when sr differs (transform defaults:
 *   sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), then zero-pad / truncate to `n_out` samples.
 * pcm: `channels` channels of `n_in` samples, int16 (scaled by 1/32768 as torchaudio.load does) or float32; element
 *   (c, i) is at pcm[c * channel_stride + i * sample_stride] -- planar [C][n] is (n, 1), interleaved WAV data is (1, C).
 * out: float32 [n_out].  The resampled clip has awt_resampled_length() = ceil(n_in * sr_out / sr_in) samples; output
 *   samples beyond it are zero.  sr_in == sr_out skips the filter, as the reference does. */
/* Device tables (DFT basis + mel bank of a front-end configuration; polyphase taps of a rate pair) are built once per context.
 * awt_ctx_create builds the two Whisper front-ends' tables; call these for any other configuration BEFORE the first compute call that
 * uses it, so that compute calls neither allocate nor synchronise (an unprepared configuration is built at first use, with a
 * hipMalloc and a blocking copy inside that one call).  slaney != 0: Slaney scale + area normalisation (Whisper); 0: HTK, no norm. */
int awt_logmel_prepare(awt_ctx* c, int n_fft, int n_mels, float f_min, float f_max, int sample_rate, int slaney);
int awt_resample_prepare(awt_ctx* c, int sr_in, int sr_out);
int64_t awt_resampled_length(int n_in, int sr_in, int sr_out);
int awt_prepare_waveform(awt_ctx* c, const void* pcm, int pcm_is_i16, int channels, int64_t channel_stride,
                         int64_t sample_stride, int n_in, int sr_in, int sr_out, float* out, int n_out, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Whisper-style audio encoder (K5-K13).  Stands behind `encoder(input_features).last_hidden_state`
 * (`WhisperModel.get_encoder()`, .charles/music2midi/model.py:33,109-110; implicitly AB/fineTune.py:199)
 * -> HF:models/whisper/modeling_whisper.py:592-646 (+ :379-413, :284-356, :215-238).
 */
typedef struct awt_encoder_cfg {
  int32_t d_model;          /* 384 tiny, 512 base, 768 small, 1024 medium, 1280 large; multiple of 128, <= 1280 */
  int32_t n_layers;
  int32_t n_heads;          /* head_dim = d_model / n_heads must be 64                                     */
  int32_t ffn_dim;          /* multiple of 128                                                             */
  int32_t n_mels;           /* 80 (tiny .. large-v2) or 128 (large-v3); multiple of 8, <= 128              */
  int32_t n_ctx;            /* S = max_source_positions: 1500 (reference) or 200 (trimmed); mel T = 2*S    */
  int32_t mfma_terms;       /* operand precision of the forward pass:
                               1 bf16: one bf16 MFMA per fragment pair (fast; ~4e-3 rel-L2 vs fp32, misses the 1e-3 bound);
                               2 fp16: one fp16 MFMA per fragment pair (11 significant bits per operand: max-abs ~2.5e-3 on
                                 Whisper-small, misses the bound as well; a measurement mode, inference only);
                               3 bf16x3: split-bf16 hi + lo planes, three MFMAs (2^-17 per operand; the training format);
                               4 fp16x3: split-fp16 planes, three MFMAs (2^-23 per operand; operands within fp16's range);
                               5 f16f8: fp16 plane + two e4m3 planes, the two cross terms on the block-scaled fp8 MFMA: two
                                 MFMA-equivalents per fragment pair (2^-16 per operand); inference only.  Its attention keeps
                                 the cross terms of q k^T and runs P V as one fp16 product           */
  int32_t lora_rank;        /* 0 = no adapters; else 1..32 (the adapter-gradient kernels' width)           */
  float lora_alpha;         /* adapter scale = lora_alpha / lora_rank                                      */
  uint32_t lora_targets;    /* bit mask of AWT_LORA_*                                                      */
  int32_t chunk_clips;      /* clips processed per kernel wave (0 = library default)                       */
  int32_t training;         /* != 0: keep transposed copies of the frozen weights so awt_encoder_backward can run
                               (mfma_terms 1 or 3 in this mode)                                             */
  int32_t backward_terms;   /* products of the backward pass' gradient contractions: 0 = mfma_terms (default: gradients
                               to 3e-5 of fp32 autograd), 1 with mfma_terms = 3 = one bf16 product (the usual
                               mixed-precision trade: ~0.5 % gradient error, 1.4x faster step); the attention scores are
                               recomputed in split-bf16 either way.  5 with mfma_terms = 3: the MLP of the training step -- fc1 / fc2
                               forward and their two backward GEMMs (d pre = (dx W2) gelu'(pre), d ln2 = d pre W1) -- runs in the
                               f16f8 operand format (2 instead of 3 MFMA-equivalents, 2^-16 per operand like split-bf16), everything
                               else in split-bf16; fp16 planes want gradients of order one: see awt_encoder_set_grad_scale_log2.
                               No fc1 / fc2 adapters.                                                                       */
  int32_t train_base;       /* != 0 (with training != 0, lora_rank = 0, backward_terms != 5): full-parameter fine-tuning -- the backward
                               pass produces the gradient of every base parameter except embed_positions.weight (see "Full-parameter
                               fine-tune step" below).  0 = the adapter-only library, unchanged bit for bit.                   */
} awt_encoder_cfg;

enum { AWT_LORA_Q = 1, AWT_LORA_K = 2, AWT_LORA_V = 4, AWT_LORA_OUT = 8, AWT_LORA_FC1 = 16, AWT_LORA_FC2 = 32 };

int awt_encoder_create(awt_ctx* c, const awt_encoder_cfg* cfg, awt_encoder** out);
void awt_encoder_destroy(awt_encoder* e);

/* Upload one parameter by its HF state-dict key (relative to the encoder module): `conv1.weight`,
 * `layers.{i}.self_attn.{q,k,v,out}_proj.{weight,bias}`, `layers.{i}.{self_attn_layer_norm,final_layer_norm}.*`,
 * `layers.{i}.fc{1,2}.*`, `layer_norm.*`, `embed_positions.weight`, plus build-defined `<module>.lora_A` [r, in] and
 * `<module>.lora_B` [out, r].  `data` is a float32 device pointer of `rank`-d `shape`; the library converts it to
 * its internal operand planes on `stream` and keeps its own copy.  In the f16f8 inference format the upload of a
 * projection matrix (q / k / v / out_proj / fc1 / fc2) also finds out whether every element is exactly representable in
 * fp16 -- true of checkpoints released in half precision -- and, to read that one flag back, synchronises `stream`;
 * such a matrix's GEMM then drops the identically-zero x_hi w_lo cross term. */
int awt_encoder_set_weight(awt_encoder* e, const char* hf_name, const float* data, const int64_t* shape, int rank,
                           void* stream);

/* How many of the encoder's projection matrices (per layer: the fused q|k|v block, out_proj, fc1, fc2) hold only fp16-representable values
 * -- i.e. run the exact-weight GEMM form with one cross term fewer -- and how many such matrices there are.  Measured at upload time
 * (awt_encoder_set_weight); bench.py derives its MFMA products per fragment pair and algorithmic bytes from this, not from a flag.
 * n_exact = 0 in the modes that never look (bf16, bf16x3, training). */
int awt_encoder_exact16_matrices(const awt_encoder* e, int* n_exact, int* n_total);

size_t awt_encoder_workspace_bytes(const awt_encoder* e, int B);

/* input_features float32 [B, n_mels, 2*n_ctx] -> last_hidden_state float32 [B, n_ctx, d_model].
 * `n_frames` must equal 2*n_ctx, otherwise AWT_ERR_VALUE (the reference raises ValueError,
 * modeling_whisper.py:612-616). */
int awt_encoder_forward(awt_encoder* e, const float* input_features, int B, int n_frames, float* last_hidden_state,
                        void* workspace, size_t ws_bytes, void* stream);

/* ---- LoRA fine-tune step (K13/K14; build-defined adapters): the encoder half of
 * `trainer.train()` (/root/reference/AB/fineTune.py:186-199), with the frozen base weights and trainable A/B.
 * awt_encoder_forward_train is awt_encoder_forward for the whole batch at once, keeping every activation the backward
 * pass needs in `saved` (>= awt_encoder_train_workspace_bytes(e, B) bytes, 256-byte aligned, caller-owned, must stay
 * untouched until awt_encoder_backward has been enqueued on the same stream).
 * awt_encoder_backward takes d(loss)/d(last_hidden_state) [B, n_ctx, d_model] and writes the gradients of every
 * adapter into `lora_grads` (float32, awt_encoder_lora_grad_count(e) elements): for each layer in order, for each
 * enabled target in the order q_proj, k_proj, v_proj, out_proj, fc1, fc2: dA [r, in_features] then dB [out_features, r], row-major
 * (in / out = d_model except fc1: out = ffn_dim, fc2: in = ffn_dim).  Gradients of frozen weights and of the input features are
 * not produced (nothing below the first adapter needs them). */
/* The backward pass carries 2^k x the gradient from the final LayerNorm on and divides the adapter gradients by 2^k on the way out (exact: powers of two).
 * With backward_terms = 5 the host picks k so that the largest |d loss / d hidden| becomes ~2^6: fp16 planes hold gradients of order one at full precision,
 * 1e-6 ones only as subnormals.  Default 0; any backward_terms accepts it. */
int awt_encoder_set_grad_scale_log2(awt_encoder* e, int k);
size_t awt_encoder_train_workspace_bytes(const awt_encoder* e, int B);
size_t awt_encoder_lora_grad_count(const awt_encoder* e);
int awt_encoder_forward_train(awt_encoder* e, const float* input_features, int B, int n_frames, float* last_hidden_state,
                              void* saved, size_t saved_bytes, void* stream);
int awt_encoder_backward(awt_encoder* e, const float* d_last_hidden_state, int B, void* saved, size_t saved_bytes,
                         float* lora_grads, size_t n_grads, void* stream);
/* Same with flags.  AWT_BWD_ACCUMULATE: lora_grads += the gradients (gradient accumulation over micro-batches) instead
 * of overwriting.  AWT_BWD_ALLREDUCE: after awt_encoder_set_comm, the gradients (after accumulation) are averaged over
 * the communicator's ranks inside this call, layer group by layer group: the group holding the upper layers is
 * all-reduced on the communicator's side stream while the lower layers' backward still runs on `stream`; `stream` waits
 * for the last group before anything enqueued after this call reads lora_grads (one flat buffer, reduced
 * in place, overlapped with the remaining backward). */
enum { AWT_BWD_ACCUMULATE = 1, AWT_BWD_ALLREDUCE = 2 };
int awt_encoder_backward_ex(awt_encoder* e, const float* d_last_hidden_state, int B, void* saved, size_t saved_bytes,
                            float* lora_grads, size_t n_grads, uint32_t flags, void* stream);

/* ---- Full-parameter fine-tune step (awt_encoder_cfg.train_base; build-defined like the adapter mode): what `trainer.train()` of
 * /root/reference/AB/fineTune.py:131-199 does to the encoder -- every parameter of it is trained, except the sinusoid table, which HF freezes too
 * (`embed_positions.requires_grad_(False)`).  awt_encoder_forward_train additionally keeps the conv stem's operands (im2col rows, conv1 output and
 * pre-activation) and every layer's fc2 input in `saved` (awt_encoder_train_workspace_bytes reports the size of this mode).
 * awt_encoder_backward[_ex] then takes, in place of `lora_grads`, ONE flat float32 buffer of awt_encoder_base_grad_count(e) elements and writes
 * into it: per layer dW and db of q_proj, k_proj (no bias), v_proj, out_proj, fc1, fc2 and dgamma / dbeta of both LayerNorms; dgamma / dbeta of the
 * final layer_norm; and -- the pass continues below layer 0, through its first LayerNorm, the position add and both GELUs -- dW and db of conv2 and
 * conv1, conv weights in the [out, in, 3] layout of the HF parameters.  No gradient for embed_positions.weight or the input features.
 * dW[n, k] = sum_m dY[m, n] X[m, k] runs on an MFMA weight-gradient GEMM over the pass' bf16 planes (csrc/wgrad.hip: products per
 * backward_terms, slab partials summed in a fixed order: bit-reproducible).
 * Layout of the buffer: the non-layer parameters first, then one contiguous block per layer, layers in order; query it, do not hard-code it:
 * awt_encoder_base_grad_params(e) parameters, and for index i < that count awt_encoder_base_grad_param gives the HF state-dict key (a string owned
 * by the handle), the element offset, the shape (3 entries, unused ones 1) and its rank.
 * AWT_BWD_ACCUMULATE and awt_encoder_set_grad_scale_log2 apply as for adapters.  AWT_BWD_ALLREDUCE reduces layer groups on the side stream as they
 * finish; the lowest group is reduced last, after the conv stem, together with the non-layer parameters in front of it. */
size_t awt_encoder_base_grad_count(const awt_encoder* e);
int awt_encoder_base_grad_params(const awt_encoder* e);
int awt_encoder_base_grad_param(const awt_encoder* e, int index, const char** name, size_t* offset, int64_t* shape /* [3] */, int* rank);

/* ------------------------------------------------------------------------------------------------------
 * Data-parallel gradient exchange over RCCL / xGMI (build-defined: the reference has no distributed code, SURVEY.md
 * §5 last row, §8a a17, §8e).  One process per GPU; rank 0 calls awt_comm_unique_id and hands the 128 bytes to the other
 * ranks out of band (torch.distributed's store in finetune.py); every rank then calls awt_comm_create (collective).
 * librccl.so is loaded on first use (dlopen), so the library itself loads on hosts without RCCL.
 * awt_allreduce_{sum,mean}_f32: in-place ncclAllReduce (ncclSum / ncclAvg) of `n` floats at device pointer `buf`,
 * enqueued on `stream`.  The fine-tune step's exchange is ONE flat buffer (r = 16 on q, v of Whisper-small: 589 824
 * floats = 2.36 MB): latency-bound, so it is never split finer than awt_encoder_set_comm's layer groups. */
typedef struct awt_comm awt_comm;
enum { AWT_COMM_ID_BYTES = 128 };
int awt_comm_unique_id(void* id_out /* host, AWT_COMM_ID_BYTES */);
int awt_comm_create(awt_ctx* c, const void* id /* host, AWT_COMM_ID_BYTES */, int rank, int world, awt_comm** out);
void awt_comm_destroy(awt_comm* m);
int awt_comm_world(const awt_comm* m);
int awt_allreduce_sum_f32(awt_comm* m, float* buf, size_t n, void* stream);
int awt_allreduce_mean_f32(awt_comm* m, float* buf, size_t n, void* stream);
/* Timing of the bucket reductions that awt_encoder_backward_ex issues on the communicator's side stream (AWT_BWD_ALLREDUCE): enable != 0 records a HIP
 * event pair around each one from now on (at most 8 between read-outs); the call returns, and clears, what was recorded since the previous call --
 * milliseconds on the side stream and bytes per bucket, in issue order -- so that a multi-GPU run can show that, and how long, the exchange ran. */
int awt_comm_bucket_stats(awt_comm* m, int enable, double* ms, int64_t* bytes, int max, int* n_out);
/* Attach a communicator to an encoder for AWT_BWD_ALLREDUCE; `groups` >= 1 layer groups (2 = upper / lower half;
 * clamped to the layer count).  m = NULL detaches. */
int awt_encoder_set_comm(awt_encoder* e, awt_comm* m, int groups);

/* PCM -> hidden states in one call (log-mel + encoder, chunked so intermediates stay cache-resident):
 * the batched form of `WhisperAudioEncoder.forward` (.charles/music2midi/model.py:42-123).
 * `input_features_out` may be NULL; when given it receives float32 [B, n_mels, 2*n_ctx]. */
size_t awt_audio_encode_workspace_bytes(const awt_encoder* e, int B);
int awt_audio_encode(awt_encoder* e, const void* pcm, int pcm_is_i16, int64_t pcm_stride, const int32_t* n_valid,
                     int max_valid, int B, float* input_features_out, float* last_hidden_state, void* workspace,
                     size_t ws_bytes, void* stream);

/* Clip lengths reach the encoder through awt_audio_encode only.  The log-mel front-end pads a clip with one constant per clip from its
 * last live frame on, so every position of the conv stem past the live frames but the last one is the same vector: awt_audio_encode
 * computes the stem for the first awt_conv_stem_positions(n_ctx, max_valid) positions of each clip and copies the rest (bit-identical
 * to computing all of them; tuning knob "conv_live").  The bound is log-mel's contract: max_valid >= every n_valid[b].  Returns n_ctx
 * when every position has to be computed (clips of the full 30 s); needs no GPU.  awt_encoder_forward and awt_encoder_forward_train
 * take a mel without lengths and compute every position. */
int awt_conv_stem_positions(int n_ctx, int max_valid);

/* ------------------------------------------------------------------------------------------------------
 * Single-operator entry points (what the encoder is made of; used by the per-kernel parity tests).
 * Row-major float32 in / out; bf16 splitting happens inside.  `terms` = 1 or 3 as in awt_encoder_cfg.
 * awt_op_linear (and awt_op_linear_fused) pack w on every call.  With terms 4 and 5 that pack also looks for fp16-exact weights as awt_encoder_set_weight
 * does and, to read the one flag back, synchronises `stream` -- except while `stream` is recording into a HIP graph, where a host read is not possible:
 * there the probe is left out and the GEMM keeps every cross term, which is the form any weight that is not fp16-exact takes anyway (for one that is,
 * the extra product is with an all-zero plane).  Terms 1 to 3 never synchronise. */
int awt_op_linear(awt_ctx* c, const float* x /*[M,K]*/, const float* w /*[N,K]*/, const float* bias /*[N] or NULL*/,
                  float* y /*[M,N]*/, int M, int N, int K, int terms, void* workspace, size_t ws_bytes, void* stream);
size_t awt_op_linear_workspace_bytes(int M, int N, int K);
int awt_op_layernorm(awt_ctx* c, const float* x /*[M,d]*/, const float* gamma, const float* beta, float* y, int M, int d,
                     float eps, void* stream);
/* q (already scaled), k, v: float32 [B, H, S, 64]; o: float32 [B, S, H*64] */
int awt_op_attention(awt_ctx* c, const float* q, const float* k, const float* v, float* o, int B, int H, int S,
                     int terms, void* workspace, size_t ws_bytes, void* stream);
size_t awt_op_attention_workspace_bytes(int B, int H, int S);
/* awt_op_attention with every output form of the forward kernels, as the encoder layer launches them.  No kernel of its own: the operand planes are
 * written into the workspace (awt_op_attention's layout and size), one launch follows, and the bytes the kernel wrote are the result.
 *   in:  q (already scaled), k, v: float32 [B, H, S, 64].
 *   out: exactly one of
 *          o_f32  float32 [B, S, H*64];
 *          planes [B*S, H*64]: terms 1 / 3 bf16, 2 / 4 fp16, o_hi (+ o_lo with terms 3 / 4; not written and may be NULL with terms 1 / 2);
 *                 terms 5: o_hi = fp16, o_hi8 = e4m3(o 2^-2) (may be NULL: not written), o_lo8 = e4m3((o - fp16(o)) 2^9);
 *          o_ilv  (terms 5) the same three images as split lines: [B*S][H] pairs of 128-byte lines, 64 fp16, then 64 hi8 | 64 lo8;
 *        and optionally lse2: float32 [B, H, S], log2 of each row's sum of 2^(score log2 e).
 * With terms 5 the f16f8 form is chosen as in the encoder (tuning knob "attn_shape", else: lse2 requested -> every cross term on 4 or 8 waves, not
 * requested -> P V as one fp16 product), and v's two e4m3 images are written only for a form that reads them.
 * AWT_ERR_INVALID before anything is written: no output or more than one output form, split lines with terms != 5, planes without o_lo (terms 3 / 4) or
 * without o_lo8 (terms 5), a shape that is not positive; AWT_ERR_WORKSPACE: ws_bytes below awt_op_attention_ex_workspace_bytes. */
int awt_op_attention_ex(awt_ctx* c, const float* q, const float* k, const float* v, float* o_f32, void* o_hi, void* o_lo, void* o_hi8, void* o_lo8,
                        void* o_ilv, float* lse2, int B, int H, int S, int terms, void* workspace, size_t ws_bytes, void* stream);
size_t awt_op_attention_ex_workspace_bytes(int B, int H, int S);
/* The attention of one encoder layer's training pass on caller tensors: the training form of the forward (row-major o planes and the saved
 * log-sum-exp), then the backward kernel with the arguments awt_encoder_backward gives it.  No kernel of its own.
 *   in:  q (already scaled by head_dim^-1/2, as for awt_op_attention), k, v: float32 [B, H, S, 64];  d_o = dL/do: float32 [B, S, H*64]
 *   out: o_hi / o_lo: bf16 planes [B*S, H*64] of o;  lse2: float32 [B, H, S], log2 of each row's sum of 2^(score log2 e);
 *        delta: float32 [B, H, S] = rowsum(d_o * o);  g_hi / g_lo: bf16 planes [B*S, 3*H*64] holding dq | dk | dv per row, which is what
 *        the QKV backward GEMM reads (a value is hi + lo).  dq = qscale * dL/dq, dk and dv are dL/dk and dL/dv.
 * `terms` = 1 (bf16) or 3 (bf16x3); `grad_terms` = terms, or 1 with terms = 3 (awt_encoder_cfg.backward_terms = 1: the scores stay split-bf16,
 * the gradient products take one bf16 plane).  Anything else is AWT_ERR_INVALID.  With terms = 1 the lo planes are not written and may be NULL. */
int awt_op_attention_backward(awt_ctx* c, const float* q, const float* k, const float* v, const float* d_o, void* o_hi, void* o_lo,
                              float* lse2, float* delta, void* g_hi, void* g_lo, int B, int H, int S, float qscale, int terms,
                              int grad_terms, void* workspace, size_t ws_bytes, void* stream);
size_t awt_op_attention_backward_workspace_bytes(int B, int H, int S);

/* One GEMM launch with any of its fused epilogues on caller tensors, with the arguments the encoder gives it.  No kernel of its own: the fp32
 * operands are written as operand planes (as awt_op_linear does, including the upload-time detection of fp16-exact weights with terms 4 and 5), one
 * launch follows, and the bytes the kernel wrote are the result -- nothing is converted back.  The tuning knobs "gemm_tile", "gemm_mfma16" and
 * "gemm_pp" = 2 are honoured as by awt_op_linear (the ping-pong kernel takes terms 5, one plain dense segment, N % 256 == 0, K >= 128 and five of
 * the epilogues; under "gemm_pp" = 2 any other epilogue with such a shape is refused).
 *   x [x_rows, ldx], w [N, ldw], bias [N] or NULL: float32.  C[m, n] = sum over the nseg <= 3 K segments of x[row_i(m), xcol_i .. + k_i) . w[n, wcol_i .. + k_i),
 *   row_i(m) = (m / rows_out) * rows_in + (m % rows_out) * row_mul + row_add, a row outside [0, rows_in) of its group reading as zero (rows_in ==
 *   row_mul * rows_out).  ldx, ldw, xcol, wcol and k are multiples of 64.  Two segments express the LoRA form [x | u] [W | B]^T, three the
 *   stride-2 conv stem.
 *   epi (GemmEpilogue of csrc/common.h): 0 out_f32 = C + bias;  1 out_f32 = resid + C + bias (resid may be out_f32);  2 planes of (C + bias) scale;
 *   3 planes of gelu(C + bias);  4 head-major q | k | v planes [3][M / S][H][S][64] (N == 3 H 64, M % S == 0, plane stride M H 64 elements), the q
 *   columns times scale;  5 out_f32 = gelu(C + bias) + pos[m % rows_pos];  6 as 3, and bf16 planes out_hi2 / out_lo2 of C + bias;  7 planes of
 *   C gelu'(pre), pre = pre_hi + pre_lo (bf16 planes, pitch ldo; pre_lo may be NULL).
 *   Plane outputs (pitch ldo, 0 = N): terms 1 / 3 bf16, 2 / 4 fp16, out_hi (+ out_lo with terms 3 / 4); terms 5: out_hi = fp16, out_hi8 = e4m3(v 2^s)
 *   (may be NULL), out_lo8 = e4m3((v - fp16(v)) 2^(s + 11)), s = -2 (q: 2, k and v: 0); skip_v8 leaves v's two e4m3 images unwritten;
 *   split_lines (ping-pong kernel, epi 2 / 3): out_ilv instead, [M][N / 64] pairs of 128-byte lines: 64 fp16, then 64 hi8 | 64 lo8.
 *   Columns >= n_valid (0 = N; a multiple of 4, of 8 with terms 5) and rows >= M are not written.  m_pick > 0: the kernel is chosen as for a launch of
 *   m_pick rows.
 * Whatever the launch itself would refuse is AWT_ERR_INVALID here, before anything is written. */
typedef struct awt_linear_fused_args {
  int32_t M, N, terms, epi, nseg;
  int32_t x_rows, ldx, ldw;
  int32_t seg_xcol[3], seg_wcol[3], seg_k[3], seg_rows_out[3], seg_rows_in[3], seg_row_mul[3], seg_row_add[3];
  int32_t rows_pos, S, H, skip_v8, n_valid, m_pick, split_lines, ldo;
  float scale;
  const float* x; const float* w; const float* bias;
  const float* resid; const float* pos; const void* pre_hi; const void* pre_lo;
  float* out_f32; void* out_hi; void* out_lo; void* out_hi8; void* out_lo8; void* out_ilv; void* out_hi2; void* out_lo2;
} awt_linear_fused_args;
int awt_op_linear_fused(awt_ctx* c, const awt_linear_fused_args* a, void* workspace, size_t ws_bytes, void* stream);
size_t awt_op_linear_fused_workspace_bytes(int x_rows, int ldx, int N, int ldw);

/* ------------------------------------------------------------------------------------------------------
 * Decoder-side operators of the fine-tune step (scope row "next" #1): what `WhisperForConditionalGeneration.forward` runs after
 * the encoder -- /root/reference/AB/fineTune.py:131,186-199 -> HF:modeling_whisper.py:416-507 (decoder layer), :649-797
 * (decoder), :994-1100 (shift labels, tied projection, cross-entropy).  B x L label tokens (L ~ 12, <= 448) against frozen
 * weights: the linears are weight-bound GEMMs on the encoder's MFMA kernel over weights packed once (`awt_weight`); attention is
 * an fp32 row kernel (causal self-attention, cross-attention over the 1500 encoder positions) that reads q / k / v in place from
 * the row-major outputs of the linears.  All float32 in / out, row-major, caller-owned device memory, deterministic.
 * The weights are frozen by default; with NativeWhisperDecoder(train_base=True) every decoder parameter trains: the weight gradients are
 * awt_op_weight_grad products on the operands the backward already holds, the biases awt_op_column_sums_ld, the LayerNorm affines
 * awt_op_layernorm_param_grad, the tied embedding awt_op_embed_backward, and awt_weight_update re-packs a stepped weight into its handle.
 */
typedef struct awt_weight awt_weight;
/* Packs a frozen nn.Linear weight [N, K] (+ bias [N] or NULL) once: N is zero-padded to a multiple of 128 (awt_weight_padded_rows),
 * K must be a multiple of 64; precision 1 (bf16) or 3 (bf16x3); with_transpose keeps the transposed copy that
 * awt_linear_backward_input needs (then K must be a multiple of 128).  Creation time: the planes are hipMalloc'd and cleared with a blocking
 * hipMemset, so this call synchronises the device and cannot be part of a stream capture; the pack itself runs on `stream`. */
int awt_weight_create(awt_ctx* c, const float* w, const float* bias, int N, int K, int precision, int with_transpose, void* stream,
                      awt_weight** out);
void awt_weight_destroy(awt_weight* w);
int awt_weight_padded_rows(const awt_weight* w);
/* A TRAINED weight (NativeWhisperDecoder train_base, after an optimizer step): packs the changed [N, K] values (and bias [N]; given iff the handle
 * was created with one) into the planes the handle already owns, the transposed copy included.  In place, no allocation; the planes come out
 * bit-identical to those awt_weight_create would build from the same data.  w must have the handle's N x K elements (the caller checks: the
 * handle cannot see a tensor's shape). */
int awt_weight_update(awt_ctx* c, awt_weight* w, const float* weight, const float* bias, void* stream);
size_t awt_linear_workspace_bytes(const awt_weight* w, int M, int backward);   /* backward != 0: for awt_linear_backward_input */
/* y [M, Np] = x [M, K] W^T + bias (+ resid [M, Np], may alias y)      F.linear / the residual adds of HF:modeling_whisper.py:468-500 */
int awt_linear_forward(awt_ctx* c, const awt_weight* w, const float* x, const float* resid, float* y, int M, void* workspace,
                       size_t ws_bytes, void* stream);
/* The same product for the rows of incremental decoding, 1 <= M <= 8 (any other M: AWT_ERR_INVALID): y [M, Np] = x [M, K] W^T + bias (+ resid [M, Np] or
 * NULL, may alias y).  The output side is awt_linear_forward's: pitch Np, columns N .. Np - 1 come out as 0 + resid, the bias is the handle's, the launch goes
 * to the caller's stream without synchronisation.  It takes NO workspace and has no plane-split launch in front: one weight-streaming kernel (csrc/gemv.hip)
 * reads the hi / lo planes the handle already owns (there is no second copy of a weight; awt_weight_update stays all a trained weight needs) and splits the
 * fp32 rows of x itself, hi = rne_bf16(x), lo = rne_bf16(x - hi).  Precisions 1 and 3; the products are the GEMM's (a_hi w_hi + a_hi w_lo + a_lo w_hi in
 * fp32), summed over K in an order that depends on (Np, K, precision) only: the result is bit-reproducible, and row m of an M-row call is bit-identical to
 * the M = 1 call on that row.  Nothing past row M - 1 of x is read, nothing past row M - 1 of y is written.  x must be 16-byte aligned. */
int awt_linear_decode(awt_ctx* c, const awt_weight* w, const float* x, const float* resid, float* y, int M, void* stream);
/* dx [M, K] = dy [M, Np] W                                             (frozen weight: no weight gradient) */
int awt_linear_backward_input(awt_ctx* c, const awt_weight* w, const float* dy, float* dx, int M, void* workspace, size_t ws_bytes,
                              void* stream);
/* Batched products C_z [M, N] = A_z [M, K] B_z [N, K]^T (+ resid_z, may alias C_z), z < batch, split-bf16 operands on the MFMA GEMM, one launch.
 * The operators of the decoder's cross-attention in its ABSORBED form (HF:modeling_whisper.py:284-356 with `key_value_states`, re-associated:
 * q_h K_h^T = (q_h W_k,h) enc^T and P_h V_h = (P_h enc) W_v,h^T + b_v, so that with L ~ 12 label rows per clip the key / value projections
 * of the B x 1500 encoder rows are never computed; csrc/bmm.hip).  B_z is written once by awt_bmm_pack into the GEMM's weight layout (zero-padded
 * to N % 128 == 0, K % 64 == 0) and reused by every product against it; A_z, resid_z and C_z are row-major fp32 with pitches lda / ldo and strides
 * stride_a / stride_o between matrices (elements; strided views inside larger matrices are fine).  N, ldo, stride_o: multiples of 4. */
size_t awt_bmm_packed_bytes(int batch, int N, int K);
int awt_bmm_pack(awt_ctx* c, const float* b, int64_t ldb, int64_t stride_b, int batch, int N, int K, void* packed, size_t packed_bytes, void* stream);
size_t awt_bmm_workspace_bytes(int batch, int M, int K);
int awt_bmm(awt_ctx* c, const float* a, int64_t lda, int64_t stride_a, const void* packed_b, const float* resid, float* out, int64_t ldo,
            int64_t stride_o, int batch, int M, int N, int K, void* workspace, size_t ws_bytes, void* stream);
/* The same with an operand given K-MAJOR (i.e. transposed in memory), optionally as two matrices stacked along K:
 * X[n, k] = (k < K1 ? x1 : x2)[z * stride + (k < K1 ? k : k - K1) * ld + n]; x2 may be NULL when K1 == K.  The backward's
 * d(enc)_b = [P_b^T | dS_b^T] [d(context)_b ; q~_b] reads all four matrices where they lie. */
int awt_bmm_pack_kmajor(awt_ctx* c, const float* b1, const float* b2, int K1, int64_t ldb, int64_t stride_b, int batch, int N, int K, void* packed,
                        size_t packed_bytes, void* stream);
int awt_bmm_kmajor(awt_ctx* c, const float* a1, const float* a2, int K1, int64_t lda, int64_t stride_a, const void* packed_b, const float* resid, float* out,
                   int64_t ldo, int64_t stride_o, int batch, int M, int N, int K, void* workspace, size_t ws_bytes, void* stream);
/* p[r, :] = softmax(scale * s[r, :]) over cols <= 4096 columns (pitch ld; p may alias s), and its backward
 * ds[r, :] = scale * p[r, :] * (dp[r, :] - sum_c p[r, c] dp[r, c]) (ds may alias dp)                      HF:modeling_whisper.py:226-231 */
int awt_op_softmax_rows(awt_ctx* c, const float* s, float* p, int rows, int cols, int64_t ld, float scale, void* stream);
int awt_op_softmax_rows_backward(awt_ctx* c, const float* p, const float* dp, float* ds, int rows, int cols, int64_t ld, float scale, void* stream);
/* x[m, :] = embed_tokens[ids[m], :] + embed_positions[pos0 + m % L, :]     HF:modeling_whisper.py:756-770
 * One fp32 add per element.  d % 4 == 0.  An id outside [0, vocab) is clamped to the nearest valid row (0 or vocab - 1): the call cannot
 * fail without a synchronisation, and it never reads outside the table.  pos must hold pos0 + L rows. */
int awt_op_embed(awt_ctx* c, const int64_t* ids, const float* tok, const float* pos, float* x, int M, int L, int d, int pos0, int vocab,
                 void* stream);
int awt_op_gelu(awt_ctx* c, const float* x, float* y, int64_t n, void* stream);                          /* exact erf GELU */
int awt_op_gelu_backward(awt_ctx* c, const float* x, const float* dy, float* dx, int64_t n, void* stream);
/* dx = dres + d(LayerNorm(x) * gamma + beta)/dx . dy   (frozen affine: no dgamma / dbeta; dres NULL or the gradient arriving over the
 * residual connection; dx may alias dres) */
int awt_op_layernorm_backward(awt_ctx* c, const float* dy, const float* x, const float* gamma, const float* dres, float* dx, int M, int d,
                              float eps, void* stream);
/* Parameter gradients of trainable consumers of the operators (the UrbanSound8K Transformer classifier trains every weight,
 * /root/reference/.charles/spectrogram.py:1059-1130).  dgamma[c] = sum_m dy[m, c] xhat[m, c], dbeta[c] = sum_m dy[m, c];
 * column_sums: sums[c] = sum_m a[m, c] (bias gradients).  Deterministic two-pass reductions; d <= 1280. */
size_t awt_op_param_grad_workspace_bytes(int M, int d);
int awt_op_layernorm_param_grad(awt_ctx* c, const float* dy, const float* x, float* dgamma, float* dbeta, int M, int d, float eps,
                                void* workspace, size_t ws_bytes, void* stream);
int awt_op_column_sums(awt_ctx* c, const float* a, float* sums, int M, int d, void* workspace, size_t ws_bytes, void* stream);
/* Pitched form, any width: sums[c] (+)= sum_{m < M} a[m * ld + col + c], c < width (accumulate != 0 adds to sums).  width, col, ld multiples of 4,
 * 16-byte aligned tensors.  The decoder's bias gradients: fc1's 4 d columns, the q / v blocks of the fused [M, 3 d] gradient, the value blocks of
 * the [B S, 2 layers d] cross-attention buffer.  Deterministic: slabs of 256 rows summed top to bottom, then added in slab order. */
size_t awt_op_column_sums_ld_workspace_bytes(int M, int width);
int awt_op_column_sums_ld(awt_ctx* c, const float* a, int64_t ld, int col, int width, float* sums, int M, int accumulate, void* workspace,
                          size_t ws_bytes, void* stream);
/* Backward of awt_op_embed, ADDED to the two tables' gradients (the tied projection's gradient is already in dtok when this runs):
 *   dtok[v, :] += sum over {m : clamp(ids[m]) = v} of dx[m, :]        dpos[pos0 + l, :] += sum_b dx[b L + l, :]
 * ids are clamped as awt_op_embed clamps them.  No atomics: one workgroup owns a table row (the first row m naming it) and adds its terms in
 * ascending m, so two runs give the same bits; rows of dtok that no id names are not touched.  M a multiple of L, d a multiple of 4, d <= 2048. */
int awt_op_embed_backward(awt_ctx* c, const int64_t* ids, const float* dx, float* dtok, float* dpos, int M, int L, int d, int pos0, int vocab,
                          void* stream);
/* The weight-gradient GEMM of the full-parameter backward as an operator (csrc/wgrad.hip):
 *   out[n * sn + k * sk] (+)= scale * sum_{m < M} dy[m, ycol + n] * x[row(m), xcol + k]      n < N, k < K
 * dy fp32 [M, ldy], x fp32 [rows_x, ldx]; both are split into bf16 hi / lo planes inside; terms = 1 (one bf16 product) or 3 (split-bf16).
 * rows_out = 0: row(m) = m and rows_x = M.  rows_out > 0 (M % rows_out == 0, rows_x = M / rows_out * rows_in): row(m) =
 * (m / rows_out) * rows_in + (m % rows_out) * row_mul + row_add, and a row outside [0, rows_in) of its group reads as zero (conv2's taps:
 * rows_out = S, rows_in = 2 S, row_mul = 2, row_add = tap - 1).  N, K, ldy, ldx, ycol, xcol: multiples of 8; M * ldy, rows_x * ldx: multiples of 4.
 * accumulate != 0 adds to `out`.  Deterministic: the slab count depends on (M, N, K) only. */
size_t awt_op_weight_grad_workspace_bytes(int M, int rows_x, int ldy, int ldx, int N, int K);
int awt_op_weight_grad(awt_ctx* c, const float* dy, int ldy, int ycol, int N, const float* x, int rows_x, int ldx, int xcol, int K, int M,
                       int rows_out, int rows_in, int row_mul, int row_add, int terms, float scale, int accumulate, float* out, int64_t sn,
                       int64_t sk, void* workspace, size_t ws_bytes, void* stream);
/* CrossEntropyLoss(ignore_index = -100, mean) over the first `vocab` of `ld` columns: *loss and d(loss)/d(logits) [M, ld]
 * (padding columns zero).  scratch: (M + 1) * 4 bytes.                    HF:modeling_whisper.py:1079-1086
 * Only -100 is ignored.  Any other target outside [0, vocab) -- torch raises for it -- makes *loss NaN (the call itself cannot fail
 * without a synchronisation); the Python wrapper validates the labels on the host side and raises before launching. */
int awt_op_cross_entropy(awt_ctx* c, const float* logits, const int64_t* labels, int M, int vocab, int ld, float* loss, float* dlogits,
                         void* scratch, void* stream);
/* softmax(0.125 q k^T [+ causal mask]) v for head_dim 64 with few query rows.  Row (b, i) of q at q + (b Lq + i) ldq + 64 h; row
 * (b, j) of k / v at k + (b Sk + j) ldk + 64 h; o like q with ldo.  causal != 0: key j is visible to query i iff
 * j <= i + causal_off (causal_off = Sk - Lq for cached decoding).  lse [B, H, Lq] (optional) feeds the backward pass.
 * HF:modeling_whisper.py:215-238, 284-356 (q scaled by head_dim^-1/2; eager attention with the causal mask).
 * Refused with AWT_ERR_INVALID, by this entry and by every other one of the family (the backward, the dropout pair, awt_op_attention_cached): a null
 * pointer, a pitch below H * 64 or not a multiple of 4, B * H * Lq >= 2^31, causal != 0 with causal_off < 0 (the first query rows would see no key at
 * all: 0 / 0 in o, -inf in lse), and q, k, v, o -- in the backward also dout, dq, dk, dv -- not 16-byte aligned (the kernels use 16-byte accesses).
 * No atomics: two runs give the same bits. */
int awt_op_attention_small(awt_ctx* c, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo,
                           float* lse, int B, int H, int Lq, int Sk, int causal, int causal_off, void* stream);
/* dq (layout of q), dk / dv (layout of k / v: every element of the B x Sk x H x 64 blocks is written); delta [B, H, Lq] = rowsum(dout * o), an
 * output.  P is recomputed as exp(s - lse) with s formed by the forward's own instruction sequence, so that it is the forward's P to fp32 rounding
 * at any score magnitude. */
int awt_op_attention_small_backward(awt_ctx* c, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o,
                                    const float* dout, int ldo, const float* lse, float* delta, float* dq, float* dk, float* dv, int B,
                                    int H, int Lq, int Sk, int causal, int causal_off, void* stream);
/* The same pair with attention-probability dropout, what torch.nn.MultiheadAttention(dropout = p) applies in train()
 * (/root/reference/.charles/spectrogram.py:977-985): P <- P * keep / (1 - p) after the softmax, before P V.  keep is a pure function of
 * (seed, batch * H + head, query, key) -- splitmix64 of ((bh * Lq + i) * Sk + j) + seed * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019, top 24 bits
 * as a uniform in [0, 1), kept when >= p -- regenerated by the forward and both backward kernels from the same (drop_p, seed), never stored;
 * urbansound_classifier.attention_keep_mask restates it on the host for tests.  drop_p = 0 is the plain pair. */
int awt_op_attention_small_dropout(awt_ctx* c, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo,
                                   float* lse, int B, int H, int Lq, int Sk, int causal, int causal_off, float drop_p, uint64_t seed, void* stream);
int awt_op_attention_small_backward_dropout(awt_ctx* c, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o,
                                            const float* dout, int ldo, const float* lse, float* delta, float* dq, float* dk, float* dv, int B,
                                            int H, int Lq, int Sk, int causal, int causal_off, float drop_p, uint64_t seed, void* stream);

/* Multi-head cross-attention for head_dim 128 without a mask, Lq != Sk (csrc/cross_attention.hip; music2midi.CrossAttentionAdapter):
 *   o[b, i, h] = softmax_j(128^-1/2 q[b, i, h] . k[b, j, h]) v[b, j, h]
 * on fp32 row-major operands in place: row (b, i) of q at q + (b Lq + i) ldq + 128 h, row (b, j) of k / v at k + (b Sk + j) ldk + 128 h (k and v may be
 * the two halves of one [B Sk, 2 H 128] matrix), o like q with ldo.  The score scale is applied inside.  A flash-style kernel on the bf16 MFMAs: terms = 3
 * splits every operand (q, k, v and the probabilities of each 64-key tile) into bf16 hi + lo and forms three products, terms = 1 one; online softmax with
 * fp32 running max, sum and output.  lse [B, H, Lq] (optional, natural log) feeds the backward.  Any Lq, Sk >= 1.
 * Backward: dq (layout of q), dk / dv (layout of k / v), every element of the B x Lq x H x 128 and B x Sk x H x 128 blocks written; P is recomputed from lse,
 * nothing of size Lq x Sk is stored; o and dout are pitched ldo.  A rowsum(dout * o) launch, a dq launch and a dk / dv launch; no atomics: two runs give the
 * same bits.  Refused with AWT_ERR_INVALID: a pitch below H * 128 or not a multiple of 4, terms other than 1 or 3, a null pointer, tensors not 16-byte
 * aligned, a workspace smaller than awt_op_cross_attention_workspace_bytes (answers without a GPU; the forward needs none). */
size_t awt_op_cross_attention_workspace_bytes(int B, int H, int Lq, int Sk, int backward);
int awt_op_cross_attention(awt_ctx* c, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo, float* lse,
                           int B, int H, int Lq, int Sk, int terms, void* workspace, size_t ws_bytes, void* stream);
int awt_op_cross_attention_backward(awt_ctx* c, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o,
                                    const float* dout, int ldo, const float* lse, float* dq, float* dk, float* dv, int B, int H, int Lq, int Sk,
                                    int terms, void* workspace, size_t ws_bytes, void* stream);

/* The operators of a Qwen3 decoder layer (music2midi.Qwen3Decoder; csrc/qwen_ops.hip, and the causal variant of csrc/cross_attention.hip's forward).  fp32
 * row-major tensors in place, the caller's stream, no synchronisation; AWT_ERR_INVALID for a null pointer, a pitch that cannot hold its row or is not a multiple
 * of 4 (the vectorised operators), tensors not 16-byte aligned (the same), and the sizes named with each.
 *
 * RMSNorm: y[m, :] = gamma * x[m, :] * rsqrt(mean(x[m, :]^2) + eps), row m of x at x + m ldx, of y at y + m ldy (y may alias x).  d: any positive multiple
 * of 4.  One wave per row, the sum of squares in a fixed order (two runs give the same bits).                         HF:modeling_qwen3.py Qwen3RMSNorm */
int awt_op_rmsnorm(awt_ctx* c, const float* x, int64_t ldx, const float* gamma, float* y, int64_t ldy, int M, int d, float eps, void* stream);
/* Everything between a layer's fused q | k | v GEMM and its attention, one launch.  qkv [B Lq, ld]: Hq query heads, then Hkv key heads, then Hkv value
 * heads, 128 columns each.  Every q and k head gets the per-head RMSNorm over its 128 dims (q_gamma / k_gamma [128], eps) and THEN the rotary embedding in
 * HF's convention x cos + rotate_half(x) sin, dim i paired with i + 64, at the row's absolute position positions[r] (device int32 [B Lq]): cos / sin are
 * fp32 tables [rows, 64] built by the caller (angle = position * theta^(-2 i / 128)).  Rotated q goes to q_out + r ldq + 128 h; rotated k and the unchanged
 * v go into the decode cache at k_cache / v_cache + b kv_batch_stride + positions[r] ldkv + 128 h (b = r / Lq; v arrives bit-identical).  No other cache
 * row is touched.  A position outside the rows that fit a batch's stride, [0, (kv_batch_stride - Hkv 128) / ldkv], is clamped into it (the call cannot
 * fail without a synchronisation and never writes outside the cache); cos / sin must hold that many rows.       HF:modeling_qwen3.py Qwen3Attention.forward */
int awt_op_qk_norm_rope(awt_ctx* c, const float* qkv, int64_t ld, const float* q_gamma, const float* k_gamma, const float* cos, const float* sin,
                        const int32_t* positions, float* q_out, int64_t ldq, float* k_cache, float* v_cache, int64_t ldkv, int64_t kv_batch_stride,
                        int B, int Lq, int Hq, int Hkv, float eps, void* stream);
/* Causal attention for head_dim 128 with grouped KV heads over that cache: o[b, i, h] = softmax_j(128^-1/2 q[b, i, h] . k[b, j, g]) v[b, j, g] over the keys
 * j <= T - Lq + i of the T live positions (the contract of awt_op_attention_cached), g = h / (Hq / Hkv).  q / o as in awt_op_cross_attention (Hq heads,
 * ldq / ldo); key / value j of batch b at k / v + b kv_batch_stride + j ldkv + 128 g.  One kernel for prefill (Lq = T) and decoding (Lq = 1): the flash-style
 * bf16 MFMA forward of awt_op_cross_attention (terms 3 or 1, the score scale applied inside) in which a workgroup of 128 queries streams key tiles up to its
 * last query's diagonal only and masks inside the tiles it does stream.  No cache row at or past T is read -- the cache may be uninitialised there -- and
 * no atomics: two runs give the same bits.  Needs Hq % Hkv == 0, 1 <= Lq <= T, kv_batch_stride >= (T - 1) ldkv + Hkv 128.  The workspace query answers
 * without a GPU (the forward needs none: 0). */
size_t awt_op_causal_attention_workspace_bytes(int B, int Hq, int Lq, int T);
int awt_op_causal_attention(awt_ctx* c, const float* q, int ldq, const float* k, const float* v, int ldkv, int64_t kv_batch_stride, float* o, int ldo,
                            int B, int Hq, int Hkv, int Lq, int T, int terms, void* workspace, size_t ws_bytes, void* stream);
/* SwiGLU's element-wise half over the output gu [M, ld] of one gate | up GEMM of width 2 I: y[m, i] = silu(gu[m, i]) * gu[m, I + i], silu(x) = x / (1 + exp(-x)).
 * I: a positive multiple of 4; 16-byte accesses.                                                                   HF:modeling_qwen3.py Qwen3MLP */
int awt_op_silu_mul(awt_ctx* c, const float* gu, int64_t ld, float* y, int64_t ldy, int M, int I, void* stream);

/* The backward of those operators (training through music2midi.Qwen3Decoder).  fp32 in and out on the caller's stream, no
 * synchronisation, no atomics (two runs give the same bits); each refuses with AWT_ERR_INVALID what its forward counterpart refuses.
 *
 * awt_op_causal_attention with the log-sum-exp lse [B, Hq, Lq] (natural log) written out: the same kernel instantiation, what the backward reads. */
int awt_op_causal_attention_lse(awt_ctx* c, const float* q, int ldq, const float* k, const float* v, int ldkv, int64_t kv_batch_stride, float* o, int ldo,
                                float* lse, int B, int Hq, int Hkv, int Lq, int T, int terms, void* workspace, size_t ws_bytes, void* stream);
/* dq (layout of q: ldq, Hq heads), dk / dv (the cache's layout with their own pitch lddkv and batch stride dkv_batch_stride: row (b, j) at
 * dk + b dkv_batch_stride + j lddkv + 128 g) of that attention under the gradient dout of o (o and dout pitched ldo).  The forward's contract, 1 <= Lq <= T.
 * Every element of dq (B x Lq x Hq x 128) and of dk / dv (B x T x Hkv x 128) is written; nothing at or past row T of k / v is read.  Three launches:
 * delta = rowsum(dout * o); dq, a workgroup of 128 queries streaming key tiles up to its last query's diagonal; dk / dv, one workgroup per (batch, KV head,
 * 64-key block) that walks the group's Hq / Hkv query heads and, per head, the 32-query tiles from the first one that sees the block, with dk and dv kept in
 * registers across the heads (the group sum in a fixed order).  P is recomputed from lse.  The workspace query answers without a GPU. */
size_t awt_op_causal_attention_backward_workspace_bytes(int B, int Hq, int Lq, int T);
int awt_op_causal_attention_backward(awt_ctx* c, const float* q, int ldq, const float* k, const float* v, int ldkv, int64_t kv_batch_stride, const float* o,
                                     const float* dout, int ldo, const float* lse, float* dq, float* dk, float* dv, int lddkv, int64_t dkv_batch_stride,
                                     int B, int Hq, int Hkv, int Lq, int T, int terms, void* workspace, size_t ws_bytes, void* stream);
/* RMSNorm backward: with r = rsqrt(mean(x^2) + eps) and u = gamma * dy, dx = [dres +] r u - x r^3 mean(x u).  One wave per row; dy, x and dx pitched
 * lddy / ldx / lddx; dres (NULL, or the residual stream's gradient, pitched lddx; dx may alias it) is added in the same pass. */
int awt_op_rmsnorm_backward(awt_ctx* c, const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* gamma, const float* dres, float* dx,
                            int64_t lddx, int M, int d, float eps, void* stream);
/* dgamma[j] = sum_m dy[m, j] x[m, j] r_m: slabs of 256 rows summed top to bottom, then added in slab order (as awt_op_column_sums_ld).  The workspace
 * (256-byte aligned) holds r and the slabs; its query answers without a GPU. */
size_t awt_op_rmsnorm_param_grad_workspace_bytes(int M, int d);
int awt_op_rmsnorm_param_grad(awt_ctx* c, const float* dy, int64_t lddy, const float* x, int64_t ldx, float* dgamma, int M, int d, float eps,
                              void* workspace, size_t ws_bytes, void* stream);
/* SwiGLU backward over gu [M, ld] (the forward's input) and dy [M, lddy] into dgu [M, lddgu] (gate | up): with s = 1 / (1 + exp(-g)),
 * dgate = dy * up * s * (1 + g (1 - s)), dup = dy * g * s.  No overflow at any g. */
int awt_op_silu_mul_backward(awt_ctx* c, const float* gu, int64_t ld, const float* dy, int64_t lddy, float* dgu, int64_t lddgu, int M, int I, void* stream);
/* Backward of awt_op_qk_norm_rope into dqkv [B Lq, ld] (the layout of qkv), one wave per (row, head).  Inputs: the forward's qkv (pre-norm), gains, tables and
 * positions; dq (pitch ldq), the gradient of the rotated q; dk / dv, the gradients of the cache rows in the cache's layout (row (b, positions[r]) at
 * dk + b kv_batch_stride + positions[r] ldkv + 128 g).  q and k heads: the transposed rotation a' = a cos + b sin, b' = b cos - a sin of the pair (i, i + 64),
 * then the per-head RMSNorm backward with r recomputed from qkv; dv is copied (bit-identical).  dq_gamma / dk_gamma [128] (both or neither): the gains'
 * gradients summed over rows and heads in a fixed order (slabs of 256 (row, head) pairs), with the 256-byte aligned workspace of the query below. */
size_t awt_op_qk_norm_rope_backward_workspace_bytes(int B, int Lq, int Hq, int Hkv);
int awt_op_qk_norm_rope_backward(awt_ctx* c, const float* qkv, int64_t ld, const float* q_gamma, const float* k_gamma, const float* cos, const float* sin,
                                 const int32_t* positions, const float* dq, int64_t ldq, const float* dk, const float* dv, int64_t ldkv,
                                 int64_t kv_batch_stride, float* dqkv, float* dq_gamma, float* dk_gamma, int B, int Lq, int Hq, int Hkv, float eps,
                                 void* workspace, size_t ws_bytes, void* stream);

/* Causal attention of Lq new query rows per batch over a preallocated decode cache: keys / values of batch b, position j at
 * k + b kv_batch_stride + j ldkv + 64 h (likewise v), T live positions (T >= Lq; query i sees keys j <= T - Lq + i).  q / o as in
 * awt_op_attention_small.  The cache is [rows, Tmax, 2 d] per layer, so kv_batch_stride = Tmax ldkv (csrc/decoder_ops.hip). */
int awt_op_attention_cached(awt_ctx* c, const float* q, int ldq, const float* k, const float* v, int ldkv, int64_t kv_batch_stride, float* o,
                            int ldo, int B, int H, int Lq, int T, void* stream);
/* Next-token selection of generate (csrc/decode_select.hip), two launches, bit-reproducible.  rows = clips x beams rows of logits
 * (pitch ld >= vocab, ld % 4 == 0, 16-byte aligned; columns >= vocab are never read as candidates).  Per row: log-softmax over all
 * vocab columns when log_softmax != 0, then columns whose bit is set in `banned` ((vocab + 31) / 32 words, or NULL) become -inf, then
 * beam_scores[row] is added (NULL: 0).  Per clip: the k best of its beams x vocab candidates, best first (NaN first, ties to the lower
 * beam x vocab index): top_scores / top_tokens / top_parent [clips, k] (top_parent = beam within the clip; may be NULL).  beams <= 8,
 * k <= 16.  beams = 1, k = 1, log_softmax = 0 is torch.argmax after banning.  workspace: awt_select_tokens_workspace_bytes. */
size_t awt_select_tokens_workspace_bytes(int rows, int vocab, int k);
int awt_op_select_tokens(awt_ctx* c, const float* logits, int ld, int rows, int vocab, int beams, const uint32_t* banned, const float* beam_scores,
                         int log_softmax, int k, float* top_scores, int64_t* top_tokens, int32_t* top_parent, void* workspace, size_t ws_bytes,
                         void* stream);
/* awt_op_select_tokens with Whisper's timestamp rules (HF WhisperTimeStampLogitsProcessor) applied after `banned`, still two launches.
 * Per row (its token history: history + row * hist_ld, tokens [begin, cur_len) generated so far; timestamp_begin = no_timestamps + 1):
 * <|notimestamps|> banned; last token a timestamp and the one before it too (or none before it): timestamps banned; last a timestamp,
 * the one before not: [0, eos) banned; timestamps below the last timestamp banned (below last + 1 unless the last two are text then
 * timestamp); at cur_len == begin [0, timestamp_begin) and, when max_initial_timestamp_index >= 0, columns above timestamp_begin +
 * max_initial_timestamp_index banned; then, when logsumexp(timestamp columns) > max(text columns) of the banned row (no NaN), the text
 * columns become -inf.  log_softmax stays over the unbanned row.  rules = NULL is awt_op_select_tokens.  Candidates of score -inf come
 * in no specified order.  workspace: awt_select_tokens_ts_workspace_bytes. */
typedef struct awt_ts_rules {
  const int64_t* history;             /* device int64 [rows, hist_ld] */
  int64_t hist_ld;
  int begin, cur_len;
  int eos_token_id, no_timestamps_token_id;
  int max_initial_timestamp_index;    /* < 0: none */
} awt_ts_rules;
size_t awt_select_tokens_ts_workspace_bytes(int rows, int vocab, int k);
int awt_op_select_tokens_ts(awt_ctx* c, const float* logits, int ld, int rows, int vocab, int beams, const uint32_t* banned, const float* beam_scores,
                            int log_softmax, int k, const awt_ts_rules* rules, float* top_scores, int64_t* top_tokens, int32_t* top_parent,
                            void* workspace, size_t ws_bytes, void* stream);
/* dst[l, r, t, :] = src[l, parent[r], t, :] for l < layers, r < dst_rows, t < T of caches laid out [layers, rows, Tmax, width]
 * (src with src_rows rows, dst with dst_rows; width % 4 == 0; src != dst).  One launch.  A parent outside [0, src_rows) leaves its
 * destination row as it was.  Beam reorder (parent = surviving beams' parents) and the B -> B x beams expansion (parent = r / beams). */
int awt_op_kv_gather(awt_ctx* c, const float* src, float* dst, const int32_t* parent, int layers, int src_rows, int dst_rows, int T, int Tmax,
                     int width, void* stream);

/* Token-level timestamps of generate (csrc/alignment.hip; HF `_extract_token_timestamps`): three launches, no atomics, bit-reproducible.
 *
 * awt_op_alignment_weights: out[clip, s, t, :frames] = softmax_j(0.125 q . k_j) over ALL S <= 1536 encoder positions (the crop to
 * `frames` <= S applies to the stores only) for the n_sel selected heads s and token rows t < T.  q: the query rows kept while decoding,
 * fp32 [n_slots, rows, Tmax, d], position t0 + t; heads: device int32 [n_sel, 3] = (slot in q, decoder layer, head), out-of-range entries
 * are clamped; src_row: device int32 [clips, T], the row of q that decoded (clip, t) (beam search), clamped to [0, rows), or NULL: row
 * clip x group.  Keys: cross_kv fp32 [(rows / group) S, 2 n_layers d] (keys of layer l at column 2 l d), those of clip src_row / group.
 * Scores are formed as awt_op_attention_small forms them (fp32 operands, the same summation order).
 *
 * awt_op_alignment_matrix: weights fp32 [clips, n_sel, T, frames] -> out fp32 [clips, T, frames]: per (clip, head, frame) the z-score over
 * the T rows ((w - mean) / std, population std), a median of odd `width` <= 15 along the clip's first num_frames[clip] frames (device
 * int32, NULL: all `frames`) with reflect padding (no filter when that count is <= width / 2), then the mean over heads (n_sel <= 32).
 * Frames at and beyond a clip's count are written as 0.
 *
 * awt_op_dtw: HF `_dynamic_time_warping` of (negate ? -matrix : matrix)[clip, :T, :num_frames[clip]], matrix fp32 [clips, T, frames],
 * T <= 448: a float32 cost array whose cells are float(double(m) + double(c)), c the smallest of diagonal / up / left (strictly smaller
 * than both others wins, diagonal first, then up, otherwise left).  jump_frame int32 [clips, T]: the first frame of every token row on
 * the path.  The path itself (HF's text_indices / time_indices) ends at element T + frames of text_idx / time_idx (int32
 * [clips, T + frames]) and starts at path_start[clip].  workspace: awt_dtw_workspace_bytes (the trace). */
int awt_op_alignment_weights(awt_ctx* c, const float* q, int n_slots, int rows, int Tmax, int d, int group, const float* cross_kv, int n_layers,
                             int S, const int32_t* heads, int n_sel, const int32_t* src_row, int clips, int t0, int T, float* out, int frames,
                             void* stream);
int awt_op_alignment_matrix(awt_ctx* c, const float* weights, int clips, int n_sel, int T, int frames, const int32_t* num_frames, int width,
                            float* out, void* stream);
size_t awt_dtw_workspace_bytes(int clips, int T, int frames);
int awt_op_dtw(awt_ctx* c, const float* matrix, int clips, int T, int frames, const int32_t* num_frames, int negate, int32_t* jump_frame,
               int32_t* text_idx, int32_t* time_idx, int32_t* path_start, void* workspace, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Operators of the 1-D CNN classifier (csrc/cnn_ops.hip; cnn_classifier.py).  Activations are channels-last fp32 rows [B T, C] (clip b,
 * frame t at row b T + t), C a multiple of 4, tensors 16-byte aligned.  Deterministic: no atomics, fixed slabs of rows added in slab order.
 *
 * awt_op_conv1d: y[b, t, :] = bias + sum_tap x[b, t + tap - 1, :] w[:, :, tap]^T (Conv1d kernel_size 3, padding 1, stride 1; frames
 * outside [0, T) of the SAME clip read as zero) as one GEMM launch of three row-mapped K segments.  w: the fp32 Conv1d weight
 * [Cout, Cin, 3], packed into the workspace per call; taps must be 3; Cin % 64 == 0 (zero-pad the channels), Cout % 128 == 0; terms 1
 * (bf16), 3 (bf16x3) or 4 (fp16x3: fp16 hi + lo planes, 22 bits per operand, for operands inside fp16's range -- the forward).  The input gradient is the same call on dy with w'[ci, co, tap] = w[co, ci, 2 - tap]; the weight gradient is
 * awt_op_weight_grad per tap with the same row map, the bias gradient awt_op_column_sums. */
size_t awt_op_conv1d_workspace_bytes(int B, int T, int Cin, int Cout);
int awt_op_conv1d(awt_ctx* c, const float* x, const float* w, const float* bias, float* y, int B, int T, int Cin, int Cout, int taps, int terms,
                  void* workspace, size_t ws_bytes, void* stream);
/* Per-channel mean and BIASED variance of x [M, C] (training-mode BatchNorm1d's batch statistics), one read of x: per 64-row slab a
 * two-pass mean / sum of squared deviations in registers, the slabs merged in order with the pairwise update of Chan et al. (never
 * E[x^2] - E[x]^2).  A constant column gives var = 0 exactly. */
size_t awt_op_batchnorm_stats_workspace_bytes(int M, int C);
int awt_op_batchnorm_stats(awt_ctx* c, const float* x, int M, int C, float* mean, float* var, void* workspace, size_t ws_bytes, void* stream);
/* y = pool(relu((x - mean) (var + eps)^-1/2 gamma + beta)) in one pass over x [B T, C]; mean / var are the batch statistics (train) or
 * the running statistics (eval).  `pool`:
 *   AWT_POOL_MEAN       the mean over T (AdaptiveAvgPool1d(1)), y [B, C];
 *   AWT_POOL_MAX2       MaxPool1d(2, 2) along T inside each clip, y [B (T / 2), C], an odd T drops its last frame (T >= 2);
 *   AWT_POOL_MAX4       MaxPool1d(4), y [B (T / 4), C], the trailing T mod 4 frames are dropped (T >= 4);
 *   AWT_POOL_MAX4_MEAN  MaxPool1d(4) then AdaptiveAvgPool1d(1): y [B, C] = the mean over the T / 4 pooled frames, added in frame order; the
 *                       pooled tensor is never written (T >= 4).
 * Any other value is refused. */
enum { AWT_POOL_MEAN = 0, AWT_POOL_MAX2 = 2, AWT_POOL_MAX4 = 4, AWT_POOL_MAX4_MEAN = 5 };
int awt_op_bn_relu_pool(awt_ctx* c, const float* x, const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                        float* y, int B, int T, int C, int pool, void* stream);
/* Backward of awt_op_bn_relu_pool under BATCH statistics (mean / var = awt_op_batchnorm_stats of x, M = B T): from dy (the pooled
 * gradient) and the saved pre-BN x, with the ReLU mask and the pooling winner recomputed (nothing else is stored),
 *   dbeta = sum dz, dgamma = sum dz xhat, dx = gamma rstd (dz - dbeta / M - xhat dgamma / M),  dz = the gradient at the BatchNorm output
 * (frames that the max-pool drops have dz = 0; the winner of a window is the FIRST frame with its largest pre-ReLU value, torch's tie-break;
 * AWT_POOL_MAX4_MEAN: dz at a winner is dy[b] / (T / 4)).  Three launches: slab partials of the two sums (reads x once), their sum in slab order
 * ([slabs, 2 C] floats), dx (reads x once). */
size_t awt_op_bn_relu_pool_backward_workspace_bytes(int B, int T, int C);
int awt_op_bn_relu_pool_backward(awt_ctx* c, const float* dy, const float* x, const float* mean, const float* var, const float* gamma,
                                 const float* beta, float eps, float* dx, float* dgamma, float* dbeta, int B, int T, int C, int pool,
                                 void* workspace, size_t ws_bytes, void* stream);

/* Conv1d(1, Cout, kernel, stride) without padding on raw waveforms (CNNWaveformClassifier's first layer):
 *   y[b, t, co] = bias[co] + sum_{k < kernel} x[b * x_pitch + t * stride + k] * w[co, 0, k],   t < T1 = (n_samples - kernel) / stride + 1,
 * x fp32 [B, n_samples] at a clip pitch of x_pitch floats, w the fp32 nn.Conv1d weight [Cout, 1, kernel], y channels-last rows [B T1, Cout].
 * Exact fp32: the products are formed on v_mfma_f32_16x16x4_f32, so each output is the k-ordered fmaf chain that starts at the bias.  A workgroup
 * stages the samples of 128 consecutive frames and the weight in LDS once; no workspace, no atomics, deterministic.  Required: stride % 8 == 0,
 * kernel % stride == 0, n_samples >= kernel, Cout % 16 == 0, (127 + kernel / stride) (stride + 4) + Cout (kernel + 4) <= 16384 (64 KiB of LDS),
 * x_pitch >= n_samples and x_pitch % 4 == 0, B <= 65535, 16-byte aligned tensors.  Samples past the last frame are not read.  The weight gradient
 * is awt_op_weight_grad per block of `stride` taps over the waveform viewed as rows of `stride` samples, the bias gradient awt_op_column_sums. */
int awt_op_conv1d_framed(awt_ctx* c, const float* x, int64_t x_pitch, const float* w, const float* bias, float* y, int B, int n_samples, int kernel,
                         int stride, int Cout, void* stream);

/* Process-wide tuning / test hooks.  key "gemm_tile": 0 = choose the GEMM block tile from the shape (default), 64 / 128 / 256 =
 * force the 64 x 128, 128 x 128 or 128 x 256 tile (256 falls back to 128 when N is not a multiple of 256) so that tests can
 * drive every tiling on small shapes.
 * "gemm_gm": row panels per tile-order group (0 = default).  "attn_shape": form of the f16f8 attention kernel (software-pipelined,
 * 32 queries per wave), 0 = automatic: P V as one fp16 product on 4 waves without lse (inference), every cross term with lse
 * (training; 8 waves when the grid has at least 256 eight-wave workgroups, else 4); 4 / 5 = every cross term, the e4m3 cross terms of
 * P V included, on 4 / 8 waves; 6 = P V as one fp16 product on 4 waves (what 0 selects for inference).  Other values are refused.
 * Only dropping P V's cross terms changes results (within the tolerances of DESIGN.md section 3); the number of waves is bit-neutral.
 * "attn_qt": query tiles per wave of the bf16 / fp16 / bf16x3 / fp16x3 attention kernel, so that tests can drive both instantiations on
 * small shapes: 0 = chosen from the grid size (default: one tile, 128 queries per workgroup, on grids that two tiles would leave under
 * or unevenly filling the device; else two, 256 queries), 1 / 2 = force that instantiation.  Other values are refused.  The f16f8
 * kernel ("attn_shape") is not affected.
 * "gemm_pp": the persistent 256 x 256 eight-wave "ping-pong" f16f8 GEMM (csrc/gemm_pp.h: both operands by LDS-DMA, split-line
 * activations, 16 x 16 MFMAs, one workgroup per CU walking its tiles): 0 = off, 1 = automatic (default: inference launches of at
 * least one tile per CU whose tile count fills its rounds of persistent workgroups to 5/6 or better, on weights that are not fp16-exact), 2 = wherever it applies (N % 256 == 0, K % 64 == 0, K >= 128, no adapter; also
 * awt_op_linear).  "gemm_pp_mask": which projections of a layer may take it, a bit set (1 qkv, 2 out_proj, 4 fc1, 8 fc2; fc2 only with
 * fc1; default 12 = the MLP pair, where it is measurably ahead).  Same products and the same accumulation order per output as the
 * 128 x 256 kernel's 16 x 16 form: bit-identical results where both apply.
 * "gemm_mfma16": 1 (default) = the 128 x 256 f16f8 GEMM issues its products as 16 x 16 MFMAs (both e4m3 cross terms in one block-scaled
 * instruction), 0 = the 32 x 32 form (results differ by the fp32 summation order only).
 * "conv_live": 1 (default) = awt_audio_encode's conv stem computes awt_conv_stem_positions(n_ctx, max_valid) positions per clip and
 * copies the padded tail, 0 = it always computes every position.  Bit-identical results; the knob exists for A/B runs and tests. */
int awt_tuning_set(const char* key, int value);

/* ------------------------------------------------------------------------------------------------------
 * In-library kernel timing with HIP events on the caller's stream (bench.py's `roofline` leg).
 * awt_prof_enable(c, mask) makes every launch of the kernel classes whose bit (1 << AWT_PROF_x) is set in `mask`
 * record an event pair (mask 0 = off);
 * awt_prof_collect synchronises the events and returns accumulated milliseconds and launch count
 * for one class, then resets that class. */
enum { AWT_PROF_LOGMEL = 0, AWT_PROF_GEMM = 1, AWT_PROF_ATTENTION = 2, AWT_PROF_LAYERNORM = 3, AWT_PROF_OTHER = 4,
       AWT_PROF_ATTENTION_BWD = 5,     /* the attention backward launches (fine-tune step), apart from the forward kernel */
       AWT_PROF_WGRAD = 6,             /* the weight-gradient GEMM launches of the full-parameter backward (both of each pair) */
       AWT_PROF_NCLASSES = 7 };
int awt_prof_enable(awt_ctx* c, int mask);
int awt_prof_collect(awt_ctx* c, int klass, double* total_ms, int64_t* launches, double* flops);

#ifdef __cplusplus
}
#endif
#endif /* AWT_H_ */
