// libawt C-ABI (include/awt.h): handles, weight upload, encoder forward orchestration, profiling hooks.
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "common.h"
#include "comm.h"
#include "wgrad.h"

// ------------------------------------------------------------------------------------------------ errors
static thread_local std::string g_err;
void awt_set_error(const std::string& msg) { g_err = msg; }
int awt_fail(int code, const std::string& msg) { g_err = msg; return code; }
extern "C" const char* awt_last_error(void) { return g_err.c_str(); }
extern "C" const char* awt_version(void) { return "awt 0.1 (gfx950)"; }

// ------------------------------------------------------------------------------------------------ profiling
struct awt_prof_state {
  struct Span { hipEvent_t a, b; };
  std::vector<Span> spans[AWT_PROF_NCLASSES];
  std::vector<Span> pool;
  double flops[AWT_PROF_NCLASSES] = {};
  Span open[AWT_PROF_NCLASSES];
};

void awt_prof_begin(awt_ctx* c, int klass, hipStream_t s, double flops) {
  awt_prof_state* p = c->prof;
  awt_prof_state::Span sp;
  if (!p->pool.empty()) { sp = p->pool.back(); p->pool.pop_back(); }
  else { (void)hipEventCreate(&sp.a); (void)hipEventCreate(&sp.b); }
  (void)hipEventRecord(sp.a, s);
  p->open[klass] = sp;
  p->flops[klass] += flops;
}
void awt_prof_end(awt_ctx* c, int klass, hipStream_t s) {
  awt_prof_state* p = c->prof;
  (void)hipEventRecord(p->open[klass].b, s);
  p->spans[klass].push_back(p->open[klass]);
}

static int g_conv_live = 1;  // tuning knob "conv_live": 1 = awt_audio_encode's conv stem computes the live positions only (conv_stem), 0 = always every position
static int g_pp_mask = 12;   // tuning knob "gemm_pp_mask": which of a layer's four projections may take the ping-pong GEMM (default: fc1 + fc2, profiles/r04_gemm_pp16_masks.txt)
extern "C" int awt_tuning_set(const char* key, int value) {
  AWT_REQUIRE(key, AWT_ERR_INVALID, "tuning_set: null key");
  if (!strcmp(key, "gemm_tile")) {
    AWT_REQUIRE(value == 0 || value == 64 || value == 128 || value == 256, AWT_ERR_INVALID, "tuning_set: gemm_tile must be 0 (auto), 64, 128 or 256");
    awt_gemm_force_tile(value);
    return AWT_OK;
  }
  if (!strcmp(key, "gemm_gm")) {
    AWT_REQUIRE(value >= 0 && value <= 64, AWT_ERR_INVALID, "tuning_set: gemm_gm must be 0 (default) .. 64");
    awt_gemm_set_gm(value);
    return AWT_OK;
  }
  if (!strcmp(key, "gemm_pp")) {
    AWT_REQUIRE(value >= 0 && value <= 2, AWT_ERR_INVALID, "tuning_set: gemm_pp must be 0 (off), 1 (automatic, default) or 2 (wherever supported)");
    awt_gemm_set_pp_mode(value);
    return AWT_OK;
  }
  if (!strcmp(key, "gemm_pp_mask")) {
    AWT_REQUIRE(value >= 0 && value <= 15, AWT_ERR_INVALID, "tuning_set: gemm_pp_mask is a bit set 0 .. 15 (1 qkv, 2 out_proj, 4 fc1, 8 fc2; fc2 only together with fc1)");
    g_pp_mask = value;
    return AWT_OK;
  }
  if (!strcmp(key, "gemm_mfma16")) {
    AWT_REQUIRE(value == 0 || value == 1, AWT_ERR_INVALID, "tuning_set: gemm_mfma16 must be 1 (default: the f16f8 GEMM's 16 x 16 MFMA form where it applies) or 0 (32 x 32 only)");
    awt_gemm_set_mfma16(value);
    return AWT_OK;
  }
  if (!strcmp(key, "conv_live")) {
    AWT_REQUIRE(value == 0 || value == 1, AWT_ERR_INVALID, "tuning_set: conv_live must be 1 (default: the conv stem of awt_audio_encode computes the live positions only) or 0 (every position)");
    g_conv_live = value;
    return AWT_OK;
  }
  if (!strcmp(key, "attn_shape")) {
    AWT_REQUIRE(value == 0 || (value >= 4 && value <= 6), AWT_ERR_INVALID, "tuning_set: attn_shape must be 0 (auto), 4, 5 or 6");
    awt_attn_force_shape(value);
    return AWT_OK;
  }
  if (!strcmp(key, "attn_qt")) {
    AWT_REQUIRE(value >= 0 && value <= 2, AWT_ERR_INVALID, "tuning_set: attn_qt must be 0 (auto), 1 or 2");
    awt_attn_force_qt(value);
    return AWT_OK;
  }
  AWT_REQUIRE(false, AWT_ERR_INVALID, "tuning_set: unknown key");
}

extern "C" int awt_prof_enable(awt_ctx* c, int on) {
  AWT_REQUIRE(c, AWT_ERR_INVALID, "prof_enable: null ctx");
  if (!c->prof) c->prof = new awt_prof_state();
  c->prof_on = on;   // bit k enables kernel class k (AWT_PROF_*)
  return AWT_OK;
}
extern "C" int awt_prof_collect(awt_ctx* c, int klass, double* total_ms, int64_t* launches, double* flops) {
  AWT_REQUIRE(c && c->prof && klass >= 0 && klass < AWT_PROF_NCLASSES, AWT_ERR_INVALID, "prof_collect: bad argument");
  awt_prof_state* p = c->prof;
  double ms = 0;
  for (auto& sp : p->spans[klass]) {
    AWT_HIP_CHECK(hipEventSynchronize(sp.b));
    float t = 0;
    AWT_HIP_CHECK(hipEventElapsedTime(&t, sp.a, sp.b));
    ms += t;
    p->pool.push_back(sp);
  }
  if (total_ms) *total_ms = ms;
  if (launches) *launches = (int64_t)p->spans[klass].size();
  if (flops) *flops = p->flops[klass];
  p->spans[klass].clear();
  p->flops[klass] = 0;
  return AWT_OK;
}

// ------------------------------------------------------------------------------------------------ ctx
extern "C" int awt_ctx_create(int device, awt_ctx** out) {
  AWT_REQUIRE(out, AWT_ERR_INVALID, "ctx_create: null out");
  int n = 0;
  AWT_HIP_CHECK(hipGetDeviceCount(&n));
  AWT_REQUIRE(device >= 0 && device < n, AWT_ERR_INVALID, "ctx_create: no such device");
  AWT_HIP_CHECK(hipSetDevice(device));
  hipDeviceProp_t prop;
  AWT_HIP_CHECK(hipGetDeviceProperties(&prop, device));
  AWT_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0, AWT_ERR_INVALID,
              std::string("libawt is built for gfx950 (MI355X) only; device is ") + prop.gcnArchName);
  awt_ctx* c = new awt_ctx();
  c->device = device;
  if (hipMalloc(&c->zeros, 256) != hipSuccess || hipMemset(c->zeros, 0, 256) != hipSuccess) {
    delete c;
    AWT_REQUIRE(false, AWT_ERR_HIP, "ctx_create: could not allocate the zero page");
  }
  // the two Whisper front-ends' tables (DFT basis of 400, Slaney banks of 80 and 128 bins) are built here, so that no compute call
  // of the hot path allocates or synchronises; other front-end configurations: awt_logmel_prepare / awt_resample_prepare
  int rc = logmel_prepare_impl(c, 400, 80, 0.0, 8000.0, 16000, 1);
  if (!rc) rc = logmel_prepare_impl(c, 400, 128, 0.0, 8000.0, 16000, 1);
  if (rc) { awt_ctx_destroy(c); return rc; }
  *out = c;
  return AWT_OK;
}
extern "C" int awt_logmel_prepare(awt_ctx* c, int n_fft, int n_mels, float f_min, float f_max, int sample_rate, int slaney) {
  return logmel_prepare_impl(c, n_fft, n_mels, (double)f_min, (double)f_max, sample_rate, slaney);
}
extern "C" int awt_resample_prepare(awt_ctx* c, int sr_in, int sr_out) { return resample_prepare_impl(c, sr_in, sr_out); }
extern "C" void awt_ctx_destroy(awt_ctx* c) {
  if (!c) return;
  awt_free_tables(c);
  if (c->zeros) (void)hipFree(c->zeros);
  if (c->prof) {
    for (int k = 0; k < AWT_PROF_NCLASSES; ++k)
      for (auto& sp : c->prof->spans[k]) { (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b); }
    for (auto& sp : c->prof->pool) { (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b); }
    delete c->prof;
  }
  delete c;
}

extern "C" int awt_logmel_whisper(awt_ctx* c, const void* pcm, int pcm_is_i16, int64_t pcm_stride, const int32_t* n_valid,
                                  int max_valid, int B, int n_frames_out, float* out, void* workspace, size_t ws_bytes,
                                  void* stream) {
  return logmel_whisper_impl(c, pcm, pcm_is_i16, pcm_stride, n_valid, max_valid, B, n_frames_out, 80, out, workspace, ws_bytes,
                             (hipStream_t)stream);
}
extern "C" int awt_logmel_whisper_mels(awt_ctx* c, const void* pcm, int pcm_is_i16, int64_t pcm_stride, const int32_t* n_valid,
                                       int max_valid, int B, int n_frames_out, int n_mels, float* out, void* workspace, size_t ws_bytes,
                                       void* stream) {
  return logmel_whisper_impl(c, pcm, pcm_is_i16, pcm_stride, n_valid, max_valid, B, n_frames_out, n_mels, out, workspace, ws_bytes,
                             (hipStream_t)stream);
}
extern "C" int awt_logmel_whisper_signal(awt_ctx* c, const void* pcm, int pcm_is_i16, int64_t pcm_stride, const int32_t* n_valid,
                                         int max_valid, int B, int n_signal, int n_mels, float* out, void* workspace, size_t ws_bytes,
                                         void* stream) {
  return logmel_whisper_impl(c, pcm, pcm_is_i16, pcm_stride, n_valid, max_valid, B, 0, n_mels, out, workspace, ws_bytes, (hipStream_t)stream,
                             n_signal);
}
extern "C" int awt_logmel_generic(awt_ctx* c, const float* pcm, int64_t pcm_stride, int B, int n_samples, int sample_rate,
                                  int n_fft, int hop, int n_mels, float f_min, float f_max, float log_eps, float* out,
                                  void* stream) {
  return logmel_generic_impl(c, pcm, pcm_stride, B, n_samples, sample_rate, n_fft, hop, n_mels, f_min, f_max, log_eps, out,
                             (hipStream_t)stream);
}

extern "C" int64_t awt_resampled_length(int n_in, int sr_in, int sr_out) {
  if (n_in <= 0 || sr_in <= 0 || sr_out <= 0) return 0;
  return resampled_length(n_in, sr_in, sr_out);
}
extern "C" int awt_prepare_waveform(awt_ctx* c, const void* pcm, int pcm_is_i16, int channels, int64_t channel_stride,
                                    int64_t sample_stride, int n_in, int sr_in, int sr_out, float* out, int n_out, void* stream) {
  return prepare_waveform_impl(c, pcm, pcm_is_i16, channels, channel_stride, sample_stride, n_in, sr_in, sr_out, out, n_out,
                               (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------ encoder
namespace {

struct Planes {  // a weight matrix as operand planes owned by the library: hi (+ lo); f16f8: hi = fp16, lo = hi8 and x8 = lo8 planes
  bf16_t* hi = nullptr; bf16_t* lo = nullptr; uint8_t* x8 = nullptr; int64_t rows = 0, ld = 0;
  // PREC_F16F8 inference: one device flag per separately uploaded row block (q | k | v): "a weight of this block is not exactly fp16";
  // exact16 = no flag set = the lo8 image is all zero and the GEMM drops that cross term (gemm.hip, WX)
  int* d_inexact = nullptr; bool exact16 = false;
  int64_t s_rows = 0;                             // rows s16 / s8 are allocated for: `rows` rounded up to whole 256-column tiles
  bf16_t* s16 = nullptr; uint8_t* s8 = nullptr;   // f16f8: the 16-row fragment copies the 16 x 16 MFMA form of the GEMM reads (w_frag_index / w8s_index; common.h)
  char* pp = nullptr;   // PREC_F16F8 inference: the same matrix in the packed region image of the ping-pong GEMM (gemm_pp.h), N % 256 == 0 only
};
struct Linear {
  Planes w; float* bias = nullptr; int N = 0, K = 0;
};
struct LoraGroup {   // adapters that share one input (q/k/v share LN1's output)
  bool active = false;
  Planes a;          // [128, K_in]: rows slot * r .. slot * r + r - 1 hold adapter `slot`'s A
  Planes b;          // [N_out, kp]: columns slot * r .. hold B (pre-scaling is applied to u, not to B)
  Planes bT;         // training: [128, N_out] = B^T  (weight of du = dy B)
  Planes aT;         // training: [K_in, kp]  = (alpha / r) A^T  (weight of the adapter term of dx)
  int kp = 0;
};
struct Layer {
  Linear qkv, out, fc1, fc2;
  Planes qkvT, outT, fc1T, fc2T;   // training: transposed copies [K, N] of the frozen weights (dX = dY W)
  Planes fc1T8, fc2T8;             // backward_terms = 5: the MLP's transposed copies in the f16f8 weight format (the MLP's two backward GEMMs run in it)
  Planes fc1_8, fc2_8;             // ... and its forward weights in the same format (the training forward's fc1 / fc2 run in it too)
  float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
  LoraGroup lq, lo_, l1, l2;
};

// conv1 as a GEMM: K = 3 taps x n_mels, zero-padded to a multiple of 64 (80 mels: 256, 128 mels: 384)
int conv1_k(int n_mels) { return (3 * n_mels + 63) / 64 * 64; }

}  // namespace

struct awt_encoder {
  awt_ctx* ctx = nullptr;
  awt_encoder_cfg cfg{};
  int planes = 1;          // 2-byte-per-element planes per matrix: 1 (bf16) or 2 (hi + lo; f16f8: fp16 + the two e4m3 planes)
  int prec = PREC_BF16X3;  // operand precision of the forward pass (cfg.mfma_terms: common.h PREC_*)
  Linear conv1, conv2;
  float* pos = nullptr;    // [S, d]
  float* zero_row = nullptr;   // [d] zeros: the "positional table" of the compact conv stem's conv2 (conv_stem)
  float *lnf_g = nullptr, *lnf_b = nullptr;
  std::vector<Layer> layers;
  std::vector<void*> allocs;
  std::vector<std::string> seen;   // names uploaded so far
  int chunk = 16;
  awt_comm* comm = nullptr;        // AWT_BWD_ALLREDUCE: adapter gradients are averaged over this communicator's ranks
  int comm_groups = 2;
  bool mlp_f8 = false;             // cfg.backward_terms == 5: the MLP's backward GEMMs in f16f8 (the others in split-bf16)
  float* wt_tmp = nullptr;         // [ffn_dim * d_model] fp32: W^T of the matrix being uploaded (packed into fc1T8 / fc2T8)
  int grad_scale_log2 = 0;         // awt_encoder_set_grad_scale_log2: the backward pass carries 2^k x the gradient (fp16 planes), adapter gradients leave unscaled
  // cfg.train_base: the backward pass produces the gradient of every base parameter but the position table (no adapters in this mode)
  bool train_base = false;
  Planes conv2T[3];                // per tap dt: [d, d] = conv2.weight[:, :, dt]^T (weight of d h1 = d pre2 W2)
  struct GradEntry { std::string name; size_t offset; int64_t shape[3]; int rank; };
  std::vector<GradEntry> glayout;  // the flat gradient buffer: the non-layer parameters, then one contiguous block per layer, layers in order
  size_t g_head = 0, g_per_layer = 0;
  // where the backward pass writes, filled with glayout by build_grad_layout: the head's entries from the buffer's start (lnf: layer_norm.weight, its
  // bias follows), a layer's from the start of its block (qkvw: q | k | v weights; ln1 / ln2: weight, then bias)
  struct GradOffsets { size_t c1w, c1b, c2w, c2b, lnf, qkvw, qb, vb, ow, ob, ln1, f1w, f1b, f2w, f2b, ln2; } goff{};
};

namespace {

int dev_alloc(awt_encoder* e, void** p, size_t bytes) {
  AWT_HIP_CHECK(hipMalloc(p, bytes));
  AWT_HIP_CHECK(hipMemset(*p, 0, bytes));
  e->allocs.push_back(*p);
  return AWT_OK;
}
// the planes of a [rows, ld] weight in the operand format of `prec` (the forward's, or PREC_F16F8 for the f16f8 MLP of a split-bf16 training step)
int alloc_planes(awt_encoder* e, Planes* pl, int64_t rows, int64_t ld, int prec) {
  pl->rows = rows; pl->ld = ld;
  int rc = dev_alloc(e, (void**)&pl->hi, (size_t)rows * ld * 2); if (rc) return rc;
  if (prec_products(prec) == 3) { rc = dev_alloc(e, (void**)&pl->lo, (size_t)rows * ld * 2); if (rc) return rc; }
  if (prec == PREC_F16F8) {
    pl->x8 = (uint8_t*)pl->lo + (size_t)rows * ld;
    pl->s_rows = (rows + 255) / 256 * 256;
    rc = dev_alloc(e, (void**)&pl->s16, (size_t)pl->s_rows * ld * 2); if (rc) return rc;
    rc = dev_alloc(e, (void**)&pl->s8, (size_t)pl->s_rows * ld * 2); if (rc) return rc;
  }
  return AWT_OK;
}
int alloc_linear(awt_encoder* e, Linear* l, int N, int K) {
  l->N = N; l->K = K;
  int rc = alloc_planes(e, &l->w, N, K, e->prec); if (rc) return rc;
  return dev_alloc(e, (void**)&l->bias, (size_t)N * 4);
}
int alloc_lora(awt_encoder* e, LoraGroup* g, int slots, int K_in, int N_out) {
  g->active = true;
  g->kp = (int)(((int64_t)slots * e->cfg.lora_rank + 63) / 64 * 64);
  int rc = alloc_planes(e, &g->a, 128, K_in, e->prec); if (rc) return rc;
  rc = alloc_planes(e, &g->b, N_out, g->kp, e->prec); if (rc) return rc;
  if (e->cfg.training) {
    rc = alloc_planes(e, &g->bT, 128, N_out, e->prec); if (rc) return rc;
    rc = alloc_planes(e, &g->aT, K_in, g->kp, e->prec); if (rc) return rc;
  }
  return AWT_OK;
}
// src [N, C, taps] fp32 into rows row_off .., columns col_off .. of `pl` in the operand format of `prec` (launch_pack_weight); flag: see probe_exact16
int pack(awt_ctx* c, const float* src, Planes& pl, int N, int C, int taps, int row_off, int col_off, int prec, hipStream_t s, int* flag = nullptr) {
  return launch_pack_weight(c, src, N, C, taps, pl.ld, row_off, col_off, 1.0f, pl.hi, pl.lo, pl.x8, prec, s, flag, pl.s16, pl.s8);
}
// pack() of a plain [N, K] block that also finds out whether the matrix is fp16-exact (checkpoints stored in half precision), which lets the GEMM drop one
// cross term: device flag `which` of `flags` is reset, the pack sets it at the first weight that is not, and pl.exact16 = none of the `nflags` flags
// (one per separately uploaded row block) is set.  Synchronises the stream: upload time only.  `who` names the caller in the error texts.
int probe_exact16(awt_ctx* c, const char* who, const float* src, Planes& pl, int N, int K, int row_off, int prec, int* flags, int which, int nflags, hipStream_t s) {
  int host[4] = {0, 0, 0, 0};
  if (hipMemsetAsync(flags + which, 0, sizeof(int), s) != hipSuccess) return awt_fail(AWT_ERR_HIP, std::string(who) + ": flag reset failed");
  int rc = pack(c, src, pl, N, K, 1, row_off, 0, prec, s, flags + which); if (rc) return rc;
  if (hipMemcpyAsync(host, flags, nflags * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return awt_fail(AWT_ERR_HIP, std::string(who) + ": flag read-back failed");
  pl.exact16 = !(host[0] | host[1] | host[2] | host[3]);
  return AWT_OK;
}

// conv-phase planes for Mt = clips x frames rows: the im2col rows [Mt, conv1_k], conv1's output [Mt, d] and, for train_base (`keep_pre1`), conv1's
// pre-activation [Mt, d].  The one carve of them: the inference workspace, its compact-stem form and the training buffer all call it.
struct ConvPlanes { PlanePair a1, h1, pre1; };
ConvPlanes take_conv_planes(const awt_encoder* e, Carver& cv, size_t Mt, bool keep_pre1) {
  const size_t d = e->cfg.d_model;
  ConvPlanes p;
  p.a1 = take_planes(cv, Mt * conv1_k(e->cfg.n_mels), e->planes);
  p.h1 = take_planes(cv, Mt * d, e->planes);
  if (keep_pre1) p.pre1 = take_planes(cv, Mt * d, e->planes);
  return p;
}

struct Workspace {  // per-chunk buffers carved from the caller's workspace
  float* x; PlanePair ln, qkv, att, ff, u; ConvPlanes conv;
  size_t bytes;
};

Workspace carve(const awt_encoder* e, char* base, int Bc) {
  const awt_encoder_cfg& c = e->cfg;
  const size_t S = c.n_ctx, T = 2 * S, d = c.d_model, f = c.ffn_dim;
  const size_t M = (size_t)Bc * S, Mt = (size_t)Bc * T;
  const int P = e->planes;
  Workspace w{};
  Carver cv(base);
  w.x = cv.take<float>(M * d * 4);
  w.ln = take_planes(cv, M * d, P);
  w.u = take_planes(cv, M * 128, P);
  // layer-phase buffers; the conv-phase buffers (im2col rows and conv1 output) alias the same region
  const size_t layer_start = cv.off;
  w.qkv = take_planes(cv, 3 * M * d, P);
  w.att = take_planes(cv, M * d, P);
  w.ff = take_planes(cv, M * f, P);
  const size_t layer_end = cv.off;
  cv.off = layer_start;
  w.conv = take_conv_planes(e, cv, Mt, false);
  w.bytes = std::max(cv.off, layer_end);
  // the ping-pong GEMM reads whole 256-row panels of its activation: up to 255 rows past the last buffer's end (never stored)
  if (e->prec == PREC_F16F8 && !c.training) w.bytes += align_up((size_t)256 * std::max(f, (size_t)conv1_k(c.n_mels)) * 4);
  return w;
}

// the one view of a buffer's plane pair (`elems` elements) as operand planes of precision `prec`; made once where the buffer is named
Act make_act(const PlanePair& p, size_t elems, int prec) {
  Act a;
  a.p16 = p.hi;
  if (prec == PREC_F16F8) { a.hi8 = (uint8_t*)p.lo; a.lo8 = a.hi8 ? a.hi8 + elems : nullptr; }
  else a.lo16 = p.lo;
  return a;
}
Act act_offset(const Act& a, int64_t elems) {
  Act r;
  r.p16 = a.p16 + elems;
  r.lo16 = a.lo16 ? a.lo16 + elems : nullptr;
  r.hi8 = a.hi8 ? a.hi8 + elems : nullptr;
  r.lo8 = a.lo8 ? a.lo8 + elems : nullptr;
  return r;
}
void set_out(GemmOut& o, const Act& a) { o.hi = a.p16; o.lo = a.lo16; o.hi8 = a.hi8; o.lo8 = a.lo8; o.ilv = a.ilv; }
// the same buffer pair as one split-line image (Act::ilv): the two 2-byte planes are adjacent, 4 bytes per element in all
Act make_ilv(const PlanePair& p) { Act a; a.ilv = (char*)p.hi; return a; }

GemmSeg seg_plain(const Act& a, int64_t lda, const Planes& w, int64_t wcol, int K, int M) {
  GemmSeg s = gemm_seg_plain(a.p16, a.lo16, lda, w.hi, w.lo, (int)(w.ld / 32), (int)(wcol / 32), K, M);
  s.a8 = a.hi8; s.al8 = a.lo8; s.w8 = (const uint8_t*)w.lo; s.wl8 = w.x8;
  s.w_exact16 = w.exact16 ? 1 : 0;
  s.a_ilv = a.ilv; s.w_pp = w.pp;
  s.ws16 = w.s16; s.ws8 = w.s8; s.ws_rows = (int)w.s_rows;
  return s;
}

// y = x W^T (+ LoRA: [x | u] [W | B]^T with u = (alpha / r) x A^T) with the given epilogue; ain: x [M, ld_in], au: the adapter group's u [M, 128]
int linear_with_lora(awt_encoder* e, const Act& au, const Act& ain, int64_t ld_in, const Linear& lin, const LoraGroup& lg,
                     int M, GemmEpilogue epi, GemmOut out, hipStream_t s) {
  const int terms = e->prec;
  GemmSeg segs[2];
  int nseg = 1;
  segs[0] = seg_plain(ain, ld_in, lin.w, 0, lin.K, M);
  if (lg.active) {
    GemmSeg us = seg_plain(ain, ld_in, lg.a, 0, lin.K, M);
    GemmOut uo{};
    set_out(uo, au); uo.ldo = lg.kp; uo.n_valid = lg.kp;
    uo.scale = e->cfg.lora_alpha / (float)e->cfg.lora_rank;
    int rc = launch_gemm(e->ctx, M, 128, &us, 1, terms, EPI_BF16, uo, s); if (rc) return rc;
    segs[1] = seg_plain(au, lg.kp, lg.b, 0, lg.kp, M);
    nseg = 2;
  }
  out.bias = lin.bias;
  out.n_valid = lin.N;
  return launch_gemm(e->ctx, M, lin.N, segs, nseg, terms, epi, out, s);
}

// The mirror image in the backward pass: dX [M, N] = dY W (+ the adapter term: [dY | du] [W^T | (alpha / r) A^T]), dY [M, ld] against wT = W^T [N, ld];
// du is the group's gradient as group_backward left it.  `prec`: the products of the gradient contractions.
int linear_backward_input(awt_encoder* e, const Act& dY, int64_t ld, const Planes& wT, const LoraGroup& lg, const Act& du, int N, GemmEpilogue epi, GemmOut out,
                          int M, int prec, hipStream_t s) {
  GemmSeg sg[2];
  sg[0] = seg_plain(dY, ld, wT, 0, (int)ld, M);
  if (lg.active) sg[1] = seg_plain(du, lg.kp, lg.aT, 0, lg.kp, M);
  out.ldo = N; out.n_valid = N;
  return launch_gemm(e->ctx, M, N, sg, lg.active ? 2 : 1, prec, epi, out, s);
}

// y = x W^T on the persistent ping-pong kernel: x as split lines (make_ilv), W's packed image; no adapter
int linear_pp(awt_encoder* e, const Act& in_ilv, const Linear& lin, int M, GemmEpilogue epi, GemmOut out, hipStream_t s) {
  GemmSeg sg = seg_plain(in_ilv, lin.K, lin.w, 0, lin.K, M);
  out.bias = lin.bias;
  out.n_valid = lin.N;
  return launch_gemm_pp(e->ctx, M, lin.N, sg, epi, out, s);
}
// whether this linear of an inference forward over M rows runs on the ping-pong kernel (tuning knob "gemm_pp": 0 never, 1 automatic, 2 wherever
// it can): automatic = a launch of at least one 256 x 256 tile per CU, and not the fp16-exact weights the one-cross-term GEMM (gemm.hip, WX) is faster on
bool use_pp(const awt_encoder* e, const Linear& lin, const LoraGroup& lg, int M, int epi) {
  const int mode = awt_gemm_pp_mode();
  if (mode == 0 || e->prec != PREC_F16F8 || !lin.w.pp || lg.active || !gemm_pp_supported(M, lin.N, lin.K, epi)) return false;
  if (mode == 2) return true;
  // automatic: weights that are not fp16-exact, at least one tile per CU, and a tile count that fills its rounds -- the workgroups are persistent and every
  // tile takes the same time, so t tiles on c CUs finish after ceil(t / c) tile times: more than 20 % of that idle (e.g. 282 tiles on 256 CUs: two rounds for
  // 1.1 rounds of work; measured at B = 16: GEMM class 9.83 vs 9.27 ms) loses to the 128 x 256 kernel, whose tiles the dispatcher packs as they come
  const int64_t t = (int64_t)((M + 255) / 256) * (lin.N / 256), c = gemm_pp_slots();
  return !lin.w.exact16 && c > 0 && t >= c && ((t + c - 1) / c) * c * 5 <= t * 6;
}

// Per-layer activation buffers.  Inference: every layer reuses one set (residual stream updated in place).
// Training: one set per layer, kept for awt_encoder_backward.
struct LayerBufs {
  float *x_in, *x_mid, *x_out;            // residual stream before the layer, after attention, after the MLP
  PlanePair ln1, qkv, att, ln2, pre, ff, u;
  PlanePair uo, u1, u2;                   // u = (alpha / r) x A^T of the out_proj / fc1 / fc2 adapters (inference: alias u; training: kept)
  float* lse;                             // [B, H, S] or null
};

struct TrainWs {   // carved from the caller's `saved` buffer
  std::vector<LayerBufs> layer;
  // conv-phase scratch (train_base: with conv1's pre-activation pre1 [B * T, d]; a1 and h1 then outlive the forward as well)
  ConvPlanes conv;
  PlanePair ff;                           // MLP hidden (not needed by the q/k/v-adapter backward)
  float* x_final;
  // backward scratch
  float *dx_a, *dx_b, *dln, *delta, *partial;
  PlanePair dxp, dpre, datt, dqkv, du;
  size_t partial_bytes, bytes;
};

TrainWs carve_train(const awt_encoder* e, char* base, int B) {
  const awt_encoder_cfg& c = e->cfg;
  const size_t S = c.n_ctx, T = 2 * S, d = c.d_model, f = c.ffn_dim, H = c.n_heads;
  const size_t M = (size_t)B * S, Mt = (size_t)B * T;
  TrainWs w{};
  Carver cv(base);
  auto planes = [&](size_t elems) { return take_planes(cv, elems, e->planes); };
  w.layer.resize(c.n_layers);
  float* x = cv.take<float>(M * d * 4);
  for (int li = 0; li < c.n_layers; ++li) {
    LayerBufs& L = w.layer[li];
    L.x_in = x;
    L.x_mid = cv.take<float>(M * d * 4);
    L.x_out = cv.take<float>(M * d * 4);
    x = L.x_out;
    L.ln1 = planes(M * d); L.qkv = planes(3 * M * d); L.att = planes(M * d); L.ln2 = planes(M * d); L.pre = planes(M * f);
    L.u = planes(M * 128);
    const bool has_o = e->layers[li].lo_.active, has_1 = e->layers[li].l1.active, has_2 = e->layers[li].l2.active;
    L.uo = has_o ? planes(M * 128) : L.u;
    L.u1 = has_1 ? planes(M * 128) : L.u;
    L.u2 = has_2 ? planes(M * 128) : L.u;
    if (has_2) L.ff = planes(M * f);
    if (e->train_base) L.ff = planes(M * f);   // fc2's weight gradient contracts d(x_out) with the fc2 input of this layer
    L.lse = cv.take<float>((size_t)B * H * S * 4);
  }
  w.x_final = x;
  if (!e->train_base) w.ff = planes(M * f);   // train_base: every layer keeps its own fc2 input
  // conv-phase scratch aliases the backward scratch (disjoint in time); train_base: the conv stem's backward reads it, so it is kept
  if (e->train_base) w.conv = take_conv_planes(e, cv, Mt, true);
  const size_t mark = cv.off;
  if (!e->train_base) w.conv = take_conv_planes(e, cv, Mt, false);
  const size_t conv_end = cv.off;
  cv.off = mark;
  w.dx_a = cv.take<float>(M * d * 4); w.dx_b = cv.take<float>(M * d * 4); w.dln = cv.take<float>(M * d * 4);
  w.delta = cv.take<float>((size_t)B * H * S * 4);
  w.dxp = planes(M * d); w.dpre = planes(M * f); w.datt = planes(M * d); w.dqkv = planes(3 * M * d); w.du = planes(M * 128);
  w.partial_bytes = outer_reduce_partial_bytes((int)M, c.lora_rank > 0 ? c.lora_rank : 1, 1024);   // Y blocks are reduced in chunks of <= 1024 columns
  if (e->train_base) {   // slab partials of the weight-gradient GEMMs (qkv, out_proj, fc1, fc2, a conv2 tap, a conv1 tap) and of the bias / LayerNorm reductions
    const int Mi = (int)M, Mti = (int)Mt, di = (int)d, fi = (int)f;
    size_t pb = std::max({wgrad_partial_bytes(Mi, 3 * di, di), wgrad_partial_bytes(Mi, di, di), wgrad_partial_bytes(Mi, fi, di), wgrad_partial_bytes(Mi, di, fi),
                          wgrad_partial_bytes(Mti, di, c.n_mels), param_grad_partial_bytes(Mti, di)});
    w.partial_bytes = std::max(w.partial_bytes, pb);
  }
  w.partial = cv.take<float>(w.partial_bytes);
  w.bytes = std::max(cv.off, conv_end);
  for (LayerBufs& L : w.layer) if (!L.ff.hi) L.ff = w.ff;   // kept per layer only under an fc2 adapter (or train_base)
  return w;
}

// conv stem (K5-K7): mel [Bc, n_mels, T] -> residual stream x [Bc * S, d] fp32
// Sc in (0, S), inference with known clip lengths only (awt_audio_encode): frames from 2 Sc - 4 on are one constant per clip (conv_stem_positions), so the
// stem runs on the first Tc = 2 Sc frames (same zero padding at both ends, mel row pitch still T) into g [Bc * Sc, d], and launch_expand_conv_rows spreads
// g's last two rows over positions Sc - 1 .. S - 1 while it adds the positional table.  a1 / h1 are then planes of Bc * Tc rows.  Bit-identical to the full
// stem: the same kernels run (GemmOut::m_pick: chosen as for the full row count), a row's dot products do not depend on the tile it lands in, conv2's
// epilogue adds a zero row (rows_pos = 1) where the full stem adds pos -- gelu + 0 is gelu -- and the expand kernel makes that same fp32 add afterwards.
// cp: the conv planes carved for those rows (take_conv_planes); with cp.pre1 (train_base) conv1's pre-activation is kept there.
int conv_stem(awt_encoder* e, const float* mel, int Bc, const ConvPlanes& cp, float* x, hipStream_t s, int Sc = 0, float* g = nullptr) {
  const awt_encoder_cfg& c = e->cfg;
  const int S = c.n_ctx, T = 2 * S, d = c.d_model, terms = e->prec;
  const bool keep_pre1 = cp.pre1.hi != nullptr;
  const bool compact = Sc > 0 && Sc < S && g && !keep_pre1;
  const int So = compact ? Sc : S, To = 2 * So;       // positions and frames computed per clip
  const int M = Bc * So, Mt = Bc * To;
  const int k1 = conv1_k(c.n_mels);
  const Act aa1 = make_act(cp.a1, (size_t)Mt * k1, terms), ah1 = make_act(cp.h1, (size_t)Mt * d, terms);
  int rc = launch_im2col_conv1(e->ctx, mel, Bc, c.n_mels, T, To, k1, aa1, terms, s); if (rc) return rc;
  {
    GemmSeg sg = seg_plain(aa1, k1, e->conv1.w, 0, k1, Mt);
    GemmOut o{}; set_out(o, ah1); o.ldo = d; o.bias = e->conv1.bias; o.n_valid = d; o.m_pick = Bc * T;
    if (keep_pre1) { o.hi2 = cp.pre1.hi; o.lo2 = cp.pre1.lo; }   // train_base: kept for its GELU' in the backward pass
    rc = launch_gemm(e->ctx, Mt, d, &sg, 1, terms, keep_pre1 ? EPI_BF16_GELU_SAVE : EPI_BF16_GELU, o, s); if (rc) return rc;
  }
  GemmSeg sg[3];
  for (int dt = 0; dt < 3; ++dt) {
    sg[dt] = seg_plain(ah1, d, e->conv2.w, (int64_t)dt * d, d, M);
    sg[dt].rows_out = So; sg[dt].rows_in = To; sg[dt].row_mul = 2; sg[dt].row_add = dt - 1;
  }
  GemmOut o{}; o.f32 = compact ? g : x; o.ldo = d; o.bias = e->conv2.bias; o.n_valid = d; o.m_pick = Bc * S;
  if (compact) { o.pos = e->zero_row; o.rows_pos = 1; } else { o.pos = e->pos; o.rows_pos = S; }
  rc = launch_gemm(e->ctx, M, d, sg, 3, terms, EPI_F32_GELU_POS, o, s); if (rc || !compact) return rc;
  return launch_expand_conv_rows(e->ctx, g, e->pos, Bc, S, Sc, d, x, s);
}

// one transformer layer (K8-K13) on the given buffers; `save` also keeps the MLP pre-activation and the softmax statistics
int encoder_layer(awt_encoder* e, Layer& L, const LayerBufs& b, int Bc, bool save, hipStream_t s) {
  const awt_encoder_cfg& c = e->cfg;
  const int S = c.n_ctx, d = c.d_model, f = c.ffn_dim, H = c.n_heads, terms = e->prec;
  const int M = Bc * S;
  const int64_t plane = (int64_t)M * d;
  // which of the four linears run on the persistent ping-pong kernel (inference only): their inputs are then written as split lines by the
  // producer (LayerNorm, the attention epilogue, fc1's GELU epilogue) instead of as three planes -- same bytes, same buffers
  const bool pp_qkv = !save && (g_pp_mask & 1) && use_pp(e, L.qkv, L.lq, M, EPI_QKV), pp_out = !save && (g_pp_mask & 2) && use_pp(e, L.out, L.lo_, M, EPI_F32_RESID);
  const bool pp_fc1 = !save && (g_pp_mask & 4) && use_pp(e, L.fc1, L.l1, M, EPI_BF16_GELU), pp_fc2 = pp_fc1 && (g_pp_mask & 8) && use_pp(e, L.fc2, L.l2, M, EPI_F32_RESID);
  // an activation whose only consumer is a GEMM on fp16-exact weights (gemm.hip, WX) needs no hi8 image: the producers skip that plane
  auto feeds = [&](Act a, const Linear& lin, const LoraGroup& lg) { if (terms == PREC_F16F8 && lin.w.exact16 && !lg.active) a.hi8 = nullptr; return a; };
  // The layer's buffers as operand planes, each viewed once: ln1, att, ln2, ff as the GEMM that consumes them reads them, and `*_w` as their producer
  // writes them (split lines for a ping-pong consumer, else the same planes without the image no consumer reads).  backward_terms = 5 runs the MLP
  // of the training step in the f16f8 operand format (no fc1 / fc2 adapters in this mode), so its two inputs are f16f8 planes whatever the forward's are.
  const bool mlp8 = save && e->mlp_f8;
  const int mprec = mlp8 ? PREC_F16F8 : terms;
  const Act qkv = make_act(b.qkv, 3 * (size_t)plane, terms), u = make_act(b.u, (size_t)M * 128, terms), uo = make_act(b.uo, (size_t)M * 128, terms);
  const Act u1 = make_act(b.u1, (size_t)M * 128, terms), u2 = make_act(b.u2, (size_t)M * 128, terms);
  const Act ln1 = make_act(b.ln1, (size_t)plane, terms), ln1_w = pp_qkv ? make_ilv(b.ln1) : feeds(ln1, L.qkv, L.lq);
  const Act att = make_act(b.att, (size_t)plane, terms), att_w = pp_out ? make_ilv(b.att) : feeds(att, L.out, L.lo_);
  const Act ln2 = make_act(b.ln2, (size_t)plane, mprec), ln2_w = pp_fc1 ? make_ilv(b.ln2) : feeds(ln2, L.fc1, L.l1);
  const Act ff = make_act(b.ff, (size_t)M * f, mprec), ff_w = pp_fc2 ? make_ilv(b.ff) : feeds(ff, L.fc2, L.l2);
  int rc = launch_layernorm(e->ctx, b.x_in, L.ln1_g, L.ln1_b, M, d, 1e-5f, nullptr, ln1_w, terms, s); if (rc) return rc;
  {
    GemmOut o{}; set_out(o, qkv); o.scale = 0.125f * 1.4426950408889634f;   // head_dim^-1/2 and log2(e): see attention.hip
    o.S = S; o.H = H; o.plane_stride = plane;
    o.skip_v8 = terms == PREC_F16F8 && !attention_f16f8_reads_v8(save);
    rc = pp_qkv ? linear_pp(e, ln1_w, L.qkv, M, EPI_QKV, o, s) : linear_with_lora(e, u, ln1, d, L.qkv, L.lq, M, EPI_QKV, o, s);
    if (rc) return rc;
  }
  float* const lse = save ? b.lse : nullptr;
  rc = terms == PREC_F16F8 ? launch_attention_f16f8(e->ctx, qkv, act_offset(qkv, plane), act_offset(qkv, 2 * plane), att_w, nullptr, lse, Bc, H, S, s)
                           : launch_attention(e->ctx, b.qkv, b.qkv.at(plane), b.qkv.at(2 * plane), b.att, nullptr, lse, Bc, H, S, terms, s);
  if (rc) return rc;
  {
    GemmOut o{}; o.f32 = b.x_mid; o.resid = b.x_in; o.ldo = d;
    rc = pp_out ? linear_pp(e, att_w, L.out, M, EPI_F32_RESID, o, s) : linear_with_lora(e, uo, att, d, L.out, L.lo_, M, EPI_F32_RESID, o, s);
    if (rc) return rc;
  }
  rc = launch_layernorm(e->ctx, b.x_mid, L.ln2_g, L.ln2_b, M, d, 1e-5f, nullptr, ln2_w, mprec, s); if (rc) return rc;
  if (mlp8) {
    GemmSeg s1 = seg_plain(ln2, d, L.fc1_8, 0, d, M);
    GemmOut o1{}; set_out(o1, ff); o1.ldo = f; o1.n_valid = f; o1.bias = L.fc1.bias; o1.hi2 = b.pre.hi; o1.lo2 = b.pre.lo; o1.scale = 1.0f;
    rc = launch_gemm(e->ctx, M, f, &s1, 1, PREC_F16F8, EPI_BF16_GELU_SAVE, o1, s); if (rc) return rc;
    GemmSeg s2 = seg_plain(ff, f, L.fc2_8, 0, f, M);
    GemmOut o2{}; o2.f32 = b.x_out; o2.resid = b.x_mid; o2.ldo = d; o2.n_valid = d; o2.bias = L.fc2.bias;
    return launch_gemm(e->ctx, M, d, &s2, 1, PREC_F16F8, EPI_F32_RESID, o2, s);
  }
  {
    GemmOut o{}; set_out(o, ff_w); o.ldo = f; o.hi2 = b.pre.hi; o.lo2 = b.pre.lo;
    rc = pp_fc1 ? linear_pp(e, ln2_w, L.fc1, M, EPI_BF16_GELU, o, s)
                : linear_with_lora(e, u1, ln2, d, L.fc1, L.l1, M, save ? EPI_BF16_GELU_SAVE : EPI_BF16_GELU, o, s);
    if (rc) return rc;
  }
  GemmOut o{}; o.f32 = b.x_out; o.resid = b.x_mid; o.ldo = d;
  return pp_fc2 ? linear_pp(e, ff_w, L.fc2, M, EPI_F32_RESID, o, s) : linear_with_lora(e, u2, ff, f, L.fc2, L.l2, M, EPI_F32_RESID, o, s);
}

// Sc: positions per clip the conv stem has to compute (conv_stem_positions; 0 or >= n_ctx: all of them)
int forward_chunk(awt_encoder* e, const float* mel, int Bc, float* hidden, char* ws_base, hipStream_t s, int Sc = 0) {
  const awt_encoder_cfg& c = e->cfg;
  const int M = Bc * c.n_ctx, d = c.d_model;
  Workspace w = carve(e, ws_base, Bc);
  ConvPlanes cp = w.conv;
  float* g = nullptr;
  if (Sc > 0 && Sc < c.n_ctx) {
    // the compact stem's planes (Bc * 2 Sc rows) and its output g [Bc * Sc, d] share the region the full-length conv planes and the layer buffers
    // alias; a shape whose region has no room for g beside the shorter planes (none of Whisper's) keeps the full stem
    char* const base = (char*)w.conv.a1.hi;
    const size_t room = (size_t)(ws_base + w.bytes - base);
    Carver cv(base);
    const ConvPlanes ccp = take_conv_planes(e, cv, (size_t)Bc * 2 * Sc, false);
    float* cg = cv.take<float>((size_t)Bc * Sc * d * 4);
    if (cv.bytes() <= room) { g = cg; cp = ccp; }
  }
  int rc = conv_stem(e, mel, Bc, cp, w.x, s, g ? Sc : 0, g); if (rc) return rc;
  LayerBufs b{};
  b.x_in = b.x_mid = b.x_out = w.x;
  b.ln1 = b.ln2 = w.ln; b.qkv = w.qkv; b.att = w.att; b.ff = w.ff; b.u = b.uo = b.u1 = b.u2 = w.u;   // one set, reused by every layer; no pre-activation kept
  for (int li = 0; li < c.n_layers; ++li) { rc = encoder_layer(e, e->layers[li], b, Bc, false, s); if (rc) return rc; }
  return launch_layernorm(e->ctx, w.x, e->lnf_g, e->lnf_b, M, d, 1e-5f, hidden, Act{}, e->prec, s);
}

bool parse_layer(const char* name, int* idx, const char** rest) {
  if (strncmp(name, "layers.", 7) != 0) return false;
  char* end = nullptr;
  long v = strtol(name + 7, &end, 10);
  if (end == name + 7 || *end != '.') return false;
  *idx = (int)v; *rest = end + 1;
  return true;
}

int check_shape(const char* name, const int64_t* shape, int rank, std::initializer_list<int64_t> want) {
  bool ok = rank == (int)want.size();
  int i = 0;
  for (int64_t w : want) { if (ok && shape[i] != w) ok = false; ++i; }
  if (!ok) {
    std::string m = std::string("set_weight: ") + name + " has shape [";
    for (int j = 0; j < rank; ++j) m += (j ? "," : "") + std::to_string(shape[j]);
    m += "], expected [";
    i = 0;
    for (int64_t w : want) m += (i++ ? "," : "") + std::to_string(w);
    return awt_fail(AWT_ERR_INVALID, m + "]");
  }
  return AWT_OK;
}

int copy_f32(float* dst, const float* src, size_t n, hipStream_t s) {
  AWT_HIP_CHECK(hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToDevice, s));
  return AWT_OK;
}

}  // namespace

namespace {
// The flat gradient buffer of cfg.train_base: head = the non-layer parameters, then one contiguous block per layer (the in-backward exchange
// reduces whole layer groups; the head goes with the lowest group, which is reduced last).  q | k | v weights are adjacent: one [3 d, d] product.
void build_grad_layout(awt_encoder* e) {
  const awt_encoder_cfg& c = e->cfg;
  const int64_t d = c.d_model, f = c.ffn_dim;
  size_t off = 0, block = 0;
  auto add = [&](const std::string& name, std::initializer_list<int64_t> shape) {   // returns the entry's offset from `block`
    awt_encoder::GradEntry g{name, off, {1, 1, 1}, (int)shape.size()};
    int i = 0; size_t n = 1;
    for (int64_t v : shape) { g.shape[i++] = v; n *= (size_t)v; }
    e->glayout.push_back(g);
    off += n;
    return g.offset - block;
  };
  awt_encoder::GradOffsets& o = e->goff;
  o.c1w = add("conv1.weight", {d, c.n_mels, 3}); o.c1b = add("conv1.bias", {d}); o.c2w = add("conv2.weight", {d, d, 3}); o.c2b = add("conv2.bias", {d});
  o.lnf = add("layer_norm.weight", {d}); add("layer_norm.bias", {d});
  e->g_head = off;
  for (int li = 0; li < c.n_layers; ++li) {   // every block has the same layout: each layer writes the same offsets
    const std::string p = "layers." + std::to_string(li) + ".";
    block = off;
    o.qkvw = add(p + "self_attn.q_proj.weight", {d, d}); add(p + "self_attn.k_proj.weight", {d, d}); add(p + "self_attn.v_proj.weight", {d, d});
    o.qb = add(p + "self_attn.q_proj.bias", {d}); o.vb = add(p + "self_attn.v_proj.bias", {d});
    o.ow = add(p + "self_attn.out_proj.weight", {d, d}); o.ob = add(p + "self_attn.out_proj.bias", {d});
    o.ln1 = add(p + "self_attn_layer_norm.weight", {d}); add(p + "self_attn_layer_norm.bias", {d});
    o.f1w = add(p + "fc1.weight", {f, d}); o.f1b = add(p + "fc1.bias", {f}); o.f2w = add(p + "fc2.weight", {d, f}); o.f2b = add(p + "fc2.bias", {d});
    o.ln2 = add(p + "final_layer_norm.weight", {d}); add(p + "final_layer_norm.bias", {d});
    e->g_per_layer = off - block;
  }
}
}  // namespace

extern "C" size_t awt_encoder_base_grad_count(const awt_encoder* e) {
  if (!e || !e->train_base) return 0;
  return e->g_head + (size_t)e->cfg.n_layers * e->g_per_layer;
}
extern "C" int awt_encoder_base_grad_params(const awt_encoder* e) { return (e && e->train_base) ? (int)e->glayout.size() : 0; }
extern "C" int awt_encoder_base_grad_param(const awt_encoder* e, int index, const char** name, size_t* offset, int64_t* shape, int* rank) {
  AWT_REQUIRE(e && e->train_base, AWT_ERR_STATE, "encoder_base_grad_param: encoder was not created with cfg.train_base");
  AWT_REQUIRE(index >= 0 && index < (int)e->glayout.size() && name && offset && shape && rank, AWT_ERR_INVALID, "encoder_base_grad_param: bad argument");
  const awt_encoder::GradEntry& g = e->glayout[index];
  *name = g.name.c_str(); *offset = g.offset; *rank = g.rank;
  for (int i = 0; i < 3; ++i) shape[i] = g.shape[i];
  return AWT_OK;
}

extern "C" int awt_encoder_create(awt_ctx* c, const awt_encoder_cfg* cfg, awt_encoder** out) {
  AWT_REQUIRE(c && cfg && out, AWT_ERR_INVALID, "encoder_create: null argument");
  AWT_REQUIRE(cfg->d_model > 0 && cfg->d_model % 128 == 0 && cfg->d_model <= 1280, AWT_ERR_INVALID, "encoder_create: d_model must be a multiple of 128, <= 1280");
  AWT_REQUIRE(cfg->n_heads > 0 && cfg->d_model == cfg->n_heads * 64, AWT_ERR_INVALID, "encoder_create: head_dim (d_model / n_heads) must be 64");
  AWT_REQUIRE(cfg->ffn_dim > 0 && cfg->ffn_dim % 128 == 0, AWT_ERR_INVALID, "encoder_create: ffn_dim must be a multiple of 128");
  AWT_REQUIRE(cfg->n_mels > 0 && cfg->n_mels % 8 == 0 && cfg->n_mels <= 128, AWT_ERR_INVALID, "encoder_create: n_mels must be a multiple of 8, <= 128");
  AWT_REQUIRE(cfg->n_layers > 0 && cfg->n_ctx > 0, AWT_ERR_INVALID, "encoder_create: n_layers and n_ctx must be positive");
  AWT_REQUIRE(prec_known(cfg->mfma_terms), AWT_ERR_INVALID,
              "encoder_create: mfma_terms must be 1 (bf16), 2 (fp16), 3 (bf16x3), 4 (fp16x3) or 5 (f16f8)");
  AWT_REQUIRE(!cfg->training || cfg->mfma_terms == PREC_BF16 || cfg->mfma_terms == PREC_BF16X3, AWT_ERR_INVALID,
              "encoder_create: training keeps its activations as bf16 planes: mfma_terms must be 1 or 3 (gradients do not fit fp16's range unscaled)");
  AWT_REQUIRE(cfg->backward_terms == 0 || cfg->backward_terms == cfg->mfma_terms || ((cfg->backward_terms == 1 || cfg->backward_terms == PREC_F16F8) && cfg->mfma_terms == 3),
              AWT_ERR_INVALID, "encoder_create: backward_terms must be 0 (= mfma_terms), mfma_terms, 1, or 5 (f16f8 MLP backward) with mfma_terms = 3");
  AWT_REQUIRE(cfg->backward_terms != PREC_F16F8 || (cfg->training && !(cfg->lora_targets & (AWT_LORA_FC1 | AWT_LORA_FC2))), AWT_ERR_INVALID,
              "encoder_create: backward_terms = 5 runs the MLP's backward GEMMs in f16f8: training mode, and no adapters on fc1 / fc2");
  AWT_REQUIRE(cfg->lora_rank >= 0 && cfg->lora_rank <= 32, AWT_ERR_INVALID, "encoder_create: lora_rank must be in 0..32");
  AWT_REQUIRE(cfg->lora_rank == 0 || cfg->lora_targets != 0, AWT_ERR_INVALID, "encoder_create: lora_rank > 0 needs lora_targets");
  AWT_REQUIRE(!cfg->training || cfg->lora_rank > 0 || cfg->train_base, AWT_ERR_INVALID, "encoder_create: training mode needs adapters (lora_rank > 0) or train_base");
  AWT_REQUIRE(!cfg->train_base || cfg->training, AWT_ERR_INVALID, "encoder_create: train_base needs training mode");
  AWT_REQUIRE(!cfg->train_base || cfg->lora_rank == 0, AWT_ERR_INVALID, "encoder_create: train_base trains the base weights themselves: no adapters in this mode (lora_rank must be 0)");
  AWT_REQUIRE(!cfg->train_base || cfg->backward_terms != PREC_F16F8, AWT_ERR_INVALID,
              "encoder_create: train_base forms its weight gradients from bf16 planes: backward_terms = 5 (f16f8 MLP backward) is not available in this mode");
  awt_encoder* e = new awt_encoder();
  e->ctx = c; e->cfg = *cfg; e->prec = cfg->mfma_terms; e->planes = (cfg->mfma_terms == PREC_BF16 || cfg->mfma_terms == PREC_F16) ? 1 : 2;
  e->chunk = cfg->chunk_clips > 0 ? cfg->chunk_clips : 64;
  e->mlp_f8 = cfg->backward_terms == PREC_F16F8;
  e->train_base = cfg->train_base != 0;
  const int d = cfg->d_model, f = cfg->ffn_dim;
  int rc = alloc_linear(e, &e->conv1, d, conv1_k(cfg->n_mels));
  if (!rc && e->mlp_f8) rc = dev_alloc(e, (void**)&e->wt_tmp, (size_t)f * d * 4);
  if (!rc && e->train_base) rc = dev_alloc(e, (void**)&e->wt_tmp, (size_t)d * d * 4);
  for (int dt = 0; dt < 3 && !rc && e->train_base; ++dt) rc = alloc_planes(e, &e->conv2T[dt], d, d, e->prec);
  if (!rc) rc = alloc_linear(e, &e->conv2, d, 3 * d);
  if (!rc) rc = dev_alloc(e, (void**)&e->pos, (size_t)cfg->n_ctx * d * 4);
  if (!rc) rc = dev_alloc(e, (void**)&e->zero_row, (size_t)d * 4);
  if (!rc) rc = dev_alloc(e, (void**)&e->lnf_g, (size_t)d * 4);
  if (!rc) rc = dev_alloc(e, (void**)&e->lnf_b, (size_t)d * 4);
  e->layers.resize(cfg->n_layers);
  const bool lora = cfg->lora_rank > 0;
  for (int i = 0; i < cfg->n_layers && !rc; ++i) {
    Layer& L = e->layers[i];
    rc = alloc_linear(e, &L.qkv, 3 * d, d);
    if (!rc) rc = alloc_linear(e, &L.out, d, d);
    if (!rc) rc = alloc_linear(e, &L.fc1, f, d);
    if (!rc) rc = alloc_linear(e, &L.fc2, d, f);
    if ((e->prec == PREC_F16F8 || e->prec == PREC_F16X3) && !cfg->training)   // four zero-initialised "not fp16-exact" flags per projection matrix (set_weight)
      for (Linear* lin : {&L.qkv, &L.out, &L.fc1, &L.fc2}) if (!rc) rc = dev_alloc(e, (void**)&lin->w.d_inexact, 4 * sizeof(int));
    if (e->prec == PREC_F16F8 && !cfg->training)     // the packed images of the ping-pong GEMM (a second copy of each weight: 4 bytes per element)
      for (Linear* lin : {&L.qkv, &L.out, &L.fc1, &L.fc2})
        if (!rc && lin->N % 256 == 0 && lin->K % 64 == 0 && lin->K >= 128) rc = dev_alloc(e, (void**)&lin->w.pp, gemm_pp_weight_bytes(lin->N, lin->K));
    if (cfg->training) {
      if (!rc) rc = alloc_planes(e, &L.qkvT, d, 3 * d, e->prec);
      if (!rc) rc = alloc_planes(e, &L.outT, d, d, e->prec);
      if (!rc) rc = alloc_planes(e, &L.fc1T, d, f, e->prec);
      if (!rc) rc = alloc_planes(e, &L.fc2T, f, d, e->prec);
      if (!rc && e->mlp_f8) rc = alloc_planes(e, &L.fc1T8, d, f, PREC_F16F8);
      if (!rc && e->mlp_f8) rc = alloc_planes(e, &L.fc2T8, f, d, PREC_F16F8);
      if (!rc && e->mlp_f8) rc = alloc_planes(e, &L.fc1_8, f, d, PREC_F16F8);
      if (!rc && e->mlp_f8) rc = alloc_planes(e, &L.fc2_8, d, f, PREC_F16F8);
    }
    float** lnp[4] = {&L.ln1_g, &L.ln1_b, &L.ln2_g, &L.ln2_b};
    for (int k = 0; k < 4 && !rc; ++k) rc = dev_alloc(e, (void**)lnp[k], (size_t)d * 4);
    if (lora && !rc && (cfg->lora_targets & (AWT_LORA_Q | AWT_LORA_K | AWT_LORA_V))) rc = alloc_lora(e, &L.lq, 3, d, 3 * d);
    if (lora && !rc && (cfg->lora_targets & AWT_LORA_OUT)) rc = alloc_lora(e, &L.lo_, 1, d, d);
    if (lora && !rc && (cfg->lora_targets & AWT_LORA_FC1)) rc = alloc_lora(e, &L.l1, 1, d, f);
    if (lora && !rc && (cfg->lora_targets & AWT_LORA_FC2)) rc = alloc_lora(e, &L.l2, 1, f, d);
  }
  if (rc) { awt_encoder_destroy(e); return rc; }
  if (e->train_base) build_grad_layout(e);
  *out = e;
  return AWT_OK;
}

extern "C" void awt_encoder_destroy(awt_encoder* e) {
  if (!e) return;
  for (void* p : e->allocs) (void)hipFree(p);
  delete e;
}

extern "C" int awt_encoder_set_weight(awt_encoder* e, const char* name, const float* data, const int64_t* shape, int rank,
                                      void* stream) {
  AWT_REQUIRE(e && name && data && shape && rank >= 1 && rank <= 3, AWT_ERR_INVALID, "set_weight: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const awt_encoder_cfg& c = e->cfg;
  const int d = c.d_model, f = c.ffn_dim, r = c.lora_rank;
  int rc = AWT_ERR_INVALID;
  // dst(row_off + c, col_off + n) = scale * src[n, c]: the transposed copies the backward pass multiplies by
  auto pack_t = [&](const float* src, const Planes& pl, int N, int C, int row_off, int col_off, float scale) {
    return launch_pack_weight_t(e->ctx, src, N, C, pl.ld, row_off, col_off, scale, PlanePair{pl.hi, pl.lo}, s);
  };
  std::string nm(name);
  if (nm == "conv1.weight") { rc = check_shape(name, shape, rank, {d, c.n_mels, 3}); if (!rc) rc = pack(e->ctx, data, e->conv1.w, d, c.n_mels, 3, 0, 0, e->prec, s); }
  else if (nm == "conv1.bias") { rc = check_shape(name, shape, rank, {d}); if (!rc) rc = copy_f32(e->conv1.bias, data, d, s); }
  else if (nm == "conv2.weight") {
    rc = check_shape(name, shape, rank, {d, d, 3}); if (!rc) rc = pack(e->ctx, data, e->conv2.w, d, d, 3, 0, 0, e->prec, s);
    for (int dt = 0; dt < 3 && !rc && e->train_base; ++dt) {   // per tap: W[:, :, dt]^T, the weight of d h1 = d pre2 W2
      rc = launch_conv_tap(e->ctx, data, d, d, dt, e->wt_tmp, s);
      if (!rc) rc = pack_t(e->wt_tmp, e->conv2T[dt], d, d, 0, 0, 1.0f);
    }
  }
  else if (nm == "conv2.bias") { rc = check_shape(name, shape, rank, {d}); if (!rc) rc = copy_f32(e->conv2.bias, data, d, s); }
  else if (nm == "embed_positions.weight") { rc = check_shape(name, shape, rank, {c.n_ctx, d}); if (!rc) rc = copy_f32(e->pos, data, (size_t)c.n_ctx * d, s); }
  else if (nm == "layer_norm.weight") { rc = check_shape(name, shape, rank, {d}); if (!rc) rc = copy_f32(e->lnf_g, data, d, s); }
  else if (nm == "layer_norm.bias") { rc = check_shape(name, shape, rank, {d}); if (!rc) rc = copy_f32(e->lnf_b, data, d, s); }
  else {
    int li = -1; const char* rest = nullptr;
    if (!parse_layer(name, &li, &rest) || li < 0 || li >= c.n_layers)
      return awt_fail(AWT_ERR_INVALID, std::string("set_weight: unknown parameter ") + name);
    Layer& L = e->layers[li];
    std::string rs(rest);
    struct Proj { const char* key; Linear* lin; int row_off; int N; int K; LoraGroup* lg; int slot; uint32_t bit; Planes* wT; Planes* wT8; Planes* w8; };
    Proj projs[] = {
        {"self_attn.q_proj", &L.qkv, 0, d, d, &L.lq, 0, AWT_LORA_Q, &L.qkvT, nullptr, nullptr},   {"self_attn.k_proj", &L.qkv, d, d, d, &L.lq, 1, AWT_LORA_K, &L.qkvT, nullptr, nullptr},
        {"self_attn.v_proj", &L.qkv, 2 * d, d, d, &L.lq, 2, AWT_LORA_V, &L.qkvT, nullptr, nullptr}, {"self_attn.out_proj", &L.out, 0, d, d, &L.lo_, 0, AWT_LORA_OUT, &L.outT, nullptr, nullptr},
        {"fc1", &L.fc1, 0, f, d, &L.l1, 0, AWT_LORA_FC1, &L.fc1T, &L.fc1T8, &L.fc1_8},            {"fc2", &L.fc2, 0, d, f, &L.l2, 0, AWT_LORA_FC2, &L.fc2T, &L.fc2T8, &L.fc2_8}};
    const float lscale = r > 0 ? c.lora_alpha / (float)r : 0.f;
    bool found = false;
    for (const Proj& p : projs) {
      const std::string key(p.key);
      if (rs == key + ".weight") {
        found = true; rc = check_shape(name, shape, rank, {p.N, p.K});
        if (!rc && (e->prec == PREC_F16F8 || e->prec == PREC_F16X3) && !c.training && p.lin->w.d_inexact)   // one flag per row block q | k | v: find out now, at upload time
          rc = probe_exact16(e->ctx, "set_weight", data, p.lin->w, p.N, p.K, p.row_off, e->prec, p.lin->w.d_inexact, p.row_off / p.N, 4, s);
        else if (!rc) rc = pack(e->ctx, data, p.lin->w, p.N, p.K, 1, p.row_off, 0, e->prec, s);
        if (!rc && p.lin->w.pp) rc = launch_pack_weight_pp(e->ctx, data, p.N, p.K, p.row_off, p.lin->w.pp, s);
        if (!rc && c.training) rc = pack_t(data, *p.wT, p.N, p.K, 0, p.row_off, 1.0f);   // W^T: [K, N_total], this projection's columns start at row_off
        if (!rc && e->mlp_f8 && p.wT8) {   // the same W^T [K, N] in the f16f8 weight format: transposed into the scratch matrix, then packed like a forward weight
          rc = launch_transpose_f32(e->ctx, data, p.N, p.K, e->wt_tmp, s);
          if (!rc) rc = pack(e->ctx, e->wt_tmp, *p.wT8, p.K, p.N, 1, 0, 0, PREC_F16F8, s);
          if (!rc) rc = pack(e->ctx, data, *p.w8, p.N, p.K, 1, 0, 0, PREC_F16F8, s);
        }
      }
      else if (rs == key + ".bias") {
        found = true;
        if (key == "self_attn.k_proj") return awt_fail(AWT_ERR_INVALID, "set_weight: k_proj has no bias (HF:modeling_whisper.py:279)");
        rc = check_shape(name, shape, rank, {p.N}); if (!rc) rc = copy_f32(p.lin->bias + p.row_off, data, p.N, s);
      } else if (rs == key + ".lora_A" || rs == key + ".lora_B") {
        found = true;
        if (r == 0 || !(c.lora_targets & p.bit) || !p.lg->active)
          return awt_fail(AWT_ERR_STATE, std::string("set_weight: ") + name + " given but this adapter is not enabled in awt_encoder_cfg");
        if (rs.back() == 'A') {
          rc = check_shape(name, shape, rank, {r, p.K}); if (!rc) rc = pack(e->ctx, data, p.lg->a, r, p.K, 1, p.slot * r, 0, e->prec, s);
          if (!rc && c.training) rc = pack_t(data, p.lg->aT, r, p.K, 0, p.slot * r, lscale);
        } else {
          rc = check_shape(name, shape, rank, {p.N, r}); if (!rc) rc = pack(e->ctx, data, p.lg->b, p.N, r, 1, p.row_off, p.slot * r, e->prec, s);
          if (!rc && c.training) rc = pack_t(data, p.lg->bT, p.N, r, p.slot * r, p.row_off, 1.0f);
        }
      }
      if (found) break;
    }
    if (!found) {
      struct Vec { const char* key; float* dst; };
      Vec vecs[] = {{"self_attn_layer_norm.weight", L.ln1_g}, {"self_attn_layer_norm.bias", L.ln1_b},
                    {"final_layer_norm.weight", L.ln2_g}, {"final_layer_norm.bias", L.ln2_b}};
      for (const Vec& v : vecs)
        if (rs == v.key) { found = true; rc = check_shape(name, shape, rank, {d}); if (!rc) rc = copy_f32(v.dst, data, d, s); break; }
    }
    if (!found) return awt_fail(AWT_ERR_INVALID, std::string("set_weight: unknown parameter ") + name);
  }
  if (rc == AWT_OK && std::find(e->seen.begin(), e->seen.end(), nm) == e->seen.end()) e->seen.push_back(nm);
  return rc;
}

static int require_weights(const awt_encoder* e) {
  // 5 stem/table entries + 2 final LN + 15 per layer (k_proj has no bias) must have been uploaded; adapters are optional
  size_t base = 0;
  for (const std::string& n : e->seen) if (n.find("lora_") == std::string::npos) ++base;
  const size_t want = 7 + 15 * (size_t)e->cfg.n_layers;
  if (base < want)
    return awt_fail(AWT_ERR_STATE, "encoder: " + std::to_string(base) + " of " + std::to_string(want) + " parameters uploaded; call awt_encoder_set_weight for every state-dict key first");
  return AWT_OK;
}

extern "C" int awt_encoder_exact16_matrices(const awt_encoder* e, int* n_exact, int* n_total) {
  AWT_REQUIRE(e && n_exact && n_total, AWT_ERR_INVALID, "encoder_exact16_matrices: null argument");
  int ex = 0, tot = 0;
  for (const Layer& L : e->layers)
    for (const Linear* lin : {&L.qkv, &L.out, &L.fc1, &L.fc2}) { ++tot; if (lin->w.exact16) ++ex; }
  *n_exact = ex; *n_total = tot;
  return AWT_OK;
}

extern "C" size_t awt_encoder_workspace_bytes(const awt_encoder* e, int B) {
  if (!e || B <= 0) return 0;
  return carve(e, nullptr, std::min(B, e->chunk)).bytes;
}

extern "C" int awt_encoder_forward(awt_encoder* e, const float* mel, int B, int n_frames, float* hidden, void* workspace,
                                   size_t ws_bytes, void* stream) {
  AWT_REQUIRE(e && mel && hidden && workspace && B > 0, AWT_ERR_INVALID, "encoder_forward: bad argument");
  const int T = 2 * e->cfg.n_ctx;
  if (n_frames != T)  // HF:modeling_whisper.py:612-616
    return awt_fail(AWT_ERR_VALUE, "Whisper expects the mel input features to be of length " + std::to_string(T) + ", but found " +
                                       std::to_string(n_frames) + ". Make sure to pad the input mel features to " + std::to_string(T) + ".");
  int rc = require_weights(e); if (rc) return rc;
  AWT_REQUIRE(ws_bytes >= awt_encoder_workspace_bytes(e, B), AWT_ERR_WORKSPACE, "encoder_forward: workspace too small");
  AWT_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)mel & 15) == 0 && ((uintptr_t)hidden & 15) == 0, AWT_ERR_INVALID,
              "encoder_forward: workspace must be 256-byte aligned, tensors 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  for (int b0 = 0; b0 < B; b0 += e->chunk) {
    const int Bc = std::min(e->chunk, B - b0);
    rc = forward_chunk(e, mel + (size_t)b0 * e->cfg.n_mels * T, Bc, hidden + (size_t)b0 * e->cfg.n_ctx * e->cfg.d_model,
                       (char*)workspace, s);
    if (rc) return rc;
  }
  return AWT_OK;
}

namespace {
// awt_audio_encode's workspace for chunks of Bc clips: the encoder's own (carve), one chunk's mel features, the log-mel workspace
struct AudioEncodeWs { char* enc; float* mel; void* logmel; size_t bytes; };
AudioEncodeWs audio_encode_layout(const awt_encoder* e, void* base, int Bc) {
  Carver cv(base);
  return {cv.take(carve(e, nullptr, Bc).bytes), cv.take<float>((size_t)Bc * e->cfg.n_mels * 2 * e->cfg.n_ctx * 4), cv.take(awt_logmel_workspace_bytes(Bc)), cv.bytes()};
}
}  // namespace
extern "C" size_t awt_audio_encode_workspace_bytes(const awt_encoder* e, int B) {
  if (!e || B <= 0) return 0;
  return audio_encode_layout(e, nullptr, std::min(B, e->chunk)).bytes;
}

extern "C" int awt_audio_encode(awt_encoder* e, const void* pcm, int pcm_is_i16, int64_t pcm_stride, const int32_t* n_valid,
                                int max_valid, int B, float* features_out, float* hidden, void* workspace, size_t ws_bytes,
                                void* stream) {
  AWT_REQUIRE(e && pcm && hidden && workspace && B > 0, AWT_ERR_INVALID, "audio_encode: bad argument");
  AWT_REQUIRE(e->cfg.n_mels == 80 || e->cfg.n_mels == 128, AWT_ERR_INVALID, "audio_encode: the Whisper front-end has 80 or 128 (large-v3) mel bins");
  int rc = require_weights(e); if (rc) return rc;
  AWT_REQUIRE(ws_bytes >= awt_audio_encode_workspace_bytes(e, B), AWT_ERR_WORKSPACE, "audio_encode: workspace too small");
  AWT_REQUIRE(((uintptr_t)workspace & 255) == 0, AWT_ERR_INVALID, "audio_encode: workspace must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int T = 2 * e->cfg.n_ctx;
  const int chunk = std::min(B, e->chunk);
  // log-mel pads every clip with one constant from its last live frame on; the conv stem computes the positions that see live frames (plus two) and copies the rest
  const int Sc = g_conv_live ? conv_stem_positions(e->cfg.n_ctx, max_valid) : 0;
  const AudioEncodeWs w = audio_encode_layout(e, workspace, chunk);
  const size_t esz = pcm_is_i16 ? 2 : 4;
  for (int b0 = 0; b0 < B; b0 += chunk) {
    const int Bc = std::min(chunk, B - b0);
    float* mel = features_out ? features_out + (size_t)b0 * e->cfg.n_mels * T : w.mel;
    rc = logmel_whisper_impl(e->ctx, (const char*)pcm + (size_t)b0 * pcm_stride * esz, pcm_is_i16, pcm_stride,
                             n_valid ? n_valid + b0 : nullptr, max_valid, Bc, T, e->cfg.n_mels, mel, w.logmel, awt_logmel_workspace_bytes(Bc), s);
    if (rc) return rc;
    rc = forward_chunk(e, mel, Bc, hidden + (size_t)b0 * e->cfg.n_ctx * e->cfg.d_model, w.enc, s, Sc);
    if (rc) return rc;
  }
  return AWT_OK;
}

extern "C" int awt_conv_stem_positions(int n_ctx, int max_valid) { return conv_stem_positions(n_ctx, max_valid); }

// ------------------------------------------------------------------------------------------------ single operators
namespace {
// awt_op_linear's workspace: the x and w operand planes, a flag word ("a weight is not fp16-exact"), the 16-row w copies (f16f8); the ping-pong form
// (tuning knob "gemm_pp" = 2) reads the same bytes as x in split lines over the two x planes and the packed weight image over the two w planes
struct OpLinearWs {
  PlanePair x, w; int* flag; bf16_t* s16; uint8_t* s8; size_t s_bytes, bytes;     // s_bytes: both copies, from s16 on
  char* x_ilv() const { return (char*)x.hi; }
  char* w_pp() const { return (char*)w.hi; }
};
// x [M, ldx] and w [N, K] with pitches of their own (awt_op_linear_fused: the conv stem's x [B 2 S, Cin] against w [N, 3 Cin]); awt_op_linear has ldx == K
OpLinearWs op_linear_layout(void* base, int M, int ldx, int N, int K) {
  const size_t sb = ((size_t)N + 255) / 256 * 256 * K * 2;      // the 16-row w copies cover whole 256-column tiles
  Carver cv(base);
  return {take_planes(cv, (size_t)M * ldx), take_planes(cv, (size_t)N * K), cv.take<int>(256), cv.take<bf16_t>(sb), cv.take<uint8_t>(sb), 2 * align_up(sb), cv.bytes()};
}
OpLinearWs op_linear_layout(void* base, int M, int N, int K) { return op_linear_layout(base, M, K, N, K); }
// w [N, K] fp32 as the operand planes of `terms` in the workspace's w pieces (fragment-major; f16f8: also the 16-row copies)
int op_linear_pack_weight(awt_ctx* c, const float* w, int N, int K, int terms, const OpLinearWs& ws, Planes& pw, hipStream_t s) {
  pw.hi = ws.w.hi; pw.lo = ws.w.lo; pw.x8 = (uint8_t*)pw.lo + (size_t)N * K; pw.rows = N; pw.ld = K;
  if (terms == PREC_F16F8) {
    pw.s_rows = ((int64_t)N + 255) / 256 * 256;
    pw.s16 = ws.s16; pw.s8 = ws.s8;
    if (N % 256 != 0) {   // the rows beyond N are read by the last column tile (never stored): keep them finite
      if (hipMemsetAsync(ws.s16, 0, ws.s_bytes, s) != hipSuccess) return awt_fail(AWT_ERR_HIP, "op_linear: weight copy reset failed");
    }
  }
  // as awt_encoder_set_weight does: fp16-exact weights take the GEMM without the x_hi w_lo product.  The probe reads one flag back on the host and
  // synchronises `s`, which a stream that is recording into a HIP graph cannot do: there the weight is packed without the probe and the GEMM keeps
  // every cross term -- the form of any weight that is not fp16-exact, and for one that is, a product with an all-zero plane more
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  const bool probe = (terms == PREC_F16F8 || terms == PREC_F16X3) && !(hipStreamIsCapturing(s, &capturing) == hipSuccess && capturing == hipStreamCaptureStatusActive);
  if (probe) return probe_exact16(c, "op_linear", w, pw, N, K, 0, terms, ws.flag, 0, 1, s);
  return pack(c, w, pw, N, K, 1, 0, 0, terms, s);     // fragment-major
}
// awt_op_attention's workspace: the two 2-byte planes of q, of k and of v
struct OpAttentionWs { PlanePair q, k, v; size_t bytes; };
OpAttentionWs op_attention_layout(void* base, int B, int H, int S) {
  const size_t n = (size_t)B * H * S * 64;
  Carver cv(base);
  return {take_planes(cv, n), take_planes(cv, n), take_planes(cv, n), cv.bytes()};
}
// awt_op_attention_backward's workspace: the two 2-byte planes of q, of k, of v (head-major) and of dO (row-major)
struct OpAttentionBwdWs { PlanePair q, k, v, d_o; size_t bytes; };
OpAttentionBwdWs op_attention_backward_layout(void* base, int B, int H, int S) {
  const size_t n = (size_t)B * H * S * 64;
  Carver cv(base);
  return {take_planes(cv, n), take_planes(cv, n), take_planes(cv, n), take_planes(cv, n), cv.bytes()};
}
}  // namespace

extern "C" size_t awt_op_linear_workspace_bytes(int M, int N, int K) { return op_linear_layout(nullptr, M, N, K).bytes; }
extern "C" int awt_op_linear(awt_ctx* c, const float* x, const float* w, const float* bias, float* y, int M, int N, int K,
                             int terms, void* workspace, size_t ws_bytes, void* stream) {
  AWT_REQUIRE(prec_known(terms), AWT_ERR_INVALID, "op_linear: terms must be 1 (bf16), 2 (fp16), 3 (bf16x3), 4 (fp16x3) or 5 (f16f8)");
  AWT_REQUIRE(c && x && w && y && workspace, AWT_ERR_INVALID, "op_linear: null argument");
  AWT_REQUIRE(M > 0 && N > 0 && N % 128 == 0 && K > 0 && K % 64 == 0, AWT_ERR_INVALID, "op_linear: N % 128 == 0 and K % 64 == 0 required");
  AWT_REQUIRE(ws_bytes >= awt_op_linear_workspace_bytes(M, N, K), AWT_ERR_WORKSPACE, "op_linear: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const OpLinearWs ws = op_linear_layout(workspace, M, N, K);
  if (terms == PREC_F16F8 && awt_gemm_pp_mode() == 2 && gemm_pp_supported(M, N, K, EPI_F32)) {
    // the persistent ping-pong kernel (tuning knob "gemm_pp" = 2): x as split lines over the two x planes' space (its 256-row panel reads beyond M
    // stay inside the workspace: the packed weight image of N >= 256 rows follows), the weight in the packed region image over the two w planes' space
    Act ai; ai.ilv = ws.x_ilv();
    int rcp = launch_split_planes(c, x, (int64_t)M * K, 1.0f, terms, kF8Act, nullptr, nullptr, nullptr, nullptr, s, ai.ilv); if (rcp) return rcp;
    if (hipMemsetAsync(ws.w_pp(), 0, gemm_pp_weight_bytes(N, K), s) != hipSuccess) return awt_fail(AWT_ERR_HIP, "op_linear: weight image reset failed");
    rcp = launch_pack_weight_pp(c, w, N, K, 0, ws.w_pp(), s); if (rcp) return rcp;
    Planes pwp; pwp.pp = ws.w_pp(); pwp.rows = N; pwp.ld = K;
    GemmSeg sgp = seg_plain(ai, K, pwp, 0, K, M);
    GemmOut op{}; op.f32 = y; op.ldo = N; op.bias = bias; op.n_valid = N;
    return launch_gemm_pp(c, M, N, sgp, EPI_F32, op, s);
  }
  const Act ax = make_act(ws.x, (size_t)M * K, terms);
  int rc = launch_split_planes(c, x, (int64_t)M * K, 1.0f, terms, kF8Act, ws.x.hi, ws.x.lo, ax.hi8, ax.lo8, s); if (rc) return rc;
  Planes pw;
  rc = op_linear_pack_weight(c, w, N, K, terms, ws, pw, s); if (rc) return rc;
  GemmSeg sg = seg_plain(ax, K, pw, 0, K, M);
  GemmOut o{}; o.f32 = y; o.ldo = N; o.bias = bias; o.n_valid = N;
  return launch_gemm(c, M, N, &sg, 1, terms, EPI_F32, o, s);
}

extern "C" size_t awt_op_linear_fused_workspace_bytes(int x_rows, int ldx, int N, int ldw) { return op_linear_layout(nullptr, x_rows, ldx, N, ldw).bytes; }
extern "C" int awt_op_linear_fused(awt_ctx* c, const awt_linear_fused_args* a, void* workspace, size_t ws_bytes, void* stream) {
  AWT_REQUIRE(c && a && a->x && a->w && workspace, AWT_ERR_INVALID, "op_linear_fused: null argument");
  const int M = a->M, N = a->N, terms = a->terms, epi = a->epi, nseg = a->nseg;
  AWT_REQUIRE(prec_known(terms), AWT_ERR_INVALID, "op_linear_fused: terms must be 1 (bf16), 2 (fp16), 3 (bf16x3), 4 (fp16x3) or 5 (f16f8)");
  AWT_REQUIRE(epi >= EPI_F32 && epi <= EPI_BF16_DGELU, AWT_ERR_INVALID, "op_linear_fused: unknown epilogue");
  AWT_REQUIRE(M > 0 && N > 0 && N % 128 == 0 && nseg >= 1 && nseg <= 3, AWT_ERR_INVALID, "op_linear_fused: N % 128 == 0 and 1..3 K segments required");
  AWT_REQUIRE(a->x_rows > 0 && a->ldx > 0 && a->ldx % 64 == 0 && a->ldw > 0 && a->ldw % 64 == 0, AWT_ERR_INVALID, "op_linear_fused: ldx and ldw must be positive multiples of 64");
  for (int i = 0; i < nseg; ++i) {
    const int k = a->seg_k[i], xc = a->seg_xcol[i], wc = a->seg_wcol[i], ro = a->seg_rows_out[i], ri = a->seg_rows_in[i], rm = a->seg_row_mul[i];
    AWT_REQUIRE(k > 0 && k % 64 == 0 && xc >= 0 && xc % 64 == 0 && wc >= 0 && wc % 64 == 0 && xc + k <= a->ldx && wc + k <= a->ldw, AWT_ERR_INVALID,
                "op_linear_fused: a K segment must be a 64-aligned column slice of x and of w");
    AWT_REQUIRE(ro > 0 && ri > 0 && rm > 0 && (int64_t)rm * ro == ri, AWT_ERR_INVALID, "op_linear_fused: bad row map (rows_in must be row_mul * rows_out)");
    AWT_REQUIRE((int64_t)((M - 1) / ro + 1) * ri <= a->x_rows, AWT_ERR_INVALID, "op_linear_fused: the row map reads beyond x_rows");
  }
  const bool f8 = terms == PREC_F16F8, planes_out = !(epi == EPI_F32 || epi == EPI_F32_RESID || epi == EPI_F32_GELU_POS);
  const int n_valid = a->n_valid > 0 ? a->n_valid : N, ldo = a->ldo > 0 ? a->ldo : N;
  AWT_REQUIRE(a->n_valid >= 0 && n_valid <= N && n_valid % (f8 ? 8 : 4) == 0 && ldo >= n_valid && ldo % 8 == 0, AWT_ERR_INVALID,
              "op_linear_fused: n_valid must be a multiple of 4 (of 8 with terms 5) in (0, N], ldo a multiple of 8 that holds it");
  AWT_REQUIRE(a->m_pick >= 0, AWT_ERR_INVALID, "op_linear_fused: m_pick must not be negative");
  // the ping-pong kernel (tuning knob "gemm_pp" = 2), as awt_op_linear takes it: one plain dense segment of a shape it supports
  const bool plain = nseg == 1 && a->seg_xcol[0] == 0 && a->seg_wcol[0] == 0 && a->seg_k[0] == a->ldx && a->ldx == a->ldw && a->x_rows == M && a->seg_rows_out[0] == M &&
                     a->seg_rows_in[0] == M && a->seg_row_mul[0] == 1 && a->seg_row_add[0] == 0;
  const bool pp_shape = f8 && awt_gemm_pp_mode() == 2 && plain && gemm_pp_supported(M, N, a->ldx, EPI_F32);
  AWT_REQUIRE(!pp_shape || gemm_pp_supported(M, N, a->ldx, epi), AWT_ERR_INVALID, "op_linear_fused: the ping-pong kernel does not have this epilogue");
  AWT_REQUIRE(!a->split_lines || (pp_shape && a->out_ilv && (epi == EPI_BF16 || epi == EPI_BF16_GELU) && ldo == N && n_valid == N), AWT_ERR_INVALID,
              "op_linear_fused: a split-line output is a dense [M, N] activation of the ping-pong kernel's EPI_BF16 / EPI_BF16_GELU");
  if (!planes_out) AWT_REQUIRE(a->out_f32 && (epi != EPI_F32_RESID || a->resid) && (epi != EPI_F32_GELU_POS || (a->pos && a->rows_pos > 0)), AWT_ERR_INVALID,
                               "op_linear_fused: null fp32 output or side input");
  else if (!a->split_lines) AWT_REQUIRE(a->out_hi && (prec_products(terms) == 1 || (f8 ? a->out_lo8 : a->out_lo)), AWT_ERR_INVALID, "op_linear_fused: null output plane");
  if (epi == EPI_BF16_GELU_SAVE) AWT_REQUIRE(a->out_hi2 && (prec_products(terms) == 1 || a->out_lo2), AWT_ERR_INVALID, "op_linear_fused: null pre-activation plane");
  if (epi == EPI_BF16_DGELU) AWT_REQUIRE(a->pre_hi, AWT_ERR_INVALID, "op_linear_fused: null saved pre-activation");
  if (epi == EPI_QKV) AWT_REQUIRE(a->S > 0 && a->H > 0 && N == 3 * a->H * 64 && M % a->S == 0, AWT_ERR_INVALID, "op_linear_fused: EPI_QKV needs N == 3 H 64 and M % S == 0");
  AWT_REQUIRE(ws_bytes >= awt_op_linear_fused_workspace_bytes(a->x_rows, a->ldx, N, a->ldw), AWT_ERR_WORKSPACE, "op_linear_fused: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const OpLinearWs ws = op_linear_layout(workspace, a->x_rows, a->ldx, N, a->ldw);

  GemmOut o{};
  o.f32 = a->out_f32; o.resid = a->resid; o.ldo = ldo; o.bias = a->bias; o.n_valid = n_valid; o.scale = a->scale; o.m_pick = a->m_pick;
  o.pos = a->pos; o.rows_pos = a->rows_pos; o.pre_hi = (const bf16_t*)a->pre_hi; o.pre_lo = (const bf16_t*)a->pre_lo;
  if (planes_out) {   // one 2-byte plane with a single product, as the encoder's buffers have then
    o.hi = (bf16_t*)a->out_hi; o.lo = (!f8 && prec_products(terms) == 3) ? (bf16_t*)a->out_lo : nullptr;
    if (f8) { o.hi8 = (uint8_t*)a->out_hi8; o.lo8 = (uint8_t*)a->out_lo8; }
    if (epi == EPI_BF16_GELU_SAVE) { o.hi2 = (bf16_t*)a->out_hi2; o.lo2 = prec_products(terms) == 3 ? (bf16_t*)a->out_lo2 : nullptr; }
    if (a->split_lines) { o.hi = nullptr; o.hi8 = o.lo8 = nullptr; o.ilv = (char*)a->out_ilv; }
  }
  if (epi == EPI_QKV) { o.S = a->S; o.H = a->H; o.plane_stride = (int64_t)M * a->H * 64; o.skip_v8 = (f8 && a->skip_v8) ? 1 : 0; }

  const int64_t nx = (int64_t)a->x_rows * a->ldx;
  if (pp_shape) {
    const int K = a->ldx;
    Act ai; ai.ilv = ws.x_ilv();
    int rcp = launch_split_planes(c, a->x, nx, 1.0f, terms, kF8Act, nullptr, nullptr, nullptr, nullptr, s, ai.ilv); if (rcp) return rcp;
    if (hipMemsetAsync(ws.w_pp(), 0, gemm_pp_weight_bytes(N, K), s) != hipSuccess) return awt_fail(AWT_ERR_HIP, "op_linear_fused: weight image reset failed");
    rcp = launch_pack_weight_pp(c, a->w, N, K, 0, ws.w_pp(), s); if (rcp) return rcp;
    Planes pwp; pwp.pp = ws.w_pp(); pwp.rows = N; pwp.ld = K;
    return launch_gemm_pp(c, M, N, seg_plain(ai, K, pwp, 0, K, M), (GemmEpilogue)epi, o, s);
  }
  const Act ax = make_act(ws.x, (size_t)nx, terms);
  int rc = launch_split_planes(c, a->x, nx, 1.0f, terms, kF8Act, ws.x.hi, ws.x.lo, ax.hi8, ax.lo8, s); if (rc) return rc;
  Planes pw;
  rc = op_linear_pack_weight(c, a->w, N, a->ldw, terms, ws, pw, s); if (rc) return rc;
  GemmSeg sg[3];
  for (int i = 0; i < nseg; ++i) {
    sg[i] = seg_plain(act_offset(ax, a->seg_xcol[i]), a->ldx, pw, a->seg_wcol[i], a->seg_k[i], M);
    sg[i].rows_out = a->seg_rows_out[i]; sg[i].rows_in = a->seg_rows_in[i]; sg[i].row_mul = a->seg_row_mul[i]; sg[i].row_add = a->seg_row_add[i];
  }
  return launch_gemm(c, M, N, sg, nseg, terms, (GemmEpilogue)epi, o, s);
}

extern "C" int awt_op_layernorm(awt_ctx* c, const float* x, const float* gamma, const float* beta, float* y, int M, int d,
                                float eps, void* stream) {
  return launch_layernorm(c, x, gamma, beta, M, d, eps, y, Act{}, PREC_BF16X3, (hipStream_t)stream);
}

namespace {
// q, k, v [B, H, S, 64] fp32 as the operand planes of `terms` in awt_op_attention's workspace (the kernels expect q * log2(e); f16f8: the second 2-byte
// plane holds the two e4m3 planes).  v8 = false (f16f8): v's fp16 plane alone, as the QKV epilogue's skip_v8 leaves it.
int op_attention_planes(awt_ctx* c, const float* q, const float* k, const float* v, int64_t n, int terms, const OpAttentionWs& ws, bool v8, hipStream_t s) {
  bf16_t* const pl[6] = {ws.q.hi, ws.q.lo, ws.k.hi, ws.k.lo, ws.v.hi, ws.v.lo};
  const float* src[3] = {q, k, v};
  const int f8exp[3] = {kF8Q, kF8KV, kF8KV};
  for (int i = 0; i < 3; ++i) {
    uint8_t* b8 = (uint8_t*)pl[2 * i + 1];
    const int prec = (terms == PREC_F16F8 && i == 2 && !v8) ? PREC_F16 : terms;      // PREC_F16 writes the same fp16 plane and nothing else
    int rc = launch_split_planes(c, src[i], n, i == 0 ? 1.4426950408889634f : 1.0f, prec, f8exp[i], pl[2 * i], pl[2 * i + 1], b8, b8 + n, s);
    if (rc) return rc;
  }
  return AWT_OK;
}
}  // namespace

extern "C" size_t awt_op_attention_workspace_bytes(int B, int H, int S) { return op_attention_layout(nullptr, B, H, S).bytes; }
extern "C" int awt_op_attention(awt_ctx* c, const float* q, const float* k, const float* v, float* o, int B, int H, int S,
                                int terms, void* workspace, size_t ws_bytes, void* stream) {
  AWT_REQUIRE(prec_known(terms), AWT_ERR_INVALID, "op_attention: terms must be 1 (bf16), 2 (fp16), 3 (bf16x3), 4 (fp16x3) or 5 (f16f8)");
  AWT_REQUIRE(c && q && k && v && o && workspace, AWT_ERR_INVALID, "op_attention: null argument");
  AWT_REQUIRE(ws_bytes >= awt_op_attention_workspace_bytes(B, H, S), AWT_ERR_WORKSPACE, "op_attention: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)B * H * S * 64;
  const OpAttentionWs ws = op_attention_layout(workspace, B, H, S);
  int rc = op_attention_planes(c, q, k, v, n, terms, ws, true, s); if (rc) return rc;
  if (terms == PREC_F16F8)
    return launch_attention_f16f8(c, make_act(ws.q, n, terms), make_act(ws.k, n, terms), make_act(ws.v, n, terms), Act{}, o, nullptr, B, H, S, s);
  return launch_attention(c, ws.q, ws.k, ws.v, PlanePair{}, o, nullptr, B, H, S, terms, s);
}

// awt_op_attention with the output forms and the log-sum-exp the encoder layer asks of the same launchers (encoder_layer): everything either launcher
// would refuse is refused here first, under this entry's name
extern "C" size_t awt_op_attention_ex_workspace_bytes(int B, int H, int S) { return op_attention_layout(nullptr, B, H, S).bytes; }
extern "C" int awt_op_attention_ex(awt_ctx* c, const float* q, const float* k, const float* v, float* o_f32, void* o_hi, void* o_lo, void* o_hi8,
                                   void* o_lo8, void* o_ilv, float* lse2, int B, int H, int S, int terms, void* workspace, size_t ws_bytes, void* stream) {
  AWT_REQUIRE(prec_known(terms), AWT_ERR_INVALID, "op_attention_ex: terms must be 1 (bf16), 2 (fp16), 3 (bf16x3), 4 (fp16x3) or 5 (f16f8)");
  AWT_REQUIRE(c && q && k && v && workspace, AWT_ERR_INVALID, "op_attention_ex: null argument");
  AWT_REQUIRE(B > 0 && H > 0 && S > 0, AWT_ERR_INVALID, "op_attention_ex: bad shape");
  const bool f8 = terms == PREC_F16F8, planes = o_hi || o_lo || o_hi8 || o_lo8;
  AWT_REQUIRE((o_f32 != nullptr) + (o_ilv != nullptr) + planes == 1, AWT_ERR_INVALID, "op_attention_ex: exactly one of o_f32, the output planes and o_ilv is required");
  AWT_REQUIRE(!o_ilv || f8, AWT_ERR_INVALID, "op_attention_ex: a split-line output is an f16f8 format (terms 5)");
  if (planes) {
    AWT_REQUIRE(o_hi, AWT_ERR_INVALID, "op_attention_ex: null o_hi");
    if (f8) AWT_REQUIRE(o_lo8 && !o_lo, AWT_ERR_INVALID, "op_attention_ex: terms 5 writes o_hi, o_hi8 (optional) and o_lo8; o_lo8 is null or o_lo is set");
    else AWT_REQUIRE(!o_hi8 && !o_lo8 && (prec_products(terms) == 1 || o_lo), AWT_ERR_INVALID, "op_attention_ex: terms 1 - 4 write o_hi and, with terms 3 / 4, o_lo");
  }
  AWT_REQUIRE(ws_bytes >= awt_op_attention_ex_workspace_bytes(B, H, S), AWT_ERR_WORKSPACE, "op_attention_ex: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)B * H * S * 64;
  const OpAttentionWs ws = op_attention_layout(workspace, B, H, S);
  int rc = op_attention_planes(c, q, k, v, n, terms, ws, !f8 || attention_f16f8_reads_v8(lse2 != nullptr), s); if (rc) return rc;
  if (f8) {
    Act ao; ao.p16 = (bf16_t*)o_hi; ao.hi8 = (uint8_t*)o_hi8; ao.lo8 = (uint8_t*)o_lo8; ao.ilv = (char*)o_ilv;
    return launch_attention_f16f8(c, make_act(ws.q, n, terms), make_act(ws.k, n, terms), make_act(ws.v, n, terms), ao, o_f32, lse2, B, H, S, s);
  }
  const PlanePair po{(bf16_t*)o_hi, prec_products(terms) == 3 ? (bf16_t*)o_lo : nullptr};     // one plane with a single product, as the encoder's buffers have then
  return launch_attention(c, ws.q, ws.k, ws.v, po, o_f32, lse2, B, H, S, terms, s);
}

// What one encoder layer's training pass runs around its attention, on caller tensors: the operand planes, the training form of the forward
// (row-major o planes and the saved log-sum-exp; forward_layer with `save`), then launch_attention_bwd as awt_encoder_backward calls it.
extern "C" size_t awt_op_attention_backward_workspace_bytes(int B, int H, int S) { return op_attention_backward_layout(nullptr, B, H, S).bytes; }
extern "C" int awt_op_attention_backward(awt_ctx* c, const float* q, const float* k, const float* v, const float* d_o, void* o_hi, void* o_lo,
                                         float* lse2, float* delta, void* g_hi, void* g_lo, int B, int H, int S, float qscale, int terms,
                                         int grad_terms, void* workspace, size_t ws_bytes, void* stream) {
  AWT_REQUIRE(terms == PREC_BF16 || terms == PREC_BF16X3, AWT_ERR_INVALID, "op_attention_backward: terms must be 1 (bf16) or 3 (bf16x3)");
  AWT_REQUIRE(grad_terms == terms || (terms == 3 && grad_terms == 1), AWT_ERR_INVALID, "op_attention_backward: grad_terms must equal terms, or be 1 with terms 3");
  AWT_REQUIRE(B > 0 && H > 0 && S > 0, AWT_ERR_INVALID, "op_attention_backward: bad shape");
  AWT_REQUIRE(c && q && k && v && d_o && o_hi && lse2 && delta && g_hi && workspace, AWT_ERR_INVALID, "op_attention_backward: null argument");
  AWT_REQUIRE(terms == 1 || (o_lo && g_lo), AWT_ERR_INVALID, "op_attention_backward: the lo planes of o and of the gradients are required with terms 3");
  AWT_REQUIRE(ws_bytes >= awt_op_attention_backward_workspace_bytes(B, H, S), AWT_ERR_WORKSPACE, "op_attention_backward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)B * H * S * 64;
  const OpAttentionBwdWs ws = op_attention_backward_layout(workspace, B, H, S);
  const PlanePair pl[4] = {ws.q, ws.k, ws.v, ws.d_o};
  const float* src[4] = {q, k, v, d_o};
  for (int i = 0; i < 4; ++i) {   // the kernels expect q * log2(e)
    int rc = launch_split_planes(c, src[i], n, i == 0 ? 1.4426950408889634f : 1.0f, terms, 0, pl[i].hi, pl[i].lo, nullptr, nullptr, s);
    if (rc) return rc;
  }
  const auto planes = [&](const PlanePair& p) { return PlanePair{p.hi, terms == 3 ? p.lo : nullptr}; };   // terms 1: one plane each, as the encoder's buffers have then
  const PlanePair po = planes({(bf16_t*)o_hi, (bf16_t*)o_lo}), pg = planes({(bf16_t*)g_hi, (bf16_t*)g_lo});
  int rc = launch_attention(c, planes(ws.q), planes(ws.k), planes(ws.v), po, nullptr, lse2, B, H, S, terms, s);
  if (rc) return rc;
  return launch_attention_bwd(c, planes(ws.q), planes(ws.k), planes(ws.v), po, planes(ws.d_o), lse2, delta, pg, B, H, S, qscale, terms, grad_terms, s);
}

// ------------------------------------------------------------------------------------------------ LoRA fine-tune step
extern "C" int awt_encoder_set_grad_scale_log2(awt_encoder* e, int k) {
  AWT_REQUIRE(e && e->cfg.training, AWT_ERR_STATE, "encoder_set_grad_scale_log2: encoder was not created with cfg.training");
  AWT_REQUIRE(k >= -60 && k <= 60, AWT_ERR_INVALID, "encoder_set_grad_scale_log2: k must be in -60 .. 60");
  e->grad_scale_log2 = k;
  return AWT_OK;
}

extern "C" size_t awt_encoder_train_workspace_bytes(const awt_encoder* e, int B) {
  if (!e || B <= 0 || !e->cfg.training) return 0;
  return carve_train(e, nullptr, B).bytes;
}

namespace {
// One layer's block of adapter gradients: for every enabled target in the order q, k, v, out, fc1, fc2: dA [r, K_in] then dB [N_out, r].
// dA[t] / dB[t]: element offsets of target t (that order) inside the block, meaningful for the enabled targets; total: the block's elements.
enum { T_Q, T_K, T_V, T_OUT, T_FC1, T_FC2, T_COUNT };
struct LoraGradSlots { size_t dA[T_COUNT], dB[T_COUNT], total; };
LoraGradSlots lora_grad_slots(const awt_encoder_cfg& c) {
  const size_t r = c.lora_rank, d = c.d_model, f = c.ffn_dim;
  const struct { uint32_t bit; size_t k_in, n_out; } target[T_COUNT] = {{AWT_LORA_Q, d, d},   {AWT_LORA_K, d, d},   {AWT_LORA_V, d, d},
                                                                       {AWT_LORA_OUT, d, d}, {AWT_LORA_FC1, d, f}, {AWT_LORA_FC2, f, d}};
  LoraGradSlots g{};
  for (int t = 0; t < T_COUNT; ++t) {
    if (!(c.lora_targets & target[t].bit)) continue;
    g.dA[t] = g.total;
    g.dB[t] = g.dA[t] + r * target[t].k_in;
    g.total = g.dB[t] + target[t].n_out * r;
  }
  return g;
}
}  // namespace

extern "C" size_t awt_encoder_lora_grad_count(const awt_encoder* e) {
  if (!e || e->cfg.lora_rank <= 0) return 0;
  return (size_t)e->cfg.n_layers * lora_grad_slots(e->cfg).total;
}

extern "C" int awt_encoder_forward_train(awt_encoder* e, const float* mel, int B, int n_frames, float* hidden, void* saved,
                                         size_t saved_bytes, void* stream) {
  AWT_REQUIRE(e && mel && hidden && saved && B > 0, AWT_ERR_INVALID, "encoder_forward_train: bad argument");
  AWT_REQUIRE(e->cfg.training, AWT_ERR_STATE, "encoder_forward_train: encoder was not created with cfg.training");
  const int T = 2 * e->cfg.n_ctx;
  if (n_frames != T)
    return awt_fail(AWT_ERR_VALUE, "Whisper expects the mel input features to be of length " + std::to_string(T) + ", but found " +
                                       std::to_string(n_frames) + ". Make sure to pad the input mel features to " + std::to_string(T) + ".");
  int rc = require_weights(e); if (rc) return rc;
  AWT_REQUIRE(saved_bytes >= awt_encoder_train_workspace_bytes(e, B), AWT_ERR_WORKSPACE, "encoder_forward_train: saved buffer too small");
  AWT_REQUIRE(((uintptr_t)saved & 255) == 0, AWT_ERR_INVALID, "encoder_forward_train: saved buffer must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  TrainWs w = carve_train(e, (char*)saved, B);
  rc = conv_stem(e, mel, B, w.conv, w.layer[0].x_in, s); if (rc) return rc;
  for (int li = 0; li < e->cfg.n_layers; ++li) { rc = encoder_layer(e, e->layers[li], w.layer[li], B, true, s); if (rc) return rc; }
  return launch_layernorm(e->ctx, w.x_final, e->lnf_g, e->lnf_b, B * e->cfg.n_ctx, e->cfg.d_model, 1e-5f, hidden, Act{}, e->prec, s);
}

extern "C" int awt_encoder_set_comm(awt_encoder* e, awt_comm* m, int groups) {
  AWT_REQUIRE(e, AWT_ERR_INVALID, "encoder_set_comm: null encoder");
  AWT_REQUIRE(groups >= 1, AWT_ERR_INVALID, "encoder_set_comm: groups must be >= 1");
  AWT_REQUIRE(!m || m->ctx == e->ctx, AWT_ERR_INVALID, "encoder_set_comm: communicator and encoder belong to different contexts");
  e->comm = m;
  e->comm_groups = std::min(std::min(groups, 4), e->cfg.n_layers);
  return AWT_OK;
}

extern "C" int awt_encoder_backward(awt_encoder* e, const float* d_hidden, int B, void* saved, size_t saved_bytes, float* lora_grads,
                                    size_t n_grads, void* stream) {
  return awt_encoder_backward_ex(e, d_hidden, B, saved, saved_bytes, lora_grads, n_grads, 0u, stream);
}

extern "C" int awt_encoder_backward_ex(awt_encoder* e, const float* d_hidden, int B, void* saved, size_t saved_bytes, float* lora_grads,
                                       size_t n_grads, uint32_t flags, void* stream) {
  AWT_REQUIRE(e && d_hidden && saved && lora_grads && B > 0, AWT_ERR_INVALID, "encoder_backward: bad argument");
  AWT_REQUIRE(!(flags & ~(uint32_t)(AWT_BWD_ACCUMULATE | AWT_BWD_ALLREDUCE)), AWT_ERR_INVALID, "encoder_backward: unknown flag");
  AWT_REQUIRE(!(flags & AWT_BWD_ALLREDUCE) || e->comm, AWT_ERR_STATE, "encoder_backward: AWT_BWD_ALLREDUCE needs awt_encoder_set_comm first");
  const int accumulate = (flags & AWT_BWD_ACCUMULATE) ? 1 : 0;
  const bool exchange = (flags & AWT_BWD_ALLREDUCE) != 0;
  AWT_REQUIRE(e->cfg.training, AWT_ERR_STATE, "encoder_backward: encoder was not created with cfg.training");
  AWT_REQUIRE(saved_bytes >= awt_encoder_train_workspace_bytes(e, B), AWT_ERR_WORKSPACE, "encoder_backward: saved buffer too small");
  const bool tb = e->train_base;
  AWT_REQUIRE(n_grads == (tb ? awt_encoder_base_grad_count(e) : awt_encoder_lora_grad_count(e)), AWT_ERR_INVALID, "encoder_backward: the gradient buffer has the wrong element count");
  hipStream_t s = (hipStream_t)stream;
  const awt_encoder_cfg& c = e->cfg;
  const int S = c.n_ctx, d = c.d_model, f = c.ffn_dim, H = c.n_heads, terms = c.mfma_terms, r = c.lora_rank;
  // products of the gradient contractions: the forward's (default), or one bf16 product per fragment pair (opt-in fast backward)
  // backward_terms = 5: the MLP's two backward GEMMs run in f16f8 (fp16 + two e4m3 planes, 2 MFMA-equivalents instead of 3), everything else in split-bf16
  const bool mlp8 = e->mlp_f8;
  const int gterms = mlp8 ? PREC_BF16X3 : (c.backward_terms ? c.backward_terms : terms);
  // the pass carries 2^k x the gradient from the final LayerNorm on (fp16 planes: awt_encoder_set_grad_scale_log2); the adapter gradients leave unscaled
  const float gscale = ldexpf(1.0f, e->grad_scale_log2), inv_gscale = ldexpf(1.0f, -e->grad_scale_log2);
  const int M = B * S;
  const int64_t plane = (int64_t)M * d;
  const float lscale = r > 0 ? c.lora_alpha / (float)r : 0.f;
  TrainWs w = carve_train(e, (char*)saved, B);
  const LoraGradSlots gslots = lora_grad_slots(c);
  const awt_encoder::GradOffsets& go = e->goff;     // train_base: where each base parameter's gradient goes (build_grad_layout)
  const size_t per_layer = tb ? e->g_per_layer : gslots.total;
  float* const layer_grads = lora_grads + (tb ? e->g_head : 0);     // train_base: the non-layer parameters come first
  // the gradient buffers, each as the plane pair the row kernels take (p) and as the GEMM operand / output it also is (a)
  struct Grad { PlanePair p; Act a; };
  auto grad = [&](const PlanePair& p, size_t elems) { return Grad{p, make_act(p, elems, PREC_BF16X3)}; };
  const Grad dxp = grad(w.dxp, (size_t)M * d), dpre = grad(w.dpre, (size_t)M * f), datt = grad(w.datt, (size_t)M * d), dqkv = grad(w.dqkv, 3 * (size_t)M * d);
  const Grad du = grad(w.du, (size_t)M * 128);
  int rc;

  // ---- cfg.train_base: gradients of the base parameters, each formed where its dY is live.  dW = dY^T X on the weight-gradient GEMM (wgrad.hip), bias and
  //      LayerNorm gradients on the column-reduction row kernels; all of them leave divided by the pass' gradient scale.
  const int wterms = (gterms == PREC_BF16 || e->planes == 1) ? 1 : 3;   // three products need the lo planes of the saved activations
  float* const partial = w.partial;
  auto dW = [&](const PlanePair& y, int64_t ldy, int ycol, int N, const PlanePair& x, int64_t ldx, int xcol, int K, int rows, const WgradRowMap* map,
                float* out, int64_t sn, int64_t sk) -> int {
    const WgradOperand yo{y.hi, wterms == 3 ? y.lo : nullptr, ldy, ycol}, xo{x.hi, wterms == 3 ? x.lo : nullptr, ldx, xcol};
    return launch_wgrad(e->ctx, yo, N, xo, K, rows, map, wterms, inv_gscale, out, sn, sk, accumulate, partial, w.partial_bytes, s);
  };
  auto dBias = [&](const PlanePair& y, int64_t ldy, int ycol, int N, int rows, float* out) -> int {   // column sums of dY, <= 1024 columns per launch
    for (int c0 = 0; c0 < N; c0 += 1024) {
      const int n = std::min(1024, N - c0);
      int rc2 = launch_param_grad(e->ctx, nullptr, y.at(ycol + c0), ldy, nullptr, rows, n, 0.f, inv_gscale, accumulate, nullptr, out + c0, partial, s);
      if (rc2) return rc2;
    }
    return AWT_OK;
  };
  auto dLN = [&](const float* dy, const float* x, float scale, float* dgamma) -> int {   // dgamma [d] then dbeta [d]
    return launch_param_grad(e->ctx, dy, PlanePair{}, 0, x, M, d, 1e-5f, scale, accumulate, dgamma, dgamma + d, partial, s);
  };
  if (tb) { rc = dLN(d_hidden, w.x_final, 1.0f, lora_grads + go.lnf); if (rc) return rc; }   // the final layer_norm sees the unscaled gradient

  // One adapter group (adapters that share an input): du = dy B into w.du, then per adapter dA = lscale du^T x_in and dB = dy^T u into the adapter's
  // slots of the layer's block `gl` (lora_grad_slots).  Forward: u = lscale x_in A^T (saved), y = x_in W^T + b + u B^T.  The group's du stays in w.du
  // for the caller's dX product, which takes it as a second K-segment against (lscale A)^T.
  struct Slot { uint32_t bit; int target; int col; int n_out; };
  auto group_backward = [&](LoraGroup& lg, const Grad& dy, int ld_dy, int n_out_total, const Slot* slots, int nslot, const PlanePair& xin, int k_in, const PlanePair& u,
                            float* gl) -> int {
    if (!lg.active) return AWT_OK;
    {
      GemmSeg sg = seg_plain(dy.a, ld_dy, lg.bT, 0, n_out_total, M);
      GemmOut o{}; set_out(o, du.a); o.ldo = lg.kp; o.n_valid = lg.kp; o.scale = 1.0f;
      int rc2 = launch_gemm(e->ctx, M, 128, &sg, 1, gterms, EPI_BF16, o, s); if (rc2) return rc2;
    }
    for (int i = 0; i < nslot; ++i) {          // adapter i of the group owns rows / columns i r .. i r + r - 1 of A / B, u and du (set_weight)
      if (!(c.lora_targets & slots[i].bit)) continue;
      int rc2 = launch_outer_reduce(e->ctx, du.p, lg.kp, i * r, r, xin, k_in, 0, k_in, M, lscale * inv_gscale, gl + gslots.dA[slots[i].target], k_in, 1,
                                    w.partial, w.partial_bytes, accumulate, s);
      if (rc2) return rc2;
      rc2 = launch_outer_reduce(e->ctx, u, lg.kp, i * r, r, dy.p, ld_dy, slots[i].col, slots[i].n_out, M, inv_gscale, gl + gslots.dB[slots[i].target], 1, r,
                                w.partial, w.partial_bytes, accumulate, s);
      if (rc2) return rc2;
    }
    return AWT_OK;
  };
  // slot order inside a group follows the order the forward packs A rows / B columns: the enabled targets of the group, in order
  const Slot qkv_slots[3] = {{AWT_LORA_Q, T_Q, 0, d}, {AWT_LORA_K, T_K, d, d}, {AWT_LORA_V, T_V, 2 * d, d}};
  const Slot out_slot[1] = {{AWT_LORA_OUT, T_OUT, 0, d}}, fc1_slot[1] = {{AWT_LORA_FC1, T_FC1, 0, f}}, fc2_slot[1] = {{AWT_LORA_FC2, T_FC2, 0, d}};

  // final LayerNorm
  float* dx = w.dx_a; float* dx_other = w.dx_b;
  // f16f8 images of d(x_out) (the fc2 backward GEMM's operand) and of d(pre) (the fc1 backward GEMM's) live in the same bytes as their bf16 hi / lo planes
  const Act dxp8 = make_act(w.dxp, (size_t)M * d, PREC_F16F8), dpre8 = make_act(w.dpre, (size_t)M * f, PREC_F16F8);
  // (mlp8: the two LayerNorm backwards that feed an fc2 backward GEMM write those images instead of the planes)
  rc = launch_layernorm_bwd(e->ctx, d_hidden, w.x_final, e->lnf_g, nullptr, M, d, 1e-5f, dx, mlp8 ? PlanePair{} : w.dxp, s, gscale, mlp8 ? &dxp8 : nullptr); if (rc) return rc;
  for (int li = c.n_layers - 1; li >= 0; --li) {
    Layer& L = e->layers[li];
    const LayerBufs& b = w.layer[li];
    // the layer's block of the gradient buffer: adapters q, k, v, out, fc1, fc2 (enabled ones; lora_grad_slots), or train_base's entries (go); the
    // groups are visited fc2, fc1, out, qkv
    float* const gl = layer_grads + (size_t)li * per_layer;
    // ---- MLP: dpre = ([dx | du2] [W2 | lscale A2]) * gelu'(pre) ; dln = [dpre | du1] [W1 | lscale A1] ; dx_mid = dx + LN2_bwd(dln)
    rc = group_backward(L.l2, dxp, d, d, fc2_slot, 1, b.ff, f, b.u2, gl); if (rc) return rc;
    if (tb) {
      rc = dW(dxp.p, d, 0, d, b.ff, f, 0, f, M, nullptr, gl + go.f2w, f, 1); if (rc) return rc;
      rc = dBias(dxp.p, d, 0, d, M, gl + go.f2b); if (rc) return rc;
    }
    if (mlp8) {   // no fc1 / fc2 adapters in this mode (encoder_create): one K segment each
      GemmSeg s8 = seg_plain(dxp8, d, L.fc2T8, 0, d, M);
      GemmOut o{}; set_out(o, dpre8); o.ldo = f; o.n_valid = f; o.pre_hi = b.pre.hi; o.pre_lo = b.pre.lo; o.scale = 1.0f;
      rc = launch_gemm(e->ctx, M, f, &s8, 1, PREC_F16F8, EPI_BF16_DGELU, o, s); if (rc) return rc;
      s8 = seg_plain(dpre8, f, L.fc1T8, 0, f, M);
      GemmOut o2{}; o2.f32 = w.dln; o2.ldo = d; o2.n_valid = d;
      rc = launch_gemm(e->ctx, M, d, &s8, 1, PREC_F16F8, EPI_F32, o2, s); if (rc) return rc;
    } else {
      GemmOut o{}; set_out(o, dpre.a); o.pre_hi = b.pre.hi; o.pre_lo = b.pre.lo;
      rc = linear_backward_input(e, dxp.a, d, L.fc2T, L.l2, du.a, f, EPI_BF16_DGELU, o, M, gterms, s); if (rc) return rc;
      rc = group_backward(L.l1, dpre, f, f, fc1_slot, 1, b.ln2, d, b.u1, gl); if (rc) return rc;
      if (tb) {
        rc = dW(dpre.p, f, 0, f, b.ln2, d, 0, d, M, nullptr, gl + go.f1w, d, 1); if (rc) return rc;
        rc = dBias(dpre.p, f, 0, f, M, gl + go.f1b); if (rc) return rc;
      }
      GemmOut o2{}; o2.f32 = w.dln;
      rc = linear_backward_input(e, dpre.a, f, L.fc1T, L.l1, du.a, d, EPI_F32, o2, M, gterms, s); if (rc) return rc;
    }
    if (tb) { rc = dLN(w.dln, b.x_mid, inv_gscale, gl + go.ln2); if (rc) return rc; }
    rc = launch_layernorm_bwd(e->ctx, w.dln, b.x_mid, L.ln2_g, dx, M, d, 1e-5f, dx_other, w.dxp, s); if (rc) return rc;
    std::swap(dx, dx_other);   // dx = d(loss)/d(x_mid)
    // ---- attention: datt = [dx_mid | duo] [Wo | lscale Ao] ; (dq, dk, dv) = attention_bwd
    rc = group_backward(L.lo_, dxp, d, d, out_slot, 1, b.att, d, b.uo, gl); if (rc) return rc;
    if (tb) {
      rc = dW(dxp.p, d, 0, d, b.att, d, 0, d, M, nullptr, gl + go.ow, d, 1); if (rc) return rc;
      rc = dBias(dxp.p, d, 0, d, M, gl + go.ob); if (rc) return rc;
    }
    {
      GemmOut o{}; set_out(o, datt.a); o.scale = 1.0f;
      rc = linear_backward_input(e, dxp.a, d, L.outT, L.lo_, du.a, d, EPI_BF16, o, M, gterms, s); if (rc) return rc;
    }
    rc = launch_attention_bwd(e->ctx, b.qkv, b.qkv.at(plane), b.qkv.at(2 * plane), b.att, w.datt, b.lse, w.delta, w.dqkv, B, H, S, 0.125f, terms, gterms, s);
    if (rc) return rc;
    rc = group_backward(L.lq, dqkv, 3 * d, 3 * d, qkv_slots, 3, b.ln1, d, b.u, gl); if (rc) return rc;
    if (tb) {   // q | k | v weights are adjacent in the block: one [3 d, d] product; k_proj has no bias
      rc = dW(dqkv.p, 3 * d, 0, 3 * d, b.ln1, d, 0, d, M, nullptr, gl + go.qkvw, d, 1); if (rc) return rc;
      rc = dBias(dqkv.p, 3 * d, 0, d, M, gl + go.qb); if (rc) return rc;
      rc = dBias(dqkv.p, 3 * d, 2 * d, d, M, gl + go.vb); if (rc) return rc;
    }
    // ---- gradient exchange: layers [li, group_hi) are final -- average them over the ranks on the side stream while the
    //      lower layers' backward continues on `s`
    if (exchange) {
      const int G = e->comm_groups, Lr = c.n_layers;
      const int grp = (int)((int64_t)li * G / Lr);                       // layer li belongs to group grp (0 = lowest layers)
      const int lo_layer = (int)(((int64_t)grp * Lr + G - 1) / G);       // first layer of that group
      if (li == lo_layer && !(tb && li == 0)) {   // train_base: the lowest group waits for the conv stem's gradients and takes the head with it
        const int hi_layer = (int)(((int64_t)(grp + 1) * Lr + G - 1) / G);
        rc = comm_reduce_async(e->comm, layer_grads + (size_t)li * per_layer, (size_t)(hi_layer - li) * per_layer, s);
        if (rc) return rc;
      }
    }
    if (li == 0 && !tb) break;   // nothing below the first adapter needs a gradient
    // ---- dln = [dqkv | du] [Wqkv | lscale A]  ; dx_in = dx_mid + LN1_bwd(dln)
    {
      GemmOut o{}; o.f32 = w.dln;
      rc = linear_backward_input(e, dqkv.a, 3 * d, L.qkvT, L.lq, du.a, d, EPI_F32, o, M, gterms, s); if (rc) return rc;
    }
    if (tb) { rc = dLN(w.dln, b.x_in, inv_gscale, gl + go.ln1); if (rc) return rc; }
    rc = launch_layernorm_bwd(e->ctx, w.dln, b.x_in, L.ln1_g, dx, M, d, 1e-5f, dx_other, mlp8 ? PlanePair{} : w.dxp, s, 1.0f, mlp8 ? &dxp8 : nullptr);     // feeds the layer below's fc2 backward GEMM
    if (rc) return rc;
    std::swap(dx, dx_other);
  }
  if (tb) {
    // ---- conv stem.  dx = d(loss)/d(x_0) (the position table gets no gradient).  conv2: x_0 = gelu(pre2) + pos, pre2 recomputed in fp32 by the forward's own GEMM;
    //      conv1: h1 = gelu(pre1), pre1 kept by the forward.  Tap dt of conv2 reads h1 row 2 s + dt - 1 (zero outside the clip).
    const int T = 2 * S, Mt = B * T, nm = c.n_mels, k1 = conv1_k(nm);
    {
      const Act h1 = make_act(w.conv.h1, (size_t)Mt * d, terms);
      GemmSeg sg[3];
      for (int dt = 0; dt < 3; ++dt) {
        sg[dt] = seg_plain(h1, d, e->conv2.w, (int64_t)dt * d, d, M);
        sg[dt].rows_out = S; sg[dt].rows_in = T; sg[dt].row_mul = 2; sg[dt].row_add = dt - 1;
      }
      GemmOut o{}; o.f32 = w.dln; o.ldo = d; o.bias = e->conv2.bias; o.n_valid = d;
      rc = launch_gemm(e->ctx, M, d, sg, 3, terms, EPI_F32, o, s); if (rc) return rc;
    }
    rc = launch_dgelu_planes(e->ctx, dx, w.dln, (int64_t)M * d, datt.p, s); if (rc) return rc;     // d pre2
    for (int dt = 0; dt < 3; ++dt) {   // conv2.weight[n, c, dt]
      const WgradRowMap map{S, T, 2, dt - 1};
      rc = dW(datt.p, d, 0, d, w.conv.h1, d, 0, d, M, &map, lora_grads + go.c2w + dt, 3 * (int64_t)d, 3); if (rc) return rc;
    }
    rc = dBias(datt.p, d, 0, d, M, lora_grads + go.c2b); if (rc) return rc;
    // d pre1 [B T, d] viewed as [B S, 2 d]: even frames t = 2 j take tap 1 of row j; odd frames t = 2 j + 1 take tap 0 of row j + 1 and tap 2 of row j
    const Grad& dh1 = dqkv;
    {
      GemmSeg sg = seg_plain(datt.a, d, e->conv2T[1], 0, d, M);
      GemmOut o{}; set_out(o, dh1.a); o.ldo = 2 * d; o.n_valid = d; o.pre_hi = w.conv.pre1.hi; o.pre_lo = w.conv.pre1.lo;
      rc = launch_gemm(e->ctx, M, d, &sg, 1, gterms, EPI_BF16_DGELU, o, s); if (rc) return rc;
      GemmSeg so[2];
      so[0] = seg_plain(datt.a, d, e->conv2T[0], 0, d, M);
      so[0].rows_out = S; so[0].rows_in = S; so[0].row_mul = 1; so[0].row_add = 1;
      so[1] = seg_plain(datt.a, d, e->conv2T[2], 0, d, M);
      const PlanePair pre1_odd = w.conv.pre1.at(d);
      GemmOut oo{}; set_out(oo, act_offset(dh1.a, d)); oo.ldo = 2 * d; oo.n_valid = d; oo.pre_hi = pre1_odd.hi; oo.pre_lo = pre1_odd.lo;
      rc = launch_gemm(e->ctx, M, d, so, 2, gterms, EPI_BF16_DGELU, oo, s); if (rc) return rc;
    }
    for (int dt = 0; dt < 3; ++dt) {   // conv1.weight[n, c, dt]: the im2col row holds tap dt at columns dt n_mels ..
      rc = dW(dh1.p, d, 0, d, w.conv.a1, k1, dt * nm, nm, Mt, nullptr, lora_grads + go.c1w + dt, 3 * (int64_t)nm, 3); if (rc) return rc;
    }
    rc = dBias(dh1.p, d, 0, d, Mt, lora_grads + go.c1b); if (rc) return rc;
    if (exchange) {   // the lowest layer group together with the non-layer parameters in front of it
      const int G = e->comm_groups, Lr = c.n_layers;
      const int hi_layer = (int)(((int64_t)Lr + G - 1) / G);
      rc = comm_reduce_async(e->comm, lora_grads, e->g_head + (size_t)hi_layer * per_layer, s); if (rc) return rc;
    }
  }
  if (exchange) { rc = comm_join(e->comm, s); if (rc) return rc; }
  return AWT_OK;
}
